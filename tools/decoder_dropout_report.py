"""Error of the EgoT2-g decoder's train-mode dropout against the fp64 oracle under the same masks, case by case (development report, GPU
box): every case of tests/decoder_dropout_gate.py. Per case: the path that ran, the logits error (max |d| / max(1, |ref|max)), the relative
norm errors of d(memory) and of the worst parameter gradient, each next to its bar, the worst quantity as a multiple of its bar (< 1 passes)
and whether a second run with the same seed had the same bits.
usage: python tools/decoder_dropout_report.py [case id ...] [--out FILE]      (profiles/decoder_dropout_parity_report.txt)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tests import decoder_dropout_gate as G  # noqa: E402
from tests.test_gpu_decoder_dropout import report_line  # noqa: E402


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    cases = [c for c in G.CASES if not argv or c.id in argv]
    dev = torch.device("cuda:0")
    lines = ["EgoT2-g decoder, train mode (p_drop = 0.3, p_pos = 0.1 unless the case says otherwise) against the fp64 oracle under the same masks:",
             "measured / bar per quantity; x bar = the worst quantity as a multiple of its bar (tests/decoder_dropout_gate.py)"]
    print("\n".join(lines), flush=True)
    for c in cases:
        t0 = time.time()
        data = G.case_data(c)
        res = G.gpu_run(c, data, dev)
        r = G.gate(res, G.oracle_run(c, data), c.bars, G.clip_rows(c))
        line = report_line(c, res, r) + ("" if r["ok"] else "  OVER") + f"  ({time.time() - t0:.1f} s)"
        lines.append(line)
        print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
