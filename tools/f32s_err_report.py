"""Error of the f32 / f32s encoder paths against the fp64 oracle, case by case (development report, GPU box): every case of the fp32-grade
table (tests/fp32_grade.py: kink-free weights, the implementation's own dropout masks) and its bf16 negative controls. Per case: the path
that ran, the worst output error (max |d| / max(1, |ref|)), the loss error, the worst relative gradient error and the worst quantity as a
multiple of its fp32-grade bound (<= 1 passes; a control must reach >= 10).
usage: python tools/f32s_err_report.py [case id ...] [--out FILE]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from egot2_amd import functional as F_egx  # noqa: E402
from tests import fp32_grade as G  # noqa: E402


def main(argv):
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    F_egx.reload_tuning_each_call = True          # the cases pin EGX_FFN_CUT / EGX_FFN_SLICES per run
    cases = G.CASES + G.CONTROLS
    if argv:
        cases = [c for c in cases if c.id in argv]
    dev = torch.device("cuda:0")
    lines = [f"{'case':18s} {'ran':12s} {'margin':>8s} {'out err':>8s} {'loss err':>8s} {'grad err':>8s} {'x bound':>8s}  worst"]
    print(lines[0], flush=True)
    for c in cases:
        t0 = time.time()
        sd, marg, data = G.prepare(c)
        res = G.gpu_run(c, sd, data, dev)
        ref = G.oracle_run(c, sd, data)
        m = G.measure(c, res, ref)
        ran = res["impl"] + (f"/{res['slices']}" if res.get("slices", 1) > 1 else "")
        if c.family == "ragged_train" and not res["pad_grad_zero"]:
            ran += " PAD!"
        line = (f"{c.id:18s} {ran:12s} {min(v[0] for v in marg.values()):8.1e} {m['out_err']:8.1e} {m.get('loss_err', 0.0):8.1e} "
                f"{m['grad_err']:8.1e} {m['worst'][1]:8.3f}  {m['worst'][0]}" + (f"  OVER {m['bad']}" if m["bad"] and c.compute != "bf16" else "")
                + f"  ({time.time() - t0:.1f} s)")
        lines.append(line)
        print(line, flush=True)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
