"""The 2048-wide HOI LTA 2-task translator recipe (HOI/configs/lta/ts_lta_2task.yaml:79-82: d = 2048, 4 heads of 512, one layer, dropout 0.5,
two streams of 2 clips) on the wide bf16 path at B = 256, train mode: forward + backward step time, and with --kernel-stats the attention
launches' share of a `rocprofv3 --kernel-trace --stats` summary. Records into profiles/wide2048_report.txt.

    python tools/wide2048_eval.py                                   # step time: 10 warm-up steps, 5 windows of 40 steps between device events
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/wide2048_eval.py --steps-only 30
    python tools/wide2048_eval.py --kernel-stats DIR                # attention share from DIR/**/*kernel_stats.csv
"""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests import wide2048_ref as w  # noqa: E402

B, N, D, HEADS, L, P = 256, 2, 2048, 4, 1, 0.5


def make_step():
    cuda = torch.device("cuda")
    m, _ = w.make_model(N, D, HEADS, L, P)
    m = m.to(cuda).set_compute("bf16").train()
    feats = [f.to(cuda) for f in w.make_feats(B, N, D)]

    def step():
        m.zero_grad(set_to_none=True)
        outs = m.forward_features(*feats)
        (outs[0].sum() + outs[1].sum()).backward()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    a = ap.parse_args()
    tag = f"B = {B}, n = {N}, d = {D}, heads = {HEADS}, L = {L}, p = {P}, train mode, forward + backward"
    if a.kernel_stats:
        f = glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0])))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        att = [r for r in rows if "attn" in r["Name"]]
        lines = [f"{tag}: kernel time {tot / 1e6:.2f} ms over the profiled run; attention launches {sum(float(r['TotalDurationNs']) for r in att) / tot * 100:.2f} % of it"]
        lines += [f"    {r['Name'][:90]}: {r['Calls']} calls, {float(r['AverageNs']) / 1e3:.1f} us average, {float(r['TotalDurationNs']) / tot * 100:.2f} %" for r in att]
        lines += [f"    top: {r['Name'][:90]}: {float(r['AverageNs']) / 1e3:.1f} us average, {float(r['TotalDurationNs']) / tot * 100:.1f} %" for r in rows[:6]]
        print("\n".join(lines))
        w.record("gpu measurement: attention share (rocprofv3 --kernel-trace --stats, a run of its own)", lines)
        return
    step = make_step()
    if a.steps_only:
        for _ in range(a.steps_only):
            step()
        torch.cuda.synchronize()
        return
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(40):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 40)
    ms.sort()
    line = f"{tag}: {ms[2]:.3f} ms per step (median of 5 windows of 40 steps between device events, after 10 warm-up steps; min {ms[0]:.3f}, max {ms[-1]:.3f}), eager launches"
    print(line)
    w.record("gpu measurement: step time", [line])


if __name__ == "__main__":
    main()
