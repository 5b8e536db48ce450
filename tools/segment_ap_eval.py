#!/usr/bin/env python3
"""Errors and times of the TTM / LAM validation metric (egx_segment_scores_update + egx_segment_ap / functional.segment_ap /
train.SegmentAPValidation) on the GPU; writes profiles/segment_ap_report.txt (or --out). Recorded, not gated.

Part 1: worst score error (against the fp64 gate tests/segment_ap_ref.py, bar 2e-6) and worst AP0 / AP1 / mAP difference (against the gate's
algorithm on the device's own scores and order, bar 8 N 2^-53) over the sizes and input kinds of tests/test_gpu_segment_ap.py.
Part 2: milliseconds per metric at N = 4096, 65536, 2^20, 2^24 rows (one window per row, prevalence 0.5, logit differences uniform in
[-40, 40]), device events around `iters` calls after warm-up:
    new                 functional.segment_ap on the filled accumulator: memset + score kernel + sort + AP launches, nothing synchronises
    stock torch         the same metric from stock device ops: softmax of the mean logits, a stable torch.sort per class, cumsum, cummax
                        of the fp64 precisions, the masked fp64 sum, four count sums (no host read inside the timed window)
    numpy (host)        the gate on this machine's CPU, host clock: its vectorised form at every size, the literal Python loops of
                        compute_average_precision up to 65536 rows
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egot2_amd import functional as F_egx  # noqa: E402
from tests import segment_ap_ref as sr  # noqa: E402


def _epoch(dev, logits, slots, labels, n):
    state = F_egx.segment_ap_state(n, dev)
    F_egx.segment_scores_update(state, n, torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(slots).to(dev))
    res = F_egx.segment_ap(state, n, n)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in res.items()}


def errors(dev, lines):
    lines.append(f"errors over the cases of tests/test_gpu_segment_ap.py: score against the fp64 gate (bar {sr.SCORE_TOL:g}), AP0 / AP1 / mAP "
                 "against the gate's algorithm on the device's own scores and order (bar 8 N 2^-53)")
    lines.append(f"  {'N':>8s} {'kinds':>6s} {'worst score err':>16s} {'worst AP diff':>14s} {'AP bar':>10s}  counts and orders")
    ok = True
    for n in sr.sizes():
        worst_s = worst_ap = 0.0
        exact = True
        for kind in sr.kinds_for(n):
            logits, slots, labels = sr.make_input(n, kind)
            ref = sr.evaluate(logits, slots, labels, n_rows=n, fast=n > 300)
            got = _epoch(dev, logits, slots, labels, n)
            score = got["score"].astype(np.float64)
            both = np.isnan(score) & np.isnan(ref["score"])
            worst_s = max(worst_s, float(np.abs(np.where(both, 0.0, score - ref["score"])).max()))
            o1, o0 = sr.stable_orders(got["score"])
            cm = sr.compute_confusion_matrix(got["score"], ref["label"])
            exact &= np.array_equal(got["order1"], o1) and np.array_equal(got["order0"], o0)
            exact &= all(int(got[k]) == v for k, v in cm.items()) and int(got["n_pos"]) == ref["n_pos"]
            want = (float("nan"),) * 3 if ref["n_nonfinite"] else sr.ap_on_order(ref["label"], o1, o0, fast=n > 300)
            for k, w in zip(("AP0", "AP1", "mAP"), want):
                g = float(got[k])
                if math.isnan(g) != math.isnan(w):
                    exact = False
                elif not math.isnan(g):
                    worst_ap = max(worst_ap, abs(g - w))
        ok &= exact and worst_s <= sr.SCORE_TOL and worst_ap <= sr.ap_tol(n)
        lines.append(f"  {n:8d} {len(sr.kinds_for(n)):6d} {worst_s:16.3e} {worst_ap:14.3e} {sr.ap_tol(n):10.2e}  {'exact' if exact else 'DIFFER'}")
    return ok


def torch_metric(mean_logits, label):
    """The metric from stock torch device ops -> (AP0, AP1, mAP, acc) as device tensors."""
    score = torch.softmax(mean_logits, dim=-1)[:, 1]
    n = score.numel()
    k = torch.arange(1, n + 1, device=score.device, dtype=torch.float64)
    aps = []
    for cls in (0, 1):
        _, idx = torch.sort(score, descending=cls == 1, stable=True)
        lab = label[idx] if cls == 1 else 1 - label[idx]
        tp = torch.cumsum(lab, 0).double()
        env = torch.flip(torch.cummax(torch.flip(tp / k, (0,)), 0).values, (0,))
        P = tp[-1]
        aps.append(((tp / P - (tp - 1) / P) * env * lab).sum())
    pred = score >= 0.5
    pos = label == 1
    acc = ((pred & pos).sum() + (~pred & ~pos).sum()).double() / n
    return aps[0], aps[1], (aps[0] + aps[1]) / 2, acc


def _events(dev, fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / iters


def timings(dev, lines, n, iters):
    rng = np.random.default_rng(n)
    diff = rng.uniform(-40.0, 40.0, size=n)
    logits = np.stack([np.zeros(n), diff], axis=1).astype(np.float32)
    labels = (rng.random(n) < 0.5).astype(np.int64)
    x, y = torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev)
    state = F_egx.segment_ap_state(n, dev)
    F_egx.segment_scores_update(state, n, x, y, None, 0)
    out = {"flat": torch.zeros(11, dtype=torch.int64, device=dev), "score": torch.zeros(n, device=dev),
           "order1": torch.zeros(n, dtype=torch.int32, device=dev), "order0": torch.zeros(n, dtype=torch.int32, device=dev)}
    t_new = _events(dev, lambda: F_egx.segment_ap(state, n, n, out=out), iters)
    t_torch = _events(dev, lambda: torch_metric(x, y), iters)
    res = F_egx.segment_ap(state, n, n, out=out)
    ref = torch_metric(x, y)
    torch.cuda.synchronize(dev)
    d_map = abs(float(res["mAP"]) - float(ref[2]))
    score = res["score"].cpu().numpy()
    t0 = time.perf_counter()
    host = sr.run_evaluation(score, labels, fast=True)
    t_np = (time.perf_counter() - t0) * 1e3
    t_lit = float("nan")
    if n <= 65536:
        t0 = time.perf_counter()
        sr.run_evaluation(score, labels)
        t_lit = (time.perf_counter() - t0) * 1e3
    lines.append(f"  {n:9d} {iters:6d} {t_new:12.4f} {t_torch:12.4f} {t_torch / t_new:8.2f}x {t_np:14.1f} {t_lit:14.1f}   "
                 f"mAP {float(res['mAP']):.12f}, |new - torch| {d_map:.1e}, |new - numpy| {abs(float(res['mAP']) - host['mAP']):.1e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_ap_report.txt"))
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--max-rows", type=int, default=1 << 24)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("segment_ap_eval: no GPU visible; nothing was measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lines = [f"TTM / LAM validation metric report ({torch.cuda.get_device_name(dev)}, torch {torch.__version__})", ""]
    ok = errors(dev, lines)
    if not args.skip_timing:
        lines += ["", "the metric of a filled accumulator, milliseconds per call (recorded, not asserted): device events around `iters` calls; "
                      "numpy on this machine's host, one call by the host clock",
                  f"  {'N':>9s} {'iters':>6s} {'new':>12s} {'stock torch':>12s} {'torch/new':>9s} {'numpy vector':>14s} {'numpy loops':>14s}"]
        for n, iters in ((4096, 2000), (65536, 1000), (1 << 20, 300), (1 << 24, 30)):
            if n <= args.max_rows:
                timings(dev, lines, n, iters)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
