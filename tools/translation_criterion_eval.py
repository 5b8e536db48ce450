#!/usr/bin/env python3
"""Errors and times of the EgoT2-g multi-task criterion (egx_sequence_ce / functional.sequence_cross_entropy / train.TranslationCriterion)
on the GPU; writes profiles/translation_criterion_report.txt (or --out).

Part 1: worst error per case of tests/seq_ce_ref.py against its bars (loss, loss_terms, d_logits by rel_err; counts and pred must match
exactly).
Part 2: forward + d loss / d logits of the criterion at the shape of the HOI step (six tasks, B = 256 - 512 for oscc -, sy = 2, 2, 2, 2, 21,
21, V = 620) and of the HHI step (three tasks, V = 7, sy = 2, B = 256, 256 and 3840 rows for asd), on (B, V, sy) views of (sy, B, V)
tensors of 3 * randn - the decoder's output - against what it replaces on the same data in the same process: one
torch.nn.functional.cross_entropy per task on the permuted logits, the ratio sum, and its backward down to the (sy, B, V) tensors.
Both sides hand the gradients to torch.autograd.grad (no accumulation into a leaf: in a training step the decoder's backward takes
them as they come). Time: device events around `iters` consecutive calls, the two variants alternating inside every round; median and
minimum over the rounds. The launch count of the torch side is the number of device kernels a profiler sees in one call; the
library's is egx_launch_count. Needs a GPU: there is no fall-back.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egot2_amd import _lib, functional as F_egx  # noqa: E402
from tests import seq_ce_ref as sr  # noqa: E402

SHAPES = {"hoi": (620, (256, 512, 256, 256, 256, 256), (2, 2, 2, 2, 21, 21), (1.0, 1.0, 1.0, 1.0, 0.5, 0.5)),
          "hhi": (7, (256, 256, 3840), (2, 2, 2), (1.0, 1.0, 0.5))}


def errors(dev, lines):
    lines.append(f"errors against the fp64 gate (tests/seq_ce_ref.py); bars = {sr.FACTOR:g} x the fp32 reference's own error: "
                 + ", ".join(f"{k} {sr.BAR[k]:.2e}" for k in sr.KINDS))
    ok = True
    for i, name in enumerate(sr.CASE_IDS):
        tasks = sr.seq_inputs(i)
        ref = sr.evaluate(i, sr.F64)
        outs = [k["logits"].permute(1, 0, 2).contiguous().to(dev).requires_grad_(k["grad"]) for k in tasks]
        loss, stats = F_egx.sequence_cross_entropy([o.permute(1, 2, 0) for o in outs], [k["target"].to(dev) for k in tasks],
                                                   [k["ratio"] for k in tasks],
                                                   [None if k["word_label"] is None else k["word_label"].to(dev) for k in tasks],
                                                   [None if k["labels"] is None else k["labels"].to(dev) for k in tasks], want_pred=True)
        with_grad = [t for t, k in enumerate(tasks) if k["grad"]]
        if with_grad:
            loss.backward(F_egx.unit_grad(dev))
        got = {"loss": loss.detach().cpu(), "loss_terms": stats["loss_terms"].cpu(), "pred": [None if p is None else p.cpu() for p in stats["pred"]],
               "d_logits": [o.grad.cpu().permute(1, 0, 2) if o.grad is not None else ref["d_logits"][t] for t, o in enumerate(outs)]}
        got.update({c: stats[c].cpu() for c in sr.COUNTS})
        errs = sr.bar_errors(got, ref, with_grad)
        counts = sr.same_counts(got, ref)
        good = counts and all(errs[k] <= sr.BAR[k] for k in sr.KINDS)
        ok &= good
        lines.append(f"  {name:14s} " + "  ".join(f"{k} {errs[k]:.2e} ({errs[k] / sr.BAR[k]:.3f} of bar)" for k in sr.KINDS)
                     + f"  counts {'exact' if counts else 'DIFFER'}  {'ok' if good else 'MISS'}")
    lines.append(f"  every case within its bars and every count exact: {ok}")
    return ok


def kernels_in(fn):
    """Device kernels of one call of `fn`, as a profiler sees them (None where it is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    except Exception as e:       # noqa: BLE001  (a report without this number is still a report)
        print(f"profiler unavailable: {e}", file=sys.stderr)
        return None


def timings(dev, lines, name, iters, rounds):
    V, Bs, sys_, ratios = SHAPES[name]
    g = torch.Generator().manual_seed(4321)
    outs = [(3 * torch.randn(sy, B, V, generator=g)).to(dev).requires_grad_(True) for B, sy in zip(Bs, sys_)]
    targets = [torch.randint(0, V, (B, sy + 1), generator=g).to(dev)[:, 1:] for B, sy in zip(Bs, sys_)]
    logits = [o.permute(1, 2, 0) for o in outs]
    lib = _lib.load()

    def ours():
        loss, _ = F_egx.sequence_cross_entropy(logits, targets, ratios)
        return torch.autograd.grad(loss, outs, F_egx.unit_grad(dev))

    def stock():
        loss = sum(r * torch.nn.functional.cross_entropy(lg, t) for r, lg, t in zip(ratios, logits, targets))
        return torch.autograd.grad(loss, outs)

    a, b = ours(), stock()
    worst = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(a, b))
    lib.egx_launch_count(1)
    ours()
    n_ours = lib.egx_launch_count(0)
    n_stock = kernels_in(stock)
    times = {"one launch": [], "torch": []}
    for _ in range(rounds):
        for label, fn in (("one launch", ours), ("torch", stock)):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[label].append(e0.elapsed_time(e1) * 1e3 / iters)
    rows = sum(B * sy for B, sy in zip(Bs, sys_))
    lines.append(f"{name} step: {len(Bs)} tasks, V = {V}, B = {Bs}, sy = {sys_} ({rows} rows); forward + d_logits, us per call, "
                 f"{rounds} rounds of {iters} calls (device events, variants interleaved); gradients agree to {worst:.1e}")
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append(f"  one launch (functional.sequence_cross_entropy)    median {med['one launch']:9.1f}  min {min(times['one launch']):9.1f}   "
                 f"library launches per call: {n_ours}")
    lines.append(f"  torch ({len(Bs)} x F.cross_entropy forward + backward)    median {med['torch']:9.1f}  min {min(times['torch']):9.1f}   "
                 f"device kernels per call: {n_stock if n_stock is not None else 'not counted (no profiler)'}")
    ratio = med["torch"] / med["one launch"]
    lines.append(f"  torch / one launch = {ratio:.2f}x: the launch is " + ("not slower than what it replaces" if ratio >= 1.0 else
                                                                         "SLOWER than what it replaces"))
    return ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "translation_criterion_report.txt"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("translation_criterion_eval needs a GPU")
    dev = torch.device("cuda:0")
    lines = [f"EgoT2-g multi-task criterion on {torch.cuda.get_device_name(0)} (tools/translation_criterion_eval.py)", ""]
    ok = errors(dev, lines)
    lines.append("")
    for name in SHAPES:
        timings(dev, lines, name, args.iters, args.rounds)
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
