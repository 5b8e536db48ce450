#!/usr/bin/env python3
"""Slacks and times of the LTA validation step (egx_lta_validate / functional.lta_validate / train.LTAValidation) on the GPU; writes
profiles/lta_validation_report.txt (or --out).

Part 1: for every case of tests/lta_val_ref.py, and for one recipe-size batch (B = 256, Z = 20, classes (115, 478), K = 5: 51 200 draws, of
which some land next to a bin edge), the worst slack of check_draws: the largest amount by which a draw's uniform lies outside its bin of the
fp64 cdf (0: every draw strictly inside). The one tolerance is TOL = 1e-5; a slack above TOL / 2 means the accumulation order needs fixing.
Edit distances must equal the reference's recurrence exactly.
Part 2, for information only (no ratio is a pass condition): one validation call at the recipe size against what it replaces, on the same
logits in the same process:
    new                 LTAValidation(k=5)(preds, labels)                         one launch + the seed step, nothing synchronises
    new + step_result   ... + step_result(): one device-to-host copy
    torch generate      the models' torch path: Categorical(logits).sample() K times per head + torch.stack
    reference step      torch generate + permute + .cpu() per head + the host `aued` of tests/lta_val_ref.py (the loop of lta_metrics.py:86-114
                        over a pure-Python Levenshtein; the reference's editdistance package is C, so its loop is faster than this one)
Needs a GPU: there is no fall-back.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egot2_amd import functional as F_egx  # noqa: E402
from egot2_amd.train import LTAValidation  # noqa: E402
from tests import lta_val_ref as vr  # noqa: E402

SEED = 0x5EED0123456789AB


def slacks(dev, lines, B, Z):
    lines.append(f"worst slack of every draw against the fp64 cdf (tests/lta_val_ref.py check_draws; tol {vr.TOL:.0e}, fix the accumulation above "
                 f"{vr.TOL / 2:.0e}); edit distances against the reference's recurrence")
    ok = True
    for i, case in enumerate(vr.CASES):
        Bc, Zc, classes, K, _, _ = case
        stack, labels = vr.val_inputs(i)
        heads = vr.heads_of(stack, case)
        tokens, stats = F_egx.lta_validate(vr.heads_of(stack.to(dev), case), labels.to(dev), k=K, seed=SEED)
        tokens = [t.cpu() for t in tokens]
        u = vr.uniforms(SEED, Bc, Zc, len(classes), K)
        if K == 1:
            good, worst = all(torch.equal(t, vr.argmax_lowest(x)) for t, x in zip(tokens, heads)), 0.0
        else:
            res = [vr.check_draws(t, x, u[h]) for h, (t, x) in enumerate(zip(tokens, heads))]
            good, worst = all(r[0] for r in res), max(r[1] for r in res)
        md = vr.min_dist(tokens, labels)
        exact = torch.equal(stats["min_dist"].cpu(), md) and torch.equal(stats["dist_sum"].cpu(), md.sum(dim=0, dtype=torch.int64))
        ok &= good and exact and worst <= vr.TOL / 2
        lines.append(f"  {vr.case_id(case):28s} {'argmax' if K == 1 else f'{Bc * Zc * K * len(classes):6d} draws'}  worst slack {worst:.2e}  "
                     f"distances {'exact' if exact else 'DIFFER'}  {'ok' if good and exact else 'MISS'}")
    classes = (115, 478)
    g = torch.Generator().manual_seed(1234)
    stack = 3 * torch.randn(B, Z, sum(classes), generator=g)
    heads = list(torch.split(stack, list(classes), dim=-1))
    tokens, _ = F_egx.lta_validate(list(torch.split(stack.to(dev), list(classes), dim=-1)), None, k=5, seed=SEED)
    u = vr.uniforms(SEED, B, Z, 2, 5)
    res = [vr.check_draws(t.cpu(), x, u[h]) for h, (t, x) in enumerate(zip(tokens, heads))]
    worst = max(r[1] for r in res)
    ok &= all(r[0] for r in res) and worst <= vr.TOL / 2
    lines.append(f"  recipe size B{B}_Z{Z}_C115x478_K5   {B * Z * 5 * 2:6d} draws  worst slack {worst:.2e}  ({worst / vr.TOL:.3f} of tol)")
    lines.append(f"  every draw within tol, every slack below tol / 2, every distance exact: {ok}")
    return ok


def timings(dev, lines, B, Z, iters, rounds):
    from torch.distributions.categorical import Categorical
    classes, K = (115, 478), 5
    g = torch.Generator().manual_seed(1234)
    stack = (3 * torch.randn(B, Z, sum(classes), generator=g)).to(dev)
    labels = torch.stack([torch.randint(0, c, (B, Z), generator=g) for c in classes], dim=-1).to(dev)
    preds = list(torch.split(stack, list(classes), dim=-1))
    val = LTAValidation(k=K)

    def new():
        return val(preds, labels)

    def new_with_result():
        val(preds, labels)
        return val.step_result()

    def torch_generate():
        out = []
        for head_x in preds:
            dist = Categorical(logits=head_x)
            out.append(torch.stack([dist.sample() for _ in range(K)], dim=1))
        return out

    def reference_step():
        step_result = {}
        for h, pred in enumerate(torch_generate()):
            pred, lab = pred.permute(0, 2, 1).cpu(), labels.cpu()
            for k, v in vr.aued(pred.numpy(), lab[:, :, h:h + 1].numpy()).items():
                step_result[f"val_{h}_{k}"] = v
        return step_result

    fns = {"new": (new, iters), "new + step_result": (new_with_result, iters), "torch generate": (torch_generate, max(iters // 4, 5)),
           "reference step": (reference_step, 1)}
    for name, (fn, n) in fns.items():
        for _ in range(0 if name == "reference step" else 3):           # warm-up (the host loop needs none)
            fn()
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        new()
    torch.cuda.synchronize(dev)
    times = {k: [] for k in list(fns) + ["new (graph replay)"]}
    for r in range(rounds):
        for name, (fn, n) in fns.items():
            if name == "reference step" and r > 0:
                continue                                                # seconds per call: once
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize(dev)
            times[name].append((time.perf_counter() - t0) / n * 1e6)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(iters):
            graph.replay()
        torch.cuda.synchronize(dev)
        times["new (graph replay)"].append((time.perf_counter() - t0) / iters * 1e6)
    lines.append(f"one validation call at B = {B}, Z = {Z}, classes {classes}, K = {K} ({B * Z * sum(classes) * 4 / 1e6:.1f} MB of logits), for "
                 f"information: microseconds per call, host clock around calls ending in a device synchronise, {rounds} interleaved rounds")
    for name, v in times.items():
        lines.append(f"  {name:20s} median {statistics.median(v):12.1f}   min {min(v):12.1f}   ({len(v)} rounds)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lta_validation_report.txt"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--future", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("lta_validation_eval: no GPU visible; nothing was measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lines = [f"LTA validation report ({torch.cuda.get_device_name(dev)}, torch {torch.__version__})", ""]
    ok = slacks(dev, lines, args.batch, args.future)
    if not args.skip_timing:
        lines.append("")
        timings(dev, lines, args.batch, args.future, args.iters, args.rounds)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
