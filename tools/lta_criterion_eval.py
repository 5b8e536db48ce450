#!/usr/bin/env python3
"""Errors and times of the LTA criterion (egx_segmented_ce / functional.segmented_cross_entropy / train.LTACriterion) on the GPU; writes
profiles/lta_criterion_report.txt (or --out).

Part 1: worst error per case of tests/seg_ce_ref.py against its bars (loss, loss_terms, d_logits by rel_err; counts must match exactly).
Part 2: forward + backward of the criterion on one (B, Z, 593) = (256, 20, 115 + 478) stack of 3 * randn logits, against two baselines on
the same data in the same process:
    (a) the two-call form of synth.py's c4 workload: F.cross_entropy(verbs.reshape(-1, 115), tv) + F.cross_entropy(nouns.reshape(-1, 478), tn)
    (b) the reference's loop, HOI/tasks/lta/long_term_anticipation.py:182-203: 40 cross-entropies, 40 topk calls, 80 .item() reads
(a) and (b) do not compute the same thing as each other: (a) has no per-(z, h) means and no top-k errors. "new + step_result" adds the one
device-to-host copy that stands for (b)'s 80 reads. Eager: host clock around N calls ending in a device synchronise (what a training loop
without a captured step pays per call); graph: the same work captured once and replayed ((b) synchronises and cannot be captured).
Variants alternate inside each round; median and minimum over the rounds are reported. Needs a GPU: there is no fall-back.
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
from egot2_amd.train import LTACriterion  # noqa: E402
from tests import seg_ce_ref as sr  # noqa: E402

KINDS = ("loss", "loss_terms", "d_logits")


def errors(dev, lines):
    lines.append(f"errors against the fp64 gate (tests/seg_ce_ref.py); bars = {sr.FACTOR:g} x the fp32 reference's own error: "
                 + ", ".join(f"{k} {sr.BAR[k]:.2e}" for k in KINDS))
    ok = True
    for i, case in enumerate(sr.CASES):
        B, Z, classes, ld, _ = case
        col0 = sr.case_col0(case)
        logits, labels, ks = sr.seg_inputs(i)
        ref = sr.segmented_ce(logits.double(), labels, classes, col0, ks)
        stack = logits.to(dev).requires_grad_(True)
        loss, stats = F_egx.segmented_cross_entropy([stack[..., c0:c0 + c] for c0, c in zip(col0, classes)], labels.to(dev), ks)
        loss.backward(F_egx.unit_grad(dev))
        got = {"loss": loss.detach().cpu(), "loss_terms": stats["loss_terms"].cpu(), "d_logits": stack.grad.cpu()}
        errs = {k: sr.rel_err(got[k], ref[k]) for k in KINDS}
        counts = torch.equal(stats["n_valid"].cpu().long(), ref["n_valid"]) and torch.equal(stats["correct"].cpu().long(), ref["correct"])
        good = counts and all(errs[k] <= sr.BAR[k] for k in KINDS)
        ok &= good
        lines.append(f"  {sr.case_id(case):34s} " + "  ".join(f"{k} {errs[k]:.2e} ({errs[k] / sr.BAR[k]:.2f} of bar)" for k in KINDS)
                     + f"  counts {'exact' if counts else 'DIFFER'}  {'ok' if good else 'MISS'}")
    lines.append(f"  every case within its bars and every count exact: {ok}")
    return ok


def timings(dev, lines, B, Z, iters, rounds):
    classes = (115, 478)
    g = torch.Generator().manual_seed(1234)
    data = (3 * torch.randn(B, Z, sum(classes), generator=g)).to(dev)
    labels = torch.stack([torch.randint(0, c, (B, Z), generator=g) for c in classes], dim=-1).to(dev)
    tv, tn = labels[..., 0].reshape(-1).contiguous(), labels[..., 1].reshape(-1).contiguous()
    unit = F_egx.unit_grad(dev)
    ce = torch.nn.functional.cross_entropy

    def variants():
        """The four step functions on a leaf and a criterion of their own (the captured ones never share a leaf with eager work)."""
        stack = data.clone().requires_grad_(True)
        crit = LTACriterion()

        def preds():
            return torch.split(stack, list(classes), dim=-1)

        def new():
            stack.grad = None
            loss = crit(preds(), labels)
            loss.backward(unit)
            return loss.detach()

        def new_with_result():
            new()
            return crit.step_result()

        def two_call():
            stack.grad = None
            verbs, nouns = preds()
            loss = ce(verbs.reshape(-1, classes[0]), tv) + ce(nouns.reshape(-1, classes[1]), tn)
            loss.backward(unit)
            return loss.detach()

        def reference_loop():
            stack.grad = None
            loss, step_result = 0, {}
            for h, p in enumerate(preds()):
                for z in range(Z):
                    y = labels[:, z, h]
                    loss = loss + ce(p[:, z], y)
                    top = torch.topk(p[:, z], 5, dim=1, largest=True, sorted=True)[1].t()
                    hit = top.eq(y.view(1, -1).expand_as(top))
                    for k in (1, 5):
                        step_result[f"train_{z}_{h}_top{k}_err"] = ((1.0 - hit[:k].reshape(-1).float().sum() / B) * 100.0).item()
            loss.backward(unit)
            return loss.detach()

        return {"new": new, "new + step_result": new_with_result, "(a) two-call CE": two_call, "(b) reference loop": reference_loop}

    # the captures first, each on a fresh leaf whose first forward / backward is the warm-up on a side stream (the pattern of train.GraphedStep)
    graphs = {}
    for name in ("new", "(a) two-call CE"):
        fn = variants()[name]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode="thread_local"):
            fn()
        torch.cuda.synchronize(dev)
        graphs[name] = (gr, fn)
    fns = variants()
    eager = {name: (fn, iters if name != "(b) reference loop" else max(iters // 10, 5)) for name, fn in fns.items()}
    for fn, n in eager.values():                                        # warm-up of every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    ref_loss = fns["(b) reference loop"]().item()
    same = abs(fns["new"]().item() - ref_loss) / abs(ref_loss)
    lines.append(f"forward + backward at B = {B}, Z = {Z}, classes {classes}: {B * Z * sum(classes) * 4 / 1e6:.1f} MB of logits read, as many of "
                 f"gradient written; new vs (b) loss: relative difference {same:.1e}")
    times = {("eager", k): [] for k in eager}
    times.update({("graph", k): [] for k in graphs})
    for _ in range(rounds):
        for name, (fn, n) in eager.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize(dev)
            times[("eager", name)].append((time.perf_counter() - t0) / n * 1e6)
        for name, (gr, _) in graphs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(iters):
                gr.replay()
            torch.cuda.synchronize(dev)
            times[("graph", name)].append((time.perf_counter() - t0) / iters * 1e6)
    lines.append(f"  microseconds per call, {rounds} interleaved rounds (eager: {iters} calls per round, (b): {eager['(b) reference loop'][1]}; graph: {iters} replays)")
    for (mode, name), v in times.items():
        lines.append(f"  {mode:5s} {name:20s} median {statistics.median(v):9.1f}   min {min(v):9.1f}")
    med = {k: statistics.median(v) for k, v in times.items()}
    lines.append(f"  new / (a): eager {med[('eager', 'new')] / med[('eager', '(a) two-call CE')]:.2f}, graph "
                 f"{med[('graph', 'new')] / med[('graph', '(a) two-call CE')]:.2f};  (new + step_result) / (b): eager "
                 f"{med[('eager', 'new + step_result')] / med[('eager', '(b) reference loop')]:.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lta_criterion_report.txt"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--future", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("lta_criterion_eval: no GPU visible; nothing was measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lines = [f"LTA criterion report ({torch.cuda.get_device_name(dev)}, torch {torch.__version__})", ""]
    ok = errors(dev, lines)
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
