#!/usr/bin/env python3
"""Errors and times of the PNR keyframe criterion (egx_keyframe_criterion / functional.keyframe_criterion / train.KeyframeCriterion) on the
GPU; writes profiles/keyframe_criterion_report.txt (or --out).

Part 1: worst error per case of tests/keyframe_ref.py against its bars (loss, loss_rows, d_logits by bar_errors; pred, label_frame and counts
must match exactly, dist exactly at T = 16 and within 1e-12 elsewhere, dist_sum within 1e-12).
Part 2: the step after the model at T = 16 and B = 32 / 256 on 3 * randn logits, timed with device events around N calls, against the
stock-torch sequence of the reference step on the same data in the same process:
    new                 KeyframeCriterion("bce") forward + backward into the logits' gradient: one launch
    new + step_result   ... plus the one device-to-host copy of step_result()
    reference step      BCELoss(sigmoid(x.squeeze(1)), labels.float()) forward + backward, then the loops of keyframe_distance and
                        keyframe_accuracy (HOI/evaluation/pnr/metrics.py:23-80) as tests/keyframe_ref.py restates them, run on the device
                        tensors: seven host reads per clip
The times are recorded, not asserted. Needs a GPU: there is no fall-back.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egot2_amd import functional as F_egx  # noqa: E402
from egot2_amd.train import KeyframeCriterion  # noqa: E402
from tests import keyframe_ref as kr  # noqa: E402

KIND_NAME = {"bce": "bce", "ce": "cross_entropy", "metric": None}


def errors(dev, lines):
    lines.append(f"errors against the fp64 gate (tests/keyframe_ref.py); bars = {kr.FACTOR:g} x the fp32 reference's own error: "
                 + ", ".join(f"{k} {kr.BAR[k]:.2e}" for k in kr.KINDS))
    ok = True
    for i, case in enumerate(kr.CASES):
        B, T, ld, cols, V, kind, flags = case
        a = kr.kf_inputs(i)
        ref = kr.evaluate(i, kr.F64)
        d = lambda t: None if t is None else t.to(dev)  # noqa: E731
        x = a["logits"].to(dev).requires_grad_(kind != "metric")
        loss, stats = F_egx.keyframe_criterion(x if ld == V else x[:, :V], d(a["target"]), d(a["label"]), d(a["state_change"]), d(a["fps"]),
                                               {k: v.to(dev) for k, v in a["info"].items()}, kind=KIND_NAME[kind], cols=cols)
        exact = all(torch.equal(stats[k].cpu().long(), ref[k]) for k in kr.EXACT)
        dist = kr.dist_ok(stats["dist"].cpu(), ref["dist"], T) and abs(stats["dist_sum"].item() - ref["dist_sum"]) <= kr.DIST_TOL * abs(ref["dist_sum"])
        text, good = "", exact and dist
        if kind != "metric":
            loss.backward(F_egx.unit_grad(dev))
            got = {"loss": loss.detach().cpu(), "loss_rows": stats["loss_rows"].cpu(), "d_logits": x.grad.cpu()}
            errs = kr.bar_errors(got, ref, i)
            good = good and all(errs[k] <= kr.BAR[k] for k in kr.KINDS)
            text = "  ".join(f"{k} {errs[k]:.2e} ({errs[k] / kr.BAR[k]:.2f} of bar)" for k in kr.KINDS)
        ok &= good
        lines.append(f"  {kr.case_id(case):28s} {text}  pred/label/counts {'exact' if exact else 'DIFFER'}  dist {'ok' if dist else 'MISS'}"
                     f"  {'ok' if good else 'MISS'}")
    lines.append(f"  every case within its bars and every exact result equal: {ok}")
    return ok


def timings(dev, lines, B, iters):
    g = torch.Generator().manual_seed(4321 + B)
    x = (3 * torch.randn(B, 1, 16, generator=g)).to(dev).requires_grad_(True)
    labels = torch.nn.functional.one_hot(torch.randint(0, 16, (B,), generator=g), 16).to(dev)
    target = labels.float()
    sc = torch.randint(0, 2, (B, 1), generator=g).to(dev)
    start = torch.randint(0, 100000, (B,), generator=g)
    info = {"clip_start_frame": start.to(dev), "clip_end_frame": (start + torch.randint(1, 400, (B,), generator=g)).to(dev),
            "pnr_frame": (start + torch.randint(0, 400, (B,), generator=g)).to(dev)}
    fps = torch.full((B,), 30.0, dtype=torch.float64, device=dev)
    unit = F_egx.unit_grad(dev)
    crit = KeyframeCriterion("bce")
    bce = torch.nn.BCELoss(reduction="mean")

    def new():
        x.grad = None
        crit(x, target, sc, fps, info).backward(unit)

    def new_with_result():
        new()
        return crit.step_result()

    def reference_step():
        x.grad = None
        loss = bce(torch.sigmoid(x.squeeze(dim=1)), labels.float())
        loss.backward(unit)
        m = kr.keyframe_criterion(x.detach()[:, 0], labels, None, sc[:, 0], fps, info, 16, None, "metric")        # .item() reads of device tensors
        n_sc, n_correct = int(m["counts"][0]), int(m["counts"][1])
        return m["dist_sum"] / max(n_sc, 1), n_correct, n_sc

    lines.append(f"  B = {B}, T = 16: milliseconds per step, device events around {iters} calls")
    for name, fn in (("new", new), ("new + step_result", new_with_result), ("reference step", reference_step)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        lines.append(f"    {name:20s} {e0.elapsed_time(e1) / iters:10.4f}")
    got, want = new_with_result(), reference_step()
    lines.append(f"    distance {got['keyframe_loc_metric_time_dist_train']:.6f} vs {want[0]:.6f}, accuracy {got['pseudo_acc']:.4f} vs "
                 f"{want[1] / max(want[2], 1):.4f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_criterion_report.txt"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("keyframe_criterion_eval: no GPU visible; nothing was measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lines = [f"PNR keyframe criterion report ({torch.cuda.get_device_name(dev)}, torch {torch.__version__})", ""]
    ok = errors(dev, lines)
    if not args.skip_timing:
        lines += ["", "the step after the model: one launch against the stock-torch sequence of the reference step (recorded, not asserted)"]
        for B in (32, 256):
            timings(dev, lines, B, args.iters)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
