#!/usr/bin/env python3
"""Outcomes and times of the action-recognition test epoch (egx_view_ensemble_update + egx_view_ensemble_topk /
functional.view_ensemble_* / train.ViewEnsembleTest) on the GPU; writes profiles/view_ensemble_report.txt (or --out). Recorded, not gated.

Part 1: the cases of tests/test_gpu_view_ensemble.py against the gate tests/view_ensemble_ref.py - rows bit for bit, labels, view counts,
rank, pred and every count exactly ("exact" or "DIFFER"; no tolerance enters) - and the recorded reference epochs of
tests/golden/live/view_ensemble.npz through ViewEnsembleTest.step_result.
Part 2: milliseconds, device events around `iters` calls after warm-up:
    update   one functional.view_ensemble_update at B = 256 clips, classes (115, 478): 30 adjacent views per video (what the test
             loader yields), and the same clips shuffled
    compute  functional.view_ensemble_topk over n = 4096 videos
    the reference-style loop on the same 4096 x 30 clips, on this machine: torch.cat of the epoch, the Python walk with three dicts (one
    `+=` per clip and head), torch.stack, four topk_errors with .item() - on the device tensors (as the reference runs it) and on host
    tensors, host clock, one run each
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egot2_amd import functional as F_egx  # noqa: E402
from egot2_amd.train import ViewEnsembleTest  # noqa: E402
from tests import view_ensemble_ref as vr  # noqa: E402

VIEWS = [30] * 9 + [2] * 10 + [1] * 32
ERR_KEYS = ("top1_verb_err", "top5_verb_err", "top1_noun_err", "top5_noun_err")


def _epoch(dev, preds, labels, ids, classes, method, cuts, capacity=None):
    slots = vr.slots_of(ids)
    n = int(slots.max()) + 1
    capacity = capacity or n
    state = F_egx.view_ensemble_state(capacity, classes, dev)
    x, y, s = torch.from_numpy(preds).to(dev), torch.from_numpy(labels).to(dev), torch.from_numpy(slots).to(dev)
    edges = [0, *cuts, len(ids)]
    for a, b in zip(edges[:-1], edges[1:]):
        F_egx.view_ensemble_update(state, capacity, classes, list(x[a:b].split(list(classes), dim=1)), y[a:b], s[a:b], method=method)
    res = F_egx.view_ensemble_topk(state, capacity, classes, n)
    torch.cuda.synchronize(dev)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    got.update({k: v[:n].cpu().numpy() for k, v in F_egx.view_ensemble_rows(state, capacity, classes).items()})
    return got


def _exact(got, ref):
    rows = np.array_equal(got["rows"].view(np.uint32), ref["rows"].view(np.uint32))
    rest = (np.array_equal(got["labels"], ref["labels"]) and np.array_equal(got["views"], ref["views"]) and np.array_equal(got["rank"], ref["rank"])
            and np.array_equal(got["pred"], ref["pred"]) and int(got["n"]) == ref["n"] and int(got["n_dropped"]) == ref["n_dropped"]
            and int(got["n_nonfinite"]) == ref["n_nonfinite"] and got["n_invalid"].tolist() == ref["n_invalid"].tolist()
            and got["correct"].tolist() == ref["correct"].tolist())
    return rows, rest


def cases(dev, lines):
    lines.append("cases against the gate tests/view_ensemble_ref.py: the accumulator rows bit for bit; labels, view counts, rank, pred, counts exactly")
    lines.append(f"  {'case':44s} {'clips':>6s} {'videos':>7s} {'rows':>8s} {'rank / pred / counts':>22s}")
    ok = True
    runs = []
    for ci, classes in enumerate([(5, 7), (115, 478), (7, 600)]):
        preds, labels, ids = vr.make_epoch(classes, VIEWS, seed=300 + ci)
        for method in ("sum", "max"):
            for cuts in ((1, 65), (100, 200)):
                runs.append((f"classes {classes} {method} calls cut at {cuts}", preds, labels, ids, classes, method, cuts, None))
    for method in ("sum", "max"):
        preds, labels, ids = vr.planted(method)
        runs.append((f"planted (ties, invalid label, NaN, dropped) {method}", preds, labels, ids, vr.PLANTED_CLASSES, method, (5,), 7))
    for name, preds, labels, ids, classes, method, cuts, cap in runs:
        ref = vr.evaluate(preds, labels, ids, classes, method)
        rows, rest = _exact(_epoch(dev, preds, labels, ids, classes, method, cuts, cap), ref)
        ok &= rows and rest
        lines.append(f"  {name:44s} {len(ids):6d} {ref['n']:7d} {'exact' if rows else 'DIFFER':>8s} {'exact' if rest else 'DIFFER':>22s}")
    z = np.load(os.path.join(ROOT, "tests", "golden", "live", "view_ensemble.npz"))
    lines += ["", "the recorded reference epochs (the REAL test_epoch_end) through ViewEnsembleTest.step_result: top1_verb, top5_verb, top1_noun, top5_noun errors"]
    for case in ("a", "b"):
        classes = tuple(int(c) for c in z[f"{case}_classes"])
        x, y = torch.from_numpy(z[f"{case}_preds"]).to(dev), torch.from_numpy(z[f"{case}_labels"]).to(dev)
        clip_ids = [f"clip{int(v):03d}" for v in z[f"{case}_clip_ids"]]
        for method in ("sum", "max"):
            ens = ViewEnsembleTest(8, classes, method=method).reset()
            for a in range(0, len(clip_ids), 8):
                ens.update(list(x[a:a + 8].split(list(classes), dim=1)), y[a:a + 8], clip_ids=clip_ids[a:a + 8])
            r = ens.step_result(prefix="")
            got, want = [r[k] for k in ERR_KEYS], z[f"{case}_{method}_err"].tolist()
            ok &= got == want
            lines.append(f"  case {case} {method:3s}  device {got}  recorded {want}  {'equal' if got == want else 'DIFFER'}")
    return ok


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


def reference_loop(preds_verbs, preds_nouns, labels, clip_ids, classes):
    """The loop of test_epoch_end restated on torch tensors of whatever device they are on ("sum"), ending in the four .item() reads."""
    video_labels, video_verb_preds, video_noun_preds = {}, {}, {}
    for i in range(preds_verbs.shape[0]):
        vid_id = clip_ids[i]
        video_labels[vid_id] = labels[i]
        if vid_id not in video_verb_preds:
            video_verb_preds[vid_id] = torch.zeros((classes[0]), device=preds_verbs.device, dtype=preds_verbs.dtype)
            video_noun_preds[vid_id] = torch.zeros((classes[1]), device=preds_nouns.device, dtype=preds_nouns.dtype)
        video_verb_preds[vid_id] += preds_verbs[i]
        video_noun_preds[vid_id] += preds_nouns[i]
    verb = torch.stack(list(video_verb_preds.values()), dim=0)
    noun = torch.stack(list(video_noun_preds.values()), dim=0)
    lab = torch.stack(list(video_labels.values()), dim=0)
    errs = []
    for p, y in ((verb, lab[:, 0]), (noun, lab[:, 1])):
        top = torch.topk(p, 5, dim=1, largest=True, sorted=True).indices.t()
        hit = top.eq(y.view(1, -1).expand_as(top))
        errs += [((1.0 - hit[:k, :].reshape(-1).float().sum() / p.size(0)) * 100.0).item() for k in (1, 5)]
    return errs


def timings(dev, lines, videos, views, iters):
    classes, B = (115, 478), 256
    rng = np.random.RandomState(7)
    N = videos * views
    preds = (3.0 * rng.standard_normal((N, sum(classes))) + 0.25).astype(np.float32)
    video_labels = np.stack([rng.randint(0, c, size=videos) for c in classes], axis=1).astype(np.int64)
    vid = np.repeat(np.arange(videos), views)
    x, y, s = torch.from_numpy(preds).to(dev), torch.from_numpy(video_labels[vid]).to(dev), torch.from_numpy(vid).to(dev)
    heads = list(x.split(list(classes), dim=1))
    state = F_egx.view_ensemble_state(videos, classes, dev)
    batch = [h[:B] for h in heads]
    t_adj = _events(dev, lambda: F_egx.view_ensemble_update(state, videos, classes, batch, y[:B], s[:B]), iters)
    perm = torch.from_numpy(rng.permutation(B)).to(dev)
    s_mixed, y_mixed, x_mixed = s[:B][perm].contiguous(), y[:B][perm].contiguous(), list(x[:B][perm].contiguous().split(list(classes), dim=1))
    t_mix = _events(dev, lambda: F_egx.view_ensemble_update(state, videos, classes, x_mixed, y_mixed, s_mixed), iters)
    state.zero_()
    for a in range(0, N, B):
        F_egx.view_ensemble_update(state, videos, classes, [h[a:a + B] for h in heads], y[a:a + B], s[a:a + B])
    out = {"flat": torch.zeros(3 + 2 + 4, dtype=torch.int32, device=dev), "rank": torch.zeros((videos, 2), dtype=torch.int32, device=dev),
           "pred": torch.zeros((videos, 2), dtype=torch.int32, device=dev)}
    t_topk = _events(dev, lambda: F_egx.view_ensemble_topk(state, videos, classes, videos, out=out), iters)
    res = F_egx.view_ensemble_topk(state, videos, classes, videos, out=out)
    torch.cuda.synchronize(dev)
    n = np.float32(videos)
    ours = [float((np.float32(1.0) - np.float32(int(res["correct"][k, h])) / n) * np.float32(100.0)) for h in (0, 1) for k in (0, 1)]
    clip_ids = [f"clip{v:05d}" for v in vid]
    loops = []
    for where, tensors in (("device tensors", (heads[0], heads[1], y)), ("host tensors", (heads[0].cpu(), heads[1].cpu(), y.cpu()))):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        errs = reference_loop(*tensors, clip_ids, classes)
        torch.cuda.synchronize(dev)
        loops.append((where, (time.perf_counter() - t0) * 1e3, errs))
    lines += ["", f"times, milliseconds (recorded, not asserted): device events around {iters} calls; classes {classes}, {views} views per video",
              f"  update, B = {B} clips, {views} adjacent views per video ({-(-B // views)} videos) {t_adj:10.4f}",
              f"  update, B = {B} clips, the same clips shuffled                       {t_mix:10.4f}",
              f"  compute (top-k launch) over n = {videos} videos                       {t_topk:10.4f}",
              f"  whole epoch here: {-(-N // B)} updates + compute, by the figures above      {-(-N // B) * t_adj + t_topk:10.2f}"]
    for where, ms, errs in loops:
        lines.append(f"  reference-style loop over the same {N} clips, {where:15s} {ms:12.1f}   errors {errs}")
    lines.append(f"  errors of the device epoch {ours}" + ("  (equal to the loops': tie-free data)" if all(ours == e for _, _, e in loops) else ""))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_ensemble_report.txt"))
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--videos", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=500)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("view_ensemble_eval: no GPU visible; nothing was measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lines = [f"action-recognition test epoch report ({torch.cuda.get_device_name(dev)}, torch {torch.__version__})", ""]
    ok = cases(dev, lines)
    if not args.skip_timing:
        timings(dev, lines, args.videos, 30, args.iters)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
