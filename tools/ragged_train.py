"""Training throughput of ragged batches (forward_features_ragged: egx_ragged_train_fwd / egx_ragged_bwd) on a TTM-like training set: N seeded
3-task clips of T ~ U[15, 150] frames per task, L = 1, train mode (p = 0.1, 0.1 positional), forward + weighted CE + backward + FusedAdam
per batch. Paths:
  (a) "reference"   the reference recipe: clips sorted by length, longest first, batches of max(400 // T, 1) clips
                    (HHI/dataset/ttm/sampler.py:14-60, --batch_size 400), every clip truncated to the shortest of its batch per task
                    (HHI/utils/ttm/utils.py:232-241), on the existing uniform path;
  (b) "sorted"      the same batches untruncated, ragged;
  (c) "shuffled"    shuffled batches of --batches clips, ragged;
  (d) "uniform"     the uniform tiled step of ONE batch with as many tokens as the average (c) batch of the largest size (equal clips of
                    T = tokens / (3 B) frames per task): the cost yardstick of a (c) step.
Each path is timed with device events over the whole set after a warm-up pass; one JSON line per path with clips/s and trained frames/s
(frames that reach the loss: (a) counts the truncated frames only). The "parity" line holds max |d logit| and the largest relative gradient
difference between a (c) batch and the per-length-group fallback (functional._encoder_grouped) at p = 0.
usage: python tools/ragged_train.py [--clips 1024] [--batches 64,256] [--compute f32s] [--out profiles/ragged_train_<tag>.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1024)
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--compute", default="f32s")
    ap.add_argument("--frames", type=int, default=400, help="frame budget of a reference batch")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from bench import csrc_sha
    from egot2_amd import functional as F_egx, hhi_ttm
    from egot2_amd.train import FusedAdam
    from tests.util import hhi_args, seeded_state_dict

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2025)
    T = rng.integers(15, 151, size=(a.clips, 3))
    target = torch.from_numpy(rng.integers(0, 2, a.clips)).long().to(dev)
    cw = torch.tensor([0.266, 0.734], device=dev)
    g = torch.Generator().manual_seed(7)
    clips = [[torch.randn(int(t), 256, generator=g) for t in row] for row in T]
    sizes = [int(x) for x in a.batches.split(",")]

    def padded(idx, T_pad):
        out = []
        for k in range(3):
            t = torch.zeros(len(idx), T_pad[k], 256)
            for j, i in enumerate(idx):
                n = min(clips[i][k].shape[0], T_pad[k])
                t[j, :n] = clips[i][k][:n]
            out.append(t.to(dev))
        return out

    # (a) / (b): the reference sampler's batches
    order = sorted(range(a.clips), key=lambda i: -int(T[i].max()))
    ref_batches, s = [], 0
    while s < a.clips:
        e = min(a.clips, s + max(a.frames // int(T[order[s]].max()), 1))
        ref_batches.append(order[s:e])
        s = e
    bat = {"reference": [], "sorted": []}
    frames = {"reference": 0, "sorted": int(T.sum())}
    for idx in ref_batches:
        tmin = [int(T[idx, k].min()) for k in range(3)]
        bat["reference"].append((idx, padded(idx, tmin), None))
        frames["reference"] += len(idx) * sum(tmin)
        bat["sorted"].append((idx, padded(idx, [int(T[idx, k].max()) for k in range(3)]), torch.from_numpy(T[idx])))
    perm = np.random.default_rng(3).permutation(a.clips)
    for bs in sizes:
        key = f"shuffled_{bs}"
        bat[key] = []
        for s in range(0, a.clips, bs):
            idx = [int(i) for i in perm[s:s + bs]]
            bat[key].append((idx, padded(idx, [int(T[idx, k].max()) for k in range(3)]), torch.from_numpy(T[idx])))
        frames[key] = int(T.sum())

    def make(p):
        model = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(num_layers=1, dropout=p))
        model.load_state_dict(seeded_state_dict(model, seed=11))
        model = model.to(dev).set_compute(a.compute).train()
        model.pos_embed.dropout.p = p
        return model

    def step(model, opt, feats, idx, lengths):
        if lengths is None:
            _, loss = model.forward_features(*feats, target=target[idx], class_weight=cw)
        else:
            _, loss = model.forward_features_ragged(*feats, lengths=lengths, target=target[idx], class_weight=cw)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    def timed(fn):
        fn()            # warm-up pass (workspaces, LDS attributes, the optimizer's flat buffers)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 1e3

    base = {"tool": "ragged_train", "csrc_sha": csrc_sha(), "compute": a.compute, "clips": a.clips, "L": 1, "p": 0.1,
            "T": "U[15,150] per task", "device": torch.cuda.get_device_name(0)}
    lines = []
    for path, bl in bat.items():
        model = make(0.1)
        if path == "reference":
            model.enable_weight_cache()
        opt = FusedAdam(model.parameters(), lr=1e-4)
        t = timed(lambda: [step(model, opt, f, idx, ln) for idx, f, ln in bl])
        if path != "reference":
            assert F_egx.last_encoder_impl() == "ragged", F_egx.last_encoder_impl()
        lines.append(dict(base, path=path, batches=len(bl), mean_batch=round(a.clips / len(bl), 1), seconds=round(t, 5),
                          ms_per_step=round(1e3 * t / len(bl), 4), clips_per_s=round(a.clips / t, 1),
                          frames_trained=frames[path], frames_per_s=round(frames[path] / t, 1)))
    ref_fps = lines[0]["frames_per_s"]
    for ln in lines[1:]:
        ln["frames_per_s_vs_reference"] = round(ln["frames_per_s"] / ref_fps, 2)
    # (d) one uniform tiled step of the average (c) batch's token count
    bs = max(sizes)
    key = f"shuffled_{bs}"
    nb = len(bat[key])
    tu = max(16, int(round(int(T.sum()) / nb / (3 * bs))))
    model = make(0.1)
    opt = FusedAdam(model.parameters(), lr=1e-4)
    g2 = torch.Generator().manual_seed(9)
    uf = [torch.randn(bs, tu, 256, generator=g2).to(dev) for _ in range(3)]
    uidx = list(range(bs))
    reps = 20
    t_u = timed(lambda: [step(model, opt, uf, uidx, None) for _ in range(reps)]) / reps
    impl = F_egx.last_encoder_impl()
    c_line = next(ln for ln in lines if ln["path"] == key)
    lines.append(dict(base, path="uniform", batch=bs, T=tu, tokens=3 * bs * tu, impl=impl, ms_per_step=round(1e3 * t_u, 4),
                      ragged_step_over_uniform=round(c_line["ms_per_step"] / (1e3 * t_u), 3)))
    # parity of a (c) batch against the per-length-group fallback at p = 0 (same weights, no dropout)
    idx, feats, ln = bat[f"shuffled_{min(sizes)}"][0]
    res = []
    for grouped in (False, True):
        model = make(0.0)
        orig = F_egx._ragged_train_refused
        if grouped:     # (encoder_ragged_train then takes functional._encoder_grouped, as it does where the ragged kernels refuse)
            F_egx._ragged_train_refused = lambda *args: True
        try:
            logits, loss = model.forward_features_ragged(*feats, lengths=ln, target=target[idx], class_weight=cw)
            loss.backward()
            impl = F_egx.last_encoder_impl()
        finally:
            F_egx._ragged_train_refused = orig
        torch.cuda.synchronize()
        res.append((impl, logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    (i0, l0, g0), (i1, l1, g1) = res
    gerr = max(((g0[n] - g1[n]).norm() / (g1[n].norm() + 1e-30)).item() for n in g0)
    lines.append(dict(base, path="parity", batch=len(idx), impls=[i0, i1], p=0.0, max_abs_dlogit=(l0 - l1).abs().max().item(),
                      max_rel_grad_diff=gerr))
    for ln_ in lines:
        print(json.dumps(ln_), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
