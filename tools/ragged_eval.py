"""Evaluation throughput of ragged batches (functional.encoder_ragged, egx_ragged_fwd) on a validation-like set: N seeded 3-task TTM clips of
T ~ U[15, 150] frames per task (HHI/dataset/ttm/data_loader_2task.py:119,150-162), L = 1, eval() + no_grad, weight cache on. Per compute mode:
  (a) "per_clip"   the reference's batch_size=1 loop: one forward_features per clip (HHI/tasks/ttm/video_task_2loader.py:84-97);
  (b) "ragged"     forward_features(..., lengths=) over batches of --batches clips (features padded, clips at their own lengths);
  (c) "padded"     the existing uniform forward on the same batches with every clip padded to its batch's longest: numerically WRONG
                   (padding attends and is pooled), an upper bound of the cost of the batch.
Each timed with device events over the whole set after a warm-up pass; one JSON line per (compute, path, batch) with clips/s, and for (b) the
max |logit (a) - logit (b)|. Inputs are resident on the device before timing.
usage: python tools/ragged_eval.py [--clips 1024] [--batches 64,256] [--computes f32s,bf16] [--out profiles/ragged_eval_<tag>.json]"""
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
    ap.add_argument("--computes", default="f32s,bf16")
    ap.add_argument("--reps", type=int, default=3, help="timed passes over the set per path (the median is reported)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from bench import csrc_sha
    from egot2_amd import functional as F_egx, hhi_ttm
    from tests.util import hhi_args, seeded_state_dict

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2024)
    T = rng.integers(15, 151, size=(a.clips, 3))
    g = torch.Generator().manual_seed(7)
    clips = [[torch.randn(1, int(t), 256, generator=g).to(dev) for t in row] for row in T]
    batch_sizes = [int(x) for x in a.batches.split(",")]

    def padded(idx, T_pad):
        return [torch.cat([torch.nn.functional.pad(clips[i][k], (0, 0, 0, T_pad[k] - clips[i][k].shape[1])) for i in idx]) for k in range(3)]

    batches = {}
    for bs in batch_sizes:
        bl = []
        for s in range(0, a.clips, bs):
            idx = list(range(s, min(s + bs, a.clips)))
            T_own = [int(T[idx, k].max()) for k in range(3)]
            Tm = max(T_own)
            bl.append((idx, padded(idx, T_own), torch.from_numpy(T[idx]), padded(idx, [Tm] * 3)))
        batches[bs] = bl

    def timed(fn):
        fn()        # warm-up pass (workspaces, the weight cache, the LDS attributes)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 1e3)
        return sorted(ts)[len(ts) // 2], out

    lines = []
    for compute in a.computes.split(","):
        model = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(num_layers=1))
        model.load_state_dict(seeded_state_dict(model, seed=11))
        model = model.to(dev).set_compute(compute).eval().enable_weight_cache(frozen=True)
        base = {"tool": "ragged_eval", "csrc_sha": csrc_sha(), "compute": compute, "clips": a.clips, "L": 1,
                "T": "U[15,150] per task", "device": torch.cuda.get_device_name(0)}
        with torch.no_grad():
            t_a, ref = timed(lambda: torch.cat([model.forward_features(*c) for c in clips]))
            lines.append(dict(base, path="per_clip", batch=1, seconds=round(t_a, 5), clips_per_s=round(a.clips / t_a, 1)))
            for bs in batch_sizes:
                bl = batches[bs]
                t_b, out = timed(lambda: torch.cat([model.forward_features(*f, lengths=ln) for _, f, ln, _ in bl]))
                assert F_egx.last_encoder_impl() == "ragged", F_egx.last_encoder_impl()
                dl = (out - ref).abs().max().item()
                lines.append(dict(base, path="ragged", batch=bs, seconds=round(t_b, 5), clips_per_s=round(a.clips / t_b, 1),
                                  speedup_vs_per_clip=round(t_a / t_b, 2), max_abs_dlogit_vs_per_clip=dl))
                t_c, _ = timed(lambda: torch.cat([model.forward_features(*fp) for _, _, _, fp in bl]))
                lines.append(dict(base, path="padded", batch=bs, seconds=round(t_c, 5), clips_per_s=round(a.clips / t_c, 1),
                                  impl=F_egx.last_encoder_impl(), ragged_over_padded_time=round(t_b / t_c, 3)))
        for ln in lines[-(1 + 2 * len(batch_sizes)):]:
            print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
