"""Evaluation throughput of ragged batches for the EgoT2-g HHI model (TaskTranslationPromptTransformer.predict_features(..., lengths=):
egx_ragged_encode + egx_decoder_ragged_fwd) on validation-like sets: N seeded clips, d = 256, h = 4, L = 3, bf16, eval() + no_grad.
  task ttm: lam = ttm length T ~ U[15, 150], asd its own length ~ U[15, 150] (S_b = 2 T + T_asd <= 450);
  task asd: T ~ U[15, 150] frames, the three segments of a clip equal (the decoder then runs over sum_b T_b frame triples).
Per task:
  (a) "per_clip"  the reference's batch_size=1 loop (HHI/tasks/multitask/video_tasktranslation.py:83-101,176-187): predict_features per
                  clip on its unpadded frames;
  (b) "ragged"    predict_features(..., lengths=) over batches of --batches clips;
  (c) "padded"    the existing uniform predict_features on the same batches with every clip padded to its batch's longest: numerically
                  WRONG (the stock encoder has no key-padding mask, padded frames are attended to), the cost of the padded batch.
Each timed with device events after a warm-up pass (median of --reps); one JSON line per (task, path, batch) with clips/s, and for (b) the
max |logit (a) - logit (b)|. A last line holds the max |memory row| difference of each ragged clip against the same clip alone through the
existing uniform path. Inputs are resident on the device before timing.
usage: python tools/ragged_eval_g.py [--clips 1024] [--batches 64,256] [--out profiles/ragged_eval_g_<tag>.json]"""
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
    ap.add_argument("--reps", type=int, default=3, help="timed passes over the set per path (the median is reported)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from bench import csrc_sha
    from egot2_amd import functional as F_egx, hhi_multitask
    from egot2_amd.synth import HHI_G_VOCAB
    from tests.util import hhi_args, seeded_state_dict

    dev = torch.device("cuda:0")
    model = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=3, dropout=0.0), HHI_G_VOCAB)
    model.load_state_dict(seeded_state_dict(model, 11))
    model.pos_embed.dropout.p = 0.0
    model = model.to(dev).set_compute("bf16").eval()
    batch_sizes = [int(x) for x in a.batches.split(",")]
    rng = np.random.default_rng(2026)
    g = torch.Generator().manual_seed(7)

    def timed(fn):
        fn()        # warm-up pass (workspaces, the LDS attributes)
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
    worst_solo = 0.0
    for task in ("ttm", "asd"):
        T = rng.integers(15, 151, size=(a.clips, 3))
        T[:, 1] = T[:, 0]
        if task == "asd":
            T[:, 2] = T[:, 0]
        clips = [[torch.randn(1, int(t), 256, generator=g).to(dev) for t in row] for row in T]

        def padded(idx, T_pad):
            return [torch.cat([torch.nn.functional.pad(clips[i][k], (0, 0, 0, T_pad[k] - clips[i][k].shape[1])) for i in idx]) for k in range(3)]

        batches = {}
        for bs in batch_sizes:
            bl = []
            for s in range(0, a.clips, bs):
                idx = list(range(s, min(s + bs, a.clips)))
                T_own = [int(T[idx, k].max()) for k in range(3)]
                Tm = max(T_own) if task == "ttm" else T_own[0]
                bl.append((idx, padded(idx, T_own), torch.from_numpy(T[idx]), padded(idx, [Tm] * 3)))
            batches[bs] = bl
        base = {"tool": "ragged_eval_g", "csrc_sha": csrc_sha(), "task": task, "compute": "bf16", "d": 256, "h": 4, "L": 3,
                "clips": a.clips, "T": "U[15,150]" + (" (lam = ttm, asd its own)" if task == "ttm" else " (equal segments)"),
                "device": torch.cuda.get_device_name(0)}
        with torch.no_grad():
            t_a, ref = timed(lambda: torch.cat([model.predict_features(task, *c) for c in clips]))
            lines.append(dict(base, path="per_clip", batch=1, seconds=round(t_a, 5), clips_per_s=round(a.clips / t_a, 1)))
            for bs in batch_sizes:
                bl = batches[bs]
                t_b, out = timed(lambda: torch.cat([model.predict_features(task, *f, lengths=ln) for _, f, ln, _ in bl]))
                assert F_egx.last_encoder_impl() == "ragged", F_egx.last_encoder_impl()
                dl = (out - ref).abs().max().item()
                lines.append(dict(base, path="ragged", batch=bs, seconds=round(t_b, 5), clips_per_s=round(a.clips / t_b, 1),
                                  speedup_vs_per_clip=round(t_a / t_b, 2), max_abs_dlogit_vs_per_clip=dl,
                                  decoder_impl=F_egx.last_decoder_impl()))
                t_c, _ = timed(lambda: torch.cat([model.predict_features(task, *fp) for _, _, _, fp in bl]))
                lines.append(dict(base, path="padded", batch=bs, seconds=round(t_c, 5), clips_per_s=round(a.clips / t_c, 1),
                                  impl=F_egx.last_encoder_impl(), ragged_over_padded_time=round(t_b / t_c, 3)))
            # memory rows of a ragged batch against each clip alone through the existing uniform path (first 64 clips)
            if task == "ttm":
                idx, f, ln, _ = batches[batch_sizes[0]][0]
                mem = model.encode_features(task, *f, lengths=ln)
                r0 = 0
                for j, i in enumerate(idx):
                    S = int(ln[j].sum())
                    solo = model.encode_features(task, *clips[i])[:, 0]
                    worst_solo = max(worst_solo, (mem[r0:r0 + S] - solo).abs().max().item())
                    r0 += S
        for line in lines[-(1 + 2 * len(batch_sizes)):]:
            print(json.dumps(line), flush=True)
    lines.append({"tool": "ragged_eval_g", "check": "max |memory row (ragged batch) - memory row (clip alone, uniform path)|", "task": "ttm",
                  "clips": batch_sizes[0], "max_abs_diff": worst_solo})
    print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
