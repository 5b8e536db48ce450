"""Training throughput of ragged batches for the EgoT2-g HHI model (TaskTranslationPromptTransformer.forward_features_ragged:
egx_ragged_encode_train_fwd / egx_ragged_encode_bwd + egx_decoder_ragged_train_fwd / egx_decoder_ragged_bwd) on training-like sets: N seeded
clips per task with T ~ U[15, 150] frames (the segments of a clip equal), d = 256, h = 4, L = 3, bf16, train mode with the reference's dropout
(0.1, positional 0.1). A step = forward from features + nn.CrossEntropyLoss + backward + FusedAdam. Per task (ttm, asd):
  (a) "reference"    the reference's scheme on the existing uniform training call: task ttm in same-length mini-batches of <= 15 clips
                     (SequenceBatchSampler, HHI/tasks/multitask/video_tasktranslation.py:144-156, configs/multitask/config.py:35), task asd
                     one clip per step (batch_size=1 over the length-bucketed dataset);
  (b) "shuffled_B"   shuffled ragged batches of --batches clips;
  (c) "uniform"      the uniform training step of ONE batch with as many tokens as the average (b) batch of the largest size (equal clips):
                     the cost yardstick of a (b) step.
(a) and (b) are timed interleaved (--reps alternating passes over the whole set after one warm-up pass each, device events, the median
reported); every pass trains the same frames, so frames/s compares directly. Each line carries ms per step and library launches per step
(egx_launch_count). Inputs are resident on the device before timing.
usage: python tools/ragged_train_g.py [--clips 1024] [--batches 64,256] [--reps 3] [--out profiles/ragged_train_g_<tag>.json]"""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tasks", default="ttm,asd")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch
    from bench import csrc_sha
    from egot2_amd import _lib, functional as F_egx, hhi_multitask
    from egot2_amd.synth import HHI_G_VOCAB
    from egot2_amd.train import FusedAdam
    from tests.util import hhi_args, seeded_state_dict

    dev = torch.device("cuda:0")
    lib = _lib.load()
    sizes = [int(x) for x in a.batches.split(",")]
    rng = np.random.default_rng(2027)
    g = torch.Generator().manual_seed(7)
    crit = torch.nn.CrossEntropyLoss()

    def make():
        m = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=3, dropout=0.1), HHI_G_VOCAB)
        m.load_state_dict(seeded_state_dict(m, 11))
        m.pos_embed.dropout.p = 0.1
        return m.to(dev).set_compute("bf16").train()

    lines = []
    for task in a.tasks.split(","):
        T = rng.integers(15, 151, size=a.clips)
        clips = [[torch.randn(1, int(t), 256, generator=g).to(dev) for _ in range(3)] for t in T]
        n_rows = (lambda idx: int(T[idx].sum())) if task == "asd" else (lambda idx: len(idx))

        def targets(idx):       # input tokens [task, answer] and labels [answer, </s>] per target row (asd: per frame)
            n = n_rows(idx)
            ans = torch.randint(5, 7, (n,), generator=g)
            return (torch.stack([torch.full((n,), HHI_G_VOCAB[task]), ans], 1).to(dev), torch.stack([ans, torch.zeros_like(ans)], 1).to(dev))

        def padded(idx, T_pad):
            return [torch.cat([torch.nn.functional.pad(clips[i][k], (0, 0, 0, T_pad - clips[i][k].shape[1])) for i in idx]) for k in range(3)]

        # (a) the reference's batches
        ref = []
        if task == "ttm":
            by_len = {}
            for i, t in enumerate(T):
                by_len.setdefault(int(t), []).append(i)
            for t, ids in sorted(by_len.items()):
                for s in range(0, len(ids), 15):
                    idx = np.array(ids[s:s + 15])
                    ref.append((padded(idx, t), None) + targets(idx))
        else:
            for i in range(a.clips):
                idx = np.array([i])
                ref.append((padded(idx, int(T[i])), None) + targets(idx))
        order = np.random.default_rng(4).permutation(len(ref))
        paths = {"reference": [ref[i] for i in order]}
        perm = np.random.default_rng(3).permutation(a.clips)
        for bs in sizes:
            bl = []
            for s in range(0, a.clips, bs):
                idx = perm[s:s + bs]
                bl.append((padded(idx, int(T[idx].max())), torch.from_numpy(T[idx])) + targets(idx))
            paths[f"shuffled_{bs}"] = bl
        # (c) one uniform batch of the largest ragged batch's average token count
        bs = max(sizes)
        tu = int(round(float(T.sum()) / a.clips))
        uidx = np.arange(bs)
        uf = [torch.randn(bs, tu, 256, generator=g).to(dev) for _ in range(3)]
        n_u = bs * tu if task == "asd" else bs
        ans = torch.randint(5, 7, (n_u,), generator=g)
        paths["uniform"] = [(uf, None, torch.stack([torch.full((n_u,), HHI_G_VOCAB[task]), ans], 1).to(dev),
                             torch.stack([ans, torch.zeros_like(ans)], 1).to(dev))] * 20
        del uidx

        state = {}
        for name in paths:
            m = make()
            state[name] = (m, FusedAdam(m.parameters(), lr=1e-4))

        def one_pass(name):
            m, opt = state[name]
            for feats, lens, y, labels in paths[name]:
                if lens is None:
                    logits = m.decode(y, m.encode_features(task, *feats)).permute(1, 2, 0)
                else:
                    logits = m.forward_features_ragged(task, *feats, y, lengths=lens)
                crit(logits, labels).backward()
                opt.step()
                opt.zero_grad(set_to_none=True)

        times = {name: [] for name in paths}
        launches, impls = {}, {}
        for name in paths:      # warm-up pass (workspaces, LDS attributes, the optimizer's flat buffers) + the launch count of a pass
            one_pass(name)
            torch.cuda.synchronize()
            lib.egx_launch_count(1)
            one_pass(name)
            torch.cuda.synchronize()
            launches[name] = int(lib.egx_launch_count(1)) / len(paths[name])
            impls[name] = (F_egx.last_encoder_impl(), F_egx.last_decoder_impl())
        for _ in range(a.reps):
            for name in paths:  # interleaved: every path sees the same box in the same minute
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                one_pass(name)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / 1e3)
        base = {"tool": "ragged_train_g", "csrc_sha": csrc_sha(), "task": task, "compute": "bf16", "d": 256, "h": 4, "L": 3, "p": 0.1,
                "clips": a.clips, "T": "U[15,150], equal segments", "device": torch.cuda.get_device_name(0), "reps": a.reps}
        frames = 3 * int(T.sum())
        first = len(lines)
        for name, bl in paths.items():
            t = sorted(times[name])[len(times[name]) // 2]
            line = dict(base, path=name, steps=len(bl), ms_per_step=round(1e3 * t / len(bl), 4), launches_per_step=round(launches[name], 1),
                        encoder_impl=impls[name][0], decoder_impl=impls[name][1], seconds_all=[round(x, 5) for x in times[name]])
            if name == "uniform":
                line.update(batch=bs, T=tu, tokens=3 * bs * tu)
            else:
                line.update(mean_batch=round(a.clips / len(bl), 1), frames_trained=frames, frames_per_s=round(frames / t, 1))
            lines.append(line)
        ref_fps = lines[first]["frames_per_s"]
        for ln in lines[first + 1:]:
            if "frames_per_s" in ln:
                ln["frames_per_s_vs_reference"] = round(ln["frames_per_s"] / ref_fps, 2)
        big = next(ln for ln in lines[first:] if ln["path"] == f"shuffled_{bs}")
        lines[-1]["ragged_step_over_uniform"] = round(big["ms_per_step"] / lines[-1]["ms_per_step"], 3)
        lines[-1]["ragged_mean_tokens"] = round(frames / big["steps"], 1)
        for ln in lines[first:]:
            print(json.dumps(ln), flush=True)
        del state, paths, clips
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
