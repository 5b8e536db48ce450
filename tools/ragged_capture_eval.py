#!/usr/bin/env python3
"""Errors and times of captured ragged d = 128 training steps (egx_ragged_cap_train_fwd / egx_ragged_cap_bwd: forward_features_ragged with
device lengths and a capacity inside train.GraphedStep) on the GPU; writes profiles/ragged_capture_report.txt (or --out). Recorded, not gated.

Part 1: per case of tests/test_gpu_ragged_cap.py the worst difference of a captured replay from the eager forward_features_ragged call on
the same clips with host lengths (logits, loss, d(feature): absolute; parameter gradients: relative) and from the per-clip fp64 oracle.
Part 2: a synthetic stream shaped like the TTM sampler (T drawn from 15 .. 150 per batch, B = 400 // T clips of 0.8 T .. T frames in each of
three segments), model TaskFusionMFTransformer3Task with one layer, FusedAdam:
    eager      forward_features_ragged with host lengths + backward + optimizer.step() per batch, features padded to the batch's longest clip
    captured   ONE GraphedStep at capacity (26 clips, 1 300 tokens, padded T = 150) replayed over the same batches (pad_ragged_batch ahead
               of the loop; the replay's copy of the batch into the captured buffers is inside the timed window)
  wall = host clock around the loop with one synchronisation at its end; events = device events around the same loop (for a host-bound loop
  the device idles between launches, and the two agree).
Part 3: the cost of capacity slack: the same batch through a step captured at (26, 1 300) and through one captured at exactly its own
(clips, tokens) - the weight-gradient launches of the first run over 1 300 token rows and the tile capacity whatever the batch holds.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from egot2_amd.train import FusedAdam, GraphedStep, pad_ragged_batch  # noqa: E402
from tests import dropmask as dm  # noqa: E402
from tests import test_gpu_ragged_cap as tc  # noqa: E402
from tests.test_gpu_ragged_train import CE_W, _model, _oracle_ttm  # noqa: E402
from tests.util import max_err, rel_err  # noqa: E402


def _vs_eager(got, want, slots):
    d_feat = max(max_err(g[slots], e) for g, e in zip(got[2], want[2]))
    return (max_err(got[0][slots], want[0]), abs(got[1].item() - want[1].item()), d_feat, max(rel_err(got[3][n], want[3][n]) for n in got[3]))


def _vs_oracle(got, slots, sd, clips, target, L, seed=0, p=0.0, p_pos=0.0):
    ref_logits, ref_loss, sd64, _ = _oracle_ttm(sd, clips, target, L, seed, p, p_pos)
    worst = max(rel_err(g, sd64[n].grad) for n, g in got[3].items() if n in sd64 and sd64[n].grad is not None)
    return max_err(got[0][slots], ref_logits), abs(got[1].item() - ref_loss.item()), worst


def errors(dev, lines):
    lines.append("captured replay against the eager call with host lengths (|d logits|, |d loss|, |d d(feature)|, worst parameter-gradient "
                 "rel_err) and against the per-clip fp64 oracle (|d logits|, |d loss|, worst parameter-gradient rel_err)")
    fmt = "  {:44s} eager {:9.2e} {:9.2e} {:9.2e} {:9.2e}   oracle {:9.2e} {:9.2e} {:9.2e}"
    for L in (1, 2):
        model, sd = _model("ttm3", L, "f32s", dev, seed=930 + L, p=0.0)
        data = {k: tc._cap_batch(b, 2000 + 10 * i, dev) for i, (k, b) in enumerate((("X", tc.X), ("Y", tc.Y), ("Z", tc.Z)))}
        want = {k: tc._eager(model, f, l, t, s, dev) for k, (f, l, t, _, s) in data.items()}
        step = tc._Step(model, data["X"][:3], (8, 400), dev)
        for k in ("X", "Y", "Z", "X"):
            f, l, t, clips, s = data[k]
            got = step(f, l, t)
            lines.append(fmt.format(f"f32s L={L} (8, 400) batch {k} ({len(s)} clips)", *_vs_eager(got, want[k], s),
                                    *_vs_oracle(got, s, sd, clips, t[s].cpu(), L)))
    for compute in ("f32s", "bf16"):
        model, sd = _model("ttm3", 1, compute, dev, seed=951, p=0.0)
        f, l, t, clips, s = tc._cap_batch([(107, 107, 107), None, (150, 150, 150)], 2200, dev, T_pad=150)
        want = tc._eager(model, f, l, t, s, dev)
        got = tc._Step(model, (f, l, t), (3, 900), dev)(f, l, t)
        lines.append(fmt.format(f"{compute} L=1 (3, 900) S = 321, 450", *_vs_eager(got, want, s), *_vs_oracle(got, s, sd, clips, t[s].cpu(), 1)))
    nan = float("nan")
    for compute in ("f32s", "bf16"):
        model, sd = _model("ttm3", 1, compute, dev, seed=961, p=0.5)
        model.enable_device_seed()
        f, l, t, clips, s = tc._cap_batch([(15, 15, 15), None, (16, 16, 17), (5, 9, 12), (17, 17, 17), None], 2300, dev)
        step = tc._Step(model, (f, l, t), (6, 200), dev)
        model._egx_seed_dev.fill_(0x5EED0123)
        got = step(f, l, t)
        lines.append(fmt.format(f"{compute} L=1 (6, 200) train mode p = 0.5 / 0.1", nan, nan, nan, nan,
                                *_vs_oracle(got, s, sd, clips, t[s].cpu(), 1, dm.lcg(0x5EED0123), 0.5, 0.1)))


def _stream(n, seed=7):
    """n sampler-like batches -> [(feats (B, T_max, 256) x 3 host, lengths (B, 3), target (B,))]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        T = int(rng.integers(15, 151))
        B = 400 // T
        lens = rng.integers(max(1, int(0.8 * T)), T + 1, size=(B, 3))
        feats = [torch.from_numpy(rng.standard_normal((B, int(lens[:, k].max()), 256), dtype=np.float32)) for k in range(3)]
        out.append((feats, torch.from_numpy(lens), torch.from_numpy(rng.integers(0, 2, B))))
    return out


def _timed(dev, fn, items):
    for it in items[:3]:
        fn(*it)
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for it in items:
        fn(*it)
    e1.record()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / len(items), e0.elapsed_time(e1) / len(items)


def _captured_step(model, example, capacity, dev, opt):
    w = torch.tensor(CE_W, device=dev)
    return GraphedStep(lambda f, l, t: model.forward_features_ragged(*f, lengths=l, target=t, class_weight=w, capacity=capacity)[1], example,
                       list(model.parameters()), optimizer=opt)


def timings(dev, lines, compute, n_batches):
    CAP = (26, 1300)
    stream = _stream(n_batches)
    w = torch.tensor(CE_W, device=dev)
    model, _ = _model("ttm3", 1, compute, dev, seed=77, p=0.0)
    opt = FusedAdam(model.parameters(), lr=1e-4)
    on_dev = [([x.to(dev) for x in f], l, t.to(dev)) for f, l, t in stream]

    def eager(f, l, t):
        opt.zero_grad(set_to_none=True)
        model.forward_features_ragged(*f, lengths=l, target=t, class_weight=w)[1].backward()
        opt.step()

    e_wall, e_ev = _timed(dev, eager, on_dev)
    model, _ = _model("ttm3", 1, compute, dev, seed=77, p=0.0)
    padded = [pad_ragged_batch([x.to(dev) for x in f], l, t, CAP, T_pad=150) for f, l, t in stream]
    step = _captured_step(model, padded[0], CAP, dev, FusedAdam(model.parameters(), lr=1e-4))
    c_wall, c_ev = _timed(dev, step, padded)
    assert model.ragged_status() == 0
    toks = [int(l.sum()) for _, l, _ in stream]
    lines.append(f"  {compute:5s} {n_batches:4d} batches, {min(toks)} .. {max(toks)} tokens (mean {sum(toks) / len(toks):.0f}), {min(len(l) for _, l, _ in stream)} .. "
                 f"{max(len(l) for _, l, _ in stream)} clips:   eager wall {e_wall:.3f} ms/step, events {e_ev:.3f}   |   captured at (26, 1300) "
                 f"wall {c_wall:.3f} ms/step, events {c_ev:.3f}   |   eager / captured {e_wall / c_wall:.2f}x")


def slack(dev, lines, compute):
    rng = np.random.default_rng(11)
    for T, B in ((15, 26), (60, 6), (150, 2)):
        lens = torch.full((B, 3), T)
        feats = [torch.from_numpy(rng.standard_normal((B, T, 256), dtype=np.float32)).to(dev) for _ in range(3)]
        tgt = torch.from_numpy(rng.integers(0, 2, B))
        res = []
        for cap, T_pad in (((26, 1300), 150), ((B, 3 * T * B), T)):
            model, _ = _model("ttm3", 1, compute, dev, seed=78, p=0.0)
            item = pad_ragged_batch(feats, lens, tgt, cap, T_pad=T_pad)
            step = _captured_step(model, item, cap, dev, FusedAdam(model.parameters(), lr=1e-4))
            res.append(_timed(dev, step, [item] * 200)[1])
        lines.append(f"  {compute:5s} {B:3d} clips of 3 x {T:3d} frames ({3 * T * B:4d} tokens): captured at (26, 1300) {res[0]:.3f} ms/step, at its own "
                     f"({B}, {3 * T * B}) {res[1]:.3f} ms/step: slack costs {res[0] - res[1]:+.3f} ms ({res[0] / res[1]:.2f}x)")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_capture_report.txt"))
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("ragged_capture_eval: no GPU visible; nothing was measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    lines = [f"captured ragged training step report ({torch.cuda.get_device_name(dev)}, torch {torch.__version__})", ""]
    errors(dev, lines)
    if not args.skip_timing:
        lines += ["", "TTM-sampler-like stream, one layer, FusedAdam, milliseconds per step (recorded, not asserted)"]
        for compute in ("f32s", "bf16"):
            timings(dev, lines, compute, args.batches)
        lines += ["", "cost of capacity slack, device events over 200 replays of one batch (the weight-gradient launches run at tok_cap rows)"]
        for compute in ("f32s", "bf16"):
            slack(dev, lines, compute)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
