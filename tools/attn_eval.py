"""The cost of the cross-attention weights as an output (decode / greedy_decode(..., return_attention=True) -> egx_decoder_cross_weights /
egx_decoder_generate_attn) against the same calls without the flag. eval() + no_grad, bf16, random memories resident on the device:
`decode` at the C5 HOI shape (B = 256, d = 512, 8 heads, 3 layers, S = 48, sy = 3) and `greedy_decode` at 40 steps, V = 600, S = 48. The
call with the flag and the call without are alternated --reps times after a warm-up, device-synchronised wall time each; medians and
spreads. No threshold is set.
  --only plain   greedy_decode WITHOUT the flag alone: one process per library for the comparison with another build
                 (EGX_LIB=<other .so> EGX_LIB_UNSAFE=1 python tools/attn_eval.py --only plain; interleave the processes on one box)
  --only prim    the primitive alone at both shapes and at Sq = 8, Sk = 1024, d = 1024 (a profiler run wants its launches:
                 rocprofv3 --kernel-trace --stats -- python tools/attn_eval.py --only prim --reps 20)
usage: python tools/attn_eval.py [--reps 9] [--out profiles/attn_weights_<tag>.json] [--only plain|prim]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "plain", "prim"])
    a = ap.parse_args()

    import torch
    from bench import csrc_sha
    from tests import greedy_ref as gr

    dev = torch.device("cuda:0")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    B, d, h, L, S, sy, V, n = 256, 512, 8, 3, 48, 3, 600, 40
    gen = torch.Generator(device=dev).manual_seed(0)
    line = {"tool": "attn_eval", "csrc_sha": csrc_sha(), "lib": os.environ.get("EGX_LIB", "product"), "compute": "bf16",
            "device": torch.cuda.get_device_name(0), "B": B, "d": d, "heads": h, "layers": L, "S": S, "sy": sy, "V": V, "n_steps": n,
            "reps": a.reps, "only": a.only}
    with torch.no_grad():
        if a.only == "prim":
            from egot2_amd import functional as F_egx
            shapes = {"decode_sq3_sk48_d512": (8, 64, 3, 48), "greedy_sq1_sk48_d512": (8, 64, 1, 48), "sq8_sk1024_d1024": (16, 64, 8, 1024)}
            for name, (H, dh, Sq, Sk) in shapes.items():
                q = torch.randn(B * Sq, H * dh, device=dev, generator=gen).bfloat16()
                kv = torch.randn(B * Sk, 2 * H * dh, device=dev, generator=gen).bfloat16()
                fn = lambda: F_egx.cross_attention_weights(q, kv[:, :H * dh], H, Sq, Sk)  # noqa: E731
                for _ in range(3):
                    fn()
                ts = [wall(fn) for _ in range(a.reps)]
                line[name + "_wall_ms"] = round(med(ts), 4)
        else:
            m, _, start = gr.hoi_model(d, h, L, V, 95)
            m = m.to(dev).set_compute("bf16").eval()
            mem = torch.randn(S, B, d, device=dev, generator=gen)
            st = torch.full((B,), start, dtype=torch.int64, device=dev)
            y = torch.randint(0, V, (B, sy), device=dev, generator=gen)
            calls = {"greedy_plain": lambda: m.greedy_decode(mem, st, n)}
            if not a.only:
                calls.update({"greedy_attn": lambda: m.greedy_decode(mem, st, n, return_attention=True),
                              "decode_plain": lambda: m.decode(y, mem), "decode_attn": lambda: m.decode(y, mem, return_attention=True)})
            for _ in range(3):
                for fn in calls.values():
                    fn()
            times = {k: [] for k in calls}
            for _ in range(a.reps):
                for k, fn in calls.items():
                    times[k].append(wall(fn))
            for k, ts in times.items():
                line.update({k + "_ms": round(med(ts), 4), k + "_min_ms": round(min(ts), 4), k + "_max_ms": round(max(ts), 4)})
            for kind in ("greedy", "decode"):
                if kind + "_attn" in times:
                    line[kind + "_attn_over_plain"] = round(med(times[kind + "_attn"]) / med(times[kind + "_plain"]), 3)
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([line], f, indent=1)


if __name__ == "__main__":
    main()
