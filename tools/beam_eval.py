"""Beam search in one call (DecoderMixin.beam_decode -> egx_decoder_beam) against the only way to run W hypothesis rows per clip without it:
greedy_decode on the memory tiled W times (B * W clips, which yields W identical sequences). eval() + no_grad, bf16, random memories
resident on the device, the LTA shape: B = 256, d = 512, 8 heads, 3 layers, S = 48, V = 600, 40 steps, W = 5 (1280 tiled clips). The two
calls are alternated --reps times after a warm-up, device-synchronised wall time each; medians, spreads, launches per call. No threshold
is set. Also recorded: item 3 of tests/test_gpu_beam.py (worst |beam - decode()| logit difference over its n_steps <= 8 cases) and, per
case, the share of clips whose best sequence equals the fp64 oracle's best (CPU).
usage: python tools/beam_eval.py [--reps 7] [--out profiles/beam_<tag>.json] [--only timing|tests]"""
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=["", "timing", "tests"], help="one section only (a profiler run wants the timing loop alone)")
    a = ap.parse_args()

    import torch
    from bench import csrc_sha
    from egot2_amd import _lib
    from tests import beam_ref as br, greedy_ref as gr

    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = []
    base = {"tool": "beam_eval", "csrc_sha": csrc_sha(), "compute": "bf16", "device": torch.cuda.get_device_name(0)}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def launches(fn):
        lib.egx_launch_count(1)
        fn()
        torch.cuda.synchronize()
        return int(lib.egx_launch_count(0))

    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    with torch.no_grad():
        if a.only != "tests":
            B, d, h, L, S, V, n, W = 256, 512, 8, 3, 48, 600, 40, 5
            m, _, start = gr.hoi_model(d, h, L, V, 95)
            m = m.to(dev).set_compute("bf16").eval()
            mem = torch.randn(S, B, d, device=dev)
            tiled = mem.repeat_interleave(W, dim=1).contiguous()
            st, st_tiled = (torch.full((k,), start, dtype=torch.int64, device=dev) for k in (B, B * W))
            beam = lambda: m.beam_decode(mem, st, n, W)  # noqa: E731
            greedy = lambda: m.greedy_decode(tiled, st_tiled, n)  # noqa: E731
            for _ in range(3):
                beam(), greedy()
            t_beam, t_greedy = [], []
            for _ in range(a.reps):
                t_beam.append(wall(beam))
                t_greedy.append(wall(greedy))
            best_is_greedy = (beam()[:, 0] == m.greedy_decode(mem, st, n)).all(dim=-1).float().mean().item()
            lines.append(dict(base, case="lta_beam_vs_tiled_greedy", B=B, d=d, heads=h, layers=L, S=S, V=V, n_steps=n, W=W, reps=a.reps,
                              beam_ms=round(med(t_beam), 4), beam_min_ms=round(min(t_beam), 4), beam_max_ms=round(max(t_beam), 4),
                              tiled_greedy_ms=round(med(t_greedy), 4), tiled_greedy_min_ms=round(min(t_greedy), 4),
                              tiled_greedy_max_ms=round(max(t_greedy), 4), tiled_greedy_over_beam=round(med(t_greedy) / med(t_beam), 3),
                              beam_launches=launches(beam), tiled_greedy_launches=launches(greedy),
                              best_beam_equals_greedy_share=best_is_greedy))
            print(json.dumps(lines[-1]), flush=True)

        if a.only != "timing":
            worst, per_case, shares = 0.0, {}, {}
            for name, (d, h, L, V, S, B, n, W) in br.CASES.items():
                mm, sd64, start, mem64 = br.build_case(name)
                mm = mm.to(dev).set_compute("bf16").eval()
                memd = mem64.float().to(dev)
                tok, sc, trace = mm.beam_decode(memd, start, n, W, return_scores=True, return_trace=True)
                rt, rs, _, gaps = br.beam(sd64, h, torch.full((B,), start, dtype=torch.int64), mem64, n, W)
                shares[name] = dict(best_equals_oracle_share=(tok.cpu()[:, 0] == rt[:, 0]).all(dim=-1).float().mean().item(),
                                    smallest_oracle_gap=gaps.min().item(), median_oracle_gap=gaps[torch.isfinite(gaps)].median().item())
                if n > 8:
                    continue
                _, pars = br.backtrack(trace.step_tokens.cpu(), trace.step_parents.cpu())
                logits = trace.step_logits.cpu()
                anc = torch.stack([logits[t].gather(1, pars[t][..., None].expand(B, W, V)) for t in range(n)], 0).view(n, B * W, V)
                y = torch.cat((torch.full((B * W, 1), start, dtype=torch.int64, device=dev), tok.view(B * W, n)[:, :-1]), dim=1)
                per_case[name] = (anc - mm.decode(y, memd.repeat_interleave(W, dim=1)).cpu()).abs().max().item()
                worst = max(worst, per_case[name])
            lines.append(dict(base, check="tests/test_gpu_beam.py item 3: max |beam - decode()| logit difference (n_steps <= 8 cases)",
                              BEAM_VS_DECODE_MEASURED=worst, per_case=per_case, oracle_agreement=shares))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
