"""Greedy generation in one call (DecoderMixin.greedy_decode -> egx_decoder_generate) against the prefix loop it replaces (predict_ac's
`_greedy`, egx_generate = False), eval() + no_grad, bf16, B = 256, random memories resident on the device:
  c5_hoi_2steps   d = 512, 8 heads, 3 layers, S = 48, V = 12, 2 steps (what predict_ac runs): loop and fused call alternated --reps times
                  after a warm-up, device-synchronised wall time each; medians, the loop's own spread, launches per call;
  steps40_S8/S48  d = 512, V = 600, 40 steps: the fused call eagerly and as a captured-graph replay, launches per step. The library has NO
                  baseline here: decode() serves at most 8 target tokens (fused and composed), so the prefix loop stops at step 9; the
                  prefix loop over the model's own nn modules in stock fp32 PyTorch is timed beside it for scale only.
Also recorded: item 3 of tests/test_gpu_generate.py (worst |generate - decode()| logit difference over its n_steps <= 8 cases) and the
decided shares of its item-4 cases (CPU, fp64 oracle).
usage: python tools/generate_eval.py [--reps 7] [--out profiles/generate_<tag>.json]"""
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
    ap.add_argument("--skip-tests-section", action="store_true", help="leave out item 3 / decided shares (they need the fp64 oracle on the CPU)")
    a = ap.parse_args()

    import torch
    from bench import csrc_sha
    from egot2_amd import _lib, functional as F_egx
    from tests import greedy_ref as gr

    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = []
    base = {"tool": "generate_eval", "csrc_sha": csrc_sha(), "compute": "bf16", "B": 256, "device": torch.cuda.get_device_name(0)}

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
    B = 256
    with torch.no_grad():
        # ---- the 2-step C5 HOI shape: today's loop against the fused call
        m, _, start = gr.hoi_model(512, 8, 3, 12, 98)
        m = m.to(dev).set_compute("bf16").eval()
        mem = torch.randn(48, B, 512, device=dev)
        like = torch.zeros(1, device=dev)

        def loop():
            m.egx_generate = False
            return m._greedy(mem, like, B)

        def fused():
            m.egx_generate = True
            return m._greedy(mem, like, B)

        for _ in range(3):
            loop(), fused()
        t_loop, t_fused = [], []
        for _ in range(a.reps):
            t_loop.append(wall(loop))
            t_fused.append(wall(fused))
        same = (loop() == fused()).float().mean().item()
        lines.append(dict(base, case="c5_hoi_2steps", d=512, heads=8, layers=3, S=48, V=12, n_steps=2, reps=a.reps,
                          loop_ms=round(med(t_loop), 4), loop_min_ms=round(min(t_loop), 4), loop_max_ms=round(max(t_loop), 4),
                          fused_ms=round(med(t_fused), 4), fused_min_ms=round(min(t_fused), 4), fused_max_ms=round(max(t_fused), 4),
                          loop_over_fused=round(med(t_loop) / med(t_fused), 3), loop_launches=launches(loop), fused_launches=launches(fused),
                          tokens_equal_share=same))
        print(json.dumps(lines[-1]), flush=True)

        # ---- 40 steps
        m, _, start = gr.hoi_model(512, 8, 3, 600, 95)
        m = m.to(dev).set_compute("bf16").eval()
        st = torch.full((B,), start, dtype=torch.int64, device=dev)
        for S in (8, 48):
            mem = torch.randn(S, B, 512, device=dev)
            call = lambda: m.greedy_decode(mem, st, 40)  # noqa: E731
            for _ in range(3):
                call()
            t_eager = [wall(call) for _ in range(a.reps)]
            n_launch = launches(call)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                call()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = call()
            g.replay()
            t_graph = [wall(g.replay) for _ in range(a.reps)]
            assert torch.equal(out, call())

            def stock_loop():
                toks = torch.empty((B, 41), dtype=torch.int64, device=dev)
                toks[:, 0] = st
                for t in range(40):
                    toks[:, t + 1] = gr.stock_decode(m, toks[:, :t + 1], mem)[-1].argmax(-1)
                return toks

            stock_loop()
            t_stock = [wall(stock_loop) for _ in range(3)]
            lines.append(dict(base, case=f"steps40_S{S}", d=512, heads=8, layers=3, S=S, V=600, n_steps=40, reps=a.reps,
                              fused_eager_ms=round(med(t_eager), 4), fused_graph_replay_ms=round(med(t_graph), 4),
                              launches_per_call=n_launch, launches_per_step=round((n_launch - (3 + len(m.transformer_decoder.layers))) / 40, 2),     # before step 0: memory cast, weight casts, embedding, a K | V projection per layer
                              library_loop_ms=None, library_loop_note="decode() serves at most 8 target tokens: the prefix loop stops at step 9",
                              stock_torch_fp32_prefix_loop_ms=round(med(t_stock), 3),
                              stock_over_fused_eager=round(med(t_stock) / med(t_eager), 2)))
            print(json.dumps(lines[-1]), flush=True)

        if not a.skip_tests_section:
            worst, per_case, shares = 0.0, {}, {}
            for name, (kind, d, h, L, V, S, Bc, n, ws, fs, item4) in gr.CASES.items():
                if n > 8:
                    continue
                mm, sd64, start, mem64 = gr.build_case(name)
                mm = mm.to(dev).set_compute("bf16").eval()
                memd = mem64.float().to(dev)
                tok, log = mm.greedy_decode(memd, start, n, return_logits=True)
                y = torch.cat((torch.full((Bc, 1), start, dtype=torch.int64, device=dev), tok[:, :-1]), dim=1)
                per_case[name] = (log - mm.decode(y, memd)).abs().max().item()
                worst = max(worst, per_case[name])
                if item4:
                    rt, rl, rm = gr.greedy(sd64, h, torch.full((Bc,), start, dtype=torch.int64), mem64, n)
                    dec = gr.decided(rm, 4e-2 * max(1.0, rl.abs().max().item()))
                    shares[name] = dict(decided_share=dec.float().mean().item(), tokens_on_decided=sorted(set(rt[dec].flatten().tolist())),
                                        device_equals_oracle_on_decided=bool(torch.equal(tok.cpu()[dec], rt[dec])))
            lines.append(dict(base, check="tests/test_gpu_generate.py item 3: max |generate - decode()| logit difference (n_steps <= 8 cases)",
                              worst=worst, per_case=per_case, item4=shares))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
