"""Teacher-forced decoding of up to 64 target tokens in one call (DecoderMixin.forced_decode -> egx_decoder_forced), eval() + no_grad, bf16:
the figures tests/test_gpu_forced.py holds it to, over that file's own cases, and the time of one call.
  timing   the LTA validation shape (model(video, target[:, :-1], 'lta_verb') of HOI/tasks/multitask/video_task_action.py:83-88): B = 256,
           d = 512, 8 heads, 3 layers, S = 4, |V| = 600, sy = 21, eagerly and as a captured-graph replay, launches per call. The library
           has no baseline at 21 tokens (decode() served at most 8 before this call existed), so sy = 8 is timed beside ONE fused decode()
           of the same rows: what the sequential route costs against a parallel pass where both exist. Reported, not asserted.
  item 2   worst |logits - fp64 oracle| and |logprob - oracle| per shape, with their bars;
  item 3   worst |forced - decode()| logit difference over the shapes cut to 7 and 8 tokens (FORCED_VS_DECODE_MEASURED);
  item 4   worst logits / logprob difference of K sequences per clip against K calls with one (FORCED_K_VS_ONE_MEASURED);
  item 9   worst |sum logprob - beam score| of beam_decode's own hypotheses, with the derived bound.
usage: python tools/forced_eval.py [--reps 7] [--out profiles/forced_<tag>.json] [--skip-tests-section]"""
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
    ap.add_argument("--skip-tests-section", action="store_true", help="timing only (the other sections need the fp64 oracle on the CPU)")
    a = ap.parse_args()

    import torch
    from bench import csrc_sha
    from egot2_amd import _lib, functional as F_egx
    from tests import beam_ref as br, greedy_ref as gr

    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = []
    base = {"tool": "forced_eval", "csrc_sha": csrc_sha(), "compute": "bf16", "device": torch.cuda.get_device_name(0)}

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
        # ---- the LTA validation shape
        B, d, h, L, S, V = 256, 512, 8, 3, 4, 600
        m, _, _ = gr.hoi_model(d, h, L, V, 95)
        m = m.to(dev).set_compute("bf16").eval()
        mem = torch.randn(S, B, d, device=dev)
        gen = torch.Generator().manual_seed(7)
        for sy in (21, 8):
            y, tgt = torch.randint(0, V, (B, sy), generator=gen).to(dev), torch.randint(0, V, (B, sy), generator=gen).to(dev)
            call = lambda: m.forced_decode(mem, y, targets=tgt)  # noqa: E731
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
            eager = call()
            assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
            line = dict(base, case=f"lta_validation_sy{sy}", B=B, d=d, heads=h, layers=L, S=S, V=V, sy=sy, reps=a.reps,
                        forced_eager_ms=round(med(t_eager), 4), forced_eager_min_ms=round(min(t_eager), 4), forced_eager_max_ms=round(max(t_eager), 4),
                        forced_graph_replay_ms=round(med(t_graph), 4), launches_per_call=n_launch)
            if sy <= 8:
                dec = lambda: m.decode(y, mem)  # noqa: E731
                for _ in range(3):
                    dec()
                assert F_egx.last_decoder_impl() == "fused"
                t_dec = [wall(dec) for _ in range(a.reps)]
                line.update(fused_decode_ms=round(med(t_dec), 4), forced_over_fused_decode=round(med(t_eager) / med(t_dec), 2),
                            fused_decode_launches=launches(dec))
            else:
                line.update(fused_decode_ms=None, fused_decode_note="decode() serves at most 8 target tokens on the fused and the composed decoder")
            lines.append(line)
            print(json.dumps(line), flush=True)

        if not a.skip_tests_section:
            from tests import test_gpu_forced as T
            item2, item3, item4, worst3, worst4 = {}, {}, {}, 0.0, [0.0, 0.0]
            for shape in T.SHAPES:
                d, h, L, V, S, B, K, sy = shape
                key = "-".join(map(str, shape))
                m, sd64, _ = T._model(d, h, L, V)
                y, tgt, mem64 = T._inputs(shape)
                mem = mem64.float().to(dev)
                yd, td = (y if K > 1 else y[:, 0]).to(dev), (tgt if K > 1 else tgt[:, 0]).to(dev)
                logits, logprob = m.forced_decode(mem, yd, targets=td)
                ref = T._oracle(sd64, h, y.view(B * K, sy), mem64.repeat_interleave(K, dim=1))
                ref_lp = torch.log_softmax(ref, -1).gather(2, tgt.view(B * K, sy).permute(1, 0)[..., None])[..., 0].permute(1, 0)
                item2[key] = dict(logits_err=(logits.cpu().view(sy, B * K, V).double() - ref).abs().max().item(),
                                  logprob_err=(logprob.cpu().view(B * K, sy).double() - ref_lp).abs().max().item(),
                                  bar=4e-2 * max(1.0, ref.abs().max().item()))
                for n in sorted({min(sy, 7), min(sy, 8)}):
                    yn = y[..., :n].contiguous().to(dev)
                    got = m.forced_decode(mem, yn if K > 1 else yn[:, 0])
                    dec = m.decode(yn.view(B * K, n), mem.repeat_interleave(K, dim=1))
                    item3[f"{key}@{n}"] = (got.reshape(n, B * K, V) - dec).abs().max().item()
                    worst3 = max(worst3, item3[f"{key}@{n}"])
                if K > 1:
                    ones = [m.forced_decode(mem, yd[:, k].contiguous(), targets=td[:, k].contiguous()) for k in range(K)]
                    dl = (logits - torch.stack([o[0] for o in ones], dim=2)).abs().max().item()
                    dp = (logprob - torch.stack([o[1] for o in ones], dim=1)).abs().max().item()
                    item4[key] = dict(logits=dl, logprob=dp)
                    worst4 = [max(worst4[0], dl), max(worst4[1], dp)]
            lines.append(dict(base, check="tests/test_gpu_forced.py item 2: worst |forced - fp64 oracle| per shape (d, heads, L, V, S, B, K, sy)", per_case=item2))
            lines.append(dict(base, check="tests/test_gpu_forced.py item 3: max |forced - decode()| logit difference (7 and 8 tokens)", worst=worst3,
                              per_case=item3))
            lines.append(dict(base, check="tests/test_gpu_forced.py item 4: K sequences per clip against K calls with one", worst_logits=worst4[0],
                              worst_logprob=worst4[1], per_case=item4))
            item9 = {}
            for name in ("base", "lta_schedule"):
                d, h, L, V, S, B, n, W = br.CASES[name]
                m, sd64, start, mem64 = br.build_case(name)
                m = m.to(dev).set_compute("bf16").eval()
                mem = mem64.float().to(dev)
                tokens, scores = m.beam_decode(mem, start, n, W, return_scores=True)
                y = torch.cat((torch.full((B, W, 1), start, dtype=torch.int64, device=dev), tokens[..., :-1]), dim=-1)
                _, logprob = m.forced_decode(mem, y, targets=tokens)
                ref = T._oracle(sd64, h, y.cpu().view(B * W, n), mem64.repeat_interleave(W, dim=1))
                item9[name] = dict(diff=(logprob.sum(-1) - scores).abs().max().item(), bound=n * 4 * 4e-2 * max(1.0, ref.abs().max().item()))
            lines.append(dict(base, check="tests/test_gpu_forced.py item 9: max |sum logprob - beam score| of beam_decode's hypotheses", per_case=item9))
            for line in lines[-4:]:
                print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
