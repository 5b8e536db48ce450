"""Token schedules (greedy_decode / beam_decode(schedule=...) -> egx_decoder_generate_sched / egx_decoder_beam_sched) against the same
calls with schedule=None. eval() + no_grad, bf16, random memories resident on the device, the LTA shape of tests/test_gpu_sched.py's
case 5 at B = 256: d = 512, 8 heads, 3 layers, S = 8, V = 600, 40 steps, W = 5, P = 2 (row 0 = words 5..119, row 1 = words 120..599).
The scheduled and the unscheduled call are alternated --reps times after a warm-up, device-synchronised wall time each; medians and
spreads. No threshold is set. --only sched | free runs one kind alone (a profiler run wants the head launches of one kind:
rocprofv3 --kernel-trace --stats -- python tools/sched_eval.py --only sched --reps 1).
usage: python tools/sched_eval.py [--reps 9] [--out profiles/sched_<tag>.json] [--only sched|free]"""
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
    ap.add_argument("--only", default="", choices=["", "sched", "free"])
    a = ap.parse_args()

    import torch
    from bench import csrc_sha
    from tests import greedy_ref as gr, sched_ref as sr

    dev = torch.device("cuda:0")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    med = lambda ts: sorted(ts)[len(ts) // 2]  # noqa: E731
    B, d, h, L, S, V, n, W = 256, 512, 8, 3, 8, 600, 40, 5
    with torch.no_grad():
        m, _, start = gr.hoi_model(d, h, L, V, 95)
        m = m.to(dev).set_compute("bf16").eval()
        mem = torch.randn(S, B, d, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
        st = torch.full((B,), start, dtype=torch.int64, device=dev)
        sched = m.token_schedule(sr.alternation(V, range(5, 120), range(120, 600)))
        calls = {"greedy_sched": lambda: m.greedy_decode(mem, st, n, schedule=sched), "greedy_free": lambda: m.greedy_decode(mem, st, n),
                 "beam_sched": lambda: m.beam_decode(mem, st, n, W, schedule=sched), "beam_free": lambda: m.beam_decode(mem, st, n, W)}
        if a.only:
            calls = {k: v for k, v in calls.items() if k.endswith(a.only)}
        for _ in range(3):
            for fn in calls.values():
                fn()
        times = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, fn in calls.items():
                times[k].append(wall(fn))
    line = {"tool": "sched_eval", "csrc_sha": csrc_sha(), "compute": "bf16", "device": torch.cuda.get_device_name(0),
            "case": "lta_scheduled_vs_unscheduled", "B": B, "d": d, "heads": h, "layers": L, "S": S, "V": V, "n_steps": n, "W": W, "P": 2,
            "counts": sched.counts, "reps": a.reps}
    for k, ts in times.items():
        line.update({k + "_ms": round(med(ts), 4), k + "_min_ms": round(min(ts), 4), k + "_max_ms": round(max(ts), 4)})
    for kind in ("greedy", "beam"):
        if kind + "_sched" in times and kind + "_free" in times:
            line[kind + "_free_over_sched"] = round(med(times[kind + "_free"]) / med(times[kind + "_sched"]), 3)
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump([line], f, indent=1)


if __name__ == "__main__":
    main()
