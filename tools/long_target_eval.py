"""decode() over 21 target tokens with autograd (DecoderMixin.egx_long_targets -> the composed fp32 decoder on egx_target_attention_*): the
time of a training step and of its forward, at the LTA shape of DESIGN.md 4.6 (model(video, target[:, :-1], 'lta_verb') of
HOI/tasks/multitask/video_task_action.py:34-53): B = 256, d = 512, 8 heads, 3 layers, S = 4, |V| = 600, sy = 21, compute bf16 (the memory's
K | V projection follows it; the target-row GEMMs are fp32), random memories resident on the device.
  train_step   forward + backward of decode() through the new route in train mode (p = 0.1, loss = cross entropy), launches per step;
  forward      its forward alone (eval mode, autograd on) beside forced_decode on the same rows, interleaved: what the parallel pass gains
               over the sequential K/V-cached route;
  stock        for scale only: the same step over the model's nn modules in stock fp32 PyTorch.
Median of --reps after a warm-up, wall time between device synchronisations. Each step runs in a child process of its own under a time
limit; the first child that fails ends the run. Reported, not asserted.
usage: python tools/long_target_eval.py [--reps 7] [--out profiles/long_target_<tag>.json]
       python tools/long_target_eval.py --step train_step --loop 20      (the body alone, e.g. under a kernel trace)"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = ("train_step", "forward", "stock")
STEP_TIMEOUT = 240
B, D, H, L, S, V, SY, P = 256, 512, 8, 3, 4, 600, 21, 0.1


def run_step(step: str, reps: int, loop: int):
    import torch
    import torch.nn.functional as F
    from bench import csrc_sha
    from egot2_amd import _lib, functional as F_egx
    from tests import greedy_ref as gr

    dev = torch.device("cuda:0")
    lib = _lib.load()
    m, _, _ = gr.hoi_model(D, H, L, V, 95)
    m = m.to(dev).set_compute("bf16")
    m.egx_long_targets = True
    m.dp_rate = P
    m.pos_embed.dropout.p = P
    for layer in m.transformer_decoder.layers:
        for mod in layer.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = P
        layer.self_attn.dropout = layer.multihead_attn.dropout = P
    gen = torch.Generator().manual_seed(7)
    mem = torch.randn(S, B, D, generator=gen).to(dev)
    y, tgt = torch.randint(0, V, (B, SY), generator=gen).to(dev), torch.randint(0, V, (B, SY), generator=gen).to(dev)
    base = {"tool": "long_target_eval", "step": step, "csrc_sha": csrc_sha(), "device": torch.cuda.get_device_name(0), "B": B, "d": D,
            "heads": H, "layers": L, "S": S, "V": V, "sy": SY, "reps": reps}

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

    def stats(ts, name):
        ts = sorted(ts)
        return {f"{name}_ms": round(ts[len(ts) // 2], 4), f"{name}_min_ms": round(ts[0], 4), f"{name}_max_ms": round(ts[-1], 4)}

    def train_step(decode):
        m.zero_grad(set_to_none=True)
        mg = mem.detach().requires_grad_(True)
        F.cross_entropy(decode(y, mg).permute(1, 2, 0), tgt).backward()

    if step == "train_step":
        m.train()
        body = lambda: train_step(m.decode)  # noqa: E731
        for _ in range(3):
            body()
        assert F_egx.last_decoder_impl() == "composed_long"
        if loop:
            for _ in range(loop):
                body()
            torch.cuda.synchronize()
            return None
        fwd = lambda: m.decode(y, mem)  # noqa: E731
        return dict(base, mode="train, p = 0.1", **stats([wall(body) for _ in range(reps)], "fwd_bwd"), **stats([wall(fwd) for _ in range(reps)], "fwd"),
                    launches_per_step=launches(body), launches_per_forward=launches(fwd))
    if step == "forward":
        m.eval()
        new = lambda: m.decode(y, mem)  # noqa: E731

        def forced():
            with torch.no_grad():
                return m.forced_decode(mem, y)

        for _ in range(3):
            new()
            assert F_egx.last_decoder_impl() == "composed_long"
            forced()
        t_new, t_forced = [], []
        for _ in range(reps):
            t_new.append(wall(new))
            t_forced.append(wall(forced))
        diff = (new().detach() - forced()).abs().max().item()
        line = dict(base, mode="eval; composed_long with autograd on, forced_decode under no_grad, interleaved", **stats(t_new, "composed_long_fwd"),
                    **stats(t_forced, "forced_decode"), launches_composed_long=launches(new), launches_forced=launches(forced),
                    max_abs_logit_difference=diff)
        line["forced_over_composed_long"] = round(line["forced_decode_ms"] / line["composed_long_fwd_ms"], 2)
        return line
    if step == "stock":
        m.train()
        body = lambda: train_step(lambda yy, mm: gr.stock_decode(m, yy, mm))  # noqa: E731
        for _ in range(3):
            body()
        return dict(base, mode="train, p = 0.1; nn.TransformerDecoder in stock fp32 PyTorch (for scale)", **stats([wall(body) for _ in range(reps)], "fwd_bwd"))
    raise SystemExit(f"unknown step {step!r}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    ap.add_argument("--step", default="", choices=("",) + STEPS)
    ap.add_argument("--loop", type=int, default=0, help="with --step train_step: run the step this many times and report nothing")
    a = ap.parse_args()
    if a.step:
        line = run_step(a.step, a.reps, a.loop)
        if line is not None:
            print("RESULT " + json.dumps(line), flush=True)
        return 0
    lines = []
    for step in STEPS:      # one fresh child per step, each under its own time limit; nothing is started after a failure
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps)], capture_output=True, text=True,
                               timeout=STEP_TIMEOUT, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {STEP_TIMEOUT} s; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"step {step}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 1
        for ln in r.stdout.splitlines():
            if ln.startswith("RESULT "):
                lines.append(json.loads(ln[7:]))
                print(ln[7:], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
