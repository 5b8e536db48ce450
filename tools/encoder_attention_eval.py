"""The errors and the cost of the encoder's self-attention weights as an output (egx_self_attention_weights, egx_attention_rollout,
egx_encoder_self_weights; model.record_attention()), written to profiles/encoder_attention_report.txt. Needs the GPU.
  errors  the figures tests/test_gpu_enc_attn.py prints (e, s and the kernel error per case): the tool runs that file with -s, or takes
          the output of a run that was kept (--tests-log);
  cost 1  egx_self_attention_weights against the existing functional.cross_attention_weights run with Sq = S on the same q / k (the
          Q | K columns of an (N, 3d) fp32 matrix, d = 128, 4 heads of 32), at B = 256, S = 45 and at B = 32, S = 450: three interleaved
          pairs each, device events around `--iters` launches after a warm-up. The new kernel reads K once per 16 query rows, the old one
          once per query row: it must not be slower at either shape (the tool says so and exits 1 if it is);
  cost 2  a recorded C2 eval forward (TTM 3-task, B = 256, T = 15, f32s, no_grad) against the plain one: segment shares alone, weights +
          shares, and with the rollout; the rollout alone at L = 6, B = 32, S = 450.
usage: python tools/encoder_attention_eval.py [--iters 200] [--pairs 3] [--tests-log FILE | --no-tests] [--out profiles/encoder_attention_report.txt]"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_figures(log: str):
    keep = ("[", "H = ", "rollout L = ")
    lines = [ln.lstrip(".").rstrip() for ln in log.splitlines()]        # (pytest's progress dots precede the first line a test prints)
    return [ln for ln in lines if ln.startswith(keep) or " passed" in ln or " failed" in ln]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--tests-log", default="")
    ap.add_argument("--no-tests", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_attention_report.txt"))
    a = ap.parse_args()

    import torch
    from bench import csrc_sha
    from egot2_amd import functional as F_egx
    from egot2_amd.synth import make_workload
    dev = torch.device("cuda:0")
    out = [f"encoder attention report: {torch.cuda.get_device_name(0)}, csrc {csrc_sha()}, iters {a.iters}, pairs {a.pairs}", ""]

    def timed(fn, iters):
        """ms per call: device events around `iters` launches"""
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / iters

    def pairs(name_a, fa, name_b, fb, iters):
        for _ in range(10):
            fa(); fb()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(a.pairs):
            ta.append(timed(fa, iters))
            tb.append(timed(fb, iters))
        fmt = lambda ts: " ".join(f"{t * 1e3:8.1f}" for t in ts)  # noqa: E731
        out.append(f"    {name_a:34s} us/call: {fmt(ta)}   median {sorted(ta)[len(ta) // 2] * 1e3:8.1f}")
        out.append(f"    {name_b:34s} us/call: {fmt(tb)}   median {sorted(tb)[len(tb) // 2] * 1e3:8.1f}")
        return sorted(ta)[len(ta) // 2], sorted(tb)[len(tb) // 2]

    slower = []
    with torch.no_grad():
        out.append("cost 1: egx_self_attention_weights against functional.cross_attention_weights(Sq = S), d = 128, 4 heads of 32")
        gen = torch.Generator(device=dev).manual_seed(0)
        for B, S in ((256, 45), (32, 450)):
            for dt in (torch.float32, torch.bfloat16):
                qkv = torch.randn(B * S, 384, device=dev, generator=gen).to(dt)
                q, k = qkv[:, :128], qkv[:, 128:256]
                new = lambda: F_egx.self_attention_weights(q, k, 4, S)  # noqa: E731
                old = lambda: F_egx.cross_attention_weights(q, k, 4, S, S)  # noqa: E731
                d = (new() - old()).abs().max().item()
                out.append(f"  B = {B}, S = {S}, {str(dt)[6:]} operands (the two kernels differ by {d:.2e})")
                tn, to = pairs("enc_self_weights_kernel", new, "dec_cross_weights_kernel (Sq = S)", old, a.iters)
                segtab = torch.tensor([[S // 3] * 3] * B, dtype=torch.int32, device=dev)        # (on the device: no copy inside the timed call)
                seg = lambda: F_egx.self_attention_weights(q, k, 4, S, segments=segtab, weights=False)  # noqa: E731
                out.append(f"    segment shares alone (w never written)  us/call: {timed(seg, a.iters) * 1e3:8.1f}")
                if tn > to:
                    slower.append(f"B = {B}, S = {S}, {str(dt)[6:]}: new {tn * 1e3:.1f} us > old {to * 1e3:.1f} us")
        out.append("  condition (the new kernel is not slower at either shape): " + ("HOLDS" if not slower else "MISSED: " + "; ".join(slower)))
        out.append("")

        out.append("cost 2: recorded C2 eval forward (TTM 3-task, B = 256, T = 15, 1 layer, f32s, no_grad) against the plain one")
        wl = make_workload("c2", dev, batch=256, dtype="f32s", dropout=0.0)
        model, feats = wl["model"].eval(), wl["feats"]
        plain = lambda: model.forward_features(*feats)  # noqa: E731

        def recorded(**kw):
            def run():
                with model.record_attention(**kw):
                    model.forward_features(*feats)
            return run
        for label, kw in (("by_segment alone", dict(weights=False)), ("weights + by_segment", dict()), ("weights + by_segment + rollout", dict(rollout=True))):
            pairs("plain forward", plain, "recorded: " + label, recorded(**kw), max(a.iters // 4, 10))
        w = torch.softmax(torch.randn(6, 32, 450, 450, device=dev, generator=gen), -1)
        roll = lambda: F_egx.attention_rollout(w, segments=[150, 150, 150])  # noqa: E731
        for _ in range(3):
            roll()
        out.append(f"    rollout alone, L = 6, B = 32, S = 450 (5 products)  us/call: {timed(roll, max(a.iters // 10, 5)) * 1e3:8.1f}")
        out.append("")

    if not a.no_tests:
        if a.tests_log:
            log = open(a.tests_log).read()
        else:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_enc_attn.py"), "-m", "gpu", "-q", "-s", "-p",
                                "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT)
            log = r.stdout
        out.append("errors: the figures of tests/test_gpu_enc_attn.py (e = max |x - oracle|, s = max |oracle - uniform answer|; kernel error = "
                   "against the fp64 softmax of the call's own Q | K)")
        out += ["  " + ln for ln in test_figures(log)]
    text = "\n".join(out) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)
    sys.exit(1 if slower else 0)


if __name__ == "__main__":
    main()
