"""The sequence decoder at the LTA eval recipe's shape (HOI/configs/eval/lta.yaml:76 ForecastingEncoderSeparateSeqDecoder: d = 2048, 8 heads
of 256, 6 + 6 layers, d_ff 2048, a memory of NUM_INPUT_CLIPS = 2 rows, one target token) at B = 256 on the bf16 path: decoder forward +
backward time, and the per-case errors against the bars. Records into profiles/seqdec2048_report.txt.

    python tools/seqdec2048_eval.py                 # decode() forward + backward: 10 warm-up steps, 5 windows of 20 steps between device events
    python tools/seqdec2048_eval.py --errors        # device against R on tests/seqdec2048_ref.py DECODE_CASES (the GPU tests' figures)
    python tools/seqdec2048_eval.py --re            # CPU only: R against E on all five rows of RE_CASES
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o r -- python tools/seqdec2048_eval.py --steps-only 30
    python tools/seqdec2048_eval.py --kernel-stats DIR                # the attention launches' share from DIR/**/*kernel_stats.csv

There is no earlier number to compare the time with: before head dim 256 / 512 was served, the fused decoder refused this shape
(`fused decoder: d_model = 2048`) and the composed decoder refused its head dim (`small_attention: head dim 256 outside 1..128`)."""
import argparse
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tests import seqdec2048_ref as s  # noqa: E402

B, D, HEADS, L, S, SY, V = 256, 2048, 8, 6, 2, 1, 600


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--re", action="store_true")
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--kernel-stats", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        f = glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
        rows = list(csv.DictReader(open(f[0])))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        att = [r for r in rows if "dec_attn" in r["Name"]]
        tag = f"decode() forward + backward, B = {B}, d = {D}, heads = {HEADS}, {L} layers, S = {S}, sy = {SY}"
        lines = [f"{tag}: kernel time {tot / 1e6:.2f} ms over the profiled run; decoder attention launches {sum(float(r['TotalDurationNs']) for r in att) / tot * 100:.2f} % of it"]
        lines += [f"    {r['Name'][:100]}: {r['Calls']} calls, {float(r['AverageNs']) / 1e3:.1f} us average, {float(r['TotalDurationNs']) / tot * 100:.2f} %" for r in att]
        lines += [f"    top: {r['Name'][:100]}: {float(r['AverageNs']) / 1e3:.1f} us average, {float(r['TotalDurationNs']) / tot * 100:.1f} %" for r in rows[:6]]
        print("\n".join(lines))
        s.record("gpu measurement: attention share (rocprofv3 --kernel-trace --stats, a run of its own)", lines)
        return
    if a.re:
        lines = []
        for d, h, L_, sy, S_ in s.RE_CASES:
            data = s.case_data("fcst", d, h, L_, sy, S_, 3, stock=True)
            lines.append(s.gate_line(f"R vs E, stock weights, d = {d}, heads = {h}, L = {L_}, sy = {sy}, S = {S_}, B = 3",
                                     s.gate(s.oracle_run(data, True), s.oracle_run(data, False), s.BF16_BAR)))
            print(lines[-1])
        s.record("cpu: R against E on the stock seeded weights, all five rows (recorded, not a bar)", lines)
        return
    cuda = torch.device("cuda")
    if a.errors:
        lines = []
        for case in s.DECODE_CASES:
            data = s.case_data(*case)
            res = s.gpu_decode_run(data, cuda)
            g = s.gate(res, s.oracle_run(data, True), s.BF16_BAR)
            lines.append(s.gate_line(f"{case[0]} d = {case[1]}, heads = {case[2]}, L = {case[3]}, sy = {case[4]}, S = {case[5]}, B = {case[6]} ({res['impl']})", g))
            print(lines[-1])
        s.record("gpu tool: device against R at the decoder's bf16 bars", lines)
        return
    m = s.new_model("fcst", D, HEADS, L, V, cls="ForecastingEncoderSeparateSeqDecoder").to(cuda).set_compute("bf16").train()
    m.pos_embed.dropout.p = 0.0
    m._dec_dropout = 0.0
    mem = torch.randn(S, B, D, device=cuda, requires_grad=True)
    y = torch.randint(0, V, (B, SY), device=cuda)

    def step():
        m.zero_grad(set_to_none=True)
        mem.grad = None
        m.decode(y, mem).sum().backward()

    if a.steps_only:
        for _ in range(a.steps_only):
            step()
        torch.cuda.synchronize()
        return
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 20)
    ms.sort()
    from egot2_amd import functional as F_egx
    line = (f"decode() forward + backward, B = {B}, d = {D}, heads = {HEADS}, {L} layers, S = {S}, sy = {SY}, V = {V}, p = 0 ({F_egx.last_decoder_impl()}): "
            f"{ms[2]:.3f} ms per step (median of 5 windows of 20 steps between device events, after 10 warm-up steps; min {ms[0]:.3f}, max {ms[-1]:.3f}), "
            f"eager launches. No earlier figure exists: the parent refused this shape on both decoder paths.")
    print(line)
    s.record("gpu measurement: decoder forward + backward at the eval recipe's shape", [line])


if __name__ == "__main__":
    main()
