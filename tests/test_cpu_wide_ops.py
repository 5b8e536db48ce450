"""The gate of tests/test_gpu_wide_ops.py tested on itself (CPU): each reference of tests/wide_ops_ref.py evaluated in fp32 (with the kernels'
documented bf16 roundings) meets the GPU test's bar on the GPU test's own inputs, every recorded yardstick is what this file measures, every
perturbed reference misses its bar at least 3x; and the host side of the unit hooks: refusals, scratch and variant queries."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from tests import dropmask as dm
from tests import wide_ops_ref as wr

F64, F32 = torch.float64, torch.float32


class _Survey:
    """Per operator: kind -> worst fp32 error, and perturbation -> smallest error / bar over the cases it applies to."""

    def __init__(self, op):
        self.op, self.fp32, self.pert = op, {}, {}

    def yard(self, kind, err):
        self.fp32[kind] = max(self.fp32.get(kind, 0.0), err)

    def miss(self, name, kind, err):
        """One case of a perturbation: kind -> error (or one kind and its error). The GPU test fails when ANY output misses its bar, so the case's
        figure is its largest error / bar; the perturbation's is the smallest over its cases."""
        errs = kind if isinstance(kind, dict) else {kind: err}
        self.pert[name] = min(self.pert.get(name, math.inf), max(e / wr.BAR[self.op][k] for k, e in errs.items()))


# ---- one pass per operator: the fp64 reference of a case is computed once and serves the yardstick and every perturbation ------------------
@functools.lru_cache(None)
def _survey_nt():
    s = _Survey("gemm_nt")
    applies = {"bias_after_relu": lambda c: c["bias"] and c["relu"], "drop_key_nm": lambda c: c["p"] > 0,
               "residual_before_dropout": lambda c: c["res"] and c["p"] > 0, "mask_scale_on_masked": lambda c: c["mask"],
               "colsum_drop_last_group": lambda c: c["colsum"]}
    for i, c in enumerate(wr.NT_CASES):
        ref = wr.nt_eval(c, F64, i)
        got = wr.nt_eval(c, F32, i)
        s.yard("out", wr.elem_err(got["C"], ref["C"], ref["scale"]))
        if c["colsum"]:
            s.yard("colsum", wr.elem_err(got["colsum"], ref["colsum"], ref["colsum_scale"]))
        for name, ok in applies.items():
            if not ok(c):
                continue
            bad = wr.nt_eval(c, F32, i, name)
            if name == "colsum_drop_last_group":
                s.miss(name, "colsum", wr.elem_err(bad["colsum"], ref["colsum"], ref["colsum_scale"]))
            else:
                s.miss(name, "out", wr.elem_err(bad["C"], ref["C"], ref["scale"]))
    return s


@functools.lru_cache(None)
def _survey_tn():
    s = _Survey("gemm_tn")
    for c in wr.TN_CASES:
        ref, scale = wr.tn_eval(c, F64)
        s.yard("out", wr.elem_err(wr.tn_eval(c, F32)[0], ref, scale))
        if c[3] % 64:
            s.miss("drop_tail_k", "out", wr.elem_err(wr.tn_eval(c, F32, "drop_tail_k")[0], ref, scale))
        if c[6]:
            s.miss("assign", "out", wr.elem_err(wr.tn_eval(c, F32, "assign")[0], ref, scale))
    return s


@functools.lru_cache(None)
def _survey_rows():
    cs, pg, pc = _Survey("colsum"), _Survey("pos_grad"), _Survey("pool_cast")
    for (rows, cols, ld, defer) in wr.COLSUM_CASES:
        x, o0 = wr.colsum_inputs(rows, cols)
        ref, scale = wr.colsum(x.double(), o0.double())
        cs.yard("out", wr.elem_err(wr.colsum(x, o0)[0], ref, scale))
    for i, c in enumerate(wr.POS_GRAD_CASES):
        dtok, dp0 = wr.pos_grad_inputs(c)
        ref, scale = wr.pos_grad(dtok.double(), dp0.double(), c, i)
        pg.yard("out", wr.elem_err(wr.pos_grad(dtok, dp0, c, i)[0], ref, scale))
        if wr.pos_grad_chunks(c[0])[0] > 1:
            pg.miss("drop_last_chunk", "out", wr.elem_err(wr.pos_grad(dtok, dp0, c, i, "drop_last_chunk")[0], ref, scale))
    for (R, pool, Cc, bf) in wr.POOL_CASES:
        x = wr.pool_inputs(R, pool, Cc, bf)
        pc.yard("out", wr.row_err(wr.pool_cast(x, pool), wr.pool_cast(x.double(), pool)))
    return cs, pg, pc


def _ln_eval(c, i, dtype, perturb=None):
    t = {k: (v.to(dtype) if v is not None else None) for k, v in wr.ln_inputs(c).items()}
    y, stats, _ = wr.ln_fwd(t, c, i, perturb)
    stats_in = wr.ln_fwd({k: v for k, v in wr.ln_inputs(c).items()}, c, i)[1].to(dtype)      # the saved statistics: fp32 numbers, an input of the backward
    return y, stats, wr.ln_bwd(t, stats_in, c, i, perturb)


@functools.lru_cache(None)
def _survey_ln():
    f, b = _Survey("ln_fwd"), _Survey("ln_bwd")
    for i, c in enumerate(wr.LN_CASES):
        ry, rs, rb = _ln_eval(c, i, F64)
        y, st, gb = _ln_eval(c, i, F32)
        f.yard("out", wr.row_err(y, ry))
        f.yard("stats", wr.elem_err(st, rs, rs.abs().clamp(min=1.0)))
        b.yard("dx", max(wr.row_err(gb["dx"], rb["dx"]), wr.row_err(gb["m"], rb["m"])))
        b.yard("dparam", max(wr.elem_err(gb[k], rb[k], rb[k + "_scale"]) for k in ("dw", "db", "dadd", "dbias")))
        T, S = c["T"], c["S"]
        if c["d"] >= 256:
            f.miss("var_dm1", "out", wr.row_err(_ln_eval(c, i, F32, "var_dm1")[0], ry))
        if c["pos"] and c["p"] > 0:
            f.miss("drop_before_pos", "out", wr.row_err(_ln_eval(c, i, F32, "drop_before_pos")[0], ry))
        if c["pos"] and not c["mapped"] and T < S and c["rows"] > S:
            f.miss("pos_row_mod_S", "out", wr.row_err(_ln_eval(c, i, F32, "pos_row_mod_S")[0], ry))
        if c["p_out"] > 0:
            bad = _ln_eval(c, i, F32, "dbias_unmasked")[2]
            b.miss("dbias_unmasked", "dparam", wr.elem_err(bad["dbias"], rb["dbias"], rb["dbias_scale"]))
        if c["p"] > 0 and (c["mapped"] or (T < S and c["rows"] > 1)):
            bad = _ln_eval(c, i, F32, "dy_mask_input_row")[2]
            b.miss("dy_mask_input_row", "dx", wr.row_err(bad["dx"], rb["dx"]))
    return f, b


def _attn_errs(got, ref, bf16_out=False):
    """bf16_out: with the GPU test's allowance for the bf16 rounding of out and d_qkv (the perturbations are judged as the device is)."""
    return {"out": wr.elem_err(got["out"], ref["out"], ref["out_scale"], bf16_out), "lse": wr.elem_err(got["lse"], ref["lse"], ref["lse_scale"]),
            "grad": max(wr.elem_err(got[k], ref[k], ref[k + "_scale"], bf16_out) for k in ("dq", "dk", "dv"))}


@functools.lru_cache(None)
def _survey_attn():
    s = _Survey("attention")
    for i, c in enumerate(wr.ATTN_CASES):
        cls, B, S, H, dh = c
        qkv, do = wr.attn_inputs(c)
        for p in wr.ATTN_PS:
            mask = wr.attn_mask(c, p, i)
            ref = wr.attention(qkv.double(), do.double(), c, mask)
            for kind, e in _attn_errs(wr.attention(qkv, do, c, mask, rounded=True), ref).items():
                s.yard(kind, e)

            def miss(name, m=mask):
                s.miss(name, _attn_errs(wr.attention(qkv, do, c, m, rounded=True, perturb=None if name == "mask_row_stride_64" else name), ref, True), None)
            if S > 1:
                miss("scale_dh_plus_1")
                miss("drop_last_key")
            if p > 0 and S > 1:
                miss("mask_row_stride_64", wr.attn_mask(c, p, i, row_stride=64))
                miss("mask_before_norm")
                if cls != "long":           # the long kernels take delta from the saved output, which holds the dropout
                    miss("delta_without_dropout")
    return s


def _surveys():
    cs, pg, pc = _survey_rows()
    f, b = _survey_ln()
    return [_survey_nt(), _survey_tn(), cs, pg, pc, f, b, _survey_attn()]


def test_fp32_reference_meets_the_bar():
    """Each reference in fp32 on the GPU test's inputs is inside the GPU test's bar, and the recorded FP32_ERR are what this measures."""
    for s in _surveys():
        assert set(s.fp32) == set(wr.FP32_ERR[s.op]), s.op
        for kind, e in s.fp32.items():
            rec, bar = wr.FP32_ERR[s.op][kind], wr.BAR[s.op][kind]
            print(f"fp32 yardstick {s.op:10s} {kind:7s} measured {e:.3e} recorded {rec:.3e} bar {bar:.3e}")
            assert bar == wr.FACTOR * rec
            assert e <= bar, f"{s.op} {kind}: the fp32 reference misses its own bar ({e} > {bar})"
            assert rec / 3 <= e <= rec * 3, f"{s.op} {kind}: recorded fp32 error {rec} is not the measured {e}"


def test_every_perturbation_misses_its_bar():
    for s in _surveys():
        assert set(s.pert) == set(wr.PERTURB_RATIO.get(s.op, {})), (s.op, sorted(s.pert))
        for name, ratio in s.pert.items():
            rec = wr.PERTURB_RATIO[s.op][name]
            print(f"perturbation {s.op:10s} {name:26s} worst error / bar = {ratio:.3g} (recorded {rec:.3g})")
            assert ratio >= 3, f"{s.op} / {name}: the bar lets the perturbed reference through (error / bar = {ratio})"
            assert ratio >= rec / 2, f"{s.op} / {name}: recorded ratio {rec} is not the measured {ratio}"


def test_bit_exact_operators_have_a_reference_that_rounds_to_nearest_even():
    """The cast reference is torch's fp32 -> bf16: ties to even, the largest finite fp32 to inf, denormals kept."""
    x = torch.tensor(wr.CAST_PLANTED)
    bits = x.to(torch.bfloat16).view(torch.int16).tolist()
    assert bits[4] == 0x3F80 and bits[5] == 0x3F82            # 1 + 2^-8 ties down to 1, 1 + 3 * 2^-8 ties up to 1 + 2^-6
    assert bits[6] == 0x7F80 and bits[7] == -128              # 3.4e38, above the largest finite bf16, rounds to +-inf
    assert bits[1] == -32768 and bits[2] == 1                 # -0 kept; 1e-40 rounds to the smallest bf16 denormal
    assert wr.bf16r(x).dtype == x.dtype


def test_mask_restatement_of_the_attention_classes():
    """The three attention classes key their mask rows (b H + h) * stride + query: 128, 512 for the long kernels, 128 for the big heads."""
    assert wr.ATTN_ROW_STRIDE == {"short": 128, "long": 512, "bighead": 128}
    c = ("long", 1, 130, 2, 32)
    m = wr.attn_mask(c, 0.5, 3)
    rows = 512 + np.arange(130)
    assert torch.equal(m[0, 1], dm.keep_scale(dm.site_key(wr.SEED, 3, dm.SITE_ATTN), rows, np.arange(130), 0.5))


# ---- the host side of the hooks ------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, *words):
    msg = lib.egx_last_error().decode()
    assert rc != 0 and msg, "the call was not refused with a message"
    for w in words:
        assert w in msg, (w, msg)


def _nt_args(**kw):
    from egot2_amd._lib import WideGemmArgs
    a = WideGemmArgs(layout=0, A=0x1000, B=0x2000, M=8, N=8, K=64, lda=64, ldb=64, Cf=0x3000, Cb=None, ldc=8, scratch=0x4000, mask_scale=1.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_gemm_hook_refusals(egx_lib):
    """Bad arguments are refused before anything is enqueued (the pointers here are never dereferenced)."""
    ex = lambda a: egx_lib.egx_wide_gemm_ex(C.byref(a), None)  # noqa: E731
    _refused(egx_lib, egx_lib.egx_wide_gemm_ex(None, None), "null")
    _refused(egx_lib, ex(_nt_args(layout=1)), "layout")
    _refused(egx_lib, ex(_nt_args(A=None)), "null")
    _refused(egx_lib, ex(_nt_args(scratch=None)), "null")
    _refused(egx_lib, ex(_nt_args(Cf=None)), "Cf or Cb")
    _refused(egx_lib, ex(_nt_args(A=0x1008)), "aligned")
    _refused(egx_lib, ex(_nt_args(bias=0x5004)), "aligned")
    _refused(egx_lib, ex(_nt_args(K=65, lda=72, ldb=72)), "K % 64")
    _refused(egx_lib, ex(_nt_args(N=6, ldc=8)), "N % 4")
    _refused(egx_lib, ex(_nt_args(lda=60)), "lda")
    _refused(egx_lib, ex(_nt_args(lda=56)), "below K")
    _refused(egx_lib, ex(_nt_args(ldc=4)), "ldc")
    _refused(egx_lib, ex(_nt_args(residual=0x6000, ldr=4)), "ldr")
    _refused(egx_lib, ex(_nt_args(mask=0x6000, ldm=6)), "ldm")
    _refused(egx_lib, ex(_nt_args(p_drop=1.5)), "probability")
    _refused(egx_lib, ex(_nt_args(accumulate=1)), "TN switches")
    _refused(egx_lib, ex(_nt_args(M=0)), "empty")
    tn = dict(layout=2, M=128, N=128, K=5, lda=128, ldb=128, ldc=128)
    _refused(egx_lib, ex(_nt_args(**{**tn, "M": 64, "lda": 64})), "multiples of 128")
    _refused(egx_lib, ex(_nt_args(**{**tn, "Cb": 0x7000})), "Cf only")
    _refused(egx_lib, ex(_nt_args(**{**tn, "relu": 1})), "no epilogue")
    _refused(egx_lib, ex(_nt_args(**{**tn, "lda": 120})), "below M")
    a = (type(_nt_args()) * 2)(_nt_args(**tn), _nt_args())
    _refused(egx_lib, egx_lib.egx_wide_gemm_tn_batch(a, 2, None), "not TN")
    _refused(egx_lib, egx_lib.egx_wide_gemm_tn_batch(a, 33, None), "1 .. 32")


def test_row_hook_refusals(egx_lib):
    from egot2_amd._lib import WideLnBwdArgs, WideLnFwdArgs
    f = lambda **kw: egx_lib.egx_wide_layernorm_fwd(C.byref(WideLnFwdArgs(**{**dict(x=0x1000, w=0x2000, b=0x3000, y32=0x4000, rows=4, d=8, T=1, S=1, eps=1e-5), **kw})), None)  # noqa: E731
    _refused(egx_lib, egx_lib.egx_wide_layernorm_fwd(None, None), "null")
    _refused(egx_lib, f(x=None), "null")
    _refused(egx_lib, f(y32=None), "null")
    _refused(egx_lib, f(d=6), "d=6")
    _refused(egx_lib, f(d=2052), "d=2052")
    _refused(egx_lib, f(d=1028, out_map=0x5000), "<= 1024")
    _refused(egx_lib, f(w=0x2004), "aligned")
    _refused(egx_lib, f(T=4, S=3), "T=4")
    _refused(egx_lib, f(pos=0x6000, pos_stride=4), "pos_stride")
    _refused(egx_lib, f(src_map=0x5000), "src_map")
    _refused(egx_lib, f(p_drop=-0.1), "probability")
    b = lambda **kw: egx_lib.egx_wide_layernorm_bwd(C.byref(WideLnBwdArgs(**{**dict(dy=0x1000, pre=0x2000, stats=0x3000, w=0x4000, dx32=0x5000, rows=4, d=8, T=1, S=1, scratch=0x6000), **kw})), None)  # noqa: E731
    _refused(egx_lib, b(scratch=None), "null")
    _refused(egx_lib, b(stats=None), "null")
    _refused(egx_lib, b(d=2052), "d=2052")
    _refused(egx_lib, b(d=1028, dy_map=0x7000), "<= 1024")
    _refused(egx_lib, b(dy_map=0x7000, defer=1), "never defers")
    _refused(egx_lib, b(dx32=0x5008), "aligned")
    _refused(egx_lib, b(p_out=2.0), "probability")
    from egot2_amd._lib import WideColsumArgs
    one = WideLnBwdArgs(dy=0x1000, pre=0x2000, stats=0x3000, w=0x4000, dx32=0x5000, rows=4, d=8, T=1, S=1, scratch=0x6000)
    _refused(egx_lib, egx_lib.egx_wide_row_reduce_batch(None, 0, None, 0, None), "reductions")
    _refused(egx_lib, egx_lib.egx_wide_row_reduce_batch(C.byref(one), 49, None, 0, None), "reductions")
    one.dy_map = 0x7000
    _refused(egx_lib, egx_lib.egx_wide_row_reduce_batch(C.byref(one), 1, None, 0, None), "never defers")
    _refused(egx_lib, egx_lib.egx_wide_row_reduce_batch(None, 0, C.byref(WideColsumArgs(x=0x1000, rows=4, cols=12, ld=16, out=0x2000, scratch=0x3000)), 1, None),
             "multiples of 8")
    _refused(egx_lib, egx_lib.egx_wide_colsum(None, 4, 8, 8, 0x1000, 0, 0x2000, None), "null")
    _refused(egx_lib, egx_lib.egx_wide_colsum(0x1000, 4, 12, 16, 0x2000, 0, 0x3000, None), "multiples of 8")
    _refused(egx_lib, egx_lib.egx_wide_colsum(0x1000, 4, 16, 8, 0x2000, 0, 0x3000, None), "ld >= cols")
    _refused(egx_lib, egx_lib.egx_wide_pos_grad(0x1000, 2, 4, 2, 3, 8, 0x2000, 8, 0.0, 0, 0, 2, 0x3000, None), "off=2")
    _refused(egx_lib, egx_lib.egx_wide_pos_grad(0x1000, 2, 4, 0, 3, 6, 0x2000, 8, 0.0, 0, 0, 2, 0x3000, None), "d=6")
    _refused(egx_lib, egx_lib.egx_wide_pos_grad(0x1000, 2, 4, 0, 3, 8, 0x2000, 4, 0.0, 0, 0, 2, 0x3000, None), "pos_stride=4")
    _refused(egx_lib, egx_lib.egx_wide_pos_grad(0x1000, 2, 4, 0, 3, 8, 0x2000, 8, 0.0, 0, 0, 2, None, None), "null")
    _refused(egx_lib, egx_lib.egx_wide_cast(3, 0x1000, 0, None, 4, 4, 4, 1, 0x2000, None, None), "mode")
    _refused(egx_lib, egx_lib.egx_wide_cast(0, 0x1000, 0, None, 6, 4, 4, 1, None, 0x2000, None), "multiples of 4")
    _refused(egx_lib, egx_lib.egx_wide_cast(0, 0x1000, 0, None, 4, 4, 4, 1, None, None, None), "null")
    _refused(egx_lib, egx_lib.egx_wide_cast(1, 0x1000, 0, None, 4, 12, 12, 2, 0x2000, None, None), "C % 8")
    _refused(egx_lib, egx_lib.egx_wide_cast(1, 0x1000, 0, None, 4, 8, 8, 0, 0x2000, None, None), "pool")
    _refused(egx_lib, egx_lib.egx_wide_cast(2, 0x1000, 0, None, 4, 8, 8, 1, 0x2000, None, None), "row list")


def test_attention_hook_refuses_what_no_kernel_serves(egx_lib):
    """S = 17 at head dim 256 / 512, a head dim no class has, S beyond the long kernels: refused by the dispatcher before any launch."""
    for (S, H, d) in [(17, 2, 512), (17, 2, 1024), (16, 2, 80), (129, 2, 192), (513, 2, 64), (0, 2, 64)]:
        _refused(egx_lib, egx_lib.egx_wide_attention_fwd(0x1000, 0x2000, 0x3000, 2, S, H, d, 0.0, 0, None), "unsupported")


def test_variant_and_scratch_queries_at_the_case_shapes(egx_lib):
    """Every case reaches the kernel it is meant for (the dispatcher's own answer), and the scratch / partial-row queries are the restated ones."""
    seen = set()
    for c in wr.NT_CASES:
        v = egx_lib.egx_wide_gemm_variant(0, c["M"], c["N"], c["K"], int(c["colsum"]))
        assert v == c["variant"], (c["name"], wr.NT_VARIANT_NAME[v])
        seen.add(v)
        if c["colsum"]:
            assert egx_lib.egx_wide_gemm_colsum_rows(c["M"], c["N"]) == wr.nt_colsum_rows(c["M"], c["variant"])
        assert egx_lib.egx_wide_gemm_scratch(0, c["M"], c["N"], c["K"]) == 1024
    assert seen == set(range(6))
    by_variant = {}            # the four large launches: M one past and one short of a tile multiple
    for c in wr.NT_CASES:
        if c["M"] > 8000:
            by_variant.setdefault(c["variant"], set()).add(c["M"] % 128)
    assert all(v == {1, 127} for v in by_variant.values()) and len(by_variant) == 4, by_variant
    seen = set()
    for (name, M, N, K, variant, splits, acc, path) in wr.TN_CASES:
        v = egx_lib.egx_wide_gemm_variant(2, M, N, K, 0)
        assert (v & 255, v >> 8) == (variant, splits), name
        assert egx_lib.egx_wide_gemm_scratch(2, M, N, K) == 1024 + splits * M * N * 4
        seen.add((variant, min(splits, 3)))
    assert seen == {(v, s) for v in range(3) for s in (1, 2, 3)}
    assert {c[3] for c in wr.TN_CASES} >= {1, 63, 65, 64, 512} and {c[7] for c in wr.TN_CASES} == {"now", "defer", "queue"}
    assert egx_lib.egx_wide_gemm_variant(2, 100, 128, 64, 0) == -1 and egx_lib.egx_wide_gemm_variant(0, 8, 8, 65, 0) == -1
    assert egx_lib.egx_wide_gemm_variant(1, 128, 128, 64, 0) == -1
    for (B, S, off, T, d, ps, p) in wr.POS_GRAD_CASES:
        assert egx_lib.egx_wide_pos_grad_scratch(B, T, d) == wr.pos_grad_chunks(B)[0] * T * d * 4
    assert egx_lib.egx_wide_pos_grad_scratch(0, 3, 8) == 0
    for (rows, cols, ld, defer) in wr.COLSUM_CASES:
        rb = min(wr.cdiv(rows, 64), wr.cdiv(1024, wr.cdiv(cols, 512)))
        assert egx_lib.egx_wide_colsum_scratch(rows, cols) == rb * cols * 4
    for c in wr.LN_CASES:
        assert egx_lib.egx_wide_layernorm_bwd_scratch(c["rows"], c["d"]) == min(1024, wr.cdiv(c["rows"], 16)) * 3 * c["d"] * 4
    assert {c["d"] for c in wr.LN_CASES} == {4, 256, 260, 1024, 1028, 2048}
    assert {c["rows"] for c in wr.LN_CASES} >= {1, 3, 4, 5, 16, 17} and max(c["rows"] for c in wr.LN_CASES) > 16 * 1024
