"""fp64 references of the wide bf16 path's kernels, one by one (csrc/wide_gemm.hip, wide_rows.hip, wide_attn.hip, wide_attn_bighead.hip), their
cases, inputs, error metric and bars: the gate of tests/test_gpu_wide_ops.py, tested on itself by tests/test_cpu_wide_ops.py.

Plain torch, one function per operator; nothing is imported from the product path (tests/dropmask.py supplies the dropout masks). Every reference
computes in the dtype (and on the device) of its arguments: fp64 arguments give the reference, fp32 arguments the yardstick. Operands are drawn in
fp32 and rounded to bf16 ONCE (`bf16r`), so the device and the reference multiply the same numbers; what is left of the device's error is its fp32
accumulation order and the roundings the kernels document (bf16 outputs; attention: P before P V, dS before the dQ / dK products, dropped P before
dV, the saved O in the long kernels' delta). `perturb=` names one deliberate mistake, used by the CPU test only.

Error metric (never one norm over a tensor)
    elem_err   per output element, |got - ref| over that element's scale: the absolute-value product sum_k |a||b| (+ |bias|, |residual|, ...) of a
               GEMM, the sum of |terms| of a column sum.
    row_err    per row, max |got - ref| over the row's largest |ref| (floored at 1e-3 of the tensor's largest |ref|): the row kernels.
    attention  per (clip, head, query) row of out, lse and dQ and per (clip, head, key) row of dK and dV - one head's dh columns of one token -
               over the row's largest absolute-value product: P |V| for out, |dS| |K| for dQ with |dS| taken before its cancellation,
               P (|mask dP| + |delta|) / sqrt(dh). A fully dropped row has scale 0 and must be exactly 0.
    A NaN, an inf or an unwritten (NaN-prefilled) element is an infinite error. bf16 outputs: `bf16_out=True` first takes one bf16 rounding of the
    reference value, 2^-8 |ref| per element, off the difference.
Bars
    BAR[op][kind] = FACTOR * FP32_ERR[op][kind]; FP32_ERR is the worst error over the operator's cases of the reference evaluated in fp32 (with the
    documented bf16 roundings) against its fp64 evaluation, measured by test_cpu_wide_ops.py, which holds each constant within 3x of what it
    measures. FACTOR = 8 as in tests/unit_ref.py. Bit-exact operators (the casts, the ReLU mask, which elements dropout zeroes) have no bar.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from tests import dropmask as dm

F64, F32 = torch.float64, torch.float32
FACTOR = 8.0
BF16_ROUND = 2.0 ** -8
SEED = 0x51DE0B5

# Measured by tests/test_cpu_wide_ops.py::test_fp32_reference_meets_the_bar (prints them with -s).
FP32_ERR = {
    "gemm_nt": {"out": 1.8e-7, "colsum": 6.9e-8},
    "gemm_tn": {"out": 1.5e-7},
    "colsum": {"out": 4.5e-8},
    "pos_grad": {"out": 7.7e-8},
    "pool_cast": {"out": 1.1e-7},
    "ln_fwd": {"out": 2.7e-7, "stats": 1.3e-7},
    "ln_bwd": {"dx": 1.1e-6, "dparam": 2.0e-7},
    "attention": {"out": 3.4e-3, "lse": 3.9e-7, "grad": 1.3e-2},       # out, grad: the bf16 roundings of P and dS
}
BAR = {op: {kind: FACTOR * e for kind, e in kinds.items()} for op, kinds in FP32_ERR.items()}
# Worst (smallest) error / bar of each perturbed reference over the cases it applies to (test_cpu_wide_ops.py requires >= 3 of every one).
PERTURB_RATIO = {
    "gemm_nt": {"bias_after_relu": 2.2e5, "drop_key_nm": 3.2e5, "residual_before_dropout": 1.7e5, "mask_scale_on_masked": 2.9e5, "colsum_drop_last_group": 7.1e4},
    "gemm_tn": {"drop_tail_k": 1.5e4, "assign": 2.2e4},
    "ln_fwd": {"var_dm1": 114.0, "drop_before_pos": 1.7e5, "pos_row_mod_S": 4.2e5},
    "ln_bwd": {"dbias_unmasked": 5.5e3, "dy_mask_input_row": 1.1e5},
    "pos_grad": {"drop_last_chunk": 6.3e4},
    # a case's figure is its largest error / bar over out, lse and the gradients (scale_dh_plus_1 shows in lse at head dim 512)
    "attention": {"scale_dh_plus_1": 272.0, "mask_row_stride_64": 19.4, "drop_last_key": 2.3e3, "mask_before_norm": 4.7, "delta_without_dropout": 4.0},
}


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def bf16r(t):
    """One rounding to bf16 (round to nearest even), kept in the dtype of `t`."""
    return t.to(torch.bfloat16).to(t.dtype)


def _finite_max(e) -> float:
    if e.numel() == 0:
        return 0.0
    m = e.max().item()
    return m if math.isfinite(m) else math.inf


def elem_err(got, ref, scale, bf16_out: bool = False) -> float:
    """max over elements of |got - ref| / scale (scale: a tensor broadcastable to ref, > 0 wherever ref can be non-zero)."""
    ref = ref.detach().to(F64)
    e = (got.detach().to(ref.device, F64) - ref).abs()
    if bf16_out:
        e = torch.where(torch.isfinite(e), (e - BF16_ROUND * ref.abs()).clamp(min=0), e)
    s = scale.to(ref.device, F64).expand_as(ref)
    e = torch.where(s > 0, e / s.clamp(min=1e-300), torch.where(e > 0, torch.full_like(e, math.inf), e))
    return _finite_max(torch.nan_to_num(e, nan=math.inf))


def row_scale(ref):
    """(..., 1): each row's largest |ref|, floored at 1e-3 of the tensor's largest (1 where the tensor is all zero)."""
    a = ref.detach().to(F64).abs()
    top = a.max().item() if a.numel() else 0.0
    return a.amax(-1, keepdim=True).clamp(min=1e-3 * top if top > 0 else 1.0)


def row_err(got, ref, bf16_out: bool = False) -> float:
    return elem_err(got, ref, row_scale(ref), bf16_out)


def drop_scale(seed: int, layer: int, site: int, rows, cols: int, p: float):
    """(len(rows), cols) fp64 keep-scale of a (row, column)-keyed site, as every row and GEMM kernel of the wide path keys it."""
    return dm.keep_scale(dm.site_key(seed, layer, site), np.asarray(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), p)


# ---- NT GEMM (wide_gemm_nt) ----------------------------------------------------------------------------------------------------------------
NT_64X64, NT_128_D4, NT_128_D2, NT_256X128, NT_PP256, NT_PP192 = range(6)      # egx_wide_gemm_variant(0, ...)
NT_VARIANT_NAME = ["64x64", "128x128 four stages", "128x128 two stages", "256x128", "ping-pong 256x256", "ping-pong 256x192"]


def _nt(name, M, N, K, variant, out="f", bias=False, relu=False, p=0.0, site=dm.SITE_RES1, res=False, mask=False, colsum=False, pad=0):
    return dict(name=name, M=M, N=N, K=K, variant=variant, out=out, bias=bias, relu=relu, p=p, site=site, res=res, mask=mask, colsum=colsum, pad=pad)


# out: "f" Cf, "b" Cb, "fb" both. pad: every leading dimension is its width + pad (lda / ldb: + 2 pad, multiples of 8).
# The production combinations of wide_host.hip: bias + dropout + residual (out-projection, FFN2), bias + ReLU + dropout into Cb (FFN1: Cb is the
# saved mask of the backward), mask x scale + colsum (the hidden gradient with its bias gradient), Cf and Cb together.
NT_CASES = [
    # each epilogue alone, 64 x 64 tiles (<= 256 tiles of 128 x 128, no column sums), more than one block, M and N off the tile
    _nt("plain", 135, 200, 64, NT_64X64, out="fb"),
    _nt("bias", 135, 200, 64, NT_64X64, bias=True),
    _nt("relu", 135, 200, 64, NT_64X64, relu=True, out="b"),
    _nt("dropout", 135, 200, 64, NT_64X64, p=0.5),
    _nt("residual", 135, 200, 64, NT_64X64, res=True),
    _nt("mask", 135, 200, 64, NT_64X64, mask=True, out="b"),
    _nt("colsum", 135, 200, 64, NT_128_D4, colsum=True),
    # edges
    _nt("m1", 1, 64, 64, NT_64X64, bias=True, res=True, out="fb"),
    _nt("n4", 65, 4, 64, NT_64X64, bias=True, p=0.1, res=True, out="fb"),              # N % 8 != 0: the accumulator-layout epilogue
    _nt("n4_colsum", 130, 4, 128, NT_128_D4, mask=True, colsum=True, out="b"),
    _nt("ld_pad", 130, 136, 128, NT_64X64, bias=True, p=0.1, site=dm.SITE_RES2, res=True, pad=8),
    _nt("ld_pad_mask", 127, 136, 64, NT_128_D4, mask=True, colsum=True, out="b", pad=4),
    _nt("t64_m63", 63, 72, 128, NT_64X64, bias=True, relu=True, p=0.5, site=dm.SITE_FFN, out="b"),
    _nt("t64_m65", 65, 128, 64, NT_64X64, bias=True, p=0.1, res=True),
    _nt("d4_m127", 127, 264, 128, NT_128_D4, colsum=True, out="fb"),
    _nt("d4_m129", 129, 256, 64, NT_128_D4, mask=True, colsum=True, out="b"),
    _nt("d2_m8193", 8193, 512, 64, NT_128_D2, bias=True, p=0.1, res=True),
    _nt("d2_m8447", 8447, 512, 128, NT_128_D2, mask=True, colsum=True, out="b"),
    _nt("t256_m43775", 43775, 384, 64, NT_256X128, bias=True, relu=True, p=0.1, site=dm.SITE_FFN, out="b"),
    _nt("t256_m43777", 43777, 384, 64, NT_256X128, mask=True, colsum=True),
    _nt("pp256_m22015", 22015, 768, 64, NT_PP256, mask=True, colsum=True, out="b"),
    _nt("pp256_m16385", 16385, 1024, 128, NT_PP256, bias=True, res=True, out="fb"),
    _nt("pp256_n1028", 16385, 1028, 64, NT_PP256, bias=True, p=0.1, res=True),          # N % 8 != 0 in the ping-pong kernel
    _nt("pp192_m22015", 22015, 768, 64, NT_PP192, bias=True, p=0.1, site=dm.SITE_FEAT, res=True),
    _nt("pp192_m22017", 22017, 768, 64, NT_PP192, bias=True, relu=True, p=0.5, site=dm.SITE_FFN, out="b"),
]
NT_MASK_P = 0.3          # the bf16 `mask` operand: a saved ReLU + dropout output, zero where either dropped


def nt_colsum_rows(M: int, variant: int) -> int:
    """wide_gemm_nt_colsum_rows: one partial row per 64 output rows of every tile (tiles of 256 rows in the three large variants, else 128)."""
    tile = 256 if variant >= NT_256X128 else 128
    return cdiv(M, tile) * (tile // 64)


def nt_inputs(c, device="cpu"):
    """-> dict of fp32 tensors on `device`: A (M, K), B (N, K) bf16-representable, bias (N,), residual (M, N), mask (M, N) bf16-representable with
    zeros. Drawn on the CPU so that both tests see the same numbers."""
    M, N, K = c["M"], c["N"], c["K"]
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K + len(c["name"]))
    t = {"A": bf16r(torch.randn(M, K, generator=g)), "B": bf16r(torch.randn(N, K, generator=g) / math.sqrt(K))}
    t["bias"] = torch.randn(N, generator=g) if c["bias"] else None
    t["residual"] = torch.randn(M, N, generator=g) if c["res"] else None
    if c["mask"]:
        keep = torch.rand(M, N, generator=g) >= NT_MASK_P
        t["mask"] = bf16r(torch.rand(M, N, generator=g) + 0.5) * keep
    else:
        t["mask"] = None
    return {k: (v.to(device) if v is not None else None) for k, v in t.items()}


def nt_mask_scale(c) -> float:
    return dm.inv_keep(NT_MASK_P) if c["mask"] else 1.0


def nt_drop(c, layer: int, swap: bool = False):
    """The (M, N) keep-scale of the case's dropout, keyed (m, n); swap: keyed (n, m) (a perturbation)."""
    if c["p"] <= 0:
        return None
    M, N = c["M"], c["N"]
    if swap:
        return drop_scale(SEED, layer, c["site"], np.arange(N), M, c["p"]).T.contiguous()
    return drop_scale(SEED, layer, c["site"], np.arange(M), N, c["p"])


def gemm_nt(A, B, bias=None, relu=False, drop=None, residual=None, mask=None, mask_scale=1.0, perturb=None):
    """-> (C, scale): C = residual + (mask != 0 ? mask_scale * v : 0), v = drop .* relu(A B^T + bias); scale = the absolute-value sum of C's terms."""
    v = A @ B.T
    s = A.abs() @ B.abs().T
    if bias is not None and perturb != "bias_after_relu":
        v, s = v + bias, s + bias.abs()
    if relu:
        v = torch.relu(v)
    if bias is not None and perturb == "bias_after_relu":
        v, s = v + bias, s + bias.abs()
    if residual is not None and perturb == "residual_before_dropout":
        v, s = v + residual, s + residual.abs()
    if drop is not None:
        d = drop.to(v.device, v.dtype)
        v, s = v * d, s * d.amax()
    if mask is not None:
        v = v * mask_scale if perturb == "mask_scale_on_masked" else torch.where(mask != 0, v * mask_scale, torch.zeros_like(v))
        s = s * abs(mask_scale)
    if residual is not None and perturb != "residual_before_dropout":
        v, s = v + residual, s + residual.abs()
    return v, s


def group_sums(C, rows: int, perturb=None):
    """(rows, N): sums of C's rows per 64 (zero rows past M)."""
    M, N = C.shape
    pad = torch.zeros(rows * 64, N, dtype=C.dtype, device=C.device)
    pad[:M] = C
    if perturb == "colsum_drop_last_group":
        pad[(M - 1) // 64 * 64:] = 0
    return pad.view(rows, 64, N).sum(1)


def nt_eval(c, dtype, layer: int, perturb=None, device="cpu"):
    """Case c in `dtype` -> dict: C, scale (M, N); colsum, colsum_scale (rows, N) when the case has column sums (of the unrounded C)."""
    t = {k: (v.to(dtype) if v is not None else None) for k, v in nt_inputs(c, device).items()}
    drop = nt_drop(c, layer, swap=perturb == "drop_key_nm")
    C, s = gemm_nt(t["A"], t["B"], t["bias"], c["relu"], drop, t["residual"], t["mask"], nt_mask_scale(c), perturb)
    r = {"C": C, "scale": s}
    if c["colsum"]:
        rows = nt_colsum_rows(c["M"], c["variant"])
        r["colsum"], r["colsum_scale"] = group_sums(C, rows, perturb), group_sums(s, rows)
    return r


# ---- TN GEMM (wide_gemm_tn, wide_tn_queue_add / _flush, wide_reduce_flush) -------------------------------------------------------------------
# (name, M, N, K, tile variant, split-K count, accumulate, path): path "now" = wide_gemm_tn, "defer" = its reduction through WideReduceBatch,
# "queue" = the grouped launch. Variant 0 = 128 x 128, 1 = 256 x 128, 2 = 256 x 256 (>= 9 tiles of it).
TN_CASES = [
    ("v0_k1", 128, 128, 1, 0, 1, 0, "now"), ("v0_k63", 128, 256, 63, 0, 1, 1, "now"), ("v0_k65", 128, 128, 65, 0, 1, 0, "defer"),
    ("v0_k512", 128, 128, 512, 0, 2, 1, "now"), ("v0_k705", 128, 256, 705, 0, 3, 0, "queue"), ("v0_k1024", 128, 128, 1024, 0, 4, 1, "defer"),
    ("v1_k64", 256, 128, 64, 1, 1, 0, "queue"), ("v1_k65", 256, 256, 65, 1, 1, 1, "defer"), ("v1_k511", 512, 384, 511, 1, 2, 0, "now"),
    ("v1_k705", 256, 128, 705, 1, 3, 1, "queue"),
    ("v2_k63", 768, 768, 63, 2, 1, 0, "now"), ("v2_k512", 768, 768, 512, 2, 2, 1, "queue"), ("v2_k705", 768, 768, 705, 2, 3, 0, "defer"),
]
# one grouped batch: every variant, different sizes, queued, deferred and immediate reductions side by side
TN_BATCH = ["v0_k705", "v1_k64", "v2_k512", "v0_k512", "v1_k65", "v1_k705", "v0_k1", "v2_k705"]


def tn_case(name):
    return next(c for c in TN_CASES if c[0] == name)


def tn_inputs(c, device="cpu"):
    """-> A (K, M), B (K, N) bf16-representable fp32, C0 (M, N) the non-zero prefill of the += target."""
    _, M, N, K = c[:4]
    g = torch.Generator().manual_seed(M * 3 + N + K * 11)
    return [t.to(device) for t in (bf16r(torch.randn(K, M, generator=g)), bf16r(torch.randn(K, N, generator=g)), torch.randn(M, N, generator=g) * 4)]


def gemm_tn(A, B, C0=None, perturb=None):
    """-> (C, scale): C = C0 + A^T B (C0 None: assign)."""
    if perturb == "drop_tail_k":
        k = A.shape[0] // 64 * 64
        A, B = A[:k], B[:k]
    C, s = A.T @ B, A.abs().T @ B.abs()
    if C0 is not None:
        s = s + C0.abs()
        if perturb != "assign":
            C = C + C0
    return C, s


def tn_eval(c, dtype, perturb=None, device="cpu"):
    A, B, C0 = [t.to(dtype) for t in tn_inputs(c, device)]
    return gemm_tn(A, B, C0 if c[6] else None, perturb)


# ---- bf16 column sums (wide_colsum_bf16 -> wide_reduce_rows / wide_row_reduce_flush) ---------------------------------------------------------
# (rows, cols, ld, defer): 70000 rows: the row blocks stop at 1024 / ceil(cols / 512), so a block sums more than 64 rows
COLSUM_CASES = [(1, 8, 8, 0), (63, 8, 16, 1), (65, 512, 512, 0), (300, 520, 528, 1), (4097, 520, 520, 0), (70000, 8, 24, 0), (70000, 520, 528, 1)]


def colsum_inputs(rows, cols, device="cpu"):
    g = torch.Generator().manual_seed(rows * 5 + cols)
    return bf16r(torch.randn(rows, cols, generator=g)).to(device), (torch.randn(cols, generator=g) * 4).to(device)


def colsum(x, out0):
    """-> (out0 + column sums, scale)."""
    return out0 + x.sum(0), out0.abs() + x.abs().sum(0)


# ---- learned positional-table gradient (wide_pos_grad) ---------------------------------------------------------------------------------------
# (B, S, off, T, d, pos_stride, p)
POS_GRAD_CASES = [(1, 7, 2, 3, 8, 8, 0.0), (2, 7, 2, 3, 260, 264, 0.5), (3, 5, 0, 5, 8, 12, 0.1), (63, 7, 4, 3, 260, 260, 0.5), (64, 7, 2, 3, 8, 16, 0.0),
                  (65, 4, 1, 2, 256, 260, 0.1), (257, 7, 2, 3, 8, 8, 0.5)]


def pos_grad_chunks(B: int):
    """wide_rows.hip pos_grad_chunks -> (chunks, clips per chunk): the partial sums the scratch must hold."""
    want = 32 if B >= 64 else cdiv(B, 2)
    bchunk = cdiv(B, want)
    return cdiv(B, bchunk), bchunk


def pos_grad_inputs(c, device="cpu"):
    B, S, off, T, d, ps, p = c
    g = torch.Generator().manual_seed(B * 13 + S + d)
    return torch.randn(B * S, d, generator=g).to(device), (torch.randn(T, ps, generator=g) * 4).to(device)


def pos_grad(dtok, dpos0, c, layer: int, perturb=None):
    """-> (dpos, scale) (T, pos_stride): dpos0 + sum_b mask .* dtok[b * S + off + t] in the first d columns, dpos0 elsewhere."""
    B, S, off, T, d, ps, p = c
    rows = (np.arange(B)[:, None] * S + off + np.arange(T)[None, :]).reshape(-1)
    x = dtok[torch.as_tensor(rows, device=dtok.device)]
    if p > 0:
        x = x * drop_scale(SEED, layer, dm.SITE_POS, rows, d, p).to(x.device, x.dtype)
    x = x.view(B, T, d)
    if perturb == "drop_last_chunk":
        chunks, bchunk = pos_grad_chunks(B)
        x = x[:(chunks - 1) * bchunk]
    out, s = dpos0.clone(), dpos0.abs().clone()
    out[:, :d] += x.sum(0)
    s[:, :d] += x.abs().sum(0)
    return out, s


# ---- casts (wide_cast, wide_pool_cast, wide_gather_cast) -------------------------------------------------------------------------------------
CAST_CASES = [(4, 4, 4), (64, 64, 64), (68, 60, 64), (132, 196, 200), (1, 8, 8), (3, 12, 12)]      # (R, C, ld); the transposed output needs R % 4 == 0
CAST_PLANTED = [0.0, -0.0, 1e-40, -1e-40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4e38, -3.4e38, math.inf, -math.inf, 2.0 ** -133, 65504.0]
POOL_CASES = [(5, 1, 8, 0), (5, 2, 8, 1), (67, 3, 264, 0), (67, 3, 264, 1), (300, 2, 1032, 0)]     # (R, pool, C, src_bf16)
GATHER_CASES = [(5, 9, 8, 0), (67, 130, 264, 1), (300, 301, 1032, 0)]                              # (R listed rows, source rows, C, src_bf16)


def cast_inputs(R, C, ld, device="cpu"):
    """(R, ld) fp32 with the planted values in front: ties, denormals, the largest finite values, infinities."""
    g = torch.Generator().manual_seed(R * 17 + C)
    x = torch.randn(R, ld, generator=g) * 3
    flat = x.view(-1)
    pl = torch.tensor(CAST_PLANTED[:flat.numel()])
    flat[:pl.numel()] = pl
    return x.to(device)


def pool_inputs(R, pool, C, src_bf16, device="cpu"):
    g = torch.Generator().manual_seed(R * 19 + pool + C)
    x = torch.randn(R * pool, C, generator=g)
    return (bf16r(x) if src_bf16 else x).to(device)


def pool_cast(x, pool: int):
    """mean over `pool` consecutive rows (the caller rounds to bf16)."""
    return x.view(-1, pool, x.shape[-1]).sum(1) / pool


def gather_rows(R, n_src):
    g = torch.Generator().manual_seed(R + n_src)
    return torch.randperm(n_src, generator=g)[:R].to(torch.int32)


# ---- LayerNorm forward (wide_ln_fwd, wide_ln_fwd_mapped) ---------------------------------------------------------------------------------------
LN_EPS = 1e-5


def _ln(name, rows, d, T=1, S=1, off=0, add=False, pos=False, pos_pad=0, p=0.0, p_out=0.0, mapped=False, out="fb", mask_dx32=False, defer=False):
    return dict(name=name, rows=rows, d=d, T=T, S=S, off=off, add=add, pos=pos, pos_pad=pos_pad, p=p, p_out=p_out, mapped=mapped, out=out,
                mask_dx32=mask_dx32, defer=defer)


# rows = clips * T. out: "f" y32 / dx32, "b" y16 / dx16, "fb" both. p: the dropout behind the LayerNorm (forward: on y; backward: the mask on dy);
# p_out (backward): the out-mask. 16400 rows: more than 16 x 1024, the backward's 1024 blocks then own 17 rows each.
LN_CASES = [
    _ln("r1_d4", 1, 4, out="f"), _ln("r3_d256", 3, 256, add=True, p=0.1, p_out=0.5), _ln("r4_d260", 4, 260, T=2, S=5, off=1, pos=True, pos_pad=4, p=0.5, p_out=0.1),
    _ln("r5_d1024", 5, 1024, T=5, S=7, off=2, add=True, pos=True, p=0.1, out="b", defer=True), _ln("r16_d1028", 16, 1028, T=4, S=6, off=1, pos=True, pos_pad=8, p=0.5, p_out=0.5, mask_dx32=True),
    _ln("r17_d2048", 17, 2048, add=True, p=0.1, p_out=0.1, out="b"), _ln("r16_d2048", 16, 2048, T=8, S=9, off=1, pos=True, p=0.5, defer=True),
    _ln("r17_d4", 17, 4, T=17, S=20, off=3, pos=True, pos_pad=4, p=0.5, p_out=0.5, out="f", mask_dx32=True),
    _ln("r16400_d256", 16400, 256, T=4, S=6, off=1, add=True, pos=True, p=0.1, p_out=0.1), _ln("r16400_d260", 16400, 260, p_out=0.5, out="b", defer=True),
    _ln("map_r17_d260", 17, 260, T=5, add=True, pos=True, pos_pad=4, p=0.5, p_out=0.1, mapped=True), _ln("map_r5_d1024", 5, 1024, T=3, pos=True, p=0.1, mapped=True, out="b"),
    _ln("map_r300_d256", 300, 256, T=7, add=True, p=0.1, p_out=0.5, mapped=True, out="f"),
]


def ln_case(name):
    return next(c for c in LN_CASES if c["name"] == name)


def ln_maps(c):
    """-> (orow (rows,), t (rows,), out_rows, out_map, src_map): where row `row` goes and which positional row it takes. Uniform: the T / S / off
    remap. Mapped: a permuted out_map (one spare row stays unwritten) and a src_map with gaps (padded source rows of a compacted feature)."""
    rows, T, S, off = c["rows"], c["T"], c["S"], c["off"]
    r = np.arange(rows)
    if not c["mapped"]:
        return (r // T) * S + off + r % T, r % T, cdiv(rows, T) * S, None, None
    g = torch.Generator().manual_seed(rows + c["d"])
    out_map = torch.randperm(rows + 1, generator=g)[:rows].numpy()
    src_map = np.cumsum(torch.randint(1, 4, (rows,), generator=g).numpy())
    return out_map, src_map % T, rows + 1, out_map.astype(np.int32), src_map.astype(np.int32)


def ln_inputs(c, device="cpu"):
    rows, d, T = c["rows"], c["d"], c["T"]
    g = torch.Generator().manual_seed(rows * 3 + d + T)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {"x": r(rows, d) * 2 + 0.5, "w": 1 + 0.5 * r(d), "b": 0.5 * r(d), "add": r(d) if c["add"] else None,
         "pos": r(T, d + c["pos_pad"]) if c["pos"] else None}
    _, _, out_rows, _, _ = ln_maps(c)
    t["dy"] = r(out_rows, d)
    for k in ("dw0", "db0", "dbias0", "dadd0"):
        t[k] = r(d) * 4
    return {k: (v.to(device) if v is not None else None) for k, v in t.items()}


def ln_stats(x, eps=LN_EPS, perturb=None):
    d = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / (d - 1 if perturb == "var_dm1" else d)
    return mean, 1 / torch.sqrt(var + eps)


def ln_fwd(t, c, layer: int, perturb=None):
    """-> (y (rows, d) in INPUT row order, stats (rows, 2), orow): y[row] is what the kernel writes to output row orow[row]."""
    orow, tpos, _, _, _ = ln_maps(c)
    x = t["x"]
    d = c["d"]
    mean, rstd = ln_stats(x, LN_EPS, perturb)
    y = (x - mean) * rstd * t["w"] + t["b"]
    if t["add"] is not None:
        y = y + t["add"]
    keep = drop_scale(SEED, layer, dm.SITE_POS, orow, d, c["p"]).to(y.device, y.dtype) if c["p"] > 0 else None
    if perturb == "drop_before_pos" and keep is not None:
        y = y * keep
    if t["pos"] is not None:
        tp = np.arange(c["rows"]) % c["S"] % c["T"] if perturb == "pos_row_mod_S" else tpos
        y = y + t["pos"][torch.as_tensor(tp, device=y.device), :d]
    if perturb != "drop_before_pos" and keep is not None:
        y = y * keep
    return y, torch.cat([mean, rstd], -1), orow


def ln_bwd(t, stats, c, layer: int, perturb=None):
    """stats: (rows, 2) the saved (mean, rstd), an input. -> dict: dx, m (= out-mask .* dx) (rows, d); dw, db, dadd, dbias (d,) added to their
    prefill, dbias from m as given (the caller substitutes the stored bf16 m); scales dx_scale (rows, 1), and per-column sums of |terms|."""
    orow, _, _, _, _ = ln_maps(c)
    d, rows = c["d"], c["rows"]
    g = t["dy"][torch.as_tensor(orow, device=t["dy"].device)]
    if c["p"] > 0:
        key_rows = np.arange(rows) if perturb == "dy_mask_input_row" else orow
        g = g * drop_scale(SEED, layer, dm.SITE_RES1, key_rows, d, c["p"]).to(g.device, g.dtype)
    mean, rstd = stats[:, :1], stats[:, 1:]
    xh = (t["x"] - mean) * rstd
    gw = g * t["w"]
    s1, s2 = gw.mean(-1, keepdim=True), (gw * xh).mean(-1, keepdim=True)
    dx = rstd * (gw - s1 - xh * s2)
    m = dx
    if c["p_out"] > 0:
        m = dx * drop_scale(SEED, layer, dm.SITE_FEAT, np.arange(rows), d, c["p_out"]).to(dx.device, dx.dtype)
    mb = dx if perturb == "dbias_unmasked" else m
    return {"dx": dx, "m": m, "dw": t["dw0"] + (g * xh).sum(0), "db": t["db0"] + g.sum(0), "dadd": t["dadd0"] + g.sum(0), "dbias": t["dbias0"] + mb.sum(0),
            "dw_scale": t["dw0"].abs() + (g * xh).abs().sum(0), "db_scale": t["db0"].abs() + g.abs().sum(0),
            "dadd_scale": t["dadd0"].abs() + g.abs().sum(0), "dbias_scale": t["dbias0"].abs() + mb.abs().sum(0)}


# ---- attention (wide_attn_fwd / _bwd) --------------------------------------------------------------------------------------------------------
ATTN_ROW_STRIDE = {"short": dm.ATTN_ROW_STRIDE["wide"], "long": 512, "bighead": 128}    # wide_attn.hip, wide_attn_bighead.hip: bh * 128 + query
ATTN_PS = [0.0, 0.1, 0.5]
# (class, B, S, H, dh). short: S <= 128 (two tile counts: S <= 64 and S <= 128); long: the online-softmax kernels, whose query tiles are split over
# 256 / (B H) workgroups (B H = 2: split; B H = 132: unsplit); bighead: one wave per (clip, head).
ATTN_CASES = ([("short", 2, S, 3, dh) for dh in (32, 64, 96, 128) for S in (1, 15, 16, 17, 64, 65, 127, 128)]
              + [("long", 1, S, 2, dh) for dh in (32, 64) for S in (129, 160, 161, 479, 480)]
              + [("long", 33, 129, 4, 32), ("long", 33, 161, 4, 64)]
              + [("bighead", 3, S, 2, dh) for dh in (256, 512) for S in (1, 15, 16)])


def attn_case_id(c):
    return f"{c[0]}_B{c[1]}S{c[2]}H{c[3]}dh{c[4]}"


def attn_inputs(c, device="cpu"):
    """-> qkv (B * S, 3d), d_out (B * S, d): bf16-representable fp32; q scaled so that the softmax is not flat."""
    _, B, S, H, dh = c
    d = H * dh
    g = torch.Generator().manual_seed(S * 7 + dh + B)
    qkv = torch.randn(B * S, 3 * d, generator=g)
    qkv[:, :d] *= 1.5
    return bf16r(qkv).to(device), bf16r(torch.randn(B * S, d, generator=g)).to(device)


def attn_mask(c, p: float, layer: int, row_stride=None):
    """(B, H, S, S) fp64 keep-scale: row (b * H + h) * stride + query, column key."""
    cls, B, S, H, dh = c
    if p <= 0:
        return None
    rs = row_stride or ATTN_ROW_STRIDE[cls]
    rows = (np.arange(B * H)[:, None] * rs + np.arange(S)[None, :]).reshape(B, H, S)
    return dm.keep_scale(dm.site_key(SEED, layer, dm.SITE_ATTN), rows, np.arange(S, dtype=np.int64), p)


def attention(qkv, d_out, c, mask=None, rounded: bool = False, perturb=None):
    """-> dict out (B, H, S, dh), lse (B, H, S), dq, dk, dv (B, H, S, dh): softmax(q k^T / sqrt(dh)) with a keep-scale on the probabilities, times
    v, and its backward written out (dS = P (mask dP - delta)). rounded: the kernels' bf16 roundings at their places."""
    cls, B, S, H, dh = c
    rb = bf16r if rounded else (lambda x: x)
    x = qkv.view(B, S, 3, H, dh)
    q, k, v = [x[:, :, i].transpose(1, 2) for i in range(3)]
    do = d_out.view(B, S, H, dh).transpose(1, 2)
    m = mask.to(q.device, q.dtype) if mask is not None else None
    if perturb == "drop_last_key":
        k, v = k[:, :, :-1], v[:, :, :-1]
        m = m[..., :-1] if m is not None else None
    s = q @ k.transpose(-1, -2) / math.sqrt(dh + 1 if perturb == "scale_dh_plus_1" else dh)
    lse = torch.logsumexp(s, -1)
    if perturb == "mask_before_norm" and m is not None:
        e = torch.exp(s - s.amax(-1, keepdim=True)) * m
        P = torch.nan_to_num(e / e.sum(-1, keepdim=True), nan=0.0)
        Pd = P
    else:
        P = torch.softmax(s, -1)
        Pd = P * m if m is not None else P
    Pd = rb(Pd)
    out = Pd @ v
    dP = do @ v.transpose(-1, -2)
    dPm = dP * m if (m is not None and perturb != "mask_before_norm") else dP
    if cls == "long":
        delta = (do * rb(out)).sum(-1, keepdim=True)                 # from the saved (bf16) attention output
    else:
        delta = (P * dPm).sum(-1, keepdim=True)
    if perturb == "delta_without_dropout":
        delta = (P * dP).sum(-1, keepdim=True)
    sc = 1 / math.sqrt(dh + 1 if perturb == "scale_dh_plus_1" else dh)
    dS = rb(P * (dPm - delta) * sc)
    r = {"out": out, "lse": lse, "dq": dS @ k, "dk": dS.transpose(-1, -2) @ q, "dv": Pd.transpose(-1, -2) @ do}
    if perturb == "drop_last_key":      # the dropped key's gradient rows: zero
        z = torch.zeros_like(q[:, :, :1])
        r["dk"], r["dv"] = torch.cat([r["dk"], z], 2), torch.cat([r["dv"], z], 2)
        return r
    # the scale of a row: its largest absolute-value product (dS before its cancellation: P (|mask dP| + |delta|))
    aS = P * (dPm.abs() + delta.abs()) * sc
    top = lambda x: x.amax(-1, keepdim=True)  # noqa: E731
    r.update(out_scale=top(Pd @ v.abs()), dq_scale=top(aS @ k.abs()), dk_scale=top(aS.transpose(-1, -2) @ q.abs()),
             dv_scale=top(Pd.transpose(-1, -2) @ do.abs()), lse_scale=lse.abs().clamp(min=1.0))
    return r


def attn_heads(t, c, cols: int = 1):
    """A packed (B * S, cols * d) device result -> `cols` tensors (B, H, S, dh)."""
    _, B, S, H, dh = c
    x = t.view(B, S, cols, H, dh)
    return [x[:, :, i].transpose(1, 2) for i in range(cols)]


# ---- the report (profiles/wide_ops_report.txt) -----------------------------------------------------------------------------------------------
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wide_ops_report.txt")
_WORST = {}


def note(op: str, kind: str, err: float, bar: float, case: str):
    """Keep the worst error of (op, kind) seen in this process and rewrite the report: one line per operator and output kind."""
    key = f"{op} {kind}"
    if key not in _WORST or err > _WORST[key][0]:
        _WORST[key] = (err, bar, case)
    old = {}
    if os.path.exists(REPORT):
        for ln in open(REPORT).read().splitlines():
            f = ln.split("|")
            if len(f) == 5 and not ln.startswith("#"):
                old[f[0].strip()] = ln
    for k, (e, b, cs) in _WORST.items():
        old[k] = f"{k:22s} | worst error {e:.3e} | bar {b:.3e} | error / bar {e / b if b else 0.0:.3f} | {cs}"
    try:
        with open(REPORT, "w") as f:
            f.write("# wide bf16 path, kernel by kernel against fp64 (tests/test_gpu_wide_ops.py; metric and bars: tests/wide_ops_ref.py).\n"
                    "# operator and output kind | worst measured device error | bar | ratio | the case it was measured at\n")
            f.write("\n".join(old[k] for k in sorted(old)) + "\n")
    except OSError as e:          # a read-only checkout: the figures are still printed by the caller
        print(f"wide ops report not written: {e}")
