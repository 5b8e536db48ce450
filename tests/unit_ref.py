"""fp64 references of the C ABI's unit operators (include/egot2x.h), their cases, inputs and bars: the gate of test_gpu_unit_ops.py.

Plain torch on the CPU, one function per operator; nothing here is imported from the product path (tests/dropmask.py supplies the dropout
masks). Every reference computes in the dtype of its arguments: fp64 arguments give the reference, fp32 arguments the yardstick ("the same
op in plain fp32 torch") the bars of the non-GEMM operators are taken from. `perturb=` names one deliberate mistake; it is used only by
tests/test_cpu_unit_ops.py, which checks that the bars reject each of them.

Bars
    GEMM-backed operators (egx_linear_fwd / _residual_fwd / _bwd): test_gemm's, GEMM_TOL[compute] * sqrt(reduction length) on randn operands;
    the reduction length is K for y, N for dx, M for dW and db.
    Every other operator: BAR[op][kind] = FACTOR * FP32_ERR[op][kind], where FP32_ERR is the worst error, over the operator's cases, of the
    fp32 evaluation of the reference against its fp64 evaluation on the GPU test's own inputs (kind "out": outputs, "grad": gradients). The
    error of a tensor is rel_err: max |got - ref| over that tensor's largest |ref|.
    FACTOR = 8 covers another summation order, __expf and rsqrtf. egx_relu_mask and egx_dropout are bit-exact and have no bar.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import dropmask as dm

F64 = torch.float64

# ---- bars ----------------------------------------------------------------------------------------------------------------------------------
GEMM_TOL = {0: 2e-5, 1: 2e-2, 2: 2e-5}          # egx compute mode (f32, bf16, f32s) -> tests/test_gpu_ops.py test_gemm's tolerance per sqrt(K)
FACTOR = 8.0
# Measured by tests/test_cpu_unit_ops.py (test_fp32_reference_meets_the_bar prints them with -s): worst rel_err of the fp32 evaluation
# over the operator's cases. The CPU test holds each constant to the value it measures (within 3x either way: another CPU's vector width
# changes torch's fp32 summation order), so a bar cannot be widened by editing the constant alone.
FP32_ERR = {
    "small_attention": {"out": 9.2e-7, "grad": 9.7e-7},
    "gelu": {"out": 1.0e-8, "grad": 7.3e-8},         # out: on the scale of the planted 40 (4.0e-7 absolute)
    "pool_head": {"out": 4.2e-7, "grad": 6.2e-7},
    "colsum": {"out": 5.7e-6},                       # (33, 65): 33 rows of 1e3 around a +-1e6 pair whose ulp is 0.06
}
BAR = {op: {kind: FACTOR * e for kind, e in kinds.items()} for op, kinds in FP32_ERR.items()}
# Worst (smallest) error / bar of each perturbed reference over the cases it applies to, as the test_perturbed_* tests of
# test_cpu_unit_ops.py measure them; they require >= 3 of every one.
PERTURB_RATIO = {
    "small_attention": {"causal_off_by_one": 7.2e4, "scale_dh_plus_1": 221.0, "mask_row_stride_64": 1.6e4, "mask_before_norm": 1.7e4,
                        "drop_last_key": 591.0},
    "linear_bwd": {"dw_assign": 7.9e3, "db_assign": 4.4e3},       # against the f32 bar 2e-5 * sqrt(M)
    "pool_head": {"pool_divisor": 447.0, "ln_var_dm1": 81.0},
    "gelu": {"tanh": 148.0},
    "dropout": {"scale_one": 854.0},                              # bit-exact check: kept elements whose bits differ (the bar is none)
}


def gemm_bar(compute: int, reduction: int) -> float:
    return GEMM_TOL[compute] * math.sqrt(reduction)


def max_err(got, ref) -> float:
    """max |got - ref| in fp64; a NaN or an inf anywhere counts as an infinite error."""
    e = (got.detach().double() - ref.detach().double()).abs()
    if e.numel() == 0:
        return 0.0
    m = e.max().item()
    return m if math.isfinite(m) else math.inf


def rel_err(got, ref) -> float:
    """max |got - ref| / max |ref|: the error of one tensor on the scale of that tensor (the plain max |got - ref| where ref is all zero).
    The metric of the non-GEMM operators: their cases span S = 1 .. 450 pooled rows and 1 .. 70000 summed ones, and a bar taken as the
    worst absolute error over such cases would be the largest case's alone."""
    m = ref.detach().double().abs().max().item() if ref.numel() else 0.0
    return max_err(got, ref) / (m if m > 0 else 1.0)


# ---- egx_small_attention_fwd / _bwd --------------------------------------------------------------------------------------------------------
SA_ROW_STRIDE = dm.DEC_ATTN_ROW_STRIDE           # 8: the mask row of query i of (clip b, head h) is (b * H + h) * 8 + i in both kernels
# (B, H, Sq, Sk, dh, causal, p_drop, layout). Layouts, with d = H * dh:
#   packed      q, k, v, o in buffers of their own, row stride d
#   self        q, q + d, q + 2d of ONE (rows, 3d) buffer
#   cross       q row stride d; k, k + d of ONE (rows, 2d) buffer
#   cross_ldo4  cross with o and d_o at row stride d + 4
#   odd         buffers of their own at row stride d + 1 (rows not 16-byte aligned)
ATTN_CASES = [
    (2, 4, 1, 1, 32, 0, 0.0, "packed"),         # degenerate softmax
    (2, 4, 5, 5, 32, 1, 0.0, "self"),           # causal, the HHI target
    (2, 4, 5, 5, 32, 1, 0.3, "self"),
    (1, 2, 8, 8, 128, 1, 0.3, "self"),          # Sq limit, dh limit, the one-wave kernel's `c += 64` channel loop
    (3, 4, 2, 63, 64, 0, 0.3, "cross"),         # idle lane in the one-wave kernel
    (3, 4, 5, 64, 64, 0, 0.3, "cross"),         # one-wave limit
    (3, 4, 5, 65, 64, 0, 0.0, "cross"),         # chunked kernel, last chunk of one key
    (3, 4, 5, 65, 64, 0, 0.3, "cross"),
    (2, 8, 8, 129, 128, 0, 0.3, "cross_ldo4"),  # all four acc[u] slots, padded rows
    (2, 2, 3, 128, 33, 0, 0.3, "odd"),          # head dim not a multiple of 32, exact chunks, unaligned rows
    (1, 4, 7, 1024, 32, 0, 0.3, "cross"),       # Sk limit
    (1, 1, 4, 200, 1, 0, 0.0, "packed"),        # dh = 1
]
ATTN_SEED = 0x5EED0A77


def attn_case_id(case) -> str:
    B, H, Sq, Sk, dh, causal, p, layout = case
    return f"B{B}H{H}_q{Sq}k{Sk}_dh{dh}_c{causal}_p{p}_{layout}"


def attn_site(case_index: int) -> int:
    """A site of the composed decoder's form 0x4000 + (l << 8) + k: layer l = case index, k = 1 (self) or 3 (cross)."""
    return 0x4000 + (case_index << 8) + (1 if ATTN_CASES[case_index][5] else 3)


def attn_inputs(case_index: int):
    """-> fp32 q (B, Sq, d) scaled by 2 (a softmax that is not flat), k, v (B, Sk, d), d_o (B, Sq, d)."""
    B, H, Sq, Sk, dh, causal, p, layout = ATTN_CASES[case_index]
    d = H * dh
    g = torch.Generator(device="cpu").manual_seed(7001 + case_index)
    q = torch.randn(B, Sq, d, generator=g) * 2
    k = torch.randn(B, Sk, d, generator=g)
    v = torch.randn(B, Sk, d, generator=g)
    d_o = torch.randn(B, Sq, d, generator=g)
    return q, k, v, d_o


def attn_mask(seed: int, site: int, B: int, H: int, Sq: int, Sk: int, p: float, row_stride: int = SA_ROW_STRIDE):
    """(B, H, Sq, Sk) fp64 keep-scale as small_attn_params keys it: layer site >> 8, site & 0xff, row (b * H + h) * 8 + i, column j."""
    if p <= 0:
        return None
    b, h, i = np.arange(B, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(Sq, dtype=np.int64)
    rows = (b[:, None, None] * H + h[None, :, None]) * row_stride + i[None, None, :]
    return dm.keep_scale(dm.site_key(seed, site >> 8, site & 0xFF), rows, np.arange(Sk, dtype=np.int64), p)


def small_attention(q, k, v, H: int, causal, mask=None, perturb=None):
    """o (B, Sq, d) = dropout(softmax(q k^T / sqrt(dh) [+ causal mask])) v per head; q (B, Sq, d), k, v (B, Sk, d), d = H * dh."""
    B, Sq, d = q.shape
    dh = d // H
    if perturb == "drop_last_key":
        k, v = k[:, :-1], v[:, :-1]
        mask = mask[..., :-1] if mask is not None else None
    Sk = k.shape[1]
    qh, kh, vh = [t.reshape(B, -1, H, dh).permute(0, 2, 1, 3) for t in (q, k, v)]
    s = qh @ kh.transpose(-1, -2) / math.sqrt(dh + 1 if perturb == "scale_dh_plus_1" else dh)
    if causal:
        i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
        s = s.masked_fill((j >= i) if perturb == "causal_off_by_one" else (j > i), -math.inf)
    m = mask.to(s.dtype) if mask is not None else None
    if perturb == "mask_before_norm" and m is not None:
        e = torch.exp(s - s.amax(-1, keepdim=True)) * m
        p = e / e.sum(-1, keepdim=True)
    else:
        p = torch.softmax(s, dim=-1)
        if m is not None:
            p = p * m
    p = torch.nan_to_num(p, nan=0.0)        # a perturbation can mask a whole row: its output is 0, not NaN
    return (p @ vh).permute(0, 2, 1, 3).reshape(B, Sq, d)


def small_attention_grads(q, k, v, d_o, H: int, causal, mask=None, perturb=None):
    """-> (o, dq, dk, dv) by autograd, in the dtype of the arguments."""
    q, k, v = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
    o = small_attention(q, k, v, H, causal, mask, perturb)
    o.backward(d_o)
    return o.detach(), q.grad, k.grad, v.grad


# ---- egx_linear_fwd / egx_linear_residual_fwd / egx_linear_bwd -----------------------------------------------------------------------------
LINEAR_FWD_SHAPES = [(1, 1, 1), (5, 7, 33), (130, 132, 68), (64, 256, 128), (257, 64, 2048)]
# (M, N, K): plain; not vectorisable; N * K = 266240 just over the 262144 atomic limit (slab path); exactly at it (atomic path); dx skinny over
# a reduction of 2304 (split-K with scratch, single pass without)
LINEAR_BWD_SHAPES = [(45, 96, 128), (300, 7, 33), (64, 520, 512), (64, 512, 512), (40, 2304, 256)]


def linear_inputs(M: int, N: int, K: int, salt: int = 0):
    """-> fp32 x (M, K), W (N, K), b (N,), residual (M, N), dy (M, N), dW0 (N, K), db0 (N,): all randn."""
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N * 3 + K + 1000 * salt)
    return (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g), torch.randn(M, N, generator=g),
            torch.randn(M, N, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g))


def linear(x, W, b=None, relu=False, residual=None):
    """-> (y, pre): y = [relu](x W^T + b) + residual; pre is the value the ReLU sees."""
    pre = x @ W.T
    if b is not None:
        pre = pre + b
    y = torch.relu(pre) if relu else pre
    if residual is not None:
        y = y + residual
    return y, pre


def linear_bwd(dy, x, W, dW0, db0, perturb=None):
    """-> (dx, dW, db): dx = dy W; dW = dW0 + dy^T x; db = db0 + colsum(dy) (the header's `+=` onto the buffers' contents dW0, db0)."""
    dW = dy.T @ x
    db = dy.sum(0)
    return dy @ W, (dW if perturb == "dw_assign" else dW0 + dW), (db if perturb == "db_assign" else db0 + db)


# ---- egx_gelu_fwd / _bwd -------------------------------------------------------------------------------------------------------------------
GELU_SIZES = [4, 1020, 1028, 4096 + 4]
GELU_PLANTED = [0.0, -0.0, 1e-30, -1e-30, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0]     # erf saturates, exp(-x^2 / 2) underflows


def gelu_inputs(n: int):
    """-> fp32 z = randn * 3 with the planted values in front (n = 4: four of them), dh = randn."""
    g = torch.Generator(device="cpu").manual_seed(9100 + n)
    z = torch.randn(n, generator=g) * 3
    planted = torch.tensor(GELU_PLANTED if n >= len(GELU_PLANTED) else [-0.0, 1e-30, -10.0, 40.0][:n])
    z[:planted.numel()] = planted
    return z, torch.randn(n, generator=g)


def gelu(z, perturb=None):
    if perturb == "tanh":
        return 0.5 * z * (1 + torch.tanh(math.sqrt(2 / math.pi) * (z + 0.044715 * z ** 3)))
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))


def gelu_bwd(z, dh, perturb=None):
    """dz = dh (Phi(z) + z phi(z)) written out (autograd of erf gives the same; this form has no 0 * inf at |z| = 40)."""
    if perturb == "tanh":
        z = z.detach().clone().requires_grad_(True)
        gelu(z, perturb).backward(dh)
        return z.grad
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    return dh * (cdf + z * pdf)


# ---- egx_relu_mask -------------------------------------------------------------------------------------------------------------------------
RELU_SIZES = [1, 255, 257, 70000]
RELU_PLANTED = [0.0, -0.0, 1e-40, -1e-40, math.nan, math.inf, -math.inf]           # 1e-40: a denormal, kept (> 0)


def relu_inputs(n: int):
    g = torch.Generator(device="cpu").manual_seed(9200 + n)
    y, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    planted = torch.tensor(RELU_PLANTED if n >= len(RELU_PLANTED) else [math.nan][:n])
    y[:planted.numel()] = planted
    return dy, y


def relu_mask(dy, y):
    """dy where y > 0, +0 elsewhere (y = NaN, -0, -inf included)."""
    return torch.where(y > 0, dy, torch.zeros_like(dy))


# ---- egx_dropout ---------------------------------------------------------------------------------------------------------------------------
DROPOUT_SHAPES = [(1, 1), (7, 3), (13, 130), (64, 1000)]
DROPOUT_PS = [0.0, 0.1, 0.5, 1.0]


def dropout_scale(rows: int, cols: int, p: float, seed: int, site: int, perturb=None):
    """(rows, cols) fp64 keep-scale of egx_dropout: key layer site >> 8, site & 0xff, row = row index, column = column."""
    s = dm.keep_scale(dm.site_key(seed, site >> 8, site & 0xFF), np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), p)
    return (s != 0).to(F64) if perturb == "scale_one" else s


def dropout(x, p: float, seed: int, site: int, perturb=None):
    """x * keep-scale rounded the way the kernel rounds it: the scale is an fp32 number, the product one fp32 multiplication."""
    s = dropout_scale(x.shape[0], x.shape[1], p, seed, site, perturb)
    return x * s.to(torch.float32).to(x.dtype)


# ---- egx_colsum_ordered --------------------------------------------------------------------------------------------------------------------
COLSUM_SHAPES = [(1, 1), (31, 64), (33, 65), (4096, 130), (70000, 8)]
COLSUM_BIG = 1.0e6


def colsum_inputs(M: int, N: int):
    """-> fp32 dy = randn * 1e3 with +BIG and -BIG on two neighbouring rows of every column (M >= 3), db0 = randn * 1e3: partial sums swing
    through BIG, so the order of the additions shows in the low bits."""
    g = torch.Generator(device="cpu").manual_seed(9300 + M + N)
    dy = torch.randn(M, N, generator=g) * 1e3
    db0 = torch.randn(N, generator=g) * 1e3
    if M >= 3:
        r = torch.randint(0, M - 1, (N,), generator=g)
        c = torch.arange(N)
        dy[r, c] += COLSUM_BIG
        dy[r + 1, c] -= COLSUM_BIG
    return dy, db0


def colsum(dy, db0):
    return db0 + dy.sum(0)


# ---- egx_pool_head_fwd / _bwd --------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 4), (5, 7, 128), (5, 33, 128), (3, 9, 64), (2, 5, 30), (2, 450, 128), (256, 3, 128), (257, 3, 128), (3, 17, 132),
               (2, 16, 130), (2, 128, 768), (1, 20, 1024)]
POOL_FORMS = {"none": (False, 0), "ln": (True, 0), "w1": (False, 1), "ln_w2": (True, 2), "ln_w64": (True, 64)}    # (LayerNorm, n_out; 0: no W)
POOL_EPS = 1e-5


def pool_inputs(B: int, S: int, d: int, form: str):
    """-> dict of fp32 tensors: tokens (B, S, d), ln_w, ln_b (d,) | None, W (n_out, d), b (n_out,) | None, d_out (B, n_out or d) and the
    prefill of the four parameter gradients."""
    ln, n_out = POOL_FORMS[form]
    g = torch.Generator(device="cpu").manual_seed(9400 + B * 131 + S * 17 + d + n_out)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {"tokens": r(B, S, d)}
    t["ln_w"], t["ln_b"] = (1 + 0.5 * r(d), 0.5 * r(d)) if ln else (None, None)
    t["W"], t["b"] = (r(n_out, d) / math.sqrt(d), r(n_out)) if n_out else (None, None)
    t["d_out"] = r(B, n_out if n_out else d)
    t["d_ln_w0"], t["d_ln_b0"] = (r(d), r(d)) if ln else (None, None)
    t["d_W0"], t["d_b0"] = (r(n_out, d), r(n_out)) if n_out else (None, None)
    return t


def pool_head(tokens, ln_w, ln_b, eps, W, b, perturb=None):
    """-> (pooled, out): pooled = mean_s tokens; y = LN(pooled) if ln_w is given; out = y W^T + b if W is given."""
    S, d = tokens.shape[1], tokens.shape[2]
    pooled = tokens.sum(1) / (S + 1 if perturb == "pool_divisor" else S)
    y = pooled
    if ln_w is not None:
        mean = y.mean(-1, keepdim=True)
        var = ((y - mean) ** 2).sum(-1, keepdim=True) / (d - 1 if perturb == "ln_var_dm1" else d)
        y = (y - mean) / torch.sqrt(var + eps) * ln_w + ln_b
    out = y
    if W is not None:
        out = y @ W.T
        if b is not None:
            out = out + b
    return pooled, out


def pool_head_grads(t: dict, dtype, perturb=None):
    """The inputs of pool_inputs in `dtype` -> dict: pooled, out, d_tokens and the four parameter gradients ADDED to their prefill."""
    c = {k: (v.to(dtype) if v is not None else None) for k, v in t.items()}
    leaves = {k: c[k].clone().requires_grad_(True) for k in ("tokens", "ln_w", "ln_b", "W", "b") if c[k] is not None}
    pooled, out = pool_head(leaves["tokens"], leaves.get("ln_w"), leaves.get("ln_b"), POOL_EPS, leaves.get("W"), leaves.get("b"), perturb)
    out.backward(c["d_out"])
    res = {"pooled": pooled.detach(), "out": out.detach(), "d_tokens": leaves["tokens"].grad}
    for k in ("ln_w", "ln_b", "W", "b"):
        res["d_" + k] = c["d_" + k + "0"] + leaves[k].grad if k in leaves else None
    return res
