"""The gate of tests/test_gpu_unit_ops.py tested on itself (CPU): each fp64 reference of tests/unit_ref.py agrees with the stock torch op,
evaluated in fp32 on the GPU test's inputs it meets the GPU test's bar, and with one deliberate mistake it misses that bar at least 3x."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dropmask as dm
from tests import unit_ref as ur

F64, F32 = torch.float64, torch.float32


def _attn_mask(ci, row_stride=ur.SA_ROW_STRIDE):
    B, H, Sq, Sk, dh, causal, p, _ = ur.ATTN_CASES[ci]
    return ur.attn_mask(ur.ATTN_SEED, ur.attn_site(ci), B, H, Sq, Sk, p, row_stride)


def _attn_eval(ci, dtype, perturb=None):
    """-> (o, (dq, dk, dv)) of case ci in `dtype`."""
    B, H, Sq, Sk, dh, causal, p, _ = ur.ATTN_CASES[ci]
    q, k, v, d_o = [t.to(dtype) for t in ur.attn_inputs(ci)]
    mask = _attn_mask(ci, 64 if perturb == "mask_row_stride_64" else ur.SA_ROW_STRIDE)
    o, dq, dk, dv = ur.small_attention_grads(q, k, v, d_o, H, causal, mask, None if perturb == "mask_row_stride_64" else perturb)
    return o, (dq, dk, dv)


_ATTN_REF = {}


def _attn_ref(ci):
    if ci not in _ATTN_REF:
        _ATTN_REF[ci] = _attn_eval(ci, F64)
    return _ATTN_REF[ci]


def _attn_errs(ci, dtype, perturb=None):
    o, grads = _attn_eval(ci, dtype, perturb)
    ro, rgrads = _attn_ref(ci)
    return ur.rel_err(o, ro), max(ur.rel_err(g, r) for g, r in zip(grads, rgrads))


# ---- the references against the stock ops ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(ur.ATTN_CASES)), ids=[ur.attn_case_id(c) for c in ur.ATTN_CASES])
def test_attention_reference_is_sdpa(ci):
    """F.scaled_dot_product_attention's arithmetic written out: softmax(q k^T / sqrt(dh) + causal mask), dropout as a keep-scale on the
    probabilities, times v; forward and, by autograd of both, backward."""
    B, H, Sq, Sk, dh, causal, p, _ = ur.ATTN_CASES[ci]
    q, k, v, d_o = [t.double() for t in ur.attn_inputs(ci)]
    mask = _attn_mask(ci)
    o, grads = _attn_ref(ci)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = [t.reshape(B, -1, H, dh).transpose(1, 2) for t in leaves]
    if mask is None:
        so = F.scaled_dot_product_attention(qh, kh, vh, is_causal=bool(causal))
    else:       # the stock op draws its own mask: its arithmetic with ours (attn_weight = dropout(softmax(q k^T * scale + bias)); weight @ v)
        bias = torch.zeros(Sq, Sk, dtype=F64)
        if causal:
            bias.masked_fill_(torch.ones(Sq, Sk, dtype=torch.bool).tril().logical_not(), -math.inf)
        so = (torch.softmax(qh @ kh.transpose(-2, -1) * (1 / math.sqrt(dh)) + bias, -1) * mask) @ vh
    so = so.transpose(1, 2).reshape(B, Sq, H * dh)
    so.backward(d_o)
    assert ur.max_err(o, so) <= 1e-12
    for g, leaf in zip(grads, leaves):
        assert ur.max_err(g, leaf.grad) <= 1e-12 * max(1.0, leaf.grad.abs().max().item())


def test_other_references_are_the_stock_ops():
    for n in ur.GELU_SIZES:
        z, dh = [t.double() for t in ur.gelu_inputs(n)]
        zz = z.clone().requires_grad_(True)
        h = F.gelu(zz)
        h.backward(dh)
        assert ur.max_err(ur.gelu(z), h) <= 1e-12 and ur.max_err(ur.gelu_bwd(z, dh), zz.grad) <= 1e-12
    for (B, S, d) in ur.POOL_SHAPES:
        for form in ur.POOL_FORMS:
            t = {k: (v.double() if v is not None else None) for k, v in ur.pool_inputs(B, S, d, form).items()}
            pooled, out = ur.pool_head(t["tokens"], t["ln_w"], t["ln_b"], ur.POOL_EPS, t["W"], t["b"])
            y = t["tokens"].mean(1)
            assert ur.max_err(pooled, y) <= 1e-12
            if t["ln_w"] is not None:
                y = F.layer_norm(y, (d,), t["ln_w"], t["ln_b"], ur.POOL_EPS)
            if t["W"] is not None:
                y = F.linear(y, t["W"], t["b"])
            assert ur.max_err(out, y) <= 1e-12 * max(1.0, y.abs().max().item())
    for (M, N, K) in ur.LINEAR_FWD_SHAPES + ur.LINEAR_BWD_SHAPES:
        x, W, b, res, dy, dW0, db0 = [t.double() for t in ur.linear_inputs(M, N, K)]
        scale = 1e-12 * max(1.0, math.sqrt(K) * 10)
        assert ur.max_err(ur.linear(x, W, b)[0], F.linear(x, W, b)) <= scale
        assert ur.max_err(ur.linear(x, W, b, relu=True, residual=res)[0], F.relu(F.linear(x, W, b)) + res) <= scale
        xx, WW, bb = [t.clone().requires_grad_(True) for t in (x, W, b)]
        F.linear(xx, WW, bb).backward(dy)
        dx, dW, db = ur.linear_bwd(dy, x, W, dW0, db0)
        assert ur.max_err(dx, xx.grad) <= 1e-12 * max(1.0, math.sqrt(N) * 10)
        assert ur.max_err(dW - dW0, WW.grad) <= 1e-12 * max(1.0, math.sqrt(M) * 10)
        assert ur.max_err(db - db0, bb.grad) <= 1e-12 * max(1.0, math.sqrt(M) * 10)
    for (M, N) in ur.COLSUM_SHAPES:
        dy, db0 = [t.double() for t in ur.colsum_inputs(M, N)]
        assert ur.max_err(ur.colsum(dy, db0) - db0, dy.sum(0)) <= 1e-12 * ur.COLSUM_BIG
    for n in ur.RELU_SIZES:
        dy, y = ur.relu_inputs(n)
        yy = torch.nan_to_num(y, nan=-1.0).double().requires_grad_(True)
        torch.relu(yy).backward(dy.double())
        assert torch.equal(ur.relu_mask(dy, y).double(), yy.grad)
        assert not torch.signbit(ur.relu_mask(dy, y)[~(y > 0)]).any()


# ---- the fp32 yardstick and the bars -------------------------------------------------------------------------------------------------------
def _fp32_errs():
    """op -> kind -> worst rel_err of the fp32 evaluation over the operator's cases."""
    e = {"small_attention": {"out": 0.0, "grad": 0.0}, "gelu": {"out": 0.0, "grad": 0.0}, "pool_head": {"out": 0.0, "grad": 0.0},
         "colsum": {"out": 0.0}}
    for ci in range(len(ur.ATTN_CASES)):
        eo, eg = _attn_errs(ci, F32)
        e["small_attention"]["out"] = max(e["small_attention"]["out"], eo)
        e["small_attention"]["grad"] = max(e["small_attention"]["grad"], eg)
    for n in ur.GELU_SIZES:
        z, dh = ur.gelu_inputs(n)
        e["gelu"]["out"] = max(e["gelu"]["out"], ur.rel_err(ur.gelu(z), ur.gelu(z.double())))
        e["gelu"]["grad"] = max(e["gelu"]["grad"], ur.rel_err(ur.gelu_bwd(z, dh), ur.gelu_bwd(z.double(), dh.double())))
    for (B, S, d) in ur.POOL_SHAPES:
        for form in ur.POOL_FORMS:
            eo, eg = _pool_errs(B, S, d, form, F32)
            e["pool_head"]["out"] = max(e["pool_head"]["out"], eo)
            e["pool_head"]["grad"] = max(e["pool_head"]["grad"], eg)
    for (M, N) in ur.COLSUM_SHAPES:
        dy, db0 = ur.colsum_inputs(M, N)
        e["colsum"]["out"] = max(e["colsum"]["out"], ur.rel_err(ur.colsum(dy, db0), ur.colsum(dy.double(), db0.double())))
    return e


_POOL_REF = {}


def _pool_errs(B, S, d, form, dtype, perturb=None):
    t = ur.pool_inputs(B, S, d, form)
    key = (B, S, d, form)
    if key not in _POOL_REF:
        _POOL_REF[key] = ur.pool_head_grads(t, F64)
    ref, got = _POOL_REF[key], ur.pool_head_grads(t, dtype, perturb)
    eo = max(ur.rel_err(got[k], ref[k]) for k in ("pooled", "out"))
    eg = max(ur.rel_err(got[k], ref[k]) for k in ("d_tokens", "d_ln_w", "d_ln_b", "d_W", "d_b") if ref[k] is not None)
    return eo, eg


def test_fp32_reference_meets_the_bar():
    """Each reference in fp32 on the GPU test's inputs is inside the GPU test's bar, and the recorded FP32_ERR are what this measures."""
    meas = _fp32_errs()
    for op, kinds in meas.items():
        for kind, e in kinds.items():
            rec, bar = ur.FP32_ERR[op][kind], ur.BAR[op][kind]
            print(f"fp32 yardstick {op:16s} {kind:4s} measured {e:.3e} recorded {rec:.3e} bar {bar:.3e}")
            assert bar == ur.FACTOR * rec
            assert e <= bar, f"{op} {kind}: the fp32 reference misses its own bar ({e} > {bar})"
            assert rec / 3 <= e <= rec * 3, f"{op} {kind}: recorded fp32 error {rec} is not the measured {e}"
    # the GEMM-backed operators at test_gemm's bars
    for (M, N, K) in ur.LINEAR_FWD_SHAPES + ur.LINEAR_BWD_SHAPES:
        x, W, b, res, dy, dW0, db0 = ur.linear_inputs(M, N, K)
        y64 = ur.linear(x.double(), W.double(), b.double(), True, res.double())[0]
        assert ur.max_err(ur.linear(x, W, b, True, res)[0], y64) <= ur.gemm_bar(0, K)
        got, ref = ur.linear_bwd(dy, x, W, dW0, db0), ur.linear_bwd(*[t.double() for t in (dy, x, W, dW0, db0)])
        for g, r, red in zip(got, ref, (N, M, M)):
            assert ur.max_err(g, r) <= ur.gemm_bar(0, red)


# ---- the perturbed references --------------------------------------------------------------------------------------------------------------
def _record(op, name, ratio):
    print(f"perturbation {op:16s} {name:20s} worst error / bar = {ratio:.3g} (recorded {ur.PERTURB_RATIO[op][name]:.3g})")
    assert ratio >= 3, f"{op} / {name}: the bar lets the perturbed reference through (error / bar = {ratio})"
    assert ratio >= ur.PERTURB_RATIO[op][name] / 2, f"{op} / {name}: recorded ratio {ur.PERTURB_RATIO[op][name]} is not the measured {ratio}"


_ATTN_APPLIES = {        # the cases a mistake can show in
    "causal_off_by_one": lambda c: c[5] == 1,
    "scale_dh_plus_1": lambda c: c[3] > 1,
    "mask_row_stride_64": lambda c: c[6] > 0,
    "mask_before_norm": lambda c: c[6] > 0,
    "drop_last_key": lambda c: c[3] > 1,
}


@pytest.mark.parametrize("name", sorted(_ATTN_APPLIES))
def test_perturbed_attention_misses_the_bar(name):
    """In fp32 (the bars must reject the mistake on top of fp32 rounding), outputs and gradients each, on every case the mistake applies to."""
    worst = math.inf
    for ci, case in enumerate(ur.ATTN_CASES):
        if not _ATTN_APPLIES[name](case):
            continue
        if name == "mask_row_stride_64" and case[0] * case[1] == 1:
            continue                    # one (clip, head): block 0's rows are i at either stride
        eo, eg = _attn_errs(ci, F32, name)
        worst = min(worst, eo / ur.BAR["small_attention"]["out"], eg / ur.BAR["small_attention"]["grad"])
    _record("small_attention", name, worst)


def test_perturbed_linear_bwd_misses_the_bar():
    for name, idx in (("dw_assign", 1), ("db_assign", 2)):
        worst = math.inf
        for (M, N, K) in ur.LINEAR_BWD_SHAPES:
            dy, x, W, dW0, db0 = [ur.linear_inputs(M, N, K)[i] for i in (4, 0, 1, 5, 6)]
            got = ur.linear_bwd(dy, x, W, dW0, db0, name)[idx]
            ref = ur.linear_bwd(*[t.double() for t in (dy, x, W, dW0, db0)])[idx]
            worst = min(worst, ur.max_err(got, ref) / ur.gemm_bar(0, M))     # the f32 bar; bf16's own rounding is the looser bar's reason
        _record("linear_bwd", name, worst)


def test_perturbed_pool_head_misses_the_bar():
    """pool_divisor shows in pooled_saved everywhere, in the gradients only without LayerNorm (LN is scale-invariant up to eps, and its rstd
    undoes the divisor in d_tokens); ln_var_dm1 shows wherever there is a LayerNorm."""
    worst = {"pool_divisor": math.inf, "ln_var_dm1": math.inf}
    for (B, S, d) in ur.POOL_SHAPES:
        for form, (ln, n_out) in ur.POOL_FORMS.items():
            eo, eg = _pool_errs(B, S, d, form, F32, "pool_divisor")
            worst["pool_divisor"] = min(worst["pool_divisor"], eo / ur.BAR["pool_head"]["out"])
            if not ln:
                worst["pool_divisor"] = min(worst["pool_divisor"], eg / ur.BAR["pool_head"]["grad"])
            if ln:
                eo, eg = _pool_errs(B, S, d, form, F32, "ln_var_dm1")
                worst["ln_var_dm1"] = min(worst["ln_var_dm1"], eo / ur.BAR["pool_head"]["out"], eg / ur.BAR["pool_head"]["grad"])
    for name, w in worst.items():
        _record("pool_head", name, w)


def test_perturbed_gelu_and_dropout_miss():
    worst = math.inf
    for n in ur.GELU_SIZES:
        z, dh = ur.gelu_inputs(n)
        if n < len(ur.GELU_PLANTED):
            continue            # four planted values alone: the tanh form is exact at 0 and where both forms saturate
        worst = min(worst, ur.rel_err(ur.gelu(z, "tanh"), ur.gelu(z.double())) / ur.BAR["gelu"]["out"],
                    ur.rel_err(ur.gelu_bwd(z, dh, "tanh"), ur.gelu_bwd(z.double(), dh.double())) / ur.BAR["gelu"]["grad"])
    _record("gelu", "tanh", worst)
    # egx_dropout is compared bit for bit: the "bar" is one differing element. Ratio = kept elements whose bits differ / 1, over the cases with 0 < p < 1.
    worst = math.inf
    for (rows, cols) in ur.DROPOUT_SHAPES[2:]:
        for p in (0.1, 0.5):
            x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols))
            good, bad = ur.dropout(x, p, 77, 0x4102), ur.dropout(x, p, 77, 0x4102, "scale_one")
            worst = min(worst, float((good.view(torch.int32) != bad.view(torch.int32)).sum()))
    _record("dropout", "scale_one", worst)


# ---- the dropout generator itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_dropout_kept_fraction(p):
    rows, cols = 64, 1000
    s = ur.dropout_scale(rows, cols, p, seed=0xABCDEF, site=0x4102)
    n = rows * cols
    kept = (s != 0).double().mean().item()
    thresh = dm.drop_threshold(p)
    assert abs(kept - (1 - thresh / 65536)) <= 5 * math.sqrt(p * (1 - p) / n)
    assert torch.equal(s[s != 0], torch.full_like(s[s != 0], dm.inv_keep(p)))          # exact: the fp32 1 / (1 - p)
    assert np.float32(dm.inv_keep(p)) == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    x = torch.ones(rows, cols)
    assert torch.equal(ur.dropout(x, p, 0xABCDEF, 0x4102).double(), s.float().double())
    # another site, another seed: another mask
    assert not torch.equal(s, ur.dropout_scale(rows, cols, p, seed=0xABCDEF, site=0x4104))
    assert not torch.equal(s, ur.dropout_scale(rows, cols, p, seed=0xABCDF0, site=0x4102))
