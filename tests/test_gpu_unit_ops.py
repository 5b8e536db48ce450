"""The unit operators of the C ABI at their edge shapes (-m gpu): each against its fp64 reference of tests/unit_ref.py, at that module's bars.

Buffers an operator overwrites start as NaN, buffers it adds into start as random values, strided operands live in larger NaN-filled
buffers whose every element outside the addressed window must still be NaN afterwards. Each test prints its figures (lines "UNITOPS ...")
before it asserts.

Not here: the deterministic mode of egx_linear_bwd, egx_colsum_ordered and egx_pool_head_bwd. That mode is egx_config.deterministic: only the
encoder / translator entry points, which carry a config, open its scope (DetScope, csrc/norm.hip), so a unit operator called on its own never
runs its deterministic branch. Those branches stay with the whole-model deterministic tests. Likewise egx_colsum_ordered's "row blocks grow to
fit a smaller scratch" branch: the entry point refuses a scratch below its query (tested), only internal callers reach the branch."""
import pytest
import torch

from tests import unit_ref as ur

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 32          # floats behind every buffer
SENTINEL = 12345.0  # guard value of buffers that are updated in place (NaN would survive a stray `*=`)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(lib, rc):
    assert rc == 0, lib.egx_last_error().decode()


def _refused(lib, rc):
    assert rc != 0 and lib.egx_last_error().decode(), "the call was not refused with a message"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _report(op, what, err, bar):
    print(f"UNITOPS {op} {what} err {err:.3e} bar {bar:.3e}")


def _nanbuf(n, cuda):
    return torch.full((n + GUARD,), NAN, device=cuda)


def _dev(t, cuda, guard=NAN):
    """A contiguous host tensor on the device with GUARD floats of `guard` behind it -> (flat buffer, view of the tensor's shape)."""
    buf = torch.full((t.numel() + GUARD,), guard, device=cuda)
    buf[:t.numel()] = t.reshape(-1).to(cuda)
    return buf, buf[:t.numel()].view(t.shape)


def _win(buf, off, rows, ld, cols):
    return buf.as_strided((rows, cols), (ld, 1), off)


def _outside_is_nan(buf, windows):
    seen = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    for w in windows:
        _win(seen, *w).fill_(True)
    return bool(torch.isnan(buf[~seen]).all())


# ---- egx_small_attention_fwd / _bwd --------------------------------------------------------------------------------------------------------
def _attn_layout(layout, d):
    """operand -> (buffer, offset, row stride)"""
    if layout == "packed":
        return {"q": ("Q", 0, d), "k": ("K", 0, d), "v": ("V", 0, d), "o": ("O", 0, d)}
    if layout == "self":
        return {"q": ("QKV", 0, 3 * d), "k": ("QKV", d, 3 * d), "v": ("QKV", 2 * d, 3 * d), "o": ("O", 0, d)}
    if layout in ("cross", "cross_ldo4"):
        return {"q": ("Q", 0, d), "k": ("KV", 0, 2 * d), "v": ("KV", d, 2 * d), "o": ("O", 0, d + 4 if layout == "cross_ldo4" else d)}
    if layout == "odd":
        return {"q": ("Q", 0, d + 1), "k": ("K", 0, d + 1), "v": ("V", 0, d + 1), "o": ("O", 0, d + 1)}
    raise ValueError(layout)


@pytest.mark.parametrize("ci", range(len(ur.ATTN_CASES)), ids=[ur.attn_case_id(c) for c in ur.ATTN_CASES])
def test_small_attention_fwd_bwd(egx_lib, cuda, ci):
    B, H, Sq, Sk, dh, causal, p, layout = ur.ATTN_CASES[ci]
    d, seed, site = H * dh, ur.ATTN_SEED, ur.attn_site(ci)
    host = dict(zip(("q", "k", "v", "o"), ur.attn_inputs(ci)))          # "o": d_o, which shares o's geometry
    mask = ur.attn_mask(seed, site, B, H, Sq, Sk, p)
    ro, rdq, rdk, rdv = ur.small_attention_grads(host["q"].double(), host["k"].double(), host["v"].double(), host["o"].double(), H, causal, mask)
    lay = _attn_layout(layout, d)
    rows = {"q": B * Sq, "k": B * Sk, "v": B * Sk, "o": B * Sq}
    win = {n: (lay[n][1], rows[n], lay[n][2], d) for n in lay}          # operand -> (offset, rows, ld, cols) inside its buffer
    size = {}
    for n, (bname, off, ld) in lay.items():
        size[bname] = max(size.get(bname, 0), rows[n] * ld)
    inp = {b: _nanbuf(s, cuda) for b, s in size.items()}                # q, k, v and d_o: NaN wherever no operand lives
    out = {b: _nanbuf(s, cuda) for b, s in size.items()}                # o and dq, dk, dv: the same geometry, all NaN
    for n in lay:
        _win(inp[lay[n][0]], *win[n]).copy_(host[n].reshape(rows[n], d).to(cuda))
    before = {b: t.clone() for b, t in inp.items()}

    def addr(bufs, n):
        return bufs[lay[n][0]].data_ptr() + 4 * lay[n][1]

    ld = {n: lay[n][2] for n in lay}
    _check(egx_lib, egx_lib.egx_small_attention_fwd(addr(inp, "q"), ld["q"], addr(inp, "k"), ld["k"], addr(inp, "v"), ld["v"], addr(out, "o"),
                                                    ld["o"], B, Sq, Sk, H, dh, causal, p, seed, site, _stream()))
    _check(egx_lib, egx_lib.egx_small_attention_bwd(addr(inp, "q"), ld["q"], addr(inp, "k"), ld["k"], addr(inp, "v"), ld["v"], addr(inp, "o"),
                                                    ld["o"], addr(out, "q"), addr(out, "k"), addr(out, "v"), B, Sq, Sk, H, dh, causal, p, seed,
                                                    site, _stream()))
    torch.cuda.synchronize()
    got = {n: _win(out[lay[n][0]], *win[n]).cpu() for n in lay}
    eo = ur.rel_err(got["o"], ro.reshape(B * Sq, d))
    eg = {n: ur.rel_err(got[n], r.reshape(rows[n], d)) for n, r in (("q", rdq), ("k", rdk), ("v", rdv))}
    case = ur.attn_case_id(ur.ATTN_CASES[ci])
    _report("small_attention", f"{case} o", eo, ur.BAR["small_attention"]["out"])
    for n, e in eg.items():
        _report("small_attention", f"{case} d{n}", e, ur.BAR["small_attention"]["grad"])
    assert eo <= ur.BAR["small_attention"]["out"]
    assert max(eg.values()) <= ur.BAR["small_attention"]["grad"], eg
    # exactly once, and nowhere else: every element outside the addressed (row, head column) windows is still NaN
    for b in out:
        assert _outside_is_nan(out[b], [win[n] for n in lay if lay[n][0] == b]), f"buffer {b} was written outside its windows"
    for b in inp:
        assert _same_bits(inp[b], before[b]), f"input buffer {b} changed"


def test_small_attention_refusals(egx_lib, cuda):
    B, H, dh = 1, 2, 32
    big = torch.zeros(1025 * 2 * 129 + GUARD, device=cuda)
    o = _nanbuf(9 * 2 * 129, cuda)
    dq, dk, dv = [_nanbuf(1025 * 2 * 129, cuda) for _ in range(3)]

    def call(Sq=4, Sk=4, dh=dh, causal=0, q=big, k=big, v=big, out=o):
        d = H * dh
        r1 = egx_lib.egx_small_attention_fwd(_ptr(q), d, _ptr(k), d, _ptr(v), d, _ptr(out), d, B, Sq, Sk, H, dh, causal, 0.0, 1, 0x4003, _stream())
        _refused(egx_lib, r1)
        r2 = egx_lib.egx_small_attention_bwd(_ptr(q), d, _ptr(k), d, _ptr(v), d, _ptr(big), d, _ptr(dq), _ptr(dk), _ptr(dv), B, Sq, Sk, H, dh,
                                             causal, 0.0, 1, 0x4003, _stream())
        _refused(egx_lib, r2)

    call(Sq=9, Sk=16)
    call(Sk=1025)
    call(dh=129)
    call(Sq=4, Sk=5, causal=1)
    call(q=None)
    call(k=None)
    call(v=None)
    _refused(egx_lib, egx_lib.egx_small_attention_fwd(_ptr(big), 64, _ptr(big), 64, _ptr(big), 64, None, 64, B, 4, 4, H, dh, 0, 0.0, 1, 0x4003, _stream()))
    _refused(egx_lib, egx_lib.egx_small_attention_bwd(_ptr(big), 64, _ptr(big), 64, _ptr(big), 64, _ptr(big), 64, None, _ptr(dk), _ptr(dv), B, 4, 4, H,
                                                      dh, 0, 0.0, 1, 0x4003, _stream()))
    torch.cuda.synchronize()
    for t in (o, dq, dk, dv):
        assert torch.isnan(t).all()


# ---- egx_linear_fwd / egx_linear_residual_fwd ----------------------------------------------------------------------------------------------
COMPUTE = [(0, "f32"), (1, "bf16"), (2, "f32s")]      # gemm() takes every mode: bf16 has MFMA bf16 operands, f32 and f32s its fp32 path


@pytest.mark.parametrize("compute,cname", COMPUTE, ids=[c[1] for c in COMPUTE])
@pytest.mark.parametrize("M,N,K", ur.LINEAR_FWD_SHAPES)
def test_linear_fwd(egx_lib, cuda, compute, cname, M, N, K):
    x, W, b, res, *_ = ur.linear_inputs(M, N, K)
    xd, Wd, bd, rd = [t.to(cuda) for t in (x, W, b, res)]
    bar = ur.gemm_bar(compute, K)
    worst = 0.0
    for bias in (True, False):
        for relu in (True, False):
            ybuf = _nanbuf(M * N, cuda)
            _check(egx_lib, egx_lib.egx_linear_fwd(_ptr(xd), _ptr(Wd), _ptr(bd) if bias else None, _ptr(ybuf), M, N, K, int(relu), compute, _stream()))
            torch.cuda.synchronize()
            ref, pre = ur.linear(x.double(), W.double(), b.double() if bias else None, relu)
            got = ybuf[:M * N].view(M, N).cpu()
            err = ur.max_err(got, ref)
            worst = max(worst, err)
            assert err <= bar, f"bias={bias} relu={relu}: max err {err} (bar {bar})"
            assert torch.isnan(ybuf[M * N:]).all()
            if relu:
                assert (got[pre < -bar] == 0).all() and (got >= 0).all()
        ybuf = _nanbuf(M * N, cuda)
        _check(egx_lib, egx_lib.egx_linear_residual_fwd(_ptr(xd), _ptr(Wd), _ptr(bd) if bias else None, _ptr(rd), _ptr(ybuf), M, N, K, compute,
                                                        _stream()))
        torch.cuda.synchronize()
        ref, _ = ur.linear(x.double(), W.double(), b.double() if bias else None, False, res.double())
        err = ur.max_err(ybuf[:M * N].view(M, N).cpu(), ref)
        worst = max(worst, err)
        assert err <= bar, f"residual, bias={bias}: max err {err} (bar {bar})"
        assert torch.isnan(ybuf[M * N:]).all()
    _report(f"linear_fwd[{cname}]", f"M{M}N{N}K{K} y", worst, bar)
    _refused(egx_lib, egx_lib.egx_linear_residual_fwd(_ptr(xd), _ptr(Wd), _ptr(bd), None, _ptr(ybuf), M, N, K, compute, _stream()))


# ---- egx_linear_bwd ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compute,cname", COMPUTE, ids=[c[1] for c in COMPUTE])
@pytest.mark.parametrize("M,N,K", ur.LINEAR_BWD_SHAPES)
def test_linear_bwd(egx_lib, cuda, compute, cname, M, N, K):
    """dx = (NaN before), dW += and db += (random before): all three, each output NULL in turn, and dx alone without scratch (the single-pass
    kernel where the scratch would have let a skinny dx split its reduction). dx, and dW above the atomic limit (N * K > 262144: slabs summed
    in slab order), have one writer per element: their bits repeat."""
    x, W, b, res, dy, dW0, db0 = ur.linear_inputs(M, N, K)
    xd, Wd, dyd = [t.to(cuda) for t in (x, W, dy)]
    rdx, rdW, rdb = ur.linear_bwd(dy.double(), x.double(), W.double(), dW0.double(), db0.double())
    rdW, rdb = rdW - dW0.double(), rdb - db0.double()           # what the call must ADD
    nbytes = egx_lib.egx_linear_bwd_scratch(M, N, K)
    scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=cuda)
    bars = {"dx": ur.gemm_bar(compute, N), "dW": ur.gemm_bar(compute, M), "db": ur.gemm_bar(compute, M)}
    worst = {"dx": 0.0, "dW": 0.0, "db": 0.0}
    kept = {}

    def run(tag, want_dx=True, want_dW=True, want_db=True, with_scratch=True):
        dxb = _nanbuf(M * K, cuda)
        dWb, dWv = _dev(dW0, cuda, SENTINEL)
        dbb, dbv = _dev(db0, cuda, SENTINEL)
        _check(egx_lib, egx_lib.egx_linear_bwd(_ptr(dyd), _ptr(xd), _ptr(Wd), _ptr(dxb) if want_dx else None, _ptr(dWb) if want_dW else None,
                                               _ptr(dbb) if want_db else None, M, N, K, compute, _ptr(scratch) if with_scratch else None,
                                               _stream()))
        torch.cuda.synchronize()
        dx = dxb[:M * K].view(M, K)
        if want_dx:
            e = ur.max_err(dx.cpu(), rdx)
            worst["dx"] = max(worst["dx"], e)
            assert e <= bars["dx"], f"{tag}: dx max err {e} (bar {bars['dx']})"
        else:
            assert torch.isnan(dxb).all()
        for name, view, pre, ref, want in (("dW", dWv, dW0, rdW, want_dW), ("db", dbv, db0, rdb, want_db)):
            if want:
                e = ur.max_err(view.cpu().double() - pre.double(), ref)
                worst[name] = max(worst[name], e)
                assert e <= bars[name], f"{tag}: {name} - prefill max err {e} (bar {bars[name]})"
            else:
                assert _same_bits(view.cpu(), pre), f"{tag}: {name} was NULL in the call and its buffer changed"
        assert torch.isnan(dxb[M * K:]).all() and (dWb[N * K:] == SENTINEL).all() and (dbb[N:] == SENTINEL).all()
        kept[tag] = (dx.clone(), dWv.clone())

    run("all")
    run("again")
    assert _same_bits(kept["all"][0], kept["again"][0]), "dx differs between two runs"
    if N * K > 262144:
        assert _same_bits(kept["all"][1], kept["again"][1]), "dW through the slabs differs between two runs"
    run("no dx", want_dx=False)
    run("no dW", want_dW=False)
    run("no db", want_db=False)
    run("dx alone, no scratch", want_dW=False, want_db=False, with_scratch=False)
    for name in worst:
        _report(f"linear_bwd[{cname}]", f"M{M}N{N}K{K} {name}", worst[name], bars[name])
    # dW without scratch (or without x) is refused and leaves dW alone
    dWb, dWv = _dev(dW0, cuda, SENTINEL)
    _refused(egx_lib, egx_lib.egx_linear_bwd(_ptr(dyd), _ptr(xd), _ptr(Wd), None, _ptr(dWb), None, M, N, K, compute, None, _stream()))
    _refused(egx_lib, egx_lib.egx_linear_bwd(_ptr(dyd), None, _ptr(Wd), None, _ptr(dWb), None, M, N, K, compute, _ptr(scratch), _stream()))
    torch.cuda.synchronize()
    assert _same_bits(dWv.cpu(), dW0)


# ---- egx_gelu_fwd / _bwd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ur.GELU_SIZES)
def test_gelu_fwd_bwd(egx_lib, cuda, n):
    from egot2_amd import functional as Fn
    z, dh = ur.gelu_inputs(n)
    zd, dhd = z.to(cuda), dh.to(cuda)
    hb, dzb = _nanbuf(n, cuda), _nanbuf(n, cuda)
    _check(egx_lib, egx_lib.egx_gelu_fwd(_ptr(zd), _ptr(hb), n, _stream()))
    _check(egx_lib, egx_lib.egx_gelu_bwd(_ptr(zd), _ptr(dhd), _ptr(dzb), n, _stream()))
    torch.cuda.synchronize()
    h, dz = hb[:n].cpu(), dzb[:n].cpu()
    assert torch.isfinite(h).all() and torch.isfinite(dz).all()
    assert torch.isnan(hb[n:]).all() and torch.isnan(dzb[n:]).all()
    eo, eg = ur.rel_err(h, ur.gelu(z.double())), ur.rel_err(dz, ur.gelu_bwd(z.double(), dh.double()))
    _report("gelu", f"n{n} h", eo, ur.BAR["gelu"]["out"])
    _report("gelu", f"n{n} dz", eg, ur.BAR["gelu"]["grad"])
    assert eo <= ur.BAR["gelu"]["out"] and eg <= ur.BAR["gelu"]["grad"]
    # the autograd bridge makes the same two calls
    zz = zd.clone().requires_grad_(True)
    hh = Fn.gelu(zz)
    hh.backward(dhd)
    assert _same_bits(hh.detach().cpu(), h) and _same_bits(zz.grad.cpu(), dz)


def test_gelu_refuses_n_not_multiple_of_4(egx_lib, cuda):
    z = torch.randn(8, device=cuda)
    hb = _nanbuf(8, cuda)
    _refused(egx_lib, egx_lib.egx_gelu_fwd(_ptr(z), _ptr(hb), 6, _stream()))
    _refused(egx_lib, egx_lib.egx_gelu_bwd(_ptr(z), _ptr(z), _ptr(hb), 6, _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(hb).all()


# ---- egx_relu_mask -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ur.RELU_SIZES)
def test_relu_mask(egx_lib, cuda, n):
    dy, y = ur.relu_inputs(n)
    dyb, dyv = _dev(dy, cuda, SENTINEL)
    yd = y.to(cuda)
    _check(egx_lib, egx_lib.egx_relu_mask(_ptr(dyb), _ptr(yd), n, _stream()))
    torch.cuda.synchronize()
    assert _same_bits(dyv.cpu(), ur.relu_mask(dy, y)), "dy is kept exactly where y > 0 and is +0 elsewhere (y = NaN included)"
    assert (dyb[n:] == SENTINEL).all()
    # n = 0 touches nothing
    dyb, dyv = _dev(dy, cuda, SENTINEL)
    _check(egx_lib, egx_lib.egx_relu_mask(_ptr(dyb), _ptr(yd), 0, _stream()))
    torch.cuda.synchronize()
    assert _same_bits(dyv.cpu(), dy) and (dyb[n:] == SENTINEL).all()


# ---- egx_dropout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", ur.DROPOUT_PS)
@pytest.mark.parametrize("rows,cols", ur.DROPOUT_SHAPES)
def test_dropout(egx_lib, cuda, rows, cols, p):
    seed, site = 0x1234ABCD5678, 0x4102
    x = torch.randn(rows, cols, generator=torch.Generator(device="cpu").manual_seed(rows * 1000 + cols))

    def apply(t, seed=seed, site=site, times=1):
        buf, view = _dev(t, cuda, SENTINEL)
        for _ in range(times):
            _check(egx_lib, egx_lib.egx_dropout(_ptr(buf), rows, cols, p, seed, site, _stream()))
        torch.cuda.synchronize()
        assert (buf[rows * cols:] == SENTINEL).all()
        return view.cpu()

    once = apply(x)
    ref = ur.dropout(x, p, seed, site)
    assert _same_bits(once, ref), f"{(~(_bits(once) == _bits(ref))).sum().item()} of {rows * cols} elements differ in their bits"
    if p == 0.0:
        assert _same_bits(once, x)
    if p == 1.0:
        assert (once == 0).all()
    # the same key applies the same mask: the zeros coincide, the kept values are scaled twice
    assert _same_bits(apply(x, times=2), ur.dropout(ref, p, seed, site))
    if 0.0 < p < 1.0 and rows * cols >= 1000:
        assert not torch.equal(apply(x, site=0x4104) == 0, once == 0), "another site, the same mask"
        assert not torch.equal(apply(x, seed=seed + 1) == 0, once == 0), "another seed, the same mask"


# ---- egx_colsum_ordered --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", ur.COLSUM_SHAPES)
def test_colsum_ordered(egx_lib, cuda, M, N):
    """db += colsum(dy) with the queried scratch (three runs, the same bits), with a scratch of exactly two partial rows and with none (both
    accepted only where they cover the query) and with one float less than the query (refused, db untouched)."""
    dy, db0 = ur.colsum_inputs(M, N)
    dyd = dy.to(cuda)
    ref = ur.colsum(dy.double(), db0.double())
    need = egx_lib.egx_colsum_ordered_scratch(M, N)
    assert (need > 0) == (M > 32), "one row block (<= 32 rows) needs no scratch"
    scratch = torch.empty(max(need, 2 * N * 4) + 256, dtype=torch.uint8, device=cuda)
    bar = ur.BAR["colsum"]["out"]

    def run(ptr, nbytes, accept=True):
        dbb, dbv = _dev(db0, cuda, SENTINEL)
        rc = egx_lib.egx_colsum_ordered(_ptr(dyd), M, N, _ptr(dbb), ptr, nbytes, _stream())
        torch.cuda.synchronize()
        assert (dbb[N:] == SENTINEL).all()
        if not accept:
            _refused(egx_lib, rc)
            assert _same_bits(dbv.cpu(), db0), "a refused call changed db"
            return None
        _check(egx_lib, rc)
        return dbv.cpu()

    runs = [run(_ptr(scratch), need) for _ in range(3)]
    err = ur.rel_err(runs[0], ref)
    _report("colsum_ordered", f"M{M}N{N} db", err, bar)
    assert err <= bar
    assert _same_bits(runs[0], runs[1]) and _same_bits(runs[0], runs[2]), "the ordered column sum changed its bits between runs"
    two = run(_ptr(scratch), 2 * N * 4, accept=2 * N * 4 >= need)
    if two is not None:
        assert _same_bits(two, runs[0])
    none = run(None, 0, accept=need == 0)
    if none is not None:
        assert _same_bits(none, runs[0])
    if need:
        run(_ptr(scratch), need - 4, accept=False)
        run(None, need, accept=False)


# ---- egx_pool_head_fwd / _bwd --------------------------------------------------------------------------------------------------------------
def _pool_call(lib, cuda, t, B, S, d, n_out):
    """The raw forward and backward on the inputs `t` of ur.pool_inputs -> dict of host tensors (parameter gradients: buffer contents)."""
    dv = {k: (v.to(cuda) if v is not None else None) for k, v in t.items() if not k.endswith("0")}
    n = n_out if n_out else d
    pooled, out, d_tokens = _nanbuf(B * d, cuda), _nanbuf(B * n, cuda), _nanbuf(B * S * d, cuda)
    grads = {k: (_dev(t[k + "0"], cuda, SENTINEL) if t[k + "0"] is not None else (None, None)) for k in ("d_ln_w", "d_ln_b", "d_W", "d_b")}
    _check(lib, lib.egx_pool_head_fwd(_ptr(dv["tokens"]), B, S, d, _ptr(dv["ln_w"]), _ptr(dv["ln_b"]), ur.POOL_EPS, _ptr(dv["W"]), _ptr(dv["b"]), n,
                                      _ptr(pooled), _ptr(out), _stream()))
    _check(lib, lib.egx_pool_head_bwd(_ptr(dv["d_out"]), _ptr(pooled), B, S, d, _ptr(dv["ln_w"]), _ptr(dv["ln_b"]), ur.POOL_EPS, _ptr(dv["W"]), n,
                                      _ptr(d_tokens), _ptr(grads["d_ln_w"][0]), _ptr(grads["d_ln_b"][0]), _ptr(grads["d_W"][0]),
                                      _ptr(grads["d_b"][0]), _stream()))
    torch.cuda.synchronize()
    assert torch.isnan(pooled[B * d:]).all() and torch.isnan(out[B * n:]).all() and torch.isnan(d_tokens[B * S * d:]).all()
    res = {"pooled": pooled[:B * d].view(B, d).cpu(), "out": out[:B * n].view(B, n).cpu(), "d_tokens": d_tokens[:B * S * d].view(B, S, d).cpu()}
    for k, (buf, view) in grads.items():
        res[k] = view.cpu() if view is not None else None
        assert buf is None or (buf[view.numel():] == SENTINEL).all()
    return res


@pytest.mark.parametrize("form", list(ur.POOL_FORMS))
@pytest.mark.parametrize("B,S,d", ur.POOL_SHAPES)
def test_pool_head_fwd_bwd(egx_lib, cuda, B, S, d, form):
    from egot2_amd import functional as Fn
    ln, n_out = ur.POOL_FORMS[form]
    t = ur.pool_inputs(B, S, d, form)
    ref = ur.pool_head_grads(t, torch.float64)
    got = _pool_call(egx_lib, cuda, t, B, S, d, n_out)
    eo = {k: ur.rel_err(got[k], ref[k]) for k in ("pooled", "out")}
    eg = {k: ur.rel_err(got[k], ref[k]) for k in ("d_tokens", "d_ln_w", "d_ln_b", "d_W", "d_b") if ref[k] is not None}
    _report("pool_head", f"B{B}S{S}d{d} {form} out", max(eo.values()), ur.BAR["pool_head"]["out"])
    _report("pool_head", f"B{B}S{S}d{d} {form} grad", max(eg.values()), ur.BAR["pool_head"]["grad"])
    assert max(eo.values()) <= ur.BAR["pool_head"]["out"], eo
    assert max(eg.values()) <= ur.BAR["pool_head"]["grad"], eg
    dt = got["d_tokens"]
    assert _same_bits(dt, dt[:, :1].expand(B, S, d)), "the rows of a clip's d_tokens differ"
    # the autograd bridge: the same forward and the same d_tokens, bit for bit
    tok = t["tokens"].to(cuda).requires_grad_(True)
    par = [t[k].to(cuda) if t[k] is not None else None for k in ("ln_w", "ln_b", "W", "b")]
    out = Fn.pool_head(tok, *par, eps=ur.POOL_EPS)
    out.backward(t["d_out"].to(cuda))
    assert _same_bits(out.detach().cpu(), got["out"]) and _same_bits(tok.grad.cpu(), dt)


def test_pool_head_refusals(egx_lib, cuda):
    B, S = 2, 3
    tok = torch.randn(B * S * 1028, device=cuda)
    W = torch.randn(65 * 1028, device=cuda)
    outs = [_nanbuf(B * S * 1028, cuda) for _ in range(3)]
    dW = _nanbuf(65 * 1028, cuda)
    for d, n_out, Wp in ((128, 65, W), (1028, 2, W), (1028, 1028, None)):
        _refused(egx_lib, egx_lib.egx_pool_head_fwd(_ptr(tok), B, S, d, None, None, ur.POOL_EPS, _ptr(Wp), None, n_out, _ptr(outs[0]), _ptr(outs[1]),
                                                    _stream()))
        _refused(egx_lib, egx_lib.egx_pool_head_bwd(_ptr(tok), _ptr(tok), B, S, d, None, None, ur.POOL_EPS, _ptr(Wp), n_out, _ptr(outs[2]), None, None,
                                                    _ptr(dW) if Wp is not None else None, None, _stream()))
    torch.cuda.synchronize()
    for t in outs + [dW]:
        assert torch.isnan(t).all()
