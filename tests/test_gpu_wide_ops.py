"""The kernels of the wide bf16 path one by one (-m gpu) through the unit hooks of the C ABI: each against its fp64 reference of
tests/wide_ops_ref.py, per output element or row, at that module's bars; the cases and what each reaches are listed there.

Buffers a kernel overwrites start as NaN, buffers it adds into start as known non-zero values, padded operands live in larger NaN-filled buffers
whose padding must still be NaN afterwards, every scratch buffer has exactly the bytes its query returns and a guard region behind it. Each test
prints its figures (lines "WIDEOPS ...") before it asserts and keeps the worst in profiles/wide_ops_report.txt. The fp64 references run in torch
on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dropmask as dm
from tests import wide_ops_ref as wr

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096        # bytes behind every scratch buffer
F64 = torch.float64
BF = torch.bfloat16


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(lib, rc):
    assert rc == 0, lib.egx_last_error().decode()


def _held(op, kind, case, err, bar=None):
    bar = wr.BAR[op][kind] if bar is None else bar
    print(f"WIDEOPS {op} {kind} {case} err {err:.3e} bar {bar:.3e}")
    wr.note(op, kind, err, bar, case)
    return err <= bar


class _Scratch:
    """Exactly `nbytes` of scratch (what the hook's query returned) with a guard region behind it."""

    def __init__(self, nbytes, cuda):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + GUARD,), 0xA5, dtype=torch.uint8, device=cuda)

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.n:] == 0xA5).all())


def _padded(t, ld, dtype, cuda):
    """A (rows, cols) host tensor inside a NaN-filled (rows, ld) device buffer of `dtype` -> (buffer, window view)."""
    rows, cols = t.shape
    buf = torch.full((rows, ld), NAN, dtype=dtype, device=cuda)
    buf[:, :cols] = t.to(cuda).to(dtype)
    return buf, buf[:, :cols]


def _nanbuf(rows, ld, dtype, cuda):
    return torch.full((rows, ld), NAN, dtype=dtype, device=cuda)


def _pad_untouched(buf, cols):
    return bool(torch.isnan(buf[:, cols:].float()).all())


# ---- NT GEMM ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(wr.NT_CASES)), ids=[c["name"] for c in wr.NT_CASES])
def test_gemm_nt(egx_lib, cuda, ci):
    from egot2_amd._lib import WideGemmArgs
    c = wr.NT_CASES[ci]
    M, N, K, pad = c["M"], c["N"], c["K"], c["pad"]
    assert egx_lib.egx_wide_gemm_variant(0, M, N, K, int(c["colsum"])) == c["variant"], "the case no longer reaches the kernel it was written for"
    t = wr.nt_inputs(c)
    A, _ = _padded(t["A"], K + 2 * pad, BF, cuda)
    B, _ = _padded(t["B"], K + 2 * pad, BF, cuda)
    bias = t["bias"].to(cuda) if c["bias"] else None
    res = _padded(t["residual"], N + pad, torch.float32, cuda)[0] if c["res"] else None
    mask = _padded(t["mask"], N + pad, BF, cuda)[0] if c["mask"] else None
    ldc = N + pad
    Cf = _nanbuf(M, ldc, torch.float32, cuda) if "f" in c["out"] else None
    Cb = _nanbuf(M, ldc, BF, cuda) if "b" in c["out"] else None
    rows = egx_lib.egx_wide_gemm_colsum_rows(M, N)
    assert rows == wr.nt_colsum_rows(M, c["variant"])
    cs = _Scratch(rows * N * 4, cuda) if c["colsum"] else None
    if cs is not None:
        cs.buf[:cs.n].view(torch.float32).fill_(NAN)
    sc = _Scratch(egx_lib.egx_wide_gemm_scratch(0, M, N, K), cuda)
    a = WideGemmArgs(layout=0, A=_ptr(A), B=_ptr(B), M=M, N=N, K=K, lda=K + 2 * pad, ldb=K + 2 * pad, Cf=_ptr(Cf), Cb=_ptr(Cb), ldc=ldc,
                     bias=_ptr(bias), relu=int(c["relu"]), p_drop=c["p"], seed=wr.SEED, layer=ci, site=c["site"], residual=_ptr(res), ldr=N + pad,
                     mask=_ptr(mask), ldm=N + pad, mask_scale=wr.nt_mask_scale(c), colsum=cs.ptr() if cs else None, scratch=sc.ptr())
    _check(egx_lib, egx_lib.egx_wide_gemm_ex(C.byref(a), _stream()))
    torch.cuda.synchronize()
    ref = wr.nt_eval(c, F64, ci, device=cuda)
    ok = True
    if Cf is not None:
        ok &= _held("gemm_nt", "out", c["name"] + " Cf", wr.elem_err(Cf[:, :N], ref["C"], ref["scale"]))
        assert _pad_untouched(Cf, N)
    if Cb is not None:
        ok &= _held("gemm_nt", "out", c["name"] + " Cb", wr.elem_err(Cb[:, :N], ref["C"], ref["scale"], bf16_out=True))
        assert _pad_untouched(Cb, N)
    got = (Cf if Cf is not None else Cb)[:, :N]
    if c["p"] > 0 and not c["res"]:      # which elements the dropout zeroes: bit for bit
        dropped = (wr.nt_drop(c, ci) == 0).to(cuda)
        assert bool((got[dropped] == 0).all())
        sure = ~dropped & (ref["C"].abs() > 4 * wr.BAR["gemm_nt"]["out"] * ref["scale"])
        assert bool((got[sure] != 0).all())
    if c["relu"] and c["p"] == 0:        # the ReLU mask
        pre = wr.gemm_nt(*[t[k].to(cuda).double() if t[k] is not None else None for k in ("A", "B", "bias")])[0]
        sure = pre.abs() > 4 * wr.BAR["gemm_nt"]["out"] * ref["scale"]
        assert torch.equal((got != 0)[sure], (pre > 0)[sure])
    if cs is not None:
        dev = cs.buf[:cs.n].view(torch.float32).view(rows, N)
        if Cb is not None:               # the sums of the values AS STORED: the bias gradient equals colsum(stored dY)
            stored = Cb[:, :N].double()
            want, scale = wr.group_sums(stored, rows), wr.group_sums(stored.abs(), rows)
            assert wr.elem_err(want, ref["colsum"], ref["colsum_scale"] * (wr.BF16_ROUND + wr.BAR["gemm_nt"]["out"])) <= 1.0
        else:
            want, scale = ref["colsum"], ref["colsum_scale"]
        ok &= _held("gemm_nt", "colsum", c["name"] + " partial rows", wr.elem_err(dev, want, scale))
        ok &= _held("gemm_nt", "colsum", c["name"] + " total", wr.elem_err(dev.double().sum(0), want.sum(0), scale.sum(0)))
        assert cs.intact()
    assert sc.intact()
    for buf, keep in ((A, t["A"]), (B, t["B"])):
        assert torch.equal(buf[:, :K].float().cpu(), keep)
    assert ok


# ---- TN GEMM ---------------------------------------------------------------------------------------------------------------------------------
def _tn_problem(lib, c, cuda):
    from egot2_amd._lib import WideGemmArgs
    name, M, N, K, variant, splits, acc, path = c
    v = lib.egx_wide_gemm_variant(2, M, N, K, 0)
    assert (v & 255, v >> 8) == (variant, splits), "the case no longer reaches the kernel / split count it was written for"
    pad = 8 if path == "defer" else 0
    A0, B0, C0 = wr.tn_inputs(c)
    A, _ = _padded(A0, M + pad, BF, cuda)
    B, _ = _padded(B0, N + pad, BF, cuda)
    Cf = C0.to(cuda).clone() if acc else torch.full((M, N), NAN, device=cuda)
    sc = _Scratch(lib.egx_wide_gemm_scratch(2, M, N, K), cuda)
    a = WideGemmArgs(layout=2, A=_ptr(A), B=_ptr(B), M=M, N=N, K=K, lda=M + pad, ldb=N + pad, Cf=_ptr(Cf), ldc=N, accumulate=acc,
                     tn_queue=int(path == "queue"), tn_defer=int(path == "defer"), scratch=sc.ptr(), mask_scale=1.0)
    return a, (A, B, Cf, sc, C0)


@pytest.mark.parametrize("ci", range(len(wr.TN_CASES)), ids=[c[0] for c in wr.TN_CASES])
def test_gemm_tn(egx_lib, cuda, ci):
    c = wr.TN_CASES[ci]
    a, (A, B, Cf, sc, C0) = _tn_problem(egx_lib, c, cuda)
    _check(egx_lib, egx_lib.egx_wide_gemm_ex(C.byref(a), _stream()))
    torch.cuda.synchronize()
    ref, scale = wr.tn_eval(c, F64, device=cuda)
    ok = _held("gemm_tn", "out", c[0], wr.elem_err(Cf, ref, scale))
    assert sc.intact()
    first = Cf.clone()
    Cf.copy_(C0.to(cuda)) if c[6] else Cf.fill_(NAN)
    _check(egx_lib, egx_lib.egx_wide_gemm_ex(C.byref(a), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), Cf.view(torch.int32))          # fixed-order slab reduction: the same bits
    assert ok


def test_gemm_tn_grouped_batch(egx_lib, cuda):
    """Problems of all three tile variants and different sizes in ONE call: the queued ones share a grouped grid per variant, the deferred
    reductions one launch, the immediate ones run in between."""
    from egot2_amd._lib import WideGemmArgs
    cases = [wr.tn_case(n) for n in wr.TN_BATCH]
    assert {c[4] for c in cases if c[7] == "queue"} == {0, 1, 2} and {c[7] for c in cases} == {"now", "defer", "queue"}
    probs = [_tn_problem(egx_lib, c, cuda) for c in cases]
    args = (WideGemmArgs * len(probs))(*[p[0] for p in probs])
    _check(egx_lib, egx_lib.egx_wide_gemm_tn_batch(args, len(probs), _stream()))
    torch.cuda.synchronize()
    ok = True
    for c, (_, (A, B, Cf, sc, C0)) in zip(cases, probs):
        ref, scale = wr.tn_eval(c, F64, device=cuda)
        ok &= _held("gemm_tn", "out", "batch " + c[0], wr.elem_err(Cf, ref, scale))
        assert sc.intact()
    assert ok


# ---- row kernels -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wr.COLSUM_CASES, ids=[f"r{c[0]}_c{c[1]}_ld{c[2]}_defer{c[3]}" for c in wr.COLSUM_CASES])
def test_colsum(egx_lib, cuda, case):
    rows, cols, ld, defer = case
    x0, o0 = wr.colsum_inputs(rows, cols)
    x, _ = _padded(x0, ld, BF, cuda)
    out = torch.cat([o0, torch.full((8,), NAN)]).to(cuda)
    sc = _Scratch(egx_lib.egx_wide_colsum_scratch(rows, cols), cuda)
    _check(egx_lib, egx_lib.egx_wide_colsum(_ptr(x), rows, cols, ld, _ptr(out), defer, sc.ptr(), _stream()))
    torch.cuda.synchronize()
    ref, scale = wr.colsum(x0.to(cuda).double(), o0.to(cuda).double())
    ok = _held("colsum", "out", f"{rows}x{cols}", wr.elem_err(out[:cols], ref, scale))
    assert sc.intact() and bool(torch.isnan(out[cols:]).all())
    assert ok


@pytest.mark.parametrize("ci", range(len(wr.POS_GRAD_CASES)), ids=[f"B{c[0]}_T{c[3]}_d{c[4]}_p{c[6]}" for c in wr.POS_GRAD_CASES])
def test_pos_grad(egx_lib, cuda, ci):
    c = wr.POS_GRAD_CASES[ci]
    B, S, off, T, d, ps, p = c
    dtok0, dp0 = wr.pos_grad_inputs(c)
    dtok, dpos = dtok0.to(cuda), dp0.to(cuda).clone()
    nbytes = egx_lib.egx_wide_pos_grad_scratch(B, T, d)
    assert nbytes == wr.pos_grad_chunks(B)[0] * T * d * 4
    sc = _Scratch(nbytes, cuda)
    _check(egx_lib, egx_lib.egx_wide_pos_grad(_ptr(dtok), B, S, off, T, d, _ptr(dpos), ps, p, wr.SEED, ci, dm.SITE_POS, sc.ptr(), _stream()))
    torch.cuda.synchronize()
    ref, scale = wr.pos_grad(dtok.double(), dp0.to(cuda).double(), c, ci)
    ok = _held("pos_grad", "out", f"B{B} d{d}", wr.elem_err(dpos, ref, scale))
    assert sc.intact(), "the chunk sums ran past the scratch the query asked for"
    assert torch.equal(dpos[:, d:], dp0[:, d:].to(cuda))          # the table's padding columns
    assert ok


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("case", wr.CAST_CASES, ids=[f"{c[0]}x{c[1]}_ld{c[2]}" for c in wr.CAST_CASES])
def test_cast_and_transpose_bit_for_bit(egx_lib, cuda, case):
    R, Cc, ld = case
    x = wr.cast_inputs(R, Cc, ld, cuda)
    want = x[:, :Cc].to(BF)
    forms = [(True, False)] + ([(False, True), (True, True)] if R % 4 == 0 else [])
    for plain, transposed in forms:
        dst = torch.full((R * Cc + 64,), NAN, dtype=BF, device=cuda) if plain else None
        dst_t = torch.full((R * Cc + 64,), NAN, dtype=BF, device=cuda) if transposed else None
        _check(egx_lib, egx_lib.egx_wide_cast(0, _ptr(x), 0, None, R, Cc, ld, 1, _ptr(dst), _ptr(dst_t), _stream()))
        torch.cuda.synchronize()
        if plain:
            assert _same_bits(dst[:R * Cc].view(R, Cc), want) and bool(torch.isnan(dst[R * Cc:].float()).all())
        if transposed:
            assert _same_bits(dst_t[:R * Cc].view(Cc, R), want.T) and bool(torch.isnan(dst_t[R * Cc:].float()).all())


@pytest.mark.parametrize("case", wr.POOL_CASES, ids=[f"R{c[0]}_pool{c[1]}_C{c[2]}_bf{c[3]}" for c in wr.POOL_CASES])
def test_pool_cast(egx_lib, cuda, case):
    R, pool, Cc, bf = case
    x = wr.pool_inputs(R, pool, Cc, bf, cuda)
    src = x.to(BF) if bf else x
    dst = torch.full((R * Cc + 64,), NAN, dtype=BF, device=cuda)
    _check(egx_lib, egx_lib.egx_wide_cast(1, _ptr(src), bf, None, R, Cc, Cc, pool, _ptr(dst), None, _stream()))
    torch.cuda.synchronize()
    got = dst[:R * Cc].view(R, Cc)
    if pool == 1:
        assert _same_bits(got, x.to(BF))
    ok = _held("pool_cast", "out", f"R{R} pool{pool} C{Cc}", wr.row_err(got, wr.pool_cast(x.double(), pool), bf16_out=True))
    assert bool(torch.isnan(dst[R * Cc:].float()).all())
    assert ok


@pytest.mark.parametrize("case", wr.GATHER_CASES, ids=[f"R{c[0]}_of{c[1]}_C{c[2]}_bf{c[3]}" for c in wr.GATHER_CASES])
def test_gather_cast_bit_for_bit(egx_lib, cuda, case):
    R, n_src, Cc, bf = case
    x = wr.cast_inputs(n_src, Cc, Cc, cuda)
    src = x.to(BF) if bf else x
    rows = wr.gather_rows(R, n_src).to(cuda)
    dst = torch.full((R * Cc + 64,), NAN, dtype=BF, device=cuda)
    _check(egx_lib, egx_lib.egx_wide_cast(2, _ptr(src), bf, _ptr(rows), R, Cc, Cc, 1, _ptr(dst), None, _stream()))
    torch.cuda.synchronize()
    assert _same_bits(dst[:R * Cc].view(R, Cc), x.to(BF)[rows.long()]) and bool(torch.isnan(dst[R * Cc:].float()).all())


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------------
def _ln_device(c, cuda):
    t = wr.ln_inputs(c)
    orow, tpos, out_rows, out_map, src_map = wr.ln_maps(c)
    dev = {k: (v.to(cuda) if v is not None else None) for k, v in t.items()}
    maps = {"out": torch.from_numpy(out_map).to(cuda) if out_map is not None else None,
            "src": torch.from_numpy(src_map).to(cuda) if src_map is not None else None}
    return t, dev, maps, torch.as_tensor(orow, device=cuda), out_rows


@pytest.mark.parametrize("ci", range(len(wr.LN_CASES)), ids=[c["name"] for c in wr.LN_CASES])
def test_layernorm_fwd(egx_lib, cuda, ci):
    from egot2_amd._lib import WideLnFwdArgs
    c = wr.LN_CASES[ci]
    rows, d = c["rows"], c["d"]
    t, dev, maps, orow, out_rows = _ln_device(c, cuda)
    y32 = _nanbuf(out_rows, d, torch.float32, cuda) if "f" in c["out"] else None
    y16 = _nanbuf(out_rows, d, BF, cuda) if "b" in c["out"] else None
    stats = _nanbuf(rows + 4, 2, torch.float32, cuda)
    a = WideLnFwdArgs(x=_ptr(dev["x"]), w=_ptr(dev["w"]), b=_ptr(dev["b"]), eps=wr.LN_EPS, stats=_ptr(stats), y32=_ptr(y32), y16=_ptr(y16), rows=rows, d=d,
                      T=c["T"], S=c["S"], off=c["off"], add_vec=_ptr(dev["add"]), pos=_ptr(dev["pos"]), pos_stride=d + c["pos_pad"], p_drop=c["p"],
                      seed=wr.SEED, layer=ci, site=dm.SITE_POS, out_map=_ptr(maps["out"]), src_map=_ptr(maps["src"] if c["pos"] or not c["mapped"] else None))
    _check(egx_lib, egx_lib.egx_wide_layernorm_fwd(C.byref(a), _stream()))
    torch.cuda.synchronize()
    ry, rs, _ = wr.ln_fwd({k: (v.double() if v is not None else None) for k, v in dev.items()}, c, ci)
    written = torch.zeros(out_rows, dtype=torch.bool, device=cuda)
    written[orow] = True
    ok = _held("ln_fwd", "stats", c["name"], wr.elem_err(stats[:rows], rs, rs.abs().clamp(min=1.0)))
    assert bool(torch.isnan(stats[rows:]).all())
    for y, bf in ((y32, False), (y16, True)):
        if y is None:
            continue
        ok &= _held("ln_fwd", "out", c["name"] + (" y16" if bf else " y32"), wr.row_err(y[orow], ry, bf16_out=bf))
        assert bool(torch.isnan(y[~written].float()).all()), "a row no input maps to was written"
    if c["p"] > 0:          # which elements the dropout zeroes
        got = (y32 if y32 is not None else y16)[orow]
        dropped = (wr.drop_scale(wr.SEED, ci, dm.SITE_POS, orow.cpu().numpy(), d, c["p"]) == 0).to(cuda)
        assert bool((got[dropped] == 0).all()) and bool((got[~dropped & (ry.abs() > 1e-3)] != 0).all())
    assert ok


def _ln_bwd_problem(lib, ci, cuda, defer=None):
    from egot2_amd._lib import WideLnBwdArgs
    c = wr.LN_CASES[ci]
    rows, d = c["rows"], c["d"]
    t, dev, maps, orow, out_rows = _ln_device(c, cuda)
    stats = wr.ln_fwd(t, c, ci)[1].to(cuda)             # the saved (mean, rstd): fp32 numbers, the same for the device and the reference
    dx32 = _nanbuf(rows, d, torch.float32, cuda) if "f" in c["out"] else None
    dx16 = _nanbuf(rows, d, BF, cuda) if "b" in c["out"] else None
    tgt = {k: torch.cat([dev[k + "0"], torch.full((4,), NAN, device=cuda)]) for k in ("dw", "db", "dbias", "dadd")}
    sc = _Scratch(lib.egx_wide_layernorm_bwd_scratch(rows, d), cuda)
    dy_map = maps["out"] if c["mapped"] else None
    a = WideLnBwdArgs(dy=_ptr(dev["dy"]), pre=_ptr(dev["x"]), stats=_ptr(stats), w=_ptr(dev["w"]), dx32=_ptr(dx32), dx16=_ptr(dx16), rows=rows, d=d, T=c["T"],
                      S=c["S"], off=c["off"], p_drop=c["p"], seed=wr.SEED, layer=ci, site=dm.SITE_RES1, p_out=c["p_out"], out_layer=ci, out_site=dm.SITE_FEAT,
                      mask_dx32=int(c["mask_dx32"]), dw=_ptr(tgt["dw"]), db=_ptr(tgt["db"]), dbias=_ptr(tgt["dbias"]), dadd=_ptr(tgt["dadd"]),
                      dy_map=_ptr(dy_map), defer=int(c["defer"] if defer is None else defer), scratch=sc.ptr())
    return a, (c, dev, stats, dx32, dx16, tgt, sc, dy_map)


def _ln_bwd_held(ci, state, tag=""):
    c, dev, stats, dx32, dx16, tgt, sc, _ = state
    d = c["d"]
    ref = wr.ln_bwd({k: (v.double() if v is not None else None) for k, v in dev.items()}, stats.double(), c, ci)
    ok = True
    if dx32 is not None:
        ok &= _held("ln_bwd", "dx", tag + c["name"] + " dx32", wr.row_err(dx32, ref["m"] if c["mask_dx32"] else ref["dx"]))
    if dx16 is not None:
        ok &= _held("ln_bwd", "dx", tag + c["name"] + " dx16", wr.row_err(dx16, ref["m"], bf16_out=True))
        stored = dx16.double()          # the branch's bias gradient is the column sum of the operand AS STORED
        ref["dbias"], ref["dbias_scale"] = dev["dbias0"].double() + stored.sum(0), dev["dbias0"].double().abs() + stored.abs().sum(0)
    for k in ("dw", "db", "dadd", "dbias"):
        ok &= _held("ln_bwd", "dparam", f"{tag}{c['name']} {k}", wr.elem_err(tgt[k][:d], ref[k], ref[k + "_scale"]))
        assert bool(torch.isnan(tgt[k][d:]).all())
    assert sc.intact()
    return ok


@pytest.mark.parametrize("ci", range(len(wr.LN_CASES)), ids=[c["name"] for c in wr.LN_CASES])
def test_layernorm_bwd(egx_lib, cuda, ci):
    a, state = _ln_bwd_problem(egx_lib, ci, cuda)
    _check(egx_lib, egx_lib.egx_wide_layernorm_bwd(C.byref(a), _stream()))
    torch.cuda.synchronize()
    assert _ln_bwd_held(ci, state)


def test_row_reductions_batched(egx_lib, cuda):
    """Several LayerNorm backwards and column sums whose second stages run as ONE wide_row_reduce_flush launch (the end of a backward): the
    workgroups find their reduction by the prefix sums of the batch."""
    from egot2_amd._lib import WideColsumArgs, WideLnBwdArgs
    ln_ids = [i for i, c in enumerate(wr.LN_CASES) if not c["mapped"] and c["rows"] < 1000]
    assert len(ln_ids) >= 6 and {wr.LN_CASES[i]["d"] for i in ln_ids} == {4, 256, 260, 1024, 1028, 2048}
    lns = [_ln_bwd_problem(egx_lib, i, cuda, defer=1) for i in ln_ids]
    css = []
    for (rows, cols, ld, _) in wr.COLSUM_CASES[:5]:
        x0, o0 = wr.colsum_inputs(rows, cols)
        x = _padded(x0, ld, BF, cuda)[0]
        out = torch.cat([o0, torch.full((8,), NAN)]).to(cuda)
        sc = _Scratch(egx_lib.egx_wide_colsum_scratch(rows, cols), cuda)
        css.append((WideColsumArgs(x=_ptr(x), rows=rows, cols=cols, ld=ld, out=_ptr(out), scratch=sc.ptr()), (x0, o0, x, out, sc)))
    la = (WideLnBwdArgs * len(lns))(*[p[0] for p in lns])
    ca = (WideColsumArgs * len(css))(*[p[0] for p in css])
    _check(egx_lib, egx_lib.egx_wide_row_reduce_batch(la, len(lns), ca, len(css), _stream()))
    torch.cuda.synchronize()
    ok = True
    for i, (_, state) in zip(ln_ids, lns):
        ok &= _ln_bwd_held(i, state, "batch ")
    for a, (x0, o0, x, out, sc) in css:
        ref, scale = wr.colsum(x0.to(cuda).double(), o0.to(cuda).double())
        ok &= _held("colsum", "out", f"batch {a.rows}x{a.cols}", wr.elem_err(out[:a.cols], ref, scale))
        assert sc.intact() and bool(torch.isnan(out[a.cols:]).all())
    assert ok


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
def _attn_run(lib, c, qkv, d_out, p, layer_seed, cuda, bwd=True):
    cls, B, S, H, dh = c
    d = H * dh
    q16, do16 = qkv.to(cuda).to(BF), d_out.to(cuda).to(BF)
    out = _nanbuf(B * S, d, BF, cuda)
    lse = torch.full((B, H, S), NAN, device=cuda)
    dqkv = _nanbuf(B * S, 3 * d, BF, cuda)
    delta = torch.full((B, H, S), NAN, device=cuda) if cls == "long" else None
    _check(lib, lib.egx_wide_attention_fwd(_ptr(q16), _ptr(out), _ptr(lse), B, S, H, d, p, layer_seed, _stream()))
    if bwd:
        _check(lib, lib.egx_wide_attention_bwd(_ptr(q16), _ptr(out), _ptr(lse), _ptr(do16), _ptr(dqkv), _ptr(delta), B, S, H, d, p, layer_seed, _stream()))
    torch.cuda.synchronize()
    return out, lse, dqkv


def _attn_mask(c, p, seed):
    """The hooks key the attention site with layer 0: site_key(seed, 0, SITE_ATTN)."""
    cls, B, S, H, dh = c
    if p <= 0:
        return None
    rows = (np.arange(B * H)[:, None] * wr.ATTN_ROW_STRIDE[cls] + np.arange(S)[None, :]).reshape(B, H, S)
    return dm.keep_scale(dm.site_key(seed, 0, dm.SITE_ATTN), rows, np.arange(S, dtype=np.int64), p)


@pytest.mark.parametrize("ci", range(len(wr.ATTN_CASES)), ids=[wr.attn_case_id(c) for c in wr.ATTN_CASES])
def test_attention_fwd_bwd(egx_lib, cuda, ci):
    """out, lse and d_qkv per (clip, head, row) at p = 0 and under the restated mask at p = 0.1 and 0.5."""
    c = wr.ATTN_CASES[ci]
    cls, B, S, H, dh = c
    qkv, d_out = wr.attn_inputs(c)
    ok = True
    for p in wr.ATTN_PS:
        seed = wr.SEED + ci
        out, lse, dqkv = _attn_run(egx_lib, c, qkv, d_out, p, seed, cuda)
        mask = _attn_mask(c, p, seed)
        ref = wr.attention(qkv.to(cuda).double(), d_out.to(cuda).double(), c, mask)
        name = f"{wr.attn_case_id(c)} p{p}"
        ok &= _held("attention", "out", name, wr.elem_err(wr.attn_heads(out, c)[0], ref["out"], ref["out_scale"], bf16_out=True))
        ok &= _held("attention", "lse", name, wr.elem_err(lse, ref["lse"], ref["lse_scale"]))
        for k, g in zip(("dq", "dk", "dv"), wr.attn_heads(dqkv, c, 3)):
            ok &= _held("attention", "grad", f"{name} {k}", wr.elem_err(g, ref[k], ref[k + "_scale"], bf16_out=True))
    assert ok


@pytest.mark.parametrize("c", [("short", 2, 65, 3, 32), ("long", 1, 161, 2, 64), ("bighead", 3, 16, 2, 256)], ids=["short", "long", "bighead"])
def test_attention_p1_and_refusals(egx_lib, cuda, c):
    """p = 1: every probability dropped, zero outputs and a finite d_qkv. A head dim of 256 with S = 17 is refused."""
    qkv, d_out = wr.attn_inputs(c)
    out, lse, dqkv = _attn_run(egx_lib, c, qkv, d_out, 1.0, 5, cuda)
    assert bool((out == 0).all()) and bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(lse).all())
    assert bool((dqkv[:, 2 * c[3] * c[4]:] == 0).all())            # dV = dropped P^T dO
    x = torch.zeros(17 * 2, 3 * 512, dtype=BF, device=cuda)
    o = torch.zeros(17 * 2, 512, dtype=BF, device=cuda)
    l = torch.zeros(2, 2, 17, device=cuda)
    assert egx_lib.egx_wide_attention_fwd(_ptr(x), _ptr(o), _ptr(l), 2, 17, 2, 512, 0.0, 0, _stream()) != 0
    assert b"head dim 256" in egx_lib.egx_last_error()


@pytest.mark.parametrize("c", [("short", 2, 100, 3, 32), ("long", 1, 161, 2, 64), ("bighead", 3, 16, 2, 256)], ids=["short", "long", "bighead"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_mask_read_back(egx_lib, cuda, c, p):
    """The mask itself, element by element: Q = K = 0 makes every probability 1 / S; V = the one-hot columns of a block of dh keys makes
    out[query][c] = keep(query, k0 + c) / ((1 - p) S). The block steps across the S keys."""
    cls, B, S, H, dh = c
    d, seed = H * dh, 0xFACE + S
    keep = (_attn_mask(c, p, seed) != 0).to(cuda)                                  # (B, H, S, S)
    val = dm.inv_keep(p) / S
    seen = torch.zeros(B, H, S, S, dtype=torch.bool, device=cuda)
    for k0 in range(0, S, dh):
        n = min(dh, S - k0)
        qkv = torch.zeros(B, S, 3, H, dh)
        qkv[:, k0:k0 + n, 2, :, :n] = torch.eye(n)[None, :, None, :].expand(B, n, H, n)
        out, _, _ = _attn_run(egx_lib, c, qkv.view(B * S, 3 * d), torch.zeros(B * S, d), p, seed, cuda, bwd=False)
        got = wr.attn_heads(out, c)[0].float()                                     # (B, H, S, dh): column c is key k0 + c
        k = keep[..., k0:k0 + n]
        assert torch.equal(got[..., :n] != 0, k), "the device dropped other elements than the restated mask"
        assert bool(((got[..., :n][k] - val).abs() <= (wr.BF16_ROUND + 1e-6) * val).all())
        assert bool((got[..., n:] == 0).all())
        seen[..., k0:k0 + n] = True
    assert bool(seen.all())
