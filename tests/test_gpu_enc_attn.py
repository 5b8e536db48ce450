"""-m gpu: the encoder's self-attention weights as an output (egx_self_attention_weights, egx_attention_rollout,
egx_encoder_self_weights through functional.self_attention_weights / attention_rollout and model.record_attention()): the head-averaged
weights a patched reference layer (self_attn(..., need_weights=True)) sees, their per-task sums and the attention rollout.
  1. the primitive alone on bf16-representable inputs, fp32 and bf16 operands, against an fp64 softmax: max |w - ref| under the kernel-level
     bar (2e-6; its condition and the cases with a bar of their own: tests/enc_attn_ref.py, checked in tests/test_cpu_enc_attn.py), rows sum
     to 1 within 1e-6, the segment sums add up to the row sum, entries beyond a clip's tokens exactly 0, NaN-filled guard bands untouched,
     the same bits under a permutation of the clips and on repetition; dense rows, the 48-row grid with gaps, a ragged table with an empty slot;
  2. the rollout on random row-stochastic inputs against fp64; L = 1 bit-exact (w + I) / 2;
  3. the models, every implementation asserted through last_encoder_impl(): (a) the weights against the fp64 softmax of the call's OWN
     Q | K | V (read back through the EGX_STAGE_QKV hook, d = 128 paths): the kernel's error without upstream error; (b) weights, segment
     shares and rollout against the gate's fp64 model oracle and the recordings of the real classes: e < s / 4, f32 / f32s paths also
     e < 8 x the fp32 oracle's error; (c) outputs bit-equal to the unrecorded call; (d) layers= returns the selected layers' rows bit for bit.
Every test prints its figures (tools/encoder_attention_eval.py collects them into profiles/encoder_attention_report.txt).
Measured on an MI355X: item 1 worst max |w - fp64| per head shape 3 .. 16 % of the case's bar; item 2 3.0e-8 (L = 1) .. 9.8e-7 (L = 2, S = 512,
bar 5.04e-6); item 3a 9.5e-9 .. 4.1e-7 beside fp32 yardsticks of 1.2e-8 .. 2.8e-7; item 3b weights e / s: f32s and f32 paths 1.8e-7 .. 4.2e-7 /
0.19 .. 0.44 (fp32 oracle 1.1e-7 .. 3.6e-7), bf16 paths 1.0e-3 .. 4.0e-3 (0.4 .. 1.1 % of s)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from oracle import translator_ref as tr
from tests import enc_attn_ref as er

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 3       # guard rows in front of and behind every output, 8 guard columns behind the S written ones


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tables(B, S, first, lengths, cuda):
    """(rowtab | None, segtab (B, 3) on the device, the host segment table) of a layout case."""
    lens = [S] * B if lengths is None else lengths
    host = torch.zeros(B, 3, dtype=torch.int32)
    for b, n in enumerate(lens):
        sp = er.primitive_segments(n) if n else []
        host[b, :len(sp)] = torch.tensor(sp, dtype=torch.int32)
    rowtab = None if first is None else torch.tensor([[f, n] for f, n in zip(first, lens)], dtype=torch.int32).to(cuda)
    return rowtab, host.to(cuda), host


def _call(lib, qv, kv, dt, rowtab, segtab, B, H, dh, S, cuda, want_w=True, want_seg=True):
    """egx_self_attention_weights into NaN-filled buffers inside guard bands; returns (w (B, S, S) | None, seg (B, S, 3) | None) on the
    CPU after checking that the guards are untouched."""
    from egot2_amd import _lib
    ldw, K = S + 8, 3
    wbuf = torch.full((2 * GUARD + B * S, ldw), NAN, device=cuda) if want_w else None
    sbuf = torch.full((2 * GUARD + B * S, K), NAN, device=cuda) if want_seg else None
    _lib.check(lib.egx_self_attention_weights(qv.data_ptr(), qv.stride(0), kv.data_ptr(), kv.stride(0), int(dt == torch.bfloat16),
                                              rowtab.data_ptr() if rowtab is not None else None, segtab.data_ptr() if want_seg else None,
                                              K if want_seg else 0, B, H, dh, S, wbuf[GUARD:].data_ptr() if want_w else None, ldw,
                                              sbuf[GUARD:].data_ptr() if want_seg else None, _stream()))
    w = seg = None
    if want_w:
        wb = wbuf.cpu()
        assert torch.isnan(wb[:GUARD]).all() and torch.isnan(wb[GUARD + B * S:]).all() and torch.isnan(wb[:, S:]).all(), "guards of w"
        w = wb[GUARD:GUARD + B * S, :S].reshape(B, S, S)
        assert not torch.isnan(w).any()
    if want_seg:
        sb = sbuf.cpu()
        assert torch.isnan(sb[:GUARD]).all() and torch.isnan(sb[GUARD + B * S:]).all(), "guards of seg"
        seg = sb[GUARD:GUARD + B * S].reshape(B, S, K)
        assert not torch.isnan(seg).any()
    return w, seg


# ---- 1. the primitive alone ----
@pytest.mark.parametrize("H,dh", er.PRIM_SHAPES)
def test_primitive_against_fp64_softmax(egx_lib, cuda, H, dh):
    d, worst = H * dh, 0.0
    for key, q, k, B, S, first, lengths in er.primitive_layout_cases(H, dh):
        ref = er.ref_weights(q, k, H, B, S, first, lengths)
        lens = [S] * B if lengths is None else lengths
        rowtab, segtab, seg_host = _tables(B, S, first, lengths, cuda)
        ref_seg = er.segment_sums(ref, seg_host)
        bar = er.kernel_bar(key)
        for dt in (torch.float32, torch.bfloat16):
            # q and k as the first and second d columns of a packed (rows, 3d) Q | K | V matrix, read in place through the strides
            qkv = torch.cat((q, k, torch.full_like(q, NAN)), 1).to(cuda, dt)
            qv, kv = qkv[:, :d], qkv[:, d:2 * d]
            w, seg = _call(egx_lib, qv, kv, dt, rowtab, segtab, B, H, dh, S, cuda)
            e = (w.double() - ref).abs().max().item()
            worst = max(worst, e / bar)
            assert e < bar, (key, dt, e, bar)
            assert (seg.double() - ref_seg).abs().max().item() < bar, (key, dt)
            for b, n in enumerate(lens):
                assert (w[b, :n, :n].double().sum(-1) - 1).abs().max().item() < 1e-6 if n else True, (key, dt, b)
                assert (seg[b, :n].double().sum(-1) - w[b, :n].double().sum(-1)).abs().max().item() < 1e-6 if n else True, (key, dt, b)
                assert w[b, n:].abs().max().item() == 0 if n < S else True         # rows beyond the clip: exact zeros
                assert w[b, :, n:].abs().max().item() == 0 if n < S else True      # and entries beyond its keys
                assert seg[b, n:].abs().max().item() == 0 if n < S else True
            # repetition, and each output alone: the same bits (seg alone never writes w)
            w2, seg2 = _call(egx_lib, qv, kv, dt, rowtab, segtab, B, H, dh, S, cuda)
            assert torch.equal(w, w2) and torch.equal(seg, seg2), (key, dt)
            w3, _ = _call(egx_lib, qv, kv, dt, rowtab, segtab, B, H, dh, S, cuda, want_seg=False)
            _, seg3 = _call(egx_lib, qv, kv, dt, rowtab, segtab, B, H, dh, S, cuda, want_w=False)
            assert torch.equal(w, w3) and torch.equal(seg, seg3), (key, dt)
            if B > 1:       # the clips in another order (through the row table): every clip's rows keep their bits
                perm = [3, 0, 4, 2, 1] if B == 5 else list(range(B - 1, -1, -1))
                f0 = [b * S for b in range(B)] if first is None else first
                ptab = torch.tensor([[f0[p], lens[p]] for p in perm], dtype=torch.int32).to(cuda)
                wp, sp = _call(egx_lib, qv, kv, dt, ptab, segtab[perm].contiguous(), B, H, dh, S, cuda)
                assert torch.equal(wp, w[perm]) and torch.equal(sp, seg[perm]), (key, dt)
    print(f"H = {H}, dh = {dh}: worst max|w - fp64| / bar = {worst:.3f}")


def test_primitive_functional_wrapper(egx_lib, cuda):
    """functional.self_attention_weights: the C entry's bits, with and without tables; an out-of-range table entry is clamped."""
    from egot2_amd import functional as F_egx
    H, dh, S, B = 4, 32, 45, 5
    q, k = er.primitive_inputs(H, dh, S, B)
    qd, kd = q.to(cuda), k.to(cuda)
    rowtab, segtab, host = _tables(B, S, None, None, cuda)
    w0, seg0 = _call(egx_lib, qd, kd, torch.float32, None, segtab, B, H, dh, S, cuda)
    w = F_egx.self_attention_weights(qd, kd, H, S)
    assert w.shape == (B, S, S) and torch.equal(w.cpu(), w0)
    w, seg = F_egx.self_attention_weights(qd, kd, H, S, segments=er.primitive_segments(S))
    assert torch.equal(w.cpu(), w0) and torch.equal(seg.cpu(), seg0)
    assert torch.equal(F_egx.self_attention_weights(qd, kd, H, S, segments=host, weights=False).cpu(), seg0)
    tab = torch.tensor([[b * S, S] for b in range(B)], dtype=torch.int32)
    tab[1, 1], tab[2, 1] = 600, -4          # clamped to S / to an empty slot
    w = F_egx.self_attention_weights(qd, kd, H, S, rowtab=tab.to(cuda)).cpu()
    assert torch.equal(w[[0, 1, 3, 4]], w0[[0, 1, 3, 4]]) and w[2].abs().max().item() == 0
    for bad in (dict(q=qd.cpu()), dict(k=kd[:-1]), dict(n_heads=3), dict(S=44)):
        args = dict(q=qd, k=kd, n_heads=H, S=S)
        args.update(bad)
        with pytest.raises(ValueError):
            F_egx.self_attention_weights(**args)


# ---- 2. the rollout ----
def test_rollout_against_fp64(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    for L, B, S in er.rollout_cases():
        w = er.rollout_inputs(L, B, S)
        ref = er.rollout(w.double())
        segs = er.primitive_segments(S)
        R, Rs = F_egx.attention_rollout(w.to(cuda), segments=segs)
        R, Rs = R.cpu(), Rs.cpu()
        bar = er.kernel_bar(("rollout", L, S))
        e = (R.double() - ref).abs().max().item()
        print(f"rollout L = {L}, B = {B}, S = {S}: max|R - fp64| = {e:.3e} (bar {bar:.2e})")
        assert e < bar, (L, S, e)
        assert (Rs.double() - er.segment_sums(ref, torch.tensor([segs] * B))).abs().max().item() < bar
        assert (R.double().sum(-1) - 1).abs().max().item() < 1e-5
        if L == 1:
            assert torch.equal(R, (w[0] + torch.eye(S)) / 2), "L = 1 must be (w + I) / 2 exactly"
        assert torch.equal(F_egx.attention_rollout(w.to(cuda)).cpu(), R)           # repetition, without the segment sums
        if B > 1 and S > 1:      # clips of their own lengths: the product over the clip's tokens, zeros beyond
            lens = [S, 1, (S + 1) // 2]
            wl = w.clone()
            for b, n in enumerate(lens):
                wl[:, b, :, n:] = 0
                wl[:, b, :n, :n] /= wl[:, b, :n, :n].sum(-1, keepdim=True)
            Rl = F_egx.attention_rollout(wl.to(cuda), lengths=torch.tensor(lens, dtype=torch.int32).to(cuda)).cpu()
            refl = er.rollout(wl.double(), lengths=lens)
            assert (Rl.double() - refl).abs().max().item() < bar
            for b, n in enumerate(lens):
                assert Rl[b, n:].abs().max().item() == 0 and Rl[b, :, n:].abs().max().item() == 0 if n < S else True


# ---- 3. the models ----
def _forward(c, m, feats, **kw):
    if c["kind"] == "hhi_g":
        return m.encode_features("ttm", *feats, **kw)
    return m.forward_features(*feats, **kw)


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b)


def _own_qkv(rec, layer, cuda):
    """Layer `layer`'s Q | K | V rows of the recorded call itself, (tokens, 3d) in token order, through the stage hooks; None where the
    implementation has none (wide, generic)."""
    from egot2_amd import _lib, functional as F_egx
    lib, lc = _lib.load(), rec.last_call
    r, cc, kd = C.c_int(0), C.c_int(0), C.c_int(0)
    item = F_egx.STAGE_ITEMS["QKV"]
    if lc["lengths"] is None:
        rc = lib.egx_encoder_stage_info(C.byref(lc["cfg"]), lc["segs"], lc["B"], lc["head_n_out"], item, layer, C.byref(r), C.byref(cc), C.byref(kd))
    else:
        rc = lib.egx_ragged_stage_info(C.byref(lc["cfg"]), lc["segs"], lc["B"], lc["lengths"].data_ptr(), lc["head_n_out"], item, layer,
                                       C.byref(r), C.byref(cc), C.byref(kd))
    if rc == F_egx.STAGE_NOT_KEPT:
        return None
    _lib.check(rc)
    out = torch.full((r.value, cc.value), NAN, device=cuda)
    if lc["lengths"] is None:
        _lib.check(lib.egx_encoder_stage_read(C.byref(lc["cfg"]), lc["segs"], lc["B"], lc["head_n_out"], lc["saved"].data_ptr(), None, item, layer,
                                              out.data_ptr(), _stream()))
    else:
        _lib.check(lib.egx_ragged_stage_read(C.byref(lc["cfg"]), lc["segs"], lc["B"], lc["lengths"].data_ptr(), lc["head_n_out"],
                                             lc["saved"].data_ptr(), None, item, layer, out.data_ptr(), _stream()))
    out = out.cpu()
    assert not torch.isnan(out).any()
    return out


def _check_own_qkv(what, rec, record, H, cuda, clip_lens=None):
    """(a): every recorded layer against the fp64 softmax of the call's own Q | K, at the kernel-level bar; the yardstick (stock fp32 torch on
    the same rows) is computed here: where it is above bar / 8 the case's bar is 8 x its yardstick."""
    L, B, S, _ = record.weights.shape
    for n, layer in enumerate(record.layers):
        qkv = _own_qkv(rec, layer, cuda)
        if qkv is None:
            return False
        d = qkv.shape[1] // 3
        lens = [S] * B if clip_lens is None else clip_lens
        first = [sum(lens[:b]) for b in range(B)]
        ref = er.ref_weights(qkv[:, :d], qkv[:, d:2 * d], H, B, S, first, lens)
        y = (er.ref_weights(qkv[:, :d], qkv[:, d:2 * d], H, B, S, first, lens, dtype=torch.float32).double() - ref).abs().max().item()
        bar = max(er.BAR_KERNEL, 8 * y)
        e = (record.weights[n].double().cpu() - ref).abs().max().item()
        print(f"[{what}] layer {layer}: kernel error against the call's own Q | K = {e:.3e} (yardstick {y:.2e}, bar {bar:.2e})")
        assert e < bar, (what, layer, e, bar)
    return True


def _check_record(what, record, oracle, cuda, e32=None):
    """(b): weights, segment shares and rollout at the model-level bars, and the derived quantities against the call's own weights at the
    kernel-level bar."""
    w, seg, R, Rs, table = oracle
    L, B, S, _ = w.shape
    uni = er.uniform_answer(L, table, S)
    assert torch.equal(record.segments, table.to(torch.int32)), what
    e, s = er.model_bar(record.weights, w, uni[0], what + " weights", e32=e32)
    er.model_bar(record.by_segment, seg, uni[1], what + " by_segment")
    er.model_bar(record.rollout, R, uni[2], what + " rollout")
    er.model_bar(record.rollout_by_segment, Rs, uni[3], what + " rollout_by_segment")
    dw = record.weights.double().cpu()
    lens = table.sum(1).tolist()
    assert (record.by_segment.double().cpu() - er.segment_sums(dw, table)).abs().max().item() < er.BAR_KERNEL, what
    dR = er.rollout(dw, lengths=lens)
    assert (record.rollout.double().cpu() - dR).abs().max().item() < er.BAR_KERNEL, what
    assert (record.rollout_by_segment.double().cpu() - er.segment_sums(dR, table)).abs().max().item() < er.BAR_KERNEL, what
    for b, n in enumerate(lens):
        assert (dw[:, b, :n, :n].sum(-1) - 1).abs().max().item() < 1e-6, what
        assert dw[:, b, n:].abs().max().item() == 0 and dw[:, b, :, n:].abs().max().item() == 0 if n < S else True
    return e, s


# name -> (compute, impl asked for, last_encoder_impl(), EGX_FFN_SLICES | None, workgroups per clip: 1, ">1" or None)
RUNS = [
    ("ttm3_T15", "f32s", "auto", "fused", "1", 1),          # one workgroup per clip: the cut mode of the f32s arithmetic
    ("ttm3_T15", "bf16", "auto", "fused", "1", 1),          # one launch
    ("ttm3_B1", "f32s", "auto", "fused", None, ">1"),       # sliced
    ("ttm3_B3", "f32s", "auto", "fused", None, ">1"),
    ("pnr3_L6", "f32s", "auto", "fused", None, None),
    ("asd_L2", "f32s", "auto", "fused", None, None),
    ("asd_L2", "bf16", "auto", "fused", None, None),
    ("ttm3_T17", "f32s", "auto", "tiled", None, None),
    ("ttm3_T50", "bf16", "auto", "tiled", None, None),
    ("lta4_d256", "bf16", "auto", "wide", None, None),
    ("lta4_d768", "bf16", "auto", "wide", None, None),
    ("hhi_g", "bf16", "auto", "wide", None, None),
    ("ttm3_T15", "f32", "generic", "generic", None, None),
    ("rec_ttm3", "f32s", "auto", "fused", None, None),
    ("rec_asd", "f32s", "auto", "fused", None, None),
    ("rec_pnr3", "f32s", "auto", "fused", None, None),
    ("rec_lta4", "bf16", "auto", "wide", None, None),
]


@pytest.mark.parametrize("name,compute,impl,ran,slices_env,wgs", RUNS, ids=[f"{r[0]}-{r[1]}-{r[3]}" for r in RUNS])
def test_models_record_attention(egx_lib, cuda, monkeypatch, name, compute, impl, ran, slices_env, wgs):
    from egot2_amd import functional as F_egx
    if slices_env is None:
        monkeypatch.delenv("EGX_FFN_SLICES", raising=False)
    else:
        monkeypatch.setenv("EGX_FFN_SLICES", slices_env)
    c = er.ALL_CASES[name]
    m, _ = er.new_model(c)
    m = m.to(cuda).set_compute(compute, impl).eval()
    feats = [f.float().to(cuda) for f in er.case_feats(c)]
    oracle = er.case_oracle(name)
    if name in er.RECORDINGS:       # the recording of the real class itself
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live", "enc_attn_ref.npz"))
        assert json.loads(str(z[name + "/config"])) == c
        oracle = (torch.from_numpy(z[name + "/weights"]),) + oracle[1:]
    what = f"{name} {compute} {ran}"
    with torch.no_grad():
        plain = _forward(c, m, feats)
        assert F_egx.last_encoder_impl() == ran
        if wgs is not None:
            assert (F_egx.last_encoder_slices() > 1) if wgs == ">1" else (F_egx.last_encoder_slices() == 1), F_egx.last_encoder_slices()
        with m.record_attention(rollout=True) as rec:
            out = _forward(c, m, feats)
            assert F_egx.last_encoder_impl() == ran
        assert _same(out, plain), "(c) the recorded call's outputs are the plain call's"
        assert _same(_forward(c, m, feats), plain)
        assert len(rec.records) == 1 and rec.records[0].impl == ran
        r = rec.records[0]
        L, B, S, _ = oracle[0].shape
        K = oracle[4].shape[1]
        assert r.weights.shape == (L, B, S, S) and r.by_segment.shape == (L, B, S, K) and r.rollout.shape == (B, S, S)
        assert r.rollout_by_segment.shape == (B, S, K) and r.layers == tuple(range(L))
        e32 = (er.case_variant(name, dtype=torch.float32) - er.case_oracle(name)[0]).abs().max().item() if compute in ("f32", "f32s") else None
        _check_record(what, r, oracle, cuda, e32=e32)
        H = m.transformer_encoder.layers[0].self_attn.num_heads if hasattr(m, "transformer_encoder") else m.transformer.layers[0].self_attn.num_heads
        served = _check_own_qkv(what, rec, r, H, cuda)
        assert served == (ran in ("fused", "tiled")), "the stage hooks serve the d = 128 paths"
        # (d) layers=: the selected layers' rows, bit for bit; weights=False: the segment shares alone, the same bits
        pick = [L - 1] if L < 3 else [1, L - 1]
        with m.record_attention(layers=pick) as rec2:
            assert _same(_forward(c, m, feats), plain)
        r2 = rec2.records[0]
        assert r2.layers == tuple(pick) and r2.rollout is None
        assert torch.equal(r2.weights, r.weights[pick]) and torch.equal(r2.by_segment, r.by_segment[pick])
        with m.record_attention(weights=False, rollout=True, layers=pick) as rec3:
            _forward(c, m, feats)
        r3 = rec3.records[0]
        assert r3.weights is None and torch.equal(r3.by_segment, r.by_segment[pick]) and torch.equal(r3.rollout, r.rollout)
    # outside the context nothing changes, down to the launches issued
    with torch.no_grad():
        egx_lib.egx_launch_count(1)
        _forward(c, m, feats)
        n_plain = egx_lib.egx_launch_count(0)
        with m.record_attention() as rec4:
            egx_lib.egx_launch_count(1)
            _forward(c, m, feats)
            n_rec = egx_lib.egx_launch_count(0)
        egx_lib.egx_launch_count(1)
        _forward(c, m, feats)
        assert egx_lib.egx_launch_count(0) == n_plain and n_rec == n_plain + L, (n_plain, n_rec, L)
    assert F_egx._attention_sink is None


def _ragged_oracle(sd64, clips, H):
    """fp64 (weights, by_segment, rollout, rollout_by_segment, table) of a ragged TTM 3-task batch: every clip alone, unpadded."""
    lens = [[f.shape[0] for f in c] for c in clips]
    S = max(sum(t) for t in lens)
    L = tr.n_layers_of(sd64, "transformer_encoder.")
    w = torch.zeros(L, len(clips), S, S, dtype=torch.float64)
    for b, c in enumerate(clips):
        x = tr.hhi_tokens(sd64, [f[None].double() for f in c], ["ttm", "lam", "asd"], [0, 1, 2])
        wb, _ = er.encoder_weights(sd64, "transformer_encoder.", x, H)
        n = x.shape[1]
        w[:, b, :n, :n] = wb[:, 0]
    table = torch.tensor(lens, dtype=torch.int32)
    R = er.rollout(w, lengths=table.sum(1).tolist())
    return w, er.segment_sums(w, table), R, er.segment_sums(R, table), table


@pytest.mark.parametrize("compute", ["f32s", "bf16"])
def test_ragged_d128_batch_records_every_clip_as_alone(egx_lib, cuda, compute):
    """forward_features(..., lengths=) and forward_features_ragged(..., lengths=) of the TTM 3-task translator (L = 2) over clips of 1 .. 60
    frames per task, mixed: S = max_b S_b, every clip's weights those of the clip alone, zeros beyond it."""
    from egot2_amd import functional as F_egx
    from tests.util import seeded_feats
    c = dict(kind="ttm3", L=2, B=0, T=0, wseed=541, fseed=542, sharp=1.25)
    m, sd64 = er.new_model(c)
    m = m.to(cuda).set_compute(compute).eval()
    tuples = [(1, 1, 1), (15, 15, 15), (16, 16, 16), (16, 16, 17), (60, 60, 60), (1, 2, 3), (60, 1, 7), (33, 48, 21)]
    clips = [[f[0] for f in seeded_feats(c["fseed"] + i, [(1, T, 256) for T in tup])] for i, tup in enumerate(tuples)]
    feats = []
    for k in range(3):
        t = torch.full((len(clips), 60, 256), NAN)          # padded frames are NaN: a kernel that reads one shows at once
        for b, cl in enumerate(clips):
            t[b, :cl[k].shape[0]] = cl[k]
        feats.append(t.to(cuda))
    lengths = torch.tensor(tuples)
    with torch.no_grad():
        oracle = _ragged_oracle(sd64, clips, 4)
    clip_lens = [sum(t) for t in tuples]
    for method in ("forward_features", "forward_features_ragged"):
        what = f"ragged {compute} {method}"
        with torch.no_grad():
            plain = getattr(m, method)(*feats, lengths=lengths)
            assert F_egx.last_encoder_impl() == "ragged"
            with m.record_attention(rollout=True) as rec:
                out = getattr(m, method)(*feats, lengths=lengths)
            assert torch.equal(out, plain)
            r = rec.records[0]
            assert r.impl == "ragged" and r.weights.shape == (2, len(clips), 180, 180)
            e32 = None
            if compute == "f32s":       # the same oracle in fp32, clip by clip
                sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd64.items()}
                w32 = torch.zeros_like(oracle[0])
                for b, cl in enumerate(clips):
                    x = tr.hhi_tokens(sd32, [f[None] for f in cl], ["ttm", "lam", "asd"], [0, 1, 2])
                    w32[:, b, :x.shape[1], :x.shape[1]] = er.encoder_weights(sd32, "transformer_encoder.", x, 4)[0][:, 0].double()
                e32 = (w32 - oracle[0]).abs().max().item()
            _check_record(what, r, oracle, cuda, e32=e32)
            assert _check_own_qkv(what, rec, r, 4, cuda, clip_lens=clip_lens)
            with m.record_attention(layers=[1]) as rec2:
                getattr(m, method)(*feats, lengths=lengths)
            assert torch.equal(rec2.records[0].weights, r.weights[[1]])


def test_functional_encoder_attention(egx_lib, cuda):
    """functional.encoder_attention: the no-autograd forward + the record in one call, against model.record_attention()."""
    from egot2_amd import functional as F_egx
    from egot2_amd.functional import SegmentSpec
    from egot2_amd.translator import encoder_layer_tensors
    c = er.ALL_CASES["asd_L2"]
    m, _ = er.new_model(c)
    m = m.to(cuda).set_compute("f32s").eval()
    feats = [f.to(cuda) for f in er.case_feats(c)]
    with torch.no_grad(), m.record_attention(rollout=True) as rec:
        m.forward_features(*feats)
    r = rec.records[0]
    order = [feats[2], feats[0], feats[1]]          # tokens asd | ttm | lam
    segs = [SegmentSpec(T=f.shape[1], d_in=f.shape[2], has_proj=True, add_row=k, pos_row0=0) for f, k in zip(order, (2, 0, 1))]
    spec = F_egx.EncoderSpec(d_model=128, n_heads=4, d_ff=m.transformer_encoder.layers[0].linear1.out_features, n_layers=2, segments=segs,
                             compute="f32s", p_drop=0.1)
    proj = [t for p in (m.proj_asd, m.proj_ttm, m.proj_lam) for t in (p.weight, p.bias)]
    tokens, r2 = F_egx.encoder_attention(spec, order, m.task_embed, m.pos_embed.pe, m.ln.weight, m.ln.bias, proj,
                                         encoder_layer_tensors(m.transformer_encoder), rollout=True)
    assert tokens.shape == (c["B"], 45, 128)
    assert torch.equal(r2.weights, r.weights) and torch.equal(r2.by_segment, r.by_segment) and torch.equal(r2.rollout, r.rollout)
    with pytest.raises(ValueError, match="max_bytes"):
        F_egx.encoder_attention(spec, order, m.task_embed, m.pos_embed.pe, m.ln.weight, m.ln.bias, proj,
                                encoder_layer_tensors(m.transformer_encoder), max_bytes=1000)
