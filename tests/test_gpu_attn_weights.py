"""-m gpu: the decoder's cross-attention weights as an output (egx_cross_attention_weights, egx_decoder_cross_weights,
egx_decoder_generate_attn through decode(..., return_attention=True) / greedy_decode(..., return_attention=True)): the head-averaged
weights a forward hook on the reference's CustomDecoderLayer.multihead_attn sees.
  1. the primitive alone on bf16-representable inputs against an fp64 softmax: max |w - ref| < 2e-6 (the bar's condition is checked on the
     CPU, tests/test_cpu_attn_weights.py), rows sum to 1 within 1e-6, entries beyond a clip's keys exactly 0;
  2. decode(..., return_attention=True) against the fp64 oracle (tests/attn_ref.py) and the recordings of the real classes: with
     e = max |w - w*| and s = max |w* - 1 / S|, e < s / 4 (an answer that ignores the scores fails by 4x) and e < 4 x the worst e measured
     on the MI355X over these cases (ORACLE_E_MEASURED); the logits equal the call's without the flag bit for bit;
  3. the composed decoder at the same bars;  4. ragged memories;  5. generation;  6. independence of the clips.
Measured on an MI355X (every test prints its figures), e / s per case of item 2: d256_h4_v40 2.05e-4 / 3.75e-2, c5_hoi 1.13e-4 / 1.73e-2,
long_memory 2.96e-4 / 4.14e-2, one_clip 4.45e-4 / 4.35e-2, attn_ref_hhi_g 2.78e-4 / 3.28e-2, attn_ref_hoi_g 1.23e-4 / 1.84e-2, sharpened
2.32e-3 / 1.89e-1 (e is 0.5 .. 1.2 % of s); item 3: f32 composed 6.4e-8 / 5.36e-2, bf16 composed 3.04e-4 / 8.14e-2; item 4: ragged clips
1.70e-3 / 3.48e-1 (S_b = 3), 2.37e-4, 3.52e-4, 4.39e-4, grouped against ragged 1.32e-3; item 5: greedy against decode(prefix) 0 (the same
bits), against the oracle 3.73e-4 / 6.66e-2 (n = 4) and 5.99e-4 / 9.64e-2 (n = 40); item 1: 7.7e-8 .. 2.0e-7."""
import json
import os

import numpy as np
import pytest
import torch

from tests import attn_ref as ar
from tests import greedy_ref as gr
from tests.util import seeded_feats

pytestmark = pytest.mark.gpu

# the worst max |w - oracle| of item 2's cases on an MI355X (the bf16 decoder's upstream error in q and k; the primitive itself is item 1)
ORACLE_E_MEASURED = 2.322e-3
# item 4: worst |grouped fallback - ragged call| (the grouped path runs the composed decoder: fp32 GEMMs on the target rows)
GROUPED_VS_RAGGED_MEASURED = 1.323e-3
# item 5: worst |greedy step t - row t of decode(prefix)| over n <= 8: measured 0, the q rows of the two calls have the same bits (the bar is <=)
GEN_VS_DECODE_MEASURED = 0.0

_ORACLE = {}


def _oracle(key, sd64, h, y, mem64):
    """fp64 (logits, weights) of a case, computed once and shared (never modified)."""
    if key not in _ORACLE:
        with torch.no_grad():
            _ORACLE[key] = ar.g_decode_attn(sd64, h, y, mem64)
    return _ORACLE[key]


def _hold(w, ref, what, measured=ORACLE_E_MEASURED, S=None):
    """Item 2's two bars on device weights `w` against fp64 `ref` (same shape; last axis the S keys)."""
    S = S or ref.shape[-1]
    e = (w.double().cpu() - ref).abs().max().item()
    s = (ref[..., :S] - 1.0 / S).abs().max().item()
    print(f"[{what}] e = max|w - oracle| = {e:.3e}, s = max|oracle - 1/S| = {s:.3e}, e / s = {e / s:.4f}")
    assert e < s / 4, (what, e, s)
    assert measured is not None, "the bar needs the difference measured on the MI355X"
    assert e < 4 * measured, (what, e, measured)
    return e


# ---- 1. the primitive alone ----
def _ref_weights(q, k, H, B, Sq, Sk, lengths=None, first=None):
    ref = torch.zeros(B, Sq, Sk, dtype=torch.float64)
    for b in range(B):
        n = Sk if lengths is None else min(max(lengths[b], 0), Sk)
        r0 = b * Sk if first is None else first[b]
        if n:
            ref[b, :, :n] = ar.softmax_weights(q[b * Sq:(b + 1) * Sq][None].double(), k[r0:r0 + n][None].double(), H)[0]
    return ref


@pytest.mark.parametrize("H,dh", ar.PRIM_SHAPES)
def test_primitive_against_fp64_softmax(egx_lib, cuda, H, dh):
    from egot2_amd import functional as F_egx
    worst = 0.0
    for Sq, Sk, B in ar.primitive_cases(H, dh):
        q, k = ar.primitive_inputs(H, dh, Sq, Sk, B)
        ref = _ref_weights(q, k, H, B, Sq, Sk)
        for dt in (torch.float32, torch.bfloat16):
            w = F_egx.cross_attention_weights(q.to(cuda, dt), k.to(cuda, dt), H, Sq, Sk)
            assert w.shape == (B, Sq, Sk) and w.dtype == torch.float32
            w = w.cpu().double()
            e = (w - ref).abs().max().item()
            worst = max(worst, e)
            assert e < 2e-6, (H, dh, Sq, Sk, B, dt, e)
            assert (w.sum(-1) - 1).abs().max().item() < 1e-6, (H, dh, Sq, Sk, B, dt)
    print(f"H = {H}, dh = {dh}: worst max|w - fp64| = {worst:.3e}")


@pytest.mark.parametrize("H,dh", ar.PRIM_SHAPES)
def test_primitive_ragged_table_strided_views_and_the_clamp(egx_lib, cuda, H, dh):
    from egot2_amd import functional as F_egx
    lengths, Sq, Sk, d = [1, 64, 65, 200, 7], 3, 200, H * dh
    B = len(lengths)
    first = [0, 1, 65, 130, 330]
    q, k = ar.primitive_inputs(H, dh, Sq, Sk, B, rows=sum(lengths) + 300)      # (rows behind the last clip: the clamp's reads stay inside)
    tab = torch.tensor([[f, n] for f, n in zip(first, lengths)], dtype=torch.int32)
    ref = _ref_weights(q, k, H, B, Sq, Sk, lengths, first)
    for dt in (torch.float32, torch.bfloat16):
        # k as the first d columns of a packed (rows, 2d) k | v buffer, q as the first d of (rows, 3d): read in place through the strides
        kv = torch.cat((k, torch.full_like(k, float("nan"))), 1).to(cuda, dt)
        q3 = torch.cat((q, torch.full((q.shape[0], 2 * d), float("nan"))), 1).to(cuda, dt)
        out = F_egx.cross_attention_weights(q3[:, :d], kv[:, :d], H, Sq, Sk, mtab=tab.to(cuda)).cpu().double()
        assert (out - ref).abs().max().item() < 2e-6
        for b, n in enumerate(lengths):
            assert (out[b, :, :n].sum(-1) - 1).abs().max().item() < 1e-6
            assert out[b, :, n:].abs().max().item() == 0 if n < Sk else True
        # a table entry above Sk is clamped to Sk, one below zero to no keys at all (a row of zeros)
        tab2 = tab.clone()
        tab2[3, 1] = 260
        tab2[4, 1] = -5
        out2 = F_egx.cross_attention_weights(q3[:, :d], kv[:, :d], H, Sq, Sk, mtab=tab2.to(cuda)).cpu().double()
        assert torch.equal(out2[:4], out[:4]) and out2[4].abs().max().item() == 0 and not torch.isnan(out2).any()
    # ldo > Sk through the C entry: the columns behind Sk stay as they were
    from egot2_amd import _lib
    qd, kd = q[:B * Sq].to(cuda), k[:B * 64].to(cuda)
    buf = torch.full((B * Sq, 72), -7.0, device=cuda)
    _lib.check(egx_lib.egx_cross_attention_weights(qd.data_ptr(), d, kd.data_ptr(), d, 0, None, B, H, dh, Sq, 64, buf.data_ptr(), 72,
                                                   torch.cuda.current_stream().cuda_stream))
    assert torch.equal(buf[:, :64].view(B, Sq, 64), F_egx.cross_attention_weights(qd, kd, H, Sq, 64)) and bool((buf[:, 64:] == -7.0).all())


# ---- 2. end to end against the fp64 oracle and the recordings ----
def _case(name, cuda, factor=None):
    kind, d, h, L, V, S, B, n, ws, fs, _ = gr.CASES[name]
    m, sd64, start, mem64 = gr.build_case(name)
    B = min(B, 16)
    mem64 = mem64[:, :B].contiguous()
    if factor:
        sd64 = ar.sharpen(sd64, factor)
        m.load_state_dict({k: v.float() for k, v in sd64.items()})
    y = torch.randint(0, V, (B, 3), generator=torch.Generator().manual_seed(9))
    y[:, 0] = start
    return m, sd64, h, y, mem64


def _decode_and_hold(m, sd64, h, y, mem64, cuda, what, impl="fused"):
    from egot2_amd import functional as F_egx
    ref_logits, ref = _oracle(what, sd64, h, y, mem64)
    mem = mem64.float().to(cuda)
    with torch.no_grad():
        plain = m.decode(y.to(cuda), mem)
        assert F_egx.last_decoder_impl() == impl
        logits, w = m.decode(y.to(cuda), mem, return_attention=True)
        assert F_egx.last_decoder_impl() == impl
    assert w.shape == ref.shape and w.dtype == torch.float32 and w.is_cuda
    assert torch.equal(logits, plain), "the logits changed with return_attention"
    assert (w.sum(-1) - 1).abs().max().item() < 1e-5
    bound = 4e-2 * max(1.0, ref_logits.abs().max().item())
    assert (logits.double().cpu() - ref_logits).abs().max().item() < bound
    return _hold(w, ref, what), w, ref


@pytest.mark.parametrize("name", ["d256_h4_v40", "c5_hoi", "long_memory", "one_clip"])
def test_decode_weights_against_the_oracle(egx_lib, cuda, name):
    m, sd64, h, y, mem64 = _case(name, cuda)
    _decode_and_hold(m.to(cuda).set_compute("bf16").eval(), sd64, h, y, mem64, cuda, name)


@pytest.mark.parametrize("fixture", list(ar.RECORDINGS))
def test_decode_weights_against_the_recorded_hooks(egx_lib, cuda, fixture):
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live", fixture + ".npz"))
    c = json.loads(str(z["config"]))
    m, sd64, y, mem64, _ = ar.recording_inputs(c)
    assert np.array_equal(y.numpy(), z["tokens"])
    _, w, _ = _decode_and_hold(m.to(cuda).set_compute("bf16").eval(), sd64, c["h"], y, mem64, cuda, fixture)
    _hold(w, torch.from_numpy(z["weights"]), fixture + " (recording)")


def test_decode_weights_of_a_sharpened_model(egx_lib, cuda):
    """Cross-attention q and k projection rows scaled by 1.8 (chosen on the CPU): the oracle's largest weight is above 0.2."""
    m, sd64, h, y, mem64 = _case("d256_h4_v40", cuda, factor=1.8)
    _, _, ref = _decode_and_hold(m.to(cuda).set_compute("bf16").eval(), sd64, h, y, mem64, cuda, "sharpened")
    assert ref.max().item() >= 0.2, ref.max().item()


# ---- 3. the composed decoder ----
@pytest.mark.parametrize("which", ["f32_d128_h8", "bf16_composed"])
def test_composed_path_weights(egx_lib, cuda, which):
    if which == "f32_d128_h8":          # head dim 16: outside the fused decoder
        m, sd64, start = gr.hhi_model(128, 8, 2, 12, 133)
        m = m.to(cuda).set_compute("f32").eval()
        h, d = 8, 128
    else:
        m, sd64, start = gr.hhi_model(256, 4, 2, 12, 134)
        m = m.to(cuda).set_compute("bf16").eval()
        m.egx_composed_decoder = True
        h, d = 4, 256
    B, S = 5, 45
    mem64 = seeded_feats(99, [(S, B, d)])[0].double()
    y = torch.randint(0, 12, (B, 3), generator=torch.Generator().manual_seed(10))
    y[:, 0] = start
    _decode_and_hold(m, sd64, h, y, mem64, cuda, which, impl="composed")


# ---- 4. ragged memories ----
def test_ragged_weights(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    lengths = [3, 64, 65, 130]
    B, d, h = len(lengths), 256, 4
    m, sd64, start = gr.hhi_model(d, h, 2, 12, 135)
    m = m.to(cuda).set_compute("bf16").eval()
    packed64 = seeded_feats(100, [(sum(lengths), d)])[0].double()
    y = torch.randint(0, 12, (B, 2), generator=torch.Generator().manual_seed(11))
    y[:, 0] = start
    with torch.no_grad():
        plain = m.decode(y.to(cuda), packed64.float().to(cuda), lengths)
        assert F_egx.last_decoder_impl() == "ragged"
        logits, w = m.decode(y.to(cuda), packed64.float().to(cuda), lengths, return_attention=True)
        assert F_egx.last_decoder_impl() == "ragged"
    assert torch.equal(logits, plain) and w.shape == (2, B, 2, 130)
    r0 = 0
    for b, n in enumerate(lengths):
        assert w[:, b, :, n:].abs().max().item() == 0 if n < 130 else True
        _, ref = _oracle(("ragged", b), sd64, h, y[b:b + 1], packed64[r0:r0 + n][:, None, :].contiguous())
        _hold(w[:, b:b + 1, :, :n], ref, f"ragged clip {b} (S_b = {n})")
        r0 += n
    # every clip at the full length: the uniform call, bit for bit
    S = 65
    mem = seeded_feats(101, [(S, B, d)])[0].to(cuda)
    with torch.no_grad():
        _, wu = m.decode(y.to(cuda), mem, return_attention=True)
        _, wr = m.decode(y.to(cuda), mem.permute(1, 0, 2).reshape(B * S, d), [S] * B, return_attention=True)
    assert torch.equal(wu, wr), "a full-length ragged batch differs from the uniform call"
    # the grouped fallback (the composed decoder per length group)
    m.egx_composed_decoder = True
    with torch.no_grad():
        lg, wg = m.decode(y.to(cuda), packed64.float().to(cuda), lengths, return_attention=True)
        assert F_egx.last_decoder_impl() == "grouped"
    diff = (wg - w).abs().max().item()
    print(f"grouped vs ragged: max |dw| = {diff:.3e}")
    assert wg.shape == w.shape and all(wg[:, b, :, n:].abs().max().item() == 0 for b, n in enumerate(lengths) if n < 130)
    assert GROUPED_VS_RAGGED_MEASURED is not None and diff < 4 * GROUPED_VS_RAGGED_MEASURED, diff


# ---- 5. generation ----
def _gen_model(cuda):
    m, sd64, start = gr.hoi_model(512, 8, 3, 600, 95)
    m = m.to(cuda).set_compute("bf16").eval()
    sched = m.verb_noun_schedule(list(range(5, 120)), list(range(100, 600)))
    return m, sd64, start, sched


@pytest.mark.parametrize("n", [4, 40])
def test_greedy_weights(egx_lib, cuda, n):
    from egot2_amd import functional as F_egx
    m, sd64, start, sched = _gen_model(cuda)
    B, S, h = 16, 48, 8
    mem64 = seeded_feats(102, [(S, B, 512)])[0].double()
    mem = mem64.float().to(cuda)
    with torch.no_grad():
        tok0, log0 = m.greedy_decode(mem, start, n, return_logits=True, schedule=sched)
        tok, log, w = m.greedy_decode(mem, start, n, return_logits=True, schedule=sched, return_attention=True)
        assert F_egx.last_decoder_impl() == "generate"
        tok1, w1 = m.greedy_decode(mem, start, n, return_attention=True)
        assert torch.equal(tok1, m.greedy_decode(mem, start, n)) and w1.shape == w.shape
    assert torch.equal(tok, tok0) and torch.equal(log, log0), "tokens or logits changed with return_attention"
    assert w.shape == (3, n, B, S) and w.dtype == torch.float32 and (w.sum(-1) - 1).abs().max().item() < 1e-5
    y = torch.cat((torch.full((B, 1), start, dtype=torch.int64, device=cuda), tok[:, :-1]), dim=1)
    if n <= 8:
        with torch.no_grad():
            _, wd = m.decode(y, mem, return_attention=True)             # (L, B, n, S): row t is step t
        diff = (w - wd.permute(0, 2, 1, 3)).abs().max().item()
        print(f"greedy vs decode(prefix) weights, n = {n}: max |dw| = {diff:.3e}")
        assert GEN_VS_DECODE_MEASURED is not None and diff <= 4 * GEN_VS_DECODE_MEASURED, diff
    _, ref = _oracle(("greedy", n, tuple(tok.cpu().flatten().tolist())), sd64, h, y.cpu(), mem64)
    _hold(w.permute(0, 2, 1, 3), ref, f"greedy n = {n}, teacher-forced")


def test_greedy_weights_prefix_loop(egx_lib, cuda):
    """Outside egx_decoder_generate (compute f32s): the prefix loop takes the last row of each step's decode weights."""
    from egot2_amd import functional as F_egx
    m, sd64, start = gr.hoi_model(256, 4, 2, 12, 95)
    m = m.to(cuda).set_compute("f32s").eval()
    B, S, n = 6, 16, 3
    mem = seeded_feats(96, [(S, B, 256)])[0].to(cuda)
    with torch.no_grad():
        tok, w = m.greedy_decode(mem, start, n, return_attention=True)
        assert F_egx.last_decoder_impl() == "loop" and torch.equal(tok, m.greedy_decode(mem, start, n))
        y = torch.cat((torch.full((B, 1), start, dtype=torch.int64, device=cuda), tok[:, :-1]), dim=1)
        _, wd = m.decode(y, mem, return_attention=True)
    assert w.shape == (2, n, B, S) and torch.equal(w, wd.permute(0, 2, 1, 3).contiguous())


def test_captured_greedy_weights_replay_on_new_contents(egx_lib, cuda):
    m, _, start = gr.hoi_model(256, 4, 2, 40, 95)
    m = m.to(cuda).set_compute("bf16").eval()
    B, S, n = 9, 48, 6
    mems = [f.to(cuda) for f in seeded_feats(98, [(S, B, 256)] * 2)]
    starts = [torch.randint(0, 40, (B,), generator=torch.Generator().manual_seed(s)).to(cuda) for s in (5, 6)]
    with torch.no_grad():
        eager = [m.greedy_decode(mems[i], starts[i], n, return_attention=True) for i in range(2)]
        eager = [(t.clone(), a.clone()) for t, a in eager]
        s_mem, s_start = mems[0].clone(), starts[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.greedy_decode(s_mem, s_start, n, return_attention=True)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tok, att = m.greedy_decode(s_mem, s_start, n, return_attention=True)
        for i in (1, 0, 1):
            s_mem.copy_(mems[i])
            s_start.copy_(starts[i])
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(tok, eager[i][0]) and torch.equal(att, eager[i][1]), f"replay on contents {i} differs from the eager call"


# ---- 6. independence ----
def test_permutation_leakage_and_determinism(egx_lib, cuda):
    m, _, start = gr.hoi_model(256, 4, 2, 40, 95)
    m = m.to(cuda).set_compute("bf16").eval()
    B, S, n = 37, 70, 5
    mem = seeded_feats(97, [(S, B, 256)])[0].to(cuda)
    y = torch.randint(0, 40, (B, 4), generator=torch.Generator().manual_seed(3)).to(cuda)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(4)).to(cuda)
    j = 11
    mem2 = mem.clone()
    mem2[:, j] = mem2[:, j] * -1.5 + 0.25
    others = torch.arange(B, device=cuda) != j
    with torch.no_grad():
        for call, axis in ((lambda mm, yy: m.decode(yy, mm, return_attention=True)[1], 1),
                           (lambda mm, yy: m.greedy_decode(mm, yy[:, 0].contiguous(), n, return_attention=True)[1], 2)):
            w = call(mem, y)
            assert torch.equal(w, call(mem, y)), "two calls differ"
            wp = call(mem[:, perm].contiguous(), y[perm])
            assert torch.equal(wp, w.index_select(axis, perm)), "permuting the clips does not permute the weights bit for bit"
            wj = call(mem2, y)
            assert torch.equal(wj.index_select(axis, others.nonzero()[:, 0]), w.index_select(axis, others.nonzero()[:, 0])), "clip j leaked"
            assert not torch.equal(wj.select(axis, j), w.select(axis, j))
