"""-m gpu: the sequence decoder at head dim 256 / 512 and d_model up to 2048 (csrc/wide_decoder_bighead.hip; the three LTA sequence-decoder
models of egot2_amd/hoi_lta_seq.py). The parent of this file's commit refuses every shape below.

Operator level: egx_decoder_attention_fwd / _bwd (exactly the launches the fused decoder makes) against fp64 autograd on the bf16-rounded
operands at the bars of tests/test_gpu_wide2048.py (output 1.5e-2 of max, gradients 1.5e-2 relative L2); NaN-poisoned outputs finite
afterwards, guard rows untouched, two runs bit-equal; the forward's and the backward's dropout masks agree.
decode() level: forward + backward against R (tests/seqdec2048_ref.py) through decoder_dropout_gate.gate at the decoder's bf16 bars, eval
mode and train mode under tests/dropmask.py decoder_masks; one mirror class end to end from clip features.
Generation: items 1, 2 and 4 of tests/test_gpu_generate.py; forced decoding bit-equal to greedy on greedy's tokens; beam search (W = 3)
held to tests/test_gpu_beam.py's items 1 and 2. The measured errors go to profiles/seqdec2048_report.txt."""
import ctypes as C

import pytest
import torch

from oracle import translator_ref as tr
from tests import beam_ref as br, dropmask as dm, greedy_ref as gr
from tests import seqdec2048_ref as s
from tests.test_gpu_wide import _stream

pytestmark = pytest.mark.gpu
_OP_LINES, _DEC_LINES, _GEN_LINES = [], [], []
GUARD = 3           # rows behind every buffer that must keep their sentinel


# ---- 1: the operator ------------------------------------------------------------------------------------------------------------------
def _args(q, k, v, ldq, ldk, ldv, bf16, o, d_o, dq, dk, dv, B, H, dh, Sq, Sk, causal, p=0.0, seed=0):
    from egot2_amd import _lib
    a = _lib.DecAttnArgs()
    a.q, a.k, a.v, a.ldq, a.ldk, a.ldv, a.operands_bf16 = q, k, v, ldq, ldk, ldv, int(bf16)
    a.o, a.ldo, a.d_o, a.dq, a.dk, a.dv = o, H * dh, d_o, dq, dk, dv
    a.B, a.H, a.dh, a.Sq, a.Sk, a.causal = B, H, dh, Sq, Sk, int(causal)
    a.p_drop, a.seed, a.layer, a.site, a.stream = p, seed, 0, 1 if causal else 3, _stream()
    return a


def _elt(t):
    return t.element_size()


def _operands(cuda, B, H, Sq, Sk, dh, causal, f32, seed):
    """The decoder's own layouts: self-attention q | k | v packed in rows of 3d; cross-attention q rows of d, k | v rows of 2d. GUARD rows
    behind each buffer. -> (bufs dict, views dict of (tensor, column offset, ld))."""
    d = H * dh
    g = torch.Generator().manual_seed(seed)
    dt = torch.float32 if f32 else torch.bfloat16
    if causal:
        qkv = torch.randn(B * Sq + GUARD, 3 * d, generator=g).to(cuda).to(dt)
        q = k = v = qkv
        offs, lds = (0, d, 2 * d), (3 * d, 3 * d, 3 * d)
    else:
        q = torch.randn(B * Sq + GUARD, d, generator=g).to(cuda).to(dt)
        k = v = torch.randn(B * Sk + GUARD, 2 * d, generator=g).to(cuda).to(dt)
        offs, lds = (0, 0, d), (d, 2 * d, 2 * d)
    d_o = torch.randn(B * Sq + GUARD, d, generator=g).to(cuda).bfloat16()
    return q, k, v, offs, lds, d_o


def _ref(q, k, v, offs, d_o, B, H, Sq, Sk, dh, causal):
    """fp64 autograd on the operands as the device reads them -> (o, dq, dk, dv) as (B, S, H * dh)."""
    d = H * dh
    Q = q[:B * Sq, offs[0]:offs[0] + d].double().cpu().view(B, Sq, H, dh).permute(0, 2, 1, 3).requires_grad_(True)
    K = k[:B * Sk, offs[1]:offs[1] + d].double().cpu().view(B, Sk, H, dh).permute(0, 2, 1, 3).requires_grad_(True)
    V = v[:B * Sk, offs[2]:offs[2] + d].double().cpu().view(B, Sk, H, dh).permute(0, 2, 1, 3).requires_grad_(True)
    sc = Q @ K.transpose(-1, -2) / dh ** 0.5
    if causal:
        sc = sc.masked_fill(~torch.tril(torch.ones(Sq, Sk, dtype=torch.bool)), float("-inf"))
    o = torch.softmax(sc, -1) @ V
    o.backward(d_o[:B * Sq].double().cpu().view(B, Sq, H, dh).permute(0, 2, 1, 3))
    back = lambda t, S: t.permute(0, 2, 1, 3).reshape(B * S, d)  # noqa: E731
    return back(o.detach(), Sq), back(Q.grad, Sq), back(K.grad, Sk), back(V.grad, Sk)


OP_SHAPES = [  # (B, H, Sq, Sk, dh, causal, fp32 operands)
    (3, 1, 1, 1, 256, True, False),        # one token
    (2, 2, 8, 8, 256, True, False),        # a full target tile
    (5, 8, 3, 3, 256, True, False),        # 40 waves at d = 2048
    (1, 2, 3, 3, 512, True, False),        # a partial workgroup
    (2, 2, 8, 8, 256, True, True),         # layer 0: fp32 q / k / v and gradients
    (1, 2, 3, 3, 512, True, True),
    (3, 4, 1, 2, 512, False, False),       # the shipped recipe's memory of 2
    (2, 1, 8, 16, 512, False, False),      # a full tile
    (2, 2, 5, 7, 256, False, False),       # ragged on both sides
]


@pytest.mark.parametrize("B,H,Sq,Sk,dh,causal,f32", OP_SHAPES)
def test_bighead_decoder_attention_fwd_bwd(egx_lib, cuda, B, H, Sq, Sk, dh, causal, f32):
    d = H * dh
    q, k, v, offs, lds, d_o = _operands(cuda, B, H, Sq, Sk, dh, causal, f32, 13 * Sq + Sk + dh)
    es = _elt(q)
    nan = float("nan")
    outs = [torch.full((B * Sq + GUARD, d), nan, device=cuda, dtype=torch.bfloat16) for _ in range(2)]
    gq, gk, gv = (torch.full_like(t, nan) for t in (q, k if not causal else q, v if not causal else q))
    if causal:
        gk = gv = gq            # the packed d(qkv) rows
    sentinel = -7.5
    for t in outs + [gq, gk, gv]:
        t[-GUARD:] = sentinel
    p = lambda t, off=0: t.data_ptr() + off * es  # noqa: E731

    def run(o):
        a = _args(p(q, offs[0]), p(k, offs[1]), p(v, offs[2]), *lds, not f32, o.data_ptr(), d_o.data_ptr(), p(gq, offs[0]), p(gk, offs[1]), p(gv, offs[2]),
                  B, H, dh, Sq, Sk, causal)
        assert egx_lib.egx_decoder_attention_fwd(C.byref(a)) == 0, egx_lib.egx_last_error()
        return a

    a = run(outs[0])
    assert egx_lib.egx_decoder_attention_bwd(C.byref(a)) == 0, egx_lib.egx_last_error()
    run(outs[1])
    torch.cuda.synchronize()
    ro, rq, rk, rv = _ref(q, k, v, offs, d_o, B, H, Sq, Sk, dh, causal)
    got_o = outs[0][:B * Sq].double().cpu()
    got = [gq[:B * Sq, offs[0]:offs[0] + d], gk[:B * Sk, offs[1]:offs[1] + d], gv[:B * Sk, offs[2]:offs[2] + d]]
    finite = bool(torch.isfinite(got_o).all()) and all(bool(torch.isfinite(t.float()).all()) for t in got)
    e_o = (got_o - ro).abs().max().item() / ro.abs().max().item()
    # (one key: softmax is constant, dq and dk are exact zeros: the error is then the norm itself)
    e_g = [((t.double().cpu() - r).norm() / (r.norm() if r.norm() > 0 else 1.0)).item() if finite else nan for t, r in zip(got, (rq, rk, rv))]
    line = (f"(B, H, Sq, Sk, dh) = ({B}, {H}, {Sq}, {Sk}, {dh}) {'self' if causal else 'cross'} {'fp32' if f32 else 'bf16'}: out {e_o:.3e} (bar 1.5e-2) "
            f"dq {e_g[0]:.3e} dk {e_g[1]:.3e} dv {e_g[2]:.3e} (1.5e-2)")
    print("SEQDEC2048 operator", line)
    _OP_LINES.append(line)
    s.record("gpu operator: egx_decoder_attention_fwd / _bwd against fp64 autograd on the operands as read", _OP_LINES)
    assert finite, "an output element was left unwritten (NaN poison)"
    assert e_o < 1.5e-2, line                                      # O rounded to bf16
    assert all(e < 1.5e-2 for e in e_g), line
    assert torch.equal(outs[0], outs[1])                           # bit-reproducible
    for t in outs + [gq, gk, gv]:
        assert bool((t[-GUARD:].float() == sentinel).all()), "a guard row was written"
    if causal:      # the head columns only: nothing else of the packed rows (there is none: 3 H dh = the row) and no q / k / v operand changed
        assert bool(torch.isfinite(q.float()).all())


@pytest.mark.parametrize("dh,Sq,Sk,causal", [(256, 8, 16, False), (512, 5, 5, True)])
def test_bighead_decoder_attention_dropout_is_consistent(egx_lib, cuda, dh, Sq, Sk, causal):
    """p = 0.5: the backward regenerates the forward's mask (tests/test_gpu_wide2048.py test_bighead_attention_dropout_is_consistent's
    method: with V := 1 the output is the row sum of the dropped probabilities, with dO := 1 dV is their column sum; both sum to the same
    total per (clip, head), and the keep rate is 1 - p), and the mask is the one tests/dropmask.py restates."""
    B, H, p, seed = 8, 2, 0.5, 1234
    d = H * dh
    q, k, v, offs, lds, _ = _operands(cuda, B, H, Sq, Sk, dh, causal, False, 11 + Sq)
    v[:, offs[2]:offs[2] + d] = 1.0
    out = torch.empty(B * Sq + GUARD, d, device=cuda, dtype=torch.bfloat16)
    es = _elt(q)
    pp = lambda t, off=0: t.data_ptr() + off * es  # noqa: E731
    gq = torch.full_like(q, float("nan"))
    gk = gq if causal else torch.full_like(k, float("nan"))
    d_o = torch.ones(B * Sq + GUARD, d, device=cuda, dtype=torch.bfloat16)
    a = _args(pp(q, offs[0]), pp(k, offs[1]), pp(v, offs[2]), *lds, True, out.data_ptr(), d_o.data_ptr(), pp(gq, offs[0]), pp(gk, offs[1]), pp(gk, offs[2]),
              B, H, dh, Sq, Sk, causal, p, seed)
    assert egx_lib.egx_decoder_attention_fwd(C.byref(a)) == 0, egx_lib.egx_last_error()
    assert egx_lib.egx_decoder_attention_bwd(C.byref(a)) == 0, egx_lib.egx_last_error()
    torch.cuda.synchronize()
    rowsum = out[:B * Sq].float()[:, ::dh].view(B, Sq, H)          # one column per head: sum_k P_drop[q, k]
    assert abs(rowsum.mean().item() - 1.0) < 0.3 and rowsum.std().item() > 0.01
    dv = gk[:B * Sk, offs[2]:offs[2] + d].float()
    assert torch.isfinite(dv).all()
    dv = dv[:, ::dh].view(B, Sk, H)
    assert torch.allclose(dv.sum(1), rowsum.sum(1), rtol=2e-2, atol=2e-2)
    # the mask itself: P_drop = P * keep-scale of the decoder's keying (rows (b * H + h) * 8 + i, column j)
    masks = dm.decoder_masks(seed, "fused", B, Sq, Sk, d, H, s.D_FF, 1, p, 0.0)["layers"][0]["self" if causal else "cross"]      # (B, H, Sq, Sk)
    Q = q[:B * Sq, offs[0]:offs[0] + d].double().cpu().view(B, Sq, H, dh).permute(0, 2, 1, 3)
    K = k[:B * Sk, offs[1]:offs[1] + d].double().cpu().view(B, Sk, H, dh).permute(0, 2, 1, 3)
    sc = Q @ K.transpose(-1, -2) / dh ** 0.5
    if causal:
        sc = sc.masked_fill(~torch.tril(torch.ones(Sq, Sk, dtype=torch.bool)), float("-inf"))
    want = (torch.softmax(sc, -1) * masks.double()).sum(-1).permute(0, 2, 1)        # (B, Sq, H)
    assert (rowsum.double().cpu() - want).abs().max().item() < 1.5e-2 * max(1.0, want.abs().max().item())


# ---- 2: decode() against R --------------------------------------------------------------------------------------------------------------
def _decode_case(cuda, case, train, tag):
    kind, d, heads, L, sy, S, B = case
    seed, masks, p = None, None, 0.0
    if train:
        seed, p = 0x5EEDDEC0DE + 7, 0.1
        masks = dm.decoder_masks(seed, "fused", B, sy, S, d, heads, s.D_FF, L, 0.1, 0.1)
    data = s.case_data(kind, d, heads, L, sy, S, B, masks=masks)
    res = s.gpu_decode_run(data, cuda, train=train, seed=seed)
    assert res["impl"] == "fused"
    ref = s.oracle_run(data, True, masks=masks)
    g = s.gate(res, ref, s.BF16_BAR)
    line = s.gate_line(f"{tag} {kind} d = {d}, heads = {heads}, L = {L}, sy = {sy}, S = {S}, B = {B}, p = {p:g}", g)
    print("SEQDEC2048 decode", line)
    _DEC_LINES.append(line)
    s.record("gpu decode(): device against R at the decoder's bf16 bars", _DEC_LINES)
    assert g["ok"], line
    return data, res


@pytest.mark.parametrize("case", s.DECODE_CASES, ids=lambda c: f"{c[0]}-d{c[1]}-h{c[2]}-L{c[3]}-sy{c[4]}-S{c[5]}")
def test_decode_fwd_bwd_against_the_rounded_oracle(egx_lib, cuda, case):
    _decode_case(cuda, case, False, "eval")


def test_decode_train_mode_under_the_drawn_masks(egx_lib, cuda):
    """p_drop 0.1 / p_pos 0.1 (the forecasting models' own rates) under the masks tests/dropmask.py decoder_masks restates, on the same
    bars; two runs under one seed are bit-equal."""
    data, res = _decode_case(cuda, s.DECODE_CASES[0], True, "train")
    res2 = s.gpu_decode_run(data, cuda, train=True, seed=0x5EEDDEC0DE + 7)
    assert torch.equal(res["logits"], res2["logits"]) and torch.equal(res["dmem"], res2["dmem"])
    assert all(torch.equal(res["grads"][k], res2["grads"][k]) for k in res["grads"])


def test_mirror_end_to_end_from_clip_features(egx_lib, cuda):
    """ForecastingEncoderSeparateSeqDecoder from clip features: the encoder on the wide path (head dim 256, S = 2) + the decoder, forward and
    backward against R on the whole model (every weight matrix and the features rounded); then predict_features' verb / noun heads."""
    from egot2_amd import functional as F_egx
    from tests.util import seeded_feats, seeded_state_dict
    d, heads, L, n, B, V = 512, 2, 1, 2, 3, 12
    m = s.new_model("fcst", d, heads, L, V, n, cls="ForecastingEncoderSeparateSeqDecoder")
    sd = seeded_state_dict(m, s.W_SEED)
    sd["embedding.weight"] = sd["embedding.weight"] * s.EMB_SCALE
    feats = s.bf16_round(seeded_feats(s.F_SEED, [(B, n, d)])[0])
    y = torch.tensor([[2], [3], [2]])          # lta_verb, lta_noun, lta_verb
    w = seeded_feats(s.F_SEED + 1, [(1, B, V)])[0]

    def oracle(sdd, f):
        x = tr.encode_prepare(f, None, None, sdd["ln.weight"], sdd["ln.bias"], None, sdd["pos_embed.pe"][:n, 0, :])
        mem = tr.encoder(x, sdd, "transformer_encoder.", L, heads).permute(1, 0, 2)
        return tr.g_decode(sdd, heads, y, mem)

    rsd = s.rounded(sd)
    sdd = {k: v.double().requires_grad_(v.is_floating_point() and not k.endswith(".pe")) for k, v in rsd.items()}
    ref = oracle(sdd, feats.double())
    (ref * w.double()).sum().backward()
    m.load_state_dict(rsd)
    m = m.to(cuda).set_compute("bf16").eval()
    logits = m.decode(y.to(cuda), m.encode_features(feats.to(cuda)))
    assert F_egx.last_encoder_impl() == "wide" and F_egx.last_decoder_impl() == "fused"
    (logits * w.to(cuda)).sum().backward()
    torch.cuda.synchronize()
    e_l = (logits.double().cpu() - ref.detach()).abs().max().item() / max(1.0, ref.abs().max().item())
    errs = {k: ((p.grad.double().cpu() - sdd[k].grad).norm() / sdd[k].grad.norm()).item() for k, p in m.named_parameters() if sdd[k].grad is not None}
    worst = max(errs, key=errs.get)
    line = f"mirror end to end, d = {d}, heads = {heads}, n = {n}, B = {B}: logits {e_l:.3e} (bar 1.5e-2), worst gradient {errs[worst]:.3e} ({worst}, bar 8e-2)"
    print("SEQDEC2048 mirror", line)
    s.record("gpu mirror: ForecastingEncoderSeparateSeqDecoder from clip features against R", [line])
    assert e_l < s.BF16_BAR["logits"], line
    assert len(errs) >= 30 and errs[worst] < s.BF16_BAR["grad"], line
    with torch.no_grad():
        pv, pn = m.predict_features(feats.to(cuda))
        v_idx, n_idx = s.idx_maps(V)
        assert pv.shape == (B, 1, len(v_idx)) and pn.shape == (B, 1, len(n_idx))
        rv = oracle({k: v.detach() for k, v in sdd.items()}, feats.double())     # y = lta_verb for clips 0 and 2
        assert (pv[0, 0].double().cpu() - rv[0, 0, v_idx]).abs().max().item() < s.BF16_BAR["logits"] * max(1.0, rv.abs().max().item())


# ---- 3: generation ----------------------------------------------------------------------------------------------------------------------
def _items_1_2(tokens, logits, sd64, h, start, mem64, allowed):
    """Items 1 and 2 of tests/test_gpu_generate.py; under a schedule over the step's word set (the call's logits are -inf elsewhere)."""
    tok, log = tokens.cpu(), logits.cpu()
    n, B, V = log.shape
    assert tok.shape == (B, n) and tok.dtype == torch.int64
    assert torch.equal(tok, gr.argmax_lowest(log).permute(1, 0)), "item 1: tokens are not the argmax of the call's own logits"
    ref = gr.teacher_forced(sd64, h, torch.full((B,), start, dtype=torch.int64), tok, mem64)
    bound = 4e-2 * max(1.0, ref.abs().max().item())
    if allowed is not None:
        on = allowed[torch.arange(n) % allowed.shape[0]][:, None, :].expand(n, B, V)
        assert bool((log[~on] == float("-inf")).all()) and bool(on.gather(2, tok.permute(1, 0)[..., None]).all())
        ref = ref.masked_fill(~on, float("-inf"))
        err = (log.double() - ref)[on].abs().max().item()
    else:
        err = (log.double() - ref).abs().max().item()
    chosen = ref.gather(2, tok.permute(1, 0)[..., None])[..., 0]
    gap = (ref.max(dim=-1).values - chosen).max().item()
    assert err < bound, (err, bound)
    assert gap < 2 * bound, (gap, bound)
    return err, bound, gap


@pytest.mark.parametrize("name", list(s.GEN_CASES))
def test_generate_holds_items_1_2_4_and_forced_is_bit_equal(egx_lib, cuda, name):
    from egot2_amd import functional as F_egx
    d, h, L, V, S, B, n, ws, fs, sched, item4 = s.GEN_CASES[name]
    m, sd64, start, mem64, allowed = s.build_gen_case(name)
    m = m.to(cuda).set_compute("bf16").eval()
    mem = mem64.float().to(cuda)
    with torch.no_grad():
        schedule = m.token_schedule(allowed) if sched else None
        tokens, logits = m.greedy_decode(mem, start, n, return_logits=True, schedule=schedule)
        assert F_egx.last_decoder_impl() == "generate"
        err, bound, gap = _items_1_2(tokens, logits, sd64, h, start, mem64, allowed)
        # forced decoding on greedy's tokens: the same cached step, the same bits
        y = torch.cat((torch.full((B, 1), start, dtype=torch.int64, device=cuda), tokens[:, :-1]), dim=1)
        forced = m.forced_decode(mem, y)
        assert F_egx.last_decoder_impl() == "forced"
        if allowed is None:
            assert torch.equal(forced, logits), "forced decoding differs from greedy on greedy's tokens"
        else:
            on = allowed[torch.arange(n) % 2][:, None, :].expand(n, B, V).to(cuda)
            assert torch.equal(forced[on], logits[on]), "forced decoding differs from greedy on greedy's tokens"
    line = f"{name} (d {d}, heads {h}, L {L}, V {V}, S {S}, B {B}, {n} steps): max|logits - oracle| {err:.3e} (bound {bound:.3e}), chosen-token gap {gap:.3e}"
    if item4:
        rt, rl, rm = gr.greedy(sd64, h, torch.full((B,), start, dtype=torch.int64), mem64, n)
        dec_clips = gr.decided(rm, 4e-2 * max(1.0, rl.abs().max().item()))
        share, distinct = dec_clips.float().mean().item(), sorted(set(rt[dec_clips].flatten().tolist()))
        line += f"; item 4: decided share {share:.2f}, tokens among them {distinct}"
        assert share >= 0.5 and len(distinct) >= 2, (share, distinct)
        assert torch.equal(tokens.cpu()[dec_clips], rt[dec_clips]), "item 4: a decided clip's sequence differs from the oracle's greedy sequence"
    print("SEQDEC2048 generate", line)
    _GEN_LINES.append(line)
    s.record("gpu generation: greedy against the fp64 oracle teacher-forced on the device's tokens", _GEN_LINES)


def test_beam_width_three_holds_the_beam_items(egx_lib, cuda):
    """W = 3 at d = 512, 2 heads of 256 (the head's LDS fits): items 1 and 2 of tests/test_gpu_beam.py, and W = 1 is greedy."""
    from egot2_amd import functional as F_egx
    from tests.test_gpu_beam import _ancestry_logits, _check_selection
    name, W = "d512_h2_v12", 3
    d, h, L, V, S, B, n = s.GEN_CASES[name][:7]
    m, sd64, start, mem64, _ = s.build_gen_case(name)
    m = m.to(cuda).set_compute("bf16").eval()
    mem = mem64.float().to(cuda)
    with torch.no_grad():
        tokens, scores, trace = m.beam_decode(mem, start, n, W, return_scores=True, return_trace=True)
        assert F_egx.last_decoder_impl() == "beam"
        one = m.beam_decode(mem, start, n, 1)
        assert torch.equal(one[:, 0], m.greedy_decode(mem, start, n))
    out = dict(tokens=tokens.cpu(), scores=scores.cpu(), **{k: getattr(trace, k).cpu() for k in trace.__slots__})
    back, _ = br.backtrack(out["step_tokens"], out["step_parents"])
    assert torch.equal(out["tokens"], back) and torch.equal(out["scores"], out["step_scores"][-1])
    _check_selection(out, W, V)
    rows = B * W
    ref = gr.teacher_forced(sd64, h, torch.full((rows,), start, dtype=torch.int64), out["tokens"].view(rows, n), mem64.repeat_interleave(W, dim=1))
    bound = 4e-2 * max(1.0, ref.abs().max().item())
    err = (_ancestry_logits(out).double() - ref).abs().max().item()
    print(f"SEQDEC2048 beam W = 3: max|logits - oracle| = {err:.3e} (bound {bound:.3e})")
    assert err < bound, (err, bound)
    # against tests/beam_ref.py beam itself: a candidate's score after step t carries up to (t + 1) * 2 * bound of logit error (item 2's score
    # bound), so a clip's W hypotheses must equal the fp64 beam's only where every gap between adjacent candidates of step t exceeds twice
    # that. With bound ~ 0.1 the gaps of these seeded models (median ~ 0.1 nats) decide few clips or none, as tests/test_gpu_beam.py found
    # for its own cases: equality is asserted on the decided clips, the shares are printed, and the checks above carry the case.
    rt, rs, _, gaps = br.beam(sd64, h, torch.full((B,), start, dtype=torch.int64), mem64, n, W)
    need = 2 * 2 * bound * torch.arange(1, n + 1, dtype=torch.float64)[:, None, None]
    decided = (gaps > need).all(dim=2).all(dim=0)                                       # (B,)
    assert torch.equal(out["tokens"][decided], rt[decided]), "a decided clip's hypotheses differ from tests/beam_ref.py beam"
    best = (out["tokens"][:, 0] == rt[:, 0]).all(dim=-1).float().mean().item()
    whole = (out["tokens"] == rt).all(dim=-1).all(dim=-1).float().mean().item()
    serr = (out["scores"].double() - rs)[(out["tokens"] == rt).all(dim=-1)].abs().max().item() if whole > 0 or best > 0 else 0.0
    line = (f"beam W = 3 against beam_ref.beam: {int(decided.sum())} of {B} clips decided (all equal); best hypothesis equal on {best:.2f}, all three on "
            f"{whole:.2f} of the clips; max|score - oracle score| on equal hypotheses {serr:.3e} (bound {n * 2 * bound:.3e})")
    print("SEQDEC2048", line)
    s.record("gpu beam: W = 3 against tests/beam_ref.py", [line])
    assert serr < n * 2 * bound, line


# ---- 4: the mirrors against the recorded REAL classes, and the egx_generate switch --------------------------------------------------------
def _recorded(name):
    import json
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live", name + ".npz"))
    return json.loads(str(z["config"])), {k: torch.from_numpy(z[k]) for k in z.files if k != "config"}


def _mirror_of(c, cuda):
    sd64, feats, y = s.recording_inputs(c)
    m = s.new_model(c["kind"], c["d"], c["h"], c["L"], c["V"], c["n"], cls=c["cls"] if c["kind"] == "fcst" else None)
    m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in sd64.items()})
    return m.to(cuda).set_compute("bf16").eval(), [f.float().to(cuda) for f in feats], y.to(cuda)


@pytest.mark.parametrize("name", list(s.RECORDINGS))
def test_mirrors_against_the_recorded_real_classes(egx_lib, cuda, name):
    """tests/golden/live/seqdec_*.npz: forward and predict of the REAL classes in fp64 (tests/golden/make_golden_seqdec.py). The mirror on
    the same seeded weights and clip features, compute bf16, within 4e-2 * max(1, max|ref|): the bound tests/test_gpu_generate.py (item 2)
    holds the bf16 decoder to against the fp64 oracle on unrounded weights. The 40-step class: its default loop step by step for as long as
    the device's fed-back tokens equal the recorded ones (step 0 always)."""
    from egot2_amd import functional as F_egx
    c, rec = _recorded(name)
    m, feats, y = _mirror_of(c, cuda)
    bound = 4e-2 * max(1.0, rec["forward"].abs().max().item())
    with torch.no_grad():
        fwd = m.forward_features(*feats, y)
        assert F_egx.last_encoder_impl() == "wide" and F_egx.last_decoder_impl() == "fused"
        pv, pn = m.predict_features(*feats)
    e_f = (fwd.double().cpu() - rec["forward"]).abs().max().item()
    assert fwd.shape == rec["forward"].shape and pv.shape == rec["pred_verb"].shape and pn.shape == rec["pred_noun"].shape
    if c["steps"]:
        # step t's verb / noun rows saw the recorded prefix while every earlier full-vocabulary argmax (which the default loop feeds back) equals
        # the recorded token; the recorded argmax is decided where its margin exceeds twice the bound
        toks, margins = rec["step_tokens"], rec["step_margins"]
        ok = torch.ones(c["B"], dtype=torch.bool)
        same = []
        for t in range(c["steps"]):
            same.append(ok.clone())
            ok &= margins[t] > 2 * bound
        same = torch.stack(same, 0)                                                  # (steps, B)
        ev = ((pv.double().cpu() - rec["pred_verb"]).abs().max(-1).values.permute(1, 0) * same[0::2]).max().item()
        en = ((pn.double().cpu() - rec["pred_noun"]).abs().max(-1).values.permute(1, 0) * same[1::2]).max().item()
        compared = int(same.sum())
        assert compared >= c["B"]
    else:
        ev = (pv.double().cpu() - rec["pred_verb"]).abs().max().item()
        en = (pn.double().cpu() - rec["pred_noun"]).abs().max().item()
        compared = c["B"]
    line = f"{name}: forward {e_f:.3e}, predict verbs {ev:.3e}, nouns {en:.3e} (bound {bound:.3e}; {compared} (step, clip) rows compared)"
    print("SEQDEC2048 recorded", line)
    s.record(f"gpu mirrors against the recorded real classes: {name}", [line])
    assert e_f < bound and ev < bound and en < bound, line


def test_egx_generate_switch_of_the_forty_step_predict(egx_lib, cuda):
    """egx_generate = True (eval mode): predict_features is ONE scheduled greedy_decode call. Against the default prefix loop, restated here
    with the full logits of every step (and asserted equal to the default predict_features bit for bit): shapes are the loop's; the verb /
    noun rows of a clip agree within 3e-2 * max(1, max|ref|) (item 3's bound of tests/test_gpu_generate.py: the same arithmetic at other GEMM
    row counts) at every step up to and including the first one whose full-vocabulary argmax is not decidedly inside the step's word set.
    From there the two may differ: the loop feeds back the full-vocabulary argmax, the schedule the set's."""
    from egot2_amd import functional as F_egx
    c, _ = _recorded("seqdec_fcst_d256_h1")
    m, feats, _ = _mirror_of(c, cuda)
    B, n, V = c["B"], 40, c["V"]
    # wide word sets (all words but one each), so that the full-vocabulary argmax the loop feeds back mostly lies in the step's set and the
    # two paths share their prefixes over many steps; the narrow sets of s.idx_maps would part them at step 0
    v_idx, n_idx = [w for w in range(V) if w != 0], [w for w in range(V) if w != 1]
    m.v_idx, m.n_idx = v_idx, n_idx
    with torch.no_grad():
        mem = m.encode_features(*feats)
        toks = torch.full((B, n + 1), m.vocab['action'], dtype=torch.int64, device=cuda)
        rows = []
        for t in range(n):
            rows.append(m.decode(toks[:, :t + 1], mem)[-1])
            toks[:, t + 1] = torch.argmax(rows[-1], dim=-1)
        full = torch.stack(rows, 0)                                                   # (n, B, V)
        lv, ln_ = m.predict_features(*feats)
        assert F_egx.last_decoder_impl() in ("fused", "forced")
        assert torch.equal(lv, full[0::2][:, :, v_idx].permute(1, 0, 2)) and torch.equal(ln_, full[1::2][:, :, n_idx].permute(1, 0, 2))
        m.egx_generate = True
        gv, gn = m.predict_features(*feats)
        assert F_egx.last_decoder_impl() == "generate"
    assert gv.shape == lv.shape == (B, n // 2, len(v_idx)) and gn.shape == ln_.shape == (B, n // 2, len(n_idx)) and gv.dtype == lv.dtype
    bound = 3e-2 * max(1.0, full.abs().max().item())
    allowed = torch.zeros((2, V), dtype=torch.bool)
    allowed[0, v_idx] = True
    allowed[1, n_idx] = True
    fc = full.cpu()
    top = fc.argmax(-1)                                                               # (n, B)
    inside = allowed[torch.arange(n) % 2][:, None, :].expand(n, B, V).gather(2, top[..., None])[..., 0] & (gr.top2_margin(fc) > 2 * bound)
    same, ok = [], torch.ones(B, dtype=torch.bool)
    for t in range(n):
        same.append(ok.clone())
        ok &= inside[t]
    same = torch.stack(same, 0)
    ev = ((gv - lv).abs().max(-1).values.permute(1, 0).cpu() * same[0::2]).max().item()
    en = ((gn - ln_).abs().max(-1).values.permute(1, 0).cpu() * same[1::2]).max().item()
    line = f"scheduled greedy_decode against the prefix loop: verbs {ev:.3e}, nouns {en:.3e} (bound {bound:.3e}) over {int(same.sum())} of {n * B} (step, clip) rows"
    print("SEQDEC2048 switch", line)
    s.record("gpu egx_generate: the 40-step predict through one scheduled greedy_decode", [line])
    assert int(same.sum()) >= 2 * B and ev < bound and en < bound, line


@pytest.mark.parametrize("name", ["seqdec_sep_d512_h1", "seqdec_lta2_d512_h2"])
def test_egx_generate_switch_of_generate(egx_lib, cuda, name):
    """generate(x, k) from the video entry with pass-through backbones: with the switch the draws come from functional.lta_validate. k = 1:
    the row argmax, equal to the default path's tokens; k = 3: (B, 3, Z) int64 tokens inside each head, repeatable under one seed only by
    the library's generator (two calls differ somewhere or the heads are saturated: not asserted), every drawn word of positive probability."""
    c, _ = _recorded(name)
    m, feats, _ = _mirror_of(c, cuda)
    if c["kind"] == "lta2":
        m.action_model = lambda pathways: pathways[0]
        m.lta_model = lambda x, *a, **k: x[1].transpose(0, 1)
        x = feats
    else:
        m.backbone = lambda pathways: pathways[0]
        x = [feats[0]]
    with torch.no_grad():
        preds = m.predict(x)
        want = [p.argmax(2)[:, None] for p in preds]
        base = m.generate(x, k=1)
        m.egx_generate = True
        one = m.generate(x, k=1)
        three = m.generate(x, k=3)
    assert len(one) == len(three) == 2
    for h in range(2):
        assert torch.equal(base[h], want[h]) and torch.equal(one[h], want[h]) and one[h].dtype == torch.int64 and one[h].shape == (c["B"], 1, 1)
        assert three[h].shape == (c["B"], 3, 1) and three[h].dtype == torch.int64
        assert int(three[h].min()) >= 0 and int(three[h].max()) < preds[h].shape[-1]
