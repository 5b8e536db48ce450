"""-m gpu: teacher-forced decoding of up to 64 target tokens in one call (egx_decoder_forced through DecoderMixin.forced_decode and, for
9 .. 64 tokens at inference, through decode()): greedy generation's K/V-cached step with the next input row taken from the caller's tokens.
Models and memories are those of tests/greedy_ref.py, the oracle is greedy_ref.teacher_forced (one causal fp64 decode). Held to:
  1. greedy's own tokens reproduce greedy's logits bit for bit, for every entry of greedy_ref.CASES, and every logprob equals the fp64
     log_softmax of the call's own logits at the target within eps = 32 * 2^-23 * max(1, |value|, max|row|) (test_gpu_beam.py item 1's
     derived bound: the fp32 max / exp / sum / log chain over at most 1024 words);
  2. arbitrary seeded tokens and targets against the fp64 oracle: logits within 4e-2 * max(1, max|ref|) (the bar of test_gpu_decoder.py and
     test_gpu_generate.py), logprob within twice that bar (a log-probability moves by at most twice the worst logit error), and to eps of
     the fp64 log_softmax of the device's own logits;
  3. against ONE fused decode() of the same rows for 7 and 8 tokens (the existing code; K > 1: its memory repeated per sequence): bound =
     4 x the worst difference measured on the MI355X over these cases (FORCED_VS_DECODE_MEASURED), never looser than 3e-2 * max(1, max|ref|);
  4. K sequences per clip against K calls with one: the GEMMs run over B * K rows against B, so bit equality is not promised; bound kept
     as in item 3 (FORCED_K_VS_ONE_MEASURED, measured 0.0: the bound asks for equality), for the logits and for logprob;
  5. targets outside the vocabulary give logprob exactly 0.0 and move no other bit; an input token of -1 embeds as the zero row;
  6. bit properties: determinism, clip permutation, no leak between clips or sequences, causality (rows before a changed token keep their
     bits), return_logits=False;
  7. the captured call replays on new tokens, targets and memory;
  8. decode() routes 9 .. 64 tokens at inference to the call and nothing else;
  9. beam_decode's scores against the summed logprob of its own hypotheses: within n * 4 * bar (both logit sets lie within bar of the
     oracle, a log-probability moves by at most twice a logit error)."""
import functools
from types import SimpleNamespace as NS

import pytest
import torch

from oracle import translator_ref as tr
from tests import beam_ref as br, greedy_ref as gr
from tests.util import seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu

# items 3 and 4: worst differences over the cases below, measured on an MI355X (profiles/forced_mi355x.json)
FORCED_VS_DECODE_MEASURED = 1.28e-2     # (512-8-3-600-4-37-1-21; four shapes 4.3e-3 .. 9.1e-3 where a bf16 rounding of a row flips between the one-row
                                        # and the B * sy-row GEMMs, the others 1.4e-6 .. 2.4e-6: the bf16 rows agree, the fp32 heads sum in different orders)
FORCED_K_VS_ONE_MEASURED = (0.0, 0.0)   # (logits, logprob): on the MI355X the rows of a (B, K, sy) call have the bits of the K = 1 calls, so the bound of
                                        # item 4 (4 x measured) asks for equality

ULP = 2.0 ** -23
DEV = "cuda:0"


def _eps(value, row_max):
    return 32 * ULP * torch.maximum(torch.ones_like(value), torch.maximum(value.abs(), row_max))


def _own_logprob_check(logits, logprob, targets):
    """logits (n, M, V) fp32, logprob / targets (M, n), every target inside the vocabulary: logprob against the fp64 log_softmax of the
    call's own logits, to eps."""
    l64 = logits.cpu().double()
    want = torch.log_softmax(l64, -1).gather(2, targets.cpu().permute(1, 0)[..., None])[..., 0].permute(1, 0)       # (M, n)
    eps = _eps(want, l64.abs().max(dim=-1).values.permute(1, 0))
    diff = (logprob.cpu().double() - want).abs()
    assert bool((diff <= eps).all()), (diff.max().item(), eps.min().item())
    return (diff / eps).max().item()


@functools.lru_cache(maxsize=None)
def _model(d, h, L, V):
    m, sd64, start = gr.hoi_model(d, h, L, V, 95)
    return m.to(DEV).set_compute("bf16").eval(), sd64, start


def _oracle(sd64, h, y, mem64):
    """fp64 logits (sy, B, V) of input tokens y (B, sy)."""
    return gr.teacher_forced(sd64, h, y[:, 0], torch.cat((y[:, 1:], y[:, :1]), dim=1), mem64)


# ---- item 1 ----
@pytest.mark.parametrize("name", list(gr.CASES))
def test_greedys_tokens_reproduce_greedys_logits_bit_for_bit(egx_lib, cuda, name):
    from egot2_amd import functional as F_egx
    kind, d, h, L, V, S, B, n, ws, fs, _ = gr.CASES[name]
    m, sd64, start, mem64 = gr.build_case(name)
    m = m.to(cuda).set_compute("bf16").eval()
    mem = mem64.float().to(cuda)
    with torch.no_grad():
        tokens, logits = m.greedy_decode(mem, start, n, return_logits=True)
        y = torch.cat((torch.full((B, 1), start, dtype=torch.int64, device=cuda), tokens[:, :-1]), dim=1)
        got, logprob = m.forced_decode(mem, y, targets=tokens)
        assert F_egx.last_decoder_impl() == "forced"
    assert got.shape == (n, B, V) and logprob.shape == (B, n) and logprob.dtype == torch.float32
    assert torch.equal(got, logits), f"forced logits differ from greedy's: max diff {(got - logits).abs().max().item():.3e}"
    worst = _own_logprob_check(got, logprob, tokens)
    print(f"item 1 [{name}]: logits bit-equal; worst |logprob - fp64 log_softmax| / eps = {worst:.3f}")


# ---- items 2, 3 ----
# (d, heads, L, V, S, B, K, sy)
SHAPES = [(256, 4, 2, 12, 16, 5, 1, 9), (256, 4, 2, 40, 65, 3, 1, 21), (512, 8, 3, 600, 4, 37, 1, 21), (256, 8, 2, 1024, 1, 2, 1, 64),
          (256, 4, 2, 40, 64, 6, 5, 7), (512, 8, 3, 12, 48, 3, 8, 40)]


def _inputs(shape):
    d, h, L, V, S, B, K, sy = shape
    g = torch.Generator().manual_seed(1000 + sum(shape))
    y = torch.randint(0, V, (B, K, sy), generator=g)
    targets = torch.randint(0, V, (B, K, sy), generator=g)
    mem64 = seeded_feats(96, [(S, B, d)])[0].double()
    return y, targets, mem64


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_arbitrary_targets_against_the_fp64_oracle(egx_lib, cuda, shape):
    d, h, L, V, S, B, K, sy = shape
    m, sd64, _ = _model(d, h, L, V)
    y, targets, mem64 = _inputs(shape)
    with torch.no_grad():
        yd, td = (y if K > 1 else y[:, 0]).to(cuda), (targets if K > 1 else targets[:, 0]).to(cuda)
        logits, logprob = m.forced_decode(mem64.float().to(cuda), yd, targets=td)
    assert logits.shape == ((sy, B, K, V) if K > 1 else (sy, B, V)) and logprob.shape == yd.shape
    ref = _oracle(sd64, h, y.view(B * K, sy), mem64.repeat_interleave(K, dim=1))                # (sy, B * K, V): the memory per sequence
    bar = 4e-2 * max(1.0, ref.abs().max().item())
    got = logits.cpu().view(sy, B * K, V)
    err = (got.double() - ref).abs().max().item()
    t2 = targets.view(B * K, sy)
    ref_lp = torch.log_softmax(ref, -1).gather(2, t2.permute(1, 0)[..., None])[..., 0].permute(1, 0)
    lp_err = (logprob.cpu().view(B * K, sy).double() - ref_lp).abs().max().item()
    print(f"item 2 {shape}: max|logits - oracle| = {err:.3e} (bar {bar:.3e}); max|logprob - oracle| = {lp_err:.3e} (bar {2 * bar:.3e})")
    assert err < bar, (err, bar)
    assert lp_err < 2 * bar, (lp_err, bar)
    _own_logprob_check(got, logprob.view(B * K, sy), t2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_against_one_fused_decode_for_seven_and_eight_tokens(egx_lib, cuda, shape):
    from egot2_amd import functional as F_egx
    d, h, L, V, S, B, K, sy = shape
    m, _, _ = _model(d, h, L, V)
    y, _, mem64 = _inputs(shape)
    mem = mem64.float().to(cuda)
    for n in sorted({min(sy, 7), min(sy, 8)}):
        with torch.no_grad():
            yd = y[..., :n].contiguous().to(cuda)
            got = m.forced_decode(mem, yd if K > 1 else yd[:, 0])
            assert F_egx.last_decoder_impl() == "forced"
            dec = m.decode(yd.view(B * K, n), mem.repeat_interleave(K, dim=1))
            assert F_egx.last_decoder_impl() == "fused"
        diff = (got.reshape(n, B * K, V) - dec).abs().max().item()
        bar = 3e-2 * max(1.0, dec.abs().max().item())
        print(f"item 3 {shape} n = {n}: max|forced - decode()| = {diff:.3e} (fused-vs-composed bar {bar:.3e})")
        assert FORCED_VS_DECODE_MEASURED is not None, "item 3 needs the measured difference"
        assert diff < min(4 * FORCED_VS_DECODE_MEASURED, bar), (diff, FORCED_VS_DECODE_MEASURED, bar)


# ---- item 4 ----
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[6] > 1], ids=lambda s: "-".join(map(str, s)))
def test_k_sequences_per_clip_against_k_calls_with_one(egx_lib, cuda, shape):
    d, h, L, V, S, B, K, sy = shape
    m, _, _ = _model(d, h, L, V)
    y, targets, mem64 = _inputs(shape)
    mem, y, targets = mem64.float().to(cuda), y.to(cuda), targets.to(cuda)
    with torch.no_grad():
        logits, logprob = m.forced_decode(mem, y, targets=targets)
        ones = [m.forced_decode(mem, y[:, k].contiguous(), targets=targets[:, k].contiguous()) for k in range(K)]
    one_logits, one_lp = torch.stack([o[0] for o in ones], dim=2), torch.stack([o[1] for o in ones], dim=1)
    diff, lp_diff = (logits - one_logits).abs().max().item(), (logprob - one_lp).abs().max().item()
    bar = 3e-2 * max(1.0, one_logits.abs().max().item())
    print(f"item 4 {shape}: K = {K} against K = 1: max logits difference {diff:.3e}, max logprob difference {lp_diff:.3e} (bar {bar:.3e})")
    assert FORCED_K_VS_ONE_MEASURED is not None, "item 4 needs the measured differences"
    assert diff <= min(4 * FORCED_K_VS_ONE_MEASURED[0], bar), (diff, FORCED_K_VS_ONE_MEASURED, bar)
    assert lp_diff <= min(4 * FORCED_K_VS_ONE_MEASURED[1], bar), (lp_diff, FORCED_K_VS_ONE_MEASURED, bar)


# ---- item 5 ----
def test_padding_targets_and_out_of_vocabulary_tokens(egx_lib, cuda):
    d, h, L, V, S, B, K, sy = 256, 4, 2, 40, 16, 5, 3, 11
    m, sd64, _ = _model(d, h, L, V)
    g = torch.Generator().manual_seed(21)
    y, targets = torch.randint(0, V - 1, (B, K, sy), generator=g), torch.randint(0, V, (B, K, sy), generator=g)     # (word V - 1 is kept out of y)
    mem64 = seeded_feats(96, [(S, B, d)])[0].double()
    mem = mem64.float().to(cuda)
    pad = targets.clone()
    pad[:, :, -3:] = -100
    pad[1, 2, 0], pad[0, 0, 4], pad[4, 1, 5] = V, -1, 1 << 40
    out = pad != targets
    with torch.no_grad():
        logits, logprob = m.forced_decode(mem, y.to(cuda), targets=targets.to(cuda))
        logits_p, logprob_p = m.forced_decode(mem, y.to(cuda), targets=pad.to(cuda))
    assert torch.equal(logits_p, logits)
    lp, lpp = logprob.cpu(), logprob_p.cpu()
    assert bool((lpp[out] == 0).all()) and not bool(torch.signbit(lpp[out]).any()), "a target outside the vocabulary must give exactly 0.0"
    assert torch.equal(lpp[~out], lp[~out]) and bool((lp[~out] < 0).all())
    # an input token of -1 (and of V): the zero embedding row. The oracle reads word V - 1 with that row zeroed.
    y_bad = y.clone()
    y_bad[2, 1, 3], y_bad[0, 0, 0], y_bad[3, 2, 10] = -1, V, -1
    sd0 = dict(sd64)
    sd0["embedding.weight"] = sd64["embedding.weight"].clone()
    sd0["embedding.weight"][V - 1] = 0
    y_ref = torch.where((y_bad < 0) | (y_bad >= V), torch.full_like(y_bad, V - 1), y_bad)
    with torch.no_grad():
        got = m.forced_decode(mem, y_bad.to(cuda)).cpu().view(sy, B * K, V)
    ref = _oracle(sd0, h, y_ref.view(B * K, sy), mem64.repeat_interleave(K, dim=1))
    bar = 4e-2 * max(1.0, ref.abs().max().item())
    err = (got.double() - ref).abs().max().item()
    moved = (ref - _oracle(sd64, h, y_ref.view(B * K, sy), mem64.repeat_interleave(K, dim=1))).abs().max().item()
    print(f"item 5: max|logits - oracle with the zero row| = {err:.3e} (bar {bar:.3e}); the zero row moves the oracle by {moved:.3e}")
    assert err < bar and moved > 2 * bar, (err, moved, bar)     # (the check can tell the zero row from word V - 1's)


# ---- item 6 ----
@pytest.mark.parametrize("K", [1, 3])
def test_bit_properties_inside_the_call(egx_lib, cuda, K):
    d, h, L, V, S, B, sy = 256, 4, 2, 40, 48, 37, 12
    m, _, _ = _model(d, h, L, V)
    g = torch.Generator().manual_seed(31 + K)
    shape = (B, K, sy) if K > 1 else (B, sy)
    y, targets = torch.randint(0, V, shape, generator=g).to(cuda), torch.randint(0, V, shape, generator=g).to(cuda)
    mem = seeded_feats(97, [(S, B, d)])[0].to(cuda)
    with torch.no_grad():
        log, lp = m.forced_decode(mem, y, targets=targets)
        log2, lp2 = m.forced_decode(mem, y, targets=targets)
        assert torch.equal(log, log2) and torch.equal(lp, lp2), "two calls differ"
        assert torch.equal(m.forced_decode(mem, y, targets=targets, return_logits=False), lp), "return_logits=False changes logprob"
        assert torch.equal(m.forced_decode(mem, y), log), "the call without targets changes the logits"
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(4)).to(cuda)
        logp, lpp = m.forced_decode(mem[:, perm].contiguous(), y[perm].contiguous(), targets=targets[perm].contiguous())
        assert torch.equal(logp, log[:, perm]) and torch.equal(lpp, lp[perm]), "permuting the clips does not permute the outputs bit for bit"
        j = 11
        mem2 = mem.clone()
        mem2[:, j] = mem2[:, j] * -1.5 + 0.25
        logj, lpj = m.forced_decode(mem2, y, targets=targets)
        others = torch.arange(B, device=cuda) != j
        assert torch.equal(logj[:, others], log[:, others]) and torch.equal(lpj[others], lp[others]), "clip j's memory leaked into another clip"
        assert not torch.equal(logj[:, j], log[:, j]) and not torch.equal(lpj[j], lp[j])
        # another token for sequence r of clip b at step t: rows < t of that sequence and every other sequence keep their bits
        b, r, t = 20, K - 1, 7
        y2 = y.clone()
        at = (b, r, t) if K > 1 else (b, t)
        y2[at] = (y2[at] + 1) % V
        logt, lpt = m.forced_decode(mem, y2, targets=targets)
        seq = (slice(None), b, r) if K > 1 else (slice(None), b)
        same = torch.ones(log.shape[:-1], dtype=torch.bool, device=cuda)
        same[seq] = False
        assert torch.equal(logt[same], log[same]), "a token of one sequence moved another sequence"
        assert torch.equal(logt[seq][:t], log[seq][:t]), "a token at step t moved an earlier row of its sequence"
        assert not torch.equal(logt[seq][t], log[seq][t]) and not torch.equal(logt[seq][t + 1:], log[seq][t + 1:])
        lsame = same[0]
        assert torch.equal(lpt[lsame], lp[lsame]) and torch.equal(lpt[at[:-1]][:t], lp[at[:-1]][:t])


# ---- item 7 ----
def test_captured_call_replays_on_new_tokens_targets_and_memory(egx_lib, cuda):
    d, h, L, V, S, B, K, sy = 256, 4, 2, 40, 48, 9, 2, 11
    m, _, _ = _model(d, h, L, V)
    mems = [f.to(cuda) for f in seeded_feats(98, [(S, B, d)] * 2)]
    gens = [torch.Generator().manual_seed(s) for s in (5, 6)]
    ys = [torch.randint(0, V, (B, K, sy), generator=g).to(cuda) for g in gens]
    ts = [torch.randint(-1, V + 1, (B, K, sy), generator=g).to(cuda) for g in gens]                   # (some targets outside the vocabulary)
    with torch.no_grad():
        eager = [m.forced_decode(mems[i], ys[i], targets=ts[i]) for i in range(2)]
        eager = [(a.clone(), b.clone()) for a, b in eager]
        s_mem, s_y, s_t = mems[0].clone(), ys[0].clone(), ts[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.forced_decode(s_mem, s_y, targets=s_t)                    # warm-up on a side stream (side stream creation, allocator)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            log, lp = m.forced_decode(s_mem, s_y, targets=s_t)
        for i in (1, 0, 1):
            s_mem.copy_(mems[i])
            s_y.copy_(ys[i])
            s_t.copy_(ts[i])
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(log, eager[i][0]) and torch.equal(lp, eager[i][1]), f"replay on contents {i} differs from the eager call"


# ---- item 8 ----
def test_decode_routes_nine_to_sixty_four_tokens_at_inference(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    d, h, L, V, S, B = 256, 4, 2, 40, 16, 5
    m, sd64, _ = _model(d, h, L, V)
    g = torch.Generator().manual_seed(41)
    y21, y8 = torch.randint(0, V, (B, 21), generator=g).to(cuda), torch.randint(0, V, (B, 8), generator=g).to(cuda)
    mem = seeded_feats(96, [(S, B, d)])[0].to(cuda)
    try:
        with torch.no_grad():
            got = m.decode(y21, mem)
            assert F_egx.last_decoder_impl() == "forced"
            assert torch.equal(got, m.forced_decode(mem, y21)) and got.shape == (21, B, V)
            got64 = m.decode(torch.cat((y21, y21, y21, y21[:, :1]), dim=1), mem)
            assert F_egx.last_decoder_impl() == "forced" and got64.shape == (64, B, V)
            # 8 tokens: the fused decoder, the bits of DecoderFn called directly
            dec8 = m.decode(y8, mem)
            assert F_egx.last_decoder_impl() == "fused"
            meta, params = m._egx_decoder_args(m.transformer_decoder, m.pos_embed, m.n_heads, m.dp_rate)
            direct = F_egx.DecoderFn.apply(meta, y8, mem.permute(1, 0, 2).contiguous().view(B * S, d), m.embedding.weight, m.pos_embed.pe[:8, 0, :],
                                           *params, m.fc.weight, m.fc.bias)
            assert torch.equal(dec8, direct.view(B, 8, -1).permute(1, 0, 2))
            with pytest.raises(Exception) as e65:                       # 65 tokens: beyond the call too, where it went before
                m.decode(torch.cat((y21, y21, y21, y21[:, :2]), dim=1), mem)
            with pytest.raises(Exception) as e_attn:                    # attention weights stay with the 8-row decoders
                m.decode(y21, mem, return_attention=True)
        assert F_egx.last_decoder_impl() != "forced"
        # grad enabled, or train mode: 9 tokens raise as they did (the composed decoder's attention serves at most 8 query rows)
        with pytest.raises(Exception) as e_grad:
            m.decode(y21[:, :9], mem)
        m.train()
        with torch.no_grad(), pytest.raises(Exception) as e_train:
            m.decode(y21[:, :9], mem)
        for e in (e65, e_attn, e_grad, e_train):
            assert "outside 1..8" in str(e.value), str(e.value)
    finally:
        m.eval()


def test_the_validation_step_of_the_action_task_model_runs_unchanged(egx_lib, cuda):
    """model(video, target[:, :-1], 'lta_verb') of HOI/tasks/multitask/video_task_action.py:83-88 over [lta_verb, 20 verbs, </s>]: the
    backbones are stand-ins that hand the seeded features through, the translator and the decoder are the library's."""
    from egot2_amd import functional as F_egx, hoi_multitask
    d, h, L, V, B = 512, 8, 3, 600, 7
    m = hoi_multitask.TaskTranslationPromptTransformerActionTask(NS(hidden_dim=d, num_heads=h, num_layers=L, dropout=0.0, ff_dim=2048), gr.vocab_of(V),
                                                                 v_idx=[0], n_idx=[0])
    sd = seeded_state_dict(m, 95)
    m.load_state_dict(sd)
    sd64 = {k: v.double() for k, v in sd.items()}
    m = m.to(cuda).set_compute("bf16").eval()
    feat_action, feat_lta = seeded_feats(96, [(B, 2, d)] * 2)
    m.action_model = lambda x: x[0]                                     # encode_clips hands it [pathway[:, i]]: the clip's feature row
    m.lta_model = lambda video, _, middle=True: feat_lta.to(cuda).transpose(0, 1)
    target = torch.randint(0, V, (B, 22), generator=torch.Generator().manual_seed(51))
    with torch.no_grad():
        out = m([feat_action.to(cuda)], target[:, :-1].to(cuda), 'lta_verb')
    assert F_egx.last_decoder_impl() == "forced" and out.shape == (B, V, 21)
    with torch.no_grad():
        ref = tr.g_decode(sd64, h, target[:, :-1], tr.hoi_ga_encode(sd64, h, 'lta_verb', feat_action.double(), feat_lta.double())).permute(1, 2, 0)
    bar = 4e-2 * max(1.0, ref.abs().max().item())
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"item 8: model(video, target[:, :-1], 'lta_verb') over 21 tokens: max|logits - oracle| = {err:.3e} (bar {bar:.3e})")
    assert err < bar, (err, bar)
    # the validation loss of the step, from logprob: the mean over the tokens that are no padding
    with torch.no_grad():
        mem = m.encode([feat_action.to(cuda)], 'lta_verb')
        tgt = target[:, 1:].clone()
        tgt[:, -4:] = -100
        lp = m.forced_decode(mem, target[:, :-1].to(cuda), targets=tgt.to(cuda), return_logits=False)
        loss = -lp.sum() / (tgt != -100).sum()
        want = torch.nn.functional.cross_entropy(out, tgt.to(cuda), ignore_index=-100)
    assert abs(loss.item() - want.item()) < 1e-4 * max(1.0, abs(want.item())), (loss.item(), want.item())


# ---- item 9 ----
@pytest.mark.parametrize("name", ["base", "lta_schedule"])
def test_beam_scores_are_the_summed_logprob_of_the_hypotheses(egx_lib, cuda, name):
    d, h, L, V, S, B, n, W = br.CASES[name]
    m, sd64, start, mem64 = br.build_case(name)
    m = m.to(cuda).set_compute("bf16").eval()
    mem = mem64.float().to(cuda)
    with torch.no_grad():
        tokens, scores = m.beam_decode(mem, start, n, W, return_scores=True)
        y = torch.cat((torch.full((B, W, 1), start, dtype=torch.int64, device=cuda), tokens[..., :-1]), dim=-1)
        logits, logprob = m.forced_decode(mem, y, targets=tokens)
    ref = _oracle(sd64, h, y.cpu().view(B * W, n), mem64.repeat_interleave(W, dim=1))
    bar = 4e-2 * max(1.0, ref.abs().max().item())
    err = (logits.cpu().view(n, B * W, V).double() - ref).abs().max().item()
    diff = (logprob.sum(-1) - scores).abs().max().item()
    print(f"item 9 [{name}]: max|sum logprob - beam score| = {diff:.3e} (bound {n * 4 * bar:.3e}); max|logits - oracle| = {err:.3e} (bar {bar:.3e})")
    assert err < bar, (err, bar)
    assert diff < n * 4 * bar, (diff, n, bar)
