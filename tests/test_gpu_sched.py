"""-m gpu: per-step token schedules of greedy generation and beam search (egx_decoder_generate_sched / egx_decoder_beam_sched through
greedy_decode / beam_decode(schedule=...)): step t may emit the words of row t % P of a (P, V) bool table only; the head computes the
listed vocabulary rows alone and every other logit is -inf. Every bar is one the project already holds its generation calls to:
  logits against the fp64 oracle (tests/sched_ref.py, tests/greedy_ref.py):  4e-2 * max(1, max|finite ref|)   (test_gpu_generate.py item 2)
  a beam score against the oracle's log-probability:                         n_steps * 2 * that bar            (test_gpu_beam.py item 2)
  selection consistency on the device's own logits:                          eps = 32 * 2^-23 * max(1, |cand|, max|finite logits of the row|)
                                                                                                               (test_gpu_beam.py item 1)
and the bit relations are exact: an all-true schedule is the unscheduled call, a listed word's logit has the unscheduled call's bits for
the same input row, scheduled beam with W = 1 is scheduled greedy, a captured call replays the eager call.
The strict-token case (CPU-checked in tests/test_cpu_sched.py: 19 of 32 clips decided with 12 distinct tokens; the schedule changes 30 of
the 32 clips' unconstrained greedy sequences) cannot pass on code that ignores the schedule."""
import functools

import pytest
import torch

from oracle import translator_ref as tr
from tests import beam_ref as br, greedy_ref as gr, sched_ref as sr
from tests.util import seeded_feats

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
NEG_INF = float("-inf")


def _bar(ref):
    return 4e-2 * max(1.0, ref[torch.isfinite(ref)].abs().max().item())


def _model(cuda, d, h, L, V, wseed, compute="bf16"):
    m, sd64, start = gr.hoi_model(d, h, L, V, wseed)
    return m.to(cuda).set_compute(compute).eval(), sd64, start


def _starts(start, B):
    return start.clone() if isinstance(start, torch.Tensor) else torch.full((B,), start, dtype=torch.int64)


def _check_greedy(tokens, logits, allowed, sd64, h, start, mem64, what):
    """Case 1's checks of one scheduled greedy call: tokens (B, n), logits (n, B, V) from the device."""
    tok, log = tokens.cpu(), logits.cpu()
    n, B, V = log.shape
    P = allowed.shape[0]
    assert tok.shape == (B, n) and tok.dtype == torch.int64
    for t in range(n):
        assert bool(allowed[t % P][tok[:, t]].all()), f"{what}: step {t} emitted a word outside its set"
        assert bool((torch.isfinite(log[t]) == allowed[t % P]).all()), f"{what}: step {t}: logits are not finite exactly on the set"
        assert bool((log[t][:, ~allowed[t % P]] == NEG_INF).all()), f"{what}: step {t}: an excluded logit is not -inf"
    assert torch.equal(tok, gr.argmax_lowest(log).permute(1, 0)), f"{what}: tokens are not the argmax of the call's own logits"
    ref = gr.teacher_forced(sd64, h, _starts(start, B), tok, mem64)
    ref = torch.stack([sr.mask(ref[t], allowed, t) for t in range(n)], 0)
    bound = _bar(ref)
    on = torch.isfinite(ref)
    err = (log.double() - ref)[on].abs().max().item()
    chosen = ref.gather(2, tok.permute(1, 0)[..., None])[..., 0]
    gap = (ref.max(dim=-1).values - chosen).max().item()
    print(f"{what}: max|logits - oracle| on the sets = {err:.3e} (bound {bound:.3e}); chosen-token gap {gap:.3e} (bound {2 * bound:.3e})")
    assert err < bound, (err, bound)
    assert gap < 2 * bound, (gap, bound)


def _trace_dict(tokens, scores, trace):
    return dict(tokens=tokens.cpu(), scores=scores.cpu(), **{k: getattr(trace, k).cpu() for k in trace.__slots__})


def _check_selection(out, W, V):
    """Item 1 of tests/test_gpu_beam.py on a scheduled trace, written for rows that hold -inf: the row maximum of eps runs over the finite
    logits, and an excluded candidate (-inf) takes no part in eps. Per step, with the host's fp64 cand = prev_score[w] +
    log_softmax(step_logits[t, b, w]) over the DEVICE's own logits (the -inf entries add nothing to the normaliser) and previous scores."""
    n, B = out["step_tokens"].shape[:2]
    prev = torch.full((B, W), NEG_INF, dtype=torch.float64)
    prev[:, 0] = 0.0
    for t in range(n):
        logits = out["step_logits"][t].double()
        cand = prev[..., None] + torch.log_softmax(logits, dim=-1)                       # (B, W, V); -inf outside the set and on dead slots
        assert not bool(torch.isnan(cand).any())
        row_max = torch.where(torch.isfinite(logits), logits.abs(), torch.zeros_like(logits)).max(dim=-1, keepdim=True).values
        mag = torch.where(torch.isfinite(cand), cand.abs(), torch.zeros_like(cand))
        eps = (32 * ULP * torch.maximum(torch.ones_like(cand), torch.maximum(mag, row_max.expand_as(cand)))).view(B, W * V)
        cand = cand.view(B, W * V)
        flat = out["step_parents"][t].long() * V + out["step_tokens"][t]
        assert int(out["step_parents"][t].min()) >= 0 and int(out["step_parents"][t].max()) < W
        assert int(out["step_tokens"][t].min()) >= 0 and int(out["step_tokens"][t].max()) < V
        got, want, e = out["step_scores"][t].double(), cand.gather(1, flat), eps.gather(1, flat)
        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got).all()), f"step {t}: a dead slot or an excluded word survived"
        assert bool(((got - want).abs() <= e).all()), (t, (got - want).abs().max().item(), e.min().item())
        for b in range(B):
            assert len(set(flat[b].tolist())) == W, f"step {t}, clip {b}: a candidate was selected twice"
        rest = cand.scatter(1, flat, NEG_INF)
        worst = rest.argmax(dim=1, keepdim=True)
        slack = 2 * torch.maximum(eps.gather(1, worst), e[:, -1:])
        assert bool((rest.gather(1, worst) - want[:, -1:] <= slack).all()), f"step {t}: an unselected candidate beats the weakest survivor"
        assert bool((want[:, :-1] - want[:, 1:] >= -2 * torch.maximum(e[:, :-1], e[:, 1:])).all()), f"step {t}: survivors out of order"
        assert bool((got[:, :-1] >= got[:, 1:]).all()), f"step {t}: reported scores do not descend"
        prev = got


def _check_beam(out, allowed, sd64, h, start, mem64, what, every_slot):
    """Case 4's checks of one scheduled beam call (out: _trace_dict)."""
    tokens, scores = out["tokens"], out["scores"]
    B, W, n = tokens.shape
    V, P = out["step_logits"].shape[-1], allowed.shape[0]
    for t in range(n):
        assert bool(allowed[t % P][tokens[:, :, t]].all()), f"{what}: a hypothesis holds a word outside step {t}'s set"
        assert bool(allowed[t % P][out["step_tokens"][t]].all()), f"{what}: step {t} kept a word outside its set"
        assert bool((torch.isfinite(out["step_logits"][t]) == allowed[t % P]).all()), f"{what}: step {t}: logits are not finite exactly on the set"
    back, pars = br.backtrack(out["step_tokens"], out["step_parents"])
    assert torch.equal(tokens, back), f"{what}: tokens_out is not the backtrack of the trace"
    assert torch.equal(scores, out["step_scores"][-1]), f"{what}: scores_out is not the last step's scores"
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), f"{what}: scores do not descend"
    for b in range(B):
        assert len({tuple(s) for s in tokens[b].tolist()}) == W, f"{what}: clip {b} holds a sequence twice"
    _check_selection(out, W, V)
    # teacher-forced oracle parity along each final hypothesis' ancestry, and each score against the oracle's log-probability over the sets
    rows = B * W
    st = _starts(start, B).repeat_interleave(W)
    mem_rep = mem64.repeat_interleave(W, dim=1)
    ref = gr.teacher_forced(sd64, h, st, tokens.view(rows, n), mem_rep)                  # (n, B * W, V)
    ref = torch.stack([sr.mask(ref[t], allowed, t) for t in range(n)], 0)
    bound = _bar(ref)
    anc = torch.stack([out["step_logits"][t].gather(1, pars[t][..., None].expand(B, W, V)) for t in range(n)], 0).view(n, rows, V)
    err = (anc.double() - ref)[torch.isfinite(ref)].abs().max().item()
    ref_score = torch.log_softmax(ref, -1).gather(2, tokens.view(rows, n).permute(1, 0)[..., None])[..., 0].sum(0).view(B, W)
    serr = (scores.double() - ref_score).abs().max().item()
    print(f"{what}: max|logits - oracle| on the sets = {err:.3e} (bound {bound:.3e}); max|score - oracle log-probability over the sets| = "
          f"{serr:.3e} (bound {n * 2 * bound:.3e})")
    assert err < bound, (err, bound)
    assert serr < n * 2 * bound, (serr, n * 2 * bound)
    if every_slot:
        worst = 0.0
        for t in range(n):
            pre = torch.full((B, W, 1), 0, dtype=torch.int64) + _starts(start, B)[:, None, None]
            if t:
                pre = torch.cat((pre, br.backtrack(out["step_tokens"], out["step_parents"], t - 1)[0]), 2)
            with torch.no_grad():
                want = sr.mask(tr.g_decode(sd64, h, pre.view(rows, t + 1), mem_rep)[-1].view(B, W, V), allowed, t)
            e = (out["step_logits"][t].double() - want)[torch.isfinite(want)].abs().max().item()
            assert e < _bar(want), (t, e)
            worst = max(worst, e)
        print(f"{what}: every slot at every step: max|logits - oracle| = {worst:.3e}")


# ---- the shared device runs: d 256, 4 heads, 2 layers, V 40, S 16, B 9, weight seed 95, memory seed 96, the standard alternation ----
@functools.lru_cache(maxsize=None)
def _base():
    dev = torch.device("cuda:0")
    m, sd64, start = _model(dev, 256, 4, 2, 40, 95)
    mem64 = seeded_feats(96, [(16, 9, 256)])[0].double()
    allowed = sr.standard_alternation()
    return m, sd64, start, mem64, mem64.float().to(dev), allowed, m.token_schedule(allowed)


def test_greedy_alternation(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64, start, mem64, mem, allowed, sched = _base()
    with torch.no_grad():
        tokens, logits = m.greedy_decode(mem, start, 6, return_logits=True, schedule=sched)
        assert F_egx.last_decoder_impl() == "generate"
        assert torch.equal(tokens, m.greedy_decode(mem, start, 6, schedule=sched)), "without return_logits"
    _check_greedy(tokens, logits, allowed, sd64, 4, start, mem64, "greedy, alternation")


def _beam(m, mem, st, n, W, schedule=None):
    tokens, scores, trace = m.beam_decode(mem, st, n, W, return_scores=True, return_trace=True, schedule=schedule)
    return [tokens, scores] + [getattr(trace, k) for k in trace.__slots__]


def test_bit_relations_to_the_unscheduled_calls(egx_lib, cuda):
    m, sd64, start, mem64, mem, allowed, sched = _base()
    everything = m.token_schedule(torch.ones((3, 40), dtype=torch.bool))
    n, W = 5, 3
    with torch.no_grad():
        # an all-true schedule is the unscheduled call
        gt, gl = m.greedy_decode(mem, start, n, return_logits=True)
        at, al = m.greedy_decode(mem, start, n, return_logits=True, schedule=everything)
        assert torch.equal(gt, at) and torch.equal(gl, al), "greedy: an all-true schedule differs from schedule=None"
        free, full = _beam(m, mem, start, n, W), _beam(m, mem, start, n, W, everything)
        assert all(torch.equal(x, y) for x, y in zip(free, full)), "beam: an all-true schedule differs from schedule=None"
        # step 0 sees the same input rows with and without a schedule: a listed word's logit keeps its bits
        st, sl = m.greedy_decode(mem, start, n, return_logits=True, schedule=sched)
        on = allowed[0].to(cuda)
        assert torch.equal(sl[0][:, on], gl[0][:, on]) and bool((sl[0][:, ~on] == NEG_INF).all()), "greedy: step 0's listed logits changed bits"
        sb = _beam(m, mem, start, n, W, sched)
        assert torch.equal(sb[5][0][..., on], free[5][0][..., on]) and bool((sb[5][0][..., ~on] == NEG_INF).all()), "beam: step 0's listed logits changed bits"
        # scheduled beam with one slot is scheduled greedy
        one = _beam(m, mem, start, n, 1, sched)
        assert torch.equal(one[0][:, 0], st), "W = 1: tokens differ from scheduled greedy_decode's"
        assert torch.equal(one[5][:, :, 0], sl), "W = 1: step_logits differ from scheduled greedy_decode's logits in some bit"
        assert int(one[3].abs().max()) == 0 and torch.equal(one[2][:, :, 0], st.permute(1, 0))
    assert not torch.equal(st, gt), "the schedule changed nothing: the relations above would be vacuous"


def test_strict_tokens_on_decided_clips(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64, start, mem64, allowed, n = sr.strict_case()
    m = m.to(cuda).set_compute("bf16").eval()
    with torch.no_grad():
        tokens = m.greedy_decode(mem64.float().to(cuda), start.to(cuda), n, schedule=m.token_schedule(allowed))
    assert F_egx.last_decoder_impl() == "generate"
    rt, rl, rm = sr.greedy(sd64, 4, start, mem64, n, allowed)
    dec = gr.decided(rm, _bar(rl))
    share, distinct = dec.float().mean().item(), sorted(set(rt[dec].flatten().tolist()))
    print(f"strict tokens: decided {int(dec.sum())} of {dec.numel()}, tokens among them {distinct}")
    assert share >= 0.5 and len(distinct) >= 2, (share, distinct)
    assert torch.equal(tokens.cpu()[dec], rt[dec]), "a decided clip's sequence differs from the scheduled fp64 greedy sequence"


def test_beam_alternation(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64, start, mem64, mem, allowed, sched = _base()
    with torch.no_grad():
        tokens, scores, trace = m.beam_decode(mem, start, 4, 3, return_scores=True, return_trace=True, schedule=sched)
        assert F_egx.last_decoder_impl() == "beam"
        assert torch.equal(tokens, m.beam_decode(mem, start, 4, 3, schedule=sched)), "without the trace"
    _check_beam(_trace_dict(tokens, scores, trace), allowed, sd64, 4, start, mem64, "beam, alternation", every_slot=True)


def test_lta_shape(egx_lib, cuda):
    """40 steps over V = 600, W = 5, P = 2: row 0 = words 5..119 (verbs), row 1 = words 120..599 (nouns), through verb_noun_schedule."""
    d, h, L, V, S, B, n, W = 512, 8, 3, 600, 8, 6, 40, 5
    m, sd64, start = _model(cuda, d, h, L, V, br.WSEED)
    mem64 = seeded_feats(br.FSEED, [(S, B, d)])[0].double()
    mem = mem64.float().to(cuda)
    allowed = sr.alternation(V, range(5, 120), range(120, 600))
    sched = m.verb_noun_schedule(torch.arange(5, 120), torch.arange(120, 600).numpy())
    assert torch.equal(sched.allowed, allowed) and sched.counts == [115, 480]
    with torch.no_grad():
        tokens, scores, trace = m.beam_decode(mem, start, n, W, return_scores=True, return_trace=True, schedule=sched)
        gt, gl = m.greedy_decode(mem, start, n, return_logits=True, schedule=sched)
    _check_beam(_trace_dict(tokens, scores, trace), allowed, sd64, h, start, mem64, "beam, LTA shape", every_slot=False)
    _check_greedy(gt, gl, allowed, sd64, h, start, mem64, "greedy, LTA shape")


def test_edges(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64, start, mem64, mem, allowed, sched = _base()
    # P = n_steps = 5: every step its own set
    each = torch.rand((5, 40), generator=torch.Generator().manual_seed(7)) < 0.3
    each[:, 5] |= ~each.any(dim=1)
    each[0, :3] = True                                                          # (step 0's set holds W = 3 words at least)
    assert len({tuple(r.tolist()) for r in each}) == 5
    s5 = m.token_schedule(each)
    # a one-word row: steps 1 and 4 can only emit word 7
    lone = sr.standard_alternation().repeat(2, 1)[:3].clone()
    lone[1] = False
    lone[1, 7] = True
    s1 = m.token_schedule(lone)
    with torch.no_grad():
        tokens, logits = m.greedy_decode(mem, start, 5, return_logits=True, schedule=s5)
        _check_greedy(tokens, logits, each, sd64, 4, start, mem64, "greedy, a set per step")
        bt, bs, btr = m.beam_decode(mem, start, 5, 3, return_scores=True, return_trace=True, schedule=s5)
        _check_beam(_trace_dict(bt, bs, btr), each, sd64, 4, start, mem64, "beam, a set per step", every_slot=False)
        tokens, logits = m.greedy_decode(mem, start, 5, return_logits=True, schedule=s1)
        assert bool((tokens[:, 1] == 7).all()) and bool((tokens[:, 4] == 7).all())
        _check_greedy(tokens, logits, lone, sd64, 4, start, mem64, "greedy, a one-word row")
        one = m.beam_decode(mem, start, 5, 1, schedule=s1)
        assert torch.equal(one[:, 0], tokens)
        b2 = m.beam_decode(mem, start, 5, 3, schedule=s1)                       # W = 3 over a one-word step: the three live slots go on
        assert bool((b2[:, :, 1] == 7).all()) and bool((b2[:, :, 4] == 7).all())
        # refusals, raised by the Python validation
        with pytest.raises(ValueError, match="beam_width = 4 exceeds the 3 words step 0 may emit"):
            few = lone.clone()
            few[0] = False
            few[0, 5:8] = True
            m.beam_decode(mem, start, 5, 4, schedule=m.token_schedule(few))
        other = F_egx.TokenSchedule(torch.ones((2, 41), dtype=torch.bool), cuda)
        for call in (lambda s: m.greedy_decode(mem, start, 3, schedule=s), lambda s: m.beam_decode(mem, start, 3, 2, schedule=s)):
            with pytest.raises(ValueError, match="over 41 words, the model's vocabulary has 40"):
                call(other)
            with pytest.raises(ValueError, match="the schedule's words are on cpu"):
                call(F_egx.TokenSchedule(allowed, "cpu"))
        # and by the functional layer on its own
        meta, params = m._egx_decoder_args(m.transformer_decoder, m.pos_embed, m.n_heads, 0.0)
        args = (meta, torch.full((9,), start, dtype=torch.int64, device=cuda), mem.permute(1, 0, 2).contiguous().view(9 * 16, 256), m.embedding.weight,
                m.pos_embed.pe[:3, 0, :], params, m.fc.weight, m.fc.bias, 3)
        with pytest.raises(ValueError, match="words are on cpu"):
            F_egx.decoder_generate(*args, schedule=F_egx.TokenSchedule(allowed, "cpu"))
        with pytest.raises(ValueError, match="exceeds the 3 words"):
            F_egx.decoder_beam(*args, 4, schedule=m.token_schedule(few))


def test_prefix_loop_applies_the_schedule(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    m, sd64, start = _model(cuda, 256, 4, 2, 40, 95, compute="f32s")
    mem64 = seeded_feats(96, [(16, 9, 256)])[0].double()
    allowed = sr.standard_alternation()
    with torch.no_grad():
        tokens, logits = m.greedy_decode(mem64.float().to(cuda), start, 3, return_logits=True, schedule=m.token_schedule(allowed))
    assert F_egx.last_decoder_impl() == "loop"
    _check_greedy(tokens, logits, allowed, sd64, 4, start, mem64, "prefix loop, alternation")


def test_captured_scheduled_call_replays_on_new_contents(egx_lib, cuda):
    m, sd64, start, mem64, _, allowed, sched = _base()          # (the schedule is built here, outside the captured region)
    B, S, n = 9, 48, 6
    mems = [f.to(cuda) for f in seeded_feats(98, [(S, B, 256)] * 2)]
    starts = [torch.randint(0, 40, (B,), generator=torch.Generator().manual_seed(s)).to(cuda) for s in (5, 6)]
    with torch.no_grad():
        eager = [m.greedy_decode(mems[i], starts[i], n, return_logits=True, schedule=sched) for i in range(2)]
        eager = [(t.clone(), l.clone()) for t, l in eager]
        assert not torch.equal(eager[0][0], eager[1][0])
        s_mem, s_start = mems[0].clone(), starts[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m.greedy_decode(s_mem, s_start, n, return_logits=True, schedule=sched)      # warm-up on a side stream (side stream creation, allocator)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            tok, log = m.greedy_decode(s_mem, s_start, n, return_logits=True, schedule=sched)
        for i in (1, 0):
            s_mem.copy_(mems[i])
            s_start.copy_(starts[i])
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(tok, eager[i][0]) and torch.equal(log, eager[i][1]), f"replay on contents {i} differs from the eager scheduled call"
            assert bool(allowed[0][tok[:, 0].cpu()].all()) and bool(allowed[1][tok[:, 1].cpu()].all())
