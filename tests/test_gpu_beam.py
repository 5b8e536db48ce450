"""-m gpu: beam search in one call (egx_decoder_beam through DecoderMixin.beam_decode). A strict "device sequences equal the fp64 oracle's"
test cannot be set: the gaps between adjacent beam candidates (median 0.006 .. 0.26 nats over the seeded models) lie below any threshold
derived from the bf16 logit bar 4e-2 * max(1, max|ref|) = 0.10 .. 0.18, so no clip is decided. Correctness is pinned by composition; every
case of tests/beam_ref.py CASES is held to:
  1. own consistency, from the call's selection trace: tokens_out is the backtrack of step_tokens / step_parents and scores_out is
     step_scores[-1], exactly; scores descend; a clip's sequences are pairwise distinct; and per step, with the host's fp64
     cand = prev_score[w] + log_softmax(step_logits[t, b, w]) over the DEVICE's own logits and previous scores ([0, -inf, ...] at step 0):
     every survivor's score is within eps of its candidate, no unselected candidate exceeds the weakest survivor by more than 2 eps, survivors
     are ordered to within 2 eps. eps = 32 * 2^-23 * max(1, |cand|, max|logits row|) is derived, not measured: at most about 10 ulp for an
     fp32 tree or lane-sequential sum of at most 1024 exponentials, a few ulp for x - max - lse, half an ulp for the add;
  2. teacher-forced parity with the fp64 oracle: for each final hypothesis (B * W rows, the memory repeated per slot) the logits the device
     computed along its ancestry are within 4e-2 * max(1, max|ref|) (the bar of test_gpu_decoder.py and test_gpu_generate.py) and its
     score within n_steps * 2 * that bar of the oracle's log-probability of the same sequence (a log-probability moves by at most twice the
     worst logit error); for n_steps <= 8 also the logits of every slot at every step, the prefixes read from the trace;
  3. teacher-forced parity with the library's own decode() for n_steps <= 8: one fused decode() of the final prefixes over B * W rows;
     bound = 4 x the worst difference measured on the MI355X over these cases (BEAM_VS_DECODE_MEASURED, profiles/beam_mi355x.json), never
     looser than 3e-2 * max(1, max|ref|); beyond 8 steps greedy_ref.stock_decode at the 3e-2 bar, as the greedy test does;
  4. (base, lta_schedule) beam_width = 1 is greedy_decode: equal tokens, step_logits equal to its logits bit for bit, scores the fp32
     log-softmax of those logits at the chosen tokens to item 1's eps.
Printed, not asserted: the share of clips whose best sequence equals the fp64 oracle's best, and the worst candidate gap."""
import functools

import pytest
import torch

from oracle import translator_ref as tr
from tests import beam_ref as br, greedy_ref as gr
from tests.util import seeded_feats

pytestmark = pytest.mark.gpu

# item 3: worst |beam - decode()| logit difference over the n_steps <= 8 cases, measured on an MI355X (profiles/beam_mi355x.json)
BEAM_VS_DECODE_MEASURED = 4.77e-6      # (lds_extreme; the others 4.8e-7 .. 1.9e-6: the bf16 rows agree, the fp32 heads sum in different orders)

ULP = 2.0 ** -23


def _eps(cand, row_max):
    return 32 * ULP * torch.maximum(torch.ones_like(cand), torch.maximum(cand.abs(), row_max))


@functools.lru_cache(maxsize=None)
def _run(name):
    """One device call per case, shared by its checks: (model on the device, fp64 state dict, start, fp64 memory, device memory, outputs on the CPU)."""
    from egot2_amd import functional as F_egx
    d, h, L, V, S, B, n, W = br.CASES[name]
    m, sd64, start, mem64 = br.build_case(name)
    dev = torch.device("cuda:0")
    m = m.to(dev).set_compute("bf16").eval()
    mem = mem64.float().to(dev)
    with torch.no_grad():
        tokens, scores, trace = m.beam_decode(mem, start, n, W, return_scores=True, return_trace=True)
        assert F_egx.last_decoder_impl() == "beam"
        assert torch.equal(tokens, m.beam_decode(mem, torch.full((B,), start, dtype=torch.int64, device=dev), n, W)), "tensor start tokens"
    out = dict(tokens=tokens.cpu(), scores=scores.cpu(), **{k: getattr(trace, k).cpu() for k in trace.__slots__})
    assert out["tokens"].shape == (B, W, n) and out["tokens"].dtype == torch.int64 and out["scores"].shape == (B, W)
    assert out["step_tokens"].shape == out["step_parents"].shape == out["step_scores"].shape == (n, B, W)
    assert out["step_parents"].dtype == torch.int32 and out["step_logits"].shape == (n, B, W, V)
    return m, sd64, start, mem64, mem, out


def _check_selection(out, W, V):
    """Item 1's per-step checks of a trace against the host's fp64 candidates over the device's own logits and previous scores."""
    n, B = out["step_tokens"].shape[:2]
    prev = torch.full((B, W), float("-inf"), dtype=torch.float64)
    prev[:, 0] = 0.0
    for t in range(n):
        logits = out["step_logits"][t].double()
        cand = prev[..., None] + torch.log_softmax(logits, dim=-1)                       # (B, W, V)
        eps = _eps(cand, logits.abs().max(dim=-1, keepdim=True).values.expand_as(cand)).view(B, W * V)
        cand = cand.view(B, W * V)
        flat = out["step_parents"][t].long() * V + out["step_tokens"][t]
        assert int(out["step_parents"][t].min()) >= 0 and int(out["step_parents"][t].max()) < W
        assert int(out["step_tokens"][t].min()) >= 0 and int(out["step_tokens"][t].max()) < V
        got, want, e = out["step_scores"][t].double(), cand.gather(1, flat), eps.gather(1, flat)
        assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got).all()), f"step {t}: a dead slot survived"
        assert bool(((got - want).abs() <= e).all()), (t, (got - want).abs().max().item(), e.min().item())
        for b in range(B):
            assert len(set(flat[b].tolist())) == W, f"step {t}, clip {b}: a candidate was selected twice"
        rest = cand.scatter(1, flat, float("-inf"))
        worst = rest.argmax(dim=1, keepdim=True)
        slack = 2 * torch.maximum(eps.gather(1, worst), e[:, -1:])
        assert bool((rest.gather(1, worst) - want[:, -1:] <= slack).all()), f"step {t}: an unselected candidate beats the weakest survivor"
        assert bool((want[:, :-1] - want[:, 1:] >= -2 * torch.maximum(e[:, :-1], e[:, 1:])).all()), f"step {t}: survivors out of order"
        assert bool((got[:, :-1] >= got[:, 1:]).all()), f"step {t}: reported scores do not descend"
        prev = got


def _ancestry_logits(out):
    """(n, B * W, V): for every final hypothesis the logits row that produced each of its tokens."""
    n, B, W, V = out["step_logits"].shape
    _, pars = br.backtrack(out["step_tokens"], out["step_parents"])
    return torch.stack([out["step_logits"][t].gather(1, pars[t][..., None].expand(B, W, V)) for t in range(n)], 0).view(n, B * W, V)


@pytest.mark.parametrize("name", list(br.CASES))
def test_beam_holds_items_1_to_3(egx_lib, cuda, name):
    from egot2_amd import functional as F_egx
    d, h, L, V, S, B, n, W = br.CASES[name]
    m, sd64, start, mem64, mem, out = _run(name)
    tokens, scores = out["tokens"], out["scores"]
    # item 1
    back, _ = br.backtrack(out["step_tokens"], out["step_parents"])
    assert torch.equal(tokens, back), "item 1: tokens_out is not the backtrack of the trace"
    assert torch.equal(scores, out["step_scores"][-1]), "item 1: scores_out is not the last step's scores"
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()), "item 1: scores do not descend"
    for b in range(B):
        assert len({tuple(s) for s in tokens[b].tolist()}) == W, f"item 1: clip {b} holds a sequence twice"
    _check_selection(out, W, V)
    # item 2
    rows = B * W
    st = torch.full((rows,), start, dtype=torch.int64)
    mem_rep = mem64.repeat_interleave(W, dim=1)
    ref = gr.teacher_forced(sd64, h, st, tokens.view(rows, n), mem_rep)                  # (n, B * W, V)
    bound = 4e-2 * max(1.0, ref.abs().max().item())
    anc = _ancestry_logits(out)
    err = (anc.double() - ref).abs().max().item()
    ref_score = torch.log_softmax(ref, -1).gather(2, tokens.view(rows, n).permute(1, 0)[..., None])[..., 0].sum(0).view(B, W)
    serr = (scores.double() - ref_score).abs().max().item()
    print(f"item 2 [{name}]: max|logits - oracle| = {err:.3e} (bound {bound:.3e}); max|score - oracle log-probability| = {serr:.3e} "
          f"(bound {n * 2 * bound:.3e})")
    assert err < bound, (err, bound)
    assert serr < n * 2 * bound, (serr, n * 2 * bound)
    if n <= 8:
        worst = 0.0
        for t in range(n):
            if t == 0:
                pre = torch.full((B, W, 1), start, dtype=torch.int64)
            else:
                pre = torch.cat((torch.full((B, W, 1), start, dtype=torch.int64), br.backtrack(out["step_tokens"], out["step_parents"], t - 1)[0]), 2)
            with torch.no_grad():
                want = tr.g_decode(sd64, h, pre.view(rows, t + 1), mem_rep)[-1].view(B, W, V)
            e = (out["step_logits"][t].double() - want).abs().max().item()
            assert e < 4e-2 * max(1.0, want.abs().max().item()), (t, e)
            worst = max(worst, e)
        print(f"item 2 [{name}]: every slot at every step: max|logits - oracle| = {worst:.3e}")
    # item 3
    dev = mem.device
    y = torch.cat((st[:, None], tokens.view(rows, n)[:, :-1]), dim=1).to(dev)
    mem_dev = mem.repeat_interleave(W, dim=1)
    with torch.no_grad():
        if n <= 8:
            dec = m.decode(y, mem_dev).cpu()
            assert F_egx.last_decoder_impl() == "fused"
            diff = (anc - dec).abs().max().item()
            bar = 3e-2 * max(1.0, dec.abs().max().item())
            print(f"item 3 [{name}]: max|beam - decode()| = {diff:.3e} (fused-vs-composed bar {bar:.3e})")
            assert BEAM_VS_DECODE_MEASURED is not None, "item 3 needs the measured difference"
            assert diff < min(4 * BEAM_VS_DECODE_MEASURED, bar), (diff, BEAM_VS_DECODE_MEASURED, bar)
        else:
            dec = gr.stock_decode(m, y, mem_dev).cpu()
            diff = (anc - dec).abs().max().item()
            bar = 3e-2 * max(1.0, dec.abs().max().item())
            print(f"item 3 [{name}]: max|beam - stock fp32 decode| = {diff:.3e} (bar {bar:.3e})")
            assert diff < bar, (diff, bar)
    # printed, not asserted: agreement with the fp64 beam
    rt, rs, rtrace, gaps = br.beam(sd64, h, torch.full((B,), start, dtype=torch.int64), mem64, n, W)
    share = (tokens[:, 0] == rt[:, 0]).all(dim=-1).float().mean().item()
    print(f"[{name}] best sequence equals the fp64 oracle's best on {share:.2f} of {B} clips; smallest gap between adjacent oracle candidates "
          f"{gaps.min().item():.3e} (median {gaps[torch.isfinite(gaps)].median().item():.3e})")


@pytest.mark.parametrize("name", ["base", "lta_schedule"])
def test_beam_width_one_is_greedy(egx_lib, cuda, name):
    d, h, L, V, S, B, n, W = br.CASES[name]
    m, sd64, start, mem64, mem, _ = _run(name)
    with torch.no_grad():
        gt, gl = m.greedy_decode(mem, start, n, return_logits=True)
        tokens, scores, trace = m.beam_decode(mem, start, n, 1, return_scores=True, return_trace=True)
    assert torch.equal(tokens[:, 0], gt), "W = 1: tokens differ from greedy_decode's"
    assert torch.equal(trace.step_logits[:, :, 0], gl), "W = 1: logits differ from greedy_decode's in some bit"
    assert int(trace.step_parents.abs().max()) == 0 and torch.equal(trace.step_tokens[:, :, 0], gt.permute(1, 0))
    gl64, got = gl.cpu().double(), trace.step_scores[:, :, 0].cpu().double()
    steps = torch.log_softmax(gl64, -1).gather(2, gt.cpu().permute(1, 0)[..., None])[..., 0]          # (n, B)
    prev = torch.zeros(B, dtype=torch.float64)
    for t in range(n):          # each step to item 1's eps, on the device's own previous score
        want = prev + steps[t]
        assert bool(((got[t] - want).abs() <= _eps(want, gl64[t].abs().max(dim=-1).values)).all()), t
        prev = got[t]
    assert torch.equal(scores[:, 0].cpu().double(), got[-1])


def _small(cuda, cls="TaskTranslationPromptTransformer"):
    m, _, start = gr.hoi_model(256, 4, 2, 40, 95, cls=cls)
    return m.to(cuda).set_compute("bf16").eval(), start


def _beam(m, mem, st, n, W):
    tokens, scores, trace = m.beam_decode(mem, st, n, W, return_scores=True, return_trace=True)
    return [tokens, scores] + [getattr(trace, k) for k in trace.__slots__]


CLIP_AXIS = (0, 0, 1, 1, 1, 1)      # of tokens, scores, step_tokens, step_parents, step_scores, step_logits


def test_permutation_leakage_and_determinism(egx_lib, cuda):
    m, _ = _small(cuda)
    B, S, n, W = 37, 48, 5, 3
    mem = seeded_feats(97, [(S, B, 256)])[0].to(cuda)
    st = torch.randint(0, 40, (B,), generator=torch.Generator().manual_seed(3)).to(cuda)
    with torch.no_grad():
        a, a2 = _beam(m, mem, st, n, W), _beam(m, mem, st, n, W)
        assert all(torch.equal(x, y) for x, y in zip(a, a2)), "two calls differ"
        perm = torch.randperm(B, generator=torch.Generator().manual_seed(4)).to(cuda)
        p = _beam(m, mem[:, perm].contiguous(), st[perm], n, W)
        assert all(torch.equal(y, x.index_select(ax, perm)) for x, y, ax in zip(a, p, CLIP_AXIS)), "permuting the clips does not permute the outputs bit for bit"
        j = 11
        mem2 = mem.clone()
        mem2[:, j] = mem2[:, j] * -1.5 + 0.25
        c = _beam(m, mem2, st, n, W)
        others = (torch.arange(B, device=cuda) != j).nonzero()[:, 0]
        assert all(torch.equal(y.index_select(ax, others), x.index_select(ax, others)) for x, y, ax in zip(a, c, CLIP_AXIS)), "clip j's memory leaked into another clip"
        assert not torch.equal(c[5][:, j], a[5][:, j])


def test_captured_call_replays_on_new_contents(egx_lib, cuda):
    m, _ = _small(cuda)
    B, S, n, W = 9, 48, 6, 4
    mems = [f.to(cuda) for f in seeded_feats(98, [(S, B, 256)] * 2)]
    starts = [torch.randint(0, 40, (B,), generator=torch.Generator().manual_seed(s)).to(cuda) for s in (5, 6)]
    with torch.no_grad():
        eager = [[x.clone() for x in _beam(m, mems[i], starts[i], n, W)] for i in range(2)]
        assert not torch.equal(eager[0][0], eager[1][0])
        s_mem, s_start = mems[0].clone(), starts[0].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _beam(m, s_mem, s_start, n, W)          # warm-up on a side stream (side stream creation, allocator)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            got = _beam(m, s_mem, s_start, n, W)
        for i in (1, 0, 1):
            s_mem.copy_(mems[i])
            s_start.copy_(starts[i])
            g.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in zip(got, eager[i])), f"replay on contents {i} differs from the eager call"


def test_unsupported_configurations_raise_and_leave_the_other_paths_alone(egx_lib, cuda):
    from egot2_amd import functional as F_egx
    B, S = 6, 16
    mem = seeded_feats(96, [(S, B, 256)])[0].to(cuda)
    with torch.no_grad():
        m, start = _small(cuda)
        with pytest.raises(ValueError, match="compute bf16"):
            m.set_compute("f32s").beam_decode(mem, start, 3, 3)
        m.set_compute("bf16")
        big, _, big_start = gr.hoi_model(256, 4, 2, 1030, 95)
        with pytest.raises(ValueError, match="vocabulary <= 1024"):
            big.to(cuda).set_compute("bf16").eval().beam_decode(mem, big_start, 3, 3)
        with pytest.raises(ValueError, match="1..8"):
            m.beam_decode(mem, start, 3, 9)
        m.greedy_decode(mem, start, 3)
        assert F_egx.last_decoder_impl() == "generate"
        assert m.beam_decode(mem, start, 3, 3).shape == (B, 3, 3) and F_egx.last_decoder_impl() == "beam"
        # predict_ac keeps its loop over decode()
        p, _ = _small(cuda, cls="TaskPromptTransformer")
        p.pos_embed.dropout.p = 0.0
        slow, fast = [f.to(cuda) for f in seeded_feats(96, [(B, 8, 2048), (B, 8, 256)])]
        p.recognition_model = lambda video, middle=True: [video[0].permute(0, 2, 1)[..., None, None], video[1].permute(0, 2, 1)[..., None, None]]
        with pytest.raises(ValueError, match="1..8"):
            p.beam_decode(mem, start, 3, 9)
        p.predict_ac([slow, fast])
        assert F_egx.last_decoder_impl() == "fused"
