"""Token schedules on the host, without a GPU (egx_decoder_generate_sched / egx_decoder_beam_sched, additions under ABI v18): symbols, the
library's refusals, TokenSchedule packing, the model methods' validation, and self-checks of the fp64 oracle the GPU tests are built on
(tests/sched_ref.py), the strict case of tests/test_gpu_sched.py re-derived. Pure host work (no HIP call), against the product library."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from egot2_amd.functional import TokenSchedule          # (the feature under test: without it nothing below can run)

NEW = ("egx_decoder_generate_sched", "egx_decoder_beam_sched")


def _dcfg(d=256, h=4, L=3, V=40, S=48, compute=1, p_drop=0.0, p_pos=0.0, dff=2048, sy=0):
    from egot2_amd._lib import DecConfig
    return DecConfig(d, h, dff, L, V, sy, S, 1e-5, compute, p_drop, p_pos, None)


def test_abi_stays_18_and_the_two_symbols_resolve(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES, name


def test_refusals_carry_their_message(egx_lib):
    """Every refusal comes before any device work: the calls below pass null device pointers (and a non-null dummy for `words`, never read on
    the host), so a call that got past its checks would stop at "null pointer argument"."""
    words = C.c_void_p(256)         # a DEVICE pointer as far as the host is concerned: only compared with null

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def gen(cfg, period, counts, wp, n=2):
        return egx_lib.egx_decoder_generate_sched(C.byref(cfg), None, None, None, None, 256, None, None, None, 4, n, None, None, None, None,
                                                  period, counts, wp)

    def beam(cfg, period, counts, wp, n=2, W=3):
        return egx_lib.egx_decoder_beam_sched(C.byref(cfg), None, None, None, None, 256, None, None, None, 4, n, W, *((None,) * 8),
                                              period, counts, wp)

    def refused(rc, frag):
        assert rc != 0 and frag in egx_lib.egx_last_error(), (frag, egx_lib.egx_last_error())

    for call, who in ((gen, b"egx_decoder_generate_sched"), (beam, b"egx_decoder_beam_sched")):
        refused(call(_dcfg(), -1, ints(3), words), who + b": period = -1")
        refused(call(_dcfg(), 65, ints(*([3] * 65)), words), who + b": period = 65")
        refused(call(_dcfg(), 2, None, words), who + b": period = 2 with a null counts or words")
        refused(call(_dcfg(), 2, ints(3, 3), None), who + b": period = 2 with a null counts or words")
        refused(call(_dcfg(), 2, ints(3, 0), words), who + b": counts[1] = 0 (1..vocab = 40)")
        refused(call(_dcfg(), 2, ints(41, 3), words), who + b": counts[0] = 41 (1..vocab = 40)")
        refused(call(_dcfg(), 3, ints(3, 40, -2), words), who + b": counts[2] = -2")
        # a valid schedule passes the schedule checks and stops at the null pointers; so does period = 0 (the unscheduled call)
        refused(call(_dcfg(), 2, ints(3, 40), words), b"null pointer")
        refused(call(_dcfg(), 64, ints(*([3] * 64)), words), b"null pointer")
        refused(call(_dcfg(), 0, None, None), b"null pointer")
        # the unscheduled calls' limits still apply, and come first
        refused(call(_dcfg(), 2, ints(3, 3), words, n=65), b"n_steps = 65")
        refused(call(_dcfg(p_drop=0.5), 2, ints(3, 3), words), b"inference only")
        refused(call(_dcfg(V=1025), 2, ints(3, 3), words), b"vocab = 1025")
        refused(call(_dcfg(compute=2), 2, ints(3, 3), words), b"bf16")
    # beam: step 0 has only counts[0] continuations of the one live slot
    refused(beam(_dcfg(), 2, ints(2, 40), words, W=3), b"egx_decoder_beam_sched: W = 3 exceeds counts[0] = 2")
    refused(beam(_dcfg(), 2, ints(3, 1), words, W=3), b"null pointer")          # (a later row may be smaller than W: W live slots by then)
    refused(beam(_dcfg(), 2, ints(3, 3), words, W=9), b"W = 9")
    refused(gen(_dcfg(), 2, ints(1, 1), words), b"null pointer")                # greedy has no such limit


def test_token_schedule_packing():
    allowed = torch.zeros((3, 10), dtype=torch.bool)
    allowed[0, [7, 2, 5]] = True
    allowed[1, :] = True
    allowed[2, 9] = True
    s = TokenSchedule(allowed, "cpu")
    assert s.period == 3 and s.vocab == 10 and s.counts == [3, 10, 1]
    assert s.words.dtype == torch.int32 and s.words.shape == (3, 10) and s.words.is_contiguous()
    assert s.words.tolist() == [[2, 5, 7] + [7] * 7, list(range(10)), [9] * 10]
    assert s.allowed.device.type == "cpu" and torch.equal(s.allowed, allowed)
    allowed[0, 0] = True
    assert s.counts == [3, 10, 1] and not bool(s.allowed[0, 0]), "the schedule must hold its own copy"
    period, counts, wp = s._args()
    assert period == 3 and list(counts) == [3, 10, 1] and wp == s.words.data_ptr()
    # random tables: ascending indices, then the last index
    g = torch.Generator().manual_seed(0)
    a = torch.rand((64, 600), generator=g) < 0.2
    a[:, 0] |= ~a.any(dim=1)
    s = TokenSchedule(a, "cpu")
    for p in range(64):
        want = a[p].nonzero()[:, 0].tolist()
        assert s.counts[p] == len(want) and s.words[p].tolist() == want + [want[-1]] * (600 - len(want))
    with pytest.raises(ValueError, match="bool"):
        TokenSchedule(torch.ones((2, 10)), "cpu")
    with pytest.raises(ValueError, match="bool"):
        TokenSchedule([[True, False]], "cpu")
    with pytest.raises(ValueError, match="shape"):
        TokenSchedule(torch.ones(10, dtype=torch.bool), "cpu")
    with pytest.raises(ValueError, match="1..64 rows"):
        TokenSchedule(torch.ones((0, 10), dtype=torch.bool), "cpu")
    with pytest.raises(ValueError, match="1..64 rows"):
        TokenSchedule(torch.ones((65, 10), dtype=torch.bool), "cpu")
    TokenSchedule(torch.ones((64, 10), dtype=torch.bool), "cpu")
    bad = torch.ones((3, 10), dtype=torch.bool)
    bad[1] = False
    with pytest.raises(ValueError, match="rows \\[1\\] are empty"):
        TokenSchedule(bad, "cpu")


def _model(V=12):
    from egot2_amd import hoi_multitask
    from tests import greedy_ref as gr
    args = NS(hidden_dim=256, num_heads=4, num_layers=1, dropout=0.0, pnr_cfg_file=None, oscc_cfg_file=None, action_cfg_file=None, lta_cfg_file=None)
    return hoi_multitask.TaskPromptTransformer(args, gr.vocab_of(V))


def test_verb_noun_schedule_and_token_schedule():
    m = _model(V=12)
    for v_idx, n_idx in (([5, 6, 7, 9], [7, 8, 9, 10, 11]), (np.array([9, 5, 7, 6, 5]), np.array([11, 10, 9, 8, 7])),
                         (torch.tensor([5, 6, 7, 9]), torch.tensor([7, 8, 9, 10, 11], dtype=torch.int32))):
        s = m.verb_noun_schedule(v_idx, n_idx)                          # overlapping sets (7, 9), duplicates, any order
        assert s.period == 2 and s.vocab == 12 and s.counts == [4, 5]
        assert s.words.tolist() == [[5, 6, 7, 9] + [9] * 8, [7, 8, 9, 10, 11] + [11] * 7]
        assert s.words.device == m.embedding.weight.device
    for v_idx, n_idx, name in (([5, 12], [7], "v_idx"), ([5], [-1, 7], "n_idx"), ([5], np.array([7, 600]), "n_idx")):
        with pytest.raises(ValueError, match=f"{name} holds an index outside the vocabulary of 12 words"):
            m.verb_noun_schedule(v_idx, n_idx)
    with pytest.raises(ValueError, match="integer word indices"):
        m.verb_noun_schedule([5.0], [7])
    with pytest.raises(ValueError, match="rows \\[1\\] are empty"):
        m.verb_noun_schedule([5], [])
    with pytest.raises(ValueError, match="over 13 words, the model's vocabulary has 12"):
        m.token_schedule(torch.ones((2, 13), dtype=torch.bool))
    s = m.token_schedule(torch.ones((5, 12), dtype=torch.bool))
    assert s.period == 5 and s.counts == [12] * 5


def test_python_validation_raises_before_any_library_call(egx_lib, monkeypatch):
    from egot2_amd import _lib
    m = _model().eval()
    sched = m.verb_noun_schedule([5, 6], [7, 8, 9])
    other = TokenSchedule(torch.ones((2, 13), dtype=torch.bool), "cpu")
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    mem = torch.zeros(16, 3, 256)
    with torch.no_grad():
        with pytest.raises(ValueError, match="beam_width = 3 exceeds the 2 words step 0 may emit"):
            m.beam_decode(mem, 4, 2, 3, schedule=sched)
        with pytest.raises(ValueError, match="over 13 words, the model's vocabulary has 12"):
            m.beam_decode(mem, 4, 2, 2, schedule=other)
        with pytest.raises(ValueError, match="over 13 words, the model's vocabulary has 12"):
            m.greedy_decode(mem, 4, 2, schedule=other)
        for bad in (torch.ones((2, 12), dtype=torch.bool), "verbs", 2):
            with pytest.raises(ValueError, match="functional.TokenSchedule"):
                m.greedy_decode(mem, 4, 2, schedule=bad)
            with pytest.raises(ValueError, match="functional.TokenSchedule"):
                m.beam_decode(mem, 4, 2, 2, schedule=bad)
        # the unscheduled checks still run, before the library too
        with pytest.raises(ValueError, match="GPU only"):
            m.beam_decode(mem, 4, 2, 2, schedule=sched)
        with pytest.raises(ValueError, match="GPU only"):
            m.greedy_decode(mem, 4, 2, schedule=sched)
        with pytest.raises(ValueError, match="positional table"):
            m.greedy_decode(mem, 4, 201, schedule=sched)
    with pytest.raises(ValueError, match="inference-only"):
        m.greedy_decode(mem, 4, 2, schedule=sched)


# ---- the fp64 oracle of the GPU tests ----
def _tiny(V, B=3, S=5):
    from tests import greedy_ref as gr
    from tests.util import seeded_feats
    m, sd64, start = gr.hoi_model(256, 4, 1, V, 95)
    return sd64, torch.full((B,), start, dtype=torch.int64), seeded_feats(96, [(S, B, 256)])[0].double()


def test_oracle_with_an_all_true_schedule_is_the_unscheduled_oracle():
    from tests import beam_ref as br, greedy_ref as gr, sched_ref as sr
    sd64, start, mem = _tiny(12)
    for P in (1, 2, 4):
        allowed = torch.ones((P, 12), dtype=torch.bool)
        for got, want in zip(sr.greedy(sd64, 4, start, mem, 4, allowed), gr.greedy(sd64, 4, start, mem, 4)):
            assert torch.equal(got, want)
        got = sr.beam(sd64, 4, start, mem, 3, 3, allowed)
        want = br.beam(sd64, 4, start, mem, 3, 3)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[3], want[3])
        assert all(torch.equal(got[2][k], want[2][k]) for k in want[2])


def test_oracle_keeps_every_step_inside_its_set():
    from tests import greedy_ref as gr, sched_ref as sr
    sd64, start, mem = _tiny(12, B=4)
    allowed = sr.alternation(12, range(5, 8), range(8, 12))
    tokens, logits, margins = sr.greedy(sd64, 4, start, mem, 4, allowed)
    for t in range(4):
        assert bool(allowed[t % 2][tokens[:, t]].all())
        assert bool((torch.isfinite(logits[t]) == allowed[t % 2]).all())
    assert torch.equal(tokens, gr.argmax_lowest(logits).permute(1, 0)) and bool((margins > 0).all()) and bool(torch.isfinite(margins).all())
    one = torch.zeros((1, 12), dtype=torch.bool)
    one[0, 7] = True
    t1, l1, m1 = sr.greedy(sd64, 4, start, mem, 2, one)
    assert bool((t1 == 7).all()) and bool(torch.isinf(m1).all())
    btok, bscore, trace, gaps = sr.beam(sd64, 4, start, mem, 4, 3, allowed)
    for t in range(4):
        assert bool(allowed[t % 2][btok[:, :, t]].all())
    assert bool(torch.isfinite(bscore).all()) and bool((bscore[:, :-1] >= bscore[:, 1:]).all())
    for b in range(4):
        assert len({tuple(s) for s in btok[b].tolist()}) == 3
    # the normaliser sums the set's words only: step 0's scores are log_softmax over the 3 verb words of the unmasked row
    row = trace["step_logits"][0][:, 0]
    want = torch.log_softmax(row[:, 5:8], -1).sort(dim=-1, descending=True).values
    assert (trace["step_scores"][0] - want).abs().max().item() < 1e-12
    # one-slot beam is scheduled greedy
    b1 = sr.beam(sd64, 4, start, mem, 4, 1, allowed)
    assert torch.equal(b1[0][:, 0], tokens) and torch.equal(b1[2]["step_logits"][:, :, 0], logits)


def test_the_strict_case_is_decided_on_at_least_half_of_its_clips():
    """tests/test_gpu_sched.py's strict-token case, re-derived: 19 of 32 clips decided with 12 distinct tokens; the schedule changes at least
    one token of 30 of the 32 clips against unconstrained greedy (so the GPU test cannot pass on code that ignores the schedule)."""
    from tests import greedy_ref as gr, sched_ref as sr
    m, sd64, start, mem, allowed, n = sr.strict_case()
    rt, rl, rm = sr.greedy(sd64, 4, start, mem, n, allowed)
    bar = 4e-2 * max(1.0, rl[torch.isfinite(rl)].abs().max().item())
    dec = gr.decided(rm, bar)
    distinct = sorted(set(rt[dec].flatten().tolist()))
    free = gr.greedy(sd64, 4, start, mem, n)[0]
    changed = int((free != rt).any(dim=1).sum())
    print(f"decided {int(dec.sum())} of 32, distinct tokens {distinct}; the schedule changes {changed} of 32 clips")
    assert int(dec.sum()) >= 16 and len(distinct) >= 2, (int(dec.sum()), distinct)
    assert changed >= 16, changed
