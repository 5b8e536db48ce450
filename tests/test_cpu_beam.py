"""Beam search on the host, without a GPU (egx_decoder_beam_workspace / egx_decoder_beam, added under ABI v18 as the generate entry points
were): symbols, the workspace query, the library's refusals, the predicate, the model method's validation, and self-checks of the fp64 beam
oracle the GPU tests are built on (tests/beam_ref.py). Pure host work (no HIP call), against the product library."""
import ctypes as C
import itertools
from types import SimpleNamespace as NS

import pytest
import torch

from egot2_amd.functional import decoder_beam_supported       # (the feature under test: without it nothing below can run)

NEW = ("egx_decoder_beam_workspace", "egx_decoder_beam")


def _dcfg(d=256, h=4, L=3, V=40, S=48, compute=1, p_drop=0.0, p_pos=0.0, dff=2048, sy=0):
    from egot2_amd._lib import DecConfig
    return DecConfig(d, h, dff, L, V, sy, S, 1e-5, compute, p_drop, p_pos, None)


def _ws(lib, cfg, B, n, W):
    nb = C.c_size_t(0)
    return lib.egx_decoder_beam_workspace(C.byref(cfg), B, n, W, C.byref(nb)), nb.value


def _ok(lib, cfg, B, n, W):
    rc, nb = _ws(lib, cfg, B, n, W)
    assert rc == 0, lib.egx_last_error()
    return nb


def test_abi_stays_18_and_the_two_symbols_resolve(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES, name


@pytest.mark.parametrize("d,L", [(256, 3), (512, 3), (256, 1)])
def test_workspace_is_linear_in_steps_in_width_and_in_clips(egx_lib, d, L):
    B, W = 40, 5
    cfg = lambda S=48: _dcfg(d=d, h=d // 64, L=L, S=S)  # noqa: E731

    def slope(B, S, W):
        a, b = _ok(egx_lib, cfg(S), B, 32, W), _ok(egx_lib, cfg(S), B, 64, W)
        assert (b - a) % 32 == 0
        return (b - a) // 32

    s = slope(B, 48, W)
    # the caches only: (B, W, n_steps, 2d) per layer, fp32 in layer 0, bf16 in the others
    assert s == B * W * 2 * d * (4 + 2 * (L - 1))
    vals = [_ok(egx_lib, cfg(), B, n, W) for n in (1, 2, 3, 17, 64)]
    assert [vals[i + 1] - vals[i] for i in range(4)] == [s, s, 14 * s, 47 * s]          # the same slope on every interval
    assert slope(2 * B, 48, W) == 2 * s                                                 # it doubles from B to 2B
    assert slope(B, 1, W) == s == slope(B, 1024, W)                                     # the memory's K | V is counted once, not per step
    # linear in W: one slope over 1 .. 8, at two depths; the step slope is linear in W too
    for n in (1, 40):
        by_w = [_ok(egx_lib, cfg(), B, n, w) for w in range(1, 9)]
        steps = {by_w[i + 1] - by_w[i] for i in range(7)}
        assert len(steps) == 1 and steps.pop() > 0, by_w
    assert [slope(B, 48, w) for w in (1, 2, 8)] == [s // W, 2 * s // W, 8 * s // W]
    # W = 1 runs greedy generation's step: at least its workspace
    for n in (1, 40, 64):
        nb = C.c_size_t(0)
        assert egx_lib.egx_decoder_generate_workspace(C.byref(cfg()), B, n, C.byref(nb)) == 0
        assert _ok(egx_lib, cfg(), B, n, 1) >= nb.value


def test_refusals_carry_their_message(egx_lib):
    def refused(cfg, frag, B=4, n=2, W=3):
        rc, _ = _ws(egx_lib, cfg, B, n, W)
        assert rc != 0 and frag in egx_lib.egx_last_error(), (frag, egx_lib.egx_last_error())

    assert _ws(egx_lib, _dcfg(sy=77), 4, 2, 3)[0] == 0                  # cfg->sy is not read
    refused(_dcfg(), b"W = 0", W=0)
    refused(_dcfg(), b"W = 9", W=9)
    refused(_dcfg(), b"W = -1", W=-1)
    assert _ws(egx_lib, _dcfg(), 4, 2, 8)[0] == 0 and _ws(egx_lib, _dcfg(), 4, 2, 1)[0] == 0
    refused(_dcfg(V=6), b"W = 7 exceeds vocab = 6", W=7)
    assert _ws(egx_lib, _dcfg(V=6), 4, 2, 6)[0] == 0
    refused(_dcfg(), b"n_steps = 0", n=0)
    refused(_dcfg(), b"n_steps = 65", n=65)
    assert _ws(egx_lib, _dcfg(), 4, 64, 3)[0] == 0
    refused(_dcfg(V=1025), b"vocab = 1025")
    refused(_dcfg(V=0), b"vocab = 0")
    assert _ws(egx_lib, _dcfg(V=1024, d=1024, h=16), 4, 2, 8)[0] == 0   # the head's LDS at every limit
    refused(_dcfg(p_drop=0.1), b"inference only")
    refused(_dcfg(p_pos=0.1), b"inference only")
    for compute in (0, 2):
        refused(_dcfg(compute=compute), b"bf16")
    refused(_dcfg(d=192, h=3), b"d_model = 192")
    refused(_dcfg(d=256, h=2), b"head dim 128")
    refused(_dcfg(dff=100), b"d_ff = 100")
    refused(_dcfg(L=17), b"17 layers")
    refused(_dcfg(S=1025), b"S = 1025")
    refused(_dcfg(), b"B = 0", B=0)
    nb = C.c_size_t(0)
    assert egx_lib.egx_decoder_beam_workspace(None, 4, 2, 3, C.byref(nb)) != 0 and b"null" in egx_lib.egx_last_error()
    assert egx_lib.egx_decoder_beam_workspace(C.byref(_dcfg()), 4, 2, 3, None) == 0            # a query for the verdict alone
    # the call itself: the same checks, then null pointers, before any device work
    nulls = (None,) * 8

    def call(cfg, n=2, W=3, stride=256):
        return egx_lib.egx_decoder_beam(C.byref(cfg), None, None, None, None, stride, None, None, None, 4, n, W, *nulls)

    assert call(_dcfg()) != 0 and b"null pointer" in egx_lib.egx_last_error()
    assert call(_dcfg(p_drop=0.5)) != 0 and b"inference only" in egx_lib.egx_last_error()
    assert call(_dcfg(), n=65) != 0 and b"n_steps = 65" in egx_lib.egx_last_error()
    assert call(_dcfg(), W=9) != 0 and b"W = 9" in egx_lib.egx_last_error()
    assert call(_dcfg(V=2)) != 0 and b"W = 3 exceeds vocab = 2" in egx_lib.egx_last_error()
    assert call(_dcfg(compute=2)) != 0 and b"bf16" in egx_lib.egx_last_error()


def test_supported_predicate_matches_the_library(egx_lib):
    configs = [("bf16", 512, 8, 2048, 48, 3, 600, 40, 5), ("bf16", 256, 4, 2048, 200, 2, 12, 3, 8), ("bf16", 1024, 16, 2048, 4, 1, 1024, 64, 8),
               ("bf16", 256, 4, 2048, 16, 2, 12, 1, 1), ("bf16", 256, 4, 2048, 16, 2, 6, 2, 6),
               ("bf16", 256, 4, 2048, 16, 2, 12, 2, 0), ("bf16", 256, 4, 2048, 16, 2, 12, 2, 9), ("bf16", 256, 4, 2048, 16, 2, 6, 2, 7),
               ("bf16", 256, 4, 2048, 8, 2, 1025, 2, 3), ("bf16", 256, 4, 2048, 8, 2, 12, 65, 3), ("bf16", 256, 4, 2048, 8, 2, 12, 0, 3),
               ("f32s", 256, 4, 2048, 8, 2, 12, 2, 3), ("f32", 256, 4, 2048, 8, 2, 12, 2, 3), ("bf16", 128, 4, 2048, 8, 2, 12, 2, 3),
               ("bf16", 256, 4, 2048, 1025, 2, 12, 2, 3), ("bf16", 256, 2, 2048, 8, 2, 12, 2, 3), ("bf16", 256, 4, 100, 8, 2, 12, 2, 3),
               ("bf16", 256, 4, 2048, 8, 17, 12, 2, 3)]
    verdicts = set()
    for compute, d, h, dff, S, L, V, n, W in configs:
        want = decoder_beam_supported(compute, d, h, dff, S, L, V, n, W)
        rc, _ = _ws(egx_lib, _dcfg(d=d, h=h, L=L, V=V, S=S, dff=dff, compute={"bf16": 1, "f32": 0, "f32s": 2}[compute]), 3, n, W)
        assert want == (rc == 0), (compute, d, h, dff, S, L, V, n, W)
        verdicts.add(want)
    assert verdicts == {True, False}


def _model(V=12):
    from egot2_amd import hoi_multitask
    from tests import greedy_ref as gr
    args = NS(hidden_dim=256, num_heads=4, num_layers=1, dropout=0.0, pnr_cfg_file=None, oscc_cfg_file=None, action_cfg_file=None, lta_cfg_file=None)
    return hoi_multitask.TaskPromptTransformer(args, gr.vocab_of(V))


def test_python_validation_raises_before_any_library_call(egx_lib, monkeypatch):
    from egot2_amd import _lib
    m = _model()
    monkeypatch.setattr(_lib, "load", lambda: (_ for _ in ()).throw(AssertionError("the library was called")))
    mem = torch.zeros(16, 3, 256)
    with pytest.raises(ValueError, match="inference-only"):
        m.train().beam_decode(mem, 4, 2, 3)
    m.eval()
    with pytest.raises(ValueError, match="inference-only"):             # eval mode, but an autograd graph over the parameters
        m.beam_decode(mem, 4, 2, 3)
    with torch.no_grad():
        for bad in (0, 9, -1, True, 2.0, None, "3"):
            with pytest.raises(ValueError, match="beam_width must be an int in 1..8"):
                m.beam_decode(mem, 4, 2, bad)
        with pytest.raises(ValueError, match="start must be a \\(3,\\)"):
            m.beam_decode(mem, torch.zeros(4, dtype=torch.int64), 2, 3)
        with pytest.raises(ValueError, match="int64"):
            m.beam_decode(mem, torch.zeros(3, dtype=torch.int32), 2, 3)
        with pytest.raises(ValueError, match="start_token"):
            m.beam_decode(mem, 4.0, 2, 3)
        with pytest.raises(ValueError, match="positional table"):
            m.beam_decode(mem, 4, 201, 3)
        with pytest.raises(ValueError, match="n_steps"):
            m.beam_decode(mem, 4, 0, 3)
        with pytest.raises(ValueError, match="\\(S, B, d\\)"):
            m.beam_decode(mem[0], 4, 2, 3)
        with pytest.raises(ValueError, match="GPU only"):               # CPU tensors: no CPU fallback and no Python search
            m.beam_decode(mem, 4, 2, 3)
        with pytest.raises(ValueError, match="GPU only"):
            _model(V=6).eval().beam_decode(mem, 4, 2, 6)
        with pytest.raises(ValueError, match="beam_width = 7 exceeds the vocabulary of 6"):
            _model(V=6).eval().beam_decode(mem, 4, 2, 7)


# ---- the fp64 oracle of the GPU tests ----
def _tiny(V, B=3, S=5):
    from tests import greedy_ref as gr
    from tests.util import seeded_feats
    m, sd64, start = gr.hoi_model(256, 4, 1, V, 95)
    return sd64, torch.full((B,), start, dtype=torch.int64), seeded_feats(96, [(S, B, 256)])[0].double()


def test_oracle_with_one_slot_is_the_greedy_oracle():
    from tests import beam_ref as br, greedy_ref as gr
    sd64, start, mem = _tiny(12)
    tokens, scores, trace, gaps = br.beam(sd64, 4, start, mem, 4, 1)
    gt, gl, gm = gr.greedy(sd64, 4, start, mem, 4)
    assert torch.equal(tokens[:, 0], gt) and torch.equal(trace["step_logits"][:, :, 0], gl)
    want = torch.log_softmax(gl, -1).gather(2, gt.permute(1, 0)[..., None])[..., 0].cumsum(0)      # (n, B)
    assert torch.equal(trace["step_scores"][:, :, 0], want) and torch.equal(scores[:, 0], want[-1])
    assert int(trace["step_parents"].abs().max()) == 0 and gaps.shape == (4, 3, 1) and bool((gaps >= 0).all())


def test_oracle_is_exhaustive_when_the_beam_holds_every_sequence():
    """V = 6, n = 2, W = 6: step 0 keeps all 6 first tokens, so step 1 ranks all 36 sequences; the 6 survivors are the 6 best by brute force."""
    from tests import beam_ref as br, greedy_ref as gr
    sd64, start, mem = _tiny(6)
    B = start.shape[0]
    tokens, scores, trace, _ = br.beam(sd64, 4, start, mem, 2, 6)
    seqs = torch.tensor(list(itertools.product(range(6), repeat=2)), dtype=torch.int64)           # (36, 2), lexicographic
    logp = torch.log_softmax(gr.teacher_forced(sd64, 4, start.repeat_interleave(36), seqs.repeat(B, 1), mem.repeat_interleave(36, dim=1)), -1)
    total = logp.gather(2, seqs.repeat(B, 1).permute(1, 0)[..., None])[..., 0].sum(0).view(B, 36)
    vals, idx = torch.sort(total, dim=-1, descending=True, stable=True)
    assert torch.equal(tokens, seqs[idx[:, :6]])
    assert (scores - vals[:, :6]).abs().max().item() < 1e-12
    back, _ = br.backtrack(trace["step_tokens"], trace["step_parents"])
    assert torch.equal(back, tokens)


def test_oracle_sequences_of_a_clip_are_pairwise_distinct():
    from tests import beam_ref as br
    sd64, start, mem = _tiny(12, B=4)
    tokens, scores, trace, gaps = br.beam(sd64, 4, start, mem, 3, 5)
    for b in range(4):
        assert len({tuple(s) for s in tokens[b].tolist()}) == 5
    assert bool((scores[:, :-1] >= scores[:, 1:]).all()) and bool(torch.isfinite(scores).all())
    assert bool((trace["step_scores"][0] <= 0).all()) and int(trace["step_parents"][0].abs().max()) == 0     # step 0: slot 0 alone is live
