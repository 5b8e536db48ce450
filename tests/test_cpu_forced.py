"""Teacher-forced decoding of up to 64 target tokens on the host, without a GPU (egx_decoder_forced_workspace / egx_decoder_forced, additions
under ABI v18): symbols, the workspace query, every refusal of the library with its message and no launch, the predicate, and the model
method's validation. Pure host work (no HIP call), against the product library."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import pytest
import torch

from egot2_amd.functional import decoder_forced_supported     # (the feature under test: without it nothing below can run)

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("egx_decoder_forced_workspace", "egx_decoder_forced")
PTR = 1 << 12       # a non-null, 16-byte aligned marker: every call below is refused before anything is read


def _dcfg(d=256, h=4, L=3, V=40, S=48, compute=1, p_drop=0.0, p_pos=0.0, dff=2048, sy=0):
    from egot2_amd._lib import DecConfig
    return DecConfig(d, h, dff, L, V, sy, S, 1e-5, compute, p_drop, p_pos, None)


def _ws(lib, cfg, B, R, n):
    nb = C.c_size_t(0)
    return lib.egx_decoder_forced_workspace(C.byref(cfg), B, R, n, C.byref(nb)), nb.value


def _ok(lib, cfg, B, R, n):
    rc, nb = _ws(lib, cfg, B, R, n)
    assert rc == 0, lib.egx_last_error()
    return nb


def test_abi_stays_18_and_the_two_symbols_resolve(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "egot2x.h")).read()
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES and name + "(" in hdr, name
    for cite in ("video_task.py:601-617", "video_task_action.py:83-88", "lta_models_seqdecoder.py:175-179"):
        assert cite in hdr, cite


def test_workspace_succeeds_at_the_limits_and_grows_with_every_extent(egx_lib):
    lib = egx_lib
    assert _ok(lib, _dcfg(d=1024, h=16, L=16, V=1024, S=1024), 4, 8, 64) > 0                    # every limit at once
    assert _ok(lib, _dcfg(d=256, h=8, L=1, V=1, S=1), 1, 1, 1) > 0
    base = _ok(lib, _dcfg(), 40, 3, 21)
    assert _ok(lib, _dcfg(), 41, 3, 21) > base and _ok(lib, _dcfg(), 40, 4, 21) > base and _ok(lib, _dcfg(), 40, 3, 22) > base
    # per step and row: the per-layer K/V caches (fp32 in layer 0, bf16 in the others) and the two fp32 slabs (input rows, last-layer rows)
    d, L, M = 256, 3, 40 * 3
    assert _ok(lib, _dcfg(), 40, 3, 64) - _ok(lib, _dcfg(), 40, 3, 32) == 32 * M * (2 * d * (4 + 2 * (L - 1)) + 2 * d * 4)
    # the rows of a clip share its memory: K sequences of one clip need less than K clips of one sequence
    assert _ok(lib, _dcfg(S=1024), 8, 8, 21) < _ok(lib, _dcfg(S=1024), 64, 1, 21)
    # R = 1 runs greedy generation's step: at least its workspace
    for n in (1, 40, 64):
        nb = C.c_size_t(0)
        assert lib.egx_decoder_generate_workspace(C.byref(_dcfg()), 40, n, C.byref(nb)) == 0
        assert _ok(lib, _dcfg(), 40, 1, n) >= nb.value
    assert lib.egx_decoder_forced_workspace(C.byref(_dcfg()), 4, 3, 2, None) == 0               # a query for the verdict alone


def test_refusals_carry_their_message_and_launch_nothing(egx_lib):
    from egot2_amd._lib import DecLayer
    lib = egx_lib
    lib.egx_launch_count(1)

    def refused(cfg, frag, B=4, R=3, n=2):
        rc, _ = _ws(lib, cfg, B, R, n)
        assert rc != 0 and frag in lib.egx_last_error(), (frag, lib.egx_last_error())

    assert _ws(lib, _dcfg(sy=77), 4, 3, 2)[0] == 0                      # cfg->sy is not read
    refused(_dcfg(), b"R = 0", R=0)
    refused(_dcfg(), b"R = 9", R=9)
    refused(_dcfg(), b"R = -1", R=-1)
    assert _ws(lib, _dcfg(), 4, 8, 2)[0] == 0 and _ws(lib, _dcfg(), 4, 1, 2)[0] == 0
    assert _ws(lib, _dcfg(V=2), 4, 8, 2)[0] == 0                        # unlike a beam, R sequences need no R distinct words
    refused(_dcfg(), b"n_steps = 0", n=0)
    refused(_dcfg(), b"n_steps = 65", n=65)
    assert _ws(lib, _dcfg(), 4, 3, 64)[0] == 0
    refused(_dcfg(V=1025), b"vocab = 1025")
    refused(_dcfg(V=0), b"vocab = 0")
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
    # the size limits egx_decoder_beam checks for B * W rows
    refused(_dcfg(d=1024, h=16), b"B = 100000 with R = 8, S = 48 is too large", B=100000, R=8)
    rc, _ = _ws(lib, _dcfg(d=1024, h=16), 100000, 8, 2)
    nbw = C.c_size_t(0)
    assert lib.egx_decoder_beam_workspace(C.byref(_dcfg(d=1024, h=16)), 100000, 2, 8, C.byref(nbw)) != 0 and rc != 0
    nb = C.c_size_t(0)
    assert lib.egx_decoder_forced_workspace(None, 4, 3, 2, C.byref(nb)) != 0 and b"null" in lib.egx_last_error()

    # the call itself: the same checks, then the outputs, null pointers and pe_stride, before any device work
    def call(cfg, frag, tokens=PTR, targets=PTR, others=PTR, stride=256, B=4, R=3, n=2, logits=PTR, logprob=PTR, ws=PTR):
        layers = C.cast(others, C.POINTER(DecLayer)) if others else None
        rc = lib.egx_decoder_forced(C.byref(cfg), tokens, targets, others, others, others, stride, layers, others, others, B, R, n, logits,
                                    logprob, ws, None)
        assert rc != 0 and frag in lib.egx_last_error(), (frag, lib.egx_last_error())

    call(_dcfg(), b"R = 9", R=9)
    call(_dcfg(), b"R = 0", R=0)
    call(_dcfg(p_drop=0.5), b"inference only")
    call(_dcfg(), b"n_steps = 65", n=65)
    call(_dcfg(compute=2), b"bf16")
    call(_dcfg(V=1025), b"vocab = 1025")
    call(_dcfg(), b"both null", logits=None, logprob=None)
    call(_dcfg(), b"logprob_out without targets", targets=None)
    call(_dcfg(), b"null pointer", tokens=None)
    call(_dcfg(), b"null pointer", others=None)
    call(_dcfg(), b"null pointer", ws=None)
    call(_dcfg(), b"pe_stride = 128", stride=128)
    call(_dcfg(), b"pe_stride = 258", stride=258)
    call(_dcfg(d=1024, h=16), b"too large", B=100000, R=8, stride=1024)
    assert lib.egx_launch_count(0) == 0                                 # nothing was launched


def test_supported_predicate_matches_the_library(egx_lib):
    configs = [("bf16", 512, 8, 2048, 4, 3, 600, 21, 1), ("bf16", 256, 4, 2048, 200, 2, 12, 9, 8), ("bf16", 1024, 16, 2048, 4, 1, 1024, 64, 8),
               ("bf16", 256, 4, 2048, 16, 2, 12, 1, 1), ("bf16", 256, 4, 2048, 16, 2, 2, 40, 8),
               ("bf16", 256, 4, 2048, 16, 2, 12, 2, 0), ("bf16", 256, 4, 2048, 16, 2, 12, 2, 9),
               ("bf16", 256, 4, 2048, 8, 2, 1025, 2, 3), ("bf16", 256, 4, 2048, 8, 2, 12, 65, 3), ("bf16", 256, 4, 2048, 8, 2, 12, 0, 3),
               ("f32s", 256, 4, 2048, 8, 2, 12, 2, 3), ("f32", 256, 4, 2048, 8, 2, 12, 2, 3), ("bf16", 128, 4, 2048, 8, 2, 12, 2, 3),
               ("bf16", 256, 4, 2048, 1025, 2, 12, 2, 3), ("bf16", 256, 2, 2048, 8, 2, 12, 2, 3), ("bf16", 256, 4, 100, 8, 2, 12, 2, 3),
               ("bf16", 256, 4, 2048, 8, 17, 12, 2, 3)]
    verdicts = set()
    for compute, d, h, dff, S, L, V, n, R in configs:
        want = decoder_forced_supported(compute, d, h, dff, S, L, V, n, R)
        rc, _ = _ws(egx_lib, _dcfg(d=d, h=h, L=L, V=V, S=S, dff=dff, compute={"bf16": 1, "f32": 0, "f32s": 2}[compute]), 3, R, n)
        assert want == (rc == 0), (compute, d, h, dff, S, L, V, n, R)
        verdicts.add(want)
    assert verdicts == {True, False}
    assert decoder_forced_supported("bf16", 512, 8, 2048, 4, 3, 600, 21) is True                # rows_per_clip defaults to 1


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
    y = torch.zeros(3, 21, dtype=torch.int64)
    with pytest.raises(ValueError, match="inference-only"):
        m.train().forced_decode(mem, y)
    m.eval()
    with pytest.raises(ValueError, match="inference-only"):             # eval mode, but an autograd graph over the parameters
        m.forced_decode(mem, y)
    with torch.no_grad():
        with pytest.raises(ValueError, match="\\(S, B, d\\)"):
            m.forced_decode(mem[0], y)
        for bad in (y[0], y[None, None], torch.zeros(4, 21, dtype=torch.int64), [1, 2, 3]):     # wrong rank, wrong batch, no tensor
            with pytest.raises(ValueError, match="y must be a \\(3, sy\\) or \\(3, K, sy\\)"):
                m.forced_decode(mem, bad)
        for bad in (torch.int32, torch.float32):
            with pytest.raises(ValueError, match="y must be int64"):
                m.forced_decode(mem, y.to(bad))
        with pytest.raises(ValueError, match="K = 9 sequences per clip: forced_decode serves 1..8"):
            m.forced_decode(mem, torch.zeros(3, 9, 21, dtype=torch.int64))
        with pytest.raises(ValueError, match="K = 0"):
            m.forced_decode(mem, torch.zeros(3, 0, 21, dtype=torch.int64))
        with pytest.raises(ValueError, match="sy = 65 target tokens: forced_decode serves 1..64"):
            m.forced_decode(mem, torch.zeros(3, 65, dtype=torch.int64))
        with pytest.raises(ValueError, match="sy = 0"):
            m.forced_decode(mem, torch.zeros(3, 0, dtype=torch.int64))
        for bad in (torch.zeros(3, 20, dtype=torch.int64), torch.zeros(3, 1, 21, dtype=torch.int64), [0]):
            with pytest.raises(ValueError, match="targets must have the shape of y \\(3, 21\\)"):
                m.forced_decode(mem, y, targets=bad)
        with pytest.raises(ValueError, match="targets must be int64"):
            m.forced_decode(mem, y, targets=y.to(torch.int32))
        with pytest.raises(ValueError, match="return_logits=False needs targets"):
            m.forced_decode(mem, y, return_logits=False)
        with pytest.raises(ValueError, match="neither return_attention nor memory_lengths"):
            m.forced_decode(mem, y, return_attention=True)
        with pytest.raises(ValueError, match="neither return_attention nor memory_lengths"):
            m.forced_decode(mem, y, memory_lengths=[16, 16, 16])
        with pytest.raises(ValueError, match="memory width 128"):
            m.forced_decode(torch.zeros(16, 3, 128), y)
        with pytest.raises(ValueError, match="GPU only"):               # CPU tensors: no CPU fallback
            m.forced_decode(mem, y)
        with pytest.raises(ValueError, match="GPU only"):
            m.forced_decode(mem, y[:, None, :].repeat(1, 8, 1), targets=y[:, None, :].repeat(1, 8, 1), return_logits=False)


def test_decode_of_nine_tokens_on_the_cpu_goes_where_it_went(egx_lib):
    """The routing of decode() to the forced path needs the GPU predicate of the fused decoder; an f32 model (the default compute) keeps the
    composed decoder, whose first library call refuses CPU tensors as before."""
    from egot2_amd import _lib
    m = _model().eval()
    with torch.no_grad(), pytest.raises(_lib.EgxError):
        m.decode(torch.zeros(3, 9, dtype=torch.int64), torch.zeros(16, 3, 256))
