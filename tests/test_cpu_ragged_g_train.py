"""Ragged-batch TRAINING for the EgoT2-g HHI model on the host, without a GPU (egx_ragged_encode_train_workspace / _train_fwd /
egx_ragged_encode_bwd, egx_decoder_ragged_train_workspace / _train_fwd / egx_decoder_ragged_bwd, added under ABI v18 as the d = 128 training
entry points were): symbols, the workspace queries, the library's refusals and the model methods' validation. Pure host work (no HIP call)."""
import ctypes as C

import pytest
import torch

NEW = ("egx_ragged_encode_train_workspace", "egx_ragged_encode_train_fwd", "egx_ragged_encode_bwd",
       "egx_decoder_ragged_train_workspace", "egx_decoder_ragged_train_fwd", "egx_decoder_ragged_bwd")


def _cfg(compute=1, L=3, p_drop=0.1, impl=0, nseg=3, d=256):
    from egot2_amd._lib import Config
    return Config(d, 4, 2048, L, nseg, 1e-5, compute, impl, p_drop, 0.1, 0.0)


def _segs(T=150, nseg=3):
    from egot2_amd._lib import Segment
    segs = (Segment * nseg)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1     # non-null marker: the query reads no weight
    return segs


def _ws(lib, cfg, segs, lengths):
    lens = (C.c_int * len(lengths))(*lengths)
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    rc = lib.egx_ragged_encode_train_workspace(C.byref(cfg), segs, len(lengths) // cfg.n_segments, lens, C.byref(sv), C.byref(sc))
    return rc, sv.value, sc.value


def _dcfg(S=1024, p_drop=0.1):
    from egot2_amd._lib import DecConfig, EGX_BF16
    return DecConfig(256, 4, 2048, 3, 7, 2, S, 1e-5, EGX_BF16, p_drop, 0.1, None)


def _dws(lib, cfg, lengths):
    lens = (C.c_int * len(lengths))(*lengths)
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    return lib.egx_decoder_ragged_train_workspace(C.byref(cfg), len(lengths), lens, C.byref(sv), C.byref(sc)), sv.value, sc.value


def test_abi_stays_18_and_the_six_symbols_resolve(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    for name in NEW:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES, name


def test_training_workspaces_grow_with_tokens_not_with_longest_clip(egx_lib):
    cfg, segs = _cfg(), _segs()
    rc, sv_mixed, sc_mixed = _ws(egx_lib, cfg, segs, [15] * 3 * 64 + [150] * 3)       # sum S_b = 64 * 45 + 450, B * S_max = 65 * 450
    assert rc == 0
    rc, sv_uni, sc_uni = _ws(egx_lib, cfg, segs, [150] * 3 * 65)
    assert rc == 0 and sv_mixed < sv_uni / 3 and sc_mixed < sc_uni / 3, (sv_mixed, sv_uni, sc_mixed, sc_uni)
    rc, sv_s, sc_s = _ws(egx_lib, cfg, segs, [20] * 3 * 200)
    rc2, sv_b, sc_b = _ws(egx_lib, cfg, segs, [40] * 3 * 200)
    rc3, sv_w, _ = _ws(egx_lib, cfg, segs, [1] * 3)                                  # ~ the bf16 weight copies (W and W^T) alone
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert 1.8 < (sv_b - sv_w) / (sv_s - sv_w) < 2.2, (sv_s, sv_b, sv_w)
    # the decoder's: sum_b S_b memory rows, not B * cfg.S
    rc, d_small, ds_small = _dws(egx_lib, _dcfg(), [1] * 63 + [1024])
    rc2, d_big, ds_big = _dws(egx_lib, _dcfg(), [1024] * 64)
    assert rc == 0 and rc2 == 0 and d_small < d_big / 4 and ds_small < ds_big / 4, (d_small, d_big, ds_small, ds_big)


def test_training_workspace_refusals_carry_their_message(egx_lib):
    from egot2_amd._lib import BUCKET_CB

    def refused(cfg, frag, segs=None, lengths=(15, 15, 15)):
        rc, _, _ = _ws(egx_lib, cfg, segs or _segs(), list(lengths))
        assert rc != 0 and frag in egx_lib.egx_last_error(), (frag, egx_lib.egx_last_error())

    assert _ws(egx_lib, _cfg(), _segs(), [15] * 3)[0] == 0                    # dropout is what these calls are for
    assert _ws(egx_lib, _cfg(p_drop=0.0), _segs(), [15] * 3)[0] == 0
    cfg = _cfg()
    keep = BUCKET_CB(lambda user, bucket: None)
    cfg.bucket_cb = C.cast(keep, C.c_void_p)
    refused(cfg, b"bucket_cb")
    for field, frag in (("ce", b"fused losses"), ("token_ce", b"fused losses"), ("out_tokens", b"out_tokens"), ("bwd_stage", b"bwd_stage")):
        cfg = _cfg()
        setattr(cfg, field, 1)
        refused(cfg, frag)
    for compute in (0, 2):                                                    # f32, f32s: the grouped fallback's business
        refused(_cfg(compute=compute), b"bf16")
    refused(_cfg(impl=1), b"impl")
    refused(_cfg(), b"S=481", segs=_segs(T=200), lengths=(200, 200, 81))      # beyond the long attention at head dim 64
    assert _ws(egx_lib, _cfg(), _segs(T=200), [200, 200, 80])[0] == 0
    for bad in ([0, 15, 15], [151, 15, 15], [-3, 15, 15]):
        refused(_cfg(), b"1 .. 150", lengths=[15] * 3 + bad)
        assert b"clip 1" in egx_lib.egx_last_error()
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    assert egx_lib.egx_ragged_encode_train_workspace(C.byref(_cfg()), _segs(), 1, None, C.byref(sv), C.byref(sc)) != 0
    # out_layout 1 (the asd memory) needs equal segment lengths per clip; refused in the planning of both directions
    lens = (C.c_int * 6)(15, 15, 15, 15, 16, 15)
    assert egx_lib.egx_ragged_encode_train_fwd(C.byref(_cfg()), _segs(), lens, None, None, None, 2, None, 1, None, 1, 0, None) != 0
    assert b"equal segment lengths" in egx_lib.egx_last_error() and b"clip 1" in egx_lib.egx_last_error()
    assert egx_lib.egx_ragged_encode_bwd(C.byref(_cfg()), _segs(), lens, None, None, 2, None, 1, None, None, None, None, None, None, 1, 0, None) != 0
    assert b"equal segment lengths" in egx_lib.egx_last_error()
    # gradients the ragged kernels do not produce: projected features, a learned positional table
    from egot2_amd._lib import Layer, LayerGrads, SegmentGrads
    ok = (C.c_int * 3)(15, 15, 15)
    for field, frag in (("feat", b"PROJECTED features"), ("pos", b"positional table")):
        sgr = (SegmentGrads * 3)()
        setattr(sgr[1], field, 1)
        rc = egx_lib.egx_ragged_encode_bwd(C.byref(_cfg()), _segs(), ok, 1, (Layer * 3)(), 1, 1, 0, 1, 1, sgr, None, None, (LayerGrads * 3)(), 1, 0, None)
        assert rc != 0 and frag in egx_lib.egx_last_error(), egx_lib.egx_last_error()
    # the inference calls keep refusing dropout
    nb = C.c_size_t(0)
    assert egx_lib.egx_ragged_encode_workspace(C.byref(_cfg()), _segs(), 1, ok, C.byref(nb)) != 0 and b"inference-only" in egx_lib.egx_last_error()
    # the decoder
    rc, _, _ = _dws(egx_lib, _dcfg(S=100), [50, 101])
    assert rc != 0 and b"clip 1" in egx_lib.egx_last_error()
    assert _dws(egx_lib, _dcfg(S=100), [0])[0] != 0
    assert _dws(egx_lib, _dcfg(S=1025), [10])[0] != 0
    from egot2_amd._lib import DecConfig
    rc, _, _ = _dws(egx_lib, DecConfig(256, 4, 2048, 3, 7, 2, 100, 1e-5, 0, 0.1, 0.1, None), [10])        # compute f32: the composed decoder's
    assert rc != 0 and b"bf16" in egx_lib.egx_last_error()
    rc, _, _ = _dws(egx_lib, DecConfig(256, 4, 2048, 3, 7, 9, 100, 1e-5, 1, 0.1, 0.1, None), [10])        # sy = 9
    assert rc != 0 and b"sy" in egx_lib.egx_last_error()
    assert _dws(egx_lib, _dcfg(S=100), [10, 100])[0] == 0
    nb = C.c_size_t(0)
    lens = (C.c_int * 1)(10)
    assert egx_lib.egx_decoder_ragged_workspace(C.byref(_dcfg(S=100)), 1, lens, C.byref(nb)) != 0 and b"inference only" in egx_lib.egx_last_error()


class _Refuse:
    """Stands in for the loaded library: any attribute access means device work was about to start."""
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} reached before validation finished")


def test_model_level_validation_runs_before_any_device_work(monkeypatch):
    from egot2_amd import _lib, functional as F_egx, hhi_multitask
    from egot2_amd.synth import HHI_G_VOCAB, hhi_args
    monkeypatch.setattr(_lib, "load", lambda: _Refuse())
    m = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=3, dropout=0.1), HHI_G_VOCAB).train()
    f = [torch.zeros(2, 20, 256)] * 3
    y = torch.zeros(2, 2, dtype=torch.long)
    with pytest.raises(ValueError, match="1 .. 20"):
        m.encode_features_ragged("ttm", *f, lengths=[15, 21])
    with pytest.raises(ValueError, match="1 .. 20"):
        m.encode_features_ragged("ttm", *f, lengths=[-1, 20])
    with pytest.raises(ValueError, match="integers"):
        m.encode_features_ragged("ttm", *f, lengths=torch.tensor([15.0, 20.0]))
    with pytest.raises(ValueError, match="equal length"):
        m.encode_features_ragged("asd", *f, lengths=[[15, 15, 15], [15, 16, 15]])
    with pytest.raises(ValueError, match="shape"):
        m.encode_features_ragged("lam", f[0], lengths=[[15, 15], [15, 15]])
    with pytest.raises(ValueError, match="1 .. 20"):
        m.forward_features_ragged("ttm", *f, y, lengths=[0, 20])
    with pytest.raises(ValueError, match="packed"):
        m.decode_ragged(y, torch.zeros(10, 256), [5, 6])
    with pytest.raises(ValueError, match="memory_lengths"):
        m.decode_ragged(y, torch.zeros(10, 256), [10])
    with pytest.raises(ValueError, match="integers"):
        m.decode_ragged(y, torch.zeros(10, 256), torch.tensor([5.0, 5.0]))
    with pytest.raises(ValueError, match="packed"):
        m.decode_ragged(y, torch.zeros(10, 256), [-5, 15])
    m.egx_defer_small = True
    with pytest.raises(ValueError, match="egx_defer_small"):
        m.encode_features_ragged("ttm", *f, lengths=[15, 20])
    m.egx_defer_small = False
    monkeypatch.setattr(F_egx, "bucket_hook", lambda flat, lo, hi: None)
    with pytest.raises(ValueError, match="bucket_cb"):
        m.encode_features_ragged("ttm", *f, lengths=[15, 20])
    monkeypatch.setattr(F_egx, "bucket_hook", None)
    # the inference keywords keep their refusals
    with pytest.raises(ValueError, match="inference-only"):
        m.encode_features("ttm", *f, lengths=[15, 20])
    with pytest.raises(ValueError, match="inference-only"):
        m.decode(y, torch.zeros(10, 256), memory_lengths=[5, 5])


def test_backward_row_maps_invert_the_forward_maps():
    """The backward reads the gradient of compacted row r at the token row the forward wrote it to, and (out_layout 1) the gradient of token
    row i at the output row the forward scattered it to: ragged_token_rows() is that map, a permutation of the output rows in both layouts, and
    its inverse gathers an output-layout tensor back into clip-major token order."""
    from egot2_amd import functional as F_egx
    lens = torch.tensor([[2, 2, 2], [1, 1, 1], [4, 4, 4]], dtype=torch.int32)
    N = int(lens.sum())
    for layout in (0, 1):
        rows = F_egx.ragged_token_rows(lens, layout)
        assert sorted(rows.tolist()) == list(range(N))                      # every output row written exactly once
        inv = torch.empty(N, dtype=torch.int64)
        inv[rows] = torch.arange(N)
        tok = torch.arange(N, dtype=torch.float32)[:, None] * torch.ones(1, 3)
        out = torch.empty_like(tok)
        out[rows] = tok                                                     # forward: token i -> output row rows[i]
        assert torch.equal(out[rows], tok) and torch.equal(out.index_select(0, rows), tok)       # backward: gradient of token i from row rows[i]
        assert torch.equal(tok.index_select(0, inv), out)
    # frame-major: row 3 f + k is segment k of frame f (frames counted over the clips in order)
    rows = F_egx.ragged_token_rows(lens, 1).tolist()
    assert rows[:6] == [0, 3, 1, 4, 2, 5] and rows[6:9] == [6, 7, 8] and rows[9:13] == [9, 12, 15, 18]
    # unequal segments (out_layout 0): packed clip after clip
    assert F_egx.ragged_token_rows(torch.tensor([[2, 5, 1], [3, 1, 1]], dtype=torch.int32), 0).tolist() == list(range(13))


def test_host_planning_against_the_product_library(egx_lib):
    from tests import host_paths_ragged_g_train as hp
    assert hp.exercise(egx_lib) == 16


def test_ragged_g_train_tables_under_address_and_ub_sanitizers():
    """The host planning of the ragged training entry points (tests/host_paths_ragged_g_train.py) against the host-sanitized build in a child
    process, as tests/test_cpu_ragged_g.py runs the inference calls': host code on a CPU build only."""
    import os
    import subprocess
    import sys
    from egot2_amd import build as egx_build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = egx_build.build_sanitized()
    env = dict(os.environ, LD_PRELOAD=egx_build.asan_runtime(), ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", PYTHONPATH=root)
    env.pop("EGX_LIB", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "host_paths_ragged_g_train.py"), lib], capture_output=True, text=True,
                       env=env, timeout=900, cwd=root)
    assert r.returncode == 0 and "ragged g train host ok: 16" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
