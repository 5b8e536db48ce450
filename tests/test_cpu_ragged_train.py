"""Ragged training batches (egx_ragged_train_workspace / egx_ragged_train_fwd / egx_ragged_bwd, ABI v18) on the host, without a GPU: the
workspace query and the argument validation of the library, and the model-level validation of forward_features_ragged, all of which must
act before any device work. The workspace query is pure host arithmetic (no HIP call), as the other workspace queries."""
import ctypes as C

import pytest
import torch


def _cfg(compute=2, L=1, p_drop=0.1, p_pos=0.1, p_feat=0.0, impl=0, nseg=3, d=128, h=4):
    from egot2_amd._lib import Config
    return Config(d, h, 2048, L, nseg, 1e-5, compute, impl, p_drop, p_pos, p_feat)


def _segs(T=150, nseg=3):
    from egot2_amd._lib import Segment
    segs = (Segment * nseg)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1     # non-null marker: the query reads no weight
    return segs


def _ws(lib, cfg, segs, lengths):
    lens = (C.c_int * len(lengths))(*lengths)
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    rc = lib.egx_ragged_train_workspace(C.byref(cfg), segs, len(lengths) // cfg.n_segments, lens, C.byref(sv), C.byref(sc))
    return rc, sv.value, sc.value


def test_ragged_train_workspace_grows_with_tokens_not_with_longest_clip(egx_lib):
    cfg, segs = _cfg(), _segs()
    rc, sv1, sc1 = _ws(egx_lib, cfg, segs, [150] * 3)
    assert rc == 0 and sv1 > 0 and sc1 > 0
    # 64 clips of 15 frames + one of 150: sum S_b = 64 * 45 + 450 tokens, far below B * S_max = 65 * 450
    rc, sv_m, sc_m = _ws(egx_lib, cfg, segs, [15] * 3 * 64 + [150] * 3)
    assert rc == 0
    rc, sv_u, sc_u = _ws(egx_lib, cfg, segs, [150] * 3 * 65)
    assert rc == 0
    assert sv_m < sv_u / 3 and sc_m < sc_u / 3, (sv_m, sv_u, sc_m, sc_u)
    # about linear in the token count (S_b = 48: one tile each, S_b = 96: two)
    rc, sv_s, sc_s = _ws(egx_lib, cfg, segs, [16] * 3 * 100)
    rc2, sv_b, sc_b = _ws(egx_lib, cfg, segs, [32] * 3 * 100)
    assert rc == 0 and rc2 == 0 and 1.6 < sv_b / sv_s < 2.4 and 1.4 < sc_b / sc_s < 2.4, (sv_s, sv_b, sc_s, sc_b)
    # the inference workspace of the same batch is the training call's `saved` minus nothing it needs: at most as large
    nb = C.c_size_t(0)
    lens = (C.c_int * 3)(20, 30, 40)
    assert egx_lib.egx_ragged_workspace(C.byref(_cfg(p_drop=0.0, p_pos=0.0)), segs, 1, lens, C.byref(nb)) == 0
    rc, sv, _ = _ws(egx_lib, _cfg(p_drop=0.0, p_pos=0.0), segs, [20, 30, 40])
    assert rc == 0 and nb.value <= sv


def test_ragged_train_refusals(egx_lib):
    from egot2_amd._lib import BUCKET_CB
    ok = [15, 20, 25, 150, 1, 7]

    def refused(cfg, what, segs=None, lengths=ok):
        rc, _, _ = _ws(egx_lib, cfg, segs if segs is not None else _segs(), lengths)
        assert rc != 0, what
        assert what in egx_lib.egx_last_error(), egx_lib.egx_last_error()

    assert _ws(egx_lib, _cfg(), _segs(), ok)[0] == 0                         # dropout (p = 0.1 + 0.1 positional) is training's own case
    refused(_cfg(p_feat=0.1), b"p_feat")
    cfg = _cfg()
    cfg.out_tokens = 15
    refused(cfg, b"out_tokens")
    cfg = _cfg()
    cfg.token_ce = 8                                                        # (any non-null egx_token_ce)
    refused(cfg, b"token_ce")
    cfg = _cfg()
    keep = BUCKET_CB(lambda user, bucket: None)
    cfg.bucket_cb = C.cast(keep, C.c_void_p)
    refused(cfg, b"bucket_cb")
    cfg = _cfg()
    cfg.bwd_stage = 1                                                       # the staged backward (defer_small)
    refused(cfg, b"bwd_stage")
    refused(_cfg(impl=1), b"impl")                                          # a forced other implementation
    refused(_cfg(impl=2), b"impl")
    refused(_cfg(compute=0), b"compute")                                    # exact fp32: not on the tiled kernels
    refused(_cfg(d=256), b"d=128")
    refused(_cfg(L=7), b"layers")
    refused(_cfg(), b"S=513", segs=_segs(T=200), lengths=[200, 200, 113])
    assert _ws(egx_lib, _cfg(), _segs(T=200), [200, 200, 112])[0] == 0    # S_b = 512: the limit
    refused(_cfg(), b"1 .. 150", lengths=[15, 15, 15, 0, 15, 15])
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    assert egx_lib.egx_ragged_train_workspace(C.byref(_cfg()), _segs(), 1, None, C.byref(sv), C.byref(sc)) != 0
    assert b"lengths" in egx_lib.egx_last_error()
    # the inference call keeps its own refusal of training configurations
    nb = C.c_size_t(0)
    lens = (C.c_int * 3)(15, 15, 15)
    assert egx_lib.egx_ragged_workspace(C.byref(_cfg(p_drop=0.1)), _segs(), 1, lens, C.byref(nb)) != 0
    assert b"inference-only" in egx_lib.egx_last_error()


def test_ragged_train_forward_and_backward_refuse_null_arguments(egx_lib):
    """Argument checks of the two calls fire before anything is enqueued (no device is touched: every pointer is null)."""
    from egot2_amd._lib import Layer, LayerGrads
    lens = (C.c_int * 3)(15, 15, 15)
    layers, lgr = (Layer * 1)(), (LayerGrads * 1)()
    assert egx_lib.egx_ragged_train_fwd(C.byref(_cfg()), _segs(), lens, None, None, layers, None, 1, None, None, None, None, 1, 7, None) != 0
    assert b"null" in egx_lib.egx_last_error()
    assert egx_lib.egx_ragged_bwd(C.byref(_cfg()), _segs(), lens, None, None, layers, None, 1, None, None, None, None, None, None, None,
                                  lgr, None, 1, 7, None) != 0
    assert b"null" in egx_lib.egx_last_error()


def test_ragged_train_model_validation_before_device_work():
    """forward_features_ragged checks its lengths, its loss arguments and the staged-backward switch on the host: these models never left
    the CPU, so any device work would fail differently."""
    from egot2_amd import hhi_asd, hhi_ttm
    from egot2_amd.synth import hhi_args
    f = [torch.zeros(2, 20, 256)] * 3
    m3 = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args()).train()
    with pytest.raises(ValueError, match="1 .. 20"):
        m3.forward_features_ragged(*f, lengths=[15, 21])
    with pytest.raises(ValueError, match="1 .. 20"):
        m3.forward_features_ragged(*f, lengths=[[15, 20, 20], [15, 0, 20]])
    with pytest.raises(ValueError, match="shape"):
        m3.forward_features_ragged(*f, lengths=[15, 20, 20])
    with pytest.raises(ValueError, match="class_weight"):
        m3.forward_features_ragged(*f, lengths=[15, 20], class_weight=torch.ones(2))
    m3.egx_defer_small = True
    with pytest.raises(ValueError, match="defer_small"):
        m3.forward_features_ragged(*f, lengths=[15, 20])
    m2 = hhi_ttm.TaskFusionMFTransformer2Task(hhi_args()).eval()
    with pytest.raises(ValueError, match="1 .. 20"):
        m2.forward_features_ragged(*f[:2], lengths=[15, 25])
    asd = hhi_asd.TaskFusionMFTransformer3Task(hhi_args())
    with pytest.raises(ValueError, match="1 .. 20"):
        asd.forward_features_ragged(*f, lengths=[15, 21])
    asd.egx_defer_small = True
    with pytest.raises(ValueError, match="defer_small"):
        asd.forward_features_ragged(*f, lengths=[15, 20])


_ASAN_CHILD = r"""
import ctypes as C, sys
from tests.host_paths import bind
from egot2_amd._lib import Config, Segment
lib = bind(sys.argv[1])
n = 0
for B, T, L, K in [(1, 150, 1, 3), (40, 150, 2, 3), (256, 150, 1, 3), (700, 60, 1, 2), (3, 170, 1, 3)]:
    segs = (Segment * K)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1
    for seed in range(4):
        lens = [1 + (b * 7919 + k * 104729 + seed * 31) % T for b in range(B) for k in range(K)]
        arr = (C.c_int * len(lens))(*lens)
        sv, sc = C.c_size_t(0), C.c_size_t(0)
        rc = lib.egx_ragged_train_workspace(C.byref(Config(128, 4, 2048, L, K, 1e-5, 2, 0, 0.1, 0.1, 0.0)), segs, B, arr, C.byref(sv), C.byref(sc))
        assert rc == 0 or b"S=" in lib.egx_last_error(), lib.egx_last_error()
        n += 1
print(f"ragged train host ok: {n}")
"""


def test_ragged_train_plan_under_address_and_ub_sanitizers():
    """The host planning of the ragged training calls (per-clip records, the tile map, the packed segment rows, the backward's scratch
    layout) against the host-sanitized build in a child process: an out-of-bounds or stale read while the table is built aborts it."""
    import os
    import subprocess
    import sys
    from egot2_amd import build as egx_build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = egx_build.build_sanitized()
    env = dict(os.environ, LD_PRELOAD=egx_build.asan_runtime(), ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", PYTHONPATH=root)
    env.pop("EGX_LIB", None)
    r = subprocess.run([sys.executable, "-c", _ASAN_CHILD, lib], capture_output=True, text=True, env=env, timeout=900, cwd=root)
    assert r.returncode == 0 and "ragged train host ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
