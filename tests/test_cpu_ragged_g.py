"""Ragged batches for the EgoT2-g HHI model on the host, without a GPU (ABI v18: egx_ragged_encode_workspace / egx_ragged_encode,
egx_decoder_ragged_workspace / egx_decoder_ragged_fwd): symbols, the workspace queries, the argument validation of the library and of the
model methods. The workspace queries and every refusal below are pure host work (no HIP call)."""
import ctypes as C

import pytest
import torch


def _cfg(compute=1, L=3, p_drop=0.0, impl=0, nseg=3, d=256):
    from egot2_amd._lib import Config
    return Config(d, 4, 2048, L, nseg, 1e-5, compute, impl, p_drop, 0.0, 0.0)


def _segs(T=150, nseg=3):
    from egot2_amd._lib import Segment
    segs = (Segment * nseg)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1     # non-null marker: the query reads no weight
    return segs


def _ws(lib, cfg, segs, lengths):
    lens = (C.c_int * len(lengths))(*lengths)
    nb = C.c_size_t(0)
    rc = lib.egx_ragged_encode_workspace(C.byref(cfg), segs, len(lengths) // cfg.n_segments, lens, C.byref(nb))
    return rc, nb.value


def _dcfg(S=1024, p_drop=0.0):
    from egot2_amd._lib import DecConfig, EGX_BF16
    return DecConfig(256, 4, 2048, 3, 7, 2, S, 1e-5, EGX_BF16, p_drop, 0.0, None)


def _dws(lib, cfg, lengths):
    lens = (C.c_int * len(lengths))(*lengths)
    nb = C.c_size_t(0)
    return lib.egx_decoder_ragged_workspace(C.byref(cfg), len(lengths), lens, C.byref(nb)), nb.value


def test_abi_18_and_symbols(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    for name in ("egx_ragged_encode_workspace", "egx_ragged_encode", "egx_decoder_ragged_workspace", "egx_decoder_ragged_fwd"):
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES


def test_encode_workspace_grows_with_tokens_not_with_longest_clip(egx_lib):
    cfg, segs = _cfg(), _segs()
    rc, one_long = _ws(egx_lib, cfg, segs, [150] * 3)
    assert rc == 0 and one_long > 0
    rc, mixed = _ws(egx_lib, cfg, segs, [15] * 3 * 64 + [150] * 3)       # sum S_b = 64 * 45 + 450, B * S_max = 65 * 450
    assert rc == 0
    rc, uniform = _ws(egx_lib, cfg, segs, [150] * 3 * 65)
    assert rc == 0 and mixed < uniform / 3, (mixed, uniform)
    rc, small = _ws(egx_lib, cfg, segs, [20] * 3 * 200)
    rc2, big = _ws(egx_lib, cfg, segs, [40] * 3 * 200)
    assert rc == 0 and rc2 == 0
    rc3, weights = _ws(egx_lib, cfg, segs, [1] * 3)                       # ~ the bf16 weight copies alone
    assert rc3 == 0 and 1.8 < (big - weights) / (small - weights) < 2.2, (small, big, weights)
    # the decoder's: sum_b S_b memory rows, not B * cfg.S
    rc, d_small = _dws(egx_lib, _dcfg(), [1] * 63 + [1024])
    rc2, d_big = _dws(egx_lib, _dcfg(), [1024] * 64)
    assert rc == 0 and rc2 == 0 and d_small < d_big / 4, (d_small, d_big)


@pytest.mark.parametrize("lengths,what", [
    ([0, 15, 15], b"1 .. 150"),
    ([151, 15, 15], b"1 .. 150"),
    ([-3, 15, 15], b"1 .. 150"),
])
def test_encode_workspace_refuses_bad_lengths(egx_lib, lengths, what):
    rc, _ = _ws(egx_lib, _cfg(), _segs(), [15] * 3 + lengths)
    assert rc != 0
    assert what in egx_lib.egx_last_error() and b"clip 1" in egx_lib.egx_last_error()


def test_encode_refuses_long_clips_training_and_other_arithmetic(egx_lib):
    rc, _ = _ws(egx_lib, _cfg(), _segs(T=200), [200, 200, 81])             # S_b = 481: beyond the long attention at head dim 64
    assert rc != 0 and b"S=481" in egx_lib.egx_last_error()
    rc, _ = _ws(egx_lib, _cfg(), _segs(T=200), [200, 200, 80])             # 480: the limit
    assert rc == 0
    rc, _ = _ws(egx_lib, _cfg(p_drop=0.1), _segs(), [15] * 3)
    assert rc != 0 and b"inference-only" in egx_lib.egx_last_error()
    for compute in (0, 2):                                                  # f32, f32s: the grouped fallback's business
        rc, _ = _ws(egx_lib, _cfg(compute=compute), _segs(), [15] * 3)
        assert rc != 0 and b"bf16" in egx_lib.egx_last_error()
    rc, _ = _ws(egx_lib, _cfg(impl=1), _segs(), [15] * 3)
    assert rc != 0 and b"impl" in egx_lib.egx_last_error()
    for field in ("ce", "token_ce", "out_tokens"):
        cfg = _cfg()
        setattr(cfg, field, 1)
        rc, _ = _ws(egx_lib, cfg, _segs(), [15] * 3)
        assert rc != 0, field
    nb = C.c_size_t(0)
    assert egx_lib.egx_ragged_encode_workspace(C.byref(_cfg()), _segs(), 1, None, C.byref(nb)) != 0
    # out_layout 1 (the asd memory) needs equal segment lengths per clip; refused in the planning, before any pointer is touched
    lens = (C.c_int * 6)(15, 15, 15, 15, 16, 15)
    assert egx_lib.egx_ragged_encode(C.byref(_cfg()), _segs(), lens, None, None, None, 2, None, 1, None, None) != 0
    assert b"equal segment lengths" in egx_lib.egx_last_error() and b"clip 1" in egx_lib.egx_last_error()
    assert egx_lib.egx_ragged_encode(C.byref(_cfg()), _segs(), lens, None, None, None, 2, None, 2, None, None) != 0
    assert b"out_layout" in egx_lib.egx_last_error()
    # the existing d = 128 ragged entry point keeps refusing d >= 256
    from egot2_amd._lib import Config
    n = C.c_size_t(0)
    assert egx_lib.egx_ragged_workspace(C.byref(Config(256, 4, 2048, 3, 3, 1e-5, 1, 0, 0.0, 0.0, 0.0)), _segs(), 1,
                                        (C.c_int * 3)(15, 15, 15), C.byref(n)) != 0


def test_decoder_ragged_refusals(egx_lib):
    rc, _ = _dws(egx_lib, _dcfg(S=100), [50, 101])
    assert rc != 0 and b"clip 1" in egx_lib.egx_last_error()
    rc, _ = _dws(egx_lib, _dcfg(S=100), [0])
    assert rc != 0
    rc, _ = _dws(egx_lib, _dcfg(S=1025), [10])
    assert rc != 0
    rc, _ = _dws(egx_lib, _dcfg(p_drop=0.1), [10])
    assert rc != 0 and b"inference only" in egx_lib.egx_last_error()


def test_model_validation_runs_before_any_device_work():
    """CPU model and CPU features: every refusal is a ValueError raised before a tensor reaches the library."""
    from egot2_amd import hhi_multitask
    from egot2_amd.synth import HHI_G_VOCAB, hhi_args
    m = hhi_multitask.TaskTranslationPromptTransformer(hhi_args(hidden_dim=256, num_heads=4, num_layers=3, dropout=0.0), HHI_G_VOCAB)
    f = [torch.zeros(2, 20, 256)] * 3
    with pytest.raises(ValueError, match="inference-only"):
        m.train().encode_features("ttm", *f, lengths=[15, 20])
    with pytest.raises(ValueError, match="inference-only"):
        m.eval().encode_features("ttm", *f, lengths=[15, 20])                  # grad enabled, trainable parameters
    with pytest.raises(ValueError, match="inference-only"):
        m.eval().predict_features("ttm", *f, lengths=[15, 20])
    with pytest.raises(ValueError, match="inference-only"):
        m.eval().decode(torch.zeros(2, 1, dtype=torch.long), torch.zeros(10, 256), memory_lengths=[5, 5])
    with torch.no_grad():
        with pytest.raises(ValueError, match="1 .. 20"):
            m.encode_features("ttm", *f, lengths=[15, 21])
        with pytest.raises(ValueError, match="equal length"):
            m.encode_features("asd", *f, lengths=[[15, 15, 15], [15, 16, 15]])
        with pytest.raises(ValueError, match="shape"):
            m.encode_features("lam", f[0], lengths=[[15, 15], [15, 15]])
        with pytest.raises(ValueError, match="packed"):
            m.decode(torch.zeros(2, 1, dtype=torch.long), torch.zeros(10, 256), memory_lengths=[5, 6])
        with pytest.raises(ValueError, match="memory_lengths"):
            m.decode(torch.zeros(2, 1, dtype=torch.long), torch.zeros(10, 256), memory_lengths=[10])


def test_token_rows_of_the_frame_major_layout():
    from egot2_amd import functional as F_egx
    lens = torch.tensor([[2, 2, 2], [1, 1, 1]], dtype=torch.int32)
    # clip-major token order (clip, segment, frame) -> row 3 f + k
    assert F_egx.ragged_token_rows(lens, 1).tolist() == [0, 3, 1, 4, 2, 5, 6, 7, 8]
    assert F_egx.ragged_token_rows(lens, 0).tolist() == list(range(9))


_ASAN_CHILD = r"""
import ctypes as C, sys
from tests.host_paths import bind
from egot2_amd._lib import Config, DecConfig, Segment
lib = bind(sys.argv[1])
n = 0
for B, T, K in [(1, 150, 3), (40, 150, 3), (256, 150, 3), (700, 60, 1)]:
    segs = (Segment * K)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1
    for seed in range(4):
        lens = [1 + (b * 7919 + k * 104729 + seed * 31) % T for b in range(B) for k in range(K)]
        arr = (C.c_int * len(lens))(*lens)
        nb = C.c_size_t(0)
        assert lib.egx_ragged_encode_workspace(C.byref(Config(256, 4, 2048, 3, K, 1e-5, 1, 0, 0.0, 0.0, 0.0)), segs, B, arr, C.byref(nb)) == 0
        # out_layout 1 with unequal lengths: the full table is built, then refused
        assert lib.egx_ragged_encode(C.byref(Config(256, 4, 2048, 3, K, 1e-5, 1, 0, 0.0, 0.0, 0.0)), segs, arr, None, None, None, B, None,
                                     1, None, None) != 0 or K == 1 or B == 1
        S = [sum(lens[b * K:(b + 1) * K]) for b in range(B)]
        darr = (C.c_int * B)(*S)
        assert lib.egx_decoder_ragged_workspace(C.byref(DecConfig(256, 4, 2048, 3, 7, 2, max(S), 1e-5, 1, 0.0, 0.0, None)), B, darr,
                                                C.byref(nb)) == 0
        n += 1
print(f"ragged g host ok: {n}")
"""


def test_ragged_g_tables_under_address_and_ub_sanitizers():
    """The host planning of egx_ragged_encode (clip records, attention classes, row maps) and egx_decoder_ragged_* against the host-sanitized
    build in a child process, as tests/test_cpu_ragged.py runs egx_ragged_fwd's."""
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
    assert r.returncode == 0 and "ragged g host ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
