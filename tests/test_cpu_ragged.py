"""Ragged batches (egx_ragged_workspace / egx_ragged_fwd, ABI v17) on the host, without a GPU: the workspace query and the argument
validation of the library, and the Python-side length handling of functional.ragged_lengths / encoder_ragged. The workspace query is
pure host arithmetic (no HIP call), as the other workspace queries tests/host_paths.py drives."""
import ctypes as C

import pytest
import torch


def _cfg(compute=2, L=1, p_drop=0.0, impl=0, nseg=3):
    from egot2_amd._lib import Config
    return Config(128, 4, 2048, L, nseg, 1e-5, compute, impl, p_drop, 0.0, 0.0)


def _segs(T=150, nseg=3):
    from egot2_amd._lib import Segment
    segs = (Segment * nseg)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1     # non-null marker: the query reads no weight
    return segs


def _ws(lib, cfg, segs, lengths):
    lens = (C.c_int * len(lengths))(*lengths)
    nb = C.c_size_t(0)
    rc = lib.egx_ragged_workspace(C.byref(cfg), segs, len(lengths) // cfg.n_segments, lens, C.byref(nb))
    return rc, nb.value


def test_ragged_workspace_grows_with_tokens_not_with_longest_clip(egx_lib):
    cfg, segs = _cfg(), _segs()
    rc, one_long = _ws(egx_lib, cfg, segs, [150] * 3)
    assert rc == 0 and one_long > 0
    # 64 clips of 15 frames + one of 150: sum S_b = 64 * 45 + 450 tokens, far below B * S_max = 65 * 450
    rc, mixed = _ws(egx_lib, cfg, segs, [15] * 3 * 64 + [150] * 3)
    assert rc == 0
    rc, uniform = _ws(egx_lib, cfg, segs, [150] * 3 * 65)
    assert rc == 0
    assert mixed < uniform / 3, (mixed, uniform)
    # linear in the token count: doubling every clip's frames (same tile count per clip up to rounding) about doubles the bytes
    rc, small = _ws(egx_lib, cfg, segs, [16] * 3 * 100)      # S_b = 48: one tile each
    rc2, big = _ws(egx_lib, cfg, segs, [32] * 3 * 100)       # S_b = 96: two tiles each
    assert rc == 0 and rc2 == 0 and 1.6 < big / small < 2.4, (small, big)
    # the weight copies live in the workspace unless a weight cache is given; the rest scales with N, not with B * S_max
    rc, b1 = _ws(egx_lib, cfg, segs, [20, 30, 40])
    assert rc == 0 and b1 < one_long


@pytest.mark.parametrize("lengths,what", [
    ([0, 15, 15], b"1 .. 150"),          # a segment without frames
    ([151, 15, 15], b"1 .. 150"),        # beyond the padded length
    ([-3, 15, 15], b"1 .. 150"),
])
def test_ragged_workspace_refuses_bad_lengths(egx_lib, lengths, what):
    rc, _ = _ws(egx_lib, _cfg(), _segs(), [15] * 3 + lengths)
    assert rc != 0
    assert what in egx_lib.egx_last_error() and b"clip 1" in egx_lib.egx_last_error()


def test_ragged_workspace_refuses_long_clips_and_training_configs(egx_lib):
    rc, _ = _ws(egx_lib, _cfg(), _segs(T=200), [200, 200, 113])      # S_b = 513
    assert rc != 0 and b"S=513" in egx_lib.egx_last_error()
    rc, _ = _ws(egx_lib, _cfg(), _segs(T=200), [200, 200, 112])      # S_b = 512: the limit
    assert rc == 0
    rc, _ = _ws(egx_lib, _cfg(p_drop=0.1), _segs(), [15] * 3)
    assert rc != 0 and b"inference-only" in egx_lib.egx_last_error()
    rc, _ = _ws(egx_lib, _cfg(compute=0), _segs(), [15] * 3)          # exact fp32: not on the tiled kernels
    assert rc != 0 and b"compute" in egx_lib.egx_last_error()
    rc, _ = _ws(egx_lib, _cfg(L=7), _segs(), [15] * 3)
    assert rc != 0
    rc, _ = _ws(egx_lib, _cfg(impl=1), _segs(), [15] * 3)             # a forced other implementation
    assert rc != 0 and b"impl" in egx_lib.egx_last_error()
    cfg = _cfg()
    cfg.out_tokens = 15
    rc, _ = _ws(egx_lib, cfg, _segs(), [15] * 3)
    assert rc != 0 and b"out_tokens" in egx_lib.egx_last_error()
    cfg = _cfg()
    cfg.ce = 1
    rc, _ = _ws(egx_lib, cfg, _segs(), [15] * 3)
    assert rc != 0 and b"ce" in egx_lib.egx_last_error()
    nb = C.c_size_t(0)
    assert egx_lib.egx_ragged_workspace(C.byref(_cfg()), _segs(), 1, None, C.byref(nb)) != 0
    assert b"lengths" in egx_lib.egx_last_error()


def test_ragged_lengths_expansion_and_validation():
    from egot2_amd import functional as F_egx
    t = F_egx.ragged_lengths([15, 20, 150], 3, [150, 150, 150])
    assert t.dtype == torch.int32 and t.device.type == "cpu" and tuple(t.shape) == (3, 3)
    assert t.tolist() == [[15] * 3, [20] * 3, [150] * 3]
    t = F_egx.ragged_lengths(torch.tensor([[1, 2, 3], [4, 5, 6]]), 2, [10, 10, 10], order=(2, 0, 1))
    assert t.tolist() == [[3, 1, 2], [6, 4, 5]]
    # the per-column bound follows the column's own padded length, after the reordering
    assert F_egx.ragged_lengths([[30, 5]], 1, [5, 30], order=(1, 0)).tolist() == [[5, 30]]
    with pytest.raises(ValueError, match="1 .. 5"):
        F_egx.ragged_lengths([[30, 6]], 1, [5, 30], order=(1, 0))
    with pytest.raises(ValueError, match="1 .. 150"):
        F_egx.ragged_lengths([15, 0], 2, [150, 150])
    with pytest.raises(ValueError, match="1 .. 150"):
        F_egx.ragged_lengths([15, 151], 2, [150, 150])
    with pytest.raises(ValueError, match="shape"):
        F_egx.ragged_lengths([15, 15, 15], 2, [150, 150])
    with pytest.raises(ValueError, match="shape"):
        F_egx.ragged_lengths([[15, 15, 15]], 1, [150, 150])
    with pytest.raises(ValueError, match="integers"):
        F_egx.ragged_lengths([15.0, 16.0], 2, [150, 150])


def test_ragged_refusals_before_any_device_work():
    """Training mode, grad mode and fused losses are refused by the model methods before a tensor is touched."""
    from egot2_amd import hhi_asd, hhi_ttm
    from egot2_amd.synth import hhi_args
    model = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args())
    f = [torch.zeros(2, 20, 256)] * 3
    with pytest.raises(ValueError, match="inference-only"):
        model.train().forward_features(*f, lengths=[15, 20])
    with pytest.raises(ValueError, match="inference-only"):
        model.eval().forward_features(*f, lengths=[15, 20])                 # grad enabled, parameters require grad
    with torch.no_grad(), pytest.raises(ValueError, match="inference-only"):
        model.eval().forward_features(*f, target=torch.zeros(2, dtype=torch.long), lengths=[15, 20])
    asd = hhi_asd.TaskFusionMFTransformer3Task(hhi_args()).eval()
    with torch.no_grad(), pytest.raises(ValueError, match="inference-only"):
        asd.forward_features(*f, lossav=hhi_asd.lossAV(128), labels=torch.zeros(35, dtype=torch.long), lengths=[15, 20])
    with torch.no_grad(), pytest.raises(ValueError, match="1 .. 20"):
        asd.forward_features(*f, lengths=[15, 21])


_ASAN_CHILD = r"""
import ctypes as C, sys
from tests.host_paths import bind
from egot2_amd._lib import Config, Segment
lib = bind(sys.argv[1])
n = 0
for B, T, L in [(1, 150, 1), (40, 150, 2), (256, 150, 1), (700, 60, 1)]:
    segs = (Segment * 3)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, 256, 1
    for seed in range(4):
        lens = [1 + (b * 7919 + k * 104729 + seed * 31) % T for b in range(B) for k in range(3)]
        arr = (C.c_int * len(lens))(*lens)
        nb = C.c_size_t(0)
        assert lib.egx_ragged_workspace(C.byref(Config(128, 4, 2048, L, 3, 1e-5, 2, 0, 0.0, 0.0, 0.0)), segs, B, arr, C.byref(nb)) == 0
        n += 1
print(f"ragged host ok: {n}")
"""


def test_ragged_batch_table_under_address_and_ub_sanitizers():
    """The host planning of egx_ragged_fwd (per-clip records + the clip of every tile) against the host-sanitized build, as
    tests/test_cpu_host.py runs the other host paths: an out-of-bounds or stale read while the table is built aborts the child."""
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
    assert r.returncode == 0 and "ragged host ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
