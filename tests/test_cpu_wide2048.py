"""d_model up to 2048 on the wide bf16 path, on the host without a GPU: the gate of tests/test_gpu_wide2048.py tested on itself (a perturbed
reference misses the output bar), the distance between the two references (tests/wide2048_ref.py: R, the oracle on bf16-rounded weights and
features, against the exact oracle E) and the library's host-only limits (egx_encoder_workspace, egx_encoder_impl,
egx_ragged_encode_workspace through ctypes)."""
import ctypes as C
import math

import pytest

from tests import wide2048_ref as w

_CACHE = {}


def _case(n, h):
    """The state dict, features and both references of (n, heads) at d = 2048, one layer, B = 3: computed once."""
    if (n, h) not in _CACHE:
        _, sd = w.make_model(n, 2048, h, 1)
        feats = w.make_feats(w.B_SMALL, n, 2048)
        _CACHE[(n, h)] = (sd, feats, w.oracle(sd, h, feats, rounded=False), w.oracle(sd, h, feats, rounded=True))
    return _CACHE[(n, h)]


# ---- 1: the gate can fail ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perturb", ["scale256", "no_pe"])
def test_perturbed_reference_misses_the_output_bar(perturb):
    """R with the attention scale of head dim 256 at head dim 512, and R without the learned positions, each against R."""
    sd, feats, _, (ro, _) = _case(2, 4)
    po, _ = w.oracle(sd, 4, feats, rounded=True, grads=False, perturb=perturb)
    e = w.out_err(po, ro)
    print(f"WIDE2048 cpu perturbed R ({perturb}) at d = 2048, h = 4, n = 2: output error {e:.3e} = {e / w.OUT_BAR:.3g} x the {w.OUT_BAR:g} bar")
    assert e > w.OUT_BAR


# ---- 2: R against E ------------------------------------------------------------------------------------------------------------------------
def test_rounded_reference_against_exact_reference():
    lines = []
    for n, h in w.RE_CASES:
        _, _, (eo, eg), (ro, rg) = _case(n, h)
        ge = w.grad_errs(rg, eg)
        worst = max(ge, key=ge.get)
        lines.append(f"n = {n}, h = {h}, d = 2048, L = 1, B = {w.B_SMALL}: R vs E outputs {w.out_err(ro, eo):.3e}, worst gradient {ge[worst]:.3e} ({worst})")
        print("WIDE2048 cpu", lines[-1])
        assert math.isfinite(w.out_err(ro, eo)) and all(math.isfinite(v) for v in ge.values())
    w.record("cpu: R against E (p = 0, weight seed 33, feature seed 40)", lines)


# ---- 3: host limits ------------------------------------------------------------------------------------------------------------------------
def _cfg(d, heads, compute=1, impl=0, d_ff=2048, L=1, nseg=2):
    from egot2_amd._lib import Config
    return Config(d, heads, d_ff, L, nseg, 1e-5, compute, impl, 0.0, 0.0, 0.0)


def _segs(d, T, proj=False):
    """Two streams of T tokens: identity segments d wide (the 2048-wide 2-task translator), or projected from 2048 (ragged encode)."""
    from egot2_amd._lib import Segment
    segs = (Segment * 2)()
    for s in segs:
        s.T, s.d_in, s.proj_w = T, (2048 if proj else d), (1 if proj else None)
    return segs


def _err(lib):
    return lib.egx_last_error().decode()


def test_host_limits_of_the_2048_wide_path(egx_lib):
    from egot2_amd import _lib
    lib = egx_lib
    sv, sc = C.c_size_t(0), C.c_size_t(0)

    def ws(cfg, segs, B=3):
        return lib.egx_encoder_workspace(C.byref(cfg), segs, B, C.byref(sv), C.byref(sc))

    # the recipe: d = 2048, 4 heads of 512, S = 4, bf16 -> the wide path, with a workspace
    assert ws(_cfg(2048, 4), _segs(2048, 2)) == 0, _err(lib)
    assert sv.value > 0 and sc.value > 0
    assert lib.egx_encoder_impl(C.byref(_cfg(2048, 4)), _segs(2048, 2), 3) == _lib.EGX_IMPL_WIDE
    assert ws(_cfg(2048, 8), _segs(2048, 8)) == 0, _err(lib)                    # head dim 256, a full 16-token tile
    assert ws(_cfg(1536, 12), _segs(1536, 4)) == 0, _err(lib)                   # head dim 128 on the S <= 128 attention
    lib.egx_launch_count(1)
    # compute f32s (2) and f32 (0): the wide path is bf16
    for compute in (2, 0):
        assert ws(_cfg(2048, 4, compute=compute), _segs(2048, 2)) != 0
        assert "compute bf16, wide path" in _err(lib) and "1024" in _err(lib), _err(lib)
    # impl generic
    assert ws(_cfg(2048, 4, impl=_lib.EGX_IMPL_GENERIC), _segs(2048, 2)) != 0
    assert "compute bf16, wide path" in _err(lib), _err(lib)
    assert lib.egx_encoder_impl(C.byref(_cfg(2048, 4, impl=_lib.EGX_IMPL_GENERIC)), _segs(2048, 2), 3) == -1
    # S = 17 at head dim 512: no attention class
    segs17 = _segs(2048, 8)
    segs17[1].T = 9
    assert ws(_cfg(2048, 4), segs17) != 0
    assert all(t in _err(lib) for t in ("compute bf16, wide path", "S=17", "head dim 512", "S <= 16")), _err(lib)
    # nothing above 2048
    assert ws(_cfg(2176, 4), _segs(2176, 2)) != 0
    assert "d_model=2176" in _err(lib) and "2048" in _err(lib), _err(lib)
    # ragged batches stay at 1024
    lengths = (C.c_int * 6)(2, 2, 1, 2, 2, 1)
    nbytes = C.c_size_t(0)
    assert lib.egx_ragged_encode_workspace(C.byref(_cfg(2048, 4)), _segs(2048, 2, proj=True), 3, C.addressof(lengths), C.byref(nbytes)) != 0
    assert "ragged encode" in _err(lib) and "[256, 1024]" in _err(lib), _err(lib)
    assert lib.egx_ragged_encode_workspace(C.byref(_cfg(1024, 8)), _segs(1024, 2, proj=True), 3, C.addressof(lengths), C.byref(nbytes)) == 0, _err(lib)
    assert lib.egx_launch_count(0) == 0           # host-only: nothing was launched
