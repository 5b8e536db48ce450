"""Host-only planning of the ragged TRAINING entry points for the EgoT2-g HHI model (egx_ragged_encode_train_* / egx_ragged_encode_bwd,
egx_decoder_ragged_train_* / egx_decoder_ragged_bwd) driven through ctypes without torch and without a GPU: clip records, attention classes,
row maps, the saved / scratch layouts over them, and every refusal that comes before the first device call. Run two ways, as
tests/host_paths.py:

  * imported by tests/test_cpu_ragged_g_train.py against the product library;
  * as a script in a subprocess with the ASAN runtime preloaded against the host-sanitized build (egot2_amd/build.py build_sanitized:
    AddressSanitizer + UBSan on the C++ orchestration, never on the GPU): `python tests/host_paths_ragged_g_train.py <lib.so>`.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def bind(path):
    from egot2_amd import _lib
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.egx_abi_version() == _lib.EGX_ABI_VERSION
    return lib


def exercise(lib) -> int:
    """Returns the number of plans built; raises AssertionError on a wrong answer."""
    from egot2_amd._lib import Config, DecConfig, Segment
    n = 0
    for B, T, K in [(1, 150, 3), (40, 150, 3), (256, 150, 3), (700, 60, 1)]:
        segs = (Segment * K)()
        for s in segs:
            s.T, s.d_in, s.proj_w = T, 256, 1
        for seed in range(4):
            lens = [1 + (b * 7919 + k * 104729 + seed * 31) % T for b in range(B) for k in range(K)]
            arr = (C.c_int * len(lens))(*lens)
            sv, sc = C.c_size_t(0), C.c_size_t(0)
            cfg = Config(256, 4, 2048, 3, K, 1e-5, 1, 0, 0.1, 0.1, 0.0)
            assert lib.egx_ragged_encode_train_workspace(C.byref(cfg), segs, B, arr, C.byref(sv), C.byref(sc)) == 0
            assert sv.value > 0 and sc.value > 0
            # the forward and the backward build the whole table (out_layout 0 and 1) before they look at a pointer
            for layout in (0, 1):
                rc = lib.egx_ragged_encode_train_fwd(C.byref(cfg), segs, arr, None, None, None, B, None, layout, None, 1, 7, None)
                assert rc != 0 and lib.egx_last_error()
                rc = lib.egx_ragged_encode_bwd(C.byref(cfg), segs, arr, None, None, B, None, layout, None, None, None, None, None, None, 1, 7, None)
                assert rc != 0 and lib.egx_last_error()
            eq = [lens[b * K] for b in range(B) for _ in range(K)]        # equal segment lengths: the frame-major map is built
            earr = (C.c_int * len(eq))(*eq)
            if 3 * max(eq) <= 480 or K == 1:
                rc = lib.egx_ragged_encode_train_fwd(C.byref(cfg), segs, earr, None, None, None, B, None, 1, None, 1, 7, None)
                assert rc != 0 and b"null pointer" in lib.egx_last_error(), lib.egx_last_error()
            S = [sum(lens[b * K:(b + 1) * K]) for b in range(B)]
            darr = (C.c_int * B)(*S)
            dc = DecConfig(256, 4, 2048, 3, 7, 2, max(S), 1e-5, 1, 0.1, 0.1, None)
            assert lib.egx_decoder_ragged_train_workspace(C.byref(dc), B, darr, C.byref(sv), C.byref(sc)) == 0 and sv.value > 0 and sc.value > 0
            rc = lib.egx_decoder_ragged_train_fwd(C.byref(dc), None, None, darr, None, None, 0, None, None, None, B, None, None, None, 1, 7, None)
            assert rc != 0 and b"null pointer" in lib.egx_last_error()
            rc = lib.egx_decoder_ragged_bwd(C.byref(dc), None, darr, None, None, B, None, None, None, None, None, None, None, None, None, 0, 1, 7, None)
            assert rc != 0 and b"null pointer" in lib.egx_last_error()
            n += 1
    return n


if __name__ == "__main__":
    print(f"ragged g train host ok: {exercise(bind(sys.argv[1]))}")
