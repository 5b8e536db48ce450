"""Host-only planning of greedy generation (egx_decoder_generate_workspace / egx_decoder_generate) driven through ctypes without torch and
without a GPU: the workspace layout over (B, n_steps, S) and every refusal that comes before the first device call. Run two ways, as
tests/host_paths.py:

  * imported by tests/test_cpu_generate.py against the product library;
  * as a script in a subprocess with the ASAN runtime preloaded against the host-sanitized build (egot2_amd/build.py build_sanitized:
    AddressSanitizer + UBSan on the C++ orchestration, never on the GPU): `python tests/host_paths_generate.py <lib.so>`.
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
    from egot2_amd._lib import DecConfig
    n = 0
    for d, h, L, V in [(256, 4, 2, 7), (512, 8, 3, 600), (1024, 16, 16, 1024), (384, 12, 1, 1)]:
        for B in (1, 37, 256):
            for S in (1, 48, 1024):
                last = 0
                for steps in (1, 2, 40, 64):
                    cfg = DecConfig(d, h, 2048, L, V, 99, S, 1e-5, 1, 0.0, 0.0, None)       # sy = 99: not read
                    nb = C.c_size_t(0)
                    assert lib.egx_decoder_generate_workspace(C.byref(cfg), B, steps, C.byref(nb)) == 0, lib.egx_last_error()
                    assert nb.value > last
                    last = nb.value
                    rc = lib.egx_decoder_generate(C.byref(cfg), None, None, None, None, d, None, None, None, B, steps, None, None, None, None)
                    assert rc != 0 and b"null pointer" in lib.egx_last_error(), lib.egx_last_error()
                    n += 1
    return n


if __name__ == "__main__":
    print(f"generate host ok: {exercise(bind(sys.argv[1]))}")
