"""Every workspace size the d = 128 paths answer, at the smallest shape of each branch of their `saved` layout (fused_host.hip SavedLayout):
per-clip with and without slice sections, tiled, ragged inference, ragged training and the ragged capacity plan. Host-only, no torch.

  * imported by tests/test_cpu_host.py, which compares sizes(lib) of the product library with tests/d128_workspace_sizes.json;
  * as a script it writes that table: `python tests/host_paths_d128_sizes.py <lib.so> <commit>` prints the JSON of a library built from <commit>.
    A refactor keeps the table; where one is needed it comes from a build of the refactor's PARENT commit, never from the code under test.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LENS = [[1, 1, 1], [16, 16, 16], [15, 7, 16], [16, 1, 1]]      # tools/lib_compare.py's ragged batch at T_pad 16
CAPACITY = (6, 112)                                            # and its capacity plan: B_cap clips, tok_cap tokens
UNIFORM = [(15, (1, 3, 256)),       # S 45, per-clip: slice sections at B 1 and 3 with d_ff 2048, none at B 256 or with d_ff 384
           (17, (2, 3)),            # S 51: two tiles per clip
           (110, (2, 3))]           # S 330: seven tiles


def sizes(lib) -> dict:
    from egot2_amd._lib import Config, Segment
    out = {}
    a, b = C.c_size_t(), C.c_size_t()

    def segs_of(T):
        s = (Segment * 3)()
        for x in s:
            x.T, x.d_in, x.proj_w = T, 256, 1       # (a non-null marker: nothing is read)
        return s

    def answer(rc, *vals):
        return [rc] + ([v.value for v in vals] if rc == 0 else [])

    lens = (C.c_int * 12)(*[t for clip in LENS for t in clip])
    for dff in (2048, 384):
        for L in (1, 2):
            for compute in (0, 1, 2):
                cfg = Config(128, 4, dff, L, 3, 1e-5, compute, 0, 0.1, 0.1, 0.0)
                tag = f"dff{dff} L{L} compute{compute}"
                out[f"{tag} weight_cache"] = [lib.egx_weight_cache_bytes(C.byref(cfg), segs_of(15))]
                for T, batches in UNIFORM:
                    for B in batches:
                        for name in ("egx_encoder_workspace", "egx_translator_workspace"):
                            rc = getattr(lib, name)(C.byref(cfg), segs_of(T), B, C.byref(a), C.byref(b))
                            out[f"{tag} T{T} B{B} {name[4:]}"] = answer(rc, a, b)
                s16 = segs_of(16)
                infer = Config(128, 4, dff, L, 3, 1e-5, compute, 0, 0.0, 0.0, 0.0)     # (ragged inference refuses dropout)
                out[f"{tag} ragged"] = answer(lib.egx_ragged_workspace(C.byref(infer), s16, len(LENS), lens, C.byref(a)), a)
                out[f"{tag} ragged_train"] = answer(lib.egx_ragged_train_workspace(C.byref(cfg), s16, len(LENS), lens, C.byref(a), C.byref(b)), a, b)
                out[f"{tag} ragged_cap"] = answer(lib.egx_ragged_cap_workspace(C.byref(cfg), s16, CAPACITY[0], CAPACITY[1], C.byref(a), C.byref(b)), a, b)
    return out


if __name__ == "__main__":
    from tests import host_paths
    rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sizes(host_paths.bind(sys.argv[1])).items())
    print(f'{{"generated_from": {json.dumps(sys.argv[2])},\n "sizes": {{\n{rows}\n }}}}')
