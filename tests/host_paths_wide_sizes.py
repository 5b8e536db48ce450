"""Every workspace size the wide bf16 paths answer, at the smallest shapes of every branch of their three plans: the wide encoder (wide_host.hip
make_wplan: uniform, ragged inference, ragged training), the fused decoder (wide_decoder.hip make_dplan: uniform, ragged memories) and the cached
step (step_layout: greedy, beam, forced). Host-only, no torch.

  * imported by tests/test_cpu_host.py, which compares sizes(lib) of the product library with tests/wide_workspace_sizes.json;
  * as a script it writes that table: `python tests/host_paths_wide_sizes.py <lib.so> <commit>` prints the JSON of a library built from <commit>.
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
ENC_HEADS = {256: 4, 768: 8, 2048: 8}                          # head dim 64, 96 and 256 (the last: S <= 16)
FEATS = {"f32": (0, 0), "bf16": (1, 1), "bf16_pool2": (1, 2)}  # (feat_bf16, pool) of the projected segment: cast copy, used in place, pooled copy
SLAB_CUT = 400 << 20                                           # make_wplan: above it no weight gradient gets a slab region of its own
GEN_GRID = dict(models=[(256, 4, 2, 7), (512, 8, 3, 600), (1024, 16, 16, 1024), (384, 12, 1, 1)], B=(1, 37, 256), S=(1, 48, 1024),
                steps=(1, 2, 40, 64), k=(1, 3, 8))             # tools/lib_compare.py --host: the three generation queries


def encoder_slab_all(lib, d, dff, L, din, rows_proj, N):
    """make_wplan's sum over the weight gradients of a backward (one projected segment of rows_proj rows): compared with SLAB_CUT"""
    tn = lambda M, Nn, K: (lib.egx_wide_gemm_scratch(2, M, Nn, K) - 1024 + 255) // 256 * 256       # noqa: E731
    return L * (tn(d, dff, N) + tn(dff, d, N) + tn(d, d, N) + tn(3 * d, d, N)) + tn(d, din, rows_proj)


def sizes(lib) -> dict:
    from egot2_amd._lib import Config, DecConfig, Segment
    out = {}
    a, b = C.c_size_t(), C.c_size_t()

    def answer(rc, *vals):
        return [rc] + ([v.value for v in vals] if rc == 0 else [])

    # the wide encoder: a projected segment (d_in 256) and, with ident, an identity segment (d_in = d_model) behind it, T frames each
    def enc_segs(d, T, ident, feat):
        s = (Segment * (2 if ident else 1))()
        s[0].T, s[0].d_in, s[0].proj_w = T, 256, 1              # (a non-null marker: nothing is read)
        s[0].feat_bf16, s[0].pool = FEATS[feat]
        if ident:
            s[1].T, s[1].d_in, s[1].proj_w = T, d, 0
        return s

    crossed = set()
    for d, H in ENC_HEADS.items():
        for L in (1, 2):
            for dff in (128, 2048):
                for ident in (0, 1):
                    for feat in FEATS:
                        for B, T in ((1, 5), (3, 5), (256, 5)) + (((256, 64),) if H * 128 >= d and not ident else ()):
                            cfg = Config(d, H, dff, L, 1 + ident, 1e-5, 1, 0, 0.1, 0.1, 0.1)
                            rc = lib.egx_encoder_workspace(C.byref(cfg), enc_segs(d, T, ident, feat), B, C.byref(a), C.byref(b))
                            out[f"enc d{d} L{L} dff{dff} ident{ident} {feat} B{B} T{T}"] = answer(rc, a, b)
                            if rc == 0:
                                crossed.add(encoder_slab_all(lib, d, dff, L, 256, B * T, B * T * (1 + ident)) > SLAB_CUT)
    out["enc slab_all on both sides of its cut-off"] = [int(crossed == {False, True})]

    # ragged batches of the wide encoder on LENS (three projected segments, padded to 16 frames)
    lens = (C.c_int * 12)(*[t for clip in LENS for t in clip])
    equal = (C.c_int * 12)(*[clip[0] for clip in LENS for _ in clip])       # out_layout 1 needs equal segment lengths in a clip
    s16 = (Segment * 3)()
    for x in s16:
        x.T, x.d_in, x.proj_w = 16, 256, 1
    for d, H in ((256, 4), (768, 8)):
        for L in (1, 2):
            for dff in (128, 2048):
                tag = f"ragged_enc d{d} L{L} dff{dff}"
                infer = Config(d, H, dff, L, 3, 1e-5, 1, 0, 0.0, 0.0, 0.0)      # (ragged inference refuses dropout)
                train = Config(d, H, dff, L, 3, 1e-5, 1, 0, 0.1, 0.1, 0.1)
                for name, arr in (("lens", lens), ("equal", equal)):             # (the queries size the table for out_layout 1 either way)
                    out[f"{tag} {name} infer"] = answer(lib.egx_ragged_encode_workspace(C.byref(infer), s16, 4, arr, C.byref(a)), a)
                    out[f"{tag} {name} train"] = answer(lib.egx_ragged_encode_train_workspace(C.byref(train), s16, 4, arr, C.byref(a), C.byref(b)), a, b)
                # the table itself with out_layout 0 and 1: the calls build it, lay the workspace out and then refuse the null pointers
                for layout in (0, 1):
                    for name, arr in (("lens", lens), ("equal", equal)):
                        rc = lib.egx_ragged_encode_train_fwd(C.byref(train), s16, arr, None, None, None, 4, None, layout, None, 1, 7, None)
                        out[f"{tag} {name} layout{layout} fwd"] = [rc, lib.egx_last_error().decode()]
                        rc = lib.egx_ragged_encode(C.byref(infer), s16, arr, None, None, None, 4, None, layout, None, None)
                        out[f"{tag} {name} layout{layout} encode"] = [rc, lib.egx_last_error().decode()]

    # the fused decoder: uniform, ragged memories (inference and training)
    for d in (256, 1024):
        for dh in (32, 64):
            for L in (1, 3):
                for sy in (1, 8):
                    for S in (1, 19):
                        dc = DecConfig(d, d // dh, 2048, L, 7, sy, S, 1e-5, 1, 0.1, 0.1, None)
                        di = DecConfig(d, d // dh, 2048, L, 7, sy, S, 1e-5, 1, 0.0, 0.0, None)
                        tag = f"dec d{d} dh{dh} L{L} sy{sy} S{S}"
                        mem = (C.c_int * 4)(*[1 + (7 * i) % S for i in range(4)])
                        for B in (1, 3, 256):
                            out[f"{tag} B{B}"] = answer(lib.egx_decoder_workspace(C.byref(dc), B, C.byref(a), C.byref(b)), a, b)
                        out[f"{tag} ragged"] = answer(lib.egx_decoder_ragged_workspace(C.byref(di), 4, mem, C.byref(a)), a)
                        out[f"{tag} ragged_train"] = answer(lib.egx_decoder_ragged_train_workspace(C.byref(dc), 4, mem, C.byref(a), C.byref(b)), a, b)

    # the cached step: greedy, beam (W = k), forced (R = k)
    for d, h, L, V in GEN_GRID["models"]:
        for B in GEN_GRID["B"]:
            for S in GEN_GRID["S"]:
                for n in GEN_GRID["steps"]:
                    cfg = DecConfig(d, h, 2048, L, V, 99, S, 1e-5, 1, 0.0, 0.0, None)       # sy = 99: not read
                    tag = f"step d{d} L{L} V{V} B{B} S{S} n{n}"
                    out[f"{tag} generate"] = answer(lib.egx_decoder_generate_workspace(C.byref(cfg), B, n, C.byref(a)), a)
                    for k in GEN_GRID["k"]:
                        out[f"{tag} beam W{k}"] = answer(lib.egx_decoder_beam_workspace(C.byref(cfg), B, n, k, C.byref(a)), a)
                        out[f"{tag} forced R{k}"] = answer(lib.egx_decoder_forced_workspace(C.byref(cfg), B, k, n, C.byref(a)), a)
    return out


if __name__ == "__main__":
    from tests import host_paths
    rows = ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in sizes(host_paths.bind(sys.argv[1])).items())
    print(f'{{"generated_from": {json.dumps(sys.argv[2])},\n "sizes": {{\n{rows}\n }}}}')
