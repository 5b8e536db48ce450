"""CPU side of the sequence decoder at head dim 256 / 512 (d_model up to 2048): the support predicates against the library's own checks,
every host refusal with its message and zero launches, the three mirror classes against the real ones (where the reference tree is
present), R against E (recorded), the perturbed references against the gate, and the decided share item 4 of the GPU test relies on."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import pytest
import torch

from tests import greedy_ref as gr
from tests import seqdec2048_ref as s

HERE = os.path.dirname(os.path.abspath(__file__))
PTR = 1 << 12       # a non-null, 16-byte aligned marker: every call below is refused before anything is read
COMPUTE = {"bf16": 1, "f32": 0, "f32s": 2}


def _dcfg(d=2048, h=8, L=1, V=12, S=2, compute=1, p_drop=0.0, p_pos=0.0, dff=2048, sy=1):
    from egot2_amd._lib import DecConfig
    return DecConfig(d, h, dff, L, V, sy, S, 1e-5, compute, p_drop, p_pos, None)


def _err(lib):
    return lib.egx_last_error().decode()


# ---- the predicates ---------------------------------------------------------------------------------------------------------------------
def test_abi_stays_18_and_the_hook_pair_resolves(egx_lib):
    from egot2_amd import _lib
    assert _lib.EGX_ABI_VERSION == 18 and egx_lib.egx_abi_version() == 18
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "egot2x.h")).read()
    for name in ("egx_decoder_attention_fwd", "egx_decoder_attention_bwd"):
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES and name + "(" in hdr, name
    assert "ABI v29" in hdr and "egx_dec_attn_args" in hdr


def test_support_predicates_agree_with_the_library_over_a_grid(egx_lib):
    from egot2_amd import functional as F
    lib, nb, sc = egx_lib, C.c_size_t(0), C.c_size_t(0)
    seen = {k: set() for k in ("decode", "generate", "forced", "beam")}
    grid = [(compute, d, h, S) for compute in ("bf16", "f32s") for d, h in ((256, 1), (256, 4), (512, 1), (512, 2), (512, 4), (1024, 2), (1024, 4), (1024, 16),
                                                                              (1152, 18), (1536, 3), (1536, 6), (2048, 4), (2048, 8), (2048, 16), (2048, 32),
                                                                              (2176, 17), (2304, 9), (384, 3), (768, 3))
            for S in (1, 2, 16, 17, 1024, 1025)]
    for compute, d, h, S in grid:
        for sy in (1, 8, 9):
            want = F.decoder_supported(compute, d, h, 2048, sy, S, 2)
            rc = lib.egx_decoder_workspace(C.byref(_dcfg(d, h, 2, 12, S, COMPUTE[compute], sy=sy)), 3, C.byref(nb), C.byref(sc))
            assert want == (rc == 0), ("decode", compute, d, h, S, sy, _err(lib))
            seen["decode"].add(want)
        for V, n in ((12, 4), (1024, 64), (1025, 2), (12, 65)):
            cfg = _dcfg(d, h, 2, V, S, COMPUTE[compute])
            want = F.decoder_generate_supported(compute, d, h, 2048, S, 2, V, n)
            assert want == (lib.egx_decoder_generate_workspace(C.byref(cfg), 3, n, C.byref(nb)) == 0), ("generate", compute, d, h, S, V, n, _err(lib))
            seen["generate"].add(want)
            for R in (1, 8, 9):
                want = F.decoder_forced_supported(compute, d, h, 2048, S, 2, V, n, R)
                assert want == (lib.egx_decoder_forced_workspace(C.byref(cfg), 3, R, n, C.byref(nb)) == 0), ("forced", compute, d, h, S, V, n, R, _err(lib))
                seen["forced"].add(want)
            for W in (1, 3, 4, 5, 8, 9):
                want = F.decoder_beam_supported(compute, d, h, 2048, S, 2, V, n, W)
                assert want == (lib.egx_decoder_beam_workspace(C.byref(cfg), 3, n, W, C.byref(nb)) == 0), ("beam", compute, d, h, S, V, n, W, _err(lib))
                seen["beam"].add(want)
    assert all(v == {True, False} for v in seen.values()), seen
    # the new ground, by name
    assert F.decoder_supported("bf16", 2048, 8, 2048, 1, 2, 6) and F.decoder_supported("bf16", 2048, 4, 2048, 3, 4, 6)
    assert F.decoder_supported("bf16", 256, 1, 2048, 8, 16, 2) and not F.decoder_supported("bf16", 256, 1, 2048, 8, 17, 2)
    assert not F.decoder_supported("bf16", 2048, 32, 2048, 1, 2, 6)                 # head dim 64 keeps d_model <= 1024
    assert not F.decoder_supported("f32s", 2048, 8, 2048, 1, 2, 6)
    assert F.decoder_generate_supported("bf16", 2048, 8, 2048, 2, 6, 1024, 40) and F.decoder_forced_supported("bf16", 2048, 8, 2048, 2, 6, 1024, 64, 8)
    assert F.decoder_beam_supported("bf16", 2048, 8, 2048, 2, 6, 12, 40, 4) and not F.decoder_beam_supported("bf16", 2048, 8, 2048, 2, 6, 12, 40, 5)
    assert F.decoder_ragged_supported("bf16", 256, 4, 2048, 2, 45, 2) and not F.decoder_ragged_supported("bf16", 512, 2, 2048, 2, 4, 2)


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------
def _hook_args(**kw):
    from egot2_amd import _lib
    a = _lib.DecAttnArgs()
    base = dict(q=PTR, k=PTR, v=PTR, ldq=2048, ldk=4096, ldv=4096, operands_bf16=1, o=PTR, ldo=2048, d_o=PTR, dq=PTR, dk=PTR, dv=PTR,
                B=3, H=8, dh=256, Sq=1, Sk=2, causal=0, p_drop=0.0, seed=0, layer=0, site=3, stream=None)
    base.update(kw)
    for k, v in base.items():
        setattr(a, k, v)
    return a


def test_every_refusal_has_its_message_and_launches_nothing(egx_lib):
    lib = egx_lib
    lib.egx_launch_count(1)

    def hook(frags, **kw):
        for fn in (lib.egx_decoder_attention_fwd, lib.egx_decoder_attention_bwd):
            assert fn(C.byref(_hook_args(**kw))) != 0
            assert all(f in _err(lib) for f in frags), (frags, _err(lib))

    # 1: the operator hook pair
    hook(("Sk=17", "Sk <= 16", "256 / 512"), Sk=17)
    hook(("Sq=9", "Sq <= 8", "256 / 512"), Sq=9, Sk=9, causal=1, ldk=2048, ldv=2048)
    hook(("causal", "Sq=3", "Sk=2"), Sq=3, causal=1)
    hook(("head dim 128",), dh=128, H=16)
    hook(("null pointer",), q=None)
    hook(("16-byte aligned",), k=PTR + 8)
    hook(("ldk = 2040",), ldk=2040)
    hook(("ldq = 1024", ">= H * head dim = 2048"), ldq=1024)
    hook(("dropout probability",), p_drop=1.5)
    hook(("B = 0",), B=0)
    hook(("needs bf16 operands",), dh=64, H=4, ldq=256, ldk=512, ldv=512, ldo=256, Sk=65, operands_bf16=0)
    assert lib.egx_decoder_attention_fwd(None) != 0 and "null" in _err(lib)
    # 2: the fused decoder's plan
    nb, sc = C.c_size_t(0), C.c_size_t(0)

    def plan(frags, **kw):
        assert lib.egx_decoder_workspace(C.byref(_dcfg(**kw)), 3, C.byref(nb), C.byref(sc)) != 0
        assert all(f in _err(lib) for f in frags), (frags, _err(lib))

    assert lib.egx_decoder_workspace(C.byref(_dcfg(S=16, sy=8)), 3, C.byref(nb), C.byref(sc)) == 0, _err(lib)
    assert lib.egx_decoder_workspace(C.byref(_dcfg(h=4, S=4, sy=3, L=6)), 256, C.byref(nb), C.byref(sc)) == 0, _err(lib)
    plan(("S <= 16", "S=17", "head dim 256"), S=17)
    plan(("S <= 16", "S=1024", "head dim 512"), h=4, S=1024)
    plan(("sy = 9",), sy=9)
    plan(("d_model = 2048", "[256, 1024]", "2048 with head dim 256 / 512"), h=32)
    plan(("d_model = 2176",), d=2176, h=17)
    plan(("head dim 128",), d=1024, h=8)
    plan(("head dim 1024",), d=1024, h=1)
    for compute in (0, 2):
        plan(("bf16",), compute=compute)
    # out of scope for big heads: ragged memories, attention weights
    lens = (C.c_int * 3)(2, 1, 2)
    assert lib.egx_decoder_ragged_workspace(C.byref(_dcfg()), 3, lens, C.byref(nb)) != 0
    assert all(f in _err(lib) for f in ("ragged memories", "32 / 64", "head dim 256")), _err(lib)
    assert lib.egx_decoder_ragged_train_workspace(C.byref(_dcfg(d=512, h=1)), 3, lens, C.byref(nb), C.byref(sc)) != 0
    assert all(f in _err(lib) for f in ("ragged memories", "32 / 64", "head dim 512")), _err(lib)
    assert lib.egx_decoder_cross_weights(C.byref(_dcfg()), 3, None, PTR, PTR, None) != 0
    assert all(f in _err(lib) for f in ("head dim 256", "16, 32, 64 or 128")), _err(lib)
    from egot2_amd._lib import DecLayer
    layers = C.cast(PTR, C.POINTER(DecLayer))
    assert lib.egx_decoder_generate_attn(C.byref(_dcfg()), PTR, PTR, PTR, PTR, 2048, layers, PTR, PTR, 3, 2, PTR, PTR, PTR, None, 0, None, None, PTR) != 0
    assert all(f in _err(lib) for f in ("head dim 256", "16, 32, 64 or 128")), _err(lib)
    # the composed path (compute f32 / f32s) says which compute type serves the head dim
    assert lib.egx_small_attention_fwd(PTR, 256, PTR, 256, PTR, 256, PTR, 256, 3, 1, 2, 1, 256, 0, 0.0, 0, 0, None) != 0
    assert all(f in _err(lib) for f in ("head dim 256", "1..128", "bf16")), _err(lib)
    # 3: the cached step keeps its other limits, and the beam head its LDS check
    assert lib.egx_decoder_generate_workspace(C.byref(_dcfg(V=1024)), 3, 64, C.byref(nb)) == 0, _err(lib)
    assert lib.egx_decoder_generate_workspace(C.byref(_dcfg(V=1025)), 3, 2, C.byref(nb)) != 0 and "vocab = 1025" in _err(lib)
    assert lib.egx_decoder_generate_workspace(C.byref(_dcfg()), 3, 65, C.byref(nb)) != 0 and "n_steps = 65" in _err(lib)
    assert lib.egx_decoder_generate_workspace(C.byref(_dcfg(S=17)), 3, 2, C.byref(nb)) != 0 and "S <= 16" in _err(lib)
    assert lib.egx_decoder_forced_workspace(C.byref(_dcfg()), 3, 9, 2, C.byref(nb)) != 0 and "R = 9" in _err(lib)
    assert lib.egx_decoder_beam_workspace(C.byref(_dcfg()), 3, 4, 4, C.byref(nb)) == 0, _err(lib)
    assert lib.egx_decoder_beam_workspace(C.byref(_dcfg()), 3, 4, 5, C.byref(nb)) != 0 and "bytes of LDS" in _err(lib)
    assert lib.egx_launch_count(0) == 0                                 # nothing was launched


def test_greedy_and_forced_head_lds_is_checked_by_the_library(egx_lib):
    """The greedy and the forced head hold 4 (d + V) floats of dynamic LDS and their launches set no larger limit than the default 64 KiB:
    generate_plan / forced_plan check it (gen_head_fits). The widest configuration the other checks let through, d = 2048 with V = 1024,
    needs 49152 bytes and passes both."""
    nb = C.c_size_t(0)
    cfg = _dcfg(d=2048, h=8, L=6, V=1024, S=16)
    assert egx_lib.egx_decoder_generate_workspace(C.byref(cfg), 256, 64, C.byref(nb)) == 0, _err(egx_lib)
    assert egx_lib.egx_decoder_forced_workspace(C.byref(cfg), 4, 8, 64, C.byref(nb)) == 0, _err(egx_lib)
    src = open(os.path.join(os.path.dirname(HERE), "egot2_amd", "csrc", "wide_decoder.hip")).read()
    assert src.count("gen_head_fits(") == 3 and src.count("gen_head_lds(d, pl.V), st, hp)") == 2      # one definition, two callers; both launches sized by it


def test_python_refusals_name_the_limits(egx_lib):
    m = s.new_model("fcst", 256, 1, 1)
    y, mem = torch.zeros(3, 2, dtype=torch.int64), torch.zeros(4, 3, 256)
    with torch.no_grad():
        with pytest.raises(ValueError, match=r"head dims \(16, 32, 64, 128\).*head dim 256"):
            m.eval().decode(y, mem, return_attention=True)
    m.egx_long_targets = True
    with pytest.raises(ValueError, match="head dim <= 128"):
        m.train().decode(torch.zeros(3, 9, dtype=torch.int64), mem)


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
def test_mirrors_are_registered_and_shaped_like_the_reference():
    from egot2_amd import hoi_lta, hoi_lta_seq
    names = ("ForecastingEncoderSeqDecoder", "ForecastingEncoderSeparateSeqDecoder", "TaskFusionMFTransformer2TaskSeqDecoder")
    for name in names:
        assert hoi_lta.MODEL_REGISTRY.get(name) is getattr(hoi_lta_seq, name)
    m = s.new_model("fcst", 256, 1, 2)
    keys = set(m.state_dict())
    assert {"ln.weight", "pos_embed.pe", "embedding.weight", "fc.bias", "transformer_encoder.layers.1.linear1.weight",
            "transformer_decoder.layers.1.multihead_attn.in_proj_weight"} <= keys and "pe" not in keys
    assert m.y_mask.shape == (200, 200) and m.n_heads == 1 and m.n_layers == 2 and m.dim == 256 and m.egx_generate is False
    m2 = s.new_model("lta2", 256, 1, 1)
    assert m2.state_dict()["pe"].shape == (1, 4, 256) and m2.y_mask.shape == (3, 3) and m2.sequence_len == 4 and m2.feature_dim == 256
    assert set(m2.state_dict()) - keys == {"pe"}


_REAL_CLASSES = r"""
import importlib, sys
from types import SimpleNamespace as NS
from oracle import ref_harness as rh
from tests import seqdec2048_ref as s
rh.use_tree("HOI")
rh._install_hoi_stubs()
seq = importlib.import_module("models.lta.lta_models_seqdecoder")
tra = importlib.import_module("models.lta.lta_models_lta_transfer")
for mod in (seq, tra):
    mod.vocab_idx_to_orig = lambda: s.idx_maps(12)
    mod.SlowFast = lambda cfg, with_head=True: rh._FeatPass()
    mod.MViT = lambda cfg, with_head=True: rh._FeatPass()
tra.ForecastingEncoderDecoder = lambda cfg, build_decoder=True: rh._FeatPass()
for name in ("load_ckpt", "load_lta_backbone", "freeze_params", "freeze_backbone_params"):
    setattr(tra, name, lambda *a, **k: None)
from egot2_amd import hoi_lta_seq
cfg = s.fcst_cfg(256, 1, 2)
cfg.RESNET = NS(WIDTH_PER_GROUP=64)
cfg.MODEL.ARCH, cfg.MODEL.NUM_CLASSES, cfg.MODEL.HEAD_ACT, cfg.MODEL.FREEZE_BACKBONE = "slowfast", [5], "softmax", False
seq._POOL1 = {"slowfast": [[1, 1, 1], [1, 1, 1]]}
pairs = []
for name in ("ForecastingEncoderSeqDecoder", "ForecastingEncoderSeparateSeqDecoder"):
    assert seq.MODEL_REGISTRY.get(name) is getattr(seq, name)                   # the registry names
    pairs.append((getattr(seq, name)(cfg, s.vocab_of(12)), getattr(hoi_lta_seq, name)(s.fcst_cfg(256, 1, 2), s.vocab_of(12), *s.idx_maps(12))))
cfg2 = s.lta2_cfg(256, 1, 1)
cfg2.MODEL.NUM_CLASSES, cfg2.MODEL.HEAD_ACT = [5], "softmax"
cfg2.CHECKPOINT_FILE_PATH_AR = cfg2.CHECKPOINT_FILE_PATH_LTA = None
assert tra.MODEL_REGISTRY.get("TaskFusionMFTransformer2TaskSeqDecoder") is tra.TaskFusionMFTransformer2TaskSeqDecoder
pairs.append((tra.TaskFusionMFTransformer2TaskSeqDecoder(cfg2, s.vocab_of(12)),
              hoi_lta_seq.TaskFusionMFTransformer2TaskSeqDecoder(s.lta2_cfg(256, 1, 1), s.vocab_of(12), *s.idx_maps(12))))
for real, mine in pairs:
    a, b = real.state_dict(), mine.state_dict()
    assert set(a) == set(b) and all(a[k].shape == b[k].shape for k in a), sorted(set(a) ^ set(b))
    assert real.y_mask.shape == mine.y_mask.shape
print("MIRRORS-MATCH", len(pairs))
"""


def test_mirror_state_dict_keys_match_the_real_classes():
    """state_dict keys and shapes, registry names and y_mask of the three mirrors against the REAL classes, backbones patched out. In a
    process of its own: the reference tree's `utils` / `models` packages must not stay importable for the tests that follow."""
    import subprocess
    import sys
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference tree is not present")
    pytest.importorskip("einops")
    r = subprocess.run([sys.executable, "-c", _REAL_CLASSES], cwd=os.path.dirname(HERE), capture_output=True, text=True)
    assert r.returncode == 0 and "MIRRORS-MATCH 3" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the references ---------------------------------------------------------------------------------------------------------------------
def test_rounded_reference_against_exact_reference_is_recorded():
    """R against E on the stock seeded weights (embedding / 16, p = 0, B = 3): recorded, not asserted beyond being of the size that makes R
    the device's reference (within 2 x a bar, and not negligible)."""
    lines = []
    for d, h, L, sy, S in s.RE_CASES:              # all five rows of the issue's table
        data = s.case_data("fcst", d, h, L, sy, S, 3, stock=True)
        g = s.gate(s.oracle_run(data, True), s.oracle_run(data, False), s.BF16_BAR)
        lines.append(s.gate_line(f"R vs E, stock weights, d = {d}, heads = {h}, L = {L}, sy = {sy}, S = {S}, B = 3", g))
        print("SEQDEC2048", lines[-1])
        assert 0.1 < g["miss"] < 2.0, lines[-1]
    s.record("cpu: R against E on the stock seeded weights (recorded, not a bar)", lines)


def test_kink_free_weights_keep_rounding_inside_the_bars_and_perturbed_references_miss_them():
    """On the GPU tests' own weights (kink-free linear1.bias) R stays within half of every bar of E, and each perturbed reference of
    tests/seqdec2048_ref.py PERTURBATIONS misses a bar against R by at least PERTURBED_MIN: scale64 (the attention scale of head dim 64),
    no_causal (no causal mask), swap (cross-attention block before the self-attention block). Inputs: the first decode case
    (d = 256, 1 head of 256, 2 layers, sy = 3, S = 4, B = 3) and the second (d = 512, 1 head of 512, sy = 8, S = 16)."""
    lines = []
    for case in s.DECODE_CASES[:2]:
        data = s.case_data(*case)
        R = s.oracle_run(data, True)
        g = s.gate(R, s.oracle_run(data, False), s.BF16_BAR)
        assert g["miss"] < 0.5, s.gate_line("R vs E, kink-free weights", g)
        assert all(v[0] > 1e-3 for v in data["margins"].values()), data["margins"]
        for p in s.PERTURBATIONS:
            miss = s.gate(s.oracle_run(data, True, perturb=p), R, s.BF16_BAR)["miss"]
            lines.append(f"{case[0]} d = {case[1]}, heads = {case[2]}: {p} misses the worst bar by {miss:.1f} x")
            assert miss >= s.PERTURBED_MIN, lines[-1]
    s.record("cpu: perturbed references against R (each must miss a bar by >= 3 x)", lines)


def test_the_decided_share_item_four_relies_on():
    """Case d512_h2_v12 (weight seed 98, feature seed 96): at least half of the clips have every top-2 margin of the fp64 greedy loop above
    twice the bf16 bound, with at least two distinct tokens among them; the 40-step case is far below that and item 2 is its check."""
    name = "d512_h2_v12"
    d, h, L, V, S, B, n = s.GEN_CASES[name][:7]
    _, sd64, start, mem64, _ = s.build_gen_case(name)
    rt, rl, rm = gr.greedy(sd64, h, torch.full((B,), start, dtype=torch.int64), mem64, n)
    dec = gr.decided(rm, 4e-2 * max(1.0, rl.abs().max().item()))
    share, distinct = dec.float().mean().item(), sorted(set(rt[dec].flatten().tolist()))
    print(f"SEQDEC2048 item 4 [{name}]: decided share {share:.2f}, tokens among them {distinct}")
    s.record("cpu: item 4's decided share", [f"{name}: {share:.2f} of {B} clips decided over all {n} steps, tokens among them {distinct}"])
    assert share >= 0.5 and len(distinct) >= 2, (share, distinct)


@pytest.mark.parametrize("name", list(s.RECORDINGS))
def test_recorded_real_classes_reproduce_the_helpers_oracle(name):
    """tests/golden/live/seqdec_*.npz (tests/golden/make_golden_seqdec.py: forward, predict and the 40-step predict loop of the REAL classes in
    fp64 on seeded weights) against tests/seqdec2048_ref.py oracle_recording, the fp64 oracle every GPU test of the mirrors is held to:
    below 1e-9, tokens equal. Needs no reference tree: weights, features and targets are re-derived from the recorded seeds."""
    import json
    import numpy as np
    path = os.path.join(HERE, "golden", "live", name + ".npz")
    assert os.path.getsize(path) < 64 * 1024
    z = np.load(path)
    c = json.loads(str(z["config"]))
    assert c == s.RECORDINGS[name]
    want = s.oracle_recording(c, *s.recording_inputs(c))
    assert set(want) == set(z.files) - {"config"}
    for k, v in want.items():
        got = torch.from_numpy(z[k])
        assert got.shape == v.shape and got.dtype == v.dtype == (torch.int64 if k == "step_tokens" else torch.float64), k
        assert torch.equal(got, v) if k == "step_tokens" else (got - v).abs().max().item() < 1e-9, k
    if c["steps"]:
        assert z["step_logits"].shape == (40, c["B"], c["V"]) and len(set(z["step_tokens"].flatten().tolist())) >= 2
