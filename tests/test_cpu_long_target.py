"""decode() over 9 .. 64 target tokens on the host, without a GPU: the gate of tests/test_gpu_long_target.py tested on itself (the fp32
evaluation of each reference meets its bar, a perturbed reference misses it at least 3x, the mask helper is dropmask's at stride 8), the
host refusals of egx_target_attention_fwd / _bwd through ctypes, and the predicate of the route."""
import ctypes as C
import math

import pytest
import torch

from egot2_amd.functional import decoder_long_supported       # (the feature under test: without it nothing below can run)
from tests import decoder_dropout_gate as ddg
from tests import dropmask as dm
from tests import long_target_ref as lt
from tests import unit_ref as ur

F64, F32 = torch.float64, torch.float32
_IDS = [lt.lt_case_id(c) for c in lt.LT_ATTN_CASES]
_REF = {}


def _ref(ci):
    if ci not in _REF:
        _REF[ci] = lt.lt_eval(ci, F64)
    return _REF[ci]


def _errs(ci, dtype, perturb=None):
    o, grads = lt.lt_eval(ci, dtype, perturb)
    ro, rgrads = _ref(ci)
    return ur.rel_err(o, ro), max(ur.rel_err(g, r) for g, r in zip(grads, rgrads))


# ---- 1: the fp32 yardstick and the operator bars ----------------------------------------------------------------------------------------
def test_fp32_reference_meets_the_operator_bar():
    meas = {"out": 0.0, "grad": 0.0}
    for ci in range(len(lt.LT_ATTN_CASES)):
        eo, eg = _errs(ci, F32)
        print(f"fp32 yardstick {_IDS[ci]:40s} out {eo:.3e} grad {eg:.3e}")
        meas["out"], meas["grad"] = max(meas["out"], eo), max(meas["grad"], eg)
    for kind, e in meas.items():
        rec, bar = lt.LT_FP32_ERR[kind], lt.LT_BAR[kind]
        print(f"fp32 yardstick target_attention {kind:4s} measured {e:.3e} recorded {rec:.3e} bar {bar:.3e}")
        assert bar == ur.FACTOR * rec
        assert e <= bar, f"{kind}: the fp32 reference misses its own bar ({e} > {bar})"
        assert rec / 3 <= e <= rec * 3, f"{kind}: recorded fp32 error {rec} is not the measured {e}"


# ---- 2: perturbed references -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lt.LT_PERTURB_APPLIES))
def test_perturbed_reference_misses_the_bar(name):
    """In fp32, outputs and gradients each, on every case the mistake applies to."""
    worst, n = math.inf, 0
    for ci, case in enumerate(lt.LT_ATTN_CASES):
        if not lt.LT_PERTURB_APPLIES[name](case):
            continue
        eo, eg = _errs(ci, F32, name)
        worst, n = min(worst, eo / lt.LT_BAR["out"], eg / lt.LT_BAR["grad"]), n + 1
    rec = lt.LT_PERTURB_RATIO[name]
    print(f"perturbation target_attention {name:20s} over {n} cases: worst error / bar = {worst:.3g} (recorded {rec:.3g})")
    assert n >= 2
    assert worst >= lt.PERTURBED_MIN, f"{name}: the bar lets the perturbed reference through (error / bar = {worst})"
    assert worst >= rec / 2, f"{name}: recorded ratio {rec} is not the measured {worst}"


# ---- 3: the mask helper ------------------------------------------------------------------------------------------------------------------
def _masks_equal(a, b):
    if not torch.equal(a["embed"], b["embed"]) or len(a["layers"]) != len(b["layers"]):
        return False
    return all(set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a["layers"], b["layers"]))


def test_long_decoder_masks_are_dropmasks_at_stride_8():
    seed, B, S, d, H, d_ff, L, p, pp = 0xC0FFEE, 3, 11, 64, 4, 96, 2, 0.3, 0.1
    assert _masks_equal(lt.long_decoder_masks(seed, B, 5, S, d, H, d_ff, L, p, pp, row_stride=8),
                        dm.decoder_masks(seed, "composed", B, 5, S, d, H, d_ff, L, p, pp))
    m8 = lt.long_decoder_masks(seed, B, 9, S, d, H, d_ff, L, p, pp, row_stride=8)
    m64 = lt.long_decoder_masks(seed, B, 9, S, d, H, d_ff, L, p, pp)
    for l in range(L):
        assert m64["layers"][l]["self"].shape == (B, H, 9, 9) and m64["layers"][l]["cross"].shape == (B, H, 9, S)
        assert not torch.equal(m8["layers"][l]["self"], m64["layers"][l]["self"])
        assert not torch.equal(m8["layers"][l]["cross"], m64["layers"][l]["cross"])
        assert torch.equal(m8["layers"][l]["self"][0, 0], m64["layers"][l]["self"][0, 0])       # block 0: rows i at either stride
        for k in ("sa_out", "ca_out", "ffn", "ffn_out"):
            assert torch.equal(m8["layers"][l][k], m64["layers"][l][k])
    # stride 8 collides from query 8 on: row 8 of (b, h) is row 0 of the next (b, h)
    assert torch.equal(m8["layers"][0]["cross"][0, 0, 8], m8["layers"][0]["cross"][0, 1, 0])
    assert not torch.equal(m64["layers"][0]["cross"][0, 0, 8], m64["layers"][0]["cross"][0, 1, 0])


# ---- 4: the decoder gate -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lt.LT_DECODER_CASES, ids=[c.id for c in lt.LT_DECODER_CASES])
def test_fp32_oracle_meets_the_decoder_bars(case):
    data, ref = lt.case_data(case), lt.reference(case)
    g = ddg.gate(ddg.oracle_run(case, data, dtype=F32), ref, case.bars)
    print(f"LONGTARGET cpu {case.id}: fp32 oracle logits {g['logits']:.3e} dmem {g['dmem']:.3e} grad {g['grad']:.3e} ({g['worst_grad']}) "
          f"margins {data['margins']}")
    assert g["ok"], g["ratio"]
    if case.p_drop > 0:
        wrong = ddg.gate(ddg.oracle_run(case, data, masks=lt.case_masks(case, case.host_seed, row_stride=8)), ref, case.bars)
        print(f"LONGTARGET cpu {case.id}: stride-8 masks miss the logits bar {wrong['ratio']['logits']:.3g}x")
        assert wrong["ratio"]["logits"] >= lt.PERTURBED_MIN


# ---- 5: host refusals ----------------------------------------------------------------------------------------------------------------------
def _err(lib):
    return lib.egx_last_error().decode()


def test_target_attention_refusals_on_the_host(egx_lib):
    lib = egx_lib
    assert hasattr(lib, "egx_target_attention_fwd") and hasattr(lib, "egx_target_attention_bwd")
    buf = (C.c_float * 16)()                # never dereferenced: every call below is refused before any device work
    a = C.addressof(buf)
    H = 2

    def both(expect, Sq=9, Sk=9, dh=32, causal=0, q=a, ldq=None):
        d = H * dh
        ldq = d if ldq is None else ldq
        lib.egx_launch_count(1)
        for rc in (lib.egx_target_attention_fwd(q, ldq, a, d, a, d, a, d, 1, Sq, Sk, H, dh, causal, 0.0, 1, 0x4003, None),
                   lib.egx_target_attention_bwd(q, ldq, a, d, a, d, a, d, a, a, a, 1, Sq, Sk, H, dh, causal, 0.0, 1, 0x4003, None)):
            assert rc != 0
            assert all(w in _err(lib) for w in expect), (_err(lib), expect)
        assert lib.egx_launch_count(0) == 0

    both(("Sq=65", "1..64"), Sq=65, Sk=65)
    both(("Sk=1025", "1..1024"), Sk=1025)
    both(("head dim 129", "1..128"), dh=129)
    both(("causal", "Sq == Sk"), Sq=9, Sk=10, causal=1)
    both(("null pointer",), q=None)
    both(("row strides", "H * dh = 64"), ldq=63)
    both(("Sq=0", "1..64"), Sq=0)
    # the small entry point keeps its limit
    rc = lib.egx_small_attention_fwd(a, 64, a, 64, a, 64, a, 64, 1, 9, 9, H, 32, 0, 0.0, 1, 0x4003, None)
    assert rc != 0 and "Sq=9 outside 1..8" in _err(lib)


# ---- 6: the predicate ----------------------------------------------------------------------------------------------------------------------
def test_decoder_long_supported_truth_table():
    ok = decoder_long_supported
    assert ok(512, 8, 21, 4) and ok(512, 8, 9, 1) and ok(512, 8, 64, 1024) and ok(256, 2, 12, 48) and ok(8, 8, 9, 1)
    assert not ok(512, 8, 8, 4) and not ok(512, 8, 65, 4)              # sy
    assert not ok(512, 8, 21, 0) and not ok(512, 8, 21, 1025)          # S
    assert not ok(512, 7, 21, 4)                                      # d % heads
    assert ok(256, 2, 21, 4) and not ok(258, 2, 21, 4) and not ok(512, 2, 21, 4)    # head dim 128 | 129 | 256
    assert not ok(512, 0, 21, 4)


def test_the_switch_is_off_by_default():
    from egot2_amd.decoder import DecoderMixin
    from egot2_amd import hhi_multitask, hoi_multitask
    assert DecoderMixin.egx_long_targets is False
    for cls in (hoi_multitask.TaskTranslationPromptTransformerActionTask, hoi_multitask.TaskTranslationPromptTransformer,
                hhi_multitask.TaskTranslationPromptTransformer):
        assert issubclass(cls, DecoderMixin) and cls.egx_long_targets is False
