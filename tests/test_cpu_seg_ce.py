"""CPU suite of the LTA criterion (egx_segmented_ce, functional.segmented_cross_entropy, train.LTACriterion): the gate tests/seg_ce_ref.py
against the recording of the reference's own loop, its bars, its perturbed references, the host refusals of the C entry point and the
arithmetic of LTACriterion.step_result."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import seg_ce_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "lta_criterion.npz")
KINDS = ("loss", "loss_terms", "d_logits")


def _eval(i, dtype, perturb=None):
    B, Z, classes, ld, _ = sr.CASES[i]
    logits, labels, ks = sr.seg_inputs(i)
    return sr.segmented_ce(logits.to(dtype), labels, classes, sr.case_col0(sr.CASES[i]), ks, perturb)


@pytest.fixture(scope="module")
def evals():
    """case index -> (fp64 reference, fp32 evaluation), computed once."""
    return {i: (_eval(i, sr.F64), _eval(i, torch.float32)) for i in range(len(sr.CASES))}


@pytest.mark.parametrize("name", ["a", "b"])
def test_gate_reproduces_the_recorded_reference_loop(name):
    """The gate in fp64 against nn.CrossEntropyLoss + the reference's topk_errors as tests/golden/make_golden_ltacrit.py recorded them."""
    z = np.load(GOLDEN)
    logits, labels = torch.from_numpy(z[f"{name}_logits"]), torch.from_numpy(z[f"{name}_labels"])
    classes = [int(c) for c in z[f"{name}_classes"]]
    col0 = [0] + list(np.cumsum(classes)[:-1])
    res = sr.segmented_ce(logits.double(), labels, classes, col0, (1, 5))
    assert abs(res["loss"].item() - float(z[f"{name}_loss"])) <= 1e-12 * abs(float(z[f"{name}_loss"]))
    assert (res["n_valid"] == logits.shape[0]).all()
    errs = sr.topk_errors_of(res).numpy()
    assert np.abs(errs[0] - z[f"{name}_top1_err"]).max() < 1e-4         # the recording went through fp32 (.item() of a float tensor)
    assert np.abs(errs[1] - z[f"{name}_top5_err"]).max() < 1e-4
    assert abs(res["loss_terms"].sum().item() - res["loss"].item()) < 1e-9


def test_inputs_carry_the_planted_cases():
    logits, labels, ks = sr.seg_inputs(4)                               # (257, 2, (115, 478), 593)
    assert logits.dtype == torch.float32 and labels.dtype == torch.int64 and ks == (1, 5)
    assert logits[0, 0, 0] == 80 and logits[0, 0, 114] == -80 and (logits[1, 0, :115] == 0.75).all()
    assert (labels == -100).any() and (labels[..., 1] == 478).any() and (labels[..., 0] == 0).any() and (labels[..., 1] == 477).any()
    ref = _eval(4, sr.F64)
    assert ref["n_valid"][1, 0] == 0 and ref["loss_terms"][1, 0] == 0 and (ref["d_logits"][:, 1, :115] == 0).all()
    assert torch.isfinite(ref["d_logits"]).all() and math.isfinite(ref["loss"].item())
    assert sr.seg_inputs(0)[2] == (1,) and sr.seg_inputs(2)[2] == (1, 5)
    gaps = _eval(8, sr.F64)                                             # columns no head covers: zero gradient
    assert (gaps["d_logits"][..., 0] == 0).all() and (gaps["d_logits"][..., 6:9] == 0).all() and (gaps["d_logits"][..., 16:] == 0).all()


def test_fp32_reference_meets_the_bar(evals):
    """The fp32 evaluation of the gate passes its own bars, matches every count, and the recorded FP32_ERR constants are what it measures."""
    worst = {k: 0.0 for k in KINDS}
    for i, (ref, f32) in evals.items():
        assert torch.equal(ref["n_valid"], f32["n_valid"]) and torch.equal(ref["correct"], f32["correct"]), sr.case_id(sr.CASES[i])
        for k in KINDS:
            e = sr.rel_err(f32[k], ref[k])
            worst[k] = max(worst[k], e)
            assert e <= sr.BAR[k], (sr.case_id(sr.CASES[i]), k, e)
    print("FP32_ERR measured:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k in KINDS:
        assert sr.FP32_ERR[k] / 3 <= worst[k] <= sr.FP32_ERR[k] * 3, (k, worst[k], sr.FP32_ERR[k])


@pytest.mark.parametrize("perturb", sr.PERTURBATIONS)
def test_perturbed_reference_is_rejected(evals, perturb):
    """Every deliberate mistake misses a bar by >= 3x, or changes a count, on every case where it changes anything; and it changes something."""
    ratios, count_hits = [], 0
    for i, (ref, _) in evals.items():
        bad = _eval(i, sr.F64, perturb)
        counts = not (torch.equal(ref["n_valid"], bad["n_valid"]) and torch.equal(ref["correct"], bad["correct"]))
        ratio = max(sr.rel_err(bad[k], ref[k]) / sr.BAR[k] for k in KINDS)
        if counts:
            count_hits += 1
        elif ratio > 0:
            ratios.append(ratio)
    print(perturb, "min ratio", min(ratios) if ratios else None, "cases with changed counts", count_hits)
    assert ratios or count_hits
    assert all(r >= 3 for r in ratios), (perturb, min(ratios))
    want = sr.PERTURB_RATIO[perturb]
    if want == "counts":
        assert count_hits > 0 and not ratios
    else:
        assert ratios and want / 3 <= min(ratios) <= want * 3, (perturb, min(ratios), want)


# ---- host refusals of egx_segmented_ce -----------------------------------------------------------------------------------------------------
def _call(lib, logits=0x1000, ld=12, target=0x1000, B=5, Z=3, col0=(0, 5), classes=(5, 7), ks=(1, 5), loss=0x1000, n_valid=0x1000,
          correct=0x1000, scratch=0x1000, H=None, n_ks=None):
    ia = lambda v: (C.c_int * max(len(v), 1))(*v)  # noqa: E731
    return lib.egx_segmented_ce(logits, ld, target, B, Z, len(classes) if H is None else H, ia(col0), ia(classes), ia(ks),
                                len(ks) if n_ks is None else n_ks, loss, None, n_valid, correct, None, scratch, None)


REFUSALS = [
    (dict(logits=None), "null pointer"),
    (dict(target=None), "null pointer"),
    (dict(loss=None), "null pointer"),
    (dict(n_valid=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(correct=None), "null pointer"),
    (dict(H=0), "1 <= H <= 4"),
    (dict(H=5, col0=(0, 1, 2, 3, 4), classes=(1, 1, 1, 1, 1)), "1 <= H <= 4"),
    (dict(classes=(0, 7)), "1 <= C <= 2048"),
    (dict(classes=(2049,), col0=(0,), ld=4096), "1 <= C <= 2048"),
    (dict(ks=(0,)), "1 <= k <= 5"),
    (dict(ks=(1, 6)), "1 <= k <= 5"),
    (dict(ks=(1, 1, 1, 1, 1)), "n_ks <= 4"),
    (dict(ld=0), "ld >= 1"),
    (dict(ld=11), "of a row of ld=11"),
    (dict(col0=(-1, 5)), "of a row of ld=12"),
    (dict(col0=(0, 4)), "overlap"),
    (dict(col0=(3, 0)), "overlap"),
    (dict(B=0), "B=0"),
    (dict(Z=0), "Z=0"),
    (dict(B=65536, Z=65536), "B * Z"),
    (dict(B=2 ** 31 - 1, Z=2), "B * Z"),
]


@pytest.mark.parametrize("kwargs,message", REFUSALS, ids=[f"{i}_{m.replace(' ', '_')}" for i, (_, m) in enumerate(REFUSALS)])
def test_host_refusals_before_any_device_work(egx_lib, kwargs, message):
    egx_lib.egx_launch_count(1)
    assert _call(egx_lib, **kwargs) != 0
    assert message.encode() in egx_lib.egx_last_error(), egx_lib.egx_last_error()
    assert egx_lib.egx_launch_count(0) == 0


def test_scratch_query(egx_lib):
    assert egx_lib.egx_segmented_ce_scratch(256, 20, 2, 2) >= 64 * 21 + 20 * 64 * 2 * 4 * 3
    assert egx_lib.egx_segmented_ce_scratch(1, 1, 1, 0) >= 64 * 2 + 4
    assert egx_lib.egx_segmented_ce_scratch(256, 20, 5, 2) == 0 and b"1 <= H <= 4" in egx_lib.egx_last_error()
    assert egx_lib.egx_segmented_ce_scratch(65536, 65536, 2, 2) == 0 and b"B * Z" in egx_lib.egx_last_error()


def test_functional_refuses_cpu_tensors(egx_lib):
    from egot2_amd import _lib, functional as F_egx
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.segmented_cross_entropy([torch.zeros(2, 3, 5), torch.zeros(2, 3, 7)], torch.zeros(2, 3, 2, dtype=torch.int64))


# ---- LTACriterion.step_result ----------------------------------------------------------------------------------------------------------------
def test_step_result_arithmetic_and_key_names():
    """The packed result buffer on CPU stand-in tensors: keys and values of the reference's step_result
    (HOI/tasks/lta/long_term_anticipation.py:194-206)."""
    from egot2_amd.train import LTACriterion
    crit = LTACriterion(ks=(1, 5))
    with pytest.raises(RuntimeError, match="no forward"):
        crit.step_result()
    Z, H = 3, 2
    b = crit._result_buffers(torch.device("cpu"), Z, H)
    assert b["flat"].numel() == 1 + Z * H * 4 and b["correct"].shape == (2, Z, H) and b["n_valid"].dtype == torch.int32
    assert crit._result_buffers(torch.device("cpu"), Z, H) is b                 # persistent per shape
    b["loss"].fill_(7.25)
    b["loss_terms"].fill_(7.25 / 6)
    b["n_valid"].copy_(torch.tensor([[8, 8], [4, 8], [0, 5]], dtype=torch.int32))
    b["correct"][0].copy_(torch.tensor([[2, 8], [1, 0], [0, 5]], dtype=torch.int32))
    b["correct"][1].copy_(torch.tensor([[6, 8], [4, 3], [0, 5]], dtype=torch.int32))
    crit._last = b
    r = crit.step_result()
    assert set(r) == {f"train_{z}_{h}_top{k}_err" for z in range(Z) for h in range(H) for k in (1, 5)} | \
        {f"train_{h}_top{k}_err" for h in range(H) for k in (1, 5)} | {"train_loss"}
    assert r["train_loss"] == 7.25
    assert r["train_0_0_top1_err"] == 75.0 and r["train_0_0_top5_err"] == 25.0 and r["train_1_0_top5_err"] == 0.0
    assert r["train_0_1_top1_err"] == 0.0 and r["train_1_1_top1_err"] == 100.0 and r["train_1_1_top5_err"] == 62.5
    assert math.isnan(r["train_2_0_top1_err"]) and math.isnan(r["train_0_top1_err"])        # a pair without a valid label
    assert r["train_1_top1_err"] == pytest.approx((0.0 + 100.0 + 0.0) / 3) and r["train_1_top5_err"] == pytest.approx(62.5 / 3)
    assert set(crit.step_result(prefix="val")) == {k.replace("train", "val", 1) for k in r}
    with pytest.raises(ValueError):
        LTACriterion(ks=(1, 2, 3, 4, 5))


def test_buffers_are_not_created_inside_a_capture(monkeypatch):
    """A buffer created inside a capture would live in that graph's private pool: refused, with the message the classifier head's scratch uses."""
    from egot2_amd.train import LTACriterion
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="run one eager step at this problem size before capturing it in a graph"):
        LTACriterion()._result_buffers(torch.device("cuda", 0), 3, 2)
