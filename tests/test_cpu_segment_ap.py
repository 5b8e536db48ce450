"""CPU suite of the TTM / LAM validation accumulator (egx_segment_scores_update, egx_segment_ap, functional.segment_ap,
train.SegmentAPValidation): the gate tests/segment_ap_ref.py against the recording of the reference's own PostProcessor and run_evaluation,
its perturbed references on the planted inputs, the host refusals of the C entry points and the host side of SegmentAPValidation."""
import math
import os

import numpy as np
import pytest
import torch

from tests import segment_ap_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "segment_ap.npz")
FIXTURE_CASES = ("ttm_a", "ttm_b", "lam_a")


# ---- the gate against the recorded reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_gate_reproduces_the_recorded_reference_epoch(name):
    """The gate in fp64 against the REAL PostProcessor.update / save / get_mAP -> run_evaluation as tests/golden/make_golden_segap.py
    recorded them: each AP and mAP to 1e-12, acc and the counts exactly, the scores (fp32 in the reference) to the fp32 bar."""
    z = np.load(GOLDEN)
    g = lambda k: z[f"{name}_{k}"]  # noqa: E731
    res = sr.evaluate(g("logits"), g("slots"), g("labels"))
    n = len(g("score"))
    assert res["n"] == n and n <= 300 and np.array_equal(res["label"], g("row_label"))
    worst = float(np.abs(res["score"] - g("score")).max())
    print(name, "rows", n, "score error against the recorded fp32 scores", f"{worst:.2e}")
    assert worst <= sr.SCORE_TOL
    # the APs on the RECORDED scores (what run_evaluation saw): to 1e-12; on the gate's own fp64 scores the order is the same (tie-free)
    rec = sr.run_evaluation(g("score"), g("row_label"))
    for k, want in (("AP0", g("AP")[0]), ("AP1", g("AP")[1]), ("mAP", float(g("mAP")))):
        print(name, k, rec[k], want)
        assert abs(rec[k] - want) <= sr.FIXTURE_AP_TOL
    assert np.array_equal(res["order1"], rec["order1"]) and np.array_equal(res["order0"], rec["order0"])
    assert [rec[k] for k in ("TP", "FN", "FP", "TN")] == g("confusion").tolist() and rec["acc"] == float(g("acc"))
    assert 0 < rec["n_pos"] < n and len(np.unique(g("score"))) == n
    if name.startswith("ttm"):
        assert 1 <= np.bincount(g("slots")).min() and np.bincount(g("slots")).max() == 7


@pytest.mark.reference
def test_fixture_reproduces_from_the_live_post_processor():
    import subprocess
    import sys
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference tree is not available")
    pytest.importorskip("pandas")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_segap.py"), "--check"], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "check True max_diff 0.000e+00" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_fast_average_precision_is_the_literal_loop():
    for n, kind in ((65, "rand50"), (65, "quant8"), (300, "rand02"), (64, "equal")):
        logits, slots, labels = sr.make_input(n, kind)
        a, b = sr.evaluate(logits, slots, labels), sr.evaluate(logits, slots, labels, fast=True)
        assert a["AP0"] == b["AP0"] and a["AP1"] == b["AP1"] and a["mAP"] == b["mAP"]
        assert np.abs(a["score"] - b["score"]).max() <= 1e-15 and np.array_equal(a["label"], b["label"])
    a, b = (sr.evaluate(*sr.make_input(64, "nonfinite"), fast=f) for f in (False, True))
    assert np.array_equal(np.isnan(a["score"]), np.isnan(b["score"])) and np.array_equal(a["order1"], b["order1"])


def test_degenerate_inputs_give_nan_as_the_reference_does():
    for kind, nan_keys, finite in (("allpos", ("AP0", "mAP"), "AP1"), ("allneg", ("AP1", "mAP"), "AP0")):
        for n in (1, 3):
            res = sr.evaluate(*sr.make_input(n, kind))
            assert all(math.isnan(res[k]) for k in nan_keys) and res[finite] == 1.0, (kind, n, res)
    res = sr.evaluate(*sr.make_input(64, "nonfinite"))
    assert res["n_nonfinite"] == 1 and math.isnan(res["AP0"]) and math.isnan(res["AP1"]) and math.isnan(res["mAP"])
    assert res["order1"][0] == 32 and res["order0"][-1] == 32 and res["TP"] + res["FN"] + res["FP"] + res["TN"] == 64
    half = sr.evaluate(*sr.make_input(64, "half"))
    assert (half["score"][::4] == 0.5).all() and half["TP"] + half["FP"] >= 16


def test_planted_inputs_carry_what_the_perturbations_need():
    logits, slots, labels = sr.planted()
    res = sr.evaluate(logits, slots, labels)
    s = res["score"]
    assert s[1] == s[2] and res["label"][1] != res["label"][2] and s[9] == s[10] and res["label"][9] != res["label"][10]
    assert s[6] == 0.5 and s[7] == 0.5 and res["label"][6] == 1 and res["label"][7] == 0
    assert res["order1"][0] == 0 and res["label"][0] == 1 and res["order0"][0] == 11 and res["label"][11] == 0
    assert list(res["order1"][1:3]) == [1, 2] and list(res["order0"][1:3]) == [9, 10]              # the lower row first, in both passes
    assert res["n_pos"] == 7 and res["n"] == 12


@pytest.mark.parametrize("perturb", sr.PERTURBATIONS)
def test_perturbed_reference_misses_its_bar(perturb):
    """Every deliberate mistake, on the planted inputs: a changed count (exact results have no margin), or an error of at least 10 x the
    bar - 2e-6 for the scores, 8 N 2^-53 for AP0 / AP1 / mAP."""
    logits, slots, labels = sr.planted()
    ref, bad = sr.evaluate(logits, slots, labels), sr.evaluate(logits, slots, labels, perturb=perturb)
    n = ref["n"]
    counts_changed = any(ref[k] != bad[k] for k in ("TP", "FN", "FP", "TN", "n_pos"))
    score_margin = float(np.abs(ref["score"] - bad["score"]).max()) / sr.SCORE_TOL
    ap_margin = max(abs(ref[k] - bad[k]) for k in ("AP0", "AP1", "mAP")) / sr.ap_tol(n)
    print(perturb, "counts changed", counts_changed, "score margin", f"{score_margin:.3g}", "AP margin", f"{ap_margin:.3g}")
    if perturb == "gt_threshold":
        assert counts_changed and bad["TP"] == ref["TP"] - 1 and bad["FP"] == ref["FP"] - 1
    elif perturb == "mean_after_softmax":
        assert score_margin >= sr.MARGIN
    else:
        assert score_margin == 0 and not counts_changed and ap_margin >= sr.MARGIN
    if perturb == "class0_on_label":
        assert bad["AP1"] == ref["AP1"] and bad["AP0"] != ref["AP0"]


# ---- host refusals -------------------------------------------------------------------------------------------------------------------------
P = 0x1000          # a non-null address: every call below is refused before any device work
CAP_MAX = 1 << 24


def _update(lib, logits=P, ld=2, B=8, slots=P, slot0=0, labels=P, capacity=64, scratch=P):
    return lib.egx_segment_scores_update(logits, ld, B, slots, slot0, labels, capacity, scratch, None)


def _ap(lib, N=8, capacity=64, scratch=P, score=P, order1=P, order0=P, result=P):
    return lib.egx_segment_ap(N, capacity, scratch, score, order1, order0, result, None)


REFUSALS = [
    (_update, dict(logits=None), "null pointer"),
    (_update, dict(labels=None), "null pointer"),
    (_update, dict(scratch=None), "null pointer"),
    (_update, dict(capacity=0), "1 <= capacity <= 16777216"),
    (_update, dict(capacity=CAP_MAX + 1), "1 <= capacity <= 16777216"),
    (_update, dict(ld=1), "ld >= 2"),
    (_update, dict(B=0), "1 <= B <= 16777216"),
    (_update, dict(B=-3), "1 <= B <= 16777216"),
    (_update, dict(slots=None, slot0=57), "slot0 + B <= capacity"),
    (_update, dict(slots=None, slot0=-1), "slot0 + B <= capacity"),
    (_ap, dict(scratch=None), "null pointer"),
    (_ap, dict(score=None), "null pointer"),
    (_ap, dict(order1=None), "null pointer"),
    (_ap, dict(order0=None), "null pointer"),
    (_ap, dict(result=None), "null pointer"),
    (_ap, dict(capacity=0), "1 <= capacity <= 16777216"),
    (_ap, dict(capacity=CAP_MAX + 1, N=CAP_MAX + 1), "1 <= capacity <= 16777216"),
    (_ap, dict(N=0), "1 <= N <= capacity"),
    (_ap, dict(N=65), "1 <= N <= capacity"),
]


@pytest.mark.parametrize("fn,kwargs,message", REFUSALS, ids=[f"{i}_{f.__name__}_{m.replace(' ', '_')}" for i, (f, _, m) in enumerate(REFUSALS)])
def test_host_refusals_before_any_device_work(egx_lib, fn, kwargs, message):
    egx_lib.egx_launch_count(1)
    assert fn(egx_lib, **kwargs) != 0
    assert message.encode() in egx_lib.egx_last_error(), egx_lib.egx_last_error()
    assert egx_lib.egx_launch_count(0) == 0


def test_scratch_query(egx_lib):
    small, big = egx_lib.egx_segment_ap_scratch(1), egx_lib.egx_segment_ap_scratch(CAP_MAX)
    assert 0 < small < big and big >= 36 * CAP_MAX
    assert egx_lib.egx_segment_ap_scratch(0) == 0 and b"1 <= capacity <= 16777216" in egx_lib.egx_last_error()
    assert egx_lib.egx_segment_ap_scratch(CAP_MAX + 1) == 0


def test_functional_refuses_cpu_tensors_and_bad_arguments(egx_lib):
    from egot2_amd import _lib, functional as F_egx
    state = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.segment_scores_update(state, 4, torch.zeros(3, 2), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.segment_ap(state, 4, 3)
    with pytest.raises(ValueError, match="capacity"):
        F_egx.segment_ap_state(0, "cpu")
    assert F_egx.SEG_AP_TILE == sr.tile() == 4096 and F_egx.SEG_AP_MAX_ROWS == CAP_MAX
    assert F_egx.SEG_AP_COUNTS == ("n", "n_pos", "TP", "FN", "FP", "TN", "n_nonfinite") and F_egx.SEG_AP_VALUES == ("AP0", "AP1", "mAP", "acc")


# ---- SegmentAPValidation on the host ---------------------------------------------------------------------------------------------------------
def test_step_result_keys_and_values_from_the_result_words():
    from egot2_amd.train import SegmentAPValidation
    val = SegmentAPValidation(64)
    with pytest.raises(RuntimeError, match="no forward"):
        val.step_result()
    with pytest.raises(RuntimeError, match="no update"):
        val.compute()
    b = val._result_buffers(torch.device("cpu"))
    assert val._result_buffers(torch.device("cpu")) is b and b["flat"].numel() == 11 and b["flat"].dtype == torch.int64
    assert b["score"].shape == (64,) and b["order1"].dtype == torch.int32 and b["mAP"].dtype == torch.float64
    b["flat"][:7] = torch.tensor([12, 7, 5, 2, 1, 4, 0])
    b["flat"][7:].view(torch.float64).copy_(torch.tensor([0.25, 0.75, 0.5, 0.75], dtype=torch.float64))
    val._last = {"buffers": b, "result": {}}
    r = val.step_result()
    assert set(r) == {"val_mAP", "val_acc", "val_AP0", "val_AP1", "val_TP", "val_FN", "val_FP", "val_TN", "val_n", "val_n_pos",
                      "val_n_nonfinite"}
    assert r["val_mAP"] == 0.5 and r["val_AP0"] == 0.25 and r["val_AP1"] == 0.75 and r["val_acc"] == 0.75
    assert (r["val_n"], r["val_n_pos"], r["val_TP"], r["val_FN"], r["val_FP"], r["val_TN"], r["val_n_nonfinite"]) == (12, 7, 5, 2, 1, 4, 0)
    assert b["TP"].item() == 5 and b["acc"].item() == 0.75            # the named views read the same words
    assert set(val.step_result("test")) == {k.replace("val_", "test_") for k in r}
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(ValueError, match="capacity"):
            SegmentAPValidation(bad)


def test_update_refusals_on_the_host(monkeypatch):
    """More rows than capacity, slots that decrease, device slots without rows=, slots with merge=False: raised before any device work
    (the functional layer is never reached)."""
    from egot2_amd import functional as F_egx
    from egot2_amd.train import SegmentAPValidation
    monkeypatch.setattr(F_egx, "segment_scores_update", lambda *a, **k: None)
    monkeypatch.setattr(SegmentAPValidation, "_result_buffers", lambda self, device, *dims: {"state": torch.zeros(4, dtype=torch.uint8)})
    x, y = torch.zeros(5, 2), torch.zeros(5, dtype=torch.int64)
    val = SegmentAPValidation(8)
    val.update(x, y)                                                  # rows 0 .. 4
    assert val._rows == 5
    with pytest.raises(ValueError, match="10 rows exceed capacity=8"):
        val.update(x, y)
    assert val._rows == 5
    val.update(x[:3], y[:3])
    assert val._rows == 8
    val.reset()
    assert val._rows == 0
    val.update(x, y, slots=[0, 0, 1, 3, 3])
    assert val._rows == 4
    val.update(x, y, slots=torch.tensor([3, 3, 3, 5, 7]))           # row 3 continues from the call before
    assert val._rows == 8
    with pytest.raises(ValueError, match="9 rows exceed capacity=8"):
        val.update(x, y, slots=[3, 3, 3, 5, 8])
    with pytest.raises(ValueError, match="non-decreasing"):
        val.update(x, y, slots=[0, 2, 1, 3, 3])
    with pytest.raises(ValueError, match="non-decreasing"):
        val.update(x, y, slots=[-1, 0, 1, 3, 3])
    with pytest.raises(ValueError, match="4 slots for 5 windows"):
        val.update(x, y, slots=[0, 1, 2, 3])
    with pytest.raises(ValueError, match="slots are not taken"):
        SegmentAPValidation(8, merge=False).update(x, y, slots=[0, 1, 2, 3, 4])


def test_update_and_compute_refuse_a_capture(monkeypatch):
    """The row cursor is host state: inside a stream capture update, compute and reset raise (the real capture: test_gpu_segment_ap.py)."""
    from egot2_amd.train import SegmentAPValidation
    monkeypatch.setattr(SegmentAPValidation, "_capturing", staticmethod(lambda device: True))
    val = SegmentAPValidation(8)
    with pytest.raises(RuntimeError, match="update cannot be captured in a graph: the row cursor is host state"):
        val.update(torch.zeros(5, 2), torch.zeros(5, dtype=torch.int64))
    val._device, val._rows = torch.device("cpu"), 5
    with pytest.raises(RuntimeError, match="compute cannot be captured"):
        val.compute()
    with pytest.raises(RuntimeError, match="reset cannot be captured"):
        val.reset()
