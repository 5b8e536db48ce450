"""CPU suite of the PNR keyframe criterion (egx_keyframe_criterion, functional.keyframe_criterion, train.KeyframeCriterion / OSCCCriterion):
the gate tests/keyframe_ref.py against the recording of the reference's own loss and metric functions, its bars, its perturbed references,
the host refusals of the C entry point and the arithmetic of the two step_result methods."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import keyframe_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "pnr_criterion.npz")
N = len(kr.CASES)


@pytest.fixture(scope="module")
def evals():
    """case index -> (fp64 reference, fp32 evaluation), computed once."""
    return {i: (kr.evaluate(i, kr.F64), kr.evaluate(i, torch.float32)) for i in range(N)}


def _same_exact(a, b, T):
    """pred, label_frame, counts equal; dist within the gate's rule; dist_sum within DIST_TOL."""
    return (all(torch.equal(a[k], b[k]) for k in kr.EXACT) and kr.dist_ok(a["dist"], b["dist"], T)
            and abs(a["dist_sum"] - b["dist_sum"]) <= kr.DIST_TOL * abs(b["dist_sum"]))


# ---- the gate against the recorded reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b"])
def test_gate_reproduces_the_recorded_reference_step(name):
    """The gate in fp64 against the REAL nn.BCELoss(sigmoid(.)) / masked CrossEntropyLoss, keyframe_distance, keyframe_accuracy and
    PnrOsccMetric as tests/golden/make_golden_pnrcrit.py recorded them: loss to 1e-9 relative, metrics exactly."""
    z = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(z[f"{name}_{k}"])  # noqa: E731
    logits, labels, sc, fps = t("logits"), t("labels"), t("sc"), t("fps")
    info = {"clip_start_frame": t("start"), "clip_end_frame": t("end"), "pnr_frame": t("pnr")}
    B = logits.shape[0]
    x = logits[:, 0].double()
    for kind, key in (("bce", "bce"), ("ce", "ce")):
        res = kr.keyframe_criterion(x, labels.float(), None, sc.reshape(B), fps, info, 16, None, kind)
        want = float(z[f"{name}_{key}"])
        assert abs(res["loss"].item() - want) <= 1e-9 * abs(want), (kind, res["loss"].item(), want)
        n_sc, n_correct = int(res["counts"][0]), int(res["counts"][1])
        assert [n_correct, n_sc] == z[f"{name}_acc"].tolist()
        assert res["dist_sum"] / n_sc == float(z[f"{name}_dist"])
        assert torch.equal(res["label_frame"], labels.argmax(1))
    dec = t("dec")
    V = dec.shape[1]
    pnr = kr.keyframe_criterion(dec.double(), None, None, None, fps, info, 16, z[f"{name}_pnr_cols"].tolist(), "metric", V)
    assert [pnr["dist_sum"] / B, int(pnr["counts"][2]) / B] == z[f"{name}_pnr_distance"].tolist()
    oscc = kr.keyframe_criterion(dec.double(), None, sc.reshape(B), None, fps, info, 2, z[f"{name}_oscc_cols"].tolist(), "metric", V)
    assert [int(oscc["counts"][1]) / B, int(oscc["counts"][2]) / B] == z[f"{name}_oscc_acc"].tolist()
    assert 0 < int(pnr["counts"][2]) < B and 0 < int(oscc["counts"][1]) < B          # the recording is no degenerate one


def test_inputs_carry_the_planted_cases(evals):
    ids = [kr.case_id(c) for c in kr.CASES]
    assert len(set(ids)) == N
    i = ids.index("B5_T16_ld16_bce")
    a, ref = kr.kf_inputs(i), evals[i][0]
    assert a["logits"].dtype == torch.float32 and a["target"].dtype == torch.float32 and a["fps"].dtype == torch.float64
    assert a["logits"][0, 8] == a["logits"][0, 15] == 12.5 and ref["pred"][0] == 8           # two equal maxima: the lower frame
    assert ref["pred"][1] == 0 and ref["pred"][2] == 15                                      # the maximum at frame 0 and at T - 1
    assert a["logits"][3, 0] == 80 and a["logits"][3, 1] == -80 and a["target"][3, 1] == 1
    assert ref["loss_rows"][3].item() == pytest.approx(160 / 16, rel=0.2)                     # two terms of 80, no clamp, no overflow
    assert a["target"][4, 0] == 0.25 and a["target"][4, 1] == 0.75 and a["target"][4].sum() == 1
    assert a["state_change"][1] == 0 and a["state_change"][0] == 1 and ref["dist"][1] == 0
    assert a["info"]["clip_end_frame"][2] == a["info"]["clip_start_frame"][2]
    assert a["fps"][0] == 29.97 and a["fps"][1] == 30.0
    assert torch.isfinite(ref["d_logits"]).all() and math.isfinite(ref["loss"].item())
    sc0 = evals[ids.index("B4_T16_ld16_ce_sc0")][0]                                            # no state-change clip at all
    assert sc0["counts"].tolist() == [0, 0, 0, 4] and sc0["dist_sum"] == 0.0 and sc0["loss"] == 0 and (sc0["d_logits"] == 0).all()
    gaps = evals[ids.index("B2_T17_ld20_bce")][0]
    assert (gaps["d_logits"][:, 17:] == 0).all() and (gaps["d_logits"][:, :17] != 0).all()
    j = ids.index("B5_T16_ld593_metric_cols")
    m, mref = kr.kf_inputs(j), evals[j][0]
    assert torch.isnan(m["logits"][3, kr.COLS16[8]]) and mref["pred"][3] == 8                  # a NaN row: pred = its frame
    assert mref["counts"].tolist() == [5, 0, 1, 5] and m["logits"][4].argmax().item() not in kr.COLS16
    o = evals[ids.index("B5_T2_ld593_metric_cols")][0]
    assert o["counts"][3] == 5 and 0 < o["counts"][1] <= 5
    k = ids.index("B5_T16_ld16_ce_label")                                                       # CE against `label`, one label out of range
    la, lref = kr.kf_inputs(k), evals[k][0]
    assert la["target"] is None and la["label"][4] == 16 and la["state_change"][4] == 1
    assert lref["label_frame"][4] == -1 and lref["loss_rows"][4] == 0 and (lref["d_logits"][4] == 0).all() and lref["loss_rows"][0] > 0
    assert kr.saturated_rows(k) == [3] and kr.saturated_rows(ids.index("B3_T2_ld2_ce")) == []
    big = evals[ids.index("B257_T16_ld16_ce")][0]
    assert 0 < big["counts"][1] < big["counts"][0] < 257


def test_fp32_reference_meets_the_bar(evals):
    """The fp32 evaluation of the gate passes its own bars, matches every exact result, and the recorded FP32_ERR constants are what it
    measures."""
    worst = {k: 0.0 for k in kr.KINDS}
    for i, (ref, f32) in evals.items():
        B, T, ld, cols, V, kind, flags = kr.CASES[i]
        assert _same_exact(f32, ref, T) and torch.equal(f32["dist"], ref["dist"]), kr.case_id(kr.CASES[i])
        if kind == "metric":
            assert ref["loss"] is None and ref["d_logits"] is None
            continue
        errs = kr.bar_errors(f32, ref, i)
        for k in kr.KINDS:
            e = errs[k]
            worst[k] = max(worst[k], e)
            assert e <= kr.BAR[k], (kr.case_id(kr.CASES[i]), k, e)
    print("FP32_ERR measured:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k in kr.KINDS:
        assert kr.FP32_ERR[k] / 3 <= worst[k] <= kr.FP32_ERR[k] * 3, (k, worst[k], kr.FP32_ERR[k])


@pytest.mark.parametrize("perturb", kr.PERTURBATIONS)
def test_perturbed_reference_is_rejected(evals, perturb):
    """Every deliberate mistake misses a bar by >= 3x, or changes an exact result (pred, counts, dist), on every case where it changes
    anything; and it changes something."""
    ratios, exact_hits = [], 0
    for i, (ref, _) in evals.items():
        B, T, ld, cols, V, kind, flags = kr.CASES[i]
        bad = kr.evaluate(i, kr.F64, perturb)
        ratio = 0.0 if kind == "metric" else max(e / kr.BAR[k] for k, e in kr.bar_errors(bad, ref, i).items())
        if not _same_exact(bad, ref, T):
            exact_hits += 1
        elif ratio > 0:
            ratios.append(ratio)
    print(perturb, "min ratio", min(ratios) if ratios else None, "cases with a changed exact result", exact_hits)
    assert ratios or exact_hits
    assert all(r >= 3 for r in ratios), (perturb, min(ratios))
    want = kr.PERTURB_RATIO[perturb]
    if want == "exact":
        assert exact_hits > 0 and not ratios
    else:
        assert ratios and want / 3 <= min(ratios) <= want * 3, (perturb, min(ratios), want)


# ---- host refusals of egx_keyframe_criterion ------------------------------------------------------------------------------------------------
P = 0x1000          # a non-null address: every call below is refused before any device work


def _call(lib, logits=P, ld=16, B=5, T=16, cols=None, V=16, kind=0, target=P, label=None, state_change=None, fps=P, clip_start=P,
          clip_end=P, pnr_frame=P, loss=P, loss_rows=None, d_logits=None, pred=P, label_frame=None, counts=P, dist=P, dist_sum=P, scratch=P):
    ca = (C.c_int * len(cols))(*cols) if cols is not None else None
    return lib.egx_keyframe_criterion(logits, ld, B, T, ca, V, kind, target, label, state_change, fps, clip_start, clip_end, pnr_frame, loss,
                                      loss_rows, d_logits, pred, label_frame, counts, dist, dist_sum, scratch, None)


COLS3 = dict(T=3, cols=(9, 2, 5), V=11, ld=12)
REFUSALS = [
    (dict(logits=None), "null pointer"),
    (dict(counts=None), "null pointer"),
    (dict(pred=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(loss=None), "null pointer"),
    (dict(B=0), "1 <= B <= 268435456"),
    (dict(B=2 ** 28 + 1), "1 <= B <= 268435456"),
    (dict(T=0, V=0), "1 <= T <= 64"),
    (dict(T=65, V=65, ld=65), "1 <= T <= 64"),
    (dict(V=15), "T <= V <= 2048"),
    (dict(**{**COLS3, "V": 2049, "ld": 4096}), "T <= V <= 2048"),
    (dict(V=17, ld=17), "without cols"),
    (dict(ld=15), "ld >= V"),
    (dict(**{**COLS3, "ld": 10}), "ld >= V"),
    (dict(**{**COLS3, "cols": (9, 2, 11)}), "0 <= column < V"),
    (dict(**{**COLS3, "cols": (-1, 2, 5)}), "0 <= column < V"),
    (dict(**{**COLS3, "cols": (9, 2, 9)}), "duplicate"),
    (dict(kind=3), "kind=3"),
    (dict(kind=-1), "kind=-1"),
    (dict(kind=0, target=None), "bce needs target"),
    (dict(kind=0, target=None, label=P), "bce needs target"),
    (dict(kind=1, target=None), "ce needs target or label"),
    (dict(kind=2), "metric takes no loss"),
    (dict(kind=2, loss=None, loss_rows=P), "metric takes no loss"),
    (dict(kind=2, loss=None, d_logits=P), "metric takes no loss"),
    (dict(fps=None), "3 of the 4 timing arrays"),
    (dict(clip_end=None, pnr_frame=None), "2 of the 4 timing arrays"),
    (dict(clip_start=None, clip_end=None, pnr_frame=None), "1 of the 4 timing arrays"),
    (dict(fps=None, clip_start=None, clip_end=None, pnr_frame=None), "without the timing arrays"),
    (dict(fps=None, clip_start=None, clip_end=None, pnr_frame=None, dist=None), "without the timing arrays"),
]


@pytest.mark.parametrize("kwargs,message", REFUSALS, ids=[f"{i}_{m.replace(' ', '_')}" for i, (_, m) in enumerate(REFUSALS)])
def test_host_refusals_before_any_device_work(egx_lib, kwargs, message):
    egx_lib.egx_launch_count(1)
    assert _call(egx_lib, **kwargs) != 0
    assert message.encode() in egx_lib.egx_last_error(), egx_lib.egx_last_error()
    assert egx_lib.egx_launch_count(0) == 0


def test_scratch_query(egx_lib):
    n = egx_lib.egx_keyframe_scratch(5)
    assert n >= 64 + 64 * (8 + 4 + 12) and egx_lib.egx_keyframe_scratch(2 ** 28) == n        # one layout for every valid B
    assert egx_lib.egx_keyframe_scratch(0) == 0 and b"1 <= B <= 268435456" in egx_lib.egx_last_error()
    assert egx_lib.egx_keyframe_scratch(2 ** 28 + 1) == 0


def test_functional_refuses_cpu_tensors_and_bad_arguments(egx_lib):
    from egot2_amd import _lib, functional as F_egx
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.keyframe_criterion(torch.zeros(2, 16), torch.zeros(2, 16))
    assert F_egx.KEYFRAME_KINDS == {"bce": 0, "cross_entropy": 1, None: 2}


# ---- KeyframeCriterion.step_result / OSCCCriterion.step_result -------------------------------------------------------------------------------
def _filled(crit, B=8, T=16, loss=0.75, counts=(5, 2, 3, 8), dist_sum=12.5):
    b = crit._result_buffers(torch.device("cpu"), B, T)
    assert crit._result_buffers(torch.device("cpu"), B, T) is b                               # persistent per shape
    b["loss"].fill_(loss)
    b["counts"].copy_(torch.tensor(counts, dtype=torch.int32))
    b["dist_sum"].fill_(dist_sum)
    crit._last = b
    return b


def test_keyframe_step_result_arithmetic_and_key_names():
    """The packed result buffer on CPU stand-in tensors: keys and values of the reference's step results
    (HOI/tasks/pnr/video_taskspecific_pnr.py:57-63 and :89-93)."""
    from egot2_amd.train import KeyframeCriterion
    crit = KeyframeCriterion("bce")
    with pytest.raises(RuntimeError, match="no forward"):
        crit.step_result()
    b = _filled(crit)
    assert b["flat"].numel() == 8 and b["counts"].dtype == torch.int32 and b["dist_sum"].dtype == torch.float64
    assert b["pred"].shape == (8,) and b["dist"].dtype == torch.float64
    r = crit.step_result()
    assert set(r) == {"keyframe_loss", "train_loss", "loss", "pseudo_acc", "keyframe_loc_metric_time_dist_train"}
    assert r["keyframe_loss"] == r["train_loss"] == r["loss"] == 0.75
    assert r["pseudo_acc"] == 2 / 5 and r["keyframe_loc_metric_time_dist_train"] == 12.5 / 5
    v = crit.step_result("val")
    assert set(v) == {"keyframe_loc_metric_time_dist_val", "keyframe_loc_metric_time_dist_val_neg", "pseudo_acc"}
    assert v["keyframe_loc_metric_time_dist_val"] == 2.5 and v["keyframe_loc_metric_time_dist_val_neg"] == -2.5 and v["pseudo_acc"] == 0.4
    with pytest.raises(ValueError):
        crit.step_result("test")
    # a batch without a state-change clip: distance 0.0 (the reference's np.mean(0.0)), accuracy nan (the reference divides by zero)
    _filled(crit, counts=(0, 0, 0, 8), dist_sum=0.0)
    e = crit.step_result()
    assert e["keyframe_loc_metric_time_dist_train"] == 0.0 and math.isnan(e["pseudo_acc"]) and e["loss"] == 0.75
    ev = crit.step_result("val")
    assert ev["keyframe_loc_metric_time_dist_val"] == 0.0 and ev["keyframe_loc_metric_time_dist_val_neg"] == 0.0 and math.isnan(ev["pseudo_acc"])
    # the EgoT2-g metric: means over all B clips
    metric = KeyframeCriterion(None, cols=range(16))
    _filled(metric, counts=(8, 6, 3, 8), dist_sum=12.0)
    assert metric.step_result("val") == {"dist": 1.5, "err": 3 / 8, "acc": 6 / 8}
    # stats() hands out only what the last call wrote: no loss without a loss_func, no distance without fps / info
    st = metric.stats()
    assert st["loss"] is None and st["loss_rows"] is None and st["dist_sum"] is not None and st["counts"] is not None
    metric._last["timed"] = False
    st = metric.stats()
    assert st["dist"] is None and st["dist_sum"] is None and st["pred"] is not None and math.isnan(metric.step_result()["dist"])
    assert all(v is not None for v in crit.stats().values())
    for bad in ("mse", "BCE", ""):
        with pytest.raises(ValueError, match="loss_func"):
            KeyframeCriterion(bad)
    with pytest.raises(ValueError, match="columns"):
        KeyframeCriterion(None, cols=range(65))
    assert KeyframeCriterion("cross_entropy").loss_func == "cross_entropy"


def test_oscc_step_result_arithmetic_and_key_names():
    """StateChangeClassification2Loader's step results (video_taskspecific_pnr.py:155-160, :182-184) from the LTA criterion's buffer."""
    from egot2_amd.train import OSCCCriterion
    crit = OSCCCriterion()
    with pytest.raises(RuntimeError, match="no forward"):
        crit.step_result()
    b = crit._crit._result_buffers(torch.device("cpu"), 1, 1)
    assert b["flat"].numel() == 4
    b["loss"].fill_(0.5)
    b["n_valid"].fill_(8)
    b["correct"].fill_(6)
    crit._crit._last, crit._B = b, 8
    r = crit.step_result()
    assert r == {"state_change_loss": 0.5, "train_loss": 0.5, "loss": 0.5, "state_change_metric_train": 0.75}
    assert crit.step_result("val") == {"state_change_metric_val": 0.75}
    b["correct"].fill_(0)
    assert crit.step_result("val") == {"state_change_metric_val": 0.0}
    with pytest.raises(ValueError):
        OSCCCriterion()(torch.zeros(4, 2), torch.zeros(4))


def test_buffers_are_not_created_inside_a_capture(monkeypatch):
    """A buffer created inside a capture would live in that graph's private pool: refused, with the message the other criteria use."""
    from egot2_amd.train import KeyframeCriterion
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="run one eager step at this problem size before capturing it in a graph"):
        KeyframeCriterion()._result_buffers(torch.device("cuda", 0), 5, 16)
