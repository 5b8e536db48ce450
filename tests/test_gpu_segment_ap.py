"""-m gpu: the TTM / LAM validation accumulator on the device - egx_segment_scores_update / egx_segment_ap against the fp64 gate
tests/segment_ap_ref.py at every size where the kernels take another path (a wave, the single-workgroup tile, the multi-launch chain, the
largest grid of the single-level cross-tile scans), the split feeds, train.SegmentAPValidation on the recorded reference epoch and behind
a TTM translator's ragged eval forward. Measured figures: tools/segment_ap_eval.py, profiles/segment_ap_report.txt."""
import math
import os

import numpy as np
import pytest
import torch

from tests import segment_ap_ref as sr
from tests.util import hhi_args, seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "segment_ap.npz")
CASES = [(n, kind) for n in sr.sizes() for kind in sr.kinds_for(n)]


def _device_epoch(cuda, logits, slots, labels, n, cuts=(), capacity=None, runs=1):
    """update() over the batch cut at `cuts`, then `runs` computes through the functional layer, every output prefilled -> list of dicts of
    host arrays (`bits`: the 11 result words)."""
    from egot2_amd import functional as F_egx
    capacity = capacity or n
    state = F_egx.segment_ap_state(capacity, cuda)
    x, s, y = (torch.from_numpy(a).to(cuda) for a in (logits, slots, labels))
    edges = [0, *cuts, len(slots)]
    for a, b in zip(edges[:-1], edges[1:]):
        F_egx.segment_scores_update(state, capacity, x[a:b], y[a:b], s[a:b])
    outs = []
    for _ in range(runs):
        out = {"flat": torch.full((11,), -7, dtype=torch.int64, device=cuda), "score": torch.full((n,), -3.0, device=cuda),
               "order1": torch.full((n,), -1, dtype=torch.int32, device=cuda), "order0": torch.full((n,), -1, dtype=torch.int32, device=cuda)}
        res = F_egx.segment_ap(state, capacity, n, out=out)
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in res.items()}
        host["bits"] = host.pop("flat").copy()
        outs.append(host)
    return outs


def _check_against_gate(got, ref, n, tag):
    """The checks of one epoch: scores to 2e-6, both orders = the stable argsort of the device's own scores, counts exact, AP0 / AP1 / mAP
    = the gate's algorithm on the device's scores and order within 8 N 2^-53 (nan = nan)."""
    score = got["score"].astype(np.float64)
    both_nan = np.isnan(score) & np.isnan(ref["score"])
    err = float(np.abs(np.where(both_nan, 0.0, score - ref["score"])).max())
    print(tag, "score err", f"{err:.3e}")
    assert not np.isnan(err) and err <= sr.SCORE_TOL, (tag, err)
    order1, order0 = sr.stable_orders(got["score"])
    assert np.array_equal(got["order1"], order1) and np.array_equal(got["order0"], order0), tag
    label = ref["label"]
    cm = sr.compute_confusion_matrix(got["score"], label)
    counts = {k: int(got[k]) for k in ("n", "n_pos", "TP", "FN", "FP", "TN", "n_nonfinite")}
    assert counts == {"n": n, "n_pos": ref["n_pos"], **cm, "n_nonfinite": ref["n_nonfinite"]}, (tag, counts)
    near_half = (np.abs(ref["score"] - 0.5) <= sr.SCORE_TOL) & (ref["score"] != 0.5)
    if not near_half.any():                                          # no row whose fp32 score may fall on the other side of 0.5
        assert {k: counts[k] for k in cm} == {k: ref[k] for k in cm}, (tag, counts)
    assert float(got["acc"]) == (cm["TP"] + cm["TN"]) / n
    if ref["n_nonfinite"]:
        want = (float("nan"),) * 3
    else:
        want = sr.ap_on_order(label, got["order1"].astype(np.int64), got["order0"].astype(np.int64), fast=n > 300)
    for k, w in zip(("AP0", "AP1", "mAP"), want):
        g = float(got[k])
        print(tag, k, g, w, "diff", 0.0 if (math.isnan(g) and math.isnan(w)) else abs(g - w), "tol", sr.ap_tol(n))
        assert sr.same(g, w, sr.ap_tol(n)), (tag, k, g, w)
    return err


@pytest.mark.parametrize("n,kind", CASES, ids=[f"N{n}_{k}" for n, k in CASES])
def test_epoch_against_the_gate(egx_lib, cuda, n, kind):
    """One epoch per size and input kind, fed in one call; two computes are bit-identical."""
    logits, slots, labels = sr.make_input(n, kind)
    ref = sr.evaluate(logits, slots, labels, n_rows=n, fast=n > 300)
    a, b = _device_epoch(cuda, logits, slots, labels, n, runs=2)
    _check_against_gate(a, ref, n, f"N{n}_{kind}")
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    if kind in ("allpos", "allneg"):
        assert math.isnan(float(a["mAP"])) and math.isnan(float(a["AP0" if kind == "allpos" else "AP1"]))
        assert abs(float(a["AP1" if kind == "allpos" else "AP0"]) - 1.0) <= sr.ap_tol(n)
    if kind == "half":
        assert (a["score"][::4] == 0.5).all()
    if kind == "nonfinite":
        assert int(a["n_nonfinite"]) == 1 and a["order1"][0] == n // 2 and a["order0"][-1] == n // 2


def test_scores_do_not_depend_on_how_the_batch_is_cut(egx_lib, cuda):
    """Segments of 1 .. 9 windows fed in one call and cut in two at EVERY position: the stored scores, both orders and every result word
    are bit-identical; so are three cuts at once, and an accumulator larger than the row count."""
    n = 11
    logits, slots, labels = sr.make_input(n, "rand50", seed=5)
    assert np.bincount(slots).min() >= 1 and np.bincount(slots).max() >= 7
    whole = _device_epoch(cuda, logits, slots, labels, n)[0]
    _check_against_gate(whole, sr.evaluate(logits, slots, labels), n, "whole")
    B = len(slots)
    feeds = [(c,) for c in range(1, B)] + [(2, B // 2, B - 1)]
    for cuts in feeds:
        got = _device_epoch(cuda, logits, slots, labels, n, cuts=cuts, capacity=n if len(cuts) == 1 else 5000)[0]
        for k in whole:
            assert whole[k].tobytes() == got[k].tobytes(), (cuts, k)


def test_lam_rows_and_out_of_range_slots(egx_lib, cuda):
    """slots=None: window i is row slot0 + i. A slot outside the accumulator is dropped: its row stays empty (a non-finite score)."""
    from egot2_amd import functional as F_egx
    n = 70
    logits, slots, labels = sr.make_input(n, "rand50", max_windows=1)
    ref = sr.evaluate(logits, slots, labels)
    state = F_egx.segment_ap_state(n, cuda)
    x, y = torch.from_numpy(logits).to(cuda), torch.from_numpy(labels).to(cuda)
    F_egx.segment_scores_update(state, n, x[:33], y[:33], None, 0)
    F_egx.segment_scores_update(state, n, x[33:], y[33:], None, 33)
    res = F_egx.segment_ap(state, n, n)
    score = res["score"].cpu().numpy()
    assert np.abs(score - ref["score"]).max() <= sr.SCORE_TOL
    own = sr.run_evaluation(score, ref["label"])                      # the gate's algorithm on the device's own fp32 scores
    assert np.array_equal(res["order1"].cpu().numpy(), own["order1"]) and np.array_equal(res["order0"].cpu().numpy(), own["order0"])
    assert all(sr.same(float(res[k]), own[k], sr.ap_tol(n)) for k in ("AP0", "AP1", "mAP"))
    state.zero_()
    bad = torch.tensor([0, 1, 2, n, n + 5, 1 << 40], device=cuda)
    F_egx.segment_scores_update(state, n, x[:6], y[:6], bad)
    res = F_egx.segment_ap(state, n, 4)
    assert int(res["n_nonfinite"]) == 1 and torch.isnan(res["score"][3]) and torch.isfinite(res["score"][:3]).all()
    assert math.isnan(float(res["mAP"]))


@pytest.mark.parametrize("name", ["ttm_a", "ttm_b", "lam_a"])
def test_validation_module_on_the_recorded_reference_epoch(egx_lib, cuda, name):
    """train.SegmentAPValidation end to end on the epochs the REAL PostProcessor / run_evaluation recorded (tie-free): reset, update per
    batch (host slots; LAM without), step_result. Counts and acc exactly, mAP and the APs to the bound of the device's own arithmetic plus
    nothing else - the recorded order is the device's order wherever no two scores are within the fp32 bar."""
    from egot2_amd.train import SegmentAPValidation
    z = np.load(GOLDEN)
    g = lambda k: z[f"{name}_{k}"]  # noqa: E731
    logits, slots, labels = g("logits"), g("slots"), g("labels")
    n = len(g("score"))
    lam = name.startswith("lam")
    val = SegmentAPValidation(512, merge=not lam).reset()
    x, y = torch.from_numpy(logits).to(cuda), torch.from_numpy(labels).to(cuda)
    for a in range(0, len(slots), 29):
        b = min(a + 29, len(slots))
        val.update(x[a:b], y[a:b], None if lam else slots[a:b].tolist())
    r = val.step_result()
    st = val.stats()
    score = st["score"].cpu().numpy()
    assert score.shape == (n,) and np.abs(score - g("score")).max() <= sr.SCORE_TOL
    assert np.array_equal(st["order1"].cpu().numpy(), np.argsort(-g("score"), kind="stable"))       # the recorded epoch is tie-free
    assert np.array_equal(st["order0"].cpu().numpy(), np.argsort(g("score"), kind="stable"))
    assert [r["val_TP"], r["val_FN"], r["val_FP"], r["val_TN"]] == g("confusion").tolist() and r["val_acc"] == float(g("acc"))
    assert r["val_n"] == n and r["val_n_pos"] == int(g("row_label").sum()) and r["val_n_nonfinite"] == 0
    for k, want in (("val_AP0", g("AP")[0]), ("val_AP1", g("AP")[1]), ("val_mAP", float(g("mAP")))):
        print(name, k, r[k], want, abs(r[k] - want))
        assert abs(r[k] - want) <= sr.ap_tol(n) + sr.FIXTURE_AP_TOL
    assert float(st["mAP"]) == r["val_mAP"]
    # a second epoch after reset() gives the same bits
    val.reset()
    val.update(x, y, None if lam else torch.from_numpy(slots).to(cuda), rows=None if lam else n)
    assert val.step_result() == r


def test_capture_is_refused_and_capacity_holds(egx_lib, cuda):
    from egot2_amd.train import SegmentAPValidation
    val = SegmentAPValidation(16, merge=False)
    x, y = torch.randn(10, 2, device=cuda), torch.zeros(10, dtype=torch.int64, device=cuda)
    val.update(x, y)
    with pytest.raises(ValueError, match="20 rows exceed capacity=16"):
        val.update(x, y)
    doubled = torch.zeros_like(x)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        with pytest.raises(RuntimeError, match="update cannot be captured in a graph"):
            val.update(x[:2], y[:2])
        with pytest.raises(RuntimeError, match="compute cannot be captured in a graph"):
            val.compute()
        torch.mul(x, 2.0, out=doubled)                               # the capture itself goes on
    torch.cuda.synchronize()
    assert val.step_result()["val_n"] == 10


def test_ttm_translator_eval_forward_feeds_the_accumulator(egx_lib, cuda):
    """A TaskFusionMFTransformer3Task eval forward over a ragged batch (windows of their own lengths) -> update -> the metric, against the
    gate on the logits the model returned."""
    from egot2_amd import hhi_ttm
    from egot2_amd.train import SegmentAPValidation
    model = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(num_layers=1))
    model.load_state_dict(seeded_state_dict(model, seed=811))
    model = model.to(cuda).eval()
    lengths = [15, 22, 9, 30, 30, 17, 12, 25, 19, 30, 11, 16, 28]
    slots = [0, 0, 0, 1, 2, 2, 3, 3, 3, 3, 4, 5, 5]
    labels = torch.tensor([1, 0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0, 0])
    feats = [f.to(cuda) for f in seeded_feats(93, [(len(lengths), 30, 256)] * 3)]
    val = SegmentAPValidation(64).reset()
    with torch.no_grad():
        for a, b in ((0, 5), (5, 13)):                               # segment 2 continues across the two batches
            logits = model.forward_features(*[f[a:b] for f in feats], lengths=lengths[a:b])
            assert logits.shape == (b - a, 2)
            val.update(logits, labels[a:b].to(cuda), slots[a:b])
            if a == 0:
                first = logits.cpu().numpy()
    r = val.step_result()
    ref = sr.evaluate(np.concatenate([first, logits.cpu().numpy()]), np.asarray(slots), labels.numpy())
    st = val.stats()
    assert np.abs(st["score"].cpu().numpy() - ref["score"]).max() <= sr.SCORE_TOL
    assert np.array_equal(st["order1"].cpu().numpy(), ref["order1"]) and np.array_equal(st["order0"].cpu().numpy(), ref["order0"])
    assert (r["val_n"], r["val_n_pos"]) == (6, 3) and [r[f"val_{k}"] for k in ("TP", "FN", "FP", "TN")] == [ref[k] for k in ("TP", "FN", "FP", "TN")]
    for k in ("AP0", "AP1", "mAP"):
        assert sr.same(r[f"val_{k}"], ref[k], sr.ap_tol(6)), (k, r[f"val_{k}"], ref[k])
