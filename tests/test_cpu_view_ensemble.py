"""CPU suite of the action-recognition test epoch (egx_view_ensemble_state / _update / _topk, functional.view_ensemble_*,
train.ViewEnsembleTest): the gate tests/view_ensemble_ref.py against the recording of the reference's own test_epoch_end, its perturbed
references on the planted inputs, the exported symbols, the host refusals of the C entry points and the host side of ViewEnsembleTest."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import view_ensemble_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "view_ensemble.npz")
FIXTURE_CASES = [(c, m) for c in ("a", "b") for m in ("sum", "max")]
ERR_KEYS = ("top1_verb_err", "top5_verb_err", "top1_noun_err", "top5_noun_err")
SYMBOLS = ("egx_view_ensemble_state", "egx_view_ensemble_update", "egx_view_ensemble_topk")


# ---- the gate against the recorded reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,method", FIXTURE_CASES)
def test_gate_reproduces_the_recorded_reference_epoch(case, method):
    """The gate against the REAL MultiTaskClassificationTask.test_epoch_end as tests/golden/make_golden_viewens.py recorded it: the rows bit
    for bit (the same fp32 operations in the same order), the labels, and the four errors exactly."""
    z = np.load(GOLDEN)
    g = lambda k: z[f"{case}_{k}"]  # noqa: E731
    classes = tuple(int(c) for c in g("classes"))
    res = vr.evaluate(g("preds"), g("labels"), g("clip_ids").tolist(), classes, method)
    rows = g(f"{method}_rows")
    assert res["rows"].dtype == np.float32 and rows.dtype == np.float32
    assert np.array_equal(res["rows"].view(np.uint32), rows.view(np.uint32))
    assert np.array_equal(res["labels"], g(f"{method}_video_labels"))
    want = dict(zip(ERR_KEYS, g(f"{method}_err").tolist()))
    got = {k: res["result"][k] for k in ERR_KEYS}
    print(case, method, got, want)
    assert got == want
    assert res["n"] == rows.shape[0] and res["n_nonfinite"] == 0 and not res["n_invalid"].any() and res["n_dropped"] == 0
    assert (res["views"] == (3 if case == "a" else 30)).all()
    # tie-free at the label, so the tie rule does not enter
    assert np.array_equal(vr.rank_rows(rows, res["labels"], classes, perturb="higher_class_wins_ties")["rank"], res["rank"])


def test_fixture_errors_are_informative():
    z = np.load(GOLDEN)
    errs = np.concatenate([z[f"{c}_{m}_err"] for c, m in FIXTURE_CASES])
    assert len(np.unique(errs)) >= 5 and errs.min() == 0.0 and errs.max() == 100.0
    ids = z["b_clip_ids"]
    assert (np.diff(ids) < 0).any() and np.bincount(ids).tolist() == [30] * 4            # interleaved, 30 views each


@pytest.mark.reference
def test_fixture_reproduces_from_the_live_test_epoch_end():
    import subprocess
    import sys
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference tree is not available")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_viewens.py"), "--check"], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0 and "check True max_diff 0.000e+00" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


# ---- the planted input and the perturbed references ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("sum", "max"))
def test_planted_inputs_carry_what_the_perturbations_need(method):
    preds, labels, ids = vr.planted(method)
    res = vr.evaluate(preds, labels, ids, vr.PLANTED_CLASSES, method)
    row = {k: i for i, k in enumerate(res["ids"])}
    assert res["ids"] == ["first", "order", "negative", "plain", "tie", "invalid", "nan"]           # first-appearance order
    assert res["n"] == 7 and res["n_dropped"] == 1 and res["n_nonfinite"] == 1 and res["n_invalid"].tolist() == [1, 0]
    assert res["views"].tolist() == [2, 3, 2, 3, 1, 1, 1]
    assert res["labels"][row["first"]].tolist() == [1, 4] and res["rank"][row["first"]].tolist() == [0, 0]
    assert res["labels"][row["plain"]].tolist() == [2, 6]                                          # the last view's label
    assert res["rank"][row["tie"]].tolist() == [1, 0] and res["pred"][row["tie"]].tolist() == [1, 3]
    assert res["rank"][row["invalid"]].tolist() == [-1, 0]
    assert res["pred"][row["nan"]].tolist() == [0, 2] and res["rank"][row["nan"]].tolist() == [0, 1]
    if method == "max":
        assert not res["rows"][row["negative"]].any() and res["rank"][row["negative"]].tolist() == [0, 0]
        assert res["rows"][row["order"]][4] == float(1 << 24)
    else:
        assert res["rank"][row["negative"]].tolist() == [4, 6]
        assert res["rows"][row["order"]][4] == 0.0


@pytest.mark.parametrize("perturb,method", [(p, m) for p, ms in vr.PERTURBATIONS.items() for m in ms])
def test_perturbed_reference_misses(perturb, method):
    """Every deliberate mistake disagrees with the gate on the planted input: in a count or an error (exact results have no margin), the
    reversed sum in the row's bits alone."""
    preds, labels, ids = vr.planted(method)
    ref = vr.evaluate(preds, labels, ids, vr.PLANTED_CLASSES, method)
    bad = vr.evaluate(preds, labels, ids, vr.PLANTED_CLASSES, method, perturb=perturb)
    same_rows = np.array_equal(ref["rows"].view(np.uint32), bad["rows"].view(np.uint32))
    same_result = ref["result"] == bad["result"]
    print(perturb, method, "rows equal", same_rows, "result equal", same_result)
    if perturb == "reverse_order":
        row = ref["ids"].index("order")
        assert not same_rows and ref["rows"][row][4] == 0.0 and bad["rows"][row][4] == 1.0
        assert same_result                                           # detectable in the sum's bits only
    elif perturb == "max_from_neg_inf":
        assert not same_rows and not same_result and bad["result"]["correct1_verb"] == ref["result"]["correct1_verb"] - 1
    elif perturb == "divide_by_valid":
        assert same_rows and ref["result"]["correct1_verb"] == bad["result"]["correct1_verb"]
        assert ref["result"]["top1_verb_err"] != bad["result"]["top1_verb_err"] and ref["result"]["top1_noun_err"] == bad["result"]["top1_noun_err"]
    else:
        assert same_rows and not same_result
        if perturb == "higher_class_wins_ties":
            row = ref["ids"].index("tie")
            assert bad["rank"][row].tolist() == [0, 1] and bad["pred"][row].tolist() == [2, 5]
        else:
            assert bad["labels"][0].tolist() == [3, 2] and bad["rank"][0].min() > 0


def test_fp32_sum_depends_on_the_order_of_the_views():
    """Seeded 3 randn + 0.25 views: the arrival-order sum and the reversed one differ in some bits (so the GPU test's bit equality tests the
    order), and no partial sum is subnormal."""
    preds, labels, ids = vr.make_epoch((115, 478), [30, 2, 1, 30], seed=11)
    fwd, rev = vr.ensemble(preds, labels, ids, "sum"), vr.ensemble(preds, labels, ids, "sum", perturb="reverse_order")
    differ = fwd["rows"].view(np.uint32) != rev["rows"].view(np.uint32)
    row = {vid: i for i, vid in enumerate(fwd["ids"])}
    assert fwd["ids"] == rev["ids"] and fwd["views"][[row[v] for v in range(4)]].tolist() == [30, 2, 1, 30]
    assert differ[row[0]].any() and differ[row[3]].any() and not differ[row[2]].any()           # one view: nothing to reorder
    assert fwd["min_partial"] >= vr.FLT_MIN and rev["min_partial"] >= vr.FLT_MIN
    assert vr.slots_of(["b", "a", vr.DROP, "b", "c"]).tolist() == [0, 1, -1, 0, 2]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported(egx_lib):
    header = open(os.path.join(ROOT, "include", "egot2x.h")).read()
    assert "ABI v23 additions" in header
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert getattr(egx_lib, name) is not None
    assert egx_lib.egx_abi_version() == 18
    from egot2_amd import _lib
    assert all(name in _lib.SIGNATURES for name in SYMBOLS)


P = 0x1000          # a non-null address: every call below is refused before any device work


def _ints(v):
    return None if v is None else (C.c_int * max(len(v), 1))(*v)


def _update(lib, preds=P, ld=12, B=8, H=2, col0=(0, 5), Cs=(5, 7), labels=P, slots=P, slot_bytes=8, slot0=0, method=0, capacity=64, state=P):
    return lib.egx_view_ensemble_update(preds, ld, B, H, _ints(col0), _ints(Cs), labels, slots, slot_bytes, slot0, method, capacity, state, None)


def _topk(lib, n=8, capacity=64, H=2, Cs=(5, 7), ks=(1, 5), n_ks=None, state=P, rank=P, pred=P, result=P):
    return lib.egx_view_ensemble_topk(n, capacity, H, _ints(Cs), _ints(ks), len(ks) if n_ks is None else n_ks, state, rank, pred, result, None)


def _state(lib, capacity=64, H=2, Cs=(5, 7)):
    return 1 if lib.egx_view_ensemble_state(capacity, H, _ints(Cs), None) == 0 else 0          # 0 bytes is the refusal


REFUSALS = [
    (_update, dict(preds=None), "null pointer"),
    (_update, dict(labels=None), "null pointer"),
    (_update, dict(state=None), "null pointer"),
    (_update, dict(col0=None), "null pointer"),
    (_update, dict(Cs=None), "null pointer"),
    (_update, dict(capacity=0), "capacity >= 1"),
    (_update, dict(capacity=-4), "capacity >= 1"),
    (_update, dict(B=0), "1 <= B <= 65536"),
    (_update, dict(B=-3), "1 <= B <= 65536"),
    (_update, dict(B=65537), "1 <= B <= 65536"),
    (_update, dict(H=0), "1 <= H <= 4"),
    (_update, dict(H=5, col0=(0, 1, 2, 3, 4), Cs=(1, 1, 1, 1, 1)), "1 <= H <= 4"),
    (_update, dict(Cs=(5, 0)), "1 <= C <= 2048"),
    (_update, dict(Cs=(5, 2049), ld=4096), "1 <= C <= 2048"),
    (_update, dict(ld=0), "ld >= 1"),
    (_update, dict(ld=-12), "ld >= 1"),
    (_update, dict(ld=11), "of a row of ld=11"),
    (_update, dict(col0=(0, 4)), "overlap"),
    (_update, dict(col0=(-1, 5)), "of a row of ld=12"),
    (_update, dict(method=2), "0 = sum or 1 = max"),
    (_update, dict(method=-1), "0 = sum or 1 = max"),
    (_update, dict(slot_bytes=2), "4 = int32 or 8 = int64"),
    (_update, dict(slots=None, slot0=57), "slot0 + B <= capacity"),
    (_update, dict(slots=None, slot0=-1), "slot0 + B <= capacity"),
    (_update, dict(capacity=(1 << 31) // 12 + 1), "needs <= 2^31"),
    (_topk, dict(state=None), "null pointer"),
    (_topk, dict(rank=None), "null pointer"),
    (_topk, dict(pred=None), "null pointer"),
    (_topk, dict(result=None), "null pointer"),
    (_topk, dict(Cs=None), "null pointer"),
    (_topk, dict(ks=None, n_ks=2), "null pointer"),
    (_topk, dict(n=0), "1 <= n <= capacity"),
    (_topk, dict(n=-1), "1 <= n <= capacity"),
    (_topk, dict(n=65), "1 <= n <= capacity"),
    (_topk, dict(capacity=0), "capacity >= 1"),
    (_topk, dict(H=5, Cs=(1, 1, 1, 1, 1)), "1 <= H <= 4"),
    (_topk, dict(ks=(1, 2, 3, 4, 5)), "1 <= n_ks <= 4"),
    (_topk, dict(ks=(), n_ks=0), "1 <= n_ks <= 4"),
    (_topk, dict(ks=(1, 6)), "the narrowest head"),
    (_topk, dict(ks=(0, 5)), "the narrowest head"),
    (_topk, dict(capacity=(1 << 31) // 12 + 1), "needs <= 2^31"),
    (_state, dict(capacity=0), "capacity >= 1"),
    (_state, dict(H=0), "1 <= H <= 4"),
    (_state, dict(Cs=None), "null pointer"),
    (_state, dict(Cs=(5, 4096)), "1 <= C <= 2048"),
    (_state, dict(capacity=(1 << 31) // 12 + 1), "needs <= 2^31"),
]


@pytest.mark.parametrize("fn,kwargs,message", REFUSALS, ids=[f"{i}_{f.__name__}_{m.replace(' ', '_')}" for i, (f, _, m) in enumerate(REFUSALS)])
def test_host_refusals_before_any_device_work(egx_lib, fn, kwargs, message):
    egx_lib.egx_launch_count(1)
    assert fn(egx_lib, **kwargs) != 0
    assert message.encode() in egx_lib.egx_last_error(), egx_lib.egx_last_error()
    assert egx_lib.egx_launch_count(0) == 0


def test_state_size_query(egx_lib):
    offs = (C.c_size_t * 3)()
    cap, Cs = 100, (115, 478)
    nbytes = egx_lib.egx_view_ensemble_state(cap, 2, _ints(Cs), offs)
    labels, views, rows = offs
    assert labels == 256 and views == labels + 8 * cap * 2 and rows % 256 == 0 and rows >= views + 4 * cap
    assert nbytes == rows + 4 * cap * 593
    assert egx_lib.egx_view_ensemble_state((1 << 31) // 593, 2, _ints(Cs), None) > 0         # the largest state that is taken
    assert egx_lib.egx_view_ensemble_state((1 << 31) // 593 + 1, 2, _ints(Cs), None) == 0


def test_functional_refuses_cpu_tensors_and_bad_arguments(egx_lib):
    from egot2_amd import _lib, functional as F_egx
    state = torch.zeros(16, dtype=torch.uint8)
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.view_ensemble_update(state, 4, (5, 7), [torch.zeros(3, 5), torch.zeros(3, 7)], torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.view_ensemble_topk(state, 4, (5, 7), 3)
    with pytest.raises(ValueError, match="classes"):
        F_egx.view_ensemble_state(4, (5, 0), "cpu")
    with pytest.raises(ValueError, match="'sum' or 'max'"):
        F_egx.view_ensemble_update(state, 4, (5, 7), [torch.zeros(3, 5), torch.zeros(3, 7)], torch.zeros(3, 2, dtype=torch.int64), method="mean")
    assert F_egx.VIEW_ENS_METHODS == {"sum": 0, "max": 1} and F_egx.VIEW_ENS_COUNTS == ("n", "n_dropped", "n_nonfinite")
    flat = torch.arange(3 + 2 + 4, dtype=torch.int32)
    v = F_egx.view_ensemble_views(flat, 2, 2)
    assert v["n"].item() == 0 and v["n_nonfinite"].item() == 2 and v["n_invalid"].tolist() == [3, 4] and v["correct"].tolist() == [[5, 6], [7, 8]]
    heads = F_egx._clip_heads(list(torch.zeros(4, 12).split([5, 7], dim=1)))
    assert [tuple(h.shape) for h in heads] == [(4, 1, 5), (4, 1, 7)] and F_egx._seg_windows(heads)[1:] == (12, [0, 5])     # read in place


# ---- ViewEnsembleTest on the host -----------------------------------------------------------------------------------------------------------
def test_step_result_keys_and_arithmetic_from_the_result_words():
    from egot2_amd.train import ViewEnsembleTest
    ens = ViewEnsembleTest(64, (5, 7))
    with pytest.raises(RuntimeError, match="no forward"):
        ens.step_result()
    with pytest.raises(RuntimeError, match="no update"):
        ens.compute()
    b = ens._result_buffers(torch.device("cpu"))
    assert ens._result_buffers(torch.device("cpu")) is b and b["flat"].numel() == 9 and b["flat"].dtype == torch.int32
    assert b["rank"].shape == (64, 2) and b["pred"].dtype == torch.int32 and b["correct"].shape == (2, 2)
    b["flat"].copy_(torch.tensor([5, 1, 0, 1, 0, 2, 4, 5, 4], dtype=torch.int32))          # n, dropped, nonfinite, invalid[2], correct[2][2]
    ens._last = {"buffers": b, "result": {}}
    r = ens.step_result()
    assert set(r) == {"test_n", "test_n_dropped", "test_n_nonfinite", "test_n_invalid_verb", "test_n_invalid_noun", "test_correct1_verb",
                      "test_correct1_noun", "test_correct5_verb", "test_correct5_noun", "test_top1_verb_err", "test_top5_verb_err",
                      "test_top1_noun_err", "test_top5_noun_err"}
    want = vr.errors(np.asarray([[2, 4], [5, 4]]), 5)              # fp32, as topk_errors: (1 - 2/5) * 100 = 60.00000381...
    assert r["test_top1_verb_err"] == float(want[0, 0]) == float(np.float32(60.000004)) and r["test_top5_verb_err"] == 0.0
    assert r["test_top1_noun_err"] == float(want[0, 1]) and r["test_top5_noun_err"] == float(want[1, 1])
    assert (r["test_n"], r["test_n_dropped"], r["test_n_nonfinite"], r["test_n_invalid_verb"], r["test_correct5_noun"]) == (5, 1, 0, 1, 4)
    assert b["correct"][0, 1].item() == 4 and b["n_invalid"][0].item() == 1                 # the named views read the same words
    assert set(ens.step_result("")) == {k[len("test_"):] for k in r}                         # the reference's bare keys
    three = ViewEnsembleTest(8, (5, 7, 9), ks=(1,))
    b3 = three._result_buffers(torch.device("cpu"))
    b3["flat"].copy_(torch.tensor([4, 0, 0, 0, 0, 0, 1, 2, 4], dtype=torch.int32))
    three._last = {"buffers": b3, "result": {}}
    r3 = three.step_result("val")
    assert (r3["val_top1_0_err"], r3["val_top1_1_err"], r3["val_top1_2_err"]) == (75.0, 50.0, 0.0)
    for bad in (dict(capacity=0), dict(method="mean"), dict(ks=(1, 6)), dict(ks=()), dict(classes=(5, 0)), dict(classes=(1,) * 5),
                dict(capacity=(1 << 31) // 12 + 1)):
        with pytest.raises(ValueError):
            ViewEnsembleTest(**{"capacity": 8, "classes": (5, 7), **bad})


def test_id_map_capacity_and_update_refusals_on_the_host(monkeypatch):
    """clip ids -> dense slots in first-appearance order (the reference's dict order); more videos than capacity, both or neither of
    clip_ids / slots, device slots without rows=: raised before any device work (the functional layer is never reached, and a refused call
    leaves the map as it was)."""
    from egot2_amd import functional as F_egx
    from egot2_amd.train import ViewEnsembleTest
    sent = []
    monkeypatch.setattr(F_egx, "view_ensemble_update", lambda state, cap, classes, preds, labels, slots, **k: sent.append(slots.tolist()))
    monkeypatch.setattr(ViewEnsembleTest, "_result_buffers", lambda self, device, *dims: {"state": torch.zeros(4, dtype=torch.uint8)})
    x, y = [torch.zeros(5, 5), torch.zeros(5, 7)], torch.zeros(5, 2, dtype=torch.int64)
    ens = ViewEnsembleTest(4, (5, 7))
    ens.update(x, y, clip_ids=["b", "a", "b", "c", "a"])
    assert sent[-1] == [0, 1, 0, 2, 1] and ens._rows == 3 and ens.video_ids() == ["b", "a", "c"]
    ens.update(x, y, clip_ids=["c", "d", "d", "a", "b"])               # videos continue over calls
    assert sent[-1] == [2, 3, 3, 1, 0] and ens._rows == 4 and ens.video_ids() == ["b", "a", "c", "d"]
    with pytest.raises(ValueError, match="5 videos exceed capacity=4"):
        ens.update(x, y, clip_ids=["a", "b", "e", "c", "d"])
    assert ens._rows == 4 and ens.video_ids() == ["b", "a", "c", "d"] and len(sent) == 2
    with pytest.raises(ValueError, match="exactly one of clip_ids and slots"):
        ens.update(x, y)
    with pytest.raises(ValueError, match="exactly one of clip_ids and slots"):
        ens.update(x, y, clip_ids=list("abcda"), slots=[0, 1, 2, 3, 0])
    with pytest.raises(ValueError, match="4 ids / slots for 5 clips"):
        ens.update(x, y, clip_ids=list("abcd"))
    with pytest.raises(ValueError, match="cannot be mixed"):
        ens.update(x, y, slots=[0, 1, 2, 3, 0])
    ens.reset()
    assert ens._rows == 0 and ens.video_ids() == []
    ens.update(x, y, slots=[3, 0, 0, 1, 3])
    assert sent[-1] == [3, 0, 0, 1, 3] and ens._rows == 4 and ens.video_ids() == [0, 1, 2, 3]
    ens.update(x, y, slots=torch.tensor([1, 1, 1, 0, 2], dtype=torch.int32))
    assert ens._rows == 4
    with pytest.raises(ValueError, match="5 videos exceed capacity=4"):
        ens.update(x, y, slots=[0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match=">= 0"):
        ens.update(x, y, slots=[0, 1, -2, 3, 0])
    with pytest.raises(ValueError, match="cannot be mixed"):
        ens.update(x, y, clip_ids=list("abcda"))


def test_update_and_compute_refuse_a_capture(monkeypatch):
    """The id map and the video count are host state: inside a stream capture update, compute and reset raise (the real capture:
    test_gpu_view_ensemble.py)."""
    from egot2_amd.train import ViewEnsembleTest
    monkeypatch.setattr(ViewEnsembleTest, "_capturing", staticmethod(lambda device: True))
    ens = ViewEnsembleTest(8, (5, 7))
    with pytest.raises(RuntimeError, match="update cannot be captured in a graph: the id map and the video count are host state"):
        ens.update([torch.zeros(5, 5), torch.zeros(5, 7)], torch.zeros(5, 2, dtype=torch.int64), clip_ids=list("abcde"))
    ens._device, ens._rows = torch.device("cpu"), 5
    with pytest.raises(RuntimeError, match="compute cannot be captured"):
        ens.compute()
    with pytest.raises(RuntimeError, match="reset cannot be captured"):
        ens.reset()
