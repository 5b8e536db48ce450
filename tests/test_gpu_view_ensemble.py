"""-m gpu: the action-recognition test epoch on the device - egx_view_ensemble_update / egx_view_ensemble_topk against the gate
tests/view_ensemble_ref.py: the accumulator rows bit for bit (sum and max; the in-register and the looped head; views interleaved and
split over calls), run-to-run reproducibility, ranks / predictions / counts on the planted input, train.ViewEnsembleTest on the recorded
reference epochs and behind an AR translator's eval forward, and the capture refusal. Measured figures: tools/view_ensemble_eval.py,
profiles/view_ensemble_report.txt."""
import os

import numpy as np
import pytest
import torch

from tests import view_ensemble_ref as vr
from tests.util import seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "view_ensemble.npz")
ERR_KEYS = ("top1_verb_err", "top5_verb_err", "top1_noun_err", "top5_noun_err")
# 9 videos of 30 views, 10 of 2, 32 of 1: 322 clips = calls of B = 1, 64, 257
VIEWS = [30] * 9 + [2] * 10 + [1] * 32
CLASS_SETS = [(5, 7), (115, 478), (7, 600)]             # ld = 12; 593 (odd: unaligned rows); a head beyond 512 (the looped segment)
CUTS = [(1, 65), (100, 200)]


def _device_epoch(cuda, preds, labels, ids, classes, method, cuts=(), capacity=None, in_place=True, slot_dtype=torch.int64, drop_slot=-1, ks=vr.KS):
    """update() over the clips cut at `cuts`, then the top-k launch, through the functional layer with every output prefilled -> dict of
    host arrays. in_place: the heads are column windows of one (N, ld) stack (read where they are), else separate tensors (one torch.cat)."""
    from egot2_amd import functional as F_egx
    slots = vr.slots_of(ids)
    n = int(slots.max()) + 1
    capacity = capacity or n
    slots = np.where(slots < 0, drop_slot, slots)
    state = F_egx.view_ensemble_state(capacity, classes, cuda)
    x, y = torch.from_numpy(preds).to(cuda), torch.from_numpy(labels).to(cuda)
    s = torch.from_numpy(slots).to(device=cuda, dtype=slot_dtype)
    edges = [0, *cuts, len(ids)]
    for a, b in zip(edges[:-1], edges[1:]):
        heads = list(x[a:b].split(list(classes), dim=1))
        if not in_place:
            heads = [h.clone() for h in heads]
        F_egx.view_ensemble_update(state, capacity, classes, heads, y[a:b], s[a:b], method=method)
    H = len(classes)
    out = {"flat": torch.full((3 + H + len(ks) * H,), -7, dtype=torch.int32, device=cuda),
           "rank": torch.full((n, H), -9, dtype=torch.int32, device=cuda), "pred": torch.full((n, H), -9, dtype=torch.int32, device=cuda)}
    res = F_egx.view_ensemble_topk(state, capacity, classes, n, ks, out=out)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in res.items()}
    host.update({k: v[:n].cpu().numpy() for k, v in F_egx.view_ensemble_rows(state, capacity, classes).items()})
    host["state"] = state.cpu().numpy()
    return host


def _check_against_gate(got, ref, tag):
    """Rows bit for bit, labels, view counts, rank, pred and every count exactly."""
    assert got["rows"].dtype == np.float32 and got["rows"].shape == ref["rows"].shape, tag
    differ = got["rows"].view(np.uint32) != ref["rows"].view(np.uint32)
    print(tag, "rows", ref["rows"].shape, "words that differ", int(differ.sum()))
    assert not differ.any(), (tag, np.argwhere(differ)[:5])
    assert np.array_equal(got["labels"], ref["labels"]) and np.array_equal(got["views"], ref["views"]), tag
    assert np.array_equal(got["rank"], ref["rank"]), (tag, got["rank"], ref["rank"])
    assert np.array_equal(got["pred"], ref["pred"]), (tag, got["pred"], ref["pred"])
    counts = (int(got["n"]), int(got["n_dropped"]), int(got["n_nonfinite"]), got["n_invalid"].tolist(), got["correct"].tolist())
    assert counts == (ref["n"], ref["n_dropped"], ref["n_nonfinite"], ref["n_invalid"].tolist(), ref["correct"].tolist()), (tag, counts)


@pytest.fixture(scope="module")
def epochs():
    """The seeded epochs and the gate's results, computed once per (classes, method) and left unchanged."""
    out = {}
    for ci, classes in enumerate(CLASS_SETS):
        preds, labels, ids = vr.make_epoch(classes, VIEWS, seed=300 + ci)
        for method in ("sum", "max"):
            ref = vr.evaluate(preds, labels, ids, classes, method)
            assert ref["min_partial"] >= vr.FLT_MIN                    # no partial sum is subnormal
            out[classes, method] = (preds, labels, ids, ref)
    return out


# ---- 1. the accumulator, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", CUTS, ids=["B1_64_257", "B100_100_122"])
@pytest.mark.parametrize("method", ("sum", "max"))
@pytest.mark.parametrize("classes", CLASS_SETS, ids=["c5_7", "c115_478", "c7_600"])
def test_accumulator_rows_are_the_arrival_order_fold_bit_for_bit(egx_lib, cuda, epochs, classes, method, cuts):
    preds, labels, ids, ref = epochs[classes, method]
    edges = [0, *cuts, len(ids)]
    call_of = np.searchsorted(edges, np.arange(len(ids)), side="right")
    spans = {v: len(set(call_of[[i for i, w in enumerate(ids) if w == v]])) for v in set(ids)}
    assert sorted(set(ref["views"].tolist())) == [1, 2, 30] and (np.diff(vr.slots_of(ids)) < 0).any()           # 1, 2 and 30 views, interleaved
    if cuts == CUTS[1]:
        assert 2 in spans.values() and 3 in spans.values()           # videos split over two and over three calls
    in_place = cuts == CUTS[0]
    got = _device_epoch(cuda, preds, labels, ids, classes, method, cuts, in_place=in_place,
                        slot_dtype=torch.int32 if method == "max" else torch.int64)
    _check_against_gate(got, ref, f"{classes} {method} cuts={cuts}")


# ---- 2. run to run ----------------------------------------------------------------------------------------------------------------------------
def test_an_epoch_run_twice_after_reset_gives_identical_state_and_results(egx_lib, cuda, epochs):
    from egot2_amd.train import ViewEnsembleTest
    classes = (115, 478)
    preds, labels, ids, ref = epochs[classes, "sum"]
    ens = ViewEnsembleTest(64, classes)
    x, y = torch.from_numpy(preds).to(cuda), torch.from_numpy(labels).to(cuda)
    runs = []
    for _ in range(2):
        ens.reset()
        for a, b in ((0, 130), (130, 322)):
            ens.update(list(x[a:b].split(list(classes), dim=1)), y[a:b], clip_ids=[f"v{i}" for i in ids[a:b]])
        r = ens.step_result()
        st = ens.stats()
        runs.append((ens._result_buffers(cuda)["state"].cpu().numpy().copy(), st["rank"].cpu().numpy().copy(), st["pred"].cpu().numpy().copy(), r))
    (s0, r0, p0, d0), (s1, r1, p1, d1) = runs
    assert np.array_equal(s0, s1) and np.array_equal(r0, r1) and np.array_equal(p0, p1) and d0 == d1
    assert np.array_equal(r0, ref["rank"]) and d0["test_n"] == 51 and ens.video_ids() == [f"v{i}" for i in ref["ids"]]
    assert not s0[:256].any()                                        # the arrival counter left itself zero, nothing was dropped


# ---- 3. rank, pred and counts on the planted input ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop_slot", (-1, 7, 1 << 40))
@pytest.mark.parametrize("method", ("sum", "max"))
def test_planted_ties_labels_nan_and_dropped_slots(egx_lib, cuda, method, drop_slot):
    """Ties at the label with a lower and a higher class, a label outside [0, C), a NaN row, an all-negative video under "max" (a row of
    zeros: rank = the label's index), n = capacity, a dropped slot (negative, = capacity, beyond int32), differing labels among a video's
    views: everything equal to the gate exactly."""
    preds, labels, ids = vr.planted(method)
    ref = vr.evaluate(preds, labels, ids, vr.PLANTED_CLASSES, method)
    got = _device_epoch(cuda, preds, labels, ids, vr.PLANTED_CLASSES, method, cuts=(5,), capacity=7, drop_slot=drop_slot, in_place=False)
    assert ref["n"] == 7 and ref["n_dropped"] == 1 and ref["n_nonfinite"] == 1 and ref["n_invalid"].tolist() == [1, 0]
    _check_against_gate(got, ref, f"planted {method} drop={drop_slot}")
    row = ref["ids"].index("negative")
    if method == "max":
        assert not got["rows"][row].any() and got["rank"][row].tolist() == [0, 0]
    for perturb, methods in vr.PERTURBATIONS.items():                # the device is told apart from every perturbed reference
        if method in methods:
            bad = vr.evaluate(preds, labels, ids, vr.PLANTED_CLASSES, method, perturb=perturb)
            same = (np.array_equal(got["rows"].view(np.uint32), bad["rows"].view(np.uint32)) and np.array_equal(got["rank"], bad["rank"])
                    and np.array_equal(got["labels"], bad["labels"]) and perturb != "divide_by_valid")
            assert not same, perturb


def test_slot0_rows_and_three_heads(egx_lib, cuda):
    """Without slots clip i is video slot0 + i; three heads, ks = (1, 2, 3); a second call folds onto the same videos."""
    from egot2_amd import functional as F_egx
    classes, ks = (3, 70, 130), (1, 2, 3)
    preds, labels, ids = vr.make_epoch(classes, [2] * 9, seed=77, interleave=False)
    ids = list(range(9)) * 2                                         # call 1: videos 0 .. 8, call 2: again
    ref = vr.evaluate(preds, labels, ids, classes, "sum", ks)
    state = F_egx.view_ensemble_state(12, classes, cuda)
    x, y = torch.from_numpy(preds).to(cuda), torch.from_numpy(labels).to(cuda)
    for a, slot0 in ((0, 0), (9, 0)):
        F_egx.view_ensemble_update(state, 12, classes, list(x[a:a + 9].split(list(classes), dim=1)), y[a:a + 9], None, slot0=slot0)
    res = F_egx.view_ensemble_topk(state, 12, classes, 9, ks)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    got.update({k: v[:9].cpu().numpy() for k, v in F_egx.view_ensemble_rows(state, 12, classes).items()})
    _check_against_gate(got, ref, "slot0, three heads")


def test_device_slots_with_rows_through_the_class(egx_lib, cuda):
    """ViewEnsembleTest.update(slots=<device tensor>, rows=): int64 and int32 slots, a slot beyond capacity dropped on the device and
    counted, n = capacity; ranks, predictions, counts and errors equal to the gate."""
    from egot2_amd.train import ViewEnsembleTest
    classes = (5, 7)
    preds, labels, ids = vr.make_epoch(classes, [3, 1, 2, 4, 1], seed=5)
    ids = [vr.DROP if v == 4 else v for v in ids]                     # the one clip of video 4 goes to a slot outside the accumulator
    ref = vr.evaluate(preds, labels, ids, classes, "max")
    slots = vr.slots_of(ids)
    rows_after = [int(slots[:5].max()) + 1, 4]
    slots = np.where(slots < 0, 99, slots)
    x, y, s = torch.from_numpy(preds).to(cuda), torch.from_numpy(labels).to(cuda), torch.from_numpy(slots).to(cuda)
    ens = ViewEnsembleTest(4, classes, method="max")
    ens.update(list(x[:5].split(list(classes), dim=1)), y[:5], slots=s[:5], rows=rows_after[0])
    ens.update(list(x[5:].split(list(classes), dim=1)), y[5:], slots=s[5:].to(torch.int32), rows=rows_after[1])
    r = ens.step_result()
    st = ens.stats()
    assert ref["n"] == 4 and ref["n_dropped"] == 1 and (r["test_n"], r["test_n_dropped"], r["test_n_nonfinite"]) == (4, 1, 0)
    assert np.array_equal(st["rank"].cpu().numpy(), ref["rank"]) and np.array_equal(st["pred"].cpu().numpy(), ref["pred"])
    assert st["correct"].cpu().numpy().tolist() == ref["correct"].tolist() and ens.video_ids() == [0, 1, 2, 3]
    assert {k: r[f"test_{k}"] for k in ERR_KEYS} == {k: ref["result"][k] for k in ERR_KEYS}


# ---- 4. the recorded reference epochs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("sum", "max"))
@pytest.mark.parametrize("case", ("a", "b"))
def test_recorded_reference_epoch_through_step_result(egx_lib, cuda, case, method):
    """train.ViewEnsembleTest on the inputs of the REAL test_epoch_end (tests/golden/make_golden_viewens.py), fed in batches of 8 with the
    loader's clip-id strings: the four errors equal the recorded ones exactly, the rows bit for bit."""
    from egot2_amd.train import ViewEnsembleTest
    z = np.load(GOLDEN)
    g = lambda k: z[f"{case}_{k}"]  # noqa: E731
    classes = tuple(int(c) for c in g("classes"))
    x, y = torch.from_numpy(g("preds")).to(cuda), torch.from_numpy(g("labels")).to(cuda)
    clip_ids = [f"clip{int(v):03d}" for v in g("clip_ids")]
    ens = ViewEnsembleTest(8, classes, method=method).reset()
    for a in range(0, len(clip_ids), 8):
        verb, noun = x[a:a + 8].split(list(classes), dim=1)
        ens.update([verb.contiguous(), noun.contiguous()], y[a:a + 8], clip_ids=clip_ids[a:a + 8])
    r = ens.step_result(prefix="")
    want = dict(zip(ERR_KEYS, g(f"{method}_err").tolist()))
    print(case, method, {k: r[k] for k in ERR_KEYS}, want)
    assert {k: r[k] for k in ERR_KEYS} == want
    n = g(f"{method}_rows").shape[0]
    from egot2_amd import functional as F_egx
    rows = F_egx.view_ensemble_rows(ens._result_buffers(cuda)["state"], 8, classes)
    assert np.array_equal(rows["rows"][:n].cpu().numpy().view(np.uint32), g(f"{method}_rows").view(np.uint32))
    assert np.array_equal(rows["labels"][:n].cpu().numpy(), g(f"{method}_video_labels"))
    pred, rank, vids = ens.predictions()
    assert vids == list(dict.fromkeys(clip_ids)) and pred.shape == (n, 2) and (r["n"], r["n_dropped"], r["n_nonfinite"]) == (n, 0, 0)
    assert int((rank[:, 0] == 0).sum()) == r["correct1_verb"] and int((rank[:, 1] < 5).sum()) == r["correct5_noun"]


# ---- 5. the model path ---------------------------------------------------------------------------------------------------------------------
def test_ar_translator_eval_forward_feeds_the_accumulator(egx_lib, cuda):
    """hoi_ar.TaskFusionMFTransformer2TaskAR in eval mode: 3 videos x 4 views through forward_features in two batches into ViewEnsembleTest,
    against the gate on the logits the model returned."""
    from egot2_amd.train import ViewEnsembleTest
    from tests.test_oracle_golden import build_ours
    c = dict(kind="ar2", L=1, d=128, h=4, n=2, classes=[11, 70])
    model = build_ours(c)
    model.load_state_dict(seeded_state_dict(model, seed=912))
    model = model.to(cuda).eval()
    clip_ids = ["v1", "v0", "v2", "v0", "v1", "v1", "v2", "v0", "v2", "v2", "v0", "v1"]
    labels = torch.tensor([[3, 10], [1, 60], [9, 5], [1, 60], [3, 10], [3, 10], [9, 5], [1, 60], [9, 5], [9, 5], [1, 61], [3, 10]])
    feats = [f.to(cuda) for f in seeded_feats(94, [(12, 8, 2048), (12, 8, 256), (12, 2, 2048)])]
    ens = ViewEnsembleTest(16, (11, 70)).reset()
    logits = []
    with torch.no_grad():
        for a, b in ((0, 5), (5, 12)):
            out = model.forward_features(*[f[a:b] for f in feats])
            assert [tuple(o.shape) for o in out] == [(b - a, 11), (b - a, 70)]
            ens.update(out, labels[a:b].to(cuda), clip_ids=clip_ids[a:b])
            logits.append(torch.cat(out, dim=1).cpu().numpy())
    r = ens.step_result()
    ref = vr.evaluate(np.concatenate(logits), labels.numpy(), clip_ids, (11, 70), "sum")
    st = ens.stats()
    from egot2_amd import functional as F_egx
    rows = F_egx.view_ensemble_rows(ens._result_buffers(cuda)["state"], 16, (11, 70))
    got = {k: v.cpu().numpy() for k, v in st.items()}
    got.update({k: v[:3].cpu().numpy() for k, v in rows.items()})
    _check_against_gate(got, ref, "ar2 model")
    assert ens.video_ids() == ["v1", "v0", "v2"] and ref["labels"][1].tolist() == [1, 61] and ref["views"].tolist() == [4, 4, 4]
    assert {k: r[f"test_{k}"] for k in ERR_KEYS} == {k: ref["result"][k] for k in ERR_KEYS}


# ---- 6. capture refusal ----------------------------------------------------------------------------------------------------------------------
def test_capture_is_refused_and_capacity_holds(egx_lib, cuda):
    from egot2_amd.train import ViewEnsembleTest
    ens = ViewEnsembleTest(4, (5, 7))
    x = [torch.randn(6, 5, device=cuda), torch.randn(6, 7, device=cuda)]
    y = torch.zeros(6, 2, dtype=torch.int64, device=cuda)
    ens.update(x, y, clip_ids=list("abcabc"))
    with pytest.raises(ValueError, match="6 videos exceed capacity=4"):
        ens.update(x, y, clip_ids=list("abcdef"))
    with pytest.raises(ValueError, match="need rows="):
        ens.update(x, y, slots=torch.zeros(6, dtype=torch.int64, device=cuda))
    doubled = torch.zeros_like(x[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        with pytest.raises(RuntimeError, match="update cannot be captured in a graph"):
            ens.update(x, y, clip_ids=list("abcabc"))
        with pytest.raises(RuntimeError, match="compute cannot be captured in a graph"):
            ens.compute()
        torch.mul(x[0], 2.0, out=doubled)                            # the capture itself goes on
    torch.cuda.synchronize()
    r = ens.step_result()
    assert r["test_n"] == 3 and ens.stats()["rank"].shape == (3, 2)
