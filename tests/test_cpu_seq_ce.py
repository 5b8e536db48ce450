"""CPU suite of the EgoT2-g multi-task criterion (egx_sequence_ce, functional.sequence_cross_entropy, train.TranslationCriterion): the gate
tests/seq_ce_ref.py against the recording of the reference's own nn.CrossEntropyLoss and metric classes, its bars, its perturbed references,
the host refusals of the C entry point, the vocabulary maps and the arithmetic of step_result."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import seq_ce_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "live", "g_criterion.npz")
N = len(sr.CASES)


@pytest.fixture(scope="module")
def evals():
    """case index -> (fp64 reference, fp32 evaluation), computed once."""
    return {i: (sr.evaluate(i, sr.F64), sr.evaluate(i, torch.float32)) for i in range(N)}


def golden_tasks(z, name, T, with_metrics):
    """The recorded case as the gate's task list: the (sy, B, V) decoder output as canonical (B, sy, V) rows, target[:, 1:], and - hoi -
    the metric objects' own maps with the labels scored at position 0."""
    tasks = []
    for t in range(T):
        logits = torch.from_numpy(z[f"{name}_logits{t}"]).permute(1, 0, 2).contiguous()
        target = torch.from_numpy(z[f"{name}_target{t}"])[:, 1:]
        wl = labels = None
        if with_metrics:
            wl = torch.from_numpy(z[f"{name}_wl{t}"])
            labels = torch.full(tuple(target.shape), -1, dtype=torch.int64)
            labels[:, 0] = torch.from_numpy(z[f"{name}_labels{t}"])
        tasks.append(dict(logits=logits, target=target, ratio=float(z[f"{name}_ratios"][t]), word_label=wl, labels=labels))
    return tasks


def pnr_dist_from_pred(pred, z):
    """PNRMetric.dist of the recorded clips from the launch's `pred`: the restricted argmax IS the keyframe index (metrics.py:179-186)."""
    start, end, pnr, fps = (z[f"hoi_{k}"] for k in ("start", "end", "pnr", "fps"))
    d = [abs(float(end[b] - start[b]) / 16 * int(pred[b, 0, 1]) - float(pnr[b] - start[b])) / float(fps[b]) for b in range(len(fps))]
    return [float(torch.Tensor([x]).item()) for x in d]                 # the reference keeps each distance as an fp32 tensor


def check_against_recording(res, z, name):
    """loss and terms within `tol` are the caller's; here: the metric classes' compute() from the counts, exactly."""
    scored, invalid, correct, restricted = (res[k].tolist() for k in ("scored", "invalid", "correct", "correct_restricted"))
    assert [invalid[0] / scored[0], float(scored[0])] == [z["hoi_pnrmetric"][0], z["hoi_pnrmetric"][2]]
    dist = pnr_dist_from_pred(res["pred"][0], z)
    assert sum(dist) / len(dist) == pytest.approx(float(z["hoi_pnrmetric"][1]), rel=1e-12)
    assert [invalid[1] / scored[1], restricted[1] / scored[1], float(scored[1])] == z["hoi_osccmetric"].tolist()
    f32 = lambda a, b: float(torch.tensor(a).float() / b)  # noqa: E731  (ARMetric.compute divides fp32 tensors)
    assert [f32(invalid[2], scored[2]), f32(invalid[3], scored[3]), f32(correct[2], scored[2]), f32(correct[3], scored[3])] == z["hoi_armetric"].tolist()
    assert [invalid[4] / scored[4], correct[4] / scored[4], invalid[5] / scored[5], correct[5] / scored[5], float(scored[4])] == z["hoi_ltametric"].tolist()


# ---- the gate against the recorded reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T", [("hhi", 3), ("hoi", 6)])
def test_gate_reproduces_the_recorded_reference_step(name, T):
    """The gate in fp64 against the REAL nn.CrossEntropyLoss on (B, V, sy) and - hoi - ARMetric, LTAMetric, OSCCMetric and PNRMetric as
    tests/golden/make_golden_gcrit.py recorded them: losses to 1e-12 relative, metrics exactly."""
    z = np.load(GOLDEN)
    V = z[f"{name}_logits0"].shape[2]
    res = sr.sequence_ce(golden_tasks(z, name, T, name == "hoi"), V, sr.F64)
    assert np.allclose(res["loss_terms"].numpy(), z[f"{name}_loss_terms"], rtol=1e-12, atol=0)
    assert abs(res["loss"].item() - float(z[f"{name}_loss"])) <= 1e-12 * abs(float(z[f"{name}_loss"]))
    if name == "hoi":
        check_against_recording(res, z, name)
        assert 0 < int(res["invalid"].sum()) < int(res["scored"].sum()) and 0 < int(res["correct"].sum())      # no degenerate recording


def test_inputs_carry_the_planted_cases(evals):
    assert len(set(sr.CASE_IDS)) == N
    i = sr.CASE_IDS.index("hhi")
    a, ref = sr.seq_inputs(i), evals[i][0]
    k = a[2]                                                    # B = 45, V = 7
    assert k["logits"].dtype == torch.float32 and k["target"].dtype == torch.int64 and k["word_label"].dtype == torch.int32
    assert k["logits"][0, 0, 0] == 80 and k["logits"][0, 0, 6] == -80 and (k["logits"][1, 0] == 0.75).all()
    assert k["logits"][2, 0, 2] == k["logits"][2, 0, 3] == 20 and k["target"][2, 0] == 3                     # the lower word wins: wrong
    assert (k["target"][3] == torch.tensor([-100, 7])).all() and k["target"][4, 0] == -100 and k["target"][4, 1] == 7
    assert ref["n_valid"][2] == 45 * 2 - 2 - 2 and 0 < ref["seq_correct"][2] < 45 and ref["token_correct"][2] > ref["seq_correct"][2]
    assert torch.isfinite(ref["d_logits"][2]).all() and (ref["d_logits"][2][3] == 0).all() and (ref["d_logits"][2][0] != 0).any()
    assert 0 < ref["invalid"][2] and 0 < ref["correct"][2] < ref["scored"][2] == 45
    assert (ref["correct"] != ref["correct_restricted"]).any()                                                # free and restricted differ
    lim, lref = sr.seq_inputs(sr.CASE_IDS.index("limits")), evals[sr.CASE_IDS.index("limits")][0]
    assert len(lim) == 8 and lim[0]["logits"].shape[1] == 64 and lim[2]["ratio"] == 0.0
    assert (lref["d_logits"][2] == 0).all() and lref["loss_terms"][2] > 0                                     # ratio 0: exact zeros
    assert lref["n_valid"][3] == 0 and lref["loss_terms"][3] == 0 and (lref["d_logits"][3] == 0).all()        # no valid label
    assert lref["scored"][0] == 2 * 64 - 1
    mo = evals[sr.CASE_IDS.index("metrics_only")][0]
    assert mo["loss"] == 0 and (mo["n_valid"] == 0).all() and mo["scored"].tolist() == [17, 5] and mo["seq_correct"].tolist() == [0, 0]
    assert math.isfinite(evals[sr.CASE_IDS.index("hoi")][0]["loss"].item())


def test_fp32_reference_meets_the_bar(evals):
    """The fp32 evaluation of the gate passes its own bars, matches every count, and the recorded FP32_ERR constants are what it measures."""
    worst = {k: 0.0 for k in sr.KINDS}
    for i, (ref, f32) in evals.items():
        assert sr.same_counts(f32, ref), sr.CASE_IDS[i]
        for k, e in sr.bar_errors(f32, ref).items():
            worst[k] = max(worst[k], e)
            assert e <= sr.BAR[k], (sr.CASE_IDS[i], k, e)
    print("FP32_ERR measured:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k in sr.KINDS:
        assert sr.FP32_ERR[k] / 3 <= worst[k] <= sr.FP32_ERR[k] * 3, (k, worst[k], sr.FP32_ERR[k])
    assert sr.FACTOR == 8.0


@pytest.mark.parametrize("perturb", sr.PERTURBATIONS)
def test_perturbed_reference_is_rejected(evals, perturb):
    """Every deliberate mistake misses a bar by >= 3x, or changes an exact count, on every case where it changes anything; and it changes
    something."""
    ratios, count_hits = [], 0
    for i, (ref, _) in evals.items():
        bad = sr.evaluate(i, sr.F64, perturb)
        ratio = max(e / sr.BAR[k] for k, e in sr.bar_errors(bad, ref).items())
        if not sr.same_counts(bad, ref):
            count_hits += 1
        elif ratio > 1e-6:          # below: the fp64 rounding of another summation order (mean per position = mean per task where every
            ratios.append(ratio)    # position has as many valid labels), no change
    print(perturb, "min ratio", min(ratios) if ratios else None, "cases with a changed count", count_hits)
    assert ratios or count_hits
    assert all(r >= 3 for r in ratios), (perturb, min(ratios))
    want = sr.PERTURB_RATIO[perturb]
    if want == "counts":
        assert count_hits > 0 and not ratios
    else:
        assert ratios and want / 3 <= min(ratios) <= want * 3, (perturb, min(ratios), want)


# ---- host refusals of egx_sequence_ce --------------------------------------------------------------------------------------------------------
P = 0x1000          # a non-null address: every call below is refused before any device work


def _call(lib, n_tasks=1, T=None, V=7, result=P, scratch=P, tasks_null=False, **fields):
    from egot2_amd._lib import SeqTask
    arr = (SeqTask * max(n_tasks, 1))()
    for k in arr:
        k.logits, k.stride_b, k.stride_s, k.B, k.sy, k.target, k.target_stride_b, k.target_stride_s, k.ratio = P, 14, 7, 5, 2, P, 3, 1, 1.0
    for name, v in fields.items():
        setattr(arr[n_tasks - 1], name, v)
    return lib.egx_sequence_ce(None if tasks_null else arr, n_tasks if T is None else T, V, result, scratch, None)


REFUSALS = [
    (dict(tasks_null=True), "null pointer"),
    (dict(result=None), "null pointer"),
    (dict(scratch=None), "null pointer"),
    (dict(logits=None), "null pointer"),
    (dict(n_tasks=3, target=None), "target of task 2"),
    (dict(T=0), "1 <= T <= 8"),
    (dict(T=9), "1 <= T <= 8"),
    (dict(V=1), "2 <= V <= 2048"),
    (dict(V=2049), "2 <= V <= 2048"),
    (dict(B=0), "B >= 1"),
    (dict(sy=0), "1 <= sy <= 64"),
    (dict(sy=65), "1 <= sy <= 64"),
    (dict(B=2 ** 21 + 1, sy=2), "B * sy <= 4194304"),
    (dict(stride_b=-1), "negative stride"),
    (dict(target_stride_s=-1), "negative stride"),
    (dict(d_logits=P, stride_s=6), "overlapping rows"),
    (dict(d_logits=P, stride_b=0), "overlapping rows"),
    (dict(labels=P), "labels without word_label"),
    (dict(word_label=P), "word_label without labels"),
    (dict(pred=P), "pred without word_label"),
]


@pytest.mark.parametrize("kwargs,message", REFUSALS, ids=[f"{i}_{m.replace(' ', '_')}" for i, (_, m) in enumerate(REFUSALS)])
def test_host_refusals_before_any_device_work(egx_lib, kwargs, message):
    egx_lib.egx_launch_count(1)
    assert _call(egx_lib, **kwargs) != 0
    assert message.encode() in egx_lib.egx_last_error(), egx_lib.egx_last_error()
    assert egx_lib.egx_launch_count(0) == 0


def test_scratch_query(egx_lib):
    """Nine 64-byte counters and 8 tasks x 256 chunks x 8 words of partials: one layout for every T and shape."""
    assert egx_lib.egx_sequence_ce_scratch() == 9 * 64 + 8 * 256 * 8 * 4


def test_functional_refuses_cpu_tensors_and_bad_arguments(egx_lib):
    from egot2_amd import _lib, functional as F_egx
    with pytest.raises(_lib.EgxError, match="no CPU fallback"):
        F_egx.sequence_cross_entropy([torch.zeros(2, 7, 2)], [torch.zeros(2, 2, dtype=torch.int64)], [1.0])
    with pytest.raises(ValueError, match="1 to 8 tasks"):
        F_egx.sequence_cross_entropy([], [], [])
    assert C.sizeof(_lib.SeqTask) == 112 and F_egx.SEQ_CE_STATS[0] == "loss_terms" and len(F_egx.SEQ_CE_STATS) == 8


# ---- the vocabulary maps ---------------------------------------------------------------------------------------------------------------------
def test_word_label_maps():
    from egot2_amd.train import binary_word_labels, oscc_word_labels, pnr_word_labels, word_label_map
    vocab = {"<pad>": 0, "True": 1, "0": 2, "False": 3, "1": 4, "take": 5, "put": 6}
    vocab.update({str(i): 5 + i for i in range(2, 16)})
    V = 21
    assert binary_word_labels(vocab, V).tolist() == [-1, -1, 0, -1, 1] + [-1] * 16
    assert oscc_word_labels(vocab, V).tolist() == [-1, 1, -1, 0] + [-1] * 17
    p = pnr_word_labels(vocab, V)
    assert p.dtype == torch.int32 and p[2] == 0 and p[4] == 1 and p[7] == 2 and p[20] == 15 and int((p >= 0).sum()) == 16
    # one word serves two labels: the later label overrides the earlier, as _map_vocab_to_orig_idx does
    m = word_label_map(vocab, {0: "take", 1: "put", 2: "take"}, V)
    assert m[5] == 2 and m[6] == 1 and int((m >= 0).sum()) == 2

    class Indexable:            # anything indexable by word, with a length
        def __getitem__(self, w):
            return vocab[w]

        def __len__(self):
            return V
    assert torch.equal(oscc_word_labels(Indexable()), oscc_word_labels(vocab, V))
    with pytest.raises(ValueError, match="outside the vocabulary"):
        oscc_word_labels(vocab, 3)


# ---- TranslationCriterion.step_result ---------------------------------------------------------------------------------------------------------
def test_step_result_arithmetic_and_key_names():
    """The packed result buffer on CPU stand-in tensors: the reference's log names (HOI/tasks/multitask/video_task.py:570-576, :730-736;
    HHI/tasks/multitask/video_tasktranslation.py:62-65) and the metric ratios."""
    from egot2_amd.train import TranslationCriterion
    crit = TranslationCriterion((1.0, 1.0, 0.5), word_labels=[None, [0, -1, 1], [-1, 0, 1]])
    assert crit.names == ("lam", "ttm", "asd")
    with pytest.raises(RuntimeError, match="no forward"):
        crit.step_result()
    b = crit._result_buffers(torch.device("cpu"), 3)
    assert crit._result_buffers(torch.device("cpu"), 3) is b and b["flat"].numel() == 25 and b["flat"].dtype == torch.int32
    b["loss"].fill_(2.25)
    b["loss_terms"].copy_(torch.tensor([1.0, 0.5, 1.5]))
    for name, vals in (("n_valid", (10, 8, 0)), ("token_correct", (5, 2, 0)), ("seq_correct", (2, 1, 0)), ("scored", (0, 4, 0)),
                       ("invalid", (0, 1, 0)), ("correct", (0, 2, 0)), ("correct_restricted", (0, 3, 0))):
        b[name].copy_(torch.tensor(vals, dtype=torch.int32))
    b["rows"] = (5, 4, 6)
    crit._last = b
    r = crit.step_result()
    assert r["train_loss"] == 2.25 and [r["train_loss_lam"], r["train_loss_ttm"], r["train_loss_asd"]] == [1.0, 0.5, 1.5]
    assert r["train_lam_token_acc"] == 0.5 and r["train_lam_seq_acc"] == 2 / 5 and "train_lam_acc" not in r
    assert [r["train_ttm_acc"], r["train_ttm_err"], r["train_ttm_acc_restricted"]] == [0.5, 0.25, 0.75]
    assert r["train_ttm_token_acc"] == 0.25 and r["train_ttm_seq_acc"] == 0.25
    assert all(math.isnan(r[f"train_asd_{k}"]) for k in ("acc", "err", "acc_restricted", "token_acc")) and r["train_asd_seq_acc"] == 0.0
    assert set(crit.step_result("val")) == {k.replace("train_", "val_", 1) for k in r}
    h = crit.host_result()
    assert h["loss"] == 2.25 and h["scored"].tolist() == [0, 4, 0] and h["loss_terms"].dtype == np.float32
    six = TranslationCriterion([1.0] * 6)
    assert six.names == ("pnr", "oscc", "ac_verb", "ac_noun", "lta_verb", "lta_noun")
    assert TranslationCriterion([1.0, 2.0]).names == ("task0", "task1") and TranslationCriterion([1.0], names=["x"]).names == ("x",)
    for bad in ([], [1.0] * 9):
        with pytest.raises(ValueError, match="tasks"):
            TranslationCriterion(bad)
    with pytest.raises(ValueError, match="distinct names"):
        TranslationCriterion([1.0, 1.0], names=["a", "a"])
    with pytest.raises(ValueError, match="word_labels"):
        TranslationCriterion([1.0, 1.0], word_labels=[None])


def test_buffers_are_not_created_inside_a_capture(monkeypatch):
    """A buffer created inside a capture would live in that graph's private pool: refused, with the message the other criteria use."""
    from egot2_amd.train import TranslationCriterion
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    crit = TranslationCriterion([1.0, 1.0, 0.5], word_labels=[None, None, [0, 1]])
    with pytest.raises(RuntimeError, match="run one eager step at this problem size before capturing it in a graph"):
        crit._result_buffers(torch.device("cuda", 0), 3)
    with pytest.raises(RuntimeError, match="run one eager step at this problem size before capturing it in a graph"):
        crit._device_maps(torch.device("cuda", 0))
