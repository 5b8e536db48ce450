"""fp64 reference of egx_segment_scores_update / egx_segment_ap (include/egot2x.h), its cases, inputs and bars: the gate of
test_gpu_segment_ap.py. The literal loops of the reference's validation epoch in fp64 numpy:

    merge_output                  PostProcessor._merge_output (HHI/utils/ttm/utils.py:71-80): softmax(mean over the row's windows)[1], the
                                  label of the first window. One window per row is the LAM PostProcessor.update (HHI/utils/lam/utils.py:34-47).
    calculate_precision_recall    HHI/utils/ttm/metrics.py:138-166 after the sort of :123-128 - with the library's DEFINED tie order: among
                                  equal scores the lower row first (pandas' quicksort leaves it unspecified)
    compute_average_precision     metrics.py:26-71, both Python loops as written
    compute_confusion_matrix      metrics.py:232-247
    run_evaluation                metrics.py:169-199: class 0 on (1 - score, 1 - label), class 1 on (score, label), mAP, acc

Class 0's order: the reference sorts 1 - score (fp64) descending. Two fp32 scores that differ by less than 2^-53 of 1 tie there; the
library orders every row by its fp32 score, so the gate's class-0 pass sorts by the score ASCENDING (stable), which is the same order
wherever 1 - score is injective.

`PERTURBATIONS` are deliberate mistakes (`perturb=`); test_cpu_segment_ap.py shows that each misses its bar on the planted inputs.
"""
import numpy as np

SCORE_TOL = 2e-6                # scores against the fp64 gate, absolute: the project's fp32-grade output bar (tests/fp32_grade.py OUT_TOL)
FIXTURE_AP_TOL = 1e-12          # the gate against the recorded reference
PERTURBATIONS = ("tie_reversed", "no_envelope", "no_endpoints", "gt_threshold", "class0_on_label", "mean_after_softmax")
MARGIN = 10.0                   # a perturbed reference misses its bar by at least this factor


def tile() -> int:
    """The tile of the kernels: up to it ONE workgroup runs the sort and the AP pass, beyond it the multi-launch chain."""
    from egot2_amd import functional
    return functional.SEG_AP_TILE


def ap_tol(n: int) -> float:
    """AP / mAP of the device against this algorithm on the device's own scores and order: n fp64 terms <= 1, each formed with at most
    four roundings, twice over."""
    return 8.0 * n * 2.0 ** -53


# ---- the literal algorithm ---------------------------------------------------------------------------------------------------------------
def _softmax1(x):
    e = np.exp(x - np.max(x))
    return (e / e.sum())[1]


def merge_output_fast(logits, slots, labels, n):
    """merge_output without the Python loop over the rows (checked against it in test_cpu_segment_ap.py), for large N."""
    logits, slots = np.asarray(logits, dtype=np.float64), np.asarray(slots, dtype=np.int64)
    first = np.flatnonzero(np.concatenate([[True], slots[1:] != slots[:-1]]))
    count = np.diff(np.concatenate([first, [len(slots)]]))
    with np.errstate(invalid="ignore"):
        mean = np.add.reduceat(logits, first, axis=0) / count[:, None]
        e = np.exp(mean - mean.max(axis=1, keepdims=True))
        s = e[:, 1] / e.sum(axis=1)
    score, label = np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    score[slots[first]] = s
    label[slots[first]] = np.asarray(labels)[first] == 1
    return score, label


def merge_output(logits, slots, labels, n_rows=None, perturb=None, fast=False):
    """-> (score (N,) fp64, label (N,) int64): utils.py:71-80 per run of equal slots. A row without a window: nan, label 0."""
    logits = np.asarray(logits, dtype=np.float64)
    slots = np.asarray(slots, dtype=np.int64)
    n = int(slots.max()) + 1 if n_rows is None else int(n_rows)
    if fast and perturb is None:
        return merge_output_fast(logits, slots, labels, n)
    score, label = np.full(n, np.nan), np.zeros(n, dtype=np.int64)
    seen = np.zeros(n, dtype=bool)
    i = 0
    while i < len(slots):
        j = i
        while j < len(slots) and slots[j] == slots[i]:
            j += 1
        pred = logits[i:j]
        with np.errstate(invalid="ignore"):
            if perturb == "mean_after_softmax":
                s = np.mean([_softmax1(p) for p in pred])
            else:
                s = _softmax1(pred.mean(0))
        r = int(slots[i])
        assert not seen[r], "a row's windows must be adjacent"
        seen[r] = True
        score[r] = s
        label[r] = 1 if int(labels[i]) == 1 else 0
        i = j
    return score, label


def stable_orders(score, perturb=None):
    """-> (order1, order0): rows by score descending / ascending, the lower row first among equal scores; a NaN ranks above every number
    (first in order1, last in order0), NaNs among themselves by row."""
    s = np.asarray(score)
    key = np.where(np.isnan(s), np.inf, s).astype(np.float64)
    nan = np.isnan(s).astype(np.int64)
    rows = np.arange(len(s))
    tie = -rows if perturb == "tie_reversed" else rows
    order0 = np.lexsort((tie, nan, key))
    order1 = np.lexsort((tie, -nan, -key))
    return order1.astype(np.int64), order0.astype(np.int64)


def calculate_precision_recall(labels_in_order):
    """metrics.py:138-166 on the class's labels in sorted order."""
    is_tp = np.asarray(labels_in_order, dtype=np.int64)
    all_positives = int(is_tp.sum())
    tp = np.cumsum(is_tp)
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = tp / (np.arange(len(tp)) + 1)
        recall = tp / np.float64(all_positives)
    return precision.astype(np.float64), recall.astype(np.float64)


def compute_average_precision(precision, recall, perturb=None):
    """metrics.py:61-71, the loops as written."""
    if perturb != "no_endpoints":
        recall = np.concatenate([[0], recall, [1]])
        precision = np.concatenate([[0], precision, [0]])
    else:
        recall, precision = recall.copy(), precision.copy()
    if perturb != "no_envelope":
        for i in range(len(precision) - 2, -1, -1):
            precision[i] = np.maximum(precision[i], precision[i + 1])
    indices = np.where(recall[1:] != recall[:-1])[0] + 1
    return float(np.sum((recall[indices] - recall[indices - 1]) * precision[indices]))


def compute_average_precision_fast(precision, recall):
    """The same sum with the envelope loop as one reversed running maximum: bit-identical (checked in test_cpu_segment_ap.py), for large N."""
    recall = np.concatenate([[0], recall, [1]])
    precision = np.concatenate([[0], precision, [0]])
    precision = np.maximum.accumulate(precision[::-1])[::-1]
    indices = np.where(recall[1:] != recall[:-1])[0] + 1
    return float(np.sum((recall[indices] - recall[indices - 1]) * precision[indices]))


def class_ap(labels_in_order, perturb=None, fast=False):
    """AP of one class from its labels in sorted order; nan without a positive row (the reference's recall is 0 / 0)."""
    precision, recall = calculate_precision_recall(labels_in_order)
    if np.isnan(recall).any():
        return float("nan")
    if fast:
        return compute_average_precision_fast(precision, recall)
    return compute_average_precision(precision, recall, perturb)


def compute_confusion_matrix(score, label, perturb=None):
    s, pos = np.asarray(score), np.asarray(label) == 1
    with np.errstate(invalid="ignore"):
        pred = s > 0.5 if perturb == "gt_threshold" else s >= 0.5
    return {"TP": int((pred & pos).sum()), "FN": int((~pred & pos).sum()), "FP": int((pred & ~pos).sum()), "TN": int((~pred & ~pos).sum())}


def ap_on_order(label, order1, order0, perturb=None, fast=False):
    """(AP0, AP1, mAP) of the rows' labels under given orders."""
    label = np.asarray(label, dtype=np.int64)
    lab0 = label if perturb == "class0_on_label" else 1 - label
    ap0 = class_ap(lab0[order0], perturb, fast)
    ap1 = class_ap(label[order1], perturb, fast)
    return ap0, ap1, float(np.mean([ap0, ap1]))


def run_evaluation(score, label, perturb=None, fast=False):
    """metrics.py:169-199 -> dict: AP0, AP1, mAP, acc, n, n_pos, TP, FN, FP, TN, n_nonfinite, order1, order0."""
    score, label = np.asarray(score), np.asarray(label, dtype=np.int64)
    n = len(score)
    order1, order0 = stable_orders(score, perturb)
    n_bad = int((~np.isfinite(score)).sum())
    if n_bad:
        ap0 = ap1 = m = float("nan")
    else:
        ap0, ap1, m = ap_on_order(label, order1, order0, perturb, fast)
    cm = compute_confusion_matrix(score, label, perturb)
    return {"AP0": ap0, "AP1": ap1, "mAP": m, "acc": (cm["TP"] + cm["TN"]) / n, "n": n, "n_pos": int((label == 1).sum()), **cm,
            "n_nonfinite": n_bad, "order1": order1, "order0": order0}


def evaluate(logits, slots, labels, n_rows=None, perturb=None, fast=False):
    score, label = merge_output(logits, slots, labels, n_rows, perturb, fast)
    return {"score": score, "label": label, **run_evaluation(score, label, perturb, fast)}


def same(a: float, b: float, tol: float) -> bool:
    """nan matches nan; otherwise |a - b| <= tol."""
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
KINDS = ("rand50", "rand02", "allpos", "allneg", "quant8", "equal", "half", "nonfinite")


def sizes():
    """The row counts of the GPU suite: around a wave, around the tile, two tiles and a part, and the largest grid <= 2^17 rows (the
    cross-tile scans have a single level)."""
    t = tile()
    return [1, 2, 3, 63, 64, 65, t - 1, t, t + 1, 2 * t + 17, 1 << 17]


def kinds_for(n: int):
    """Every input kind at every size."""
    return KINDS


def make_input(n: int, kind: str, seed: int = 0, max_windows: int = 9):
    """-> (logits (B, 2) fp32, slots (B,) int64, labels (B,) int64) of n rows with 1 .. max_windows windows each.
    rand50 / rand02 / allpos / allneg: logit differences uniform in [-40, 40] (scores from 4e-18 to 1: keys that differ in every radix
    digit) plus window noise; labels at prevalence 0.5 / 0.02 / 1 / 0.  quant8: 8 exactly representable score levels (ties between rows of
    both labels).  equal: one score for every row.  half: every fourth row has equal logits in every window (score exactly 0.5), the rest as
    rand50.  nonfinite: rand50 with one +inf logit in a window of row n // 2."""
    rng = np.random.default_rng(1000 * n + 17 * KINDS.index(kind) + seed)
    n_w = rng.integers(1, max_windows + 1, size=n) if max_windows > 1 else np.ones(n, dtype=np.int64)
    slots = np.repeat(np.arange(n, dtype=np.int64), n_w)
    B = len(slots)
    prevalence = {"rand02": 0.02, "allpos": 1.0, "allneg": 0.0}.get(kind, 0.5)
    row_label = (rng.random(n) < prevalence).astype(np.int64)
    labels = row_label[slots].copy()
    later = np.concatenate([[False], slots[1:] == slots[:-1]])
    labels[later] = 1 - labels[later]                          # only the FIRST window's label counts (utils.py:78)
    if kind == "quant8":
        level = rng.integers(-4, 4, size=n)
        logits = np.stack([np.zeros(B), 0.5 * level[slots]], axis=1)
    elif kind == "equal":
        logits = np.tile(np.array([[1.0, 2.0]]), (B, 1))
    else:
        diff = rng.uniform(-40.0, 40.0, size=n)
        base = rng.normal(size=n)
        logits = np.stack([base[slots], (base + diff)[slots]], axis=1) + rng.normal(scale=2.0, size=(B, 2))
        if kind == "half":
            on = (slots % 4) == 0
            logits[on, 1] = logits[on, 0]
        if kind == "nonfinite":
            logits[int(np.searchsorted(slots, n // 2)), 1] = np.inf
    return logits.astype(np.float32), slots, labels


def planted():
    """Small inputs on which every perturbation shows: ties between rows of both labels (tie order), a precision that rises again
    (envelope), a positive row in first place of both classes (endpoints), a score of exactly 0.5 on a positive and a negative row
    (threshold), uneven classes (class-0 labels), and rows whose windows disagree strongly (mean before softmax).
    -> (logits, slots, labels) with the windows of 12 rows."""
    rows = [  # (label, windows of (logit0, logit1))
        (1, [(0.0, 6.0)]),                       # the top row of class 1, positive
        (0, [(0.0, 3.0), (0.0, 3.0)]),
        (1, [(0.0, 3.0)]),                       # ties with the row above: the negative row comes first by row order
        (0, [(0.0, 2.0)]),
        (1, [(0.0, 1.0), (0.0, 1.0), (0.0, 1.0)]),
        (1, [(0.0, 1.0)]),
        (1, [(2.0, 2.0)]),                       # exactly 0.5, positive
        (0, [(-1.0, -1.0), (3.0, 3.0)]),         # exactly 0.5, negative
        (1, [(0.0, -9.0), (0.0, 7.0)]),          # windows that disagree: mean -1 -> 0.27, mean of softmaxes -> 0.50
        (0, [(0.0, -2.0)]),
        (1, [(0.0, -2.0)]),                      # ties with the row above in class 0's pass too
        (0, [(0.0, -6.0)]),                      # the top row of class 0, positive there
    ]
    logits, slots, labels = [], [], []
    for r, (lab, wins) in enumerate(rows):
        for w in wins:
            logits.append(w)
            slots.append(r)
            labels.append(lab)
    return np.asarray(logits, dtype=np.float32), np.asarray(slots, dtype=np.int64), np.asarray(labels, dtype=np.int64)
