"""The gate of the action-recognition test epoch on the device (egx_view_ensemble_update / egx_view_ensemble_topk, ABI v23;
train.ViewEnsembleTest): the literal loop of MultiTaskClassificationTask.test_epoch_end (HOI/tasks/lta/long_term_anticipation.py:96-158)
restated on numpy.

    ensemble()   dicts keyed by clip id; an fp32 `+=` or maximum per clip from a row of zeros, in ARRIVAL order; a video's label is its
                 last clip's; the dict values stacked in insertion order. Every operation is the fp32 operation the reference runs, in its
                 order, so the rows are compared BIT FOR BIT (bars: none - equality).
    rank_rows()  the ranks in fp64 on those fp32 rows: rank = #{c : x_c > x_y} + #{c < y : x_c == x_y} (the lower class wins ties; where the
                 reference is tie-free this is torch.topk's order), a NaN as the greatest value, -1 for a label outside [0, C_h) (never
                 correct); pred = the class of rank 0; the counts. Integers: compared exactly.
    errors()     (1 - correct / n) * 100 in fp32 with n = the number of videos, as topk_errors computes it on fp32 tensors.

`perturb` turns one deliberate mistake on (PERTURBATIONS); `planted(method)` holds an input on which each of them shows (asserted in
tests/test_cpu_view_ensemble.py, not assumed). `make_epoch` builds the seeded epochs of the GPU tests."""
import numpy as np

KS = (1, 5)
DROP = object()                   # a clip whose slot lies outside [0, capacity): dropped and counted, it opens no video
FLT_MIN = float(np.finfo(np.float32).tiny)
# the mistake -> the methods on whose planted input it shows
PERTURBATIONS = {"first_label": ("sum", "max"), "max_from_neg_inf": ("max",), "higher_class_wins_ties": ("sum", "max"),
                 "divide_by_valid": ("sum", "max"), "reverse_order": ("sum",)}


def ensemble(preds, labels, ids, method="sum", perturb=None):
    """preds fp32 (N, ld), labels int64 (N, H), ids: N hashables -> dict(rows fp32 (n, ld), labels (n, H), ids, views (n,), n_dropped,
    min_partial: the smallest non-zero |partial value| met on the way)."""
    preds = np.asarray(preds, dtype=np.float32)
    labels = np.asarray(labels, dtype=np.int64)
    assert method in ("sum", "max") and preds.shape[0] == labels.shape[0] == len(ids)
    video_labels, video_preds, views = {}, {}, {}
    n_dropped, min_partial = 0, np.inf
    start = -np.inf if (perturb == "max_from_neg_inf" and method == "max") else 0.0
    for i, vid in enumerate(ids):                           # the reference's walk: insertion order of the dicts, the labels
        if vid is DROP:
            n_dropped += 1
            continue
        if not (perturb == "first_label" and vid in video_labels):
            video_labels[vid] = labels[i]
        if vid not in video_preds:
            video_preds[vid] = np.full(preds.shape[1], start, dtype=np.float32)
            views[vid] = 0
        views[vid] += 1
    order = range(len(ids) - 1, -1, -1) if perturb == "reverse_order" else range(len(ids))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in order:
            vid = ids[i]
            if vid is DROP:
                continue
            if method == "sum":
                video_preds[vid] += preds[i]                  # fp32 + fp32 -> fp32
            else:
                video_preds[vid] = np.maximum(video_preds[vid], preds[i])       # torch.max of two tensors: a NaN stays
            mag = np.abs(video_preds[vid])
            mag = mag[mag > 0]
            if mag.size:
                min_partial = min(min_partial, float(mag.min()))
    keys = list(video_preds)
    H = labels.shape[1]
    return {"rows": np.stack([video_preds[k] for k in keys]) if keys else np.zeros((0, preds.shape[1]), np.float32),
            "labels": np.stack([video_labels[k] for k in keys]) if keys else np.zeros((0, H), np.int64),
            "ids": keys, "views": np.asarray([views[k] for k in keys], dtype=np.int32), "n_dropped": n_dropped, "min_partial": min_partial}


def rank_rows(rows, labels, classes, ks=KS, perturb=None):
    """-> dict(rank (n, H) int32, pred (n, H) int32, n, n_nonfinite, n_invalid (H,), correct (len(ks), H)) of the fp32 rows, in fp64."""
    rows = np.asarray(rows, dtype=np.float32)
    n, H = rows.shape[0], len(classes)
    rank = np.zeros((n, H), dtype=np.int32)
    pred = np.zeros((n, H), dtype=np.int32)
    nonfinite = np.zeros(n, dtype=bool)
    higher = perturb == "higher_class_wins_ties"
    c0 = 0
    for h, C in enumerate(classes):
        for v in range(n):
            x = rows[v, c0:c0 + C].astype(np.float64)
            nonfinite[v] |= not np.isfinite(x).all()
            key = np.where(np.isnan(x), np.inf, x)
            top = np.flatnonzero(key == key.max())
            pred[v, h] = top[-1] if higher else top[0]
            y = int(labels[v, h])
            if not 0 <= y < C:
                rank[v, h] = -1
                continue
            ties = (key[y + 1:] == key[y]).sum() if higher else (key[:y] == key[y]).sum()
            rank[v, h] = int((key > key[y]).sum() + ties)
        c0 += C
    n_invalid = (rank < 0).sum(axis=0).astype(np.int64)
    correct = np.asarray([[int(((rank[:, h] >= 0) & (rank[:, h] < k)).sum()) for h in range(H)] for k in ks], dtype=np.int64).reshape(len(ks), H)
    return {"rank": rank, "pred": pred, "n": n, "n_nonfinite": int(nonfinite.sum()), "n_invalid": n_invalid, "correct": correct}


def errors(correct, n, n_invalid=None, perturb=None):
    """(1 - correct / n) * 100 in fp32 -> (len(ks), H) fp32 (topk_errors: a float32 tensor divided by preds.size(0))."""
    correct = np.asarray(correct)
    den = np.full(correct.shape[1], n, dtype=np.float32)
    if perturb == "divide_by_valid":
        den = den - np.asarray(n_invalid, dtype=np.float32)
    return (np.float32(1.0) - correct.astype(np.float32) / den[None, :]) * np.float32(100.0)


def head_names(H):
    return ("verb", "noun") if H == 2 else tuple(str(h) for h in range(H))


def evaluate(preds, labels, ids, classes, method="sum", ks=KS, perturb=None):
    """The whole epoch -> the ensemble, the ranks and counts, `err` (len(ks), H) fp32 and `result`: the step_result keys without a prefix."""
    ens = ensemble(preds, labels, ids, method, perturb)
    res = rank_rows(ens["rows"], ens["labels"], classes, ks, perturb)
    err = errors(res["correct"], res["n"], res["n_invalid"], perturb)
    out = {**ens, **res, "err": err, "result": {"n": res["n"], "n_dropped": ens["n_dropped"], "n_nonfinite": res["n_nonfinite"]}}
    for h, name in enumerate(head_names(len(classes))):
        out["result"][f"n_invalid_{name}"] = int(res["n_invalid"][h])
        for ki, k in enumerate(ks):
            out["result"][f"correct{k}_{name}"] = int(res["correct"][ki, h])
            out["result"][f"top{k}_{name}_err"] = float(err[ki, h])
    return out


# ---- planted input ---------------------------------------------------------------------------------------------------------------------
PLANTED_CLASSES = (5, 7)


def planted(method="sum"):
    """-> (preds (N, 12) fp32, labels (N, 2), ids) on classes (5, 7): small integers, so every sum but the planted one is exact.
        first     two views with DIFFERENT labels; the last one's is the argmax of both heads, the first one's is not
        negative  every logit negative, label (0, 0) at the LOWEST values: under "max" the row stays zeros and the rank is the label's index, 0
        tie       verb: the label 2 ties with the lower class 1 at the maximum (rank 1); noun: the label 3 ties with the higher class 5 (rank 0)
        invalid   verb label 7 is outside [0, 5); the noun is right
        order     verb column 4 sees 1, 2^24, -2^24: 0 in arrival order, 1 in reverse ("sum"); its labels sit on other, larger columns
        nan       a NaN in the noun head: non-finite, the NaN is the prediction
        plain     three more views of an ordinary video; a dropped clip in between
    The views are interleaved."""
    big = float(1 << 24)
    v = {  # id -> list of (verb row, noun row, label)
        "first": [([1, 5, 0, 2, 0], [0, 1, 0, 2, 6, 0, 1], (3, 2)), ([0, 4, 1, 1, 0], [1, 0, 1, 0, 5, 1, 0], (1, 4))],
        "negative": [([-9, -2, -3, -1, -4], [-9, -1, -2, -3, -4, -5, -6], (0, 0)), ([-8, -1, -1, -2, -3], [-7, -2, -1, -1, -2, -3, -4], (0, 0))],
        "tie": [([0, 4, 4, 1, 2], [0, 1, 2, 6, 3, 6, 1], (2, 3))],
        "invalid": [([3, 0, 1, 0, 2], [0, 0, 7, 1, 0, 2, 1], (7, 2))],
        "order": [([9, 0, 2, 1, 1], [1, 8, 0, 0, 2, 0, 1], (0, 1)), ([9, 1, 0, 0, big], [0, 9, 1, 0, 0, 1, 0], (0, 1)),
                  ([9, 0, 1, 1, -big], [2, 9, 0, 1, 0, 0, 0], (0, 1))],
        "nan": [([2, 1, 0, 0, 1], [0, 1, float("nan"), 0, 3, 0, 1], (0, 4))],
        "plain": [([0, 1, 6, 1, 0], [1, 0, 0, 2, 0, 7, 0], (2, 5)), ([1, 0, 5, 0, 2], [0, 2, 1, 0, 0, 6, 1], (2, 5)),
                  ([0, 2, 4, 1, 1], [0, 0, 1, 1, 2, 5, 0], (2, 6))],
    }
    arrival = [("first", 0), ("order", 0), ("negative", 0), ("plain", 0), ("tie", 0), ("order", 1), (DROP, 0), ("first", 1), ("plain", 1),
               ("invalid", 0), ("nan", 0), ("order", 2), ("negative", 1), ("plain", 2)]
    preds, labels, ids = [], [], []
    for vid, k in arrival:
        verb, noun, lab = v["plain"][0] if vid is DROP else v[vid][k]
        preds.append(list(verb) + list(noun))
        labels.append(lab)
        ids.append(vid)
    assert method in ("sum", "max")
    return np.asarray(preds, dtype=np.float32), np.asarray(labels, dtype=np.int64), ids


# ---- seeded epochs -----------------------------------------------------------------------------------------------------------------------
def make_epoch(classes, views, seed, interleave=True):
    """`views[v]` clips for video v -> (preds (N, sum classes) fp32 = 3 randn + 0.25, labels (N, H), ids): interleaved by a seeded shuffle
    (or video after video), differing labels among a video's views. The shift keeps partial sums off the subnormals (checked by the
    caller through ensemble()["min_partial"])."""
    rng = np.random.RandomState(seed)
    ids = [v for v, k in enumerate(views) for _ in range(k)]
    if interleave:
        ids = [ids[i] for i in rng.permutation(len(ids))]
    N = len(ids)
    preds = (3.0 * rng.standard_normal((N, sum(classes))) + 0.25).astype(np.float32)
    labels = np.stack([rng.randint(0, C, size=N) for C in classes], axis=1).astype(np.int64)
    return preds, labels, ids


def slots_of(ids):
    """The dense slot of every id in first-appearance order (the reference's dict order); DROP -> -1."""
    seen = {}
    return np.asarray([-1 if i is DROP else seen.setdefault(i, len(seen)) for i in ids], dtype=np.int64)
