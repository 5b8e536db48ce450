"""fp64 reference of egx_sequence_ce (include/egot2x.h), its cases, inputs and bars: the gate of test_gpu_seq_ce.py.

Plain torch on the CPU; nothing here is imported from the product path. The reference is the literal restatement of the EgoT2-g steps:
per task nn.CrossEntropyLoss() on the (B, V, sy) logits against the (B, sy) target and the ratio sum
(HHI/tasks/multitask/video_tasktranslation.py:39-66, HOI/tasks/multitask/video_task.py:537-577), and the update / compute loops of ARMetric
and LTAMetric (HOI/evaluation/lta/lta_metrics.py:164-211, 229-292: the argmax word mapped to its original label, -1 = error), PNRMetric and
OSCCMetric (HOI/evaluation/pnr/metrics.py:139-257: the free argmax outside the task's words = error, the argmax over the task's words against
the label) and the HHI accuracy (video_tasktranslation.py:101-102), all of which are the three counts invalid / correct / correct_restricted
over the scored positions. It computes in the dtype it is asked for: fp64 gives the reference, fp32 the yardstick ("the same criterion in
plain fp32 torch") the bars are taken from. `perturb=` names one deliberate mistake; it is used only by tests/test_cpu_seq_ce.py, which
checks that the bars (or the exact counts) reject each of them.

Bars
    BAR[kind] = FACTOR * FP32_ERR[kind], kind in loss, loss_terms, d_logits - the rule and the FACTOR of tests/seg_ce_ref.py: FP32_ERR is the
    worst error, over the cases below, of the fp32 evaluation of the reference against its fp64 evaluation on these same inputs; the error of
    a tensor is tests/unit_ref.py's rel_err (max |got - ref| over that tensor's largest |ref|); d_logits is compared per task.
    The d_logits constant is set by the rows with a large planted maximum (15 .. 80): x - max carries ulp(max) there in ANY fp32 evaluation,
    and the softmax inherits it as a relative error.
    The integer counts (n_valid, token_correct, seq_correct, scored, invalid, correct, correct_restricted) and pred have NO bar: the inputs
    are fp32 numbers and the fp64 reference compares those same numbers, so a correct kernel matches every count exactly, on every case.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.seg_ce_ref import FACTOR
from tests.unit_ref import rel_err  # noqa: F401  (the metric of the bars; re-exported for the tests)

F64 = torch.float64
KINDS = ("loss", "loss_terms", "d_logits")
COUNTS = ("n_valid", "token_correct", "seq_correct", "scored", "invalid", "correct", "correct_restricted")
# Measured by tests/test_cpu_seq_ce.py (test_fp32_reference_meets_the_bar prints them with -s): worst rel_err of the fp32 evaluation over
# the cases. The CPU test holds each constant to the value it measures (within 3x either way: another CPU's vector width changes torch's
# fp32 summation order), so a bar cannot be widened by editing the constant alone.
FP32_ERR = {"loss": 8.3e-8, "loss_terms": 7.4e-8, "d_logits": 5.7e-6}
BAR = {kind: FACTOR * e for kind, e in FP32_ERR.items()}
# Worst (smallest) error / bar of each perturbed reference over the cases it changes without changing a count, as test_cpu_seq_ce.py
# measures them (it requires >= 3), or "counts" where the perturbation shows in the exact counts on every case it changes.
PERTURB_RATIO = {"mean_per_position": 6.7e4, "ignored_in_normaliser": 8.5e4, "ratio_dropped": 1.1e5, "ties_high": "counts",
                 "restricted_is_free": "counts", "seq_counts_empty": "counts"}
PERTURBATIONS = tuple(PERTURB_RATIO)

# A case: (name, V, tasks); a task: dict(B, sy, ratio, layout, metric, grad, valid).
#   layout  "perm": the (sy, B, V) decoder output seen through its (B, V, sy) view; "contig": a contiguous (B, sy, V) tensor;
#           "unaligned": rows of stride V + 1 (a (B, sy, V + 1) tensor's first V columns)
#   metric  None, or the number of original labels L: words are mapped to labels 0 .. L - 1 at scattered indices, the rest to -1
#   grad    d_logits is asked for;  valid: False = every target is ignored (a task without a valid label)
def _t(B, sy, ratio=1.0, layout="perm", metric=None, grad=True, valid=True, score_all=False):
    return dict(B=B, sy=sy, ratio=ratio, layout=layout, metric=metric, grad=grad, valid=valid, score_all=score_all)


CASES = [
    ("minimal", 2, [_t(1, 1)]),
    ("hhi", 7, [_t(5, 2, 1.0, metric=2), _t(3, 2, 1.0, metric=2), _t(45, 2, 0.5, metric=2)]),     # B = 45: 12 chunks of 4 rows, the last one short
    ("hoi", 620, [_t(4, 2, 1.0, metric=16), _t(8, 2, 1.0, metric=2), _t(4, 2, 1.0, metric=115), _t(4, 2, 1.0, metric=478),
                  _t(3, 21, 0.5, metric=115), _t(3, 21, 0.5, metric=478)]),
    ("V64", 64, [_t(5, 3, metric=3)]),                  # one register per lane, full
    ("V65", 65, [_t(5, 3, metric=3)]),                  # ... one word into the second
    ("V512", 512, [_t(5, 3, metric=3)]),                # the register path's limit
    ("V513", 513, [_t(5, 3, metric=3)]),                # the re-read loop
    ("V2048", 2048, [_t(5, 3, metric=3)]),              # the vocabulary limit
    ("limits", 33, [_t(2, 64, metric=4, score_all=True), _t(2, 1), _t(3, 2, 0.0, metric=2), _t(6, 2, valid=False), _t(2, 3, 2.0),
                    _t(1, 5, metric=5), _t(9, 2, 0.25), _t(2, 2, 1.0, metric=2)]),      # T = 8, sy = 64, ratio 0, a task without a valid label
    ("contig", 70, [_t(5, 3, layout="contig", metric=3), _t(6, 2, 0.5, layout="contig")]),
    ("unaligned", 129, [_t(5, 3, layout="unaligned", metric=3), _t(7, 2, 0.5, layout="unaligned")]),
    ("no_grad", 70, [_t(5, 3, metric=3, grad=False), _t(6, 2, 0.5, grad=False)]),
    ("metrics_only", 70, [_t(6, 3, metric=3, grad=False, valid=False, score_all=True), _t(5, 1, metric=2, grad=False, valid=False)]),
    ("many_rows", 5, [_t(1030, 1, metric=2), _t(7, 2, 0.5)]),     # 206 chunks of 5 rows: a wave walks two rows, a lane of the last workgroup adds four chunks
]
CASE_IDS = [c[0] for c in CASES]


def word_label_of(V: int, L: int, seed: int) -> torch.Tensor:
    """int32 (V,): L labels at scattered words (when V allows it, fewer words than V, so unmapped words exist), -1 elsewhere."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = min(L, max(1, V - 1))
    words = torch.randperm(V, generator=g)[:n]
    m = torch.full((V,), -1, dtype=torch.int32)
    m[words] = torch.arange(n, dtype=torch.int32)
    return m


def seq_inputs(case_index: int) -> list:
    """-> per task a dict: logits (B, sy, V) fp32 (the rows in canonical order; the GPU test lays them out as `layout` says), target (B, sy)
    int64, ratio, word_label (V,) int32 or None, labels (B, sy) int64 or None (position 0 is scored, every position with score_all), and the
    task's layout / grad flags. Seeded 3 * randn with, where the task has the rows for them, planted
      * rows b = 0 mod 3: the target's logit raised at every position, so whole rows are right (seq_correct counts something),
      * row 0, position 0: a row holding +80 and -80 (an exp that overflows without the max subtraction),
      * row 1, position 0: all-equal logits (every word ties with the target),
      * row 2, position 0: a tie between the target and the word below it, both the maximum (the lower word wins: the token is wrong),
      * row 3: no valid position at all (targets -100 and V): the clip must not count as a right sequence,
      * row 4: targets -100 at position 0 and V at the last position,
      * metric tasks: rows b = 6, 8, ... have the label's word raised at position 0 (correct), row 3 - whose targets are all ignored - has
        the top logit on an unmapped word (invalid; the restricted argmax differs from the free one), row 4 a tie between two mapped words."""
    name, V, tasks = CASES[case_index]
    out = []
    for ti, k in enumerate(tasks):
        B, sy = k["B"], k["sy"]
        g = torch.Generator(device="cpu").manual_seed(9700 + 31 * case_index + ti)
        logits = 3 * torch.randn(B, sy, V, generator=g)
        target = torch.randint(0, V, (B, sy), generator=g)
        for b in range(0, B, 3):
            for s in range(sy):
                logits[b, s, target[b, s]] = 15.0
        target[0, 0] = min(1, V - 1)
        logits[0, 0, 0], logits[0, 0, V - 1] = 80.0, -80.0
        if B >= 2:
            logits[1, 0, :] = 0.75
            target[1, 0] = min(2, V - 1)
        if B >= 3 and V >= 5:
            y = V // 2
            target[2, 0] = y
            logits[2, 0, y - 1] = logits[2, 0, y] = 20.0
        if B >= 4:
            target[3, :] = -100
            target[3, sy - 1] = V
        if B >= 5:
            target[4, 0] = -100
            target[4, sy - 1] = V
        if not k["valid"]:
            target[:] = -100
        wl = labels = None
        if k["metric"] is not None:
            wl = word_label_of(V, k["metric"], 9900 + 31 * case_index + ti)
            mapped = (wl >= 0).nonzero().flatten()
            L = int(mapped.numel())
            labels = torch.full((B, sy), -1, dtype=torch.int64)
            labels[:, 0] = torch.randint(0, L, (B,), generator=g)
            if k["score_all"]:
                labels[:] = torch.randint(0, L, (B, sy), generator=g)
                labels[B - 1, sy - 1] = -1
            unmapped = (wl < 0).nonzero().flatten()
            for b in range(0, B, 2):
                if b not in (0, 2, 4):
                    w = int((wl == labels[b, 0]).nonzero()[0])
                    logits[b, 0, w] = 30.0
            if B >= 4 and unmapped.numel():
                logits[3, 0, int(unmapped[0])] = 25.0
            if B >= 5 and L >= 2:
                w0, w1 = sorted((int(mapped[0]), int(mapped[1])))
                logits[4, 0, w0] = logits[4, 0, w1] = 22.0
                labels[4, 0] = int(wl[w0])
        out.append(dict(logits=logits, target=target, ratio=float(k["ratio"]), word_label=wl, labels=labels, layout=k["layout"],
                        grad=k["grad"]))
    return out


def _argmax(v, perturb=None) -> int:
    """Among equal logits the lower index wins (the header's rule)."""
    hit = (v == v.max()).nonzero().flatten()
    return int(hit[-1] if perturb == "ties_high" else hit[0])


def task_loss(lg, target, V: int, perturb=None):
    """nn.CrossEntropyLoss() on (B, V, sy) logits against the (B, sy) target, labels outside [0, V) ignored; a task without a valid label
    gives 0 (the header's rule; torch: nan)."""
    valid = (target >= 0) & (target < V)
    n = int(valid.sum())
    tgt = torch.where(valid, target, torch.full_like(target, -100))
    if n == 0:
        return lg.sum() * 0, n
    if perturb == "mean_per_position":
        terms = [F.cross_entropy(lg[:, :, s], tgt[:, s], ignore_index=-100) for s in range(lg.shape[2]) if int(valid[:, s].sum()) > 0]
        return sum(terms) / len(terms), n
    if perturb == "ignored_in_normaliser":
        return F.cross_entropy(lg, tgt, ignore_index=-100, reduction="sum") / target.numel(), n
    return torch.nn.CrossEntropyLoss()(lg, tgt), n


def task_metrics(rows, word_label, labels, perturb=None):
    """The metric classes' update loops on one task: rows (B, sy, V), word_label (V,), labels (B, sy) -> (scored, invalid, correct,
    correct_restricted, pred (B, sy, 2) int64)."""
    B, sy, V = rows.shape
    mapping = {int(w): int(word_label[w]) for w in range(V) if int(word_label[w]) >= 0}           # vocab2orig
    indices = sorted(mapping)
    scored = invalid = correct = restricted = 0
    pred = torch.full((B, sy, 2), -1, dtype=torch.int64)
    for b in range(B):
        for s in range(sy):
            v = rows[b, s]
            a = _argmax(v, perturb)
            orig = -1 if a not in mapping else mapping[a]
            r = a if perturb == "restricted_is_free" else indices[_argmax(v[indices], perturb)]
            orig_r = mapping.get(r, -1)
            pred[b, s, 0], pred[b, s, 1] = orig, orig_r
            lab = int(labels[b, s])
            if lab < 0:
                continue
            scored += 1
            invalid += orig == -1
            correct += orig == lab
            restricted += orig_r == lab
    return scored, invalid, correct, restricted, pred


def sequence_ce(tasks, V: int, dtype=F64, perturb=None) -> dict:
    """The step in `dtype` -> dict: loss (), loss_terms (T,), the seven counts (T,) int64, d_logits (list of (B, sy, V), autograd of the
    loss; zeros where nothing depends on a logit) and pred (list of (B, sy, 2) int64 or None)."""
    T = len(tasks)
    xs = [k["logits"].to(dtype).clone().requires_grad_(True) for k in tasks]
    terms = torch.zeros(T, dtype=dtype)
    counts = {c: torch.zeros(T, dtype=torch.int64) for c in COUNTS}
    preds = []
    loss = torch.zeros((), dtype=dtype)
    for t, (k, x) in enumerate(zip(tasks, xs)):
        target = k["target"]
        term, n = task_loss(x.permute(0, 2, 1), target, V, perturb)
        terms[t] = term.detach()
        loss = loss + (1.0 if perturb == "ratio_dropped" else k["ratio"]) * term
        counts["n_valid"][t] = n
        valid = (target >= 0) & (target < V)
        rows = x.detach()
        for b in range(rows.shape[0]):
            right = [_argmax(rows[b, s], perturb) == int(target[b, s]) for s in range(rows.shape[1]) if valid[b, s]]
            counts["token_correct"][t] += sum(right)
            counts["seq_correct"][t] += int(all(right) and (len(right) > 0 or perturb == "seq_counts_empty"))
        if k["word_label"] is not None:
            sc, inv, cor, res, pred = task_metrics(rows, k["word_label"], k["labels"], perturb)
            counts["scored"][t], counts["invalid"][t], counts["correct"][t], counts["correct_restricted"][t] = sc, inv, cor, res
            preds.append(pred)
        else:
            preds.append(None)
    loss.backward()
    return {"loss": loss.detach(), "loss_terms": terms, **counts, "d_logits": [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs],
            "pred": preds}


def evaluate(case_index: int, dtype=F64, perturb=None) -> dict:
    return sequence_ce(seq_inputs(case_index), CASES[case_index][1], dtype, perturb)


def bar_errors(got: dict, ref: dict, grads=None) -> dict:
    """kind -> rel_err of `got` against `ref`; d_logits: the worst over the tasks (those in `grads`, default all)."""
    T = len(ref["d_logits"])
    which = range(T) if grads is None else grads
    errs = [rel_err(got["d_logits"][t], ref["d_logits"][t]) for t in which]
    return {"loss": rel_err(got["loss"], ref["loss"]), "loss_terms": rel_err(got["loss_terms"], ref["loss_terms"]),
            "d_logits": max(errs) if errs else 0.0}


def same_counts(a: dict, b: dict) -> bool:
    return all(torch.equal(a[c].long(), b[c].long()) for c in COUNTS) and all(
        (p is None) == (q is None) and (p is None or torch.equal(p.long(), q.long())) for p, q in zip(a["pred"], b["pred"]))
