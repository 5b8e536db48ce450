"""fp64 reference of egx_segmented_ce (include/egot2x.h), its cases, inputs and bars: the gate of test_gpu_seg_ce.py.

Plain torch on the CPU; nothing here is imported from the product path. The reference is the literal double loop of
LongTermAnticipationTask.training_step (HOI/tasks/lta/long_term_anticipation.py:182-203) over heads and future steps, F.cross_entropy on the
rows with a valid label, plus the header's rank rule for the top-k counts. It computes in the dtype of its arguments: fp64 arguments give
the reference, fp32 arguments the yardstick ("the same criterion in plain fp32 torch") the bars are taken from. `perturb=` names one
deliberate mistake; it is used only by tests/test_cpu_seg_ce.py, which checks that the bars (or the exact counts) reject each of them.

Bars
    BAR[kind] = FACTOR * FP32_ERR[kind], kind in loss, loss_terms, d_logits: FP32_ERR is the worst error, over the cases below, of the fp32
    evaluation of the reference against its fp64 evaluation on these same inputs; the error of a tensor is tests/unit_ref.py's rel_err
    (max |got - ref| over that tensor's largest |ref|). FACTOR = 8 covers another summation order and another exp / log.
    n_valid and the top-k counts have NO bar: the inputs are fp32 numbers and the fp64 reference compares those same numbers, so a correct
    kernel matches every count exactly, on every case.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.unit_ref import rel_err  # noqa: F401  (the metric of the bars; re-exported for the tests)

F64 = torch.float64
FACTOR = 8.0
KS = (1, 5)
# Measured by tests/test_cpu_seg_ce.py (test_fp32_reference_meets_the_bar prints them with -s): worst rel_err of the fp32 evaluation over
# the cases. The CPU test holds each constant to the value it measures (within 3x either way: another CPU's vector width changes torch's
# fp32 summation order), so a bar cannot be widened by editing the constant alone.
FP32_ERR = {"loss": 1.1e-7, "loss_terms": 1.1e-7, "d_logits": 4.3e-7}
BAR = {kind: FACTOR * e for kind, e in FP32_ERR.items()}
# Worst (smallest) error / bar of each perturbed reference over the cases it changes, as test_cpu_seg_ce.py measures them (it requires
# >= 3), or "counts" where the perturbation shows in the exact counts.
PERTURB_RATIO = {"mean_over_all_B": 4.4e3, "one_normaliser": 2.9e4, "rank_ge": "counts", "col0_plus_1": "counts"}
PERTURBATIONS = tuple(PERTURB_RATIO)

# (B, Z, classes, ld, col0): col0 None = the heads tile the row from column 0
CASES = [
    (1, 1, (1,), 1, None),                      # one row, one class: loss 0, gradient 0
    (3, 1, (2,), 2, None),                      # the TTM shape
    (5, 3, (5, 7), 12, None),                   # the small LTA model of the model-level tests
    (4, 2, (63, 64, 65), 192, None),            # around one lane-stride (64): 1 and 2 registers per lane, three heads
    (257, 2, (115, 478), 593, None),            # the LTA heads at an odd row stride, more than one chunk of clips, B no multiple of the chunk
    (2, 20, (115, 478), 593, None),             # the LTA shape: Z = 20
    (3, 2, (513, 1000), 1513, None),            # just above the register path: the re-read loop
    (2, 1, (2048,), 2048, None),                # the class limit
    (3, 2, (5, 7), 20, (1, 9)),                 # heads at columns 1 and 9: the row has gaps
]


def case_id(case) -> str:
    B, Z, classes, ld, col0 = case
    return f"B{B}_Z{Z}_C{'x'.join(map(str, classes))}_ld{ld}" + ("_gaps" if col0 is not None else "")


def case_col0(case):
    B, Z, classes, ld, col0 = case
    if col0 is not None:
        return list(col0)
    out, off = [], 0
    for c in classes:
        out.append(off)
        off += c
    return out


def seg_inputs(case_index: int):
    """-> (logits (B, Z, ld) fp32, labels (B, Z, H) int64, ks): seeded 3 * randn (gap columns included: they must not matter) with, where the
    case has the rows for them, planted
      * a row holding +80 and -80 (an exp that overflows without the max subtraction),
      * a row of all-equal logits (every class ties with the label),
      * ties at and around the label: a class below and a class above the label equal to it, and a class equal to the k-th largest,
      * labels 0 and C - 1, the labels -100 and C (ignored), and - with Z >= 2 - one (z, h) pair without any valid label."""
    B, Z, classes, ld, _ = CASES[case_index]
    col0 = case_col0(CASES[case_index])
    H = len(classes)
    g = torch.Generator(device="cpu").manual_seed(8800 + case_index)
    logits = 3 * torch.randn(B, Z, ld, generator=g)
    labels = torch.stack([torch.randint(0, c, (B, Z), generator=g) for c in classes], dim=-1)
    for h, (c0, C) in enumerate(zip(col0, classes)):
        seg = logits[:, :, c0:c0 + C]           # a view: planting writes through
        labels[0, 0, h] = 0
        labels[B - 1, Z - 1, h] = C - 1
        if C >= 2:
            seg[0, 0, 0], seg[0, 0, C - 1] = 80.0, -80.0
        if B >= 2:
            seg[1, 0, :] = 0.75                 # all equal
            labels[1, 0, h] = min(2, C - 1)
        if B >= 3 and C >= 5:
            y = C // 2
            labels[2, 0, h] = y
            seg[2, 0, y - 1] = seg[2, 0, y]     # a tie below the label (outranks it) and one above (does not)
            seg[2, 0, y + 1] = seg[2, 0, y]
        if B >= 4 and C >= 7:                   # four classes above the label, two tied with it: rank 4 or 5 decides top-5
            y = 5
            labels[3, 0, h] = y
            seg[3, 0, :] = -5.0
            seg[3, 0, 0:4] = 6.0
            seg[3, 0, 4] = seg[3, 0, 5] = seg[3, 0, 6] = 2.5
        if B >= 5:
            labels[4, 0, h] = -100
        if B >= 3 and Z >= 2:
            labels[1, 1, h] = C                 # out of range: ignored
    if Z >= 2:
        labels[:, Z - 1, 0] = -100              # a (z, h) pair without any valid label
        if B >= 2:
            labels[0, Z - 1, 0] = classes[0]
    return logits, labels, tuple(k for k in KS if k <= min(classes))


def rank_of_label(z, y, perturb=None):
    """z (n, C), y (n,) -> rank (n,) = #{c : z_c > z_y} + #{c < y : z_c == z_y}."""
    zy = z.gather(1, y[:, None])
    c = torch.arange(z.shape[1])[None, :]
    if perturb == "rank_ge":
        return (z >= zy).sum(1) - 1
    return (z > zy).sum(1) + ((z == zy) & (c < y[:, None])).sum(1)


def segmented_ce(logits, labels, classes, col0, ks, perturb=None):
    """The criterion in the dtype of `logits` -> dict: loss (), loss_terms (Z, H), n_valid (Z, H) int64, correct (len(ks), Z, H) int64 and
    d_logits (B, Z, ld) = d loss / d logits by autograd (zero where nothing depends on a logit)."""
    B, Z, ld = logits.shape
    H = len(classes)
    x = logits.detach().clone().requires_grad_(True)
    terms = torch.zeros(Z, H, dtype=logits.dtype)
    n_valid = torch.zeros(Z, H, dtype=torch.int64)
    correct = torch.zeros(len(ks), Z, H, dtype=torch.int64)
    loss = torch.zeros((), dtype=logits.dtype)
    n_all = sum(int(((labels[:, :, h] >= 0) & (labels[:, :, h] < classes[h])).sum()) for h in range(H))
    for h in range(H):
        c0 = col0[h] + (1 if perturb == "col0_plus_1" and col0[h] + classes[h] < ld else 0)
        for z in range(Z):
            y = labels[:, z, h]
            ok = (y >= 0) & (y < classes[h])
            n = int(ok.sum())
            n_valid[z, h] = n
            if n == 0:
                continue                                    # the header's rule: such a pair adds nothing (torch: nan)
            seg = x[ok, z, c0:c0 + classes[h]]
            if perturb == "mean_over_all_B":
                t = F.cross_entropy(seg, y[ok], reduction="sum") / B
            elif perturb == "one_normaliser":
                t = F.cross_entropy(seg, y[ok], reduction="sum") / n_all * (Z * H)
            else:
                t = F.cross_entropy(seg, y[ok])
            terms[z, h] = t.detach()
            loss = loss + t
            r = rank_of_label(seg.detach(), y[ok], perturb)
            for ki, k in enumerate(ks):
                correct[ki, z, h] = int((r < k).sum())
    if loss.requires_grad:
        loss.backward()
    d = x.grad if x.grad is not None else torch.zeros_like(logits)
    return {"loss": loss.detach(), "loss_terms": terms, "n_valid": n_valid, "correct": correct, "d_logits": d}


def topk_errors_of(res: dict):
    """(len(ks), Z, H) fp64: (1 - correct / n_valid) * 100, nan where no label is valid."""
    return (1.0 - res["correct"].double() / res["n_valid"].double()[None]) * 100.0
