"""fp64 reference of egx_keyframe_criterion (include/egot2x.h), its cases, inputs and bars: the gate of test_gpu_keyframe.py.

Plain torch on the CPU; nothing here is imported from the product path. The metrics are the literal loops of keyframe_distance /
keyframe_accuracy (HOI/evaluation/pnr/metrics.py:23-80) and PnrOsccMetric.pnr_distance / oscc_acc (:102-134); the loss is the criterion of
KeyframeLocalisation2Loader.training_step (HOI/tasks/pnr/video_taskspecific_pnr.py:24-63) in LOGIT form - BCELoss(sigmoid(x), y) =
softplus(-x) y + softplus(x) (1 - y), each clamped at 100 as BCELoss clamps its logs at -100 - so that it stays exact where sigmoid
saturates. It computes in the dtype of the logits: fp64 logits give the reference, fp32 logits the yardstick ("the same criterion in plain
fp32 torch") the bars are taken from. The distances are fp64 either way (Python floats, as the reference's .item() values are).
`perturb=` names one deliberate mistake; it is used only by tests/test_cpu_keyframe.py, which checks that the bars (or the exact results)
reject each of them.

Bars
    BAR[kind] = FACTOR * FP32_ERR[kind], kind in loss, loss_rows, d_logits: FP32_ERR is the worst error, over the cases below, of the fp32
    evaluation of the reference against its fp64 evaluation on these same inputs; the error of a tensor is tests/unit_ref.py's rel_err
    (max |got - ref| over that tensor's largest |ref|). FACTOR = 8 covers another summation order and another exp / log.
    The clip that holds the planted +80 / -80 is compared on `loss` only (bar_errors): in loss_rows and d_logits it would set the scale
    rel_err divides by (160 nats under CE) for every other clip of its case.
    pred, label_frame and counts have NO bar: the inputs are fp32 numbers and the fp64 reference compares those same numbers, so a correct
    kernel matches each of them exactly. dist is exact at T = 16 (the product (span / 16) * pred is exact, so a fused multiply-subtract
    rounds as the separate operations do) and within DIST_TOL relative elsewhere (one extra fp64 rounding); dist_sum is within DIST_TOL
    relative (summation order).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.unit_ref import rel_err  # noqa: F401  (the metric of the bars; re-exported for the tests)

F64 = torch.float64
FACTOR = 8.0
DIST_TOL = 1e-12
KINDS = ("loss", "loss_rows", "d_logits")
EXACT = ("pred", "label_frame", "counts")
# Measured by tests/test_cpu_keyframe.py (test_fp32_reference_meets_the_bar prints them with -s): worst error (bar_errors below) of the fp32
# evaluation over ALL the cases, one constant per tensor (the rule of seg_ce_ref.py: a constant per loss kind would rest on a handful of
# rows each). The CPU test holds each constant to the value it measures (within 3x either way: another CPU's vector width changes torch's
# fp32 summation order), so a bar cannot be widened by editing the constant alone.
FP32_ERR = {"loss": 1.0e-7, "loss_rows": 1.3e-7, "d_logits": 1.7e-7}
BAR = {k: FACTOR * e for k, e in FP32_ERR.items()}
# Worst (smallest) error / bar of each perturbed reference over the cases it changes without changing an exact result, as
# test_cpu_keyframe.py measures them (it requires >= 3), or "exact" where the perturbation shows in pred / counts / dist on every such case.
PERTURB_RATIO = {"mean_over_B": 1.9e7, "ce_over_n_sc": 3.1e5, "mask_ignored": "exact", "dist_over_16": "exact", "ties_high": "exact",
                 "cols_plus_1": "exact"}
PERTURBATIONS = tuple(PERTURB_RATIO)

COLS16 = (41, 7, 300, 12, 588, 64, 65, 129, 2, 500, 333, 592, 100, 256, 77, 450)       # the vocabulary columns of '0' .. '15': scattered
# (B, T, ld, cols, V, kind, flags). Without cols V = T. The kernel gives a workgroup max(4, ceil(B / 64)) clips: B = 5 is one clip above a
# workgroup's 4, B = 257 is 52 workgroups of 5 clips (a wave takes two of them) with the last one short.
CASES = [
    (1, 1, 1, None, 1, "bce", ""),                  # one clip, one frame
    (1, 1, 1, None, 1, "ce", ""),                   # ... under CE: loss 0, gradient 0
    (3, 2, 2, None, 2, "ce", ""),                   # the OSCC-like shape
    (5, 16, 16, None, 16, "bce", ""),               # the recipe, B no multiple of the four waves, one clip above a workgroup's rows
    (5, 16, 16, None, 16, "ce", ""),
    (4, 16, 16, None, 16, "ce", "sc0"),             # no state-change clip at all: distance 0.0, accuracy nan, loss 0
    (4, 16, 16, None, 16, "bce", "sc0"),
    (6, 63, 63, None, 63, "bce", ""),               # one lane short of a wave
    (6, 64, 64, None, 64, "ce", ""),                # a full wave
    (6, 64, 64, None, 64, "bce", ""),
    (2, 17, 20, None, 17, "bce", ""),               # ld > T: gap columns get a zero gradient and do not matter
    (2, 17, 20, None, 17, "ce", ""),
    (257, 16, 16, None, 16, "bce", ""),             # the cross-workgroup sum: 52 workgroups, two clips per wave, a short last workgroup
    (257, 16, 16, None, 16, "ce", ""),
    (4, 3, 12, (9, 2, 5), 11, "ce", ""),            # a loss through cols, V < ld: the gradient lands on the frames' columns only
    (5, 16, 593, COLS16, 593, "metric", ""),        # the EgoT2-g PNR metric
    (5, 2, 593, (7, 3), 593, "metric", ""),         # the EgoT2-g OSCC metric: descending column order, the label is the state-change label
    (5, 16, 16, None, 16, "ce", "label"),           # CE against `label` with target NULL; one label outside [0, T): no loss, no gradient
]


def case_id(case) -> str:
    B, T, ld, cols, V, kind, flags = case
    return f"B{B}_T{T}_ld{ld}_{kind}" + ("_cols" if cols is not None else "") + (f"_{flags}" if flags else "")


def kf_inputs(case_index: int) -> dict:
    """-> logits (B, ld) fp32, target (B, T) fp32 or None, label (B,) int64 or None, state_change (B,) int64 or None, fps (B,) fp64,
    info {clip_start_frame, clip_end_frame, pnr_frame} int64: seeded 3 * randn (gap columns included: they must not matter) with, where the
    case has the rows for them, planted
      * row 0: two equal maxima (the lower frame wins), a state-change clip, fps 29.97,
      * row 1: the maximum at frame 0, state_change 0,
      * row 2: the maximum at frame T - 1, clip_end == clip_start,
      * row 3: a row holding +80 and -80 (loss cases; against a 0 and a 1 target under BCE); a NaN at one frame (metric cases: pred = it),
      * row 4: soft targets 0.25 / 0.75 (BCE); a global argmax outside cols (cols cases),
      * flags "sc0": state_change 0 for every clip,
      * flags "label": the label frames as int64 `label`, no target; row 4 is a state-change clip whose label is T (outside [0, T))."""
    B, T, ld, cols, V, kind, flags = CASES[case_index]
    g = torch.Generator(device="cpu").manual_seed(9300 + case_index)
    logits = 3 * torch.randn(B, ld, generator=g)
    fcol = list(cols) if cols is not None else list(range(T))
    frames = torch.randint(0, T, (B,), generator=g)
    sc = torch.randint(0, 2, (B,), generator=g)
    start = torch.randint(0, 100000, (B,), generator=g)
    span = torch.randint(1, 400, (B,), generator=g)
    fps = torch.where(torch.arange(B) % 2 == 0, torch.tensor(29.97, dtype=F64), torch.tensor(30.0, dtype=F64))
    sc[0] = 1
    if B >= 2:
        sc[1] = 0
        logits[1, fcol[0]] = 11.0
    if T >= 2:
        logits[0, fcol[T // 2]] = logits[0, fcol[T - 1]] = 12.5
        frames[0] = T // 2
    if B >= 3:
        logits[2, fcol[T - 1]] = 13.0
        span[2] = 0
        sc[2] = 1
    if B >= 4 and T >= 2:
        if kind == "metric":
            logits[3, fcol[T // 2]] = float("nan")
        else:
            logits[3, fcol[0]], logits[3, fcol[1]] = 80.0, -80.0
            frames[3] = 1                           # BCE: y = 0 against +80 and y = 1 against -80: two terms of 80
        sc[3] = 1
    if flags == "sc0":
        sc[:] = 0
    pnr = start + (span.double() * torch.rand(B, generator=g, dtype=F64)).long()
    target = label = None
    if flags == "label":
        label = frames.clone()
        label[4], sc[4] = T, 1
    elif kind != "metric":
        target = F.one_hot(frames, T).float()
        if kind == "bce" and B >= 5 and T >= 2:
            target[4] = 0
            target[4, 0], target[4, 1] = 0.25, 0.75
    elif T == 2:
        label = sc.clone()                          # oscc_acc: the label is the state-change label, every clip counts
    if cols is not None and B >= 5:
        out = next(c for c in range(V) if c not in fcol)
        logits[4, out] = 50.0
    return {"logits": logits, "target": target, "label": label, "state_change": None if kind == "metric" else sc, "fps": fps,
            "info": {"clip_start_frame": start, "clip_end_frame": start + span, "pnr_frame": pnr}}


def _argmax(v, perturb):
    if perturb == "ties_high":
        return v.numel() - 1 - int(torch.argmax(v.flip(0)))
    return int(torch.argmax(v))


def keyframe_criterion(logits, target, label, state_change, fps, info, T, cols, kind, V=None, perturb=None) -> dict:
    """The step in the dtype of `logits` -> dict: loss (), loss_rows (B,), d_logits (B, ld) = d loss / d logits by autograd (zero where
    nothing depends on a logit) - None for kind "metric" -, pred (B,) int64, label_frame (B,) int64 (-1: none), counts (4,) int64 =
    [n_sc, n_correct, n_outside, B], dist (B,) fp64, dist_sum fp64 (a Python float)."""
    B, ld = logits.shape
    V = ld if V is None else V
    fcol = list(cols) if cols is not None else list(range(T))
    if perturb == "cols_plus_1" and cols is not None:
        fcol = [(c + 1) % V for c in fcol]
    x = logits.detach().clone().requires_grad_(kind != "metric")
    sub = x[:, fcol]
    # ---- the metrics: the reference's loops ----
    pred = torch.zeros(B, dtype=torch.int64)
    label_frame = torch.full((B,), -1, dtype=torch.int64)
    dist = torch.zeros(B, dtype=F64)
    n_sc = n_correct = n_outside = 0
    dist_list = []
    for b in range(B):
        pred_ = _argmax(sub[b].detach(), perturb)
        pred[b] = pred_
        if label is not None:
            label_frame[b] = int(label[b]) if 0 <= int(label[b]) < T else -1      # the header's rule: such a label equals no prediction
        elif target is not None:
            label_frame[b] = int(torch.argmax(target[b]))
        if cols is not None and int(torch.argmax(logits[b, :V])) not in fcol:
            n_outside += 1
        counted = True if state_change is None or perturb == "mask_ignored" else int(state_change[b]) == 1
        if counted:
            n_sc += 1
            if pred_ == int(label_frame[b]):
                n_correct += 1
            start_frame, end_frame = int(info["clip_start_frame"][b]), int(info["clip_end_frame"][b])
            mapped = (end_frame - start_frame) / (16 if perturb == "dist_over_16" else T) * pred_
            gt = int(info["pnr_frame"][b]) - start_frame
            err_sec = abs(mapped - gt) / float(fps[b])
            dist[b] = err_sec
            dist_list.append(err_sec)
    res = {"pred": pred, "label_frame": label_frame, "counts": torch.tensor([n_sc, n_correct, n_outside, B]), "dist": dist,
           "dist_sum": float(sum(dist_list)), "loss": None, "loss_rows": None, "d_logits": None}
    if kind == "metric":
        return res
    # ---- the loss ----
    if kind == "bce":
        y = target.to(logits.dtype)
        term = torch.clamp(-F.logsigmoid(sub), max=100.0) * y + torch.clamp(-F.logsigmoid(-sub), max=100.0) * (1 - y)
        rows = term.sum(1) / T
        loss = term.sum() / B if perturb == "mean_over_B" else term.mean()
    else:
        mask = torch.ones(B, dtype=logits.dtype) if (state_change is None or perturb == "mask_ignored") else (state_change == 1).to(logits.dtype)
        mask = mask * (label_frame >= 0).to(logits.dtype)                         # ... and adds no loss and no gradient
        rows = mask * F.cross_entropy(sub, label_frame.clamp(min=0), reduction="none")
        loss = rows.sum() / max(n_sc, 1) if perturb == "ce_over_n_sc" else rows.mean()
    loss.backward()
    res.update(loss=loss.detach(), loss_rows=rows.detach(), d_logits=x.grad)
    return res


def evaluate(case_index: int, dtype=F64, perturb=None) -> dict:
    B, T, ld, cols, V, kind, flags = CASES[case_index]
    a = kf_inputs(case_index)
    return keyframe_criterion(a["logits"].to(dtype), a["target"], a["label"], a["state_change"], a["fps"], a["info"], T, cols, kind, V, perturb)


def saturated_rows(case_index: int):
    """Rows of case i that hold the planted +80 / -80: their elements are compared on `loss` only."""
    B, T, ld, cols, V, kind, flags = CASES[case_index]
    return [3] if (B >= 4 and T >= 2 and kind != "metric") else []


def bar_errors(got: dict, ref: dict, case_index: int) -> dict:
    """kind -> rel_err of `got` against `ref` for the three barred tensors. The saturated +80 / -80 row is left out of loss_rows and
    d_logits (it stays in loss): its 160-nat nll / 80-nat BCE terms would otherwise be the largest |ref| that rel_err divides by, and
    every other clip of the case would get that much more absolute slack."""
    keep = [b for b in range(ref["loss_rows"].shape[0]) if b not in saturated_rows(case_index)]
    return {"loss": rel_err(got["loss"], ref["loss"]), "loss_rows": rel_err(got["loss_rows"][keep], ref["loss_rows"][keep]),
            "d_logits": rel_err(got["d_logits"][keep], ref["d_logits"][keep])}


def dist_ok(got, ref, T: int) -> bool:
    """dist (B,) fp64 against the reference: exact at T = 16, DIST_TOL relative elsewhere."""
    got, ref = torch.as_tensor(got, dtype=F64), torch.as_tensor(ref, dtype=F64)
    if T == 16:
        return bool(torch.equal(got, ref))
    return bool(((got - ref).abs() <= DIST_TOL * ref.abs()).all())
