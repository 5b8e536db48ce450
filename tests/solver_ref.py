"""The gate of tests/test_cpu_solver.py and tests/test_gpu_solver.py: cases, bars and fp64 references of the on-device learning-rate
schedules (egx_lr_update, train.LRSchedule) and of the fused SGD (egx_sgd_step, train.FusedSGD).

Plain Python / torch on the CPU; nothing here is imported from the product path. `perturb=` names one deliberate mistake; the CPU tests
check that the bars reject each of them.

Schedules
    The references are the recordings of the reference's lr_factory in tests/golden/live/solver_schedules.npz (make_golden_solver.py): at
    BASE_LR = 1 the recorded learning rates are the factors f(k) themselves, k the 0-based update index.
    Host bar (LRSchedule.factor): |f - ref| <= factor_bar * |ref|, factor_bar = unit_ref.FACTOR * the recorded relative difference between
    torch's recursive CosineAnnealingLR and the closed form at T = 50 000 (plus, past T_max only, the rounding of torch's restart step:
    factor_bar's docstring); exactly 0 where the reference is exactly 0.
    Device bound (lr_bound): |lr_dev - fp32(lr_ref)| <= 2^-23 |lr_ref| + 2^-50 base_lr: one fp32 ulp plus the fp64 rounding of the factor
    at a zero of the cosine.
SGD
    sgd_run() is torch.optim.SGD's update written out (checked against torch.optim.SGD itself by the CPU test), in the dtype asked for, on
    the gradients of sgd_grads(): fp64 gives the reference, fp32 the yardstick. BAR_SGD = unit_ref.FACTOR * SGD_FP32_ERR, the worst
    unit_ref.rel_err of the fp32 run against the fp64 run over SGD_CONFIGS and the tensors of SGD_SHAPES after SGD_STEPS steps.
"""
from __future__ import annotations

import functools
import json
import math
import os

import numpy as np
import torch

from tests import unit_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "live", "solver_schedules.npz")


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(FIXTURE)
    return {k: (json.loads(str(z[k])) if k == "config" else z[k]) for k in z.files}


def factor_bar(ctor: str = "", args=(), k: int = 0) -> float:
    """Relative bar of LRSchedule.factor(k) against the recording. Past T_max the recorded CosineAnnealingLR no longer is the closed form to
    rounding: torch restarts its recursion at k = T_max + 1 from lr + (1 - cos(pi / T_max)) / 2, a subtraction that carries half an ulp of 1
    (2^-53) on a quantity of size 1 - cos(pi / T_max), and every later step of that period inherits this relative error (T_max = 30: 2.0e-14).
    That is the recording's own error, so it is added to the measured difference there - and only there."""
    own = float(fixture()["cosine_recursive_vs_closed_T50000"])
    if ctor == "cosine_annealing" and k > args[0]:
        own += 2.0 ** -53 / (1.0 - math.cos(math.pi / args[0]))
    return unit_ref.FACTOR * own


def lr_bound(lr_ref: float, base_lr: float) -> float:
    return 2.0 ** -23 * abs(lr_ref) + 2.0 ** -50 * base_lr


def epoch_lr(cur_epoch: float, ep: dict, max_epoch: int) -> float:
    """The `steps_with_relative_lrs` policy with its warm-up, as the fixture's config sets it (our restatement of what get_epoch_lr
    computes: the LRS entry of the last STEPS boundary at or below the epoch; below WARMUP_EPOCHS a line from WARMUP_START_LR to the
    policy's value at WARMUP_EPOCHS)."""
    def at(e):
        bounds = ep["STEPS"] + [max_epoch]
        ind = 0
        for ind, b in enumerate(bounds):
            if e < b:
                break
        return ep["LRS"][max(ind - 1, 0)]
    lr = at(cur_epoch)
    if cur_epoch < ep["WARMUP_EPOCHS"]:
        alpha = (at(ep["WARMUP_EPOCHS"]) - ep["WARMUP_START_LR"]) / ep["WARMUP_EPOCHS"]
        lr = cur_epoch * alpha + ep["WARMUP_START_LR"]
    return lr


def schedule_cases():
    """-> [(case id, LRSchedule constructor name, its arguments, fixture key)]: every kind on the main configuration, the warm-up kinds on
    the edge configurations (WARMUP_STEPS 0 and 1, t_total == WARMUP_STEPS)."""
    c = fixture()["config"]
    t_total, w = c["max_epoch"] * c["steps_in_epoch"], c["warmup_steps"]
    ep = c["epoch_policy"]
    table = [epoch_lr(k / c["steps_in_epoch"], ep, c["max_epoch"]) for k in range(t_total)]
    cases = [("cosine", "cosine_annealing", (t_total,), "lr_cosine"), ("constant", "constant", (), "lr_constant"),
             ("cosine_warmup", "warmup_cosine", (w, t_total), "lr_cosine_warmup"), ("linear_warmup", "warmup_linear", (w, t_total), "lr_linear_warmup"),
             ("table", "from_factors", (table,), "lr_steps_with_relative_lrs")]
    for policy, ctor in (("cosine_warmup", "warmup_cosine"), ("linear_warmup", "warmup_linear")):
        for we, e in c["edges"]:
            t = e * c["steps_in_epoch"]
            cases.append((f"{policy}_w{we}_t{t}", ctor, (we, t), f"edge_{policy}_w{we}_t{t}"))
    return cases


def perturbed_factor(ctor: str, args, k: int, perturb: str) -> float:
    """f(k) of a warm-up kind (or cosine annealing for "index_t") with one mistake:
    index_t        evaluated at the 1-based count t = k + 1 instead of k = t - 1
    no_max         the max(1, .) guards of the denominators dropped (a zero denominator gives inf / nan, as the division would on the device)
    cycles_1       cycles = 1 instead of 0.5 (cosine warm-up)
    clamp_t_total  k clamped at t_total"""
    if ctor == "cosine_annealing":
        kk = k + 1 if perturb == "index_t" else k
        return 0.5 * (1.0 + math.cos(math.pi * kk / args[0]))
    w, t_total = args
    guard = (lambda x: x) if perturb == "no_max" else (lambda x: max(1, x))
    div = lambda a, b: a / b if b != 0 else (math.nan if a == 0 else math.copysign(math.inf, a))  # noqa: E731
    if perturb == "index_t":
        k = k + 1
    if perturb == "clamp_t_total":
        k = min(k, t_total)
    if k < w:
        return div(float(k), float(guard(w)))
    if ctor == "warmup_linear":
        return max(0.0, div(float(t_total - k), float(guard(t_total - w))))
    progress = div(float(k - w), float(guard(t_total - w)))
    x = math.pi * (1.0 if perturb == "cycles_1" else 0.5) * 2.0 * progress
    return max(0.0, 0.5 * (1.0 + (math.cos(x) if math.isfinite(x) else math.nan)))


# ---- SGD -----------------------------------------------------------------------------------------------------------------------------------
SGD_STEPS = 8
SGD_LR = 0.05
SGD_GRID_CAP_ELEMS = 2048 * 256 * 4           # sgd_kernel: at most 2048 workgroups of 256 threads, 4 elements a thread, striding over the rest
# the first three take their gradients as unaligned views of one shared buffer; then the n % 4 tails, several workgroups, a 2-D tensor, and one
# thread's worth beyond the grid cap
SGD_SHAPES = [(1023,), (1024,), (1025,), (1,), (3,), (4,), (5,), (4099,), (2048, 128), (SGD_GRID_CAP_ELEMS + 4,)]
SGD_MODES = [dict(momentum=0.0, dampening=0.0, nesterov=False), dict(momentum=0.9, dampening=0.0, nesterov=False),
             dict(momentum=0.9, dampening=0.0, nesterov=True), dict(momentum=0.9, dampening=0.1, nesterov=False)]
SGD_WDS = [0.0, 1e-4, 5e-2]
SGD_CONFIGS = [dict(m, weight_decay=wd) for m in SGD_MODES for wd in SGD_WDS]
# Measured by tests/test_cpu_solver.py::test_sgd_yardstick (printed with -s), which holds the constant to what it measures within 3x either way.
SGD_FP32_ERR = 2.7e-7
BAR_SGD = unit_ref.FACTOR * SGD_FP32_ERR


def sgd_config_id(c) -> str:
    return f"mu{c['momentum']}_d{c['dampening']}_n{int(c['nesterov'])}_wd{c['weight_decay']}"


@functools.lru_cache(maxsize=None)
def sgd_params():
    g = torch.Generator(device="cpu").manual_seed(4100)
    return tuple(torch.randn(s, generator=g) for s in SGD_SHAPES)


@functools.lru_cache(maxsize=None)
def sgd_grads(step: int):
    """-> (flat, grads): fp32 gradients of step `step`; the first three are views of `flat` at offsets 3, 3 + n0 + 1, ... (not 16-byte aligned)."""
    g = torch.Generator(device="cpu").manual_seed(4200 + step)
    n3 = [torch.Size(s).numel() for s in SGD_SHAPES[:3]]
    flat = torch.randn(3 + sum(n + 1 for n in n3), generator=g)
    grads, off = [], 3
    for i, s in enumerate(SGD_SHAPES):
        if i < 3:
            grads.append(flat[off:off + n3[i]].view(s))
            off += n3[i] + 1
        else:
            grads.append(torch.randn(s, generator=g))
    return flat, tuple(grads)


def sgd_grad_offsets():
    n3 = [torch.Size(s).numel() for s in SGD_SHAPES[:3]]
    offs, off = [], 3
    for n in n3:
        offs.append(off)
        off += n + 1
    return offs


def sgd_run(cfg: dict, dtype, perturb=None, steps: int = SGD_STEPS, lr=SGD_LR, shapes=None):
    """torch.optim.SGD's update written out, `steps` steps in `dtype` -> list of parameters. `lr`: a number or a function of the 0-based step.
    perturb: first_recurrence (the first update goes through buf = mu * 0 + (1 - dampening) g instead of buf = g), nesterov_swap
    (g = buf where Nesterov takes g + mu buf), decoupled_wd (p *= 1 - lr wd in place of g += wd p)."""
    mu, damp, nes, wd = cfg["momentum"], cfg["dampening"], cfg["nesterov"], cfg["weight_decay"]
    idx = range(len(SGD_SHAPES)) if shapes is None else shapes
    ps = [sgd_params()[i].to(dtype).clone() for i in idx]
    bufs = [None] * len(ps)
    for t in range(steps):
        lr_t = lr(t) if callable(lr) else lr
        grads = [sgd_grads(t)[1][i] for i in idx]
        for j, (p, g32) in enumerate(zip(ps, grads)):
            g = g32.to(dtype)
            if perturb == "decoupled_wd":
                p.mul_(1 - lr_t * wd)
            elif wd != 0:
                g = g + wd * p
            if mu != 0:
                if bufs[j] is None:
                    bufs[j] = (1 - damp) * g if perturb == "first_recurrence" else g.clone()
                else:
                    bufs[j] = mu * bufs[j] + (1 - damp) * g
                g = bufs[j] if (not nes or perturb == "nesterov_swap") else g + mu * bufs[j]
            p.sub_(lr_t * g)
    return ps


def sgd_torch(cfg: dict, dtype, steps: int = SGD_STEPS, lr: float = SGD_LR, shapes=None):
    """torch.optim.SGD itself on the same inputs (CPU) -> (parameters, optimizer)."""
    idx = range(len(SGD_SHAPES)) if shapes is None else shapes
    ps = [torch.nn.Parameter(sgd_params()[i].to(dtype).clone()) for i in idx]
    opt = torch.optim.SGD(ps, lr=lr, **cfg)
    for t in range(steps):
        for p, i in zip(ps, idx):
            p.grad = sgd_grads(t)[1][i].to(dtype).clone()
        opt.step()
    return [p.detach() for p in ps], opt


def sgd_reference(config_index: int):
    """fp64 torch.optim.SGD after SGD_STEPS steps (each configuration has one user: not cached, the largest tensor is 2 M elements)."""
    return sgd_torch(SGD_CONFIGS[config_index], torch.float64)[0]


def worst_rel_err(got, ref) -> float:
    return max(unit_ref.rel_err(a, b) for a, b in zip(got, ref))
