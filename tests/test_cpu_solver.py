"""CPU suite of the solver pieces (train.LRSchedule, construct_solver, the host side of egx_lr_update / egx_sgd_step /
egx_adam_step_dev_lr) and of the gate tests/solver_ref.py itself: the bars hold for a correct evaluation and reject the mistakes they are
there to catch."""
import ctypes as C
import math
import os
import subprocess
import sys
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import solver_ref as sr
from tests import unit_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = sr.schedule_cases()


def _schedule(ctor, args):
    from egot2_amd.train import LRSchedule
    return getattr(LRSchedule, ctor)(*args)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_schedule_factor_matches_the_recorded_lr_factory(case):
    """LRSchedule.factor(k) against the real lr_factory's per-step learning rates (BASE_LR = 1: the factors), both parameter groups, 40
    steps, past t_total. Bar: unit_ref.FACTOR x the recorded recursive-vs-closed cosine difference, relative (solver_ref.factor_bar); exact
    where the reference is 0."""
    name, ctor, args, key = case
    ref = sr.fixture()[key]
    s = _schedule(ctor, args)
    worst = 0.0                                                    # largest relative difference over the bar of its step
    assert ref.shape == (sr.fixture()["config"]["steps"], 2) and 0 < sr.factor_bar() < 1e-14
    for k in range(ref.shape[0]):
        f, bar = s.factor(k), sr.factor_bar(ctor, args, k)
        for g in range(2):
            if ref[k, g] == 0.0:
                assert f == 0.0, (name, k, f)
            else:
                worst = max(worst, abs(f - ref[k, g]) / abs(ref[k, g]) / bar)
        assert s.lr_at(k, 3e-4) == 3e-4 * f
    print(f"{name}: worst relative difference / bar {worst:.3f} (bar {sr.factor_bar():.2e}; past T_max {sr.factor_bar(ctor, args, 10 ** 9):.2e})")
    assert worst <= 1.0, (name, worst)
    if ctor in ("warmup_cosine", "warmup_linear") and args[0] > 0:
        assert ref[0, 0] == 0.0                                    # k = 0 of a warm-up
    from egot2_amd.train import LRSchedule
    if ctor == "from_factors":                                     # the LambdaLR route: the same table from the function
        c = sr.fixture()["config"]
        lam = LRSchedule.from_lambda(lambda step: sr.epoch_lr(step / c["steps_in_epoch"], c["epoch_policy"], c["max_epoch"]), len(args[0]))
        assert lam.factors == s.factors and lam.factor(10 ** 6) == s.factors[-1]


PERTURBED = [("index_t", "cosine_warmup"), ("index_t", "cosine"), ("index_t", "linear_warmup"),
             ("no_max", "cosine_warmup_w10_t10"),           # the edge where a guard acts and the result shows: t_total == WARMUP_STEPS
             ("cycles_1", "cosine_warmup"), ("clamp_t_total", "cosine_warmup"), ("clamp_t_total", "cosine_warmup_w10_t10")]


@pytest.mark.parametrize("perturb,case_id", PERTURBED, ids=[f"{p}-{c}" for p, c in PERTURBED])
def test_lr_bound_rejects_a_perturbed_schedule(perturb, case_id):
    """The device bound of tests/test_gpu_solver.py (one fp32 ulp + 2^-50 base_lr) must see each mistake: on at least one recorded step the
    perturbed learning rate misses it by more than 10x (the factor is printed)."""
    name, ctor, args, key = next(c for c in CASES if c[0] == case_id)
    ref = sr.fixture()[key][:, 0]
    base = 1e-4
    ratio = 0.0
    for k in range(len(ref)):
        f = sr.perturbed_factor(ctor, args, k, perturb)
        lr_ref = base * ref[k]
        got = float(np.float32(base * f)) if math.isfinite(f) else math.inf
        err = abs(got - float(np.float32(lr_ref))) if math.isfinite(got) else math.inf
        ratio = max(ratio, err / sr.lr_bound(lr_ref, base))
        # and the unperturbed evaluation meets the bound on the same step
        ok = base * sr.perturbed_factor(ctor, args, k, None)
        assert abs(float(np.float32(ok)) - float(np.float32(lr_ref))) <= sr.lr_bound(lr_ref, base), (name, k)
    print(f"{perturb} on {name}: misses the bound by {ratio:.3g}x")
    assert ratio > 10, (perturb, name, ratio)


def test_sgd_yardstick_and_written_out_update():
    """BAR_SGD's constant: torch.optim.SGD in fp32 against fp64 on the GPU test's own configurations, shapes and gradients (worst
    unit_ref.rel_err over everything), held to the measured value within 3x; sgd_run (the form the perturbations are made on) is
    torch.optim.SGD to fp64 rounding."""
    worst = 0.0
    for ci, cfg in enumerate(sr.SGD_CONFIGS):
        ref = sr.sgd_reference(ci)
        e = sr.worst_rel_err(sr.sgd_torch(cfg, torch.float32)[0], ref)
        worst = max(worst, e)
        assert sr.worst_rel_err(sr.sgd_run(cfg, torch.float64), ref) < 1e-14, cfg
        assert sr.worst_rel_err(sr.sgd_run(cfg, torch.float32), ref) <= sr.BAR_SGD, cfg
    print(f"fp32 torch.optim.SGD against fp64: worst rel_err {worst:.3e}; SGD_FP32_ERR {sr.SGD_FP32_ERR:.3e}; BAR_SGD {sr.BAR_SGD:.3e}")
    assert sr.SGD_FP32_ERR / 3 <= worst <= sr.SGD_FP32_ERR * 3, worst
    assert sr.BAR_SGD == unit_ref.FACTOR * sr.SGD_FP32_ERR


@pytest.mark.parametrize("perturb", ["first_recurrence", "nesterov_swap", "decoupled_wd"])
def test_sgd_bar_rejects_a_perturbed_update(perturb):
    """Each mistake, made in fp64 on every configuration it applies to, misses BAR_SGD (by the printed factor, at least 3 as in unit_ref)."""
    applies = {"first_recurrence": lambda c: c["momentum"] != 0 and c["dampening"] != 0, "nesterov_swap": lambda c: c["nesterov"],
               "decoupled_wd": lambda c: c["momentum"] != 0 and c["weight_decay"] != 0}[perturb]
    small = list(range(len(sr.SGD_SHAPES) - 1))                     # without the 2 M element tensor: the mistake shows on every size
    ratios = []
    for ci, cfg in enumerate(sr.SGD_CONFIGS):
        if applies(cfg):
            ref = sr.sgd_torch(cfg, torch.float64, shapes=small)[0]
            ratios.append(min(unit_ref.rel_err(a, b) for a, b in zip(sr.sgd_run(cfg, torch.float64, perturb, shapes=small), ref)) / sr.BAR_SGD)
    print(f"{perturb}: error / BAR_SGD on its worst tensor and configuration {min(ratios):.3g}")
    assert len(ratios) >= 1 and min(ratios) >= 3, ratios


# ---- the C ABI's host side (no device is touched: every call below is refused, or returns before a launch) ---------------------------------
def _sched(kind, warmup=0, t_total=0, T_max=1, cycles=0.5, factors=None, n=0):
    from egot2_amd import _lib
    return _lib.LrSchedule(kind, warmup, t_total, T_max, cycles, factors, n)


def _refused(lib, rc, *words):
    assert rc != 0
    msg = lib.egx_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_host_refusals_of_the_solver_entry_points(egx_lib):
    from egot2_amd import _lib
    lib = egx_lib
    assert lib.egx_abi_version() == 18 and _lib.EGX_ABI_VERSION == 18
    P = 0x1000                                                    # a non-null marker: never dereferenced on the host
    base = (C.c_double * 16)(*[1e-3] * 16)
    upd = lambda s, step=P, b=base, n=2, out=P: lib.egx_lr_update(C.byref(s) if s is not None else None, step, b, n, out, None)  # noqa: E731
    _refused(lib, upd(None), "null")
    _refused(lib, upd(_sched(0), step=None), "null pointer")
    _refused(lib, upd(_sched(0), b=None), "null pointer")
    _refused(lib, upd(_sched(0), out=None), "null pointer")
    _refused(lib, upd(_sched(5)), "kind 5", "0..4")
    _refused(lib, upd(_sched(-1)), "kind -1")
    _refused(lib, upd(_sched(0), n=0), "n_groups=0", "1..16")
    _refused(lib, upd(_sched(0), n=17), "n_groups=17", "1..16")
    _refused(lib, upd(_sched(2, warmup=-1, t_total=10)), "warmup_steps=-1", ">= 0")
    _refused(lib, upd(_sched(3, warmup=2, t_total=-3)), "t_total=-3", ">= 0")
    _refused(lib, upd(_sched(1, T_max=0)), "T_max=0", ">= 1")
    _refused(lib, upd(_sched(4, factors=P, n=0)), "n=0", "n >= 1")
    _refused(lib, upd(_sched(4, factors=None, n=4)), "n=4", "pointer")

    sgd = lambda p=P, g=P, buf=P, n=8, step=P, lr_dev=None, lr=0.1, mu=0.9, damp=0.0, wd=0.0, nes=0: \
        lib.egx_sgd_step(p, g, buf, n, step, lr_dev, lr, mu, damp, wd, nes, 1.0, None)  # noqa: E731
    _refused(lib, sgd(p=None), "null pointer")
    _refused(lib, sgd(g=None), "null pointer")
    _refused(lib, sgd(step=None), "null step")
    _refused(lib, sgd(lr=-0.1), "lr >= 0")
    _refused(lib, sgd(mu=-0.5), "momentum >= 0")
    _refused(lib, sgd(damp=1.5), "dampening <= 1")
    _refused(lib, sgd(damp=-0.1), "0 <= dampening")
    _refused(lib, sgd(wd=-1e-4), "weight_decay >= 0")
    _refused(lib, sgd(mu=0.0, buf=None, nes=1), "Nesterov", "momentum > 0")
    _refused(lib, sgd(damp=0.1, nes=1), "Nesterov", "dampening == 0")
    _refused(lib, sgd(mu=0.0), "momentum buffer")                  # a buffer without momentum
    _refused(lib, sgd(buf=None), "momentum buffer")                # momentum without a buffer
    assert sgd(n=0) == 0 and sgd(n=0, mu=0.0, buf=None, step=None) == 0

    adam = lambda p=P, g=P, m=P, v=P, n=8, step=P, lr=P, b1=0.9, b2=0.999, eps=1e-8: \
        lib.egx_adam_step_dev_lr(p, g, m, v, n, step, lr, b1, b2, eps, 0.0, 0, 1.0, None)  # noqa: E731
    for kw in ("p", "g", "m", "v", "step", "lr"):
        _refused(lib, adam(**{kw: None}), "null pointer")
    _refused(lib, adam(b1=1.0), "beta")
    _refused(lib, adam(b2=-0.1), "beta")
    _refused(lib, adam(eps=-1.0), "eps")
    assert adam(n=0) == 0


def test_python_classes_refuse_what_torch_refuses():
    from egot2_amd.train import FusedSGD, LRSchedule
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1.0), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            FusedSGD(p, **kw)
    for bad in (lambda: LRSchedule.cosine_annealing(0), lambda: LRSchedule.warmup_cosine(-1, 5), lambda: LRSchedule.warmup_linear(1, -5),
                lambda: LRSchedule.from_factors([]), lambda: LRSchedule("step")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError, match="at most 16"):
        FusedSGD([{"params": [torch.nn.Parameter(torch.zeros(1))]} for _ in range(17)], lr=0.1, schedule=LRSchedule.constant())


class _Net(torch.nn.Module):
    def __init__(self, with_bn):
        super().__init__()
        self.proj = torch.nn.Linear(4, 4)
        if with_bn:
            self.bn1 = torch.nn.BatchNorm1d(4)


def _cfg(method, policy, max_epoch, **solver):
    s = dict(OPTIMIZING_METHOD=method, BASE_LR=1e-4, MOMENTUM=0.9, DAMPENING=0.0, NESTEROV=True, WEIGHT_DECAY=1e-4, LR_POLICY=policy,
             WARMUP_STEPS=500, MAX_EPOCH=max_epoch)
    s.update(solver)
    return NS(SOLVER=NS(**s), BN=NS(WEIGHT_DECAY=0.0))


def test_construct_solver_on_the_reference_solver_blocks():
    """The SOLVER blocks of HOI/configs/recognition/ts_ar.yaml:39-45 (SGD, momentum 0.9, weight decay 1e-4, cosine_warmup, 30 epochs; Nesterov
    and dampening 0 by the defaults) and HOI/configs/lta/ts_lta_4task.yaml:66-72 (Adam, cosine_warmup, 50 epochs)."""
    from egot2_amd.train import FusedAdam, FusedSGD, construct_solver
    net = _Net(with_bn=True)
    opt, sch = construct_solver(net, _cfg("sgd", "cosine_warmup", 30), steps_in_epoch=100)
    assert type(opt) is FusedSGD and opt.schedule is sch
    assert [len(g["params"]) for g in opt.param_groups] == [2, 2] and [g["weight_decay"] for g in opt.param_groups] == [0.0, 1e-4]
    assert all(g["lr"] == 1e-4 and g["momentum"] == 0.9 and g["dampening"] == 0.0 and g["nesterov"] is True for g in opt.param_groups)
    assert (sch.kind, sch.warmup_steps, sch.t_total, sch.cycles) == ("warmup_cosine", 500, 3000, 0.5)

    net = _Net(with_bn=False)                                      # the translators have no "bn" parameter: the first group is empty
    opt, sch = construct_solver(net, _cfg("adam", "cosine_warmup", 50), steps_in_epoch=20)
    assert type(opt) is FusedAdam and [len(g["params"]) for g in opt.param_groups] == [0, 2]
    assert all(g["betas"] == (0.9, 0.999) and g["adamw"] is False and g["lr"] == 1e-4 for g in opt.param_groups)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.0, 1e-4]
    assert (sch.kind, sch.warmup_steps, sch.t_total) == ("warmup_cosine", 500, 1000)

    opt, sch = construct_solver(net, _cfg("adamw", "cosine", 2), steps_in_epoch=7)
    assert opt.param_groups[1]["adamw"] is True and opt.param_groups[1]["weight_decay"] == 1e-4 and (sch.kind, sch.T_max) == ("cosine_annealing", 14)
    assert construct_solver(net, _cfg("sgd", "linear_warmup", 2), 7)[1].kind == "warmup_linear"
    assert construct_solver(net, _cfg("sgd", "cosine", 2), 7, lr_policy="constant")[1].kind == "constant"
    opt, sch = construct_solver(net, _cfg("sgd", "steps_with_relative_lrs", 2), 5, lr_lambda=lambda step: 1.0 / (1 + step))
    assert sch.kind == "table" and sch.factors == [1.0 / (1 + k) for k in range(10)]
    with pytest.raises(ValueError, match="cosine_warmup"):
        construct_solver(net, _cfg("sgd", "steps_with_relative_lrs", 2), 5)
    with pytest.raises(NotImplementedError):
        construct_solver(net, _cfg("rmsprop", "cosine", 2), 5)


@pytest.mark.reference
def test_fixture_reproduces_from_the_live_lr_factory():
    from oracle import ref_harness as rh
    if not rh.reference_available():
        pytest.skip("the reference tree is not available")
    r = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_solver.py"), "--check"], capture_output=True, text=True,
                       cwd=os.path.dirname(HERE), timeout=600)
    assert r.returncode == 0 and "check True max_diff 0.000e+00" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
