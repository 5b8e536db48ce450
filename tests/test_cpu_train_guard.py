"""CPU suite of the clipped / guarded step (ABI v28 additions; train.GradGuard): the gate tests/train_guard_ref.py held to itself - the
yardstick re-measured, each perturbed reference missing its bar, the decision table - and the host side of the new entry points: every
refusal through ctypes before any device work, the constructors' refusals, the exported symbols and the documents."""
from __future__ import annotations

import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import train_guard_ref as gr
from tests import unit_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG_IDS = [gr.config_id(c) for c in gr.CONFIGS]


# ---- the gate on itself ------------------------------------------------------------------------------------------------------------------
def test_written_out_run_is_torch_in_fp64():
    """The fp64 reference of the bars is clip_grad_norm_ + torch.optim: the written-out run agrees with them far below any bar, and counts
    the clipped steps as they do."""
    worst = {False: 0.0, True: 0.0}
    for ci, cfg in enumerate(gr.CONFIGS):
        for mn in [None] + gr.MAX_NORMS:
            ref, stock = gr.reference(ci, mn), gr.run_torch(cfg, torch.float64, mn)
            worst[mn is not None] = max(worst[mn is not None], gr.worst_rel_err(stock, ref))
            assert gr.counts_equal(stock, ref), (gr.config_id(cfg), mn)
    print(f"written-out fp64 run against torch in fp64: worst rel_err {worst[False]:.3g} unclipped, {worst[True]:.3g} clipped")
    assert worst[False] <= 1e-13, worst
    # clipped: the contract's coefficient is an fp32 (2^-24 relative on every gradient, twice that on exp_avg_sq), torch's an fp64
    assert worst[True] <= 2.0 ** -23, worst


def test_max_norms_sit_below_between_and_above_the_step_norms():
    norms = [gr.decision(list(gr.grads(k)))["norm"] for k in range(gr.STEPS)]
    lo, near, hi = gr.MAX_NORMS
    assert lo < min(norms) and hi > max(norms)
    assert 0 < sum(n + 1e-6 > near for n in norms) < gr.STEPS, norms
    for ci in range(len(gr.CONFIGS)):
        assert gr.reference(ci, lo)["clipped"] == gr.STEPS and gr.reference(ci, hi)["clipped"] == 0
        assert 0 < gr.reference(ci, near)["clipped"] < gr.STEPS


def test_yardstick():
    """GUARD_FP32_ERR is what stock clip_grad_norm_ + torch.optim in fp32 on the CPU miss the fp64 reference by (within 3x either way:
    another CPU's vector width changes torch's fp32 summation order), so the bar cannot be widened by editing the constant alone."""
    worst = 0.0
    for ci, cfg in enumerate(gr.CONFIGS):
        for mn in gr.MAX_NORMS:
            e = gr.worst_rel_err(gr.run_torch(cfg, torch.float32, mn), gr.reference(ci, mn))
            print(f"{gr.config_id(cfg)} max_norm {mn}: fp32 rel_err {e:.3g}")
            worst = max(worst, e)
    print(f"measured {worst:.3g}, recorded GUARD_FP32_ERR = {gr.GUARD_FP32_ERR:.3g}, BAR_STEP = {gr.BAR_STEP:.3g}")
    assert gr.GUARD_FP32_ERR / 3 <= worst <= gr.GUARD_FP32_ERR * 3, worst
    assert gr.BAR_STEP == unit_ref.FACTOR * gr.GUARD_FP32_ERR


def test_betas_of_the_cases_are_fp32_numbers_and_the_defaults_have_an_allowance():
    for b in gr.BETAS:
        assert float(np.float32(b)) == b and float(np.float32(1.0) - np.float32(b)) == 1.0 - b and gr.beta_allowance(b) == 0.0
    a1, a2 = (gr.beta_allowance(b) for b in gr.DEFAULT_BETAS)
    print(f"beta_allowance: beta1 = 0.9: {a1:.3g}, beta2 = 0.999: {a2:.3g} (BAR_STEP {gr.BAR_STEP:.3g})")
    assert 1e-7 < a1 < 1e-6 and 1.2e-5 < a2 < 1.4e-5
    # torch's own fp32 Adam forms 1 - beta in fp64: at the default betas it stays inside the yardstick's 3x window
    for ci in range(3):
        e = gr.worst_rel_err(gr.run_torch(gr.CONFIGS[ci], torch.float32, 85.0, betas=gr.DEFAULT_BETAS), gr.reference(ci, 85.0, betas=gr.DEFAULT_BETAS))
        assert e <= 3 * gr.GUARD_FP32_ERR, e


def test_decision_table():
    d = {cid: gr.decision(bufs, mn) for cid, bufs, mn in gr.decision_cases()}
    assert d["over"]["coef"] < 1 and d["over"]["clipped"] and d["over"]["apply"]
    assert d["under"]["coef"] == np.float32(1.0) and not d["under"]["clipped"]
    assert d["none"]["coef"] == np.float32(1.0) and d["none"]["apply"]
    assert d["zeros"]["norm"] == 0.0 and d["zeros"]["coef"] == np.float32(1e-7 / 1e-6)
    assert d["huge"]["finite"] and d["huge"]["apply"] and d["huge"]["norm"] > gr.FLT_MAX and 0 < d["huge"]["coef"] < 1e-29
    for val in gr.PLANT_VALUES:
        for cid, sizes, bi, ei in gr.plant_cases():
            bufs = [torch.ones(n) for n in sizes]
            bufs[bi][ei] = val
            for mn in (None, 1.0):
                skip, keep = gr.decision(bufs, mn, True), gr.decision(bufs, mn, False)
                assert not skip["finite"] and not skip["apply"] and not skip["clipped"], (cid, val)
                assert keep["apply"], (cid, val)
                if mn is None or math.isnan(val):
                    assert keep["coef"] == np.float32(1.0), (cid, val, mn)        # a NaN norm fails the comparison c < 1
                else:
                    assert keep["coef"] == np.float32(0.0), (cid, val, mn)        # clip_grad_norm_'s formula at an infinite norm
    # 3e38 squared is finite in fp64 and so is the sum of 2^31 of them: a finite gradient is never skipped
    assert math.isfinite((3.4028234663852886e38 ** 2) * 2.0 ** 40)


@pytest.mark.parametrize("perturb", ["no_clamp", "no_eps", "first_buffer", "abs_sum"])
def test_perturbed_decisions_miss_their_bars(perturb):
    caught = []
    for cid, bufs, mn in gr.decision_cases():
        ref, bad = gr.decision(bufs, mn), gr.decision(bufs, mn, perturb=perturb)
        n_total = sum(b.numel() for b in bufs)
        ok = gr.norm_ok(bad["norm"], ref["norm"], n_total) and gr.coef_ok(bad["coef"], ref["coef"])
        assert gr.norm_ok(ref["norm"], ref["norm"], n_total) and gr.coef_ok(ref["coef"], ref["coef"])
        if not ok:
            caught.append(cid)
    print(f"{perturb}: rejected on {caught}")
    want = {"no_clamp": "under", "no_eps": "tiny", "first_buffer": "two", "abs_sum": "over"}[perturb]
    assert want in caught, caught
    if perturb == "no_eps":
        assert "zeros" in caught, caught


@pytest.mark.parametrize("perturb", ["no_clamp", "no_eps", "first_buffer", "abs_sum"])
def test_perturbed_decisions_move_the_steps_past_the_bar(perturb):
    """The same mistakes through six clipped steps: error / BAR_STEP >= 3 on some configuration's worst tensor wherever the mistake changes a
    coefficient at all (no_eps changes it by 1e-8 at these norms: it is the decision bars' to catch, not this one's)."""
    ratios = []
    for ci, cfg in enumerate(gr.CONFIGS):
        for mn in gr.MAX_NORMS:
            ratios.append(gr.worst_rel_err(gr.run(cfg, torch.float64, mn, perturb=perturb), gr.reference(ci, mn)) / gr.BAR_STEP)
    print(f"{perturb}: largest error / BAR_STEP {max(ratios):.3g}")
    if perturb == "no_eps":
        assert max(ratios) < 1
    else:
        assert max(ratios) >= 3, ratios


@pytest.mark.parametrize("perturb", ["skip_advances_step", "skip_decays_exp_avg"])
@pytest.mark.parametrize("ci", range(len(gr.CONFIGS)), ids=CONFIG_IDS)
def test_perturbed_skips_are_rejected(perturb, ci):
    """A skipped step that still advances the count is caught by the exact comparison of the counts (and, for Adam, by the parameters through
    the bias correction); one that still decays exp_avg / the momentum buffer by that tensor's bar."""
    cfg = gr.CONFIGS[ci]
    ref = gr.reference(ci, 85.0, (2,))
    assert ref["skipped"] == 1 and ref["step"] == gr.STEPS - 1 and ref["steps"] == gr.STEPS
    bad = gr.run(cfg, torch.float64, 85.0, (2,), perturb=perturb)
    ratio = gr.worst_rel_err(bad, ref) / gr.BAR_STEP
    print(f"{perturb} {gr.config_id(cfg)}: error / BAR_STEP {ratio:.3g}, counts equal {gr.counts_equal(bad, ref)}")
    if perturb == "skip_advances_step":
        assert not gr.counts_equal(bad, ref)
        if cfg["kind"] == "adam":
            assert ratio >= 3, ratio
    elif ref["state"]:
        assert ratio >= 3, ratio
    else:
        assert ratio == 0.0                     # SGD without momentum has nothing to decay


def test_norm_bar_is_the_derived_one():
    assert gr.norm_bar(1) == 2.0 ** -52 and gr.norm_bar(4099) == 4099 * 2.0 ** -52 and gr.norm_bar(0) == 2.0 ** -52
    x = gr.spread_values(4099, 3)
    mags = x.abs().double()
    assert mags.min() >= 1e-20 * 0.99 and mags.max() <= 1e19 * 1.01 and mags.max() / mags.min() > 1e30
    # any order of the fp64 sum stays inside the bar: ascending, descending and torch's own
    sq = x.double() ** 2
    ref = math.sqrt(math.fsum(sq.tolist()))
    for order in (sq.sort().values, sq.sort(descending=True).values, sq):
        s = 0.0
        for t in order.tolist():
            s += t
        assert gr.norm_ok(math.sqrt(s), ref, x.numel())
    assert gr.sizes_for(gr.TABLE + 1)[1] == 0 and len(gr.sizes_for(gr.TABLE + 1)) == gr.TABLE + 1 and gr.sizes_for(1) == [1]


# ---- the C ABI's host side (no device is touched: every call below is refused before a launch) ------------------------------------------------
def _refused(lib, rc, *words):
    assert rc != 0
    msg = lib.egx_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_host_refusals_of_the_guard_entry_points(egx_lib):
    from egot2_amd import _lib
    lib = egx_lib
    assert lib.egx_abi_version() == 18 and _lib.EGX_ABI_VERSION == 18 and _lib.EGX_GRAD_NORM_TABLE == gr.TABLE
    assert C.sizeof(_lib.GuardBlock) == 40 and _lib.GuardBlock.coef.offset == 8 and _lib.GuardBlock.apply.offset == 12 and \
        _lib.GuardBlock.steps.offset == 16 and _lib.GuardBlock.clipped.offset == 32
    P = 0x1000                                                    # a non-null marker: never dereferenced on the host
    ns = (C.c_size_t * 3)(5, 0, 1025)
    bufs = (C.c_void_p * 3)(P, None, P + 0x100)                   # an empty buffer may be a null pointer
    cfg = _lib.GradNormCfg(1.0, 1, 1)
    need = lib.egx_grad_norm_scratch_bytes(ns, 3)
    assert need >= 8 * 3 and need % 8 == 0
    assert lib.egx_grad_norm_scratch_bytes(None, 3) == 0 and lib.egx_grad_norm_scratch_bytes(ns, 0) == 0
    # one workgroup per 1024 elements up to the cap of 2048 per grouped launch; a 33rd buffer opens a second launch
    one = lambda n: lib.egx_grad_norm_scratch_bytes((C.c_size_t * 1)(n), 1)  # noqa: E731
    assert one(gr.GRID_CAP_ELEMS) == one(gr.GRID_CAP_ELEMS + 4) == one(1 << 33) == 2048 * 8
    assert one(0) == one(1) == one(1024) == 256 and one(1024 * 32 + 1) == align256(33 * 8)
    big = (C.c_size_t * 33)(*[1 << 30] * 33)
    assert lib.egx_grad_norm_scratch_bytes(big, 32) == 2048 * 8 and lib.egx_grad_norm_scratch_bytes(big, 33) == 2 * 2048 * 8

    def norm(b=bufs, n=ns, k=3, scratch=P, nbytes=need, c=cfg, guard=P):
        return lib.egx_grad_norm(b, n, k, scratch, nbytes, C.byref(c) if c is not None else None, guard, None)
    _refused(lib, norm(b=None), "null pointer")
    _refused(lib, norm(n=None), "null pointer")
    _refused(lib, norm(scratch=None), "null pointer")
    _refused(lib, norm(guard=None), "null pointer")
    _refused(lib, norm(c=None), "null pointer", "cfg")
    _refused(lib, norm(k=0), "n_bufs = 0", "n_bufs >= 1")
    _refused(lib, norm(k=-2), "n_bufs = -2")
    _refused(lib, norm(nbytes=need - 1), f"{need - 1} bytes", str(need))
    _refused(lib, norm(c=_lib.GradNormCfg(-0.5, 1, 1)), "max_norm = -0.5", ">= 0")
    _refused(lib, norm(c=_lib.GradNormCfg(math.nan, 1, 1)), "max_norm", "NaN")
    _refused(lib, norm(b=(C.c_void_p * 3)(P, None, P + 0x102)), "buffer 2", "4-byte aligned")
    _refused(lib, norm(b=(C.c_void_p * 3)(P + 1, None, P)), "buffer 0", "4-byte aligned")
    _refused(lib, norm(b=(C.c_void_p * 3)(None, None, P)), "null pointer", "buffer 0")       # 5 elements behind a null pointer

    _refused(lib, lib.egx_counter_add_gated(None, 1, P, None), "null pointer")
    _refused(lib, lib.egx_counter_add_gated(P, 1, None, None), "null pointer")
    base = (C.c_double * 16)(*[1e-3] * 16)
    sched = _lib.LrSchedule(0, 0, 0, 1, 0.5, None, 0)
    upd = lambda s=sched, step=P, n=2, out=P, guard=P: lib.egx_lr_update_gated(C.byref(s) if s is not None else None, step, base, n, out, guard, None)  # noqa: E731
    _refused(lib, upd(s=None), "null")
    _refused(lib, upd(guard=None), "null pointer", "guard")
    _refused(lib, upd(step=None), "null pointer")
    _refused(lib, upd(n=17), "n_groups=17", "1..16")
    _refused(lib, upd(s=_lib.LrSchedule(1, 0, 0, 0, 0.5, None, 0)), "T_max=0")

    adam = lambda p=P, g=P, m=P, v=P, n=8, step=P, lr_dev=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, guard=P: \
        lib.egx_adam_step_guarded(p, g, m, v, n, step, lr_dev, lr, b1, b2, eps, 0.0, 0, guard, None)  # noqa: E731
    for kw in ("p", "g", "m", "v", "step", "guard"):
        _refused(lib, adam(**{kw: None}), "null pointer")
    _refused(lib, adam(lr=-1.0), "lr >= 0")
    _refused(lib, adam(b1=1.0), "beta")
    _refused(lib, adam(eps=-1.0), "eps")
    assert adam(n=0) == 0 and adam(n=0, lr_dev=P, lr=-1.0) == 0

    sgd = lambda p=P, g=P, buf=P, n=8, step=P, lr=0.1, mu=0.9, nes=0, guard=P: \
        lib.egx_sgd_step_guarded(p, g, buf, n, step, None, lr, mu, 0.0, 0.0, nes, guard, None)  # noqa: E731
    _refused(lib, sgd(guard=None), "null pointer", "guard")
    _refused(lib, sgd(p=None), "null pointer")
    _refused(lib, sgd(lr=-0.1), "lr >= 0")
    _refused(lib, sgd(mu=0.0, buf=None, nes=1), "Nesterov")
    _refused(lib, sgd(buf=None), "momentum buffer")
    assert sgd(n=0) == 0


def align256(x: int) -> int:
    return (x + 255) // 256 * 256


def test_python_classes_refuse_bad_guards():
    from egot2_amd.train import FusedAdam, FusedSGD, GradGuard, grad_norm
    for bad in (-1.0, -1e-30, math.nan):
        with pytest.raises(ValueError, match="max_norm"):
            GradGuard(max_norm=bad)
    for bad in ("1.0", True, [1.0]):
        with pytest.raises(TypeError, match="max_norm"):
            GradGuard(max_norm=bad)
    with pytest.raises(TypeError, match="skip_nonfinite"):
        GradGuard(skip_nonfinite=1)
    g = GradGuard(max_norm=0)
    assert g.max_norm == 0.0 and g.skip_nonfinite is True and GradGuard().max_norm is None
    assert g.result() == {"grad_norm": 0.0, "clip_coef": 1.0, "applied": 1, "steps": 0, "skipped": 0, "clipped": 0}
    with pytest.raises(RuntimeError, match="no step"):
        g.block
    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls in (FusedAdam, FusedSGD):
        with pytest.raises(TypeError, match="guard"):
            cls(p, guard=1.0)
        with pytest.raises(TypeError, match="guard"):
            cls(p, guard=dict(max_norm=1.0))
        opt = cls(p, guard=g)
        assert opt.guard is g and opt.guard_result()["steps"] == 0
        with pytest.raises(RuntimeError, match="without a guard"):
            cls(p).guard_result()
        assert "guard" not in opt.state_dict()["param_groups"][0] and not opt.state_dict()["state"]
    p[0].grad = torch.zeros(3)
    with pytest.raises(ValueError, match="GPU"):
        grad_norm(p)                                 # a CPU gradient: refused before the library is asked
    with pytest.raises(ValueError, match="no parameter"):
        grad_norm([torch.nn.Parameter(torch.zeros(2))])


def test_construct_solver_hands_the_guard_on():
    from types import SimpleNamespace as NS
    from egot2_amd.train import GradGuard, construct_solver
    model = torch.nn.Sequential(torch.nn.Linear(3, 2))
    g = GradGuard(max_norm=2.0)
    for method in ("sgd", "adam", "adamw"):
        cfg = NS(SOLVER=NS(OPTIMIZING_METHOD=method, BASE_LR=0.1, MOMENTUM=0.9, DAMPENING=0.0, NESTEROV=True, WEIGHT_DECAY=1e-4, LR_POLICY="constant",
                           WARMUP_STEPS=0, MAX_EPOCH=1), BN=NS(WEIGHT_DECAY=0.0))
        opt, _ = construct_solver(model, cfg, 4, guard=g)
        assert opt.guard is g
        assert construct_solver(model, cfg, 4)[0].guard is None


def test_symbols_header_and_documents(egx_lib):
    from egot2_amd import _lib
    new = ["egx_grad_norm_scratch_bytes", "egx_grad_norm", "egx_counter_add_gated", "egx_lr_update_gated", "egx_adam_step_guarded",
           "egx_sgd_step_guarded"]
    hdr = open(os.path.join(ROOT, "include", "egot2x.h")).read()
    assert "ABI v28 additions" in hdr and re.search(r"#define EGX_ABI_VERSION 18\b", hdr)
    tail = hdr[hdr.index("ABI v28 additions"):]
    for name in new:
        assert hasattr(egx_lib, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b" + name + r"\s*\(", tail), name
    for word in ("egx_guard_block", "egx_grad_norm_cfg", "EGX_GRAD_NORM_TABLE 32", "fixed order", "apply"):
        assert word in tail, word
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Clipping and the non-finite guard in a captured step" in integ
    sect = integ[integ.index("Clipping and the non-finite guard in a captured step"):]
    for word in ("allreduce_gradients", "EgxComm", "GradGuard", "same decision"):
        assert word in sect, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    for word in ("grad_guard.hip", "test_gpu_train_guard.py", "train_guard_eval.py"):
        assert word in readme, word
