"""-m gpu: the solver of the captured step - learning-rate schedules evaluated on the device (egx_lr_update), the fused SGD (egx_sgd_step,
train.FusedSGD), Adam with its learning rate in device memory (egx_adam_step_dev_lr) and all of it under train.GraphedStep. Cases, bars and
references: tests/solver_ref.py (checked on the CPU by tests/test_cpu_solver.py)."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import solver_ref as sr
from tests import unit_ref
from tests.util import hhi_args, seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu
CASES = sr.schedule_cases()
ADAM_TOL = dict(rtol=2e-5, atol=2e-6)            # test_adam_kernel_semantics's own bar
SMALL = list(range(len(sr.SGD_SHAPES) - 1))      # every shape but the 2 M element one


def _schedule(ctor, args):
    from egot2_amd.train import LRSchedule
    return getattr(LRSchedule, ctor)(*args)


def _gpu_grads(step, cuda, shapes=None):
    """The gradients of solver_ref.sgd_grads(step) on the device, the first three as unaligned views of one shared buffer."""
    flat, grads = sr.sgd_grads(step)
    dflat = flat.to(cuda)
    out = []
    for i in (range(len(grads)) if shapes is None else shapes):
        if i < 3:
            off = sr.sgd_grad_offsets()[i]
            out.append(dflat[off:off + grads[i].numel()].view(grads[i].shape))
        else:
            out.append(grads[i].to(cuda))
    return out


def _gpu_params(cuda, shapes=None):
    return [torch.nn.Parameter(sr.sgd_params()[i].to(cuda)) for i in (range(len(sr.SGD_SHAPES)) if shapes is None else shapes)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_learning_rates_on_the_device(egx_lib, cuda, case):
    """Every schedule kind over the recorded steps of the real lr_factory, two groups of different base learning rates, the vector read back
    after every egx_lr_update: one fp32 ulp plus the fp64 rounding of the factor at a zero of the cosine; exactly 0 where the reference is;
    the step count ends at the number of calls."""
    name, ctor, args, key = case
    ref = sr.fixture()[key]
    schedule = _schedule(ctor, args)               # owns the table's device copy: it has to outlive the calls
    sched = schedule._struct(cuda)
    base = [1e-4, 3e-2]
    step = torch.zeros((), dtype=torch.int64, device=cuda)
    lr = torch.full((2,), -1.0, device=cuda)
    cbase = (C.c_double * 2)(*base)
    stream = torch.cuda.current_stream().cuda_stream
    worst = 0.0
    for k in range(ref.shape[0]):
        assert egx_lib.egx_lr_update(C.byref(sched), step.data_ptr(), cbase, 2, lr.data_ptr(), stream) == 0, egx_lib.egx_last_error()
        got = lr.tolist()
        for g in range(2):
            want = base[g] * ref[k, g]
            if ref[k, g] == 0.0:
                assert got[g] == 0.0, (name, k, g, got[g])
            else:
                err, bound = abs(got[g] - float(np.float32(want))), sr.lr_bound(want, base[g])
                worst = max(worst, err / bound)
                assert err <= bound, (name, k, g, got[g], want)
    print(f"{name}: worst error / bound {worst:.3f}")
    assert int(step.item()) == ref.shape[0]


@pytest.mark.parametrize("ci", range(len(sr.SGD_CONFIGS)), ids=[sr.sgd_config_id(c) for c in sr.SGD_CONFIGS])
def test_sgd_kernel_semantics(egx_lib, cuda, ci):
    """Identical gradients into FusedSGD and torch.optim.SGD in fp64, 8 steps: stand-alone tensors of every n % 4, several workgroups, one
    buffer one thread's worth beyond the grid cap, three gradients that are unaligned views of one shared buffer."""
    from egot2_amd.train import FusedSGD
    cfg = sr.SGD_CONFIGS[ci]
    ps = _gpu_params(cuda)
    opt = FusedSGD(ps, lr=sr.SGD_LR, **cfg)
    for t in range(sr.SGD_STEPS):
        for p, g in zip(ps, _gpu_grads(t, cuda)):
            p.grad = g
        opt.step()
    ref = sr.sgd_reference(ci)
    errs = [unit_ref.rel_err(p.detach().cpu(), r) for p, r in zip(ps, ref)]
    print(f"{sr.sgd_config_id(cfg)}: worst rel_err {max(errs):.3e}, BAR_SGD {sr.BAR_SGD:.3e}")
    for s, e in zip(sr.SGD_SHAPES, errs):
        assert e <= sr.BAR_SGD, (s, e)
    st = opt.state[ps[3]]
    assert int(st["step"].item()) == sr.SGD_STEPS and (("momentum_buffer" in st) == (cfg["momentum"] != 0))
    if cfg["momentum"] != 0:
        assert st["momentum_buffer"].shape == ps[3].shape
    assert len({ps[i].untyped_storage().data_ptr() for i in range(3)}) == 1        # re-pointed behind the shared gradient buffer


@pytest.mark.parametrize("n,shift", [(1029, 0), (1029, 1), (3, 1), (sr.SGD_GRID_CAP_ELEMS + 4, 0)])
def test_sgd_first_update_assigns_the_momentum_buffer(egx_lib, cuda, n, shift):
    """The C entry point alone: a momentum buffer pre-filled with NaN comes back finite after the first update (*step == 1: buf = g, the
    buffer is not read) and is used by the second (the recurrence); `shift` floats off the 16-byte alignment take the scalar kernel."""
    g = torch.Generator().manual_seed(n + shift)
    p0, g0 = torch.randn(n + shift, generator=g), torch.randn(n + shift, generator=g)
    p, gr = p0.to(cuda), g0.to(cuda)
    buf = torch.full((n + shift,), math.nan, device=cuda)
    step = torch.ones((), dtype=torch.int64, device=cuda)
    lr_dev = torch.tensor([0.5, 0.1], device=cuda)
    stream = torch.cuda.current_stream().cuda_stream
    a = lambda t: t.data_ptr() + 4 * shift  # noqa: E731
    assert egx_lib.egx_sgd_step(a(p), a(gr), a(buf), n, step.data_ptr(), lr_dev.data_ptr() + 4, 7.0, 0.9, 0.0, 0.0, 1, 1.0, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[shift:].cpu(), g0[shift:])                               # weight decay 0, grad_scale 1: buf == g bit for bit
    want = p0.double() - 0.1 * (g0.double() + 0.9 * g0.double())                   # lr from the device pointer (0.1), not the 7.0 by value
    assert unit_ref.rel_err(p[shift:].cpu(), want[shift:]) <= sr.BAR_SGD
    if shift:
        assert torch.equal(p[:shift].cpu(), p0[:shift]) and torch.isnan(buf[:shift]).all()      # nothing in front of the window is touched
    step.fill_(2)
    assert egx_lib.egx_sgd_step(a(p), a(gr), a(buf), n, step.data_ptr(), None, 0.1, 0.9, 0.0, 0.0, 1, 1.0, stream) == 0
    b2 = 0.9 * g0.double() + g0.double()
    assert unit_ref.rel_err(buf[shift:].cpu(), b2[shift:]) <= sr.BAR_SGD
    assert unit_ref.rel_err(p[shift:].cpu(), (want - 0.1 * (g0.double() + 0.9 * b2))[shift:]) <= sr.BAR_SGD


@pytest.mark.parametrize("adamw,wd", [(False, 0.0), (False, 0.05), (True, 0.05)])
def test_adam_with_a_device_learning_rate(egx_lib, cuda, adamw, wd):
    """A constant schedule is by-value FusedAdam bit for bit (the same arithmetic, the learning rate read from memory); a warm-up cosine
    follows torch.optim.Adam / AdamW driven by the recorded factors; at k = 0 of the warm-up (lr 0) the parameters do not move and the
    moments do."""
    from egot2_amd.train import FusedAdam, LRSchedule
    kw = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    pa, pb, pc, pd = (_gpu_params(cuda) for _ in range(4))
    oa = FusedAdam(pa, adamw=adamw, **kw)
    ob = FusedAdam(pb, adamw=adamw, schedule=LRSchedule.constant(), **kw)
    oc = FusedAdam(pc, adamw=adamw, schedule=LRSchedule.warmup_cosine(5, 30), **kw)
    od = (torch.optim.AdamW if adamw else torch.optim.Adam)(pd, **kw)
    factors = sr.fixture()["lr_cosine_warmup"][:, 0]
    for t in range(8):
        grads = _gpu_grads(t, cuda)
        for ps in (pa, pb, pc, pd):
            for p, g in zip(ps, grads):
                p.grad = g
        for group in od.param_groups:
            group["lr"] = 1e-2 * factors[t]
        for o in (oa, ob, oc, od):
            o.step()
        if t == 0:
            torch.cuda.synchronize()
            for p, r in zip(pc, sr.sgd_params()):
                assert torch.equal(p.detach().cpu(), r)                                  # lr 0: bitwise unchanged
                assert float(oc.state[p]["exp_avg"].abs().max()) > 0 and float(oc.state[p]["exp_avg_sq"].abs().max()) > 0
            assert oc.current_lr() == [0.0]
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    for x, y in zip(pc, pd):
        assert torch.allclose(x, y, **ADAM_TOL), (x - y).abs().max().item()
    assert ob.current_lr() == [float(np.float32(1e-2))] and oa.current_lr() == [1e-2]


def test_sgd_at_a_zero_learning_rate_keeps_the_parameters_and_fills_the_buffer(egx_lib, cuda):
    """k = 0 of a warm-up: lr = 0 leaves the parameters bitwise unchanged; the momentum buffer is the gradient."""
    from egot2_amd.train import FusedSGD, LRSchedule
    ps = _gpu_params(cuda, SMALL)
    opt = FusedSGD(ps, lr=0.1, momentum=0.9, nesterov=True, schedule=LRSchedule.warmup_cosine(5, 30))
    grads = _gpu_grads(0, cuda, SMALL)
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()
    torch.cuda.synchronize()
    for i, p, g in zip(SMALL, ps, grads):
        assert torch.equal(p.detach().cpu(), sr.sgd_params()[i]) and torch.equal(opt.state[p]["momentum_buffer"], g)
    assert opt.current_lr() == [0.0]


def _torch_only_problem(cuda, seed):
    g = torch.Generator().manual_seed(seed)
    shapes = [(257,), (33, 5)]
    w0 = [torch.randn(s, generator=g) for s in shapes]
    xs = [[torch.randn(s, generator=g).to(cuda) for s in shapes] for _ in range(13)]          # the example batch and twelve more
    loss_of = lambda ws: (lambda *x: sum((w * xi).square().sum() for w, xi in zip(ws, x)))  # noqa: E731
    return w0, xs, loss_of


@pytest.mark.parametrize("which", ["sgd_warmup_cosine", "adam_cosine_annealing"])
def test_schedule_under_graphed_step(egx_lib, cuda, which):
    """GraphedStep over a torch-only loss (exact gradients), twelve replays on different inputs: the parameters follow the eager torch
    optimizer under the torch scheduler; the warm-up steps leave no trace (parameters, step count: the first replay runs f(0)); and the
    same optimizer WITHOUT the schedule, captured the same way, misses the bar - the test sees the schedule."""
    from egot2_amd.train import FusedAdam, FusedSGD, GraphedStep, LRSchedule
    w0, xs, loss_of = _torch_only_problem(cuda, 91)
    new = lambda: [torch.nn.Parameter(w.to(cuda)) for w in w0]  # noqa: E731
    if which == "sgd_warmup_cosine":
        base, sched = 2e-2, LRSchedule.warmup_cosine(5, 10)
        fused = lambda ps, s: FusedSGD(ps, lr=base, momentum=0.9, nesterov=True, weight_decay=1e-4, schedule=s)  # noqa: E731
        wr = new()
        opt_r = torch.optim.SGD(wr, lr=base, momentum=0.9, nesterov=True, weight_decay=1e-4)
        sch_r = torch.optim.lr_scheduler.LambdaLR(opt_r, lambda k: sr.perturbed_factor("warmup_cosine", (5, 10), k, None))
    else:
        base, sched = 1e-2, LRSchedule.cosine_annealing(8)
        fused = lambda ps, s: FusedAdam(ps, lr=base, betas=(0.9, 0.99), schedule=s)  # noqa: E731
        wr = new()
        opt_r = torch.optim.Adam(wr, lr=base, betas=(0.9, 0.99))
        sch_r = torch.optim.lr_scheduler.CosineAnnealingLR(opt_r, 8)
    for x in xs[1:]:
        opt_r.zero_grad(set_to_none=True)
        loss_of(wr)(*x).backward()
        opt_r.step()
        sch_r.step()

    results = {}
    for tag, s in (("scheduled", sched), ("by_value", None)):
        ws = new()
        opt = fused(ws, s)
        step = GraphedStep(loss_of(ws), example_inputs=tuple(xs[0]), params=ws, optimizer=opt, warmup=3)
        torch.cuda.synchronize()
        assert all(torch.equal(w.detach().cpu(), v) for w, v in zip(ws, w0)), "the warm-up steps must not leave updates behind"
        assert int(opt._step_dev.item()) == 0
        for x in xs[1:]:
            step(*x)
        torch.cuda.synchronize()
        assert int(opt._step_dev.item()) == 12
        results[tag] = (ws, opt)
    ws, opt = results["scheduled"]
    for a, b in zip(ws, wr):
        assert torch.allclose(a, b, **ADAM_TOL), (which, (a - b).abs().max().item())
    want = sched.lr_at(11, base)
    assert abs(opt.current_lr()[0] - float(np.float32(want))) <= sr.lr_bound(want, base), (opt.current_lr(), want)
    assert not all(torch.allclose(a, b, **ADAM_TOL) for a, b in zip(results["by_value"][0], wr)), "a constant learning rate passes: the test is blind"


CE_W = [0.266, 0.734]


def _ttm(cuda, seed=3):
    from egot2_amd import hhi_ttm
    m = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(dropout=0.0))
    m.pos_embed.dropout.p = 0.0
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.to(cuda).train().set_compute("f32s")


def test_scheduled_sgd_on_the_real_step(egx_lib, cuda):
    """The TTM translator at p = 0, f32s, B = 12: three batches through GraphedStep + FusedSGD + warmup_cosine leave the parameters where
    the eager loop leaves them (FusedSGD by value, the host applying lr_at) within test_graphed_step_helper_follows_the_eager_loop's bars
    (2 lr per step at most, a median of 0.04 lr, losses to 2e-3) at the largest scheduled learning rate; and a scheduled FusedAdam step
    costs as many launches as an unscheduled one."""
    from egot2_amd.train import CrossEntropyLoss, FusedAdam, FusedSGD, GraphedStep, LRSchedule
    crit = CrossEntropyLoss(torch.FloatTensor(CE_W)).to(cuda)
    batches = [([f.to(cuda) for f in seeded_feats(300 + i, [(12, 15, 256)] * 3)],
                torch.randint(0, 2, (12,), generator=torch.Generator().manual_seed(i)).to(cuda)) for i in range(4)]
    loss_of = lambda model: (lambda f, y: crit(model.forward_features(*f), y))  # noqa: E731
    base, sched = 1e-2, LRSchedule.warmup_cosine(2, 6)
    kw = dict(momentum=0.9, nesterov=True, weight_decay=1e-4)
    lr_max = max(sched.lr_at(k, base) for k in range(3))
    assert lr_max == base and sched.lr_at(0, base) == 0.0

    ref = _ttm(cuda)
    opt_r = FusedSGD(ref.parameters(), lr=base, **kw)
    ref_losses = []
    for k, (f, y) in enumerate(batches[1:]):
        for group in opt_r.param_groups:
            group["lr"] = sched.lr_at(k, base)
        opt_r.zero_grad(set_to_none=True)
        loss = loss_of(ref)(f, y)
        loss.backward()
        opt_r.step()
        ref_losses.append(loss.item())

    m = _ttm(cuda)
    opt_m = FusedSGD(m.parameters(), lr=base, schedule=sched, **kw)
    step = GraphedStep(loss_of(m), example_inputs=batches[0], params=list(m.parameters()), optimizer=opt_m, warmup=2)
    got = [step(f, y).item() for f, y in batches[1:]]
    torch.cuda.synchronize()
    for a, b in zip(got, ref_losses):
        assert abs(a - b) < 2e-3 * max(1.0, abs(b)), (got, ref_losses)
    moved = 0.0
    for (n, pa), (_, pb), p0 in zip(m.named_parameters(), ref.named_parameters(), _ttm(cuda).parameters()):
        assert (pa - pb).abs().max().item() <= 2.0 * lr_max * 3, n
        assert (pa - pb).abs().median().item() < 0.04 * lr_max, n
        moved = max(moved, (pa - p0).abs().max().item())
    print(f"largest parameter movement {moved:.3e}; bars {2.0 * lr_max * 3:.1e} (max), {0.04 * lr_max:.1e} (median)")
    assert moved > 4 * 0.04 * lr_max, moved                                   # the updates are larger than the bars: they were applied
    assert abs(opt_m.current_lr()[0] - float(np.float32(sched.lr_at(2, base)))) <= sr.lr_bound(sched.lr_at(2, base), base)

    counts = {}
    for tag, s in (("by_value", None), ("scheduled", LRSchedule.warmup_cosine(2, 6))):
        mm = _ttm(cuda)
        opt = FusedAdam(mm.parameters(), lr=1e-4, schedule=s)
        for i in range(2):
            opt.zero_grad(set_to_none=True)
            loss_of(mm)(*batches[i]).backward()
            if i == 1:
                egx_lib.egx_launch_count(1)
            opt.step()
        counts[tag] = int(egx_lib.egx_launch_count(1))
    assert counts["scheduled"] == counts["by_value"] >= 2, counts


@pytest.mark.parametrize("which", ["sgd", "adam"])
def test_resume_continues_schedule_and_state(egx_lib, cuda, which):
    """state_dict() after 5 steps into a fresh optimizer with the same schedule: the next 3 updates are the uninterrupted run's, bit for bit."""
    from egot2_amd.train import FusedAdam, FusedSGD, LRSchedule
    sched = lambda: LRSchedule.warmup_cosine(5, 30)  # noqa: E731
    make = (lambda ps: FusedSGD(ps, lr=sr.SGD_LR, momentum=0.9, dampening=0.1, weight_decay=1e-4, schedule=sched())) if which == "sgd" \
        else (lambda ps: FusedAdam(ps, lr=1e-2, betas=(0.9, 0.99), weight_decay=1e-4, schedule=sched()))

    def run(opt, ps, steps):
        for t in steps:
            for p, g in zip(ps, _gpu_grads(t, cuda, SMALL)):
                p.grad = g
            opt.step()
    pa = _gpu_params(cuda, SMALL)
    oa = make(pa)
    run(oa, pa, range(5))
    saved = copy.deepcopy(oa.state_dict())
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = make(pb)
    ob.load_state_dict(saved)
    run(oa, pa, range(5, 8))
    run(ob, pb, range(5, 8))
    torch.cuda.synchronize()
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    assert int(ob._step_dev.item()) == 8 and ob.current_lr() == oa.current_lr()
    assert ob.current_lr()[0] not in (0.0, oa.param_groups[0]["lr"])           # a scheduled value: k = 7 of the warm-up cosine


def test_torch_sgd_state_dict_loads_and_continues(egx_lib, cuda):
    """torch.optim.SGD's state dict (momentum buffers, no step count) into FusedSGD: the count starts at 1, the first-update rule does not
    fire, and 5 torch steps + 3 fused steps stay within BAR_SGD of 8 fp64 steps."""
    from egot2_amd.train import FusedSGD
    cfg = dict(momentum=0.9, dampening=0.1, nesterov=False, weight_decay=1e-4)
    ps = _gpu_params(cuda, SMALL)
    ot = torch.optim.SGD(ps, lr=sr.SGD_LR, **cfg)
    for t in range(5):
        for p, g in zip(ps, _gpu_grads(t, cuda, SMALL)):
            p.grad = g.clone()
        ot.step()
    of = FusedSGD(ps, lr=sr.SGD_LR, **cfg)
    of.load_state_dict(copy.deepcopy(ot.state_dict()))
    for t in range(5, 8):
        for p, g in zip(ps, _gpu_grads(t, cuda, SMALL)):
            p.grad = g
        of.step()
    torch.cuda.synchronize()
    assert int(of._step_dev.item()) == 4
    ref = sr.sgd_torch(cfg, torch.float64, shapes=SMALL)[0]
    for p, r in zip(ps, ref):
        assert unit_ref.rel_err(p.detach().cpu(), r) <= sr.BAR_SGD
