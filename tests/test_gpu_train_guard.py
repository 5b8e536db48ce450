"""-m gpu: gradient-norm clipping and the non-finite guard of the captured step - egx_grad_norm (grad_sqsum_kernel + guard_finish_kernel), the
gated bump, the guarded Adam / SGD updates, train.GradGuard under FusedAdam / FusedSGD / GraphedStep and behind the gradient exchange. Cases,
planted inputs, bars and fp64 references: tests/train_guard_ref.py (norm: n_total * 2^-52 relative, derived; coef: one fp32 ulp; six clipped
steps: unit_ref.FACTOR * the error of stock clip_grad_norm_ + torch.optim in fp32). Skipped steps and max_norm=None are compared bit for bit.
Every test prints its worst error / bar under -s in a line starting with "[guard"; tools/train_guard_eval.py keeps them in
profiles/train_guard_report.txt."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import train_guard_ref as gr
from tests.util import hhi_args, seeded_feats, seeded_state_dict

pytestmark = pytest.mark.gpu
CE_W = [0.266, 0.734]
CONFIG_IDS = [gr.config_id(c) for c in gr.CONFIGS]


def _read(words) -> dict:
    w = words.cpu()
    return {"norm": float(w[0:1].view(torch.float64)[0]), "coef": np.float32(w[1:2].view(torch.float32)[0].item()),
            "apply": int(w[1:2].view(torch.int32)[1]), "steps": int(w[2]), "skipped": int(w[3]), "clipped": int(w[4])}


def _measure(lib, bufs, max_norm=None, skip=True, words=None):
    """egx_grad_norm through the C ABI on `bufs` (device tensors) -> the 5-word guard block (a fresh zeroed one unless `words`)."""
    from egot2_amd import _lib
    n = len(bufs)
    ns = (C.c_size_t * n)(*[b.numel() for b in bufs])
    ptrs = (C.c_void_p * n)(*[b.data_ptr() if b.numel() else None for b in bufs])
    need = lib.egx_grad_norm_scratch_bytes(ns, n)
    scratch = torch.empty(need, dtype=torch.uint8, device=bufs[0].device)
    if words is None:
        words = torch.zeros(5, dtype=torch.int64, device=bufs[0].device)
    cfg = _lib.GradNormCfg(0.0 if max_norm is None else max_norm, int(max_norm is not None), int(skip))
    rc = lib.egx_grad_norm(ptrs, ns, n, scratch.data_ptr(), need, C.byref(cfg), words.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.egx_last_error()
    torch.cuda.synchronize()
    return words


def _misaligned(t, cuda):
    """`t` on the device, starting 4 bytes past a 16-byte boundary."""
    flat = torch.zeros(t.numel() + 8, device=cuda)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _check_decision(got: dict, ref: dict, n_total: int, tag: str) -> float:
    assert gr.norm_ok(got["norm"], ref["norm"], n_total), (tag, got["norm"], ref["norm"], gr.norm_bar(n_total))
    assert gr.coef_ok(got["coef"], ref["coef"]), (tag, got["coef"], ref["coef"])
    assert got["apply"] == int(ref["apply"]), (tag, got, ref)
    if math.isfinite(ref["norm"]) and ref["norm"] > 0:
        return abs(got["norm"] - ref["norm"]) / ref["norm"] / gr.norm_bar(n_total)
    return 0.0


# ---- the norm and the decision -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", gr.G_CASES)
def test_norm_against_fp64(egx_lib, cuda, G):
    """G buffers of the edge sizes (one of them empty), magnitudes spread over 1e-20 .. 1e19: the norm inside the derived bar, the coefficient
    inside one ulp at max_norm = half the norm, without one and far above it; three calls agree bit for bit and count as three steps."""
    sizes = gr.sizes_for(G)
    host = [gr.spread_values(n, 900 + 37 * G + i) for i, n in enumerate(sizes)]
    bufs = [h.to(cuda) for h in host]
    n_total = sum(sizes)
    half = gr.decision(host)["norm"] / 2
    worst = 0.0
    for mn in (None, half, 1e30):
        words = _measure(egx_lib, bufs, mn)
        got, ref = _read(words), gr.decision(host, mn)
        worst = max(worst, _check_decision(got, ref, n_total, (G, mn)))
        assert got["steps"] == 1 and got["skipped"] == 0 and got["clipped"] == int(ref["clipped"])
        first = words.clone()
        for rep in (2, 3):
            _measure(egx_lib, bufs, mn, words=words)
            assert torch.equal(words[:2], first[:2]), (G, mn, rep)          # norm, coef and apply: the same bits
        assert _read(words)["steps"] == 3 and _read(words)["clipped"] == 3 * int(ref["clipped"])
    print(f"[guard norm] G = {G}, n = {n_total}: worst norm error / bar {worst:.3g} (bar {gr.norm_bar(n_total):.3g} relative)")


def test_norm_past_the_grid_cap_and_off_alignment(egx_lib, cuda):
    """One buffer of 2048 * 256 * 4 + 4 elements (the workgroups stride), and every edge size starting 4 bytes past a 16-byte boundary (the
    4-byte loads): inside the bar, and the same bits as the aligned buffer - the summation order is a function of the sizes alone."""
    worst = 0.0
    for n in [gr.GRID_CAP_ELEMS + 4] + gr.NORM_SIZES:
        host = gr.spread_values(n, 4000 + n % 1000)
        ref = gr.decision([host], 1.0)
        aligned, shifted = host.to(cuda), _misaligned(host, cuda)
        assert aligned.data_ptr() % 16 == 0
        wa, ws = _measure(egx_lib, [aligned], 1.0), _measure(egx_lib, [shifted], 1.0)
        worst = max(worst, _check_decision(_read(wa), ref, n, n), _check_decision(_read(ws), ref, n, (n, "shifted")))
        assert torch.equal(wa, ws), n
    # the same buffers in one grouped launch, the large one in the middle
    hosts = [gr.spread_values(1025, 1), gr.spread_values(gr.GRID_CAP_ELEMS + 4, 2), gr.spread_values(5, 3)]
    got = _read(_measure(egx_lib, [h.to(cuda) for h in hosts], None))
    worst = max(worst, _check_decision(got, gr.decision(hosts), sum(h.numel() for h in hosts), "grouped"))
    print(f"[guard norm] grid cap and misaligned buffers: worst norm error / bar {worst:.3g}")


def test_norm_of_the_planted_magnitudes(egx_lib, cuda):
    """All 3e38: finite, applied, a norm above FLT_MAX held in fp64 and clipped (max_norm 1e10: a coefficient near 5e-31, a normal fp32); all
    zeros: norm 0, coef 1 at max_norm 1; and the gate's decision cases."""
    huge = torch.full((4099,), 3e38)
    got, ref = _read(_measure(egx_lib, [huge.to(cuda)], 1e10)), gr.decision([huge], 1e10)
    _check_decision(got, ref, 4099, "huge")
    assert got["apply"] == 1 and got["skipped"] == 0 and got["clipped"] == 1 and got["norm"] > gr.FLT_MAX and 0 < got["coef"] < 1e-29
    got = _read(_measure(egx_lib, [torch.zeros(1025, device=cuda), torch.zeros(3, device=cuda)], 1.0))
    assert got["norm"] == 0.0 and got["coef"] == np.float32(1.0) and got["apply"] == 1 and got["clipped"] == 0
    worst = 0.0
    for cid, bufs, mn in gr.decision_cases():
        got, ref = _read(_measure(egx_lib, [b.to(cuda) for b in bufs], mn)), gr.decision(bufs, mn)
        worst = max(worst, _check_decision(got, ref, sum(b.numel() for b in bufs), cid))
        assert got["clipped"] == int(ref["clipped"]), cid
    print(f"[guard norm] decision cases: worst norm error / bar {worst:.3g}")


# ---- optimizers on the gate's parameters and gradients ---------------------------------------------------------------------------------------
class _Problem:
    """The gate's parameters on the device with persistent gradient tensors: the first two as views of ONE flat buffer at offsets that are
    not 16-byte aligned (what functional._GradPacker hands out), the others on their own: three gradient buffers for the norm."""

    def __init__(self, cuda, sizes=None):
        shapes = gr.SHAPES if sizes is None else [(n,) for n in sizes]
        init = gr.params() if sizes is None else [torch.randn(s, generator=torch.Generator().manual_seed(60 + i)) for i, s in enumerate(shapes)]
        self.params = [torch.nn.Parameter(p.clone().to(cuda)) for p in init]
        packed = 2 if sizes is None else 0
        n2 = [self.params[i].numel() for i in range(packed)]
        self.flat = torch.zeros(3 + sum(n + 1 for n in n2), device=cuda) if packed else None
        off = 3
        for i, p in enumerate(self.params):
            if i < packed:
                p.grad = self.flat[off:off + n2[i]].view(p.shape)
                off += n2[i] + 1
            else:
                p.grad = torch.zeros_like(p)

    def set_grads(self, tensors):
        for p, g in zip(self.params, tensors):
            p.grad.copy_(g)

    def state_bits(self, opt):
        """Everything the optimizer owns, as integer tensors on the host."""
        out = [p.detach().view(torch.int32).cpu().clone() for p in self.params]
        for p in self.params:
            for key in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
                if key in opt.state.get(p, {}):
                    out.append(opt.state[p][key].view(torch.int32).cpu().clone())
        out.append(opt._step_dev.cpu().clone())
        if opt._lr_dev is not None:
            out.append(opt._lr_dev.view(torch.int32).cpu().clone())
        return out

    def result(self, opt, keys) -> dict:
        return {"params": [p.detach().cpu() for p in self.params], "state": {k: [opt.state[p][k].cpu() for p in self.params] for k in keys}}


def _optimizer(cfg, params, guard=None, schedule=None, betas=gr.BETAS):
    from egot2_amd.train import FusedAdam, FusedSGD
    if cfg["kind"] == "adam":
        return FusedAdam(params, lr=gr.ADAM_LR, betas=betas, eps=gr.EPS, weight_decay=cfg["weight_decay"], adamw=cfg["adamw"],
                         schedule=schedule, guard=guard)
    return FusedSGD(params, lr=gr.SGD_LR, momentum=cfg["momentum"], nesterov=cfg["nesterov"], weight_decay=cfg["weight_decay"],
                    schedule=schedule, guard=guard)


def _state_keys(cfg):
    return ("exp_avg", "exp_avg_sq") if cfg["kind"] == "adam" else (("momentum_buffer",) if cfg["momentum"] != 0 else ())


@pytest.mark.parametrize("scheduled", [False, True], ids=["by_value", "scheduled"])
@pytest.mark.parametrize("ci", range(len(gr.CONFIGS)), ids=CONFIG_IDS)
def test_unclipped_guard_is_bit_identical_to_no_guard(egx_lib, cuda, ci, scheduled):
    """max_norm=None and finite gradients: six steps behind a guard leave the bits the unguarded optimizer leaves - parameters, moments, the
    step count and the scheduled learning rates."""
    from egot2_amd.train import GradGuard, LRSchedule
    cfg = gr.CONFIGS[ci]
    sched = (lambda: LRSchedule.warmup_cosine(2, 9)) if scheduled else (lambda: None)
    plain, guarded = _Problem(cuda), _Problem(cuda)
    opt_p, opt_g = _optimizer(cfg, plain.params, None, sched()), _optimizer(cfg, guarded.params, GradGuard(), sched())
    for k in range(gr.STEPS):
        for prob, opt in ((plain, opt_p), (guarded, opt_g)):
            prob.set_grads(gr.grads(k))
            opt.step()
    torch.cuda.synchronize()
    for a, b in zip(plain.state_bits(opt_p), guarded.state_bits(opt_g)):
        assert torch.equal(a, b)
    res = opt_g.guard_result()
    ref = gr.decision(list(gr.grads(gr.STEPS - 1)))
    assert res["steps"] == gr.STEPS and res["skipped"] == 0 and res["clipped"] == 0 and res["applied"] == 1 and res["clip_coef"] == 1.0
    assert gr.norm_ok(res["grad_norm"], ref["norm"], guarded.flat.numel() + sum(p.numel() for p in guarded.params[2:]))
    assert int(opt_g._step_dev) == gr.STEPS
    blk = opt_g.guard.block
    assert blk["grad_norm"].dtype == torch.float64 and blk["clip_coef"].dtype == torch.float32 and blk["applied"].dtype == torch.int32
    assert float(blk["grad_norm"]) == res["grad_norm"] and int(blk["steps"]) == gr.STEPS


@pytest.mark.parametrize("mn", gr.MAX_NORMS, ids=["below", "near", "above"])
@pytest.mark.parametrize("ci", range(len(gr.CONFIGS)), ids=CONFIG_IDS)
def test_clipped_steps_follow_the_fp64_reference(egx_lib, cuda, ci, mn):
    """Six steps with max_norm below, between and above the steps' norms: parameters and moments inside BAR_STEP of the fp64 clip + update,
    the clipped count and the step count equal to the reference's, every step's norm and coefficient inside their bars."""
    from egot2_amd.train import GradGuard
    cfg = gr.CONFIGS[ci]
    prob = _Problem(cuda)
    opt = _optimizer(cfg, prob.params, GradGuard(max_norm=mn))
    n_total = prob.flat.numel() + sum(p.numel() for p in prob.params[2:])
    worst_norm = 0.0
    for k in range(gr.STEPS):
        prob.set_grads(gr.grads(k))
        opt.step()
        res, ref = opt.guard_result(), gr.decision(list(gr.grads(k)), mn)
        worst_norm = max(worst_norm, _check_decision({"norm": res["grad_norm"], "coef": res["clip_coef"], "apply": res["applied"]}, ref, n_total, k))
    ref = gr.reference(ci, mn)
    got = prob.result(opt, _state_keys(cfg))
    err = gr.worst_rel_err(got, ref)
    res = opt.guard_result()
    print(f"[guard step] {gr.config_id(cfg)} max_norm {mn}: error / BAR_STEP {err / gr.BAR_STEP:.3g} (BAR_STEP {gr.BAR_STEP:.3g}), "
          f"norm error / bar {worst_norm:.3g}, clipped {res['clipped']} of {res['steps']}")
    assert err <= gr.BAR_STEP, (err, gr.BAR_STEP)
    assert gr.counts_equal({"step": int(opt._step_dev), **res}, ref), (res, int(opt._step_dev))


@pytest.mark.parametrize("ci", range(3), ids=CONFIG_IDS[:3])
def test_clipped_adam_at_torchs_default_betas(egx_lib, cuda, ci):
    """betas = (0.9, 0.999) are not fp32 numbers and the update text forms 1 - beta in fp32 (measured with them: exp_avg_sq at 4.0 x BAR_STEP,
    1.29e-5, all of it the representation error of 1 - fp32(0.999), which cancels in the update itself). The parameters stay at BAR_STEP; each
    moment's bar gains train_guard_ref.beta_allowance of its beta, the representation error alone, nothing measured."""
    from egot2_amd.train import GradGuard
    cfg, mn = gr.CONFIGS[ci], 85.0
    prob = _Problem(cuda)
    opt = _optimizer(cfg, prob.params, GradGuard(max_norm=mn), betas=gr.DEFAULT_BETAS)
    for k in range(gr.STEPS):
        prob.set_grads(gr.grads(k))
        opt.step()
    ref = gr.reference(ci, mn, betas=gr.DEFAULT_BETAS)
    errs = gr.rel_errs(prob.result(opt, _state_keys(cfg)), ref)
    bars = {"params": gr.BAR_STEP, "exp_avg": gr.BAR_STEP + gr.beta_allowance(gr.DEFAULT_BETAS[0]),
            "exp_avg_sq": gr.BAR_STEP + gr.beta_allowance(gr.DEFAULT_BETAS[1])}
    print(f"[guard step] {gr.config_id(cfg)} default betas, max_norm {mn}: error / bar " + ", ".join(f"{k} {errs[k] / bars[k]:.3g}" for k in bars))
    for k in bars:
        assert errs[k] <= bars[k], (k, errs[k], bars[k])
    assert gr.counts_equal({"step": int(opt._step_dev), **opt.guard_result()}, ref)


@pytest.mark.parametrize("case", gr.plant_cases(), ids=[c[0] for c in gr.plant_cases()])
def test_planted_nonfinite_gradient_skips_the_step(egx_lib, cuda, case):
    """+inf, -inf and NaN at the case's position, under scheduled FusedAdam (AdamW) and FusedSGD (momentum, Nesterov): apply == 0, skipped + 1,
    and every byte the optimizer owns - parameters, moments / momentum buffer, step count, device learning rates - as it was; the next clean
    step is applied and is update number 3."""
    from egot2_amd.train import GradGuard, LRSchedule
    _, sizes, bi, ei = case
    gen = torch.Generator().manual_seed(11)
    for cfg in (gr.CONFIGS[2], gr.CONFIGS[5]):
        for mn in (None, 1.0):
            prob = _Problem(cuda, sizes)
            opt = _optimizer(cfg, prob.params, GradGuard(max_norm=mn), LRSchedule.warmup_cosine(2, 9))
            clean = lambda: [torch.randn(n, generator=gen) for n in sizes]  # noqa: E731
            for _ in range(2):
                prob.set_grads(clean())
                opt.step()
            skipped = 0
            for val in gr.PLANT_VALUES:
                before = prob.state_bits(opt)
                g = clean()
                g[bi][ei] = val
                prob.set_grads(g)
                opt.step()
                skipped += 1
                res = opt.guard_result()
                assert res["applied"] == 0 and res["skipped"] == skipped and res["steps"] == 2 + skipped, (val, res)
                assert not math.isfinite(res["grad_norm"])
                after = prob.state_bits(opt)
                assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), (gr.config_id(cfg), mn, val)
            prob.set_grads(clean())
            opt.step()
            res = opt.guard_result()
            assert res["applied"] == 1 and res["skipped"] == 3 and res["steps"] == 6 and int(opt._step_dev) == 3
            assert not all(torch.equal(a, b) for a, b in zip(after, prob.state_bits(opt)))
            sched = LRSchedule.warmup_cosine(2, 9)
            assert opt.current_lr()[0] == float(np.float32(sched.lr_at(2, opt.param_groups[0]["lr"])))      # update index 2: applied updates


@pytest.mark.parametrize("case", gr.plant_cases(), ids=[c[0] for c in gr.plant_cases()])
def test_planted_nonfinite_gradient_without_the_skip(egx_lib, cuda, case):
    """skip_nonfinite=False: apply == 1 whatever the gradients hold; coef == 1 without a max_norm and for a NaN norm (the comparison c < 1
    fails), clip_grad_norm_'s 0 for an infinite norm under a max_norm. The optimizer then applies the step: the count advances."""
    from egot2_amd.train import GradGuard
    _, sizes, bi, ei = case
    for val in gr.PLANT_VALUES:
        host = [torch.ones(n) for n in sizes]
        host[bi][ei] = val
        bufs = [h.to(cuda) for h in host]
        for mn in (None, 1.0):
            got, ref = _read(_measure(egx_lib, bufs, mn, skip=False)), gr.decision(host, mn, False)
            assert got["apply"] == 1 and got["skipped"] == 0 and not math.isfinite(got["norm"]), (val, mn, got)
            assert got["coef"] == ref["coef"] and (mn is None or math.isnan(val) or got["coef"] == 0.0), (val, mn, got)
            if mn is None:
                assert got["coef"] == np.float32(1.0) and got["clipped"] == 0
            got = _read(_measure(egx_lib, bufs, mn, skip=True))
            assert got["apply"] == 0 and got["skipped"] == 1 and got["clipped"] == 0
    prob = _Problem(cuda, sizes)
    opt = _optimizer(gr.CONFIGS[0], prob.params, GradGuard(skip_nonfinite=False))
    g = [torch.ones(n) for n in sizes]
    g[bi][ei] = math.nan
    prob.set_grads(g)
    opt.step()
    res = opt.guard_result()
    assert res["applied"] == 1 and res["clip_coef"] == 1.0 and res["skipped"] == 0 and int(opt._step_dev) == 1
    assert torch.isnan(prob.params[bi].detach().reshape(-1)[ei]).item()


def test_grad_norm_without_an_optimizer(egx_lib, cuda):
    """train.grad_norm: a device fp64 scalar, the gate's norm of the gradients; parameters without a gradient do not count."""
    from egot2_amd.train import grad_norm
    prob = _Problem(cuda)
    prob.set_grads(gr.grads(0))
    extra = torch.nn.Parameter(torch.ones(7, device=cuda))
    out = grad_norm(prob.params + [extra])
    assert out.dtype == torch.float64 and out.is_cuda and out.dim() == 0
    ref = gr.decision(list(gr.grads(0)))["norm"]
    assert gr.norm_ok(float(out), ref, prob.flat.numel() + sum(p.numel() for p in prob.params[2:]))
    assert gr.norm_ok(float(grad_norm(prob.params[3])), gr.decision([gr.grads(0)[3]])["norm"], prob.params[3].numel())


# ---- the real step ---------------------------------------------------------------------------------------------------------------------------
def _ttm(cuda, seed=3):
    from egot2_amd import hhi_ttm
    m = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(dropout=0.0))
    m.pos_embed.dropout.p = 0.0
    m.load_state_dict(seeded_state_dict(m, seed))
    return m.to(cuda).train().set_compute("f32s").set_deterministic()


def _bits(model, opt):
    out = [p.detach().view(torch.int32).cpu().clone() for p in model.parameters()]
    for p in model.parameters():
        for key in ("exp_avg", "exp_avg_sq"):
            out.append(opt.state[p][key].view(torch.int32).cpu().clone())
    return out + [opt._step_dev.cpu().clone(), opt._lr_dev.view(torch.int32).cpu().clone()]


def test_guard_on_the_real_captured_step(egx_lib, cuda):
    """The TTM 3-task translator (B = 4, T = 15, d = 128, one layer, every dropout 0, f32s, fixed-order backward) under GraphedStep with
    FusedAdam(warmup_cosine, GradGuard(max_norm=1)): six replays, batch 3 with one +inf feature element. The bad replay is skipped and changes
    no byte of parameters / moments / count / learning rates; after batch 6 the parameters are, bit for bit, those of a twin that replayed only
    the five clean batches; the counters say 6 steps, 1 skipped, and 0 right after construction in spite of the warm-up steps."""
    from egot2_amd.train import CrossEntropyLoss, FusedAdam, GradGuard, GraphedStep, LRSchedule
    crit = CrossEntropyLoss(torch.FloatTensor(CE_W)).to(cuda)
    batches = [([f.to(cuda) for f in seeded_feats(700 + i, [(4, 15, 256)] * 3)],
                torch.randint(0, 2, (4,), generator=torch.Generator().manual_seed(i)).to(cuda)) for i in range(7)]
    batches[3][0][1][2, 7, 100] = math.inf                         # batch 3 of 1 .. 6 (batch 0 is the example the step is captured on)
    loss_of = lambda model: (lambda f, y: crit(model.forward_features(*f), y))  # noqa: E731

    def make():
        m = _ttm(cuda)
        opt = FusedAdam(m.parameters(), lr=1e-3, schedule=LRSchedule.warmup_cosine(2, 12), guard=GradGuard(max_norm=1.0))
        step = GraphedStep(loss_of(m), example_inputs=batches[0], params=list(m.parameters()), optimizer=opt, warmup=2)
        return m, opt, step

    m, opt, step = make()
    assert opt.guard_result()["steps"] == 0 and opt.guard_result()["skipped"] == 0 and int(opt._step_dev) == 0
    for i in (1, 2):
        step(*batches[i])
    torch.cuda.synchronize()
    after2 = _bits(m, opt)
    assert opt.guard_result()["steps"] == 2 and int(opt._step_dev) == 2
    step(*batches[3])
    torch.cuda.synchronize()
    res = opt.guard_result()
    assert not math.isfinite(res["grad_norm"])
    assert res["applied"] == 0 and res["skipped"] == 1 and res["steps"] == 3, res
    after3 = _bits(m, opt)
    assert len(after2) == len(after3) and all(torch.equal(a, b) for a, b in zip(after2, after3))
    for i in (4, 5, 6):
        step(*batches[i])
    torch.cuda.synchronize()
    res = opt.guard_result()
    assert res["steps"] == 6 and res["skipped"] == 1 and res["applied"] == 1 and int(opt._step_dev) == 5, res
    assert math.isfinite(res["grad_norm"]) and res["grad_norm"] > 0
    assert 0 <= res["clipped"] <= 5
    assert (res["clip_coef"] < 1.0) == (1.0 / (res["grad_norm"] + 1e-6) < 1.0)

    tm, topt, tstep = make()
    for i in (1, 2, 4, 5, 6):
        tstep(*batches[i])
    torch.cuda.synchronize()
    tres = topt.guard_result()
    assert tres["steps"] == 5 and tres["skipped"] == 0 and tres["clipped"] == res["clipped"] and tres["grad_norm"] == res["grad_norm"]
    moved = 0
    for (name, a), (_, b), p0 in zip(m.named_parameters(), tm.named_parameters(), _ttm(cuda).parameters()):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), name
        moved += int((a.detach() != p0.detach()).sum())
    assert moved > 0                                               # the five clean updates were applied
    assert all(torch.equal(a, b) for a, b in zip(_bits(m, opt), _bits(tm, topt)))
    print(f"[guard real step] 6 replays, 1 skipped, {res['clipped']} clipped; last norm {res['grad_norm']:.6g}, coef {res['clip_coef']:.6g}; "
          f"bit-identical to the 5-batch twin over {sum(p.numel() for p in m.parameters())} parameters")


def test_guarded_step_behind_the_gradient_exchange(egx_lib, cuda):
    """One rank: ddp.allreduce_gradients(force=True) on the C ABI communicator, then a guarded step. The norm the guard measured is the gate's
    norm of the exchanged gradient buffers, and train.grad_norm gives the same bits."""
    from egot2_amd import ddp, functional as F_egx
    from egot2_amd.train import CrossEntropyLoss, FusedAdam, GradGuard, grad_norm
    crit = CrossEntropyLoss(torch.FloatTensor(CE_W)).to(cuda)
    comm = ddp.EgxComm(0, 1)
    ddp.use_egx_comm(comm)
    try:
        m = _ttm(cuda, 12)
        params = list(m.parameters())
        opt = FusedAdam(params, lr=1e-3, guard=GradGuard(max_norm=0.5))
        feats = [f.to(cuda) for f in seeded_feats(41, [(4, 15, 256)] * 3)]
        y = torch.tensor([0, 1, 1, 0], device=cuda)
        crit(m.forward_features(*feats), y).backward()
        assert ddp.allreduce_gradients(params, force=True) >= 1
        torch.cuda.synchronize()
        seen, host = set(), []
        for p in params:
            key = p.grad.untyped_storage().data_ptr()
            if key not in seen:
                seen.add(key)
                host.append(F_egx.flat_storage_view(p.grad).cpu().clone())
        alone = float(grad_norm(params))
        opt.step()
        res = opt.guard_result()
    finally:
        ddp.use_egx_comm(None)
        comm.close()
    ref = gr.decision(host, 0.5)
    n_total = sum(h.numel() for h in host)
    ratio = _check_decision({"norm": res["grad_norm"], "coef": res["clip_coef"], "apply": res["applied"]}, ref, n_total, "exchange")
    assert res["grad_norm"] == alone and res["steps"] == 1 and res["clipped"] == int(ref["clipped"])
    print(f"[guard exchange] {len(host)} buffer(s), {n_total} elements: norm {res['grad_norm']:.9g}, error / bar {ratio:.3g}")
