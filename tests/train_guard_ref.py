"""The gate of tests/test_cpu_train_guard.py and tests/test_gpu_train_guard.py: cases, planted inputs, bars and fp64 references of the
gradient-norm clipping and the non-finite guard of the captured step (egx_grad_norm and the gated / guarded twins, train.GradGuard).

Plain Python / torch on the CPU; nothing here is imported from the product path. `perturb=` names one deliberate mistake; the CPU tests
check that the bars reject each of them.

Decision (decision())
    sqsum = sum of (double)g^2 over all buffers, norm = sqrt(sqsum), finite = isfinite(sqsum), c = max_norm / (norm + 1e-6) in fp64,
    coef = fp32(c) if c < 1 else 1 (1 without a max_norm; a comparison, so a NaN gives 1), apply = finite or not skip_nonfinite.
    Norm bar (norm_bar): |norm - ref| <= n_total * 2^-52 * ref. DERIVED: every square of an fp32 is exact in fp64, a sum of n non-negative
    fp64 terms carries at most (n - 1) 2^-53 relative error in ANY order, so two orders differ by at most (n - 1) 2^-52 in sqsum; the square
    root halves that and adds its own rounding on both sides (2^-52 together).
    coef bar (coef_ok): within one fp32 ulp of the fp64 formula rounded to fp32; exactly 1 where the reference is 1.
Steps (run())
    clip + Adam / AdamW / SGD written out, STEPS steps in the dtype asked for, on the gradients of grads(): fp64 is the reference (checked
    against torch.nn.utils.clip_grad_norm_ + torch.optim in fp64 by the CPU test), and the yardstick is STOCK clip_grad_norm_ + torch.optim in
    fp32 on the CPU against it: BAR_STEP = unit_ref.FACTOR * GUARD_FP32_ERR, the worst unit_ref.rel_err over CONFIGS x MAX_NORMS and every
    parameter / moment tensor after STEPS steps. Step counts and the counters steps / skipped / clipped are integers and compare exactly.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests import unit_ref

F64 = torch.float64

# ---- the norm and the decision -------------------------------------------------------------------------------------------------------------
TABLE = 32                                   # buffers per grouped launch (EGX_GRAD_NORM_TABLE)
GRID_CAP_ELEMS = 2048 * 256 * 4              # grad_sqsum_kernel: at most 2048 workgroups of 256 threads, 4 elements a thread per turn
NORM_SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099]      # n % 4 tails, one thread, a workgroup boundary either side, several workgroups
G_CASES = [1, 2, TABLE, TABLE + 1]
FLT_MAX = float(np.finfo(np.float32).max)


def norm_bar(n_total: int) -> float:
    """Relative bar of the device norm against the fp64 reference (module docstring): n_total * 2^-52."""
    return max(int(n_total), 1) * 2.0 ** -52


def spread_values(n: int, seed: int) -> torch.Tensor:
    """n fp32 values of either sign with magnitudes spread over 1e-20 .. 1e19 (their squares span 1e-40 .. 1e38: all exact in fp64)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=F64) * 39.0 - 20.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).to(F64)
    return (mag * sign).float()


def sizes_for(G: int, with_empty: bool = True):
    """The buffer sizes of a G-buffer case: NORM_SIZES in turn, and (G >= 2) one empty buffer in second place."""
    ns = [NORM_SIZES[i % len(NORM_SIZES)] for i in range(G)]
    if with_empty and G >= 2:
        ns[1] = 0
    return ns


def decision(bufs, max_norm=None, skip_nonfinite: bool = True, perturb=None) -> dict:
    """-> norm (float, fp64), coef (np.float32), finite, apply, clipped (bool) of the buffers `bufs` (fp32 tensors).
    perturb: no_clamp (coef = fp32(c) also where c >= 1), no_eps (the 1e-6 of the denominator dropped), first_buffer (the norm of bufs[0]
    alone), abs_sum (sum of |g| in place of the squares)."""
    use = bufs[:1] if perturb == "first_buffer" else bufs
    with np.errstate(all="ignore"):
        if perturb == "abs_sum":
            sqsum = float(sum(b.to(F64).abs().sum().item() for b in use))
        else:
            sqsum = float(sum((b.to(F64) ** 2).sum().item() for b in use))
        norm = math.sqrt(sqsum) if sqsum == sqsum and sqsum >= 0 else math.nan
        finite = math.isfinite(sqsum)
        coef = np.float32(1.0)
        if max_norm is not None:
            den = np.float64(norm) + (np.float64(0.0) if perturb == "no_eps" else np.float64(1e-6))
            c = np.float64(max_norm) / den
            if c < 1.0 or (perturb == "no_clamp" and c == c):
                coef = np.float32(c)
    apply = bool(finite or not skip_nonfinite)
    return {"norm": norm, "coef": coef, "finite": finite, "apply": apply, "clipped": bool(apply and coef < 1.0)}


def norm_ok(got: float, ref: float, n_total: int) -> bool:
    if not math.isfinite(ref):
        return (math.isnan(got) and math.isnan(ref)) or got == ref
    return abs(got - ref) <= norm_bar(n_total) * abs(ref)


def coef_ok(got, ref) -> bool:
    got, ref = np.float32(got), np.float32(ref)
    if ref == np.float32(1.0):
        return bool(got == ref)
    return bool(abs(np.float64(got) - np.float64(ref)) <= np.float64(np.spacing(ref)))


def decision_cases():
    """-> [(id, buffers, max_norm)]: where each term of the formula decides. tiny: norm 1e-3 against max_norm 1e-4 (the 1e-6 is 1e-3 of the
    denominator); zeros: 0 / 1e-6; under: max_norm above the norm (the clamp); two: most of the norm in the second buffer; huge: all 3e38
    (max_norm 1e10 keeps the coefficient a normal fp32)."""
    g = torch.Generator(device="cpu").manual_seed(77)
    a, b = torch.randn(1025, generator=g), torch.randn(4099, generator=g) * 3.0
    tiny = torch.randn(1024, generator=g) * (1e-3 / 32.0)
    return [("over", [a, b], 1.0), ("under", [a, b], 1e4), ("tiny", [tiny], 1e-4), ("zeros", [torch.zeros(1023)], 1e-7),
            ("two", [a * 1e-3, b], 10.0), ("huge", [torch.full((1025,), 3e38)], 1e10), ("none", [a, b], None)]


PLANT_VALUES = [math.inf, -math.inf, math.nan]


def plant_cases():
    """-> [(id, sizes, buffer index, element index)]: where a non-finite value is planted. Element 0, the last element (in the n % 4 tail of a
    1025 + 2 buffer), the tail's first element, the second of two buffers, a 1-element buffer."""
    return [("first", [4099], 0, 0), ("last", [1027], 0, 1026), ("tail", [1027], 0, 1024), ("second_buffer", [1024, 1025], 1, 513),
            ("one_element", [1023, 1], 1, 0)]


# ---- clipped optimizer steps ---------------------------------------------------------------------------------------------------------------
STEPS = 6
SHAPES = [(1023,), (5,), (4099,), (64, 33)]         # 7239 elements: randn gradients have a norm near 85 at scale 1
STEP_SCALE = [1.0, 0.5, 2.0, 1.0, 0.97, 1.03]      # the norm of step t is near 85 * STEP_SCALE[t]
MAX_NORMS = [8.0, 85.0, 1000.0]                     # below every step's norm, between them ("near"), above all of them
ADAM_LR, SGD_LR = 1e-2, 0.05
CONFIGS = [
    dict(kind="adam", adamw=False, weight_decay=0.0), dict(kind="adam", adamw=False, weight_decay=0.05),
    dict(kind="adam", adamw=True, weight_decay=0.05),
    dict(kind="sgd", momentum=0.0, nesterov=False, weight_decay=1e-4), dict(kind="sgd", momentum=0.9, nesterov=False, weight_decay=1e-4),
    dict(kind="sgd", momentum=0.9, nesterov=True, weight_decay=1e-4),
]
# The C ABI carries the hyper-parameters as fp32 and the Adam update text forms 1 - beta in fp32 (torch forms it in Python's fp64 and rounds
# once). The cases at the bar therefore use betas that ARE fp32 numbers, 1 - 2^-3 and 1 - 2^-10, so the reference, the fp32 yardstick and the
# device all run the same Adam. torch's defaults are not: fp32(0.999) is 0.99900001287, and 1 - fp32(0.999) misses 0.001 by 1.29e-5 relative,
# which exp_avg_sq inherits in full. DEFAULT_BETAS is checked with exactly that representation error added to the moments' bars (beta_allowance).
BETAS, EPS = (1.0 - 2.0 ** -3, 1.0 - 2.0 ** -10), 1e-8
DEFAULT_BETAS = (0.9, 0.999)
# Measured by tests/test_cpu_train_guard.py::test_yardstick (printed with -s), which holds the constant to what it measures within 3x either way.
GUARD_FP32_ERR = 3.1e-7
BAR_STEP = unit_ref.FACTOR * GUARD_FP32_ERR


def beta_allowance(beta: float, steps: int = STEPS) -> float:
    """What carrying `beta` as an fp32 adds to a moment's relative error over `steps` steps: the representation error of 1 - beta formed in
    fp32, |fl32(1 - fl32(beta)) - (1 - beta)| / (1 - beta), plus steps times that of beta itself (the decay beta^k). 0 for an fp32 number."""
    b32 = np.float32(beta)
    one_minus = float(np.float32(1.0) - b32)
    return abs(one_minus - (1.0 - beta)) / (1.0 - beta) + steps * abs(float(b32) - beta) / beta


def config_id(c) -> str:
    if c["kind"] == "adam":
        return f"{'adamw' if c['adamw'] else 'adam'}_wd{c['weight_decay']}"
    return f"sgd_mu{c['momentum']}_n{int(c['nesterov'])}"


@functools.lru_cache(maxsize=None)
def params():
    g = torch.Generator(device="cpu").manual_seed(5100)
    return tuple(torch.randn(s, generator=g) for s in SHAPES)


@functools.lru_cache(maxsize=None)
def grads(step: int):
    g = torch.Generator(device="cpu").manual_seed(5200 + step)
    return tuple(torch.randn(s, generator=g) * STEP_SCALE[step % len(STEP_SCALE)] for s in SHAPES)


def run(cfg: dict, dtype, max_norm=None, bad_steps=(), skip_nonfinite: bool = True, perturb=None, steps: int = STEPS, betas=BETAS) -> dict:
    """clip + update written out, `steps` steps in `dtype`. A step in `bad_steps` carries a non-finite gradient (with skip_nonfinite it is
    skipped: nothing changes). -> params, state (name -> tensors: exp_avg, exp_avg_sq | momentum_buffer), step (applied updates), steps,
    skipped, clipped. perturb: any of decision()'s, skip_advances_step (a skipped step still counts in the step count), skip_decays_exp_avg
    (a skipped step still multiplies exp_avg / momentum_buffer by beta1 / momentum)."""
    if bad_steps and not skip_nonfinite:
        raise ValueError("the written-out run models bad steps only as skipped ones")
    adam = cfg["kind"] == "adam"
    ps = [p.to(dtype).clone() for p in params()]
    m = [torch.zeros_like(p) for p in ps]
    v = [torch.zeros_like(p) for p in ps]
    buf = [None] * len(ps)
    t = skipped = clipped = 0
    wd = cfg["weight_decay"]
    b1, b2 = betas
    for k in range(steps):
        g32 = grads(k)
        if k in bad_steps:
            skipped += 1
            if perturb == "skip_advances_step":
                t += 1
            if perturb == "skip_decays_exp_avg":
                for j in range(len(ps)):
                    m[j] = b1 * m[j]
                    if buf[j] is not None:
                        buf[j] = cfg.get("momentum", 0.0) * buf[j]
            continue
        d = decision(list(g32), max_norm, True, perturb if perturb in ("no_clamp", "no_eps", "first_buffer", "abs_sum") else None)
        clipped += int(d["clipped"])
        coef = float(d["coef"])
        t += 1
        for j, p in enumerate(ps):
            g = g32[j].to(dtype) * coef
            if adam:
                if cfg["adamw"]:
                    p.mul_(1 - ADAM_LR * wd)
                elif wd != 0:
                    g = g + wd * p
                m[j] = b1 * m[j] + (1 - b1) * g
                v[j] = b2 * v[j] + (1 - b2) * g * g
                bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
                p.sub_((ADAM_LR / bc1) * m[j] / (v[j].sqrt() / math.sqrt(bc2) + EPS))
            else:
                mu = cfg["momentum"]
                if wd != 0:
                    g = g + wd * p
                if mu != 0:
                    buf[j] = g.clone() if buf[j] is None else mu * buf[j] + g
                    g = g + mu * buf[j] if cfg["nesterov"] else buf[j]
                p.sub_(SGD_LR * g)
    state = {"exp_avg": m, "exp_avg_sq": v} if adam else ({"momentum_buffer": [b if b is not None else torch.zeros_like(p) for b, p in zip(buf, ps)]}
                                                          if cfg["momentum"] != 0 else {})
    return {"params": ps, "state": state, "step": t, "steps": steps, "skipped": skipped, "clipped": clipped}


def run_torch(cfg: dict, dtype, max_norm=None, steps: int = STEPS, betas=BETAS) -> dict:
    """torch.nn.utils.clip_grad_norm_ + torch.optim themselves on the same inputs (CPU), every step clean."""
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in params()]
    if cfg["kind"] == "adam":
        cls = torch.optim.AdamW if cfg["adamw"] else torch.optim.Adam
        opt = cls(ps, lr=ADAM_LR, betas=betas, eps=EPS, weight_decay=cfg["weight_decay"])
    else:
        opt = torch.optim.SGD(ps, lr=SGD_LR, momentum=cfg["momentum"], nesterov=cfg["nesterov"], weight_decay=cfg["weight_decay"])
    clipped = 0
    for k in range(steps):
        for p, g in zip(ps, grads(k)):
            p.grad = g.to(dtype).clone()
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
            clipped += int(max_norm / (float(total) + 1e-6) < 1.0)
        opt.step()
    keys = ("exp_avg", "exp_avg_sq") if cfg["kind"] == "adam" else (("momentum_buffer",) if cfg["momentum"] != 0 else ())
    state = {key: [opt.state[p][key].detach() for p in ps] for key in keys}
    return {"params": [p.detach() for p in ps], "state": state, "step": steps, "steps": steps, "skipped": 0, "clipped": clipped}


def rel_errs(got: dict, ref: dict) -> dict:
    """Worst unit_ref.rel_err of two runs per kind of tensor: "params" and every state key (the same tensors in the same order)."""
    assert set(got["state"]) == set(ref["state"]), (sorted(got["state"]), sorted(ref["state"]))
    out = {"params": max(unit_ref.rel_err(a, b) for a, b in zip(got["params"], ref["params"]))}
    for key, tensors in ref["state"].items():
        out[key] = max(unit_ref.rel_err(a, b) for a, b in zip(got["state"][key], tensors))
    return out


def worst_rel_err(got: dict, ref: dict) -> float:
    return max(rel_errs(got, ref).values())


def counts_equal(got: dict, ref: dict) -> bool:
    return all(int(got[k]) == int(ref[k]) for k in ("step", "steps", "skipped", "clipped"))


@functools.lru_cache(maxsize=None)
def reference(config_index: int, max_norm, bad_steps=(), betas=BETAS) -> dict:
    """The fp64 run of CONFIGS[config_index]; shared by the tests that need it and left unchanged by them."""
    return run(CONFIGS[config_index], F64, max_norm, bad_steps, betas=betas)
