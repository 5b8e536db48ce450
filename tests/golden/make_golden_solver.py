#!/usr/bin/env python3
"""Records live/solver_schedules.npz: the per-step learning rates the REAL lr_factory (HOI/optimizers/lta/lr_scheduler.py:11-41, with
construct_optimizer and get_epoch_lr behind it) hands its optimizer, on a small config namespace. Only runnable where the reference tree
exists (it is imported here and nowhere else); the fixture travels with the repo.

    python tests/golden/make_golden_solver.py            # writes the fixture
    python tests/golden/make_golden_solver.py --check    # re-records and compares with the committed fixture: prints "check <ok> max_diff <d>"

The config: OPTIMIZING_METHOD sgd on a model with one "bn" parameter and one other (two parameter groups), BASE_LR = 1 - the recorded
learning rates ARE the factors the scheduler applies, with no product rounding on top -, steps_in_epoch = 10, MAX_EPOCH = 3 (t_total = 30),
WARMUP_STEPS = 5, 40 steps (the warm-up policies run past t_total). Arrays, all fp64:
    lr_<policy>            (40, 2)  policy in cosine, constant, cosine_warmup, linear_warmup, steps_with_relative_lrs (a get_epoch_lr policy:
                                    STEPS [0, 1, 2], LRS [1, 0.1, 0.01], WARMUP_EPOCHS 0.5 from WARMUP_START_LR 0.01); row k is the learning
                                    rate of update k, i.e. what the optimizer holds when its (k + 1)-th step() runs
    edge_<policy>_w<W>_t<T> (40, 2)  the warm-up policies at WARMUP_STEPS = 0 and 1 (t_total 30) and at t_total == WARMUP_STEPS (= 10, MAX_EPOCH 1)
    cosine_recursive_vs_closed_T50000   ()   max_k |lr_k - c_k| / c_k, c_k = 0.5 (1 + cos(pi k / T)) > 0, over k <= T = 50 000 of torch's recursive
                                    CosineAnnealingLR: the relative rounding a correct evaluation of these schedules accumulates (the host test's bar)
    config                 JSON of the numbers above
"""
import json
import os
import sys
from types import SimpleNamespace as NS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

STEPS, STEPS_IN_EPOCH, MAX_EPOCH, WARMUP_STEPS = 40, 10, 3, 5
POLICIES = ["cosine", "constant", "cosine_warmup", "linear_warmup", "steps_with_relative_lrs"]
EDGES = [(0, 3), (1, 3), (10, 1)]            # (WARMUP_STEPS, MAX_EPOCH): W = 0, W = 1, t_total == W
EPOCH_POLICY = dict(STEPS=[0, 1, 2], LRS=[1.0, 0.1, 0.01], WARMUP_EPOCHS=0.5, WARMUP_START_LR=0.01)
FIXTURE = os.path.join(HERE, "live", "solver_schedules.npz")


def cfg_of(policy, warmup_steps=WARMUP_STEPS, max_epoch=MAX_EPOCH):
    solver = NS(OPTIMIZING_METHOD="sgd", BASE_LR=1.0, MOMENTUM=0.9, DAMPENING=0.0, NESTEROV=True, WEIGHT_DECAY=1e-4, LR_POLICY=policy,
                WARMUP_STEPS=warmup_steps, MAX_EPOCH=max_epoch, **EPOCH_POLICY)
    return NS(SOLVER=solver, BN=NS(WEIGHT_DECAY=0.0))


def record(lr_factory, policy, cfg, steps=STEPS, steps_in_epoch=STEPS_IN_EPOCH):
    import numpy as np
    import torch

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.bn = torch.nn.BatchNorm1d(2)
            self.fc = torch.nn.Linear(2, 2)
    model = Tiny()
    (opt,), (sched,) = lr_factory(model, cfg, steps_in_epoch, policy)
    assert sched["interval"] == "step" and len(opt.param_groups) == 2
    rows = []
    for _ in range(steps):
        rows.append([g["lr"] for g in opt.param_groups])
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        opt.step()
        sched["scheduler"].step()
    return np.asarray(rows, dtype=np.float64)


def recordings():
    import math
    import numpy as np
    from oracle import ref_harness as rh
    rh.use_tree("HOI")
    from optimizers.lta.lr_scheduler import lr_factory
    out = {}
    for policy in POLICIES:
        out["lr_" + policy] = record(lr_factory, policy, cfg_of(policy))
    for policy in ("cosine_warmup", "linear_warmup"):
        for w, e in EDGES:
            out[f"edge_{policy}_w{w}_t{e * STEPS_IN_EPOCH}"] = record(lr_factory, policy, cfg_of(policy, w, e))
    T = 50000
    rec = record(lr_factory, "cosine", cfg_of("cosine", max_epoch=T // STEPS_IN_EPOCH), steps=T + 1)[:, 0]
    closed = np.asarray([0.5 * (1.0 + math.cos(math.pi * k / T)) for k in range(T + 1)])
    pos = closed > 0
    out["cosine_recursive_vs_closed_T50000"] = np.asarray((np.abs(rec - closed)[pos] / closed[pos]).max())
    out["config"] = np.array(json.dumps(dict(steps=STEPS, steps_in_epoch=STEPS_IN_EPOCH, max_epoch=MAX_EPOCH, warmup_steps=WARMUP_STEPS,
                                             base_lr=1.0, policies=POLICIES, edges=EDGES, epoch_policy=EPOCH_POLICY)))
    return out


def main():
    import numpy as np
    out = recordings()
    if "--check" in sys.argv:
        z = np.load(FIXTURE)
        same = sorted(z.files) == sorted(out) and str(z["config"]) == str(out["config"])
        diff = max(float(np.abs(z[k] - out[k]).max()) for k in out if k != "config") if same else float("inf")
        print(f"check {same} max_diff {diff:.3e}")
        return 0 if same and diff == 0.0 else 1
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {os.path.relpath(FIXTURE, ROOT)}: {os.path.getsize(FIXTURE)} bytes; recursive vs closed cosine at T = 50000: "
          f"{float(out['cosine_recursive_vs_closed_T50000']):.2e}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
