#!/usr/bin/env python3
"""What the on-device learning-rate schedule and the fused SGD cost in the captured step -> profiles/solver_mi355x.json.

    python tools/solver_eval.py [--seconds 3] [--batch 256] [--out profiles/solver_mi355x.json]

The headline TTM configuration (synth c2: 3-task translator, B = 256, f32s, dropout 0.5 with the device-resident seed), one
train.GraphedStep per variant, the replays timed by device events in trials of --trial-steps steps, the variants ALTERNATED trial by trial
inside this one process until each has --seconds of replays behind it (after a warm-up):
    adam_by_value        FusedAdam(lr=5e-4): egx_counter_add + egx_adam_step, what bench.py --optimizer runs
    adam_warmup_cosine   FusedAdam + LRSchedule.warmup_cosine: egx_lr_update + egx_adam_step_dev_lr
    sgd_warmup_cosine    FusedSGD(momentum 0.9, Nesterov, weight decay 1e-4) + the same schedule: egx_lr_update + egx_sgd_step
    adam_constant / adam_table   FusedAdam + LRSchedule.constant() / a 64-entry table: the same two launches WITHOUT the fp64 cosine, which
                         splits what the schedule costs into the launches themselves and the one-lane cosine (diagnostic)
Reported per variant: median, p10 and p90 of the trial means (ms per step) and the library's launches per step. The expectation the
schedule is held to: adam_warmup_cosine's median inside adam_by_value's own p10 - p90 spread (`scheduled_median_inside_by_value_spread`).
Also: sgd_kernel alone on one flat buffer of the C4 (HOI LTA 4-task) translator's parameter count, momentum and Nesterov on, against
20 B per element over the HBM streaming rate a float4 copy reaches (MI355X: 6.29 TB/s measured) - a reported share, nothing is asserted.
A kernel trace is taken in a run of its own: rocprofv3 --kernel-trace --stats -d profiles/solver_trace -- python tools/solver_eval.py --seconds 0.2
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_STREAM_BPS = 6.29e12


def percentile(xs, q):
    xs = sorted(xs)
    i = q * (len(xs) - 1)
    lo, hi = int(i), min(int(i) + 1, len(xs) - 1)
    return xs[lo] + (xs[hi] - xs[lo]) * (i - lo)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0, help="replay time per variant")
    ap.add_argument("--trial-steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solver_mi355x.json"))
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("solver_eval.py needs a GPU: nothing here is measured on a CPU")
    from egot2_amd import _lib, synth
    from egot2_amd.train import FusedAdam, FusedSGD, GraphedStep, LRSchedule
    lib = _lib.load()
    dev = torch.device("cuda:0")
    sched = lambda: LRSchedule.warmup_cosine(500, 50000)  # noqa: E731
    variants = {
        "adam_by_value": lambda ps: FusedAdam(ps, lr=5e-4),
        "adam_warmup_cosine": lambda ps: FusedAdam(ps, lr=5e-4, schedule=sched()),
        "sgd_warmup_cosine": lambda ps: FusedSGD(ps, lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4, schedule=sched()),
        "adam_constant": lambda ps: FusedAdam(ps, lr=5e-4, schedule=LRSchedule.constant()),
        "adam_table": lambda ps: FusedAdam(ps, lr=5e-4, schedule=LRSchedule.from_factors([1.0 - k / 128 for k in range(64)])),
    }
    steps, launches, describe = {}, {}, None
    for name, make in variants.items():
        wl = synth.make_workload("c2", dev, batch=args.batch, dtype="f32s")
        model, describe = wl["model"], wl["describe"]
        model.enable_device_seed()
        model.enable_weight_cache(frozen=False)
        cw = torch.tensor([0.266, 0.734], device=dev)
        loss_fn = (lambda m, w: (lambda f, y: m.forward_features(*f, target=y, class_weight=w)[1]))(model, cw)
        target = torch.randint(0, 2, (wl["B"],), device=dev)
        step = GraphedStep(loss_fn, example_inputs=(wl["feats"], target), params=wl["params"], optimizer=make(wl["params"]))
        lib.egx_launch_count(1)
        step._step()                                   # one eager step: the library's launches of a step
        torch.cuda.synchronize()
        launches[name] = int(lib.egx_launch_count(1))
        steps[name] = step
    n = args.trial_steps
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def trial(step):
        ev[0].record()
        for _ in range(n):
            step.graph.replay()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]) / n           # ms per step
    for step in steps.values():                        # warm-up: every variant, two trials
        trial(step), trial(step)
    times = {k: [] for k in steps}
    while min(sum(t) * n for t in times.values()) < args.seconds * 1e3:
        for k, step in steps.items():                  # alternated: a, b, c, ..., a, b, c, ...
            times[k].append(trial(step))
    out = {"workload": describe + " + optimizer, one GraphedStep per variant, replays timed by device events", "trial_steps": n,
           "seconds_per_variant": args.seconds, "variants": {}}
    for k, t in times.items():
        out["variants"][k] = {"ms_per_step_median": percentile(t, 0.5), "p10": percentile(t, 0.1), "p90": percentile(t, 0.9),
                              "trials": len(t), "launches_per_step": launches[k]}
    a, b = out["variants"]["adam_by_value"], out["variants"]["adam_warmup_cosine"]
    out["scheduled_median_inside_by_value_spread"] = bool(a["p10"] <= b["ms_per_step_median"] <= a["p90"])
    out["scheduled_minus_by_value_us"] = (b["ms_per_step_median"] - a["ms_per_step_median"]) * 1e3

    # sgd_kernel alone, on the C4 translator's parameter count
    from egot2_amd import hoi_lta
    n_par = sum(p.numel() for p in hoi_lta.TaskFusionMFTransformerLTA4Task(synth.lta4_cfg(32, 768, 8, 4, 0.1)).parameters())
    p, g, buf = (torch.randn(n_par, device=dev) for _ in range(3))
    cnt = torch.full((), 2, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    call = lambda: _lib.check(lib.egx_sgd_step(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n_par, cnt.data_ptr(), None, 1e-6, 0.9, 0.0,  # noqa: E731
                                               1e-4, 1, 1.0, stream))
    for _ in range(20):
        call()
    ks = []
    for _ in range(15):
        ev[0].record()
        for _ in range(50):
            call()
        ev[1].record()
        ev[1].synchronize()
        ks.append(ev[0].elapsed_time(ev[1]) / 50 * 1e3)      # us per launch, back to back
    us = percentile(ks, 0.5)
    floor_us = 20.0 * n_par / HBM_STREAM_BPS * 1e6
    out["sgd_kernel_c4"] = {"elements": n_par, "bytes": 20 * n_par, "us_median": us, "p10": percentile(ks, 0.1), "p90": percentile(ks, 0.9),
                            "hbm_streaming_floor_us": floor_us, "share_of_streaming_rate": floor_us / us,
                            "note": "50 back-to-back launches per sample (includes the launch boundary); 20 B per element over 6.29 TB/s"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
