#!/usr/bin/env python3
"""Writes profiles/bf16_stage_report.txt: every case of tests/bf16_stage_ref.py on the GPU in compute bf16 and f32s, every stage's worst
device error as a fraction of its bar (what tests/test_gpu_bf16_stages.py asserts, as a table). Usage, from the repository root on a
machine with an MI355X:  python tools/bf16_stage_report.py [--out profiles/bf16_stage_report.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_stage_report.txt"))
    args = ap.parse_args()
    import torch
    from egot2_amd import functional as F
    F.reload_tuning_each_call = True        # the cases pin EGX_FFN_CUT / EGX_FFN_SLICES per run
    from tests import bf16_stage_ref as R
    from tests.test_gpu_bf16_stages import run_device
    cuda = torch.device("cuda:0")
    lines, worst_all = [], {}
    for case in R.CASES:
        for mode in ("bf16", "f32s"):
            st, sd, data = R.setup(case, mode)
            dev, absent = run_device(case, mode, st, sd, data, cuda)
            worst, detail, notes = R.stage_errors(st, dev)
            for k, v in worst.items():
                r = v / R.bar(k, mode)
                if (k, mode) not in worst_all or r > worst_all[(k, mode)][0]:
                    worst_all[(k, mode)] = (r, v, case.id, max(detail[k], key=lambda x: x[1])[0])
            lines.append(f"{case.id:22s} {mode:5s} " + " ".join(f"{k}={v / R.bar(k, mode):.2f}" for k, v in worst.items())
                         + f" | alive bad {notes['alive_bad']} skipped {notes['alive_skip']:.1e} | not kept: {', '.join(sorted(absent)) or '-'}"
                         + (f" | missing: {notes['missing']}" if notes["missing"] else ""))
    with open(args.out, "w") as f:
        f.write(f"Stage-wise bf16 gate on an MI355X (tools/bf16_stage_report.py; tests/test_gpu_bf16_stages.py, tests/bf16_stage_ref.py): worst device error of\n"
                f"every stage over the {len(R.CASES)} cases, as a fraction of its bar (8 x the fp32 yardstick). Every case runs in compute=bf16 against the rounding\n"
                "reference and in f32s against the unrounded one. 'not kept': items the stage hook reports as not held by that implementation (the\n"
                "log-sum-exp of a per-clip call).\n\n")
        f.write("stage           mode   worst error / bar   error      bar        case                    item\n")
        for (k, mode), (r, v, cid, item) in sorted(worst_all.items(), key=lambda kv: (R.STAGE_NAMES.index(kv[0][0]), kv[0][1])):
            f.write(f"{k:15s} {mode:5s}  {r:10.3f}          {v:.2e}   {R.bar(k, mode):.2e}   {cid:22s}  {item}\n")
        f.write("\nper case (error / bar of every stage):\n" + "\n".join(lines) + "\n")
    print(open(args.out).read().split("per case")[0])
    return 0 if all(r <= 1.0 for r, _, _, _ in worst_all.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
