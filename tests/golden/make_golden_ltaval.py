#!/usr/bin/env python3
"""Records live/lta_validation.npz: what the REAL `AUED` of the reference (HOI/evaluation/lta/lta_metrics.py:86-114) returns on two seeded
cases. Only runnable where the reference tree exists (it is imported here and nowhere else); the fixture travels with the repo and holds
data only.

    python tests/golden/make_golden_ltaval.py            # writes the fixture
    python tests/golden/make_golden_ltaval.py --check    # re-records and compares with the committed fixture

lta_metrics.py imports the `editdistance` package, which is not installed where this recording is made: sys.modules["editdistance"] gets a
stand-in before the import whose `eval` is the textbook Levenshtein recurrence of tests/lta_val_ref.py (insert, delete, substitute - what the
package computes, whatever the docstring at lta_metrics.py:88 says). Everything around it - the prefix loop, the minimum over the K sequences,
the division by the prefix length, the mean over clips, np.trapz - is the reference's own code.

Cases (predictions and labels uniform over the classes, so that prefixes match, mismatch and need shifts):
    a   N = 6, Z = 3, K = 5, 7 classes
    b   N = 4, Z = 20, K = 5, 115 classes
Arrays per case <c>: <c>_preds (N, Z, K) int64, <c>_labels (N, Z, 1) int64, <c>_AUED (1,) fp64, <c>_ED (Z,) fp64 (ED[z] = the reference's
`ED_z`, prefix length z + 1).
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(1, HERE)

FIXTURE = os.path.join(HERE, "live", "lta_validation.npz")
CASES = {"a": (6, 3, 5, 7, 4201), "b": (4, 20, 5, 115, 4202)}


def record(AUED, N, Z, K, classes, seed):
    import numpy as np
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    labels = torch.randint(0, classes, (N, Z, 1), generator=g)
    preds = torch.randint(0, classes, (N, Z, K), generator=g)
    # half of the predictions copy the label, some shifted by one step: distances between 0 and the prefix length
    copy = torch.rand(N, Z, K, generator=g) < 0.5
    preds = torch.where(copy, labels.expand(N, Z, K), preds)
    preds[:, 1:, 0] = torch.where(torch.rand(N, Z - 1, generator=g) < 0.5, labels[:, :-1, 0], preds[:, 1:, 0])
    out = AUED(preds.clone(), labels.clone())
    return {"preds": preds.numpy(), "labels": labels.numpy(), "AUED": np.asarray(out["AUED"], dtype=np.float64).reshape(1),
            "ED": np.asarray([np.asarray(out[f"ED_{z}"]).reshape(()) for z in range(Z)], dtype=np.float64)}


def recordings():
    from make_golden_ltacrit import _import_reference
    from oracle import ref_harness as rh
    from tests import lta_val_ref as vr
    stand_in = types.ModuleType("editdistance")
    stand_in.eval = vr.levenshtein
    sys.modules["editdistance"] = stand_in
    rh.use_tree("HOI")
    metrics = _import_reference("evaluation.lta.lta_metrics")
    assert metrics.editdistance is stand_in
    out = {}
    for name, (N, Z, K, classes, seed) in CASES.items():
        for k, v in record(metrics.AUED, N, Z, K, classes, seed).items():
            out[f"{name}_{k}"] = v
    return out


def main():
    import numpy as np
    out = recordings()
    if "--check" in sys.argv:
        z = np.load(FIXTURE)
        same = sorted(z.files) == sorted(out)
        diff = max(float(np.abs(z[k].astype(np.float64) - out[k].astype(np.float64)).max()) for k in out) if same else float("inf")
        print(f"check {same} max_diff {diff:.3e}")
        return 0 if same and diff == 0.0 else 1
    os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {os.path.relpath(FIXTURE, ROOT)}: {os.path.getsize(FIXTURE)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
