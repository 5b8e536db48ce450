#!/usr/bin/env python3
"""Records live/lta_criterion.npz: what the loop of LongTermAnticipationTask.training_step (HOI/tasks/lta/long_term_anticipation.py:182-203)
computes on two seeded cases, with the REAL nn.CrossEntropyLoss and the reference's own topk_errors / topks_correct
(HOI/evaluation/lta/lta_metrics.py:38-84). Only runnable where the reference tree exists (it is imported here and nowhere else); the
fixture travels with the repo and holds data only.

    python tests/golden/make_golden_ltacrit.py            # writes the fixture
    python tests/golden/make_golden_ltacrit.py --check    # re-records and compares with the committed fixture

Cases (every label valid and no tied logits: there the reference and egx_segmented_ce mean the same thing - with ignored labels the
reference's error divides by B and counts the row as wrong, and torch.topk leaves ties unspecified):
    a   B = 6, Z = 3, classes (5, 7): the small LTA model of the tests
    b   B = 4, Z = 20, classes (115, 478): the LTA heads at Z = 20
Arrays per case <c>: <c>_logits (B, Z, sum classes) fp32 = 3 * randn, <c>_labels (B, Z, H) int64, <c>_classes (H,), <c>_loss () fp64 - the
criterion on the logits promoted to fp64 -, <c>_top1_err / <c>_top5_err (Z, H) fp64 as the reference's `.item()` returns them.
"""
import importlib
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "live", "lta_criterion.npz")
CASES = {"a": (6, 3, (5, 7), 4101), "b": (4, 20, (115, 478), 4102)}


def _import_reference(name):
    """Import a reference module; third-party packages it names but this recording never calls (edit distance, average precision,
    loggers) are replaced by empty stand-ins."""
    for _ in range(32):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as e:
            top = (e.name or "").split(".")[0]
            if not top or os.path.exists(os.path.join(sys.path[0], top)):
                raise
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                mod_name = ".".join(parts[:i])
                if mod_name not in sys.modules:
                    m = types.ModuleType(mod_name)
                    m.__path__ = []
                    m.__getattr__ = lambda attr: type(attr, (), {"__init__": lambda self, *a, **k: None})     # callable, and a base class
                    sys.modules[mod_name] = m
    raise RuntimeError(f"could not import {name}")


def record(topk_errors, B, Z, classes, seed):
    import numpy as np
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = 3 * torch.randn(B, Z, sum(classes), generator=g)
    labels = torch.stack([torch.randint(0, c, (B, Z), generator=g) for c in classes], dim=-1)
    preds = torch.split(logits.double(), list(classes), dim=-1)
    loss_fun = torch.nn.CrossEntropyLoss()
    loss = 0
    errs = np.zeros((2, Z, len(classes)))
    for head_idx, pred_head in enumerate(preds):                       # the reference's loop, lines 184-195
        for seq_idx in range(pred_head.shape[1]):
            loss += loss_fun(pred_head[:, seq_idx], labels[:, seq_idx, head_idx])
            top1_err, top5_err = topk_errors(pred_head[:, seq_idx], labels[:, seq_idx, head_idx], (1, 5))
            errs[0, seq_idx, head_idx], errs[1, seq_idx, head_idx] = top1_err.item(), top5_err.item()
    return {"logits": logits.numpy(), "labels": labels.numpy(), "classes": np.asarray(classes), "loss": np.asarray(loss.item()),
            "top1_err": errs[0], "top5_err": errs[1]}


def recordings():
    from oracle import ref_harness as rh
    rh.use_tree("HOI")
    metrics = _import_reference("evaluation.lta.lta_metrics")
    out = {}
    for name, (B, Z, classes, seed) in CASES.items():
        for k, v in record(metrics.topk_errors, B, Z, classes, seed).items():
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
