#!/usr/bin/env python3
"""Records live/segment_ap.npz: what the reference's validation epoch computes after the model on three seeded cases, with the REAL
PostProcessor.update / save / get_mAP -> run_evaluation of HHI/utils/ttm (utils.py:46-114, metrics.py:26-247) and HHI/utils/lam
(utils.py:24-81 and its metrics.py): the Python list of window outputs, the CSV files, `cat`, the pandas merge and sort, and the Python
loops of compute_average_precision. Only runnable where the reference tree exists (it is imported here and nowhere else); the fixture
travels with the repo and holds data only.

    python tests/golden/make_golden_segap.py            # writes the fixture
    python tests/golden/make_golden_segap.py --check    # re-records and compares with the committed fixture

Import-time stand-ins only: packages the modules name but this recording never calls (torchvision) are empty modules, and `np.float`, which
numpy 2 no longer has and metrics.py:47 compares dtypes with, is set to `float` before the import.
Cases (logits = a per-row difference uniform in [-6, 6] plus window noise; the generator asserts that no two rows share a score and, for
TTM, that no two segments share a start:end pair - the reference's uid there, which would merge them):
    ttm_a  N = 37 segments of 1 .. 7 windows, one update() call per segment chunk of 1 .. 3 windows      prevalence 0.5
    ttm_b  N = 300 segments of 1 .. 7 windows                                                            prevalence 0.1
    lam_a  N = 211 frames in batches of 16                                                               prevalence 0.3
Arrays per case <c>:
    <c>_logits (B, 2) fp32, <c>_slots (B,) int64 (the row of every window), <c>_labels (B,) int64 (per window; a row takes its first)
    <c>_score (N,) fp64: the score column of the prediction file, <c>_row_label (N,) int64: the label column of the ground-truth file
    <c>_AP (2,) fp64 = [AP0, AP1], <c>_mAP, <c>_acc fp64, <c>_confusion (4,) int64 = TP, FN, FP, TN
"""
import contextlib
import importlib
import io
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "live", "segment_ap.npz")


def _import_reference(name):
    """Import a reference module; third-party packages it names but this recording never calls are replaced by empty stand-ins."""
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
                    m.__getattr__ = lambda attr: type(attr, (), {"__init__": lambda self, *a, **k: None})
                    sys.modules[mod_name] = m
    raise RuntimeError(f"could not import {name}")


def _case(seed, n, max_windows, prevalence):
    import numpy as np
    rng = np.random.default_rng(seed)
    n_w = rng.integers(1, max_windows + 1, size=n) if max_windows > 1 else np.ones(n, dtype=np.int64)
    slots = np.repeat(np.arange(n, dtype=np.int64), n_w)
    diff, base = rng.uniform(-6.0, 6.0, size=n), rng.normal(size=n)
    logits = (np.stack([base[slots], (base + diff)[slots]], axis=1) + rng.normal(scale=1.5, size=(len(slots), 2))).astype(np.float32)
    row_label = (rng.random(n) < prevalence).astype(np.int64)
    row_label[:2] = (0, 1)                                      # both classes present
    labels = row_label[slots].copy()
    later = np.concatenate([[False], slots[1:] == slots[:-1]])
    labels[later] = 1 - labels[later]                           # only the first window's label reaches the ground-truth file
    return rng, logits, slots, labels


def _get_map(post, metrics_name):
    """post.get_mAP() -> (mAP, acc, [AP0, AP1] as compute_average_precision returned them, what run_evaluation printed)."""
    metrics = sys.modules[metrics_name]
    real, aps = metrics.compute_average_precision, []

    def recording(precision, recall):
        aps.append(float(real(precision, recall)))
        return aps[-1]

    metrics.compute_average_precision = recording
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            mAP, acc = post.get_mAP()
    finally:
        metrics.compute_average_precision = real
    assert len(aps) == 2
    return mAP, acc, aps, out.getvalue()


def _confusion(printed):
    """TP, FN, FP, TN as compute_confusion_matrix printed them ('TP a\\tFN b\\nFP c\\tTN d')."""
    import re
    m = re.search(r"TP (\d+)\tFN (\d+)\nFP (\d+)\tTN (\d+)", printed)
    return [int(v) for v in m.groups()]


def _read_back(exp_path):
    """The score and label columns of the merged files, in file (= row) order."""
    import pandas as pd
    pred = pd.read_csv(os.path.join(exp_path, "result", "pred.csv"), header=None)
    gt = pd.read_csv(os.path.join(exp_path, "result", "gt.csv"), header=None)
    return pred.iloc[:, -1].to_numpy(dtype="float64"), gt.iloc[:, -1].to_numpy(dtype="int64")


def record_ttm(ttm_utils, seed, n, prevalence):
    import numpy as np
    import torch
    rng, logits, slots, labels = _case(seed, n, 7, prevalence)
    starts = np.sort(rng.choice(100000, size=n, replace=False))
    ends = starts + rng.integers(5, 60, size=n)
    assert len({(int(s), int(e)) for s, e in zip(starts, ends)}) == n        # start:end is the reference's uid: unique, or rows would merge
    with tempfile.TemporaryDirectory() as exp:
        post = ttm_utils.PostProcessor(types.SimpleNamespace(exp_path=exp, rank=0))
        i = 0
        while i < len(slots):                                   # one update() per chunk of 1 .. 3 windows of ONE segment
            r = int(slots[i])
            j = min(i + int(rng.integers(1, 4)), int(np.searchsorted(slots, r, side="right")))
            targets = [[f"video{r % 5}"], None, torch.tensor(int(labels[i])), torch.tensor(int(starts[r])), torch.tensor(int(ends[r])),
                       torch.tensor(r)]
            post.update(torch.from_numpy(logits[i:j]), targets)
            i = j
        post.save()
        mAP, acc, aps, printed = _get_map(post, "utils.ttm.metrics")
        score, row_label = _read_back(exp)
    return _pack(logits, slots, labels, score, row_label, mAP, acc, aps, printed)


def record_lam(lam_utils, seed, n, prevalence):
    import numpy as np
    import torch
    rng, logits, slots, labels = _case(seed, n, 1, prevalence)
    with tempfile.TemporaryDirectory() as exp:
        post = lam_utils.PostProcessor(types.SimpleNamespace(exp_path=exp, rank=0))
        for i in range(0, n, 16):
            j = min(i + 16, n)
            box = [torch.from_numpy(rng.integers(0, 200, size=j - i)) for _ in range(4)]
            targets = [[f"video{r % 7}" for r in range(i, j)], [f"track{r % 3}" for r in range(i, j)], torch.arange(i, j), box,
                       torch.from_numpy(labels[i:j])]
            post.update(torch.from_numpy(logits[i:j]), targets)
        post.save()
        mAP, acc, aps, printed = _get_map(post, "utils.lam.metrics")
        score, row_label = _read_back(exp)
    return _pack(logits, slots, labels, score, row_label, mAP, acc, aps, printed)


def _pack(logits, slots, labels, score, row_label, mAP, acc, aps, printed):
    import numpy as np
    n = int(slots.max()) + 1
    assert len(score) == n and len(row_label) == n              # nothing was merged away or dropped
    assert len(set(score.tolist())) == n and len(set((1.0 - score).tolist())) == n       # tie-free in both classes' passes
    assert abs(np.mean(aps) - mAP) == 0.0
    return {"logits": logits, "slots": slots, "labels": labels, "score": score, "row_label": row_label,
            "AP": np.asarray(aps, dtype=np.float64), "mAP": np.asarray(float(mAP)), "acc": np.asarray(float(acc)),
            "confusion": np.asarray(_confusion(printed), dtype=np.int64)}


def recordings():
    import numpy as np
    from oracle import ref_harness as rh
    rh.use_tree("HHI")
    if not hasattr(np, "float"):
        np.float = float                                        # metrics.py:47 (numpy >= 1.24 dropped the alias)
    ttm_utils = _import_reference("utils.ttm.utils")
    lam_utils = _import_reference("utils.lam.utils")
    out = {}
    for name, rec in (("ttm_a", record_ttm(ttm_utils, 7101, 37, 0.5)), ("ttm_b", record_ttm(ttm_utils, 7102, 300, 0.1)),
                      ("lam_a", record_lam(lam_utils, 7103, 211, 0.3))):
        for k, v in rec.items():
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
