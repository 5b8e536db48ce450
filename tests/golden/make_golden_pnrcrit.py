#!/usr/bin/env python3
"""Records live/pnr_criterion.npz: what KeyframeLocalisation2Loader.training_step (HOI/tasks/pnr/video_taskspecific_pnr.py:24-63) and the
EgoT2-g validation (HOI/tasks/multitask/video_task.py:67,80) compute on two seeded cases, with the REAL nn.BCELoss / nn.CrossEntropyLoss
and the reference's own keyframe_distance, keyframe_accuracy and PnrOsccMetric (HOI/evaluation/pnr/metrics.py:23-134). Only runnable
where the reference tree exists (it is imported here and nowhere else); the fixture travels with the repo and holds data only.

    python tests/golden/make_golden_pnrcrit.py            # writes the fixture
    python tests/golden/make_golden_pnrcrit.py --check    # re-records and compares with the committed fixture

Cases (logits = 3 * randn, so |x| stays where fp64 BCELoss(sigmoid(x)) and the logit form agree; no tied logits):
    a   B = 6, T = 16 keyframe logits; B = 6, V = 40 decoder logits
    b   B = 4, T = 16 keyframe logits; B = 4, V = 593 decoder logits
Arrays per case <c>:
    <c>_logits (B, 1, 16) fp32, <c>_labels (B, 16) int64 one-hot, <c>_sc (B, 1) int64, <c>_fps (B,) fp64, <c>_start / _end / _pnr (B,) int64
    <c>_bce () fp64 = BCELoss(mean)(sigmoid(logits.double().squeeze(1)), labels.double())
    <c>_ce () fp64  = mean(sc.T * CrossEntropyLoss(none)(logits.double().permute(0, 2, 1).squeeze(-1), argmax(labels, 1)))
    <c>_dist () fp64 = keyframe_distance(logits, labels, sc, fps, info); <c>_acc (2,) int64 = keyframe_accuracy(...) = (correct, total)
    <c>_dec (B, V) fp32 decoder logits, <c>_pnr_cols (16,) / <c>_oscc_cols (2,) int64: the vocabulary's columns of '0'..'15' / 'False', 'True'
    <c>_pnr_distance (2,) fp64 = PnrOsccMetric.pnr_distance(dec, labels, fps, info) = (mean distance, error share)
    <c>_oscc_acc (2,) fp64 = PnrOsccMetric.oscc_acc(dec, sc) = (accuracy, error share)
"""
import contextlib
import importlib
import io
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "live", "pnr_criterion.npz")
CASES = {"a": (6, 40, 5101), "b": (4, 593, 5102)}


def _import_reference(name):
    """Import a reference module; third-party packages it names but this recording never calls (torchmetrics) are replaced by empty
    stand-ins."""
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


def record(metrics, B, V, seed):
    import numpy as np
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    logits = 3 * torch.randn(B, 1, 16, generator=g)
    frames = torch.randint(0, 16, (B,), generator=g)
    frames[0] = int(logits[0, 0].argmax())                  # one state-change clip is predicted right
    labels = torch.nn.functional.one_hot(frames, 16)
    sc = torch.randint(0, 2, (B, 1), generator=g)
    sc[0, 0], sc[1, 0] = 1, 0
    fps = torch.where(torch.arange(B) % 2 == 0, torch.tensor(29.97, dtype=torch.float64), torch.tensor(30.0, dtype=torch.float64))
    start = torch.randint(0, 100000, (B,), generator=g)
    end = start + torch.randint(1, 400, (B,), generator=g)
    pnr = start + torch.randint(0, 400, (B,), generator=g)
    info = {"clip_start_frame": start, "clip_end_frame": end, "pnr_frame": pnr}
    # training_step, lines 29-42, on the logits promoted to fp64
    x = logits.double()
    bce = torch.nn.BCELoss(reduction="mean")(torch.sigmoid(x.squeeze(dim=1)), labels.double())
    ce = torch.nn.CrossEntropyLoss(reduction="none")(x.permute(0, 2, 1).squeeze(dim=-1), torch.argmax(labels.long(), dim=1))
    ce = torch.mean(sc.T * ce)
    dist = metrics.keyframe_distance(logits, labels, sc, fps, info)
    correct, total = metrics.keyframe_accuracy(logits.squeeze(1), labels, sc)
    # the EgoT2-g validation: decoder logits over a vocabulary that holds '0'..'15', 'False', 'True' at scattered indices
    perm = torch.randperm(V, generator=g)[:18].tolist()
    vocab = {str(i): perm[i] for i in range(16)}
    vocab["False"], vocab["True"] = perm[16], perm[17]
    dec = 3 * torch.randn(B, V, generator=g)
    dec[:, perm] += 4.0                                     # most rows peak inside the vocabulary entries of the two tasks
    outside = next(c for c in range(V) if c not in perm)
    dec[1, outside] = 40.0                                  # one row whose unrestricted argmax is no vocabulary entry of either task
    with contextlib.redirect_stdout(io.StringIO()):         # the constructor prints its index lists
        m = metrics.PnrOsccMetric(vocab)
    pnr_distance = m.pnr_distance(dec, labels, fps, info)
    oscc_acc = m.oscc_acc(dec, sc)
    return {"logits": logits.numpy(), "labels": labels.numpy(), "sc": sc.numpy(), "fps": fps.numpy(), "start": start.numpy(),
            "end": end.numpy(), "pnr": pnr.numpy(), "bce": np.asarray(bce.item()), "ce": np.asarray(ce.item()),
            "dist": np.asarray(float(dist)), "acc": np.asarray([correct, total], dtype=np.int64), "dec": dec.numpy(),
            "pnr_cols": np.asarray(m.pnr_indices, dtype=np.int64), "oscc_cols": np.asarray(m.oscc_indices, dtype=np.int64),
            "pnr_distance": np.asarray([float(v) for v in pnr_distance]), "oscc_acc": np.asarray([float(v) for v in oscc_acc])}


def recordings():
    from oracle import ref_harness as rh
    rh.use_tree("HOI")
    metrics = _import_reference("evaluation.pnr.metrics")
    out = {}
    for name, (B, V, seed) in CASES.items():
        for k, v in record(metrics, B, V, seed).items():
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
