#!/usr/bin/env python3
"""Records live/view_ensemble.npz: what the test epoch of the action-recognition tasks computes on two seeded cases, for both ensemble
methods. The recording drives the REAL MultiTaskClassificationTask.test_epoch_end (HOI/tasks/lta/long_term_anticipation.py:96-158) as an
unbound function on a stub `self` - a cfg namespace (MODEL.NUM_CLASSES, DATA.ENSEMBLE_METHOD) and a collecting `log` -, with
du.all_gather / du.all_gather_unaligned as the identity of one process, and the reference's own topk_errors
(HOI/evaluation/lta/lta_metrics.py:38-84) behind it; the stacked per-video rows and labels are collected where it hands them to
topk_errors. (The preferred way of the two the task allows; the fallback - the real topk_errors around a restated loop - was not needed.)
Only runnable where the reference tree exists (it is imported here and nowhere else); the fixture travels with the repo and holds data only.

    python tests/golden/make_golden_viewens.py            # writes the fixture
    python tests/golden/make_golden_viewens.py --check    # re-records and compares with the committed fixture

Cases (tie-free, every label valid, fp32 logits as the reference keeps them):
    a   5 videos x 3 views, classes (5, 7), video after video
    b   4 videos x 30 views (TEST.NUM_ENSEMBLE_VIEWS x TEST.NUM_SPATIAL_CROPS), interleaved, classes (115, 478)
Arrays per case <c>: <c>_preds (N, sum classes) fp32 = 3 * randn, the label's logit lifted by BOOST[h] * (video + 1) / videos, <c>_labels (N, 2) int64 - the same for all views of a video, as a loader
yields them -, <c>_clip_ids (N,) int64 (the video of every clip), <c>_classes (2,); per method <m> in sum, max: <c>_<m>_rows (n, sum classes)
fp32 and <c>_<m>_video_labels (n, 2) as handed to topk_errors, <c>_<m>_err (4,) fp64: top1_verb_err, top5_verb_err, top1_noun_err,
top5_noun_err as `self.log(k, v.item())` received them.
"""
import importlib
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(HERE, "live", "view_ensemble.npz")
CASES = {"a": (5, 3, (5, 7), False, 5101), "b": (4, 30, (115, 478), True, 5102)}
METHODS = ("sum", "max")
BOOST = (3.0, 4.5)
ERR_KEYS = ("top1_verb_err", "top5_verb_err", "top1_noun_err", "top5_noun_err")


class _AnyMeta(type):
    def __getattr__(cls, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return cls


class _Any(metaclass=_AnyMeta):
    """What a stand-in module hands out for any name: a class that can be called, subclassed, used as a decorator and asked for
    attributes to any depth (av.container.Container in an annotation). Nothing recorded here ever runs it."""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return a[0] if len(a) == 1 and callable(a[0]) and not k else self

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self


def _import_reference(name):
    """Import a reference module; third-party packages it names but this recording never calls (video decoding, Lightning, fvcore,
    edit distance ...) are replaced by empty stand-ins."""
    for _ in range(64):
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
                    m.__getattr__ = lambda attr: _Any
                    sys.modules[mod_name] = m
    raise RuntimeError(f"could not import {name}")


def inputs(videos, views, classes, interleave, seed):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    N = videos * views
    preds = 3 * torch.randn(N, sum(classes), generator=g)
    video_labels = torch.stack([torch.randint(0, c, (videos,), generator=g) for c in classes], dim=-1)
    vid = torch.arange(videos).repeat_interleave(views)
    if interleave:
        vid = vid[torch.randperm(N, generator=g)]
    labels = video_labels[vid]
    col0 = 0
    for h, c in enumerate(classes):                     # lift the label's logit, more for later videos: some videos right, some wrong
        preds[torch.arange(N), col0 + labels[:, h]] += BOOST[h] * (vid.float() + 1) / videos
        col0 += c
    return preds, labels, vid


def record(task_module, preds, labels, vid, classes, method, batch=8):
    """One epoch through the real test_epoch_end: `outputs` is what test_step returns per batch."""
    import torch
    seen, logged = [], {}
    real = task_module.metrics.topk_errors

    def collecting_topk_errors(video_preds, video_labels, ks):
        seen.append((video_preds.clone(), video_labels.clone()))
        return real(video_preds, video_labels, ks)

    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(NUM_CLASSES=list(classes)), DATA=types.SimpleNamespace(ENSEMBLE_METHOD=method))
    stub = types.SimpleNamespace(cfg=cfg, log=lambda k, v: logged.__setitem__(k, v))
    verb, noun = torch.split(preds, list(classes), dim=-1)
    outputs = [{"preds_verb": verb[i:i + batch], "preds_noun": noun[i:i + batch], "labels": labels[i:i + batch],
                "clip_ids": [f"clip{int(v):03d}" for v in vid[i:i + batch]]} for i in range(0, preds.shape[0], batch)]
    saved = (task_module.du.all_gather, task_module.du.all_gather_unaligned, task_module.metrics.topk_errors)
    task_module.du.all_gather = lambda tensors: tensors                       # one process: the gathered list is the list
    task_module.du.all_gather_unaligned = lambda data: [data]
    task_module.metrics.topk_errors = collecting_topk_errors
    try:
        task_module.MultiTaskClassificationTask.test_epoch_end(stub, outputs)
    finally:
        task_module.du.all_gather, task_module.du.all_gather_unaligned, task_module.metrics.topk_errors = saved
    assert list(logged) == list(ERR_KEYS) and len(seen) == 2
    (verb_rows, verb_labels), (noun_rows, noun_labels) = seen
    rows = torch.cat([verb_rows, noun_rows], dim=1)
    assert rows.dtype == torch.float32
    for r, lab in ((verb_rows, verb_labels), (noun_rows, noun_labels)):          # tie-free where it matters: no class equals the label's value
        assert ((r == r.gather(1, lab.view(-1, 1))).sum(dim=1) == 1).all(), "a tie at the label: choose another seed"
    return rows, torch.stack([verb_labels, noun_labels], dim=1), [logged[k] for k in ERR_KEYS]


def recordings():
    import numpy as np
    from oracle import ref_harness as rh
    rh.use_tree("HOI")
    task_module = _import_reference("tasks.lta.long_term_anticipation")
    out = {}
    for name, (videos, views, classes, interleave, seed) in CASES.items():
        preds, labels, vid = inputs(videos, views, classes, interleave, seed)
        out[f"{name}_preds"], out[f"{name}_labels"] = preds.numpy(), labels.numpy()
        out[f"{name}_clip_ids"], out[f"{name}_classes"] = vid.numpy(), np.asarray(classes)
        for method in METHODS:
            rows, video_labels, errs = record(task_module, preds, labels, vid, classes, method)
            out[f"{name}_{method}_rows"], out[f"{name}_{method}_video_labels"] = rows.numpy(), video_labels.numpy()
            out[f"{name}_{method}_err"] = np.asarray(errs, dtype=np.float64)
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
