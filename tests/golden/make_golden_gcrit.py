#!/usr/bin/env python3
"""Records live/g_criterion.npz: what the EgoT2-g multi-task steps compute after the model on two seeded cases - Unified3TaskTranslation
(HHI/tasks/multitask/video_tasktranslation.py:39-66) and Unified6TaskTranslation (HOI/tasks/multitask/video_task.py:537-577, validation
:683-736) - with the REAL nn.CrossEntropyLoss on (B, V, sy) logits and the reference's own ARMetric, LTAMetric
(HOI/evaluation/lta/lta_metrics.py:164-211, 229-310), PNRMetric and OSCCMetric (HOI/evaluation/pnr/metrics.py:139-257) update / compute.
Only runnable where the reference tree exists (it is imported here and nowhere else); the fixture travels with the repo and holds data only.

    python tests/golden/make_golden_gcrit.py            # writes the fixture
    python tests/golden/make_golden_gcrit.py --check    # re-records and compares with the committed fixture

Import-time stand-ins only: torchmetrics.Metric is a base class that holds the states add_state declares (the metric classes use nothing
else of it), and map_label_to_action - whose taxonomy JSON is not part of the reference tree - returns a small synthetic taxonomy (5 verbs, 7 nouns).
Cases (logits = 3 * randn in the decoder's (sy, B, V) layout, the words of a task raised so that most rows peak inside them; no tied logits):
    hhi  V = 7,  T = 3 tasks (lam, ttm, asd), B = (5, 3, 9), sy = 2, ratios (1, 1, 0.5)
    hoi  V = 40, T = 6 tasks (pnr, oscc, ac_verb, ac_noun, lta_verb, lta_noun), B = (4, 6, 4, 4, 3, 3), sy = (2, 2, 2, 2, 4, 4)
Arrays per case <c> and task t:
    <c>_logits<t> (sy, B, V) fp32, <c>_target<t> (B, sy + 1) int64 (the step uses target[:, 1:]), <c>_ratios (T,) fp64
    <c>_loss_terms (T,) fp64 = nn.CrossEntropyLoss()(logits.double().permute(1, 2, 0), target[:, 1:]);  <c>_loss () fp64 = their ratio sum
hoi only (the metrics take the position-0 logits, which under the causal mask are predict()'s):
    hoi_wl<t> (V,) int32: the metric object's own word -> label mapping (pnr_indices, oscc_indices, verb_mapping, noun_mapping), -1 elsewhere
    hoi_labels<t> (B,) int64;  hoi_fps (B,) fp64, hoi_start / hoi_end / hoi_pnr (B,) int64: the PNR clips' timing
    hoi_pnrmetric (3,) = PNRMetric.compute() = (err / cnt, dist / cnt, cnt);  hoi_osccmetric (3,) = OSCCMetric.compute() = (error / cnt, correct / cnt, cnt)
    hoi_armetric (4,) = ARMetric.compute() = (v_err / v_cnt, n_err / n_cnt, v_correct / v_cnt, n_correct / n_cnt)
    hoi_ltametric (5,) = LTAMetric.compute() = (v_error / cnt, v_correct / cnt, n_error / cnt, n_correct / cnt, cnt)
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

FIXTURE = os.path.join(HERE, "live", "g_criterion.npz")
VERBS = {i: f"verb{i}" for i in range(5)}
NOUNS = {i: f"noun{i}" for i in range(7)}


def _import_reference(name):
    """Import a reference module; third-party packages it names but this recording never calls (torchtext, editdistance, loggers) are
    replaced by empty stand-ins."""
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


class Metric:
    """The part of torchmetrics.Metric the reference's metric classes use: the states add_state declares, held as attributes."""

    def __init__(self, *a, **k):
        pass

    def add_state(self, name, default, dist_reduce_fx=None):
        setattr(self, name, list(default) if isinstance(default, list) else default.clone())


def _logits(g, sy, B, V, words):
    import torch
    x = 3 * torch.randn(sy, B, V, generator=g)
    x[:, :, words] += 8.0                                   # most rows peak inside the task's words
    return x


def record_hhi():
    import numpy as np
    import torch
    g = torch.Generator(device="cpu").manual_seed(6101)
    V, ratios = 7, (1.0, 1.0, 0.5)
    out, terms = {"ratios": np.asarray(ratios)}, []
    criterion = torch.nn.CrossEntropyLoss()
    for t, B in enumerate((5, 3, 9)):
        logits = _logits(g, 2, B, V, [3, 4])
        target = torch.randint(0, V, (B, 3), generator=g)
        terms.append(criterion(logits.double().permute(1, 2, 0), target[:, 1:]))          # lines 48-59
        out[f"logits{t}"], out[f"target{t}"] = logits.numpy(), target.numpy()
    loss = ratios[0] * terms[0] + ratios[1] * terms[1] + ratios[2] * terms[2]             # line 61
    out["loss_terms"], out["loss"] = np.asarray([v.item() for v in terms]), np.asarray(loss.item())
    return out


def record_hoi(lta_metrics, pnr_metrics):
    import numpy as np
    import torch
    g = torch.Generator(device="cpu").manual_seed(6102)
    V, ratios = 40, (1.0, 1.0, 1.0, 1.0, 0.5, 0.5)
    perm = torch.randperm(V, generator=g).tolist()
    vocab = {str(i): perm[i] for i in range(16)}
    vocab["False"], vocab["True"] = perm[16], perm[17]
    for i, w in VERBS.items():
        vocab[w] = perm[18 + i]
    for i, w in NOUNS.items():
        vocab[w] = perm[23 + i]
    with contextlib.redirect_stdout(io.StringIO()):
        pnrmetric, osccmetric = pnr_metrics.PNRMetric(vocab), pnr_metrics.OSCCMetric(vocab)
        armetric, ltametric = lta_metrics.ARMetric(vocab), lta_metrics.LTAMetric(vocab)

    def as_map(mapping):
        m = np.full(V, -1, dtype=np.int32)
        for word, label in mapping.items():
            m[word] = label
        return m

    maps = [as_map({w: i for i, w in enumerate(pnrmetric.pnr_indices)}), as_map({w: i for i, w in enumerate(osccmetric.oscc_indices)}),
            as_map(armetric.verb_mapping), as_map(armetric.noun_mapping), as_map(ltametric.verb_mapping), as_map(ltametric.noun_mapping)]
    shapes = ((4, 2), (6, 2), (4, 2), (4, 2), (3, 4), (3, 4))
    n_labels = (16, 2, 5, 7, 5, 7)
    out, terms, first = {"ratios": np.asarray(ratios)}, [], []
    criterion = torch.nn.CrossEntropyLoss()
    for t, (B, sy) in enumerate(shapes):
        words = [int(w) for w in np.nonzero(maps[t] >= 0)[0]]
        logits = _logits(g, sy, B, V, words)
        outside = next(c for c in range(V) if maps[t][c] < 0)
        logits[0, 1, outside] = 40.0                        # one row whose free argmax is no word of the task
        target = torch.randint(0, V, (B, sy + 1), generator=g)
        terms.append(criterion(logits.double().permute(1, 2, 0), target[:, 1:]))          # lines 541-565
        labels = torch.randint(0, n_labels[t], (B,), generator=g)
        labels[0] = max(int(maps[t][int(logits[0, 0].argmax())]), 0)                            # one clip is predicted right
        first.append(logits[0])                             # position 0: the logits predict() sees
        out[f"logits{t}"], out[f"target{t}"], out[f"wl{t}"], out[f"labels{t}"] = logits.numpy(), target.numpy(), maps[t], labels.numpy()
    loss = sum(r * v for r, v in zip(ratios, terms))                                       # lines 567-568
    out["loss_terms"], out["loss"] = np.asarray([v.item() for v in terms]), np.asarray(loss.item())
    lab = [torch.from_numpy(out[f"labels{t}"]) for t in range(6)]
    # the validation step, lines 691-725
    B = shapes[0][0]
    fps = torch.where(torch.arange(B) % 2 == 0, torch.tensor(29.97, dtype=torch.float64), torch.tensor(30.0, dtype=torch.float64))
    start = torch.randint(0, 100000, (B,), generator=g)
    end = start + torch.randint(1, 400, (B,), generator=g)
    pnr = start + torch.randint(0, 400, (B,), generator=g)
    uid = [f"clip{i}" for i in range(8)]
    pnrmetric.pnr_dict = {u: i for i, u in enumerate(uid)}
    osccmetric.oscc_dict = {u: i for i, u in enumerate(uid)}
    ltametric.lta_mapping = {u: i for i, u in enumerate(uid)}
    with contextlib.redirect_stdout(io.StringIO()):
        pnrmetric.update(first[0], lab[0], fps, {"clip_start_frame": start, "clip_end_frame": end, "pnr_frame": pnr, "unique_id": uid[:B]})
        osccmetric.update(first[1], lab[1], {"unique_id": uid[:shapes[1][0]]})
        armetric.update(torch.stack([first[2].argmax(1), first[3].argmax(1)], dim=1), torch.stack([lab[2], lab[3]], dim=1))
        ltametric.update(torch.stack([first[4].argmax(1), first[5].argmax(1)], dim=1), torch.stack([lab[4], lab[5]], dim=1), uid[:shapes[4][0]])
        results = {"pnrmetric": pnrmetric.compute(), "osccmetric": osccmetric.compute(), "armetric": armetric.compute(),
                   "ltametric": ltametric.compute()}
    for k, v in results.items():
        out[k] = np.asarray([float(x) for x in v], dtype=np.float64)
    out.update(fps=fps.numpy(), start=start.numpy(), end=end.numpy(), pnr=pnr.numpy())
    return out


def recordings():
    from oracle import ref_harness as rh
    rh.use_tree("HOI")
    tm = sys.modules.get("torchmetrics") or types.ModuleType("torchmetrics")
    tm.Metric = Metric
    sys.modules["torchmetrics"] = tm
    lta_metrics = _import_reference("evaluation.lta.lta_metrics")
    pnr_metrics = _import_reference("evaluation.pnr.metrics")
    lta_metrics.map_label_to_action = lambda: (dict(VERBS), dict(NOUNS))
    out = {}
    for name, rec in (("hhi", record_hhi()), ("hoi", record_hoi(lta_metrics, pnr_metrics))):
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
