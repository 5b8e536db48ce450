"""Training-step pieces around the translator: the TTM criterion and the optimizer.

`CrossEntropyLoss` mirrors `nn.CrossEntropyLoss(weight=...)` as built at HHI/tasks/ttm/video_task_2loader.py:21-22
(same constructor argument and `weight` buffer name, so Lightning checkpoints carrying `criterion.weight` load).
`FusedAdam` mirrors `torch.optim.Adam` / `AdamW` as configured at HHI/tasks/ttm/video_task_2loader.py:62-64 and
HOI/tasks/multitask/video_task.py:624-626: the translator's gradients already arrive as views of ONE flat buffer
(functional._GradPacker), so the parameters are re-pointed into a flat buffer with the same layout and the whole
update is a single launch per buffer, with the step count in device memory (hipGraph-replayable).
`FusedSGD` mirrors `torch.optim.SGD` as HOI/optimizers/lta/optimizer.py:54-62 builds it on the same machinery, `LRSchedule` the reference's
per-step learning-rate schedulers (HOI/optimizers/lta/lr_scheduler.py:11-41) evaluated on the device from that step count, and `construct_solver`
restates construct_optimizer + lr_factory on both.
`GradGuard` (and `grad_norm`) is what Lightning's Trainer offers as gradient_clip_val / track_grad_norm (left at their defaults by the reference,
HHI/scripts/run_ttm.py:21, HOI/scripts/lta/run_lta.py:238) for a captured step: the fp64 gradient norm in a fixed summation order, the clip
coefficient and the decision to skip a step with a non-finite gradient, all on the device, obeyed by the optimizers' bump and update launches.
`LTACriterion` is the criterion of the long-term-anticipation task (HOI/tasks/lta/long_term_anticipation.py:182-203: 40 cross-entropies
and the top-1 / top-5 errors of every (future step, head) pair) as one launch without a host synchronisation.
`LTAValidation` is that task's validation step (:222-248: K sampled futures per clip and head, and the edit distances behind AUED,
HOI/evaluation/lta/lta_metrics.py:86-114) as one launch, capturable, with one device-to-host copy in step_result().
`KeyframeCriterion` is the PNR keyframe task's step after the model (HOI/tasks/pnr/video_taskspecific_pnr.py:24-63: BCE or masked CE,
keyframe_distance and keyframe_accuracy of HOI/evaluation/pnr/metrics.py:23-80; with `cols` the EgoT2-g PnrOsccMetric) as one launch, and
`OSCCCriterion` the state-change classification step (:138-160) on the LTA criterion's launch.
`TranslationCriterion` is the criterion of the EgoT2-g multi-task steps (HHI/tasks/multitask/video_tasktranslation.py:39-66,
HOI/tasks/multitask/video_task.py:537-577, :683-736: 3 or 6 cross-entropies on (B, |V|, sy) logits times their ratios, and the counts behind
ARMetric / LTAMetric / PNRMetric / OSCCMetric) as one launch; `word_label_map` builds its vocabulary maps.
`SegmentAPValidation` is the validation epoch of the TTM and LAM tasks (HHI/tasks/ttm/video_task_2loader.py:38-50: PostProcessor.update /
save / get_mAP, HHI/utils/ttm/utils.py:46-114, and run_evaluation, HHI/utils/ttm/metrics.py:26-247 - the checkpoint metric val_mAP) as a
device-resident accumulator: reset / update per batch / step_result, with one 88-byte device-to-host copy per epoch.
`ViewEnsembleTest` is the test epoch of the action-recognition translators (HOI/tasks/lta/long_term_anticipation.py:86-158: the sum or max of
a video's clip predictions per clip id, then the top-1 / top-5 errors of verb and noun over the videos) on the same life cycle.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from . import functional as F_egx
from ._lib import check, ptr


class CrossEntropyLoss(nn.Module):
    def __init__(self, weight: Optional[torch.Tensor] = None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else weight.detach().clone().float())

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return F_egx.weighted_cross_entropy(input, target, self.weight)


class _DeviceCriterion(nn.Module):
    """What the one-launch criteria share: persistent result buffers per (device, *problem dims) - `_bufs`, laid out by the subclass's
    `_allocate(device, *dims)` - and `_last`, the buffers of the most recent forward, which every call or replay refreshes."""

    def __init__(self):
        super().__init__()
        self._bufs: Dict[tuple, dict] = {}
        self._last: Optional[dict] = None

    @staticmethod
    def _capturing(device) -> bool:
        return device.type == "cuda" and torch.cuda.is_current_stream_capturing()

    def _result_buffers(self, device, *dims) -> dict:
        device = torch.device(device)
        key = (device.type, device.index, *dims)
        b = self._bufs.get(key)
        if b is None:
            if self._capturing(device):
                # a buffer created inside a capture would live in that graph's private pool
                raise RuntimeError(f"{type(self).__name__}: run one eager step at this problem size before capturing it in a graph")
            b = self._bufs[key] = self._allocate(device, *dims)
        return b

    def _latest(self) -> dict:
        if self._last is None:
            raise RuntimeError(f"{type(self).__name__}: no forward has run yet")
        return self._last


class LTACriterion(_DeviceCriterion):
    """The criterion of the long-term-anticipation task, LongTermAnticipationTask.training_step (HOI/tasks/lta/long_term_anticipation.py:182-203):

        loss = sum over heads h, future steps z of nn.CrossEntropyLoss()(preds[h][:, z], labels[:, z, h])
        step_result[f"train_{z}_{h}_top{k}_err"] = topk_errors(preds[h][:, z], labels[:, z, h], (1, 5))[..].item()

    as ONE launch (functional.segmented_cross_entropy) without a host synchronisation, so it can be the `loss_fn` of a GraphedStep; the
    reference's 40 cross-entropy calls, 40 topk calls and 80 `.item()` reads become that launch plus ONE device-to-host copy in
    `step_result()`. preds: the list of (B, Z, C_h) tensors `forward_features` of the LTA translators returns; labels: int64 (B, Z, H).

    The loss, its (Z, H) terms, the valid-label counts and the top-k correct counts live in ONE persistent buffer per (device, Z, H),
    allocated on the first eager call (a capture cannot allocate it: run an eager step first, GraphedStep's warm-up does) and refreshed by
    every call or replay. Labels outside [0, C_h) are ignored; a (z, h) pair without a valid label adds 0 to the loss and reports nan errors;
    among equal logits the lower class index ranks first."""

    def __init__(self, ks=(1, 5)):
        super().__init__()
        self.ks = tuple(int(k) for k in ks)
        if not 1 <= len(self.ks) <= F_egx.SEG_CE_MAX_KS or min(self.ks) < 1:
            raise ValueError(f"LTACriterion: ks={ks} (needs 1 to {F_egx.SEG_CE_MAX_KS} values >= 1)")

    def _allocate(self, device, Z: int, H: int) -> dict:
        """loss | loss_terms (Z, H) | n_valid (Z, H) | correct (len(ks), Z, H) as views of one buffer of 4-byte words (`flat`)."""
        n = Z * H
        flat = torch.zeros(1 + n * (2 + len(self.ks)), dtype=torch.int32, device=device)
        return {"flat": flat, "Z": Z, "H": H,
                "loss": flat[0:1].view(torch.float32).view(()),
                "loss_terms": flat[1:1 + n].view(torch.float32).view(Z, H),
                "n_valid": flat[1 + n:1 + 2 * n].view(Z, H),
                "correct": flat[1 + 2 * n:].view(len(self.ks), Z, H)}

    def forward(self, preds, labels: torch.Tensor) -> torch.Tensor:
        preds = list(preds)
        b = self._result_buffers(preds[0].device, preds[0].shape[1], len(preds))
        loss, _ = F_egx.segmented_cross_entropy(preds, labels, self.ks, out=b)
        self._last = b
        return loss

    def stats(self) -> dict:
        """Device tensors of the most recent call (or replay): `loss`, `loss_terms`, `n_valid`, `correct`. Reading them does not synchronise."""
        b = self._latest()
        return {k: b[k] for k in ("loss", "loss_terms", "n_valid", "correct")}

    def host_result(self):
        """-> (loss, n_valid (Z, H), correct (len(ks), Z, H)) of the most recent call (or replay) as host values, from ONE device-to-host
        copy of `flat` (it synchronises)."""
        b = self._latest()
        Z, H, n = b["Z"], b["H"], b["Z"] * b["H"]
        host = b["flat"].cpu().numpy()
        return float(host[0:1].view("float32")[0]), host[1 + n:1 + 2 * n].reshape(Z, H), host[1 + 2 * n:].reshape(len(self.ks), Z, H)

    def step_result(self, prefix: str = "train") -> Dict[str, float]:
        """The reference's step_result of the most recent call (or replay), from ONE device-to-host copy (it synchronises: for logging):
        f"{prefix}_{z}_{h}_top{k}_err" = (1 - correct / n_valid) * 100 for every k of `ks`, f"{prefix}_{h}_top{k}_err" = their mean over z,
        f"{prefix}_loss"."""
        loss, n_valid, correct = self.host_result()
        (Z, H), n_valid, correct = n_valid.shape, n_valid.astype("float64"), correct.astype("float64")
        res: Dict[str, float] = {}
        for ki, k in enumerate(self.ks):
            for h in range(H):
                errs = []
                for z in range(Z):
                    nv = n_valid[z, h]
                    e = (1.0 - correct[ki, z, h] / nv) * 100.0 if nv > 0 else float("nan")
                    res[f"{prefix}_{z}_{h}_top{k}_err"] = float(e)
                    errs.append(e)
                res[f"{prefix}_{h}_top{k}_err"] = float(sum(errs) / len(errs))
        res[f"{prefix}_loss"] = loss
        return res


class LTAValidation(_DeviceCriterion):
    """The validation step of the long-term-anticipation task, LongTermAnticipationTask.validation_step
    (HOI/tasks/lta/long_term_anticipation.py:222-248; :313-341 for the sequence tasks):

        preds = model.generate(input, k=K)                                   # K x Categorical(logits).sample() per head, argmax at K = 1
        step_result[f"val_{h}_" + key] = AUED(pred.permute(0, 2, 1).cpu(), labels[:, :, h:h + 1])[key]       # one .cpu() per head, a Python
                                                                             # loop of editdistance.eval (evaluation/lta/lta_metrics.py:86-114)

    as ONE launch (functional.lta_validate) without a host synchronisation, capturable in a graph; `step_result()` is ONE device-to-host copy.
    preds: the list of (B, Z, C_h) tensors `forward_features` of the LTA translators returns; labels: int64 (B, Z, H).

    The tokens (H, B, K, Z), min_dist (B, Z, H) and dist_sum (Z, H) live in persistent buffers per (device, B, Z, H), allocated on the first
    eager call (a capture cannot allocate them: run an eager call first) and refreshed by every call or replay. The module owns a seed word
    per device; every call reads it on the stream and enqueues egx_seed_advance behind the launch, so consecutive calls - and replays of a
    captured call - draw fresh sequences. `manual_seed(s)` sets it. A host `seed=` (repeatable draws) is refused inside a capture when K > 1,
    as a host dropout seed is. A row with a NaN or +inf, or without a finite logit, yields token -1 (the reference raises); ties at K = 1 go
    to the lowest index."""

    def __init__(self, k: int = 5):
        super().__init__()
        self.k = int(k)
        if not 1 <= self.k <= F_egx.LTA_VAL_MAX_K:
            raise ValueError(f"LTAValidation: k={k} (needs 1 <= k <= {F_egx.LTA_VAL_MAX_K} sequences per clip)")
        self._seeds: Dict[tuple, torch.Tensor] = {}
        self._seed0: Optional[int] = None

    def manual_seed(self, s: int) -> "LTAValidation":
        """Set the device seed word (of every device used so far, and of those to come) to `s`."""
        self._seed0 = int(s) & (2**64 - 1)
        signed = self._seed0 - (1 << 64) if self._seed0 >= (1 << 63) else self._seed0
        for t in self._seeds.values():
            t.fill_(signed)
        return self

    def seed_word(self, device) -> torch.Tensor:
        """The one-element int64 device tensor that holds the seed the NEXT call on `device` draws with (its bits are the uint64 seed)."""
        device = torch.device(device)
        key = (device.type, device.index)
        t = self._seeds.get(key)
        if t is None:
            if self._capturing(device):
                raise RuntimeError("LTAValidation: run one eager step at this problem size before capturing it in a graph")
            s = self._seed0 if self._seed0 is not None else (torch.initial_seed() * 0x9E3779B97F4A7C15 + 0x17A) & (2**64 - 1)
            t = self._seeds[key] = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s], dtype=torch.int64, device=device)
        return t

    def _allocate(self, device, B: int, Z: int, H: int) -> dict:
        return {"B": B, "Z": Z, "H": H,
                "preds": torch.zeros((H, B, self.k, Z), dtype=torch.int64, device=device),
                "min_dist": torch.zeros((B, Z, H), dtype=torch.int32, device=device),
                "dist_sum": torch.zeros((Z, H), dtype=torch.int64, device=device)}

    def forward(self, preds, labels: torch.Tensor, seed: Optional[int] = None):
        """-> tokens, the list of (B, K, Z) int64 tensors `generate` returns (views of the persistent buffer). seed: a host seed for
        repeatable draws (the device word is then neither read nor advanced)."""
        preds = list(preds)
        dev = preds[0].device
        b = self._result_buffers(dev, preds[0].shape[0], preds[0].shape[1], len(preds))
        if seed is not None:
            if self.k > 1 and self._capturing(dev):
                raise RuntimeError("LTAValidation: k > 1 draws with a host seed cannot be captured in a graph: every replay would repeat the same "
                                   "sequences; leave seed=None (the device seed word advances on the stream)")
            tokens, _ = F_egx.lta_validate(preds, labels, self.k, seed=seed, out=b)
        else:
            word = self.seed_word(dev)
            tokens, _ = F_egx.lta_validate(preds, labels, self.k, seed_ptr=word, out=b)
            _lib.check(_lib.load().egx_seed_advance(word.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self._last = b
        return tokens

    def stats(self) -> dict:
        """Device tensors of the most recent call (or replay): `tokens` (H, B, K, Z), `min_dist`, `dist_sum`. Reading them does not synchronise."""
        b = self._latest()
        return {"tokens": b["preds"], "min_dist": b["min_dist"], "dist_sum": b["dist_sum"]}

    def step_result(self, prefix: str = "val") -> Dict[str, float]:
        """The reference's step_result of the most recent call (or replay), from ONE device-to-host copy (it synchronises), in fp64:
        f"{prefix}_{h}_ED_{z}" = dist_sum[z, h] / (B (z + 1)), f"{prefix}_{h}_AUED" = trapz over z / (Z - 1) (nan at Z = 1, as numpy gives
        the reference). Across ranks: all-reduce dist_sum and B first."""
        b = self._latest()
        import numpy as np
        B, Z, H = b["B"], b["Z"], b["H"]
        ds = b["dist_sum"].cpu().numpy().astype(np.float64)
        res: Dict[str, float] = {}
        for h in range(H):
            ed = ds[:, h] / (B * np.arange(1, Z + 1, dtype=np.float64))
            with np.errstate(invalid="ignore", divide="ignore"):
                area = float(((ed[1:] + ed[:-1]) / 2.0).sum()) if Z > 1 else 0.0        # np.trapz, dx = 1
                res[f"{prefix}_{h}_AUED"] = float(np.float64(area) / np.float64(Z - 1))
            for z in range(Z):
                res[f"{prefix}_{h}_ED_{z}"] = float(ed[z])
        return res


class KeyframeCriterion(_DeviceCriterion):
    """The training / validation step of the PNR keyframe task after the model, KeyframeLocalisation2Loader.training_step
    (HOI/tasks/pnr/video_taskspecific_pnr.py:24-63, recipe HOI/configs/pnr/ts_pnr.yaml: LOSS_FUNC "bce"):

        loss = BCELoss(mean)(sigmoid(preds.squeeze(1)), labels.float())       # "cross_entropy": mean(state_change_label.T * CE(preds, argmax(labels)))
        keyframe_distance(preds, labels, state_change_label, fps, info), keyframe_accuracy(...)          # evaluation/pnr/metrics.py:23-80

    as ONE launch (functional.keyframe_criterion) without a host synchronisation, so it can be the `loss_fn` of a GraphedStep; the reference's
    two Python loops with four to six `.item()` reads per clip become that launch plus ONE device-to-host copy in `step_result()`.
    preds: the (B, 1, T) tensor `forward_features` of the PNR translators returns (or (B, T)); labels: the one-hot (B, T) labels.

    With `cols=` (the vocabulary columns of the frames) and `loss_func=None` it is the EgoT2-g metric on (B, V) decoder logits,
    PnrOsccMetric.pnr_distance / oscc_acc (metrics.py:102-134); `labels` is then the int64 (B,) label index (for the two-column OSCC use: the
    state-change label) or None.

    loss, the four counts and dist_sum live in ONE persistent buffer per (device, B, T), the per-clip results next to it, allocated on the
    first eager call (a capture cannot allocate them: run an eager step first, GraphedStep's warm-up does) and refreshed by every call or
    replay. The loss is evaluated in logit form (where fp32 sigmoid saturates, BCELoss(sigmoid(x)) returns its clamp of 100 and a zero
    gradient; this returns the true softplus and sigmoid - y), and pseudo_acc without a state-change clip is NaN (the reference divides by
    zero)."""

    def __init__(self, loss_func: Optional[str] = "bce", cols=None):
        super().__init__()
        if loss_func not in F_egx.KEYFRAME_KINDS:
            raise ValueError(f"KeyframeCriterion: loss_func={loss_func!r} (needs 'bce', 'cross_entropy' or None)")
        self.loss_func = loss_func
        self.cols = None if cols is None else tuple(int(c) for c in cols)
        if self.cols is not None and not 1 <= len(self.cols) <= F_egx.KEYFRAME_MAX_T:
            raise ValueError(f"KeyframeCriterion: {len(self.cols)} columns (needs 1 to {F_egx.KEYFRAME_MAX_T} frames)")

    def _allocate(self, device, B: int, T: int) -> dict:
        """dist_sum (fp64) | loss | pad | counts [n_sc, n_correct, n_outside, B] as views of one buffer of 4-byte words (`flat`), and the
        per-clip pred, label_frame, loss_rows, dist."""
        flat = torch.zeros(8, dtype=torch.int32, device=device)
        return {"flat": flat, "B": B, "T": T,
                "dist_sum": flat[0:2].view(torch.float64).view(()),
                "loss": flat[2:3].view(torch.float32).view(()),
                "counts": flat[4:8],
                "pred": torch.zeros(B, dtype=torch.int32, device=device),
                "label_frame": torch.zeros(B, dtype=torch.int32, device=device),
                "loss_rows": torch.zeros(B, dtype=torch.float32, device=device),
                "dist": torch.zeros(B, dtype=torch.float64, device=device)}

    def forward(self, preds, labels=None, state_change_label=None, fps=None, info=None):
        """-> loss (None with loss_func=None). labels: (B, T) one-hot (the reference's `labels`), or - the metric with cols - the (B,) /
        (B, 1) int64 label index."""
        B = preds.shape[0]
        T = len(self.cols) if self.cols is not None else preds.shape[-1]
        b = self._result_buffers(preds.device, B, T)
        target = label = None
        if labels is not None:
            if labels.dim() == 2 and tuple(labels.shape) == (B, T) and (T > 1 or self.loss_func is not None):
                target = labels
            else:
                label = labels
        loss, _ = F_egx.keyframe_criterion(preds, target, label, state_change_label, fps, info, kind=self.loss_func, cols=self.cols, out=b)
        b["timed"] = fps is not None
        self._last = b
        return loss

    def stats(self) -> dict:
        """Device tensors of the most recent call (or replay): `loss`, `counts`, `dist_sum`, `pred`, `label_frame`, `loss_rows`, `dist`.
        Reading them does not synchronise. What that call did not write is None, as functional.keyframe_criterion returns it: `dist` and
        `dist_sum` without fps / info, `loss` and `loss_rows` with loss_func=None."""
        b = self._latest()
        unwritten = (() if b.get("timed", True) else ("dist", "dist_sum")) + (("loss", "loss_rows") if self.loss_func is None else ())
        return {k: None if k in unwritten else b[k] for k in ("loss", "counts", "dist_sum", "pred", "label_frame", "loss_rows", "dist")}

    def step_result(self, prefix: str = "train") -> Dict[str, float]:
        """The reference's step_result of the most recent call (or replay), from ONE device-to-host copy (it synchronises: for logging).
        "train": keyframe_loss, train_loss, loss, pseudo_acc = n_correct / n_sc (nan without a state-change clip),
        keyframe_loc_metric_time_dist_train = dist_sum / n_sc (0.0 without one, as the reference returns). "val":
        keyframe_loc_metric_time_dist_val, its negative (the checkpoint metric) and pseudo_acc. With cols and loss_func=None (the EgoT2-g
        metric, any prefix): dist = dist_sum / B, err = n_outside / B, acc = n_correct / B. Across ranks: all-reduce counts and dist_sum."""
        b = self._latest()
        host = b["flat"].cpu().numpy()
        dist_sum = float(host[0:2].view("float64")[0]) if b.get("timed", True) else float("nan")      # no fps / info: no distance
        loss = float(host[2:3].view("float32")[0])
        n_sc, n_correct, n_outside, B = (int(v) for v in host[4:8])
        if self.cols is not None and self.loss_func is None:
            return {"dist": dist_sum / B, "err": n_outside / B, "acc": n_correct / B}
        acc = n_correct / n_sc if n_sc > 0 else float("nan")
        dist = dist_sum / n_sc if n_sc > 0 else 0.0
        if prefix == "train":
            return {"keyframe_loss": loss, "train_loss": loss, "loss": loss, "pseudo_acc": acc, "keyframe_loc_metric_time_dist_train": dist}
        if prefix == "val":
            return {"keyframe_loc_metric_time_dist_val": dist, "keyframe_loc_metric_time_dist_val_neg": -dist, "pseudo_acc": acc}
        raise ValueError(f"KeyframeCriterion.step_result: prefix={prefix!r} (needs 'train' or 'val')")


class OSCCCriterion(nn.Module):
    """The training step of the state-change classification task after the model, StateChangeClassification2Loader.training_step
    (HOI/tasks/pnr/video_taskspecific_pnr.py:138-160): mean cross-entropy of the (B, 2, 1) output against the state-change label plus
    state_change_accuracy (evaluation/pnr/metrics.py:11-20), as functional.segmented_cross_entropy with one future step, one head and
    ks = (1,): one launch, no host synchronisation, `step_result()` is one device-to-host copy. Among equal logits the lower class wins."""

    def __init__(self):
        super().__init__()
        self._crit = LTACriterion(ks=(1,))
        self._B = 0

    def forward(self, preds: torch.Tensor, state_change_label: torch.Tensor) -> torch.Tensor:
        if preds.dim() != 3 or preds.shape[2] != 1:
            raise ValueError(f"OSCCCriterion expects the (B, classes, 1) output of the OSCC translator, got {tuple(preds.shape)}")
        B = preds.shape[0]
        self._B = B
        return self._crit([preds.squeeze(2).unsqueeze(1)], state_change_label.reshape(B, 1, 1).long())

    def stats(self) -> dict:
        return self._crit.stats()

    def step_result(self, prefix: str = "train") -> Dict[str, float]:
        """"train": state_change_loss, train_loss, loss, state_change_metric_train = correct / B; "val": state_change_metric_val."""
        if self._crit._last is None:
            raise RuntimeError("OSCCCriterion: no forward has run yet")
        loss, _, correct = self._crit.host_result()             # one future step, one head, ks = (1,)
        acc = int(correct[0, 0, 0]) / max(self._B, 1)
        if prefix == "train":
            return {"state_change_loss": loss, "train_loss": loss, "loss": loss, "state_change_metric_train": acc}
        if prefix == "val":
            return {"state_change_metric_val": acc}
        raise ValueError(f"OSCCCriterion.step_result: prefix={prefix!r} (needs 'train' or 'val')")


def word_label_map(vocab, label_words, size: Optional[int] = None) -> torch.Tensor:
    """int32 (V,): the original label of every vocabulary word, -1 for a word that stands for none - the `word_labels` of
    TranslationCriterion. vocab: a dict, or anything indexable by word (the reference's Vocabulary), word -> index; label_words:
    {label: word} (the verb / noun dictionaries of map_label_to_action). A word that serves several labels keeps the LATER one, as the
    reference's _map_vocab_to_orig_idx does (HOI/evaluation/lta/lta_metrics.py:178-183). size: V, default len(vocab)."""
    V = int(size) if size is not None else len(vocab)
    m = torch.full((V,), -1, dtype=torch.int32)
    for label, word in label_words.items():
        idx = int(vocab[word])
        if not 0 <= idx < V:
            raise ValueError(f"word_label_map: word {word!r} has index {idx}, outside the vocabulary of {V} words")
        if int(label) < 0:
            raise ValueError(f"word_label_map: label {label!r} of word {word!r} is negative (negative labels mean 'no label')")
        m[idx] = int(label)
    return m


def binary_word_labels(vocab, size: Optional[int] = None) -> torch.Tensor:
    """{'0': 0, '1': 1}: the HHI tasks' answers (Accuracy() on predict(...)[:, -2:], HHI/tasks/multitask/video_tasktranslation.py:101-102)."""
    return word_label_map(vocab, {0: "0", 1: "1"}, size)


def oscc_word_labels(vocab, size: Optional[int] = None) -> torch.Tensor:
    """{'False': 0, 'True': 1}: OSCCMetric's oscc_indices (HOI/evaluation/pnr/metrics.py:224-226)."""
    return word_label_map(vocab, {0: "False", 1: "True"}, size)


def pnr_word_labels(vocab, size: Optional[int] = None) -> torch.Tensor:
    """{'0': 0, ..., '15': 15}: PNRMetric's pnr_indices (HOI/evaluation/pnr/metrics.py:163-167)."""
    return word_label_map(vocab, {i: str(i) for i in range(16)}, size)


class TranslationCriterion(_DeviceCriterion):
    """The criterion of an EgoT2-g multi-task step, Unified3TaskTranslation.training_step (HHI/tasks/multitask/video_tasktranslation.py:39-66)
    and Unified6TaskTranslation.training_step / validation_step (HOI/tasks/multitask/video_task.py:537-577, :683-736):

        loss_t = nn.CrossEntropyLoss()(logits_t, target_t[:, 1:]);  loss = sum_t ratio_t * loss_t;  self.log(..., loss_t.item())
        metric_t.update(self.model.predict(...), labels_t)           # a second forward per task, Python loops with .item() per clip

    as ONE launch (functional.sequence_cross_entropy) without a host synchronisation, so it can be the `loss_fn` of a GraphedStep; the
    reference's 3 (6) cross-entropy calls - each on a copy of the permuted decoder output - and 4 (7) `.item()` reads become that launch
    plus ONE device-to-host copy in `step_result()`. With the causal mask the position-0 logits of the teacher-forced forward are those
    of predict(), so in eval mode the forward that gives the loss gives the metrics too.

    ratios: one float per task; names: the log names (default: the reference's for 3 and 6 tasks); word_labels: per task None or the int32
    (V,) map of `word_label_map` (a task with a map takes labels in forward). All results live in ONE persistent buffer per (device, T),
    allocated on the first eager call (a capture cannot allocate it: run an eager step first, GraphedStep's warm-up does) and refreshed by
    every call or replay. Labels outside [0, V) are ignored; a task without a valid label adds 0 to the loss (torch: nan); among equal
    logits the lower word wins."""
    NAMES = {3: ("lam", "ttm", "asd"), 6: ("pnr", "oscc", "ac_verb", "ac_noun", "lta_verb", "lta_noun")}

    def __init__(self, ratios, names=None, word_labels=None, want_pred: bool = False):
        super().__init__()
        self.ratios = tuple(float(r) for r in ratios)
        T = len(self.ratios)
        if not 1 <= T <= F_egx.SEQ_CE_MAX_TASKS:
            raise ValueError(f"TranslationCriterion: {T} ratios (needs 1 to {F_egx.SEQ_CE_MAX_TASKS} tasks)")
        self.names = tuple(names) if names is not None else self.NAMES.get(T, tuple(f"task{t}" for t in range(T)))
        if len(self.names) != T or len(set(self.names)) != T:
            raise ValueError(f"TranslationCriterion: names={self.names} (needs {T} distinct names)")
        word_labels = list(word_labels) if word_labels is not None else [None] * T
        if len(word_labels) != T:
            raise ValueError(f"TranslationCriterion: {len(word_labels)} word_labels for {T} tasks")
        self._maps = [None if m is None else torch.as_tensor(m).to(dtype=torch.int32, device="cpu").contiguous() for m in word_labels]
        self._maps_dev: Dict[tuple, list] = {}
        self.want_pred = bool(want_pred)
        self._pred = None

    def _allocate(self, device, T: int) -> dict:
        """loss | loss_terms (T) | n_valid | token_correct | seq_correct | scored | invalid | correct | correct_restricted (T each) as views of
        one buffer of 4-byte words (`flat`)."""
        flat = torch.zeros(1 + 8 * T, dtype=torch.int32, device=device)
        return {"flat": flat, "T": T, **F_egx.sequence_ce_views(flat, T)}

    def _device_maps(self, device) -> list:
        device = torch.device(device)
        key = (device.type, device.index)
        m = self._maps_dev.get(key)
        if m is None:
            if self._capturing(device) and any(x is not None for x in self._maps):
                raise RuntimeError(f"{type(self).__name__}: run one eager step at this problem size before capturing it in a graph")
            m = self._maps_dev[key] = [None if x is None else x.to(device) for x in self._maps]
        return m

    def forward(self, logits_list, targets_list, labels_list=None) -> torch.Tensor:
        """-> loss. logits_list: the tasks' (B_t, V, sy_t) logits; targets_list: their int64 (B_t, sy_t) targets (target[:, 1:] views are
        read in place); labels_list: per task the int64 original labels ((B_t, sy_t), < 0 = not scored, or (B_t,) = position 0) or None -
        None also for the whole list (a training step: no metric)."""
        logits_list = list(logits_list)
        T = len(self.ratios)
        if len(logits_list) != T:
            raise ValueError(f"TranslationCriterion: {len(logits_list)} logits for {T} tasks")
        dev = logits_list[0].device
        b = self._result_buffers(dev, T)
        maps = self._device_maps(dev)
        labels_list = list(labels_list) if labels_list is not None else [None] * T
        maps = [m if lab is not None else None for m, lab in zip(maps, labels_list)]       # a task without labels in this call: no metric
        if any(lab is not None and m is None for m, lab in zip(maps, labels_list)):
            raise ValueError("TranslationCriterion: labels for a task that was built without word_labels")
        loss, stats = F_egx.sequence_cross_entropy(logits_list, targets_list, self.ratios, maps, labels_list, out=b, want_pred=self.want_pred)
        b["rows"] = tuple(int(lg.shape[0]) for lg in logits_list)
        self._pred = stats["pred"]
        self._last = b
        return loss

    def stats(self) -> dict:
        """Device tensors of the most recent call (or replay): `loss`, `loss_terms` and the seven (T,) int32 counts of
        functional.sequence_cross_entropy, plus `pred` (with want_pred). Reading them does not synchronise."""
        b = self._latest()
        return {**{k: b[k] for k in ("loss",) + F_egx.SEQ_CE_STATS}, "pred": self._pred}

    def host_result(self) -> dict:
        """The results of the most recent call (or replay) as host values, from ONE device-to-host copy of `flat` (it synchronises): `loss`
        (float), `loss_terms` (T,) float32 and the seven (T,) int32 counts as numpy arrays."""
        b = self._latest()
        T = b["T"]
        host = b["flat"].cpu().numpy()
        res = {"loss": float(host[0:1].view("float32")[0]), "loss_terms": host[1:1 + T].view("float32").copy()}
        for i, name in enumerate(F_egx.SEQ_CE_STATS[1:], start=1):
            res[name] = host[1 + i * T:1 + (i + 1) * T].copy()
        return res

    def step_result(self, prefix: str = "train") -> Dict[str, float]:
        """The reference's logged values of the most recent call (or replay), from ONE device-to-host copy (it synchronises: for logging):
        f"{prefix}_loss_{name}" per task and f"{prefix}_loss" (train_loss_lam, val_loss_ac_verb, ...); f"{prefix}_{name}_token_acc" =
        token_correct / n_valid and f"{prefix}_{name}_seq_acc" = seq_correct / B_t; and for a task with word_labels
        f"{prefix}_{name}_acc" = correct / scored, f"{prefix}_{name}_err" = invalid / scored, f"{prefix}_{name}_acc_restricted" =
        correct_restricted / scored. An accuracy is nan where nothing was scored (or valid). Across ranks: all-reduce the counts first."""
        b = self._latest()
        h = self.host_result()

        def ratio(num, den):
            return float(num) / float(den) if den > 0 else float("nan")

        res: Dict[str, float] = {}
        for t, name in enumerate(self.names):
            res[f"{prefix}_loss_{name}"] = float(h["loss_terms"][t])
            res[f"{prefix}_{name}_token_acc"] = ratio(h["token_correct"][t], h["n_valid"][t])
            res[f"{prefix}_{name}_seq_acc"] = ratio(h["seq_correct"][t], b.get("rows", (0,) * len(self.names))[t])
            if self._maps[t] is not None:
                n = h["scored"][t]
                res[f"{prefix}_{name}_acc"] = ratio(h["correct"][t], n)
                res[f"{prefix}_{name}_err"] = ratio(h["invalid"][t], n)
                res[f"{prefix}_{name}_acc_restricted"] = ratio(h["correct_restricted"][t], n)
        res[f"{prefix}_loss"] = h["loss"]
        return res


class _EpochAccumulator(_DeviceCriterion):
    """What the device-resident epoch accumulators share: the host state machine (`_rows`, the count of rows that hold or are reserved for
    an entry; `_device`; `_computed`) behind reset() / update(...) per batch / compute() / step_result(). A subclass has `capacity`, the
    wording of its messages (_INPUT, _UNIT, _HOST_STATE), `_allocate(device)` with the accumulator `state` and the result words `flat`,
    `_metric(buffers)`, which runs the metric over the rows so far into the buffers, and its own slot rules in update()."""
    _INPUT, _UNIT, _HOST_STATE = "input", "rows", "the row count is"

    def __init__(self):
        super().__init__()
        self._rows = 0
        self._device: Optional[torch.device] = None
        self._computed = False

    def _refuse_capture(self, device, what: str):
        if self._capturing(device):
            raise RuntimeError(f"{type(self).__name__}.{what} cannot be captured in a graph: {self._HOST_STATE} host state (a replay would "
                               f"fold the batch into the same {self._UNIT} again); call it eagerly")

    def _forget(self):
        """reset(): whatever else a subclass keeps per epoch"""

    def reset(self):
        """Empty the accumulator (one memset on the stream) and forget the epoch's host state."""
        if self._device is not None:
            self._refuse_capture(self._device, "reset")
            self._result_buffers(self._device)["state"].zero_()
        self._rows, self._computed, self._last = 0, False, None
        self._forget()
        return self

    def _on_device(self, dev):
        if self._device is not None and dev != self._device:
            raise ValueError(f"{type(self).__name__}: {self._INPUT} on {dev}, the accumulator is on {self._device}")

    def _device_reach(self, rows: Optional[int]) -> int:
        """The rows reached after an update with device slots, which the caller has to state."""
        if rows is None:
            raise ValueError(f"{type(self).__name__}.update: device slots need rows= (the number of {self._UNIT} they reach): the host cannot "
                             "read them without a synchronisation")
        return max(self._rows, int(rows))

    def _stage(self, dev, reach: int, slot_t):
        """The capacity check of an update that reaches `reach` rows -> (the buffers, the slots on the device)."""
        if reach > self.capacity:
            raise ValueError(f"{type(self).__name__}.update: {reach} {self._UNIT} exceed capacity={self.capacity}")
        b = self._result_buffers(dev)
        return b, (slot_t.to(dev) if slot_t is not None and not slot_t.is_cuda else slot_t)

    def _commit(self, dev, reach: int):
        self._device, self._rows, self._computed = dev, reach, False

    def compute(self) -> dict:
        """-> the device tensors of the subclass's metric over the rows so far. Nothing synchronises."""
        if self._device is None or self._rows == 0:
            raise RuntimeError(f"{type(self).__name__}: no update has run yet")
        self._refuse_capture(self._device, "compute")
        b = self._result_buffers(self._device)
        self._last = {"buffers": b, "result": {k: v for k, v in self._metric(b).items() if k != "flat"}}
        self._computed = True
        return dict(self._last["result"])

    def stats(self) -> dict:
        """The device tensors of the most recent compute()."""
        return dict(self._latest()["result"])

    def _host_flat(self):
        """The result words on the host: compute() first when rows arrived since the last one, then ONE device-to-host copy."""
        if not self._computed and self._device is not None and self._rows > 0:
            self.compute()
        return self._latest()["buffers"]["flat"].cpu().numpy()


class SegmentAPValidation(_EpochAccumulator):
    """The validation epoch of the TTM and LAM tasks after the model (HHI/tasks/ttm/video_task_2loader.py:19,46-50): the reference's
    PostProcessor (HHI/utils/ttm/utils.py:46-114, HHI/utils/lam/utils.py:24-81)

        postprocess.update(outputs, targets)          # per batch: a Python list of window outputs, one .item() per segment
        postprocess.save(); mAP, acc = postprocess.get_mAP()      # two CSV files per rank, `cat` in a subshell, pandas merge + sort, two
                                                                  # Python loops over every row (HHI/utils/ttm/metrics.py:26-71, 138-199)

    as a device-resident accumulator: `reset()` at the start of the epoch, `update(logits, labels, slots)` per batch (one launch, nothing
    synchronises), `step_result()` at its end - the metric's launches (functional.segment_ap) and ONE device-to-host copy of 88 bytes.

    A row is a segment (TTM) or a frame (LAM); score = softmax(mean of the row's window logits)[1], label = the label of its first window.
    `update(logits (B, 2), labels (B,), slots)`: slots=None appends one row per input row (LAM). Otherwise `slots` names the row of every
    window, non-decreasing within the call (the windows of a segment are adjacent; a segment may continue in the next call): a host
    sequence or CPU tensor - checked here, the row count follows from it - or a device tensor together with `rows=`, the number of rows
    it reaches (the metric covers the rows below the largest such count; a slot outside [0, capacity) is dropped on the device).
    `merge=False` (LAM) refuses slots.

    The row count is host state, so update and compute cannot be captured in a graph, and more than `capacity` rows raise here. Among equal
    scores the lower row ranks first in both classes' passes (the reference's order of ties is unspecified), and rows are never
    deduplicated (the reference's uid is start:end, which merges segments of different videos with equal frame ranges). Across ranks:
    all-gather the logits, labels and slots (or the rows' sums) before update. Buffers are allocated per device on the first eager call."""

    def __init__(self, capacity: int, merge: bool = True):
        super().__init__()
        self.capacity = F_egx._seg_ap_capacity("SegmentAPValidation", capacity)
        self.merge = bool(merge)         # (_rows is the row cursor: rows 0 .. _rows - 1 hold, or are reserved for, a score)

    _INPUT, _UNIT, _HOST_STATE = "logits", "rows", "the row cursor is"

    def _allocate(self, device) -> dict:
        """The accumulator + work area, the 11 result words (`flat`) and the per-row outputs."""
        cap = self.capacity
        if device.type != "cuda":       # host stand-in (the step_result arithmetic): no accumulator
            state = torch.zeros(0, dtype=torch.uint8)
        else:
            state = F_egx.segment_ap_state(cap, device)
        flat = torch.zeros(len(F_egx.SEG_AP_COUNTS) + len(F_egx.SEG_AP_VALUES), dtype=torch.int64, device=device)
        return {"state": state, "flat": flat, **F_egx.segment_ap_views(flat),
                "score": torch.zeros(cap, dtype=torch.float32, device=device),
                "order1": torch.zeros(cap, dtype=torch.int32, device=device),
                "order0": torch.zeros(cap, dtype=torch.int32, device=device)}

    def update(self, logits: torch.Tensor, labels: torch.Tensor, slots=None, rows: Optional[int] = None) -> None:
        dev = logits.device
        self._refuse_capture(dev, "update")
        B = int(logits.shape[0])
        if slots is not None and not self.merge:
            raise ValueError("SegmentAPValidation(merge=False): every input row is its own row, slots are not taken")
        self._on_device(dev)
        if slots is None:
            reach = self._rows + B
            slot_t, slot0 = None, self._rows
        elif isinstance(slots, torch.Tensor) and slots.is_cuda:
            reach, slot_t, slot0 = self._device_reach(rows), slots, 0
        else:
            host = torch.as_tensor(slots, dtype=torch.int64).reshape(-1)
            if host.numel() != B:
                raise ValueError(f"SegmentAPValidation.update: {host.numel()} slots for {B} windows")
            if B and (int(host[0]) < 0 or bool((host[1:] < host[:-1]).any())):
                raise ValueError("SegmentAPValidation.update: slots must be >= 0 and non-decreasing within a call")
            reach, slot0 = max(self._rows, int(host[-1]) + 1 if B else 0), 0
            slot_t = host
        b, slot_t = self._stage(dev, reach, slot_t)
        F_egx.segment_scores_update(b["state"], self.capacity, logits, labels.to(device=dev, dtype=torch.int64), slot_t, slot0)
        self._commit(dev, reach)

    def _metric(self, b: dict) -> dict:
        """compute(): `score`, `order1`, `order0` (n), the int64 counts `n`, `n_pos`, `TP`, `FN`, `FP`, `TN`, `n_nonfinite` and fp64 `AP0`,
        `AP1`, `mAP`, `acc`."""
        return F_egx.segment_ap(b["state"], self.capacity, self._rows, out=b)

    def step_result(self, prefix: str = "val") -> Dict[str, float]:
        """The epoch's logged values from ONE device-to-host copy (it synchronises): f"{prefix}_mAP" (the checkpoint metric),
        f"{prefix}_acc", f"{prefix}_AP0", f"{prefix}_AP1" and the counts f"{prefix}_TP", _FN, _FP, _TN, _n, _n_pos, _n_nonfinite.
        Runs compute() first when rows arrived since the last one."""
        host = self._host_flat()
        nc = len(F_egx.SEG_AP_COUNTS)
        res: Dict[str, float] = {f"{prefix}_{name}": int(host[i]) for i, name in enumerate(F_egx.SEG_AP_COUNTS)}
        values = host[nc:].view("float64")
        res.update({f"{prefix}_{name}": float(values[i]) for i, name in enumerate(F_egx.SEG_AP_VALUES)})
        return res


class ViewEnsembleTest(_EpochAccumulator):
    """The test epoch of the action-recognition translators after the model: MultiTaskClassificationTask.test_step / test_epoch_end
    (HOI/tasks/lta/long_term_anticipation.py:86-158; the same code in long_term_anticipation_taskspecfic.py:88-162), the number the
    EgoT2-s AR models are reported with. Every video is seen as TEST.NUM_ENSEMBLE_VIEWS x TEST.NUM_SPATIAL_CROPS clips; the reference

        torch.cat's every clip's logits of the epoch, walks the clips in a Python loop with three dicts of per-video tensors (one `+=` or
        torch.max launch per clip and head), stacks the dict values and calls topk_errors four times, each read with .item()

    Here: `reset()` at the start of the epoch, `update(preds, labels, clip_ids)` per batch (one launch, nothing synchronises),
    `step_result()` at its end - one launch (functional.view_ensemble_topk) and ONE device-to-host copy of 3 + H + len(ks) * H words.

    `ViewEnsembleTest(capacity, classes, method, ks)`: at most `capacity` videos; `classes` = cfg.MODEL.NUM_CLASSES; `method` =
    cfg.DATA.ENSEMBLE_METHOD. "sum" adds a video's clips in fp32 in ARRIVAL order from 0 - the reference's operations in its order, so the
    rows have its bits; "max" keeps the running maximum, which starts from 0 as the reference's torch.zeros makes it: a video whose
    logits are all negative ends as a row of zeros (kept as it is, not "fixed"). A video's label is its last clip's.
    `update(preds, labels, clip_ids=...)`: preds = the [(B, C_verb), (B, C_noun)] list `forward_features` returns, labels int64 (B, H),
    clip_ids a host sequence of hashables (the loader's clip_id strings), mapped to dense slots in first-appearance order - the order of
    the reference's dicts, so row i of every output is the reference's i-th video. `slots=` (instead of clip_ids) takes a host sequence /
    CPU tensor of slots, or a device tensor together with `rows=`, the number of videos it reaches (a slot outside [0, capacity) is
    dropped on the device and counted in n_dropped). The views of a video need not be adjacent and may be spread over batches.

    The id map and the video count are host state, so update, compute and reset cannot be captured in a graph, and more than `capacity`
    videos raise here. Ties go to the lower class (torch.topk: unspecified); a video whose label is outside [0, C_h) is never correct and
    is counted in n_invalid; errors divide by the number of videos, as topk_errors divides by preds.size(0). Across ranks: gather
    predictions, labels and ids before update - what the reference does (du.all_gather, :104-107). Buffers are allocated per device on the
    first eager call."""

    HEAD_NAMES = ("verb", "noun")

    def __init__(self, capacity: int, classes, method: str = "sum", ks=(1, 5)):
        super().__init__()
        self.classes = F_egx._view_ens_classes("ViewEnsembleTest", classes)
        self.capacity = int(capacity)
        if not 1 <= self.capacity or self.capacity * sum(self.classes) > 1 << 31:
            raise ValueError(f"ViewEnsembleTest: capacity={capacity} (needs capacity >= 1 and capacity * sum(classes) <= 2^31)")
        if method not in F_egx.VIEW_ENS_METHODS:
            raise ValueError(f"ViewEnsembleTest: method={method!r} (needs 'sum' or 'max', cfg.DATA.ENSEMBLE_METHOD)")
        self.method = method
        self.ks = tuple(int(k) for k in ks)
        if not 1 <= len(self.ks) <= F_egx.SEG_CE_MAX_KS or min(self.ks) < 1 or max(self.ks) > min(self.classes):
            raise ValueError(f"ViewEnsembleTest: ks={ks} (needs 1 to {F_egx.SEG_CE_MAX_KS} values in 1 .. {min(self.classes)}, the narrowest head)")
        # clip id -> slot, in first-appearance order (the reference's dict order); videos 0 .. _rows - 1 hold (or are reserved for) a row
        self._slot_of: Dict[object, int] = {}

    _INPUT, _UNIT, _HOST_STATE = "predictions", "videos", "the id map and the video count are"

    def _allocate(self, device) -> dict:
        """The accumulator, the result words (`flat`) and the per-video outputs."""
        cap, H = self.capacity, len(self.classes)
        if device.type != "cuda":       # host stand-in (the step_result arithmetic): no accumulator
            state = torch.zeros(0, dtype=torch.uint8)
        else:
            state = F_egx.view_ensemble_state(cap, self.classes, device)
        flat = torch.zeros(len(F_egx.VIEW_ENS_COUNTS) + H + len(self.ks) * H, dtype=torch.int32, device=device)
        return {"state": state, "flat": flat, **F_egx.view_ensemble_views(flat, H, len(self.ks)),
                "rank": torch.zeros((cap, H), dtype=torch.int32, device=device),
                "pred": torch.zeros((cap, H), dtype=torch.int32, device=device)}

    def _forget(self):
        self._slot_of = {}

    def _slots_of_ids(self, clip_ids) -> Tuple[List[int], Dict[object, int]]:
        """-> (the slot of every id, the id map grown by the new ids); nothing of self changes (the caller commits after its checks)."""
        grown = dict(self._slot_of)
        base = self._rows
        if base != len(grown):
            raise ValueError("ViewEnsembleTest.update: clip_ids and slots cannot be mixed within an epoch")
        return [grown.setdefault(cid, len(grown)) for cid in clip_ids], grown

    def update(self, preds, labels: torch.Tensor, clip_ids=None, slots=None, rows: Optional[int] = None) -> None:
        preds = [preds] if isinstance(preds, torch.Tensor) else list(preds)
        dev = preds[0].device
        self._refuse_capture(dev, "update")
        B = int(preds[0].shape[0])
        if (clip_ids is None) == (slots is None):
            raise ValueError("ViewEnsembleTest.update takes exactly one of clip_ids and slots")
        self._on_device(dev)
        grown = self._slot_of
        if clip_ids is not None:
            host, grown = self._slots_of_ids(list(clip_ids))
            host = torch.tensor(host, dtype=torch.int32)
            reach, slot_t = len(grown), host
        elif isinstance(slots, torch.Tensor) and slots.is_cuda:
            reach, slot_t = self._device_reach(rows), slots
        else:
            if self._slot_of:
                raise ValueError("ViewEnsembleTest.update: clip_ids and slots cannot be mixed within an epoch")
            host = torch.as_tensor(slots, dtype=torch.int64).reshape(-1)
            if B and int(host.min()) < 0:
                raise ValueError("ViewEnsembleTest.update: host slots must be >= 0")
            reach, slot_t = max(self._rows, int(host.max()) + 1 if host.numel() else 0), host
        if slot_t.numel() != B:
            raise ValueError(f"ViewEnsembleTest.update: {slot_t.numel()} ids / slots for {B} clips")
        b, slot_t = self._stage(dev, reach, slot_t)
        F_egx.view_ensemble_update(b["state"], self.capacity, self.classes, preds, labels.to(device=dev, dtype=torch.int64), slot_t,
                                   method=self.method)
        self._slot_of = grown
        self._commit(dev, reach)

    def _metric(self, b: dict) -> dict:
        """compute(): `rank`, `pred` (n, H) int32 and the int32 counts `n`, `n_dropped`, `n_nonfinite`, `n_invalid` (H,), `correct`
        (len(ks), H)."""
        return F_egx.view_ensemble_topk(b["state"], self.capacity, self.classes, self._rows, self.ks, out=b)

    def video_ids(self) -> list:
        """The clip ids in row order (first appearance); with slots= the rows are the caller's slots and this is range(n)."""
        return list(self._slot_of) if self._slot_of else list(range(self._rows))

    def predictions(self):
        """-> (pred (n, H), rank (n, H), video ids in row order) of the most recent compute(), for a submission file. Device tensors."""
        r = self._latest()["result"]
        return r["pred"], r["rank"], self.video_ids()

    def head_names(self) -> Tuple[str, ...]:
        return self.HEAD_NAMES if len(self.classes) == 2 else tuple(str(h) for h in range(len(self.classes)))

    def step_result(self, prefix: str = "test") -> Dict[str, float]:
        """The epoch's logged values from ONE device-to-host copy (it synchronises): f"{prefix}_top{k}_{head}_err" for every k of `ks` and
        head (verb / noun with two heads: the reference's top1_verb_err, top5_verb_err, top1_noun_err, top5_noun_err; the head's index
        otherwise) = (1 - correct / n) * 100 in fp32, as the reference's fp32 tensors compute it, with n = the number of videos; and the
        counts f"{prefix}_n", _n_dropped, _n_nonfinite, f"{prefix}_n_invalid_{head}", f"{prefix}_correct{k}_{head}". Runs compute() first
        when clips arrived since the last one. prefix="" gives the reference's bare keys."""
        host = self._host_flat()
        import numpy as np
        H, nc = len(self.classes), len(F_egx.VIEW_ENS_COUNTS)
        pre = f"{prefix}_" if prefix else ""
        res: Dict[str, float] = {f"{pre}{name}": int(host[i]) for i, name in enumerate(F_egx.VIEW_ENS_COUNTS)}
        n = np.float32(host[0])
        invalid, correct = host[nc:nc + H], host[nc + H:].reshape(len(self.ks), H)
        for h, name in enumerate(self.head_names()):
            res[f"{pre}n_invalid_{name}"] = int(invalid[h])
            for ki, k in enumerate(self.ks):
                res[f"{pre}correct{k}_{name}"] = int(correct[ki, h])
                err = (np.float32(1.0) - np.float32(correct[ki, h]) / n) * np.float32(100.0) if host[0] > 0 else np.float32("nan")
                res[f"{pre}top{k}_{name}_err"] = float(err)
        return res


class LRSchedule:
    """Per-step learning-rate factor f(k), k = 0, 1, ... the 0-based index of the update (k = t - 1 for the optimizer's 1-based step count t):
    the closed forms of the reference's per-step schedulers (HOI/optimizers/lta/lr_scheduler.py:11-41 lr_factory, "interval": "step"),
    evaluated on the device by egx_lr_update from the optimizer's device-resident step count, so that a captured step (GraphedStep)
    replays the schedule instead of the learning rate it was captured with. `factor(k)` is the same closed form on the host in fp64.

        constant()                                   1                                            lr_policy "constant"
        cosine_annealing(T_max)                      0.5 (1 + cos(pi k / T_max))                  "cosine" (CosineAnnealingLR, eta_min 0; periodic)
        warmup_cosine(warmup_steps, t_total, cycles) WarmupCosineSchedule.lr_lambda               "cosine_warmup" (rises again beyond t_total)
        warmup_linear(warmup_steps, t_total)         WarmupLinearSchedule.lr_lambda               "linear_warmup"
        from_factors(seq) / from_lambda(fn, n_steps) seq[min(k, n - 1)]                           any LambdaLR (the get_epoch_lr policies)
    """
    KINDS = ("constant", "cosine_annealing", "warmup_cosine", "warmup_linear", "table")

    def __init__(self, kind: str, warmup_steps: int = 0, t_total: int = 0, T_max: int = 1, cycles: float = 0.5, factors=None):
        if kind not in self.KINDS:
            raise ValueError(f"LRSchedule: kind {kind!r} is not one of {self.KINDS}")
        self.kind, self.warmup_steps, self.t_total, self.T_max, self.cycles = kind, int(warmup_steps), int(t_total), int(T_max), float(cycles)
        self.factors = None if factors is None else [float(x) for x in factors]
        if kind == "cosine_annealing" and self.T_max < 1:
            raise ValueError(f"LRSchedule: T_max={self.T_max} (needs T_max >= 1)")
        if kind in ("warmup_cosine", "warmup_linear") and (self.warmup_steps < 0 or self.t_total < 0):
            raise ValueError(f"LRSchedule: warmup_steps={self.warmup_steps}, t_total={self.t_total} (both need to be >= 0)")
        if kind == "table" and not self.factors:
            raise ValueError("LRSchedule: a table needs at least one factor")
        self._table_dev: Dict[torch.device, torch.Tensor] = {}

    @classmethod
    def constant(cls):
        return cls("constant")

    @classmethod
    def cosine_annealing(cls, T_max: int):
        return cls("cosine_annealing", T_max=T_max)

    @classmethod
    def warmup_cosine(cls, warmup_steps: int, t_total: int, cycles: float = 0.5):
        return cls("warmup_cosine", warmup_steps=warmup_steps, t_total=t_total, cycles=cycles)

    @classmethod
    def warmup_linear(cls, warmup_steps: int, t_total: int):
        return cls("warmup_linear", warmup_steps=warmup_steps, t_total=t_total)

    @classmethod
    def from_factors(cls, factors):
        return cls("table", factors=factors)

    @classmethod
    def from_lambda(cls, fn, n_steps: int):
        """The table fn(0), ..., fn(n_steps - 1) of a LambdaLR's function; steps beyond it keep the last factor."""
        return cls("table", factors=[fn(k) for k in range(int(n_steps))])

    def factor(self, k: int) -> float:
        k = max(int(k), 0)
        if self.kind == "constant":
            return 1.0
        if self.kind == "cosine_annealing":
            return 0.5 * (1.0 + math.cos(math.pi * k / self.T_max))
        if self.kind == "table":
            return self.factors[min(k, len(self.factors) - 1)]
        if k < self.warmup_steps:
            return float(k) / float(max(1, self.warmup_steps))
        span = float(max(1, self.t_total - self.warmup_steps))
        if self.kind == "warmup_linear":
            return max(0.0, float(self.t_total - k) / span)
        progress = float(k - self.warmup_steps) / span
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * self.cycles * 2.0 * progress)))

    def lr_at(self, k: int, base_lr: float) -> float:
        """Learning rate of update k (fp64; the device holds it rounded to fp32)."""
        return base_lr * self.factor(k)

    def _struct(self, device) -> "_lib.LrSchedule":
        """The C ABI's view; a table's device copy is made on first use (eagerly, before any capture: GraphedStep's warm-up steps do it)."""
        s = _lib.LrSchedule(self.KINDS.index(self.kind), self.warmup_steps, self.t_total, self.T_max, self.cycles, None, 0)
        if self.kind == "table":
            device = torch.device(device)
            t = self._table_dev.get(device)
            if t is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("LRSchedule: the table's device copy cannot be made inside a capture; run one eager step first")
                t = self._table_dev[device] = torch.tensor(self.factors, dtype=torch.float64, device=device)
            s.factors, s.n = t.data_ptr(), t.numel()
        return s


class GradGuard:
    """Gradient-norm clipping and the non-finite guard of an optimizer step, decided on the device so that a captured step (GraphedStep)
    replays the decision: what Lightning's Trainer offers as gradient_clip_val / track_grad_norm (the reference leaves both at their defaults,
    HHI/scripts/run_ttm.py:21, HOI/scripts/lta/run_lta.py:238). Hand it to FusedAdam / FusedSGD / construct_solver as `guard=`. Every step then
    measures the fp64 norm of ALL its gradient buffers in a fixed summation order (egx_grad_norm: two launches, one read of the gradients),

        coef  = clip_grad_norm_'s max_norm / (norm + 1e-6) where that is below 1, else 1 (1 with max_norm=None: measure and guard only)
        apply = every gradient element is finite, or not skip_nonfinite

    and the step-count / learning-rate bump and the updates obey it: a skipped step changes nothing the optimizer owns (parameters, moments,
    momentum buffers, the step count, the scheduled learning rates - the schedule index is the number of APPLIED updates), an applied one is
    today's update with the gradients scaled by coef, bit for bit the unguarded step while coef == 1. A gradient of 3e38 is finite: its norm
    is held in fp64 and the step is clipped, not skipped.

    `max_norm` and `skip_nonfinite` are read when a step is enqueued and are therefore baked into a capture, as the base learning rate is: a
    changed value needs a new capture. The guard owns a per-device scratch and a 40-byte guard block; the first EAGER step creates them
    (GraphedStep's warm-up steps do), a capture refuses to. `block` holds the device tensors for sync-free use, `result()` copies them to the
    host. The counters (`steps`, `skipped`, `clipped`) count since construction or reset_counters(); they are not part of any state_dict."""

    def __init__(self, max_norm: Optional[float] = None, skip_nonfinite: bool = True):
        if max_norm is not None:
            if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)):
                raise TypeError(f"GradGuard: max_norm must be a number or None, got {type(max_norm).__name__}")
            if not max_norm >= 0:                       # refuses a NaN too
                raise ValueError(f"GradGuard: max_norm={max_norm} (needs max_norm >= 0)")
        if not isinstance(skip_nonfinite, bool):
            raise TypeError(f"GradGuard: skip_nonfinite must be a bool, got {type(skip_nonfinite).__name__}")
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = skip_nonfinite
        self._bufs: Dict[tuple, dict] = {}
        self._last: Optional[dict] = None

    def _buffers(self, device, scratch_bytes: int) -> dict:
        device = torch.device(device)
        key = (device.type, device.index)
        b = self._bufs.get(key)
        if b is None or b["scratch"].numel() < scratch_bytes:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                # a buffer created inside a capture would live in that graph's private pool
                raise RuntimeError("GradGuard: run one eager step with these gradient buffers before capturing it in a graph")
            if b is None:
                words = torch.zeros(5, dtype=torch.int64, device=device)      # egx_guard_block: fp64 | fp32, int32 | 3 x int64
                b = self._bufs[key] = {"words": words, "grad_norm": words[0:1].view(torch.float64)[0],
                                       "clip_coef": words[1:2].view(torch.float32)[0], "applied": words[1:2].view(torch.int32)[1],
                                       "steps": words[2], "skipped": words[3], "clipped": words[4]}
            b["scratch"] = torch.empty(scratch_bytes, dtype=torch.uint8, device=device)
        return b

    def measure(self, buffers, stream=None) -> dict:
        """Enqueue the norm and the decision over `buffers` (flat contiguous fp32 device tensors; an empty one is legal) -> `block`."""
        lib = _lib.load()
        buffers = list(buffers)
        if not buffers:
            raise ValueError("GradGuard: no gradient buffers")
        for t in buffers:
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError("GradGuard needs contiguous fp32 gradients on the GPU")
        n = len(buffers)
        ns = (C.c_size_t * n)(*[t.numel() for t in buffers])
        ptrs = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in buffers])
        need = lib.egx_grad_norm_scratch_bytes(ns, n)
        b = self._buffers(buffers[0].device, need)
        cfg = _lib.GradNormCfg(0.0 if self.max_norm is None else self.max_norm, int(self.max_norm is not None), int(self.skip_nonfinite))
        if stream is None:
            stream = torch.cuda.current_stream(buffers[0].device).cuda_stream
        check(lib.egx_grad_norm(ptrs, ns, n, ptr(b["scratch"]), b["scratch"].numel(), C.byref(cfg), ptr(b["words"]), stream))
        self._last = b
        return b

    @property
    def block(self) -> dict:
        """The device tensors of the guard block the last step wrote: `grad_norm` (fp64), `clip_coef` (fp32), `applied` (int32) and the int64
        counters `steps`, `skipped`, `clipped`; every call or replay refreshes them. Reading them does not synchronise."""
        if self._last is None:
            raise RuntimeError("GradGuard: no step has run yet")
        return {k: v for k, v in self._last.items() if k not in ("words", "scratch")}

    def result(self) -> dict:
        """The guard block on the host (one 40-byte copy; it synchronises: for logging). Before the first step: zeros."""
        if self._last is None:
            return {"grad_norm": 0.0, "clip_coef": 1.0, "applied": 1, "steps": 0, "skipped": 0, "clipped": 0}
        w = self._last["words"].cpu()
        return {"grad_norm": float(w[0:1].view(torch.float64)[0]), "clip_coef": float(w[1:2].view(torch.float32)[0]),
                "applied": int(w[1:2].view(torch.int32)[1]), "steps": int(w[2]), "skipped": int(w[3]), "clipped": int(w[4])}

    def reset_counters(self) -> "GradGuard":
        for b in self._bufs.values():
            b["words"][2:].zero_()
        return self


def grad_norm(params) -> torch.Tensor:
    """-> the 2-norm of every `.grad` of `params` as a device fp64 scalar, without a host synchronisation (Lightning's track_grad_norm=2):
    GradGuard's norm - fp64 sums in a fixed order over the flat buffers the gradients are views of - without an optimizer. Parameters whose
    `.grad` is None do not count, as for torch.nn.utils.clip_grad_norm_. Eager use (it allocates its result)."""
    if isinstance(params, torch.Tensor):
        params = [params]
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        raise ValueError("grad_norm: no parameter has a gradient")
    return GradGuard().measure(_grad_buffers(grads))["grad_norm"].clone()


def _grad_buffers(grads) -> List[torch.Tensor]:
    """The distinct flat buffers a list of gradients lives in, each as ONE whole-storage view (the buffers _FlatOptimizer.step updates: all the
    views _GradPacker carved out of a storage count once, through it; a stand-alone gradient is its own storage)."""
    out, seen = [], set()
    for g in grads:
        if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
            raise ValueError("grad_norm needs contiguous fp32 gradients on the GPU")
        key = g.untyped_storage().data_ptr()
        if key in seen:
            continue
        seen.add(key)
        out.append(F_egx.flat_storage_view(g).reshape(-1))
    return out


class _Bucket:
    __slots__ = ("sig", "param", "exp_avg", "exp_avg_sq", "momentum_buffer", "keys", "numel", "members")


class _FlatOptimizer(torch.optim.Optimizer):
    """What FusedAdam and FusedSGD share: gradients grouped by the flat buffer they are views of, the parameters re-pointed into a flat buffer
    of the same layout (one launch per buffer), per-parameter state as views of per-bucket buffers, the step count in device memory, and -
    with a `schedule` - the learning rates of the parameter groups in device memory, advanced by the same launch that bumps the count.
    A subclass names its state buffers (_state_keys) and enqueues its update (_update)."""

    def __init__(self, params, defaults, schedule: Optional[LRSchedule], guard: Optional[GradGuard] = None):
        super().__init__(params, defaults)
        if schedule is not None and len(self.param_groups) > _lib.EGX_LR_MAX_GROUPS:
            raise ValueError(f"{type(self).__name__}: a schedule serves at most {_lib.EGX_LR_MAX_GROUPS} parameter groups, got {len(self.param_groups)}")
        if guard is not None and not isinstance(guard, GradGuard):
            raise TypeError(f"{type(self).__name__}: guard must be a train.GradGuard or None, got {type(guard).__name__}")
        self.schedule = schedule
        self.guard = guard
        self._buckets: Dict[tuple, _Bucket] = {}
        self._step_dev: Optional[torch.Tensor] = None
        self._lr_dev: Optional[torch.Tensor] = None
        self._resume_step = 0          # step count restored by load_state_dict before the device counter exists

    def _state_keys(self, group) -> Tuple[str, ...]:
        raise NotImplementedError

    def _update(self, lib, b: _Bucket, gflat: torch.Tensor, group, lr_dev: Optional[int], stream):
        raise NotImplementedError

    def _update_guarded(self, lib, b: _Bucket, gflat: torch.Tensor, group, lr_dev: Optional[int], guard: int, stream):
        raise NotImplementedError

    def guard_result(self) -> dict:
        """The last step's `grad_norm`, `clip_coef`, `applied` and the counters `steps`, `skipped`, `clipped` of the optimizer's GradGuard, on
        the host. It synchronises: for logging (optimizer.guard.block holds the device tensors)."""
        if self.guard is None:
            raise RuntimeError(f"{type(self).__name__}: constructed without a guard (guard=GradGuard(...))")
        return self.guard.result()

    def _make_bucket(self, sig, base: torch.Tensor, members, keys) -> _Bucket:
        b = _Bucket()
        b.sig = sig
        b.numel = base.numel()
        if len(members) == 1 and members[0][1] == 0 and members[0][0].numel() == base.numel() and members[0][0].is_contiguous():
            b.param = members[0][0].data.view(-1)          # stand-alone tensor: update it in place where it lives
        else:
            b.param = torch.zeros_like(base)
            for p, off in members:                          # move the parameters behind the gradient layout
                n = p.numel()
                b.param[off:off + n].copy_(p.data.reshape(-1))
                p.data = b.param[off:off + n].view(p.shape)
        b.keys = tuple(keys)
        for key in b.keys:
            setattr(b, key, torch.zeros_like(b.param))
        b.members = list(members)
        self._adopt_state(b)
        return b

    def _adopt_state(self, b: _Bucket):
        """Make self.state[p] views of the bucket's state buffers. Values that are already there (restored by
        load_state_dict, or carried over from a bucket that had to be rebuilt) are copied in first, so a resumed run
        continues from the saved buffers instead of restarting them from zero."""
        for p, off in b.members:
            n = p.numel()
            old = self.state.get(p)
            for key in b.keys:
                view = getattr(b, key)[off:off + n]
                if old is not None and torch.is_tensor(old.get(key)) and old[key].numel() == n \
                        and old[key].data_ptr() != view.data_ptr():
                    view.copy_(old[key].reshape(-1).to(view.device, view.dtype))
            st = {"step": self._step_dev}
            for key in b.keys:
                st[key] = getattr(b, key)[off:off + n].view(p.shape)
            self.state[p] = st

    def _loaded_step(self) -> int:
        steps = [st["step"] for st in self.state.values() if st.get("step") is not None]
        return max((int(s.item()) if torch.is_tensor(s) else int(s)) for s in steps) if steps else 0

    def load_state_dict(self, state_dict):
        """torch's Optimizer.load_state_dict replaces self.state with fresh copies; the real buffers and the step count
        live in the bucket buffers / the device counter, so push the loaded values back into them (buckets that do not
        exist yet pick them up in _make_bucket). Mirrors the optimizer resume of the reference's Lightning trainer
        (`trainer.fit(ckpt_path=...)`, HOI/scripts/pnr/train.py:57)."""
        super().load_state_dict(state_dict)
        step = self._loaded_step()
        self._resume_step = step
        if self._step_dev is not None:
            self._step_dev.fill_(step)
        for b in self._buckets.values():
            for p, off in b.members:        # a parameter WITHOUT loaded state starts from zero buffers again (a state_dict taken before the first step)
                if p not in self.state:
                    for key in b.keys:
                        getattr(b, key)[off:off + p.numel()].zero_()
            self._adopt_state(b)

    def current_lr(self) -> List[float]:
        """The learning rate of every parameter group as the last enqueued step used it. With a schedule this reads the device values
        (it synchronises: for logging, not for the loop); without one it is param_groups[g]["lr"]."""
        if self.schedule is None or self._lr_dev is None:
            return [float(g["lr"]) for g in self.param_groups]
        return self._lr_dev[:len(self.param_groups)].tolist()

    def _bump(self, lib, device, stream, guard: Optional[int] = None):
        """Advance the device step count once per step(); with a schedule the same launch writes every group's learning rate. `guard` (the
        device address of a guard block): the gated twins, which leave both alone when the step is skipped."""
        if self._step_dev is None:
            self._step_dev = torch.full((), self._resume_step, dtype=torch.int64, device=device)
        if self.schedule is None:
            if guard is None:
                check(lib.egx_counter_add(ptr(self._step_dev), 1, stream))
            else:
                check(lib.egx_counter_add_gated(ptr(self._step_dev), 1, guard, stream))
            return
        if self._lr_dev is None:
            self._lr_dev = torch.zeros(_lib.EGX_LR_MAX_GROUPS, dtype=torch.float32, device=device)
        n = len(self.param_groups)
        base = (C.c_double * n)(*[float(g["lr"]) for g in self.param_groups])     # read here: baked into a capture
        sched = self.schedule._struct(device)
        if guard is None:
            check(lib.egx_lr_update(C.byref(sched), ptr(self._step_dev), base, n, ptr(self._lr_dev), stream))
        else:
            check(lib.egx_lr_update_gated(C.byref(sched), ptr(self._step_dev), base, n, ptr(self._lr_dev), guard, stream))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        if self.guard is not None:
            self._step_guarded(lib, stream)
            return loss
        bumped = False
        for gi, group in enumerate(self.param_groups):
            for base, members in self._by_base(group).values():
                if not bumped:
                    self._bump(lib, base.device, stream)
                    bumped = True
                b = self._bucket(gi, group, base, members)
                gflat = base.reshape(-1)
                F_egx.note_weights_changed()       # (raw-pointer update: no version counter moves; packed-weight caches re-pack)
                lr_dev = None if self.schedule is None else self._lr_dev.data_ptr() + 4 * gi
                self._update(lib, b, gflat, group, lr_dev, stream)
        return loss

    def _by_base(self, group) -> Dict[int, Tuple[torch.Tensor, List]]:
        """The group's gradients by the flat buffer they are views of: storage address -> (whole-storage view, [(parameter, offset)])."""
        by_base: Dict[int, Tuple[torch.Tensor, List]] = {}
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
                raise ValueError(f"{type(self).__name__} needs contiguous fp32 gradients on the GPU")
            key = g.untyped_storage().data_ptr()        # the flat buffer this gradient was carved out of: one view per buffer,
            ent = by_base.get(key)                       # not one per parameter (25 tensor constructions per step on the TTM translator)
            if ent is None:
                ent = by_base[key] = (F_egx.flat_storage_view(g), [])
            ent[1].append((p, g.storage_offset()))
        return by_base

    def _bucket(self, gi: int, group, base: torch.Tensor, members) -> _Bucket:
        sig = (gi,) + tuple((id(p), off) for p, off in members) + (base.numel(),)
        b = self._buckets.get(sig)
        if b is not None and any(p.data_ptr() != b.param.data_ptr() + 4 * off for p, off in members):
            b = None                                 # somebody re-allocated a parameter: rebuild the bucket
        if b is None:
            b = self._buckets[sig] = self._make_bucket(sig, base.reshape(-1), members, self._state_keys(group))
        return b

    def _step_guarded(self, lib, stream):
        """step() behind self.guard: every group's buffers are collected first, then the norm over all of them (a buffer two groups share
        counts once), then the gated bump, then the guarded updates."""
        work = [(gi, group, base, members) for gi, group in enumerate(self.param_groups) for base, members in self._by_base(group).values()]
        if not work:
            return
        flats, seen = [], set()
        for _, _, base, _ in work:
            if base.data_ptr() not in seen:
                seen.add(base.data_ptr())
                flats.append(base.reshape(-1))
        guard = self.guard.measure(flats, stream)["words"].data_ptr()
        self._bump(lib, work[0][2].device, stream, guard)
        for gi, group, base, members in work:
            b = self._bucket(gi, group, base, members)
            F_egx.note_weights_changed()
            lr_dev = None if self.schedule is None else self._lr_dev.data_ptr() + 4 * gi
            self._update_guarded(lib, b, base.reshape(-1), group, lr_dev, guard, stream)


class FusedAdam(_FlatOptimizer):
    """Adam (adamw=False) / AdamW (adamw=True) with torch.optim semantics, one launch per flat gradient buffer.

    `schedule` (an LRSchedule): the learning rate of update k is param_groups[g]["lr"] * schedule.factor(k), computed on the device from the
    step count, so a captured step replays the schedule. param_groups[g]["lr"] stays the BASE learning rate; it is read when the step is
    enqueued and is therefore baked into a capture: a changed base needs a new capture. Without a schedule nothing changes: the learning
    rate goes to egx_adam_step by value.

    `guard` (a GradGuard): clip the gradients to guard.max_norm and skip a step with a non-finite gradient, decided on the device per step or
    replay; guard_result() / guard.block report it. Without one the step enqueues exactly what it did before."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, adamw: bool = False, schedule: Optional[LRSchedule] = None, guard: Optional[GradGuard] = None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, adamw=adamw), schedule, guard)

    def _state_keys(self, group):
        return ("exp_avg", "exp_avg_sq")

    def _update(self, lib, b, gflat, group, lr_dev, stream):
        if lr_dev is None:
            check(lib.egx_adam_step(ptr(b.param), ptr(gflat), ptr(b.exp_avg), ptr(b.exp_avg_sq), b.numel,
                                    ptr(self._step_dev), group["lr"], group["betas"][0], group["betas"][1],
                                    group["eps"], group["weight_decay"], int(group["adamw"]), 1.0, stream))
        else:
            check(lib.egx_adam_step_dev_lr(ptr(b.param), ptr(gflat), ptr(b.exp_avg), ptr(b.exp_avg_sq), b.numel,
                                           ptr(self._step_dev), lr_dev, group["betas"][0], group["betas"][1],
                                           group["eps"], group["weight_decay"], int(group["adamw"]), 1.0, stream))

    def _update_guarded(self, lib, b, gflat, group, lr_dev, guard, stream):
        check(lib.egx_adam_step_guarded(ptr(b.param), ptr(gflat), ptr(b.exp_avg), ptr(b.exp_avg_sq), b.numel, ptr(self._step_dev), lr_dev,
                                        group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"],
                                        int(group["adamw"]), guard, stream))


class FusedSGD(_FlatOptimizer):
    """torch.optim.SGD (momentum, dampening, weight decay, Nesterov) with one launch per flat gradient buffer: the optimizer the reference's
    construct_optimizer builds for OPTIMIZING_METHOD "sgd" (HOI/optimizers/lta/optimizer.py:54-62; HOI/configs/recognition/ts_ar.yaml:39-45).

    state[p] holds `momentum_buffer` (a view of the bucket's buffer; absent with momentum 0) and `step` (the device step count). The first
    update ASSIGNS momentum_buffer = g, decided on the device by step == 1, as torch does on a missing buffer; with a zeroed buffer and
    dampening 0 that equals the recurrence bit for bit. `schedule`, `guard` and param_groups[g]["lr"]: as for FusedAdam (a skipped first step
    leaves the count at 0, so the first APPLIED update assigns the buffer).

    load_state_dict accepts this class's state dicts and torch.optim.SGD's. A torch state dict has momentum buffers and no step count: the
    count then starts at 1, so the first-update rule does not fire and the loaded buffers are continued (and a schedule continues at k = 1:
    torch keeps its position in the scheduler's own state dict, not here)."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, schedule: Optional[LRSchedule] = None, guard: Optional[GradGuard] = None):
        if lr < 0 or momentum < 0 or weight_decay < 0 or not (0 <= dampening <= 1):
            raise ValueError("invalid SGD hyper-parameters")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov), schedule, guard)

    def _state_keys(self, group):
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    def _loaded_step(self) -> int:
        step = super()._loaded_step()
        if step == 0 and any(torch.is_tensor(st.get("momentum_buffer")) and st.get("step") is None for st in self.state.values()):
            return 1            # torch.optim.SGD's state: buffers without a count
        return step

    def _update(self, lib, b, gflat, group, lr_dev, stream):
        buf = b.momentum_buffer if b.keys else None
        check(lib.egx_sgd_step(ptr(b.param), ptr(gflat), ptr(buf), b.numel, ptr(self._step_dev), lr_dev, group["lr"], group["momentum"],
                               group["dampening"], group["weight_decay"], int(group["nesterov"]), 1.0, stream))

    def _update_guarded(self, lib, b, gflat, group, lr_dev, guard, stream):
        buf = b.momentum_buffer if b.keys else None
        check(lib.egx_sgd_step_guarded(ptr(b.param), ptr(gflat), ptr(buf), b.numel, ptr(self._step_dev), lr_dev, group["lr"],
                                       group["momentum"], group["dampening"], group["weight_decay"], int(group["nesterov"]), guard, stream))


SOLVER_POLICIES = ("cosine", "constant", "cosine_warmup", "linear_warmup")


def construct_solver(model, cfg, steps_in_epoch: int, lr_policy: Optional[str] = None, lr_lambda=None, guard: Optional[GradGuard] = None):
    """-> (optimizer, schedule): the reference's construct_optimizer (HOI/optimizers/lta/optimizer.py:15-73) plus lr_factory
    (HOI/optimizers/lta/lr_scheduler.py:11-41) restated on the fused optimizers, reading the reference's config fields: cfg.SOLVER
    .OPTIMIZING_METHOD ("sgd" | "adam" | "adamw"), .BASE_LR, .MOMENTUM, .DAMPENING, .NESTEROV, .WEIGHT_DECAY, .LR_POLICY, .WARMUP_STEPS,
    .MAX_EPOCH and cfg.BN.WEIGHT_DECAY. Two parameter groups as there: names containing "bn" take BN.WEIGHT_DECAY (the group may be empty),
    the rest SOLVER.WEIGHT_DECAY. `lr_policy` (default cfg.SOLVER.LR_POLICY): "cosine", "constant", "cosine_warmup", "linear_warmup";
    any other policy is a LambdaLR in the reference and needs `lr_lambda`, the function of the 0-based step it hands LambdaLR (for the
    get_epoch_lr policies: lambda step: get_epoch_lr(step / steps_in_epoch, cfg)), tabulated over MAX_EPOCH * steps_in_epoch steps.
    `guard` (a GradGuard, not a field of the reference's config): handed to the optimizer."""
    S = cfg.SOLVER
    bn, rest = [], []
    for name, p in model.named_parameters():
        (bn if "bn" in name else rest).append(p)
    groups = [{"params": bn, "weight_decay": cfg.BN.WEIGHT_DECAY}, {"params": rest, "weight_decay": S.WEIGHT_DECAY}]
    total = int(S.MAX_EPOCH) * int(steps_in_epoch)
    policy = S.LR_POLICY if lr_policy is None else lr_policy
    if policy == "cosine":
        schedule = LRSchedule.cosine_annealing(total)
    elif policy == "constant":
        schedule = LRSchedule.constant()
    elif policy == "cosine_warmup":
        schedule = LRSchedule.warmup_cosine(S.WARMUP_STEPS, total)
    elif policy == "linear_warmup":
        schedule = LRSchedule.warmup_linear(S.WARMUP_STEPS, total)
    elif lr_lambda is not None:
        schedule = LRSchedule.from_lambda(lr_lambda, max(total, 1))
    else:
        raise ValueError(f"construct_solver: lr_policy {policy!r} is not one of {SOLVER_POLICIES}; pass lr_lambda=<function of the step> "
                         "for a LambdaLR policy")
    method = S.OPTIMIZING_METHOD
    if method == "sgd":
        opt = FusedSGD(groups, lr=S.BASE_LR, momentum=S.MOMENTUM, dampening=S.DAMPENING, weight_decay=S.WEIGHT_DECAY,
                       nesterov=S.NESTEROV, schedule=schedule, guard=guard)
    elif method == "adam":
        opt = FusedAdam(groups, lr=S.BASE_LR, betas=(0.9, 0.999), weight_decay=S.WEIGHT_DECAY, schedule=schedule, guard=guard)
    elif method == "adamw":
        opt = FusedAdam(groups, lr=S.BASE_LR, betas=(0.9, 0.999), adamw=True, schedule=schedule, guard=guard)   # the groups' weight decays override the default
    else:
        raise NotImplementedError(f"Does not support {method} optimizer")
    return opt, schedule


def pad_ragged_batch(feats, lengths, target, capacity, T_pad=None):
    """A sampler batch of B clips -> the fixed shapes of a capacity-plan ragged step (forward_features_ragged(..., lengths=<device tensor>,
    capacity=)), so that ONE GraphedStep serves every batch: feats[k] (B, T, d_in) -> (B_cap, T_pad[k], d_in) zero-padded, lengths ((B,) or
    (B, K) frame counts, list or tensor) -> int32 (B_cap, K) with 0 for the unused rows (empty clips), target (B,) -> int64 (B_cap,) with -1
    there. capacity = (B_cap, tok_cap); T_pad (an int or one per segment; default: each tensor's own T) is the padded frame count the step
    was captured with. Everything lands on feats[0]'s device. Checked on the host, where the sampler's lengths still are: B <= B_cap,
    1 <= length <= T_pad and the batch's tokens <= tok_cap."""
    B_cap, tok_cap = int(capacity[0]), int(capacity[1])
    K, dev = len(feats), feats[0].device
    B = feats[0].shape[0]
    T_pad = [f.shape[1] for f in feats] if T_pad is None else ([int(T_pad)] * K if isinstance(T_pad, int) else [int(t) for t in T_pad])
    lens = torch.as_tensor(lengths).to("cpu", torch.int64)
    if lens.dim() == 1:
        lens = lens[:, None].expand(B, K)
    if tuple(lens.shape) != (B, K) or len(T_pad) != K:
        raise ValueError(f"lengths must have shape ({B},) or ({B}, {K}) and T_pad one entry per segment")
    if B > B_cap:
        raise ValueError(f"{B} clips in a batch of capacity B_cap = {B_cap}")
    for k, f in enumerate(feats):
        if f.shape[0] != B or f.shape[1] > T_pad[k]:
            raise ValueError(f"feats[{k}] has shape {tuple(f.shape)}: {B} clips of at most T_pad = {T_pad[k]} frames expected")
        if B and (int(lens[:, k].min()) < 1 or int(lens[:, k].max()) > f.shape[1]):
            raise ValueError(f"segment {k}: lengths must be 1 .. {f.shape[1]}, the frames feats[{k}] holds")
    if int(lens.sum()) > tok_cap:
        raise ValueError(f"the batch has {int(lens.sum())} tokens, the capacity tok_cap = {tok_cap}")
    out = []
    for k, f in enumerate(feats):
        p = torch.zeros((B_cap, T_pad[k], f.shape[2]), dtype=f.dtype, device=dev)
        p[:B, :f.shape[1]] = f
        out.append(p)
    lp = torch.zeros((B_cap, K), dtype=torch.int32)
    lp[:B] = lens.to(torch.int32)
    tp = torch.full((B_cap,), -1, dtype=torch.int64)
    tp[:B] = torch.as_tensor(target).to("cpu", torch.int64)
    return out, lp.to(dev), tp.to(dev)


class GraphedStep:
    """One training step — forward, loss, backward and (optionally) the optimizer update — captured ONCE as a hipGraph and replayed.

    The library only enqueues kernels on the current stream and keeps what changes from step to step in device memory (the dropout seed after
    `model.enable_device_seed()`, the optimizer's step count, - with an `LRSchedule` - its learning rates and - with a `GradGuard` - the clip / skip decision of the step), so a replay is exact training work with fresh masks; what the capture removes is the
    host side of the step (Python, the autograd engine's worker thread, a dozen launches: 0.54 - 0.90 ms per step on the bench configuration with
    FusedAdam against 0.41 ms of GPU time). This is the
    loop `bench.py` times, packaged for a training script:

        step = GraphedStep(lambda f, y: criterion(model.forward_features(*f), y), example_inputs=(feats, target),
                           params=model.parameters(), optimizer=FusedAdam(model.parameters(), lr=1e-4))
        for feats, target in loader:
            loss = step(feats, target)          # copies the batch into the captured buffers, replays, returns the loss tensor (device)

    `loss_fn(*inputs)` must be a pure function of its (possibly nested list / tuple of) tensor arguments with FIXED shapes and dtypes: a batch of
    another shape needs another GraphedStep (the reference's length-bucketed TTM sampler yields a handful of shapes — keep one per shape, or
    pad every batch to ONE capacity with pad_ragged_batch and capture forward_features_ragged(..., lengths=<device tensor>, capacity=): the
    lengths are then data of the step like the features, INTEGRATION.md "Ragged batches in a captured step").
    Gradients stay in `.grad` after every replay (`optimizer=None`: update them yourself outside the graph)."""

    def __init__(self, loss_fn, example_inputs, params, optimizer=None, warmup: int = 3):
        self.loss_fn, self.optimizer = loss_fn, optimizer
        self.params = [p for p in params if p.requires_grad]
        self.static = self._clone_tree(example_inputs)
        self._one = None
        dev = self.params[0].device
        # The warm-up runs REAL steps on `example_inputs` (allocator, lazy initialisation, FusedAdam re-pointing the parameters into its flat
        # buffers: all of that has to happen before the capture). With an optimizer they would leave `warmup` updates from the example batch
        # behind: parameters, optimizer moments / step count and the device-resident dropout seeds are snapshotted here and
        # restored afterwards, so the first replay starts exactly where the caller's model and optimizer were.
        snap_p = [p.detach().clone() for p in self.params]
        snap_o = None
        if optimizer is not None:
            import copy
            snap_o = copy.deepcopy(optimizer.state_dict())
        seeds = [m._egx_seed_dev for m in self._seed_owners(loss_fn)]
        snap_s = [t.clone() for t in seeds]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 1)):
                self._step()
            with torch.no_grad():
                for p, v in zip(self.params, snap_p):
                    p.copy_(v)
                for t, v in zip(seeds, snap_s):
                    t.copy_(v)
            if optimizer is not None:
                optimizer.load_state_dict(snap_o)
                if getattr(optimizer, "guard", None) is not None:
                    optimizer.guard.reset_counters()       # the warm-up steps are not the caller's: a fresh step reports steps == 0
            F_egx.note_weights_changed()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.loss = self._step()
        torch.cuda.synchronize(dev)

    @staticmethod
    def _seed_owners(loss_fn):
        """Modules with a device-resident dropout seed that `loss_fn` closes over (model.enable_device_seed())."""
        found = []
        cells = getattr(loss_fn, "__closure__", None) or ()
        objs = [c.cell_contents for c in cells if c is not None]
        objs += [getattr(loss_fn, "__self__", None)]
        for o in objs:
            mods = o.modules() if isinstance(o, nn.Module) else ()
            for m in mods:
                if isinstance(getattr(m, "_egx_seed_dev", None), torch.Tensor) and all(m is not f for f in found):
                    found.append(m)
        return found

    def _clone_tree(self, t):
        if isinstance(t, torch.Tensor):
            return t.detach().clone()
        if isinstance(t, (list, tuple)):
            return type(t)(self._clone_tree(x) for x in t)
        raise TypeError(f"GraphedStep: inputs must be tensors or nested lists / tuples of tensors, got {type(t).__name__}")

    def _copy_tree(self, dst, src):
        if isinstance(dst, torch.Tensor):
            if dst.shape != src.shape or dst.dtype != src.dtype:
                raise ValueError(f"GraphedStep: input of shape {tuple(src.shape)} / {src.dtype} where the step was captured with "
                                 f"{tuple(dst.shape)} / {dst.dtype} (one GraphedStep per batch shape)")
            dst.copy_(src, non_blocking=True)
        else:
            if len(dst) != len(src):
                raise ValueError("GraphedStep: input structure differs from the captured one")
            for d, s in zip(dst, src):
                self._copy_tree(d, s)

    def _step(self):
        for p in self.params:
            p.grad = None
        loss = self.loss_fn(*self.static)
        if self._one is None:
            self._one = torch.ones_like(loss)
        loss.backward(gradient=self._one)
        if self.optimizer is not None:
            self.optimizer.step()
        return loss.detach()

    def __call__(self, *inputs):
        self._copy_tree(self.static, type(self.static)(inputs) if isinstance(self.static, (list, tuple)) else inputs[0])
        self.graph.replay()
        if self.optimizer is not None:
            F_egx.note_weights_changed()           # the replayed update wrote the parameters behind torch's back
        return self.loss
