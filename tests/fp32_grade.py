"""fp32-grade gate of the f32 / f32s encoder paths: the case table, the weights that keep every ReLU pre-activation away from its kink,
the fp64 oracle run of a case, the GPU run of a case and the metric that tells fp32-grade arithmetic from bf16-grade.

Why the kink matters: a pre-activation within ~1e-6 of zero can land on the other side of the ReLU in fp32 and move a weight gradient by
~1e-3 (tools/fuzz_parity.py ReluSpy), which is why the older parity tests hold f32 / f32s to 1e-3 / 1e-2. kink_free() re-chooses only
every layer's linear1.bias so that no pre-activation of the case comes near zero (>= 1e-4 x rms, hundreds of fp32 roundings), under the
case's own dropout masks; with the flips gone the whole comparison is held to fp32 grade:
    logits / per-frame rows   max |d| / max(1, |ref|) <= 2e-6
    loss                      relative error <= 2e-6
    every gradient            ||d|| <= 2e-5 ||ref|| + 2e-7 sqrt(n)   (the floor form of tests/test_gpu_step_fusion.py _same)
A single GEMM operand rounded to bf16 misses the gradient bound by 20x and more (tests/test_cpu_fp32_grade.py).

Shared by tests/test_gpu_fp32_grade.py (-m gpu), tests/test_cpu_fp32_grade.py and tools/f32s_err_report.py. Test infrastructure only."""
from __future__ import annotations

import math
import os
from contextlib import contextmanager
from dataclasses import dataclass, replace
from types import SimpleNamespace as NS
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import translator_ref as tr
from tests import dropmask as dm
from tests.util import hhi_args, seeded_feats, seeded_state_dict

OUT_TOL = 2e-6          # logits and per-frame rows: max |d| / max(1, |ref|)
LOSS_TOL = 2e-6         # loss: relative
GRAD_RTOL = 2e-5        # gradients: ||d|| <= GRAD_RTOL ||ref|| + GRAD_FLOOR sqrt(n)
GRAD_FLOOR = 2e-7
GRAD_RTOL_MAX = 1e-4    # no case may carry a looser gradient bound than this
MARGIN_MIN = 1e-4       # min |a| / rms(a) of every layer's ReLU pre-activations after kink_free
CE_W = [0.266, 0.734]
LOSSAV_W = [1.0, 4.0]
EDGES3 = ((10, 10, 10), (15, 15, 15), (16, 16, 16), (16, 16, 17), (32, 32, 32), (32, 32, 33), (107, 107, 107), (150, 150, 150),
          (170, 170, 172), (15, 90, 150), (48, 1, 2), (100, 49, 1))            # S_b = 30 45 48 49 96 97 321 450 512 255 51 150
EDGES2 = ((15, 15), (22, 23), (24, 24), (24, 25), (48, 48), (48, 49), (160, 161), (225, 225), (256, 256), (1, 150), (90, 7))


# ---- the weights ---------------------------------------------------------------------------------------------------------------------
@contextmanager
def _probe(fn):
    old = tr.relu_probe
    tr.relu_probe = fn
    try:
        yield
    finally:
        tr.relu_probe = old


def preacts(sd, forward) -> Dict[str, torch.Tensor]:
    """{layer prefix: (N, d_ff) fp64 pre-activations} of forward(sd64) (every call of the layer pooled: all clips of a ragged batch)."""
    got: Dict[str, list] = {}
    sd64 = tr.to_dtype(sd, torch.float64)
    with torch.no_grad(), _probe(lambda prefix, a: got.setdefault(prefix, []).append(a.reshape(-1, a.shape[-1]))):
        forward(sd64)
    return {k: torch.cat(v, 0) for k, v in got.items()}


def kink_free(sd, forward, n_layers: int, prefix: str, lo: float = 0.3, hi: float = 0.7):
    """Re-choose every layer's linear1.bias, layer by layer from the bottom (layer l's pre-activations depend on the biases below it),
    unit by unit: with the unit's bias at 0, take its fp64 pre-activations over the whole case (forward(sd64) runs the oracle under the
    case's masks) and set the bias to minus the midpoint of the widest gap between consecutive values from the `lo` to the `hi` quantile.
    Every token keeps its own on / off pattern and 30 .. 70 % of the pre-activations stay positive. Biases are rounded to fp32 and the
    margins recomputed with them. -> (new state dict, {layer: (min |a| / rms(a), fraction of a > 0)})."""
    sd = dict(sd)
    for layer in range(n_layers):
        lp = f"{prefix}layers.{layer}."
        key = lp + "linear1.bias"
        sd[key] = torch.zeros_like(sd[key])
        v, _ = preacts(sd, forward)[lp].sort(dim=0)
        n = v.shape[0]
        i0, i1 = int(math.floor(lo * (n - 1))), int(math.ceil(hi * (n - 1)))
        i1 = max(i1, i0 + 1)
        k = (v[i0 + 1:i1 + 1] - v[i0:i1]).argmax(dim=0)[None]
        mid = 0.5 * (v.gather(0, i0 + k) + v.gather(0, i0 + k + 1))[0]
        sd[key] = (-mid).to(torch.float32)
    return sd, margins(sd, forward, n_layers, prefix)


def margins(sd, forward, n_layers: int, prefix: str):
    a = preacts(sd, forward)
    out = {}
    for layer in range(n_layers):
        x = a[f"{prefix}layers.{layer}."]
        out[layer] = ((x.abs().min() / x.pow(2).mean().sqrt()).item(), (x > 0).double().mean().item())
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    family: str                 # perclip | sliced | tiled | ragged_inf | ragged_train | generic | hoi
    kind: str                   # ttm3 | ttm2 | asd | pnr3 | lta4
    compute: str = "f32s"
    B: int = 1
    T: int = 15                 # frames per segment (ragged: `clips`)
    L: int = 1
    p: float = 0.0              # encoder-layer dropout
    p_pos: float = 0.0          # positional dropout (HHI)
    p_feat: float = 0.0         # feature dropout (HOI)
    impl: str = "auto"          # the implementation asked for
    expect: str = "fused"       # last_encoder_impl() it must run
    slices: int = 1             # last_encoder_slices() (per-clip families)
    env: Tuple[Tuple[str, int], ...] = ()      # EGX_FFN_CUT / EGX_FFN_SLICES pinned for the run
    det: bool = False           # set_deterministic(True)
    wcache: bool = False        # enable_weight_cache()
    loss: str = "ce"            # ce | ce_fused (target= in the forward) | rows | lossav (fused lossAV) | lin | none
    clips: tuple = ()           # ragged: frame counts per clip in argument order
    seed: int = 0
    grad_rtol: Optional[float] = None       # a looser gradient bound, with its measured number next to it (never above GRAD_RTOL_MAX)
    out_tol: Optional[float] = None         # a looser output bound, likewise (per-frame rows: the max over ~10^5 fp32 LayerNorm outputs)

    @property
    def prefix(self) -> str:
        return "transformer." if self.kind in ("pnr3", "lta4") else "transformer_encoder."

    @property
    def rtol(self) -> float:
        return GRAD_RTOL if self.grad_rtol is None else self.grad_rtol

    def control(self) -> "Case":
        """The same run in bf16: the negative control of its family."""
        return replace(self, id=self.id + "-bf16", compute="bf16")


CUT0, CUT1 = (("EGX_FFN_CUT", 0), ("EGX_FFN_SLICES", 1)), (("EGX_FFN_CUT", 1), ("EGX_FFN_SLICES", 1))
_PC = dict(family="perclip", kind="ttm3", impl="fused", expect="fused")
_TL = dict(family="tiled", kind="ttm3", L=2, p=0.5, p_pos=0.1)
CASES = [
    # per-clip kernels, one launch (EGX_FFN_CUT=0) and cut at the FFN (=1), one workgroup per clip
    Case("pc-b256-p0-one", B=256, env=CUT0, seed=101, **_PC),
    Case("pc-b256-p0-cut", B=256, env=CUT1, seed=101, **_PC),
    Case("pc-b256-p05-one", B=256, p=0.5, p_pos=0.1, env=CUT0, seed=102, **_PC),
    Case("pc-b256-p05-cut", B=256, p=0.5, p_pos=0.1, env=CUT1, seed=102, **_PC),
    Case("pc-b1-p05-one", B=1, p=0.5, p_pos=0.1, env=CUT0, seed=103, **_PC),
    Case("pc-b257-p05-cut", B=257, T=3, p=0.5, p_pos=0.1, env=CUT1, seed=104, **_PC),
    Case("pc-t1-l3-one", B=9, T=1, L=3, p=0.5, p_pos=0.1, env=CUT0, seed=105, **_PC),
    Case("pc-t7-l2-cut", B=33, T=7, L=2, p=0.5, p_pos=0.1, env=CUT1, seed=106, **_PC),
    Case("pc-t16-l3-one", B=6, T=16, L=3, p=0.5, p_pos=0.1, env=CUT0, seed=107, **_PC),
    Case("pc-t16-l2-cut", B=40, T=16, L=2, seed=108, env=CUT1, **_PC),
    Case("pc-f32-b256-p05", compute="f32", B=256, p=0.5, p_pos=0.1, env=CUT0, seed=102, **_PC),
    Case("pc-f32-t16-l2", compute="f32", B=6, T=16, L=2, p=0.5, p_pos=0.1, env=CUT0, seed=107, **_PC),
    # deterministic backward, cut, cross entropy inside the forward (bench "high" configuration)
    Case("pc-det-cut-ce", B=256, p=0.5, p_pos=0.1, env=CUT1, det=True, loss="ce_fused", seed=109, **_PC),
    # packed weight cache: the keep-scale 1 / 0.9 folded into the packed copies
    Case("pc-wcache-p01", B=64, L=2, p=0.1, p_pos=0.1, env=CUT0, wcache=True, seed=110, **_PC),
    # sliced mode: eight workgroups per clip
    Case("sl-b26", family="sliced", kind="ttm3", B=26, p=0.5, p_pos=0.1, impl="fused", slices=8, env=(("EGX_FFN_SLICES", 8),), seed=111),
    Case("sl-b1", family="sliced", kind="ttm3", B=1, p=0.5, p_pos=0.1, impl="fused", slices=8, env=(("EGX_FFN_SLICES", 8),), seed=112),
    # ASD: per-frame rows through a fixed linear functional, and the fused lossAV (egx_token_ce)
    # (rows: the max over 491 520 LayerNorm outputs; measured 2.4e-6 on MI355X, 4.7e-6 for the oracle itself in fp32)
    Case("asd-rows-b256", family="perclip", kind="asd", B=256, L=2, p=0.1, p_pos=0.1, impl="fused", env=CUT1, loss="rows", seed=113,
         out_tol=1e-5),
    Case("asd-lossav", family="perclip", kind="asd", B=140, L=2, p=0.1, p_pos=0.1, impl="fused", env=CUT0, wcache=True, loss="lossav",
         seed=114),
    # HOI d = 128 PNR / OSCC recipe on the per-clip kernels: 8 heads, d_ff = 256, 6 layers, feature dropout, learned pe
    Case("hoi-pnr3-f32s", family="hoi", kind="pnr3", B=4, L=6, p=0.1, p_feat=0.2, impl="fused", env=CUT0, loss="lin", seed=115),
    Case("hoi-pnr3-f32", family="hoi", kind="pnr3", compute="f32", B=4, L=6, p=0.1, p_feat=0.2, impl="fused", env=CUT0, loss="lin",
         seed=115),
    # tiled (48 < S <= 512): 3-task S = 51, 60, 96, 321, 450; 2-task S = 320, 512
    Case("tl-s51", B=5, T=17, seed=121, expect="tiled", **_TL),
    Case("tl-s60", B=6, T=20, seed=122, expect="tiled", **_TL),
    Case("tl-s96", B=4, T=32, seed=123, expect="tiled", **_TL),
    Case("tl-s320", B=2, T=160, seed=124, expect="tiled", **{**_TL, "kind": "ttm2"}),
    Case("tl-s321", B=2, T=107, seed=125, expect="tiled", **_TL),
    Case("tl-s450", B=2, T=150, seed=126, expect="tiled", **_TL),
    Case("tl-s512", B=2, T=256, seed=127, expect="tiled", **{**_TL, "kind": "ttm2"}),
    Case("tl-s90-det", B=8, T=30, seed=128, expect="tiled", det=True, **_TL),
    # ragged inference (forward_features(lengths=)), eval: with the pooled head, and the ASD rows
    Case("ri-ttm3", family="ragged_inf", kind="ttm3", L=2, clips=EDGES3, expect="ragged", loss="none", seed=131),
    Case("ri-ttm2", family="ragged_inf", kind="ttm2", L=1, clips=EDGES2, expect="ragged", loss="none", seed=132),
    Case("ri-asd", family="ragged_inf", kind="asd", L=2, clips=EDGES3, expect="ragged", loss="none", seed=133,
         out_tol=1e-5),         # (rows: measured 1.9e-6 on MI355X, 2.2e-6 for the oracle itself in fp32)
    # ragged training (forward_features_ragged + the weighted cross entropy over the batch)
    Case("rt-ttm3-l1-p0", family="ragged_train", kind="ttm3", L=1, clips=EDGES3, expect="ragged", loss="ce_fused", seed=141),
    Case("rt-ttm2-l2-p0", family="ragged_train", kind="ttm2", L=2, clips=EDGES2, expect="ragged", loss="ce_fused", seed=142),
    Case("rt-ttm3-l2-p05", family="ragged_train", kind="ttm3", L=2, p=0.5, p_pos=0.1, clips=EDGES3, expect="ragged", loss="ce_fused",
         seed=143),
    Case("rt-ttm2-l1-p05", family="ragged_train", kind="ttm2", L=1, p=0.5, p_pos=0.1, clips=EDGES2, expect="ragged", loss="ce_fused",
         seed=144),
    # the shape-generic kernels in exact fp32
    Case("gen-ttm3-s69", family="generic", kind="ttm3", compute="f32", B=5, T=23, L=2, p=0.5, p_pos=0.1, impl="generic",
         expect="generic", seed=151),
    Case("gen-lta4-d256", family="generic", kind="lta4", compute="f32", B=3, T=4, L=2, p=0.3, impl="generic", expect="generic",
         loss="lin", seed=152),
]
BY_ID = {c.id: c for c in CASES}
# one bf16 run per family through the same metric: it must miss the bound by >= 10x (the comparison is live)
CONTROLS = [BY_ID[i].control() for i in ("pc-b256-p05-cut", "tl-s321", "ri-ttm3", "rt-ttm3-l1-p0")]
CONTROL_MIN = 10.0


# ---- one case: model, data, oracle ---------------------------------------------------------------------------------------------------
def _lta_cfg(n, d, heads, layers, p):
    return NS(FORECASTING=NS(NUM_INPUT_CLIPS=n, NUM_ACTIONS_TO_PREDICT=3),
              MODEL=NS(TRANSLATION_HEADS=heads, TRANSLATION_LAYERS=layers, TRANSLATION_INPUT_FEATURES=d, TRANSLATION_DROPOUT=p,
                       NUM_CLASSES=[5, 7], DROPOUT_RATE=0.0, HEAD_ACT="softmax"), TEST=NS(NO_ACT=False))


def new_model(case: Case):
    """The case's translator on the CPU with seeded_state_dict weights."""
    from egot2_amd import hhi_asd, hhi_ttm, hoi_lta, hoi_pnr
    if case.kind in ("ttm3", "ttm2", "asd"):
        cls = {"ttm3": hhi_ttm.TaskFusionMFTransformer3Task, "ttm2": hhi_ttm.TaskFusionMFTransformer2Task,
               "asd": hhi_asd.TaskFusionMFTransformer3Task}[case.kind]
        m = cls(hhi_args(num_layers=case.L, dropout=case.p))
    elif case.kind == "pnr3":
        m = hoi_pnr.TaskFusionMFTransformer3TaskDropout(NS(DATA=NS(TASK="state_change_detection"), MODEL=NS(
            TRANSLATION_INPUT_FEATURES=128, TRANSLATION_LAYERS=case.L, FEAT_DROPOUT_RATE=case.p_feat, TRANSFORMER_DROPOUT_RATE=case.p)))
    else:
        m = hoi_lta.TaskFusionMFTransformerLTA4Task(_lta_cfg(case.T, 256, 8, case.L, case.p))
    m.load_state_dict(seeded_state_dict(m, case.seed))
    if hasattr(m, "pos_embed"):
        m.pos_embed.dropout.p = case.p_pos
    return m


def _seg_shapes(case: Case):
    B, T = case.B, case.T
    if case.kind == "pnr3":
        return [(B, 16, 8192), (B, 16, 8192), (B, 8, 2048), (B, 8, 256)]
    if case.kind == "lta4":
        return [(B, T, 8192), (B, T, 8192), (B, T, 256), (B, T, 2048)]
    return [(B, T, 256)] * (2 if case.kind == "ttm2" else 3)


def _cast(masks, dtype):
    if masks is None:
        return None
    if isinstance(masks, torch.Tensor):
        return masks.to(dtype)
    if isinstance(masks, dict):
        return {k: _cast(v, dtype) for k, v in masks.items()}
    return [_cast(v, dtype) for v in masks]


def mask_seed(case: Case) -> int:
    return 0x0F32_0000 + case.seed


def case_data(case: Case):
    """Inputs of the case (fp32, CPU), its masks as the implementation draws them (fp64 keep-scales) and the loss's fixed tensors."""
    rng = np.random.default_rng(case.seed)
    seed = mask_seed(case)
    d = {"seed": seed}
    if case.family.startswith("ragged"):
        d["clips"] = [[f[0] for f in seeded_feats(case.seed * 100 + i, [(1, T, 256) for T in tup])] for i, tup in enumerate(case.clips)]
        d["target"] = torch.from_numpy(rng.integers(0, 2, len(case.clips))).long()
        d["clip_masks"] = [None] * len(case.clips)
        if case.family == "ragged_train" and (case.p > 0 or case.p_pos > 0):
            tok0 = 0
            for i, tup in enumerate(case.clips):
                d["clip_masks"][i] = dm.ragged_clip_masks(seed, tok0, sum(tup), case.L, case.p, case.p_pos)
                tok0 += sum(tup)
        return d
    d["feats"] = seeded_feats(case.seed + 1, _seg_shapes(case))
    B, T = case.B, case.T
    impl = {"perclip": "fused", "sliced": "fused", "hoi": "fused"}.get(case.family, case.family)
    masks = None
    if case.p > 0 or case.p_pos > 0 or case.p_feat > 0:
        if case.kind == "pnr3":
            masks = dm.encoder_masks(seed, impl, B, [16, 16, 8, 8], 128, 8, 256, case.L, case.p, 0.0, case.p_feat)
        elif case.kind == "lta4":
            masks = dm.encoder_masks(seed, impl, B, [T] * 4, 256, 8, 2048, case.L, case.p)
        else:
            masks = dm.encoder_masks(seed, impl, B, [T] * len(_seg_shapes(case)), 128, 4, 2048, case.L, case.p, case.p_pos)
    d["masks"] = masks
    if case.loss in ("ce", "ce_fused"):
        d["target"] = torch.from_numpy(rng.integers(0, 2, B)).long()
    elif case.loss == "rows":
        d["w"] = torch.from_numpy(rng.standard_normal((B * T, 128), dtype=np.float32) / B)
    elif case.loss == "lossav":
        d["labels"] = torch.from_numpy(rng.integers(0, 2, B * T)).long()
        d["fc_w"] = torch.from_numpy(rng.standard_normal((2, 128), dtype=np.float32) * 0.2)
        d["fc_b"] = torch.from_numpy(rng.standard_normal(2, dtype=np.float32) * 0.1)
    return d


def lin_w(n: int) -> torch.Tensor:
    """The fixed linear functional of `lin` cases: n weights from -1 to 1 (fp32, the same on both sides)."""
    return torch.from_numpy(np.linspace(-1, 1, n, dtype=np.float32))


def oracle_outputs(case: Case, sd, data, feats=None, dtype=torch.float64):
    """The oracle forward of the case on `sd` (already in `dtype`): a flat tuple of output tensors (one per clip for a ragged case)."""
    n = 4 if case.kind in ("ttm3", "ttm2", "asd") else 8
    if case.family.startswith("ragged"):
        clips = feats if feats is not None else [[x.to(dtype) for x in c] for c in data["clips"]]
        outs = []
        for c, mk in zip(clips, data["clip_masks"]):
            xs = [x[None] for x in c]
            mk = _cast(mk, dtype)
            outs.append(tr.asd_forward(sd, n, *xs, masks=mk) if case.kind == "asd" else tr.ttm_forward(sd, n, *xs, masks=mk))
        return tuple(outs)
    xs = feats if feats is not None else [f.to(dtype) for f in data["feats"]]
    mk = _cast(data["masks"], dtype)
    if case.kind == "asd":
        return (tr.asd_forward(sd, n, *xs, masks=mk),)
    if case.kind == "pnr3":
        return (tr.pnr3_forward(sd, n, *xs, masks=mk),)
    if case.kind == "lta4":
        return tuple(tr.lta4_forward(sd, n, *xs, [5, 7], masks=mk))
    return (tr.ttm_forward(sd, n, *xs, masks=mk),)


def kink_free_sd(case: Case, sd, data):
    return kink_free(sd, lambda sd64: oracle_outputs(case, sd64, data), case.L, case.prefix)


def prepare(case: Case):
    """(kink-free state dict, margins, data): everything a run of the case needs, from the seeds alone."""
    m = new_model(case)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}       # (pnr3: `ln` is shared with linear_head.0)
    data = case_data(case)
    sd, marg = kink_free_sd(case, sd, data)
    return sd, marg, data


def _loss(case: Case, out, data, dtype):
    """The scalar the backward starts from, on flat outputs (logits / rows, one tensor per clip for ragged); None without one."""
    if case.loss == "none":
        return None
    if case.loss in ("ce", "ce_fused"):
        return tr.weighted_ce(out, data["target"], CE_W)
    if case.loss == "lossav":
        return None     # needs the classifier's own leaves (oracle_run)
    w = data["w"] if case.loss == "rows" else lin_w(out.numel())
    return (out.reshape(-1) * w.to(dtype).reshape(-1)).sum()


def oracle_run(case: Case, sd, data, dtype=torch.float64, want_grads=True):
    """-> {"out": flat outputs (logits of every clip / rows, concatenated), "loss", "grads": {name: gradient}, "feat_grads": {name: ...}}
    computed by the oracle in `dtype` (fp64: the reference; fp32: what fp32-grade looks like)."""
    grads_on = want_grads and case.loss != "none"
    sdd = {k: v.to(dtype).requires_grad_(grads_on and v.is_floating_point() and not k.endswith(".pe")) if v.is_floating_point() else v
           for k, v in sd.items()}
    feats = None
    if case.family.startswith("ragged"):
        feats = [[x.to(dtype).requires_grad_(grads_on and case.family == "ragged_train") for x in c] for c in data["clips"]]
    with torch.set_grad_enabled(grads_on):
        outs = oracle_outputs(case, sdd, data, feats=feats, dtype=dtype)
        if case.family.startswith("ragged"):
            out = torch.cat([o.reshape(o.shape[0], -1) for o in outs], 0)
        else:
            out = outs[0] if len(outs) == 1 else torch.cat([o.reshape(-1) for o in outs])
        res = {"out": out.detach()}
        extra = {}
        if case.loss == "lossav":
            fw = data["fc_w"].to(dtype).requires_grad_(True)
            fb = data["fc_b"].to(dtype).requires_grad_(True)
            z = out.reshape(-1, 128) @ fw.t() + fb
            loss = tr.weighted_ce(z, data["labels"], LOSSAV_W)
            res["out"] = torch.softmax(z.detach(), dim=-1).reshape(-1)      # the fused form returns the scores, not the rows
            extra = {"FC.weight": fw, "FC.bias": fb}
        else:
            loss = _loss(case, out, data, dtype)
        if loss is not None:
            res["loss"] = loss.item()
        if grads_on:
            loss.backward()
            res["grads"] = {k: v.grad for k, v in {**sdd, **extra}.items() if isinstance(v, torch.Tensor) and v.grad is not None}
            if feats is not None:
                res["feat_grads"] = {f"feat{k}/clip{b}": x.grad for b, c in enumerate(feats) for k, x in enumerate(c)}
    return res


# ---- the metric ----------------------------------------------------------------------------------------------------------------------
def out_err(a, ref) -> float:
    a, ref = a.detach().double().cpu().reshape(ref.shape), ref.double()
    return ((a - ref).abs() / ref.abs().clamp(min=1.0)).max().item()


def grad_ratio(g, ref, rtol=GRAD_RTOL) -> float:
    """||g - ref|| / (rtol ||ref|| + GRAD_FLOOR sqrt(n)): <= 1 is fp32 grade."""
    g, ref = g.detach().double().cpu(), ref.double().cpu()
    return (g - ref).norm().item() / (rtol * ref.norm().item() + GRAD_FLOOR * ref.numel() ** 0.5)


def measure(case: Case, res, ref, rtol: Optional[float] = None):
    """Every quantity of `res` against `ref` as a multiple of its bound: {"ratio": {name: x bound}, "out_err", "loss_err", "grad_err"
    (worst relative gradient error), "worst": (name, x bound), "bad": names over the bound}."""
    rtol = case.rtol if rtol is None else rtol
    assert rtol <= GRAD_RTOL_MAX, (case.id, rtol)
    r, rel = {}, {}
    m = {"out_err": out_err(res["out"], ref["out"])}
    r["out"] = m["out_err"] / (OUT_TOL if case.out_tol is None else case.out_tol)
    if "loss" in ref and case.loss in ("ce", "ce_fused", "lossav"):      # (a fixed linear functional's value is only the outputs again)
        m["loss_err"] = abs(res["loss"] - ref["loss"]) / max(abs(ref["loss"]), 1e-30)
        r["loss"] = m["loss_err"] / LOSS_TOL
    for group in ("grads", "feat_grads"):
        if group not in ref:
            continue
        assert set(res[group]) == set(ref[group]), (case.id, group, sorted(set(res[group]) ^ set(ref[group])))
        for k, g in ref[group].items():
            r[k] = grad_ratio(res[group][k], g, rtol)
            rel[k] = (res[group][k].double().cpu() - g.double()).norm().item() / max(g.double().norm().item(), 1e-30)
    m["ratio"] = r
    m["grad_err"] = max(rel.values()) if rel else 0.0
    m["worst"] = max(r.items(), key=lambda kv: kv[1])
    m["bad"] = {k: round(v, 2) for k, v in r.items() if not v <= 1.0}
    return m


# ---- one case on the GPU -------------------------------------------------------------------------------------------------------------
@contextmanager
def _env(kv):
    old = {k: os.environ.get(k) for k, _ in kv}
    os.environ.update({k: str(v) for k, v in kv})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pad(clips, cuda, grad):
    K = len(clips[0])
    feats = []
    for k in range(K):
        Tm = max(c[k].shape[0] for c in clips)
        t = torch.full((len(clips), Tm, 256), float("nan"), dtype=torch.float32)
        for b, c in enumerate(clips):
            t[b, :c[k].shape[0]] = c[k]
        feats.append(t.to(cuda).requires_grad_(grad))
    return feats, torch.tensor([[c[k].shape[0] for k in range(K)] for c in clips])


def gpu_run(case: Case, sd, data, cuda):
    """Forward, loss and backward of the case through the HIP library -> the oracle_run layout plus "impl" / "slices" (what ran) and
    "pad_grad_zero" (ragged training: every padded frame's gradient is exactly 0)."""
    from egot2_amd import functional as F_egx, hhi_asd
    with _env(case.env):
        m = new_model(case)
        m.load_state_dict(sd)
        m = m.to(cuda).set_compute(case.compute, case.impl)
        m.train(case.family != "ragged_inf")
        if case.det:
            m.set_deterministic(True)
        if case.wcache:
            m.enable_weight_cache()
        m._egx_seed = lambda: data["seed"]
        res = {}
        extra = {}
        if case.family == "ragged_inf":
            feats, lengths = _pad(data["clips"], cuda, False)
            with torch.no_grad():
                out = m.forward_features(*feats, lengths=lengths)
            res["impl"] = F_egx.last_encoder_impl()
        elif case.family == "ragged_train":
            feats, lengths = _pad(data["clips"], cuda, True)
            out, loss = m.forward_features_ragged(*feats, lengths=lengths, target=data["target"].to(cuda),
                                                  class_weight=torch.tensor(CE_W, device=cuda))
            res["impl"] = F_egx.last_encoder_impl()
            loss.backward()
        else:
            feats = [f.to(cuda) for f in data["feats"]]
            if case.loss == "ce_fused":
                out, loss = m.forward_features(*feats, target=data["target"].to(cuda), class_weight=torch.tensor(CE_W, device=cuda))
            elif case.loss == "lossav":
                head = hhi_asd.lossAV(128)
                with torch.no_grad():
                    head.FC.weight.copy_(data["fc_w"])
                    head.FC.bias.copy_(data["fc_b"])
                head = head.to(cuda)
                loss, out = m.forward_features(*feats, lossav=head, labels=data["labels"].to(cuda))[:2]      # (nloss, predScore)
                extra = {"FC.weight": head.FC.weight, "FC.bias": head.FC.bias}
            else:
                out = m.forward_features(*feats)
            res["impl"], res["slices"] = F_egx.last_encoder_impl(), F_egx.last_encoder_slices()
            if case.loss == "ce":
                loss = torch.nn.functional.cross_entropy(out, data["target"].to(cuda), weight=torch.tensor(CE_W, device=cuda))
            elif case.loss in ("rows", "lin"):
                flat = torch.cat([o.reshape(-1) for o in out]) if isinstance(out, (list, tuple)) else out.reshape(-1)
                loss = (flat * (data["w"] if case.loss == "rows" else lin_w(flat.numel())).to(cuda).reshape(-1)).sum()
            loss.backward()
        torch.cuda.synchronize()
    if isinstance(out, (list, tuple)):
        out = torch.cat([o.reshape(-1) for o in out])
    res["out"] = out.detach().double().cpu()
    if case.family.startswith("ragged"):
        res["out"] = res["out"].reshape(res["out"].shape[0], -1)
    else:
        res["out"] = res["out"].reshape(-1)
    if case.loss != "none":
        res["loss"] = loss.item()
        named = {**dict(m.named_parameters()), **extra}
        res["grads"] = {k: p.grad.detach().double().cpu() for k, p in named.items() if p.grad is not None}
    if case.family == "ragged_train":
        res["feat_grads"], res["pad_grad_zero"] = {}, True
        for k, f in enumerate(feats):
            for b, c in enumerate(data["clips"]):
                T = c[k].shape[0]
                res["feat_grads"][f"feat{k}/clip{b}"] = f.grad[b, :T].detach().double().cpu()
                res["pad_grad_zero"] &= bool(torch.all(f.grad[b, T:] == 0).item())
    return res
