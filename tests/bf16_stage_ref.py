"""Stage-wise fp64 references of the d = 128 encoder kernels (per-clip one-launch / cut / sliced, tiled, ragged training), the bf16 rounding
map they apply, the error metric and the bars: the gate of tests/test_gpu_bf16_stages.py, tested on itself by tests/test_cpu_bf16_stages.py.

Why stage by stage. A model-level oracle that rounds every MFMA operand where the kernels do is useless as a sharp gate: two correct
evaluations of it (fp32 against fp64) already differ by 4.4e-3 on the logits and 1.6e-2 on the worst gradient after two layers, because an
upstream difference delta moves a share delta / 2^-8 of the next operand's elements to the neighbouring bf16 value (test_cpu_bf16_stages.py
re-measures this). So every stage here is TEACHER-FORCED: it starts from the items the device itself held going into the stage (read back
through the ABI v26 stage hooks, egot2_amd.functional.EncoderStages) and is compared with the item the device held coming out of it.
Identical fp32 inputs round identically; what is left is fp32 accumulation order and the few roundings inside the stage.

Plain torch; nothing comes from the product path except tests/dropmask.py for the masks. Every function computes in the dtype of its
arguments (fp64: the reference; fp32: the yardstick), as in tests/wide_ops_ref.py, whose elem_err / row_err are the metric (imported).

ROUNDING MAP of compute="bf16" (r(.) = one round-to-nearest-even to bf16: pack_bf16x2, csrc/common.h; every product accumulates in fp32;
csrc/ paths, line numbers of this commit). compute="f32s" splits every operand exactly into three bf16 parts instead: no rounding at all.
  stage                      operands rounded / kept                                                             where
  features -> PRE            r(feat) r(W_proj)^T + b, x feature-dropout scale                                    fused.hip:390 (to_frag), pack_weights (fused.hip:45); epilogue :409-421
  PRE -> XIN[0]              fp32: LayerNorm, + task embedding, + position, x positional-dropout scale           fused.hip:471-483
  XIN -> QKV                 r(xin) r(W_in)^T + b_in                                                             fused.hip:556 (load_frag), :575
  QKV, XIN -> RES1           per-clip kernels: S = r(Q) r(K)^T / sqrt(dh) in fp32; P = softmax(S) in fp32;       fused.hip:618-625, :637-666
   (per-clip)                Pd = r(P x attention keep-scale); O = Pd r(V) in fp32; res1 = (r(O) r(W_o)^T + b_o)  :683 (chain_frag), :679, :720, :737-744
                             x res1 keep-scale + xin (fp32 residual)
  QKV -> ATTN_O, LSE         tiled / ragged: s = r(Q c2) r(K)^T in log2 units, c2 = log2(e) / sqrt(dh) applied   tiled_attn.hip:171 (load_frag_scaled), :188-190
   (tiled, ragged)           in fp32 BEFORE the rounding; online softmax over 32-key blocks: p = exp2(s - m_run), :204-225 (chain_frag: r(p x keep01))
                             rounded relative to the RUNNING maximum; O = sum_blocks r(p keep) r(V / (1 - p_drop)) :179 (stage_planes with vscale), :229-231, :241-248
                             rescaled in fp32; lse2 = m + log2(l), l summed before the mask
  ATTN_O, XIN -> RES1        tiled / ragged: (r(O) r(W_o)^T + b_o) x res1 keep-scale + xin                        fused.hip:294-299, :720-744
  RES1 -> X1                 fp32 LayerNorm1; the device-held X1 is r(x1) (one bf16 plane): bf16_out              fused.hip:755-774 (store_block_bf16, fused_dev.h:527); ffn_cut.hip:266-272
  X1 -> HID, ALIVE           a = r(x1) r(s W1)^T + s b1 with s = 1 / (1 - p) multiplied into W1 in fp32 BEFORE    fused_host.hip:282 (fill_layer), fused.hip:45, :882-889, :898
                             its rounding; a dropped unit is set to -1; alive = sign bit of a clear;             :918-941 (relu_bits); ffn_cut.hip:324-414
                             H = r(relu(a)): the keep-scale is inside a, so H is rounded AFTER it                 :951 (chain_frag) = the stored tile (store_hid_tile_bf16, fused_dev.h:299)
  HID, RES1 -> RES2          (H r(W2)^T + b2) x res2 keep-scale + x1 with x1 = LayerNorm1(res1) in FP32 (the      fused.hip:971-979, :1045-1054; ffn_cut.hip:262
                             residual is never rounded; the bf16 plane is only the MFMA operand)
  RES2 -> XIN[l+1] / out     fp32 LayerNorm2; pooled head: token mean, LayerNorm, Linear, all fp32                fused.hip:1061-1065, :1172-1187; norm.hip (pool_head_fwd)
  G2, ALIVE -> DHID          dH = r(alive ? r(g2) r(s W2^T) : 0); the device-held G2 is r(g2) already             fused_bwd.hip:1671 (store_block_bf16), :1737, :1805-1824; fused_host.hip:287
  G1, QKV -> ATTN_O, DQKV    per-clip kernels: dO = r(g1) r(W_o) in fp32; r(Q), r(K), r(V), r(dO); P as in the    fused_bwd.hip:1999 (gemm_packed), :2050-2053, :2068-2069
   (per-clip)                forward; dPm = (dO V^T) x keep-scale; delta = sum_k P dPm (WITH the dropout);        :2093-2113
                             dS = r(P (dPm - delta) / sqrt(dh)); Pd = r(P x keep-scale); O = Pd V; dQ = dS K;    :2119-2120, :2140-2145 (chain_frag), :2155
                             dK = dS^T Q; dV = Pd^T dO (P, dS recomputed in the other orientation: same values)   :2181-2184, :2205-2210, :2229-2232
  G1, QKV, ATTN_O, LSE       tiled / ragged: dO = r(g1) r(W_o) in fp32 (dense, between the launches); delta =       fused_bwd.hip:1999-2012; tiled_attn.hip:283-293
   -> DQKV (tiled, ragged)   rowsum(dO . O) on the unrounded dO and the saved O; p = exp2(s - lse2) from the saved  :320, :420
                             log-sum-exp. dQ pass: s = r(Q c2) r(K)^T, dP = r(dO) r(V / (1 - p))^T x keep01,        :282, :291, :299-300, :314-321
                             dS = r(p (dP - delta)), dQ = (dS r(K)) / sqrt(dh) applied to the finished tile.         :336-351
                             dK / dV pass: s = r(Q) r(K c2)^T, dP = r(dO / (1 - p)) r(V)^T x keep01 (the scales      :382-383, :389-390, :411-424
                             multiplied in fp32 BEFORE the rounding), Pn = r(p x keep01), dS as above;              :430-438
                             dV = Pn^T r(dO / (1 - p)), dK = (dS^T r(Q)) / sqrt(dh)                                   :447-451
  weight gradients           dW_in = r(dqkv)^T r(xin), dW_o = r(g1)^T r(attn_o), dW_proj = r(dseg)^T r(feat)      fused_bwd.hip:1010 (small_dw_kernel `put`), fused_host.hip:614-618
                             dW1 = dH^T x1, dW2 = g2^T H from the four bf16 items as they are held                fused_bwd.hip:568-700 (ffn_dw_bf16_ring_kernel)
                             db1 = column sums of the bf16 dH (alive-masked); db_in, db_o, db_proj = fp32 column  fused_bwd.hip:664-671; :1986, :2246-2249, :2328 (partial rows)
                             sums of the fp32 dqkv, g1, dseg
Not derivable from held items (left to the model-level tests): db2 and the LayerNorm parameter gradients in bf16 mode (their operands, the
unrounded g2 / dY . xhat, never leave the workgroup).

Bars: BAR[stage][mode] = 8 x FP32_ERR[stage][mode] (the factor of tests/unit_ref.py and wide_ops_ref.py). FP32_ERR is this reference evaluated
in fp32, with the map's roundings, against its own fp64 evaluation from the same inputs, worst over CPU_CASES; test_cpu_bf16_stages.py
re-measures every entry and holds the constant within 3x. No bar was chosen by looking at the device.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from tests import dropmask as dm
from tests.wide_ops_ref import FACTOR, bf16r, elem_err, row_err

F64, F32 = torch.float64, torch.float32
LN_EPS = 1e-5
ALIVE_MARGIN = 1e-5         # |a| below this share of the layer's rms: the unit is left out of ALIVE and HID
ALIVE_SKIP_MAX = 1e-4       # at most this share of a layer's units may be left out
TA_C2 = float(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))      # tiled_attn.hip TA_C2 (an fp32 product)

# Measured by tests/test_cpu_bf16_stages.py::test_fp32_reference_meets_the_bar (prints them with -s): worst over CPU_CASES.
FP32_ERR: Dict[str, Dict[str, float]] = {
    "pre": {"bf16": 1.3e-7, "f32s": 2.9e-7}, "xin0": {"bf16": 2.2e-7, "f32s": 2.2e-7}, "qkv": {"bf16": 1.8e-7, "f32s": 4.2e-7},
    "res1_attn": {"bf16": 1.2e-7, "f32s": 4.4e-7}, "attn_tiled": {"bf16": 9.2e-7, "f32s": 3.0e-6}, "res1": {"bf16": 1.8e-7, "f32s": 3.6e-7},
    "x1": {"bf16": 5.2e-8, "f32s": 2.4e-7}, "hid": {"bf16": 4.4e-8, "f32s": 3.3e-7}, "res2": {"bf16": 2.0e-7, "f32s": 2.4e-7},
    "ln2": {"bf16": 2.1e-7, "f32s": 2.1e-7}, "out": {"bf16": 1.5e-7, "f32s": 1.8e-7}, "dhid": {"bf16": 4.9e-8, "f32s": 3.4e-7},
    "attn_bwd": {"bf16": 6.0e-7, "f32s": 4.0e-6}, "attn_bwd_tiled": {"bf16": 5.8e-8, "f32s": 6.5e-7},
    "wgrad": {"bf16": 5.2e-7, "f32s": 6.4e-7},
}


# Worst (smallest) error / bar of each perturbed reference over the cases it applies to (test_cpu_bf16_stages.py requires >= 3 of every one).
PERTURB_RATIO: Dict[str, float] = {
    "wgrad_g_unrounded": 299.0, "wgrad_x_unrounded": 291.0, "dw1_drop_last_block": 1.2e5, "dw2_drop_last_block": 1.2e5, "db1_without_alive": 1.3e5,
    "colsum_counts_padded_row": 1.1e4, "h_rounded_before_scale": 4.1e3, "p_unrounded": 716.0, "delta_without_dropout": 2.2e3,
    "res1_wrong_keep_scale": 8.3e3, "ln_var_dm1": 2.0e3, "attn_row_stride": 5.6e4, "tiled_ds_unrounded": 80.0, "tiled_q_scaled_after_rounding": 1.7e3,
    "ffn_mask_row_key": math.inf, "bias_unscaled": math.inf,       # (ALIVE bits differ outside the margin: an infinite error)
}
# Share of the values rounded INSIDE a stage that carry a flip allowance (rnd_track), bf16 mode, over CASES: measured by
# test_cpu_bf16_stages.py::test_flip_allowance_share_is_as_recorded, which holds each within 1.5x (a wider AMB shows there first).
AMB_SHARE = {"res1_attn": 0.031, "attn_tiled": 0.017, "attn_bwd": 0.37, "attn_bwd_tiled": 0.45}


def bar(stage: str, mode: str) -> float:
    return FACTOR * FP32_ERR[stage][mode]


def rnd(t, mode: str):
    return bf16r(t) if mode == "bf16" else t


def rnd_scaled(t, c: float, mode: str):
    """r(t c) with the product taken in fp32 first, as the kernels do (a keep-scale folded into a packed weight, c2 on Q)."""
    return rnd((t.to(F32) * np.float32(c)).to(t.dtype), mode)


# ---- the model and the batch as the stages see them ------------------------------------------------------------------------------------------
@dataclass
class Batch:
    """Token bookkeeping of one call. lens[b] = tokens of clip b; seg_T[b][k] = frames of segment k in clip b (token order)."""
    family: str                     # perclip | tiled | ragged
    lens: List[int]
    seg_T: List[List[int]]
    H: int
    d: int = 128
    dff: int = 2048
    tok0: List[int] = field(default_factory=list)
    seg_tok: List[torch.Tensor] = field(default_factory=list)      # per segment: the flat token index of each of its packed rows

    def __post_init__(self):
        self.tok0 = list(np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(int))
        K = len(self.seg_T[0])
        self.seg_tok = []
        for k in range(K):
            idx = []
            for b, Ts in enumerate(self.seg_T):
                off = self.tok0[b] + sum(Ts[:k])
                idx.extend(range(off, off + Ts[k]))
            self.seg_tok.append(torch.tensor(idx, dtype=torch.long))

    @property
    def N(self) -> int:
        return int(sum(self.lens))

    @property
    def dh(self) -> int:
        return self.d // self.H


@dataclass
class Model:
    """The parameters (fp32 masters) in token order of the segments."""
    proj: List[tuple]               # per segment (W, b, name of W, name of b)
    add_rows: Optional[torch.Tensor]        # (N, d) task-embedding row of every token, or None
    pos_rows: torch.Tensor          # (N, d) positional row of every token
    ln: tuple                       # shared LayerNorm (w, b)
    layers: List[dict]
    layer_prefix: List[str]
    head: Optional[tuple]           # (ln_w, ln_b, W, b) of the pooled head, or None (ASD rows)
    out_T: int = 0                  # head-less: first out_T tokens of every clip leave


_LAYER_KEYS = {"in_w": "self_attn.in_proj_weight", "in_b": "self_attn.in_proj_bias", "out_w": "self_attn.out_proj.weight",
               "out_b": "self_attn.out_proj.bias", "w1": "linear1.weight", "b1": "linear1.bias", "w2": "linear2.weight", "b2": "linear2.bias",
               "n1w": "norm1.weight", "n1b": "norm1.bias", "n2w": "norm2.weight", "n2b": "norm2.bias"}


def build(kind: str, sd, L: int, batch: Batch) -> Model:
    """kind ttm3 | ttm2 | asd | pnr3 (tests/fp32_grade.py Case.kind) on state dict `sd`."""
    N, d = batch.N, batch.d
    pos = torch.zeros(N, d)
    add = None
    if kind == "pnr3":
        names, prefix = ["proj1", "proj2", "proj3_slow", "proj3_fast"], "transformer."
        for b, S in enumerate(batch.lens):
            pos[batch.tok0[b]:batch.tok0[b] + S] = sd["pe"][0, :S]
        head = (sd["ln.weight"], sd["ln.bias"], sd["linear_head.1.weight"], sd["linear_head.1.bias"])
    else:
        names, ids = {"ttm3": (["ttm", "lam", "asd"], [0, 1, 2]), "ttm2": (["ttm", "lam"], [0, 1]), "asd": (["asd", "ttm", "lam"], [2, 0, 1])}[kind]
        names, prefix = [f"proj_{n}" for n in names], "transformer_encoder."
        add, pe = torch.zeros(N, d), sd["pos_embed.pe"][:, 0, :]
        for k, tid in enumerate(ids):
            add[batch.seg_tok[k]] = sd["task_embed"][0, tid]
            row = 0
            for Ts in batch.seg_T:
                pos[batch.seg_tok[k][row:row + Ts[k]]] = pe[:Ts[k]]
                row += Ts[k]
        head = None if kind == "asd" else tuple(sd[f"linear_head.{i}.{p}"] for i, p in ((0, "weight"), (0, "bias"), (1, "weight"), (1, "bias")))
    lp = [f"{prefix}layers.{l}." for l in range(L)]
    return Model(proj=[(sd[n + ".weight"], sd[n + ".bias"], n + ".weight", n + ".bias") for n in names], add_rows=add, pos_rows=pos,
                 ln=(sd["ln.weight"], sd["ln.bias"]), layers=[{k: sd[p + v] for k, v in _LAYER_KEYS.items()} for p in lp], layer_prefix=lp,
                 head=head, out_T=batch.seg_T[0][0] if kind == "asd" else 0)


class Masks:
    """The dropout decisions of one call (tests/dropmask.py): keep = bool tensors, the keep-scale 1 / (1 - p) as fp32 value. Keys as the
    kernels form them: token sites by the flat token index; FFN by clip * 64 + s in the per-clip kernels, by the token elsewhere; ATTN rows
    (clip H + h) 64 + query per-clip, (clip H + h) S + query tiled, tok0 H + h S_b + query ragged; FEAT by the segment's own row."""

    def __init__(self, seed: int, batch: Batch, L: int, p: float, p_pos: float = 0.0, p_feat: float = 0.0):
        self.seed, self.b, self.L, self.p, self.p_pos, self.p_feat = seed, batch, L, p, p_pos, p_feat
        self.s = dm.inv_keep(p) if p > 0 else 1.0
        self.s_pos = dm.inv_keep(p_pos) if p_pos > 0 else 1.0
        self.s_feat = dm.inv_keep(p_feat) if p_feat > 0 else 1.0

    def _keep(self, layer, site, rows, ncol, p):
        if p <= 0:
            return torch.ones(len(rows), ncol, dtype=torch.bool)
        return dm.keep_scale(dm.site_key(self.seed, layer, site), np.asarray(rows, dtype=np.int64), np.arange(ncol, dtype=np.int64), p) > 0

    def pos(self):
        return self._keep(0, dm.SITE_POS, np.arange(self.b.N), self.b.d, self.p_pos)

    def feat(self, k):
        return self._keep(k, dm.SITE_FEAT, np.arange(len(self.b.seg_tok[k])), self.b.d, self.p_feat)

    def res(self, l, which):
        return self._keep(l, dm.SITE_RES1 if which == 1 else dm.SITE_RES2, np.arange(self.b.N), self.b.d, self.p)

    def ffn(self, l, by_token=False):
        b = self.b
        rows = np.concatenate([c * 64 + np.arange(S) for c, S in enumerate(b.lens)]) if (b.family == "perclip" and not by_token) else np.arange(b.N)
        return self._keep(l, dm.SITE_FFN, rows, b.dff, self.p)

    def attn(self, l, c, stride_S=False):
        """(H, S_c, S_c) keep decisions of clip c."""
        b = self.b
        S, H = b.lens[c], b.H
        h, q = np.arange(H)[:, None], np.arange(S)[None, :]
        if b.family == "perclip" and not stride_S:
            rows = (c * H + h) * 64 + q
        elif b.family == "tiled":
            rows = (c * H + h) * S + q
        else:
            rows = b.tok0[c] * H + h * S + q
        return self._keep(l, dm.SITE_ATTN, rows.reshape(-1), S, self.p).reshape(H, S, S)


# ---- the stages --------------------------------------------------------------------------------------------------------------------------------
def layer_norm(x, w, b, perturb=None):
    mean = x.mean(-1, keepdim=True)
    n = x.shape[-1] - (1 if perturb == "ln_var_dm1" else 0)
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / n
    return (x - mean) / torch.sqrt(var + LN_EPS) * w + b


def gemm_nt(x, w, b, mode, round_x=True):
    """r(x) r(w)^T + b -> (value, absolute-value product)."""
    xr, wr = (rnd(x, mode) if round_x else x), rnd(w, mode)
    v, s = xr @ wr.T, xr.abs() @ wr.abs().T
    return (v, s) if b is None else (v + b, s + b.abs())


def wgrad(G, X, mode, perturb=None, round_g=True, round_x=True):
    """dW = r(G)^T r(X) over the token rows -> (value, absolute-value product)."""
    Gr = G if (not round_g or perturb == "wgrad_g_unrounded") else rnd(G, mode)
    Xr = X if (not round_x or perturb == "wgrad_x_unrounded") else rnd(X, mode)
    return Gr.T @ Xr, Gr.abs().T @ Xr.abs()


def colsum(G):
    return G.sum(0), G.abs().sum(0)


def _heads(t, S, H):
    return t.reshape(S, H, -1).permute(1, 0, 2)        # (H, S, dh)


def _unheads(t):
    H, S, dh = t.shape
    return t.permute(1, 0, 2).reshape(S, H * dh)


# ---- roundings INSIDE a stage: rounding flips, and what they may cost -------------------------------------------------------------------------
# A value that is rounded inside a stage (P, dS, dO, the attention output in front of the out-projection) is itself a computed number: the
# device's fp32 value and the reference's fp64 value differ by some fp32 error, and where that straddles a bf16 rounding boundary the two
# round to NEIGHBOURING values, one bf16 ulp apart. Such a flip is correct arithmetic on both sides, but under a max-metric one flip sets
# the stage's error to ~1e-3, the size of the mistakes the gate is for (measured without this: 2.7e-4 .. 2.5e-3 on the attention stages).
# So every in-stage rounding goes through rnd_track(): an element closer to a rounding boundary than the error its value can carry (AMB x
# its absolute-value scale, plus whatever earlier flips can move it) is AMBIGUOUS, and one ulp of it is carried forward as an ALLOWANCE
# through the same absolute-value products as the scale. The comparison takes the allowance of an output element off its difference
# before the metric sees it; an element without an allowance is held to the full bar.
# How much this gives away (AMB_SHARE, measured): in the forward 2 - 3 % of the rounded values are ambiguous. In the backward the first
# rounding is dO = g1 W_o, a 128-term product with cancellation (|g1||W_o| ~ 10 |dO|): ~1.5 % of its elements are ambiguous, and one such
# element can move dP of its whole (token, head) score row by 2^-8 |dO||V|, enough to flip a third of that row's dS: 37 - 45 % of the
# backward's rounded values carry an allowance (of ONE ulp of the flipped operand, through the products: ~1e-3 of the element's scale).
# The other elements, and every element against a mistake larger than that, are held sharply: leaving out the dS or the P rounding, which
# moves every element by up to half an ulp, misses the bars by 80x and 700x (PERTURB_RATIO).
# AMB is not fitted to anything: it is the worst-case relative error n 2^-24 of an fp32 accumulation of n = 64 exact products (the
# kernels' dot products have 32 .. 128 terms), about 2.5 x the bars of the GEMM stages.
AMB = 4e-6


AMB_STATS: Dict[str, list] = {}     # stage -> [elements that got an allowance, non-zero elements rounded inside the stage] since the last clear()
_AMB_STAGE = ["-"]


def bf16_ulp(t):
    """One bf16 ulp (8 significant bits) at every element of t, 0 at 0."""
    _, ex = torch.frexp(t.detach().abs().to(F64))
    return torch.where(t == 0, torch.zeros_like(t, dtype=F64), torch.ldexp(torch.ones_like(t, dtype=F64), ex - 8)).to(t.dtype)


def rnd_track(t, mode, err_abs, upstream=None):
    """-> (r(t), allowance): allowance = upstream + one ulp where t lies within err_abs + upstream of a rounding boundary (bf16 mode)."""
    up = torch.zeros_like(t) if upstream is None else upstream
    if mode != "bf16":
        return t, up
    ulp = bf16_ulp(t)
    safe = ulp.clamp(min=1e-300)
    frac = (t.abs() / safe) % 1.0
    dist = (frac - 0.5).abs() * ulp                     # distance to the nearest midpoint between two bf16 values
    amb = (dist <= err_abs + up) & (ulp > 0)
    st = AMB_STATS.setdefault(_AMB_STAGE[0], [0, 0])     # (audit: test_cpu_bf16_stages.py holds the share of ambiguous elements down)
    st[0] += int(amb.sum().item())
    st[1] += int((ulp > 0).sum().item())
    return bf16r(t), up + torch.where(amb, ulp, torch.zeros_like(ulp))


def _softmax_tracked(q, k, scale):
    """P = softmax(q k^T scale) and the absolute error its elements can carry: P (AMB (1 + |q||k| scale))."""
    sc = (q @ k.transpose(-1, -2)) * scale
    sabs = (q.abs() @ k.abs().transpose(-1, -2)) * scale
    p = torch.softmax(sc, -1)
    return p, p * (AMB * (1.0 + sabs))


def attn_perclip_fwd(qkv, keep, s_keep, H, mode, perturb=None):
    """One clip of the per-clip kernels: qkv (S, 3d), keep (H, S, S) -> (O (S, d), its absolute-value product, its flip allowance)."""
    S, d = qkv.shape[0], qkv.shape[1] // 3
    q, k, v = (_heads(rnd(qkv[:, i * d:(i + 1) * d], mode), S, H) for i in range(3))
    p, perr = _softmax_tracked(q, k, 1.0 / math.sqrt(d // H))
    ks = keep.to(p.dtype) * s_keep
    if perturb == "p_unrounded":
        pd, al = p * ks, torch.zeros_like(p)
    else:
        pd, al = rnd_track(p * ks, mode, perr * ks)
    return _unheads(pd @ v), _unheads(pd.abs() @ v.abs()), _unheads(al @ v.abs())


def attn_tiled_fwd(qkv, keep, s_keep, H, mode):
    """One clip of tiled_attn_fwd_planes_kernel -> (O (S, d), its absolute-value product, its flip allowance, lse2 (H, S) in log2 units)."""
    S, d = qkv.shape[0], qkv.shape[1] // 3
    q = _heads(rnd_scaled(qkv[:, :d], TA_C2, mode), S, H)
    k = _heads(rnd(qkv[:, d:2 * d], mode), S, H)
    v = _heads(rnd_scaled(qkv[:, 2 * d:], s_keep, mode), S, H)
    sc = q @ k.transpose(-1, -2)                                    # (H, S queries, S keys), log2 units
    sabs = q.abs() @ k.abs().transpose(-1, -2)
    nb = (S + 31) // 32
    npad = nb * 32 - S

    def blocks(t, fill):
        return torch.cat([t, torch.full((H, S, npad), fill, dtype=t.dtype)], -1).reshape(H, S, nb, 32)
    blk = blocks(sc, -math.inf)
    m_run = torch.cummax(blk.amax(-1), -1).values                   # running maximum behind every 32-key block
    m_fin = m_run[..., -1:]
    p = torch.exp2(blk - m_run[..., None])                          # relative to the RUNNING maximum, as rounded
    l = torch.exp2(blk - m_fin[..., None]).sum((-1, -2))
    kp = blocks(keep, False).to(p.dtype)
    pk, al = rnd_track(p * kp, mode, p * kp * (AMB * (1.0 + blocks(sabs, 0.0))))
    corr = torch.exp2(m_run - m_fin)[..., None]                     # the fp32 rescaling of the running sums
    pk, al = (pk * corr).reshape(H, S, nb * 32)[..., :S], (al * corr).reshape(H, S, nb * 32)[..., :S]
    li = 1.0 / l[..., None]
    return _unheads((pk @ v) * li), _unheads((pk.abs() @ v.abs()) * li), _unheads((al @ v.abs()) * li), m_fin[..., 0] + torch.log2(l)


def attn_perclip_bwd(g1, qkv, out_w, keep, s_keep, H, mode, perturb=None):
    """One clip of the per-clip backward (P7 - P10): g1 (S, d), qkv (S, 3d) -> {"attn_o": (value, scale, allowance), "dqkv": ...}."""
    S, d = g1.shape
    scale = 1.0 / math.sqrt(d // H)
    gr, wr = rnd(g1, mode), rnd(out_w, mode)
    do_abs = gr.abs() @ wr.abs()
    dO, a_do = rnd_track(gr @ wr, mode, AMB * do_abs)               # dO = g1 W_o
    q, k, v = (_heads(rnd(qkv[:, i * d:(i + 1) * d], mode), S, H) for i in range(3))
    do, a_do, do_abs = _heads(dO, S, H), _heads(a_do, S, H), _heads(do_abs, S, H)
    p, perr = _softmax_tracked(q, k, scale)
    ks = keep.to(p.dtype) * s_keep
    T = lambda t: t.transpose(-1, -2)  # noqa: E731
    dp = do @ T(v)
    dpm = dp * ks
    dp_abs = (do_abs @ T(v.abs())) * ks                             # the absolute-value product behind dPm (dO itself is one: |g1| |W_o|)
    e_dpm = AMB * dp_abs + (a_do @ T(v.abs())) * ks                 # fp32 error + what a flipped dO moves
    delta = (p * (dp if perturb == "delta_without_dropout" else dpm)).sum(-1, keepdim=True)
    e_delta = (perr * dp_abs + p * e_dpm).sum(-1, keepdim=True)
    delta_abs = (p * dp_abs).sum(-1, keepdim=True)
    ds, a_ds = rnd_track(p * (dpm - delta) * scale, mode, (perr * (dp_abs + delta_abs) + p * (e_dpm + e_delta)) * scale)
    ds_abs = p * (dp_abs + delta_abs) * scale                       # |dS| before any of its cancellations
    pd, a_pd = rnd_track(p * ks, mode, perr * ks)
    out = {"attn_o": (pd @ v, pd.abs() @ v.abs(), a_pd @ v.abs())}
    dq = (ds @ k, ds_abs @ k.abs(), a_ds @ k.abs())
    dk = (T(ds) @ q, T(ds_abs) @ q.abs(), T(a_ds) @ q.abs())
    dv = (T(pd) @ do, T(pd.abs()) @ do_abs, T(a_pd) @ do.abs() + T(pd.abs()) @ a_do)
    out["attn_o"] = tuple(_unheads(t) for t in out["attn_o"])
    out["dqkv"] = tuple(torch.cat([_unheads(x[i]) for x in (dq, dk, dv)], 1) for i in range(3))
    return out


def attn_tiled_bwd(g1, qkv, o, lse2, out_w, keep, s_keep, H, mode, perturb=None):
    """One clip of the tiled / ragged attention backward (fused_bwd.hip P7 + tiled_attn_dq_planes_kernel + tiled_attn_dkv_planes_kernel):
    g1 (S, d), qkv (S, 3d), o = the saved attention output (S, d), lse2 (H, S) the saved log-sum-exp in log2 units
    -> (dqkv (S, 3d), its absolute-value product, its flip allowance)."""
    S, d = g1.shape
    TA_SCALE = float(np.float32(0.17677669529663687))
    T = lambda t: t.transpose(-1, -2)  # noqa: E731
    gr, wr = rnd(g1, mode), rnd(out_w, mode)
    dO, do_abs = gr @ wr, gr.abs() @ wr.abs()                       # d(attention output), dense fp32 between the launches
    e_do = AMB * do_abs
    delta = _heads(dO * o, S, H).sum(-1, keepdim=True)              # rowsum(dO . O) on the UNROUNDED dO and the saved O, per head
    delta_abs = _heads(do_abs * o.abs(), S, H).sum(-1, keepdim=True)
    e_delta = AMB * delta_abs
    L = lse2[..., None]
    kp = keep.to(g1.dtype)
    q, k, v = qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:]
    if perturb == "tiled_q_scaled_after_rounding":
        qs = _heads(rnd(q, mode) * TA_C2, S, H)
    else:
        qs = _heads(rnd_scaled(q, TA_C2, mode), S, H)
    kr, qr, vr = _heads(rnd(k, mode), S, H), _heads(rnd(q, mode), S, H), _heads(rnd(v, mode), S, H)
    ks, vs = _heads(rnd_scaled(k, TA_C2, mode), S, H), _heads(rnd_scaled(v, s_keep, mode), S, H)
    do_abs_h = _heads(do_abs, S, H)
    # -- dQ pass: s = r(Q c2) r(K)^T, dP = r(dO) r(V / (1 - p))^T
    do1, a_do1 = rnd_track(dO, mode, e_do)
    do1, a_do1 = _heads(do1, S, H), _heads(a_do1, S, H)
    p1 = torch.exp2(qs @ T(kr) - L)
    e_p1 = p1 * (AMB * (1.0 + qs.abs() @ T(kr.abs())))
    dp1, dp1_abs = (do1 @ T(vs)) * kp, (do_abs_h @ T(vs.abs())) * kp
    e_dp1 = AMB * dp1_abs + (a_do1 @ T(vs.abs())) * kp
    ds1_abs = p1 * (dp1_abs + delta_abs)
    if perturb == "tiled_ds_unrounded":
        ds1, a_ds1 = p1 * (dp1 - delta), torch.zeros_like(p1)
    else:
        ds1, a_ds1 = rnd_track(p1 * (dp1 - delta), mode, e_p1 * (dp1_abs + delta_abs) + p1 * (e_dp1 + e_delta))
    dq = ((ds1 @ kr) * TA_SCALE, (ds1_abs @ kr.abs()) * TA_SCALE, (a_ds1 @ kr.abs()) * TA_SCALE)
    # -- dK / dV pass: s = r(Q) r(K c2)^T, dP = r(dO / (1 - p)) r(V)^T
    do2, a_do2 = rnd_track((dO.to(F32) * np.float32(s_keep)).to(dO.dtype), mode, e_do * s_keep)
    do2, a_do2 = _heads(do2, S, H), _heads(a_do2, S, H)
    p2 = torch.exp2(qr @ T(ks) - L)
    e_p2 = p2 * (AMB * (1.0 + qr.abs() @ T(ks.abs())))
    dp2, dp2_abs = (do2 @ T(vr)) * kp, (do_abs_h * s_keep) @ T(vr.abs()) * kp
    e_dp2 = AMB * dp2_abs + (a_do2 @ T(vr.abs())) * kp
    ds2_abs = p2 * (dp2_abs + delta_abs)
    ds2, a_ds2 = rnd_track(p2 * (dp2 - delta), mode, e_p2 * (dp2_abs + delta_abs) + p2 * (e_dp2 + e_delta))
    pn, a_pn = rnd_track(p2 * kp, mode, e_p2 * kp)
    dk = ((T(ds2) @ qr) * TA_SCALE, (T(ds2_abs) @ qr.abs()) * TA_SCALE, (T(a_ds2) @ qr.abs()) * TA_SCALE)
    dv = (T(pn) @ do2, T(pn.abs()) @ (do_abs_h * s_keep), T(a_pn) @ do2.abs() + T(pn.abs()) @ a_do2)
    return tuple(torch.cat([_unheads(x[i]) for x in (dq, dk, dv)], 1) for i in range(3))


def hidden(x1, w1, b1, keep, s, mode, perturb=None):
    """-> (relu(a) on the kept units BEFORE its rounding to bf16, a, absolute-value product): a = r(x1) r(s W1)^T + s b1."""
    if perturb == "h_rounded_before_scale":        # the keep-scale applied to the rounded H instead of riding on W1
        a, sa = gemm_nt(x1, w1, b1, mode)
        return rnd(torch.relu(a), mode) * keep.to(a.dtype) * s, a * s, sa * s
    xr, wr = rnd(x1, mode), rnd_scaled(w1, s, mode)
    bs = b1 if perturb == "bias_unscaled" else b1 * s
    a, sa = xr @ wr.T + bs, xr.abs() @ wr.abs().T + bs.abs()
    return torch.relu(a) * keep.to(a.dtype), a, sa


# ---- one call, stage by stage ------------------------------------------------------------------------------------------------------------------
@dataclass
class Out:
    """One output item of a stage. scale None: the per-row metric (row_err). stored_bf16: the device holds r(value) (X1, HID, DHID in bf16
    mode): `value` is the UNROUNDED reference and the comparison takes exactly one rounding (half a bf16 ulp of it) off the difference,
    which is sharper than elem_err's bf16_out (2^-8 |ref|). allow: the flip allowance (rnd_track), or None."""
    value: torch.Tensor
    scale: Optional[torch.Tensor] = None
    stored_bf16: bool = False
    allow: Optional[torch.Tensor] = None
    aux: Optional[torch.Tensor] = None        # ALIVE: the pre-activation


_MASK_CACHE: dict = {}


class Stages:
    """Every stage of one call. A stage function takes the items it starts from (in the dtype to compute in) and returns {output item:
    Out}. The same functions serve simulate() (chained in fp32: the CPU stand-in for the device) and stage_errors() (teacher-forced)."""

    def __init__(self, model: Model, batch: Batch, masks: Masks, feats: List[torch.Tensor], mode: str, perturb: Optional[str] = None):
        self.m, self.b, self.k, self.feats, self.mode, self.perturb = model, batch, masks, feats, mode, perturb
        self.L = len(model.layers)

    def mask(self, name, *a):
        kw = {}
        if name == "attn" and self.perturb == "attn_row_stride":
            kw = {"stride_S": True}
        if name == "ffn" and self.perturb == "ffn_mask_row_key":
            kw = {"by_token": True}
        k, b = self.k, self.b
        key = (k.seed, b.family, tuple(b.lens), b.H, b.dff, k.p, k.p_pos, k.p_feat, name, a, tuple(kw))
        if key not in _MASK_CACHE:      # (a function of the key alone; shared by the modes and the perturbed runs of a case)
            _MASK_CACHE[key] = getattr(k, name)(*a, **kw)
        return _MASK_CACHE[key]

    # -- forward
    def pre(self, it, dt):
        b, mode = self.b, self.mode
        val, sc = torch.zeros(b.N, b.d, dtype=dt), torch.zeros(b.N, b.d, dtype=dt)
        for k, (W, bias, _, _) in enumerate(self.m.proj):
            v, s = gemm_nt(self.feats[k].to(dt), W.to(dt), bias.to(dt), mode)
            fm = self.mask("feat", k).to(dt) * self.k.s_feat
            val[b.seg_tok[k]], sc[b.seg_tok[k]] = v * fm, s * fm
        return {"PRE": Out(val, sc)}

    def xin0(self, it, dt):
        m = self.m
        x = layer_norm(it["PRE"], m.ln[0].to(dt), m.ln[1].to(dt), self.perturb)
        if m.add_rows is not None:
            x = x + m.add_rows.to(dt)
        x = (x + m.pos_rows.to(dt)) * (self.mask("pos").to(dt) * self.k.s_pos)
        return {"XIN0": Out(x)}

    def qkv(self, l, it, dt):
        w = self.m.layers[l]
        v, s = gemm_nt(it[f"XIN{l}"], w["in_w"].to(dt), w["in_b"].to(dt), self.mode)
        return {f"QKV{l}": Out(v, s)}

    def _res1(self, l, o, so, ao, o_err, xin, dt):
        """(r(o) r(W_o)^T + b_o) x keep-scale + xin; o_err: the fp32 error o itself can carry (None: o is a held item, exact)."""
        w = self.m.layers[l]
        wr = rnd(w["out_w"].to(dt), self.mode)
        orr, ao = (rnd(o, self.mode), ao) if o_err is None else rnd_track(o, self.mode, o_err, ao)
        s_keep = 1.0 if self.perturb == "res1_wrong_keep_scale" else self.k.s
        m1 = self.mask("res", l, 1).to(dt) * s_keep
        bo = w["out_b"].to(dt)
        return Out((orr @ wr.T + bo) * m1 + xin, (so @ wr.abs().T + bo.abs()) * m1 + xin.abs(), False, None if ao is None else (ao @ wr.abs().T) * m1)

    def res1_perclip(self, l, it, dt):
        qkv, b = it[f"QKV{l}"], self.b
        o, so, ao = _cat([attn_perclip_fwd(qkv[sl], self.mask("attn", l, c), self.k.s, b.H, self.mode, self.perturb) for c, sl in _clips(b)])
        return {f"RES1{l}": self._res1(l, o, so, ao, AMB * so, it[f"XIN{l}"], dt)}

    def attn_tiled(self, l, it, dt):
        qkv, b = it[f"QKV{l}"], self.b
        outs = [attn_tiled_fwd(qkv[sl], self.mask("attn", l, c), self.k.s, b.H, self.mode) for c, sl in _clips(b)]
        o, so, ao = _cat([x[:3] for x in outs])
        lse = torch.cat([x[3].reshape(-1) for x in outs])[:, None]         # (clip, head, token of the clip)
        return {f"ATTN_O{l}": Out(o, so, False, ao), f"LSE{l}": Out(lse, lse.abs().clamp(min=1.0))}

    def res1_tiled(self, l, it, dt):
        o = it[f"ATTN_O{l}"]
        return {f"RES1{l}": self._res1(l, o, rnd(o, self.mode).abs(), None, None, it[f"XIN{l}"], dt)}

    def x1(self, l, it, dt):
        w = self.m.layers[l]
        return {f"X1{l}": Out(layer_norm(it[f"RES1{l}"], w["n1w"].to(dt), w["n1b"].to(dt), self.perturb), None, self.mode == "bf16")}

    def hid(self, l, it, dt):
        w = self.m.layers[l]
        keep = self.mask("ffn", l)
        h, a, sa = hidden(it[f"X1{l}"], w["w1"].to(dt), w["b1"].to(dt), keep, self.k.s, self.mode, self.perturb)
        return {f"HID{l}": Out(h, sa, self.mode == "bf16"), f"ALIVE{l}": Out((a >= 0) & keep, aux=a)}

    def res2(self, l, it, dt):
        w = self.m.layers[l]
        x1f = layer_norm(it[f"RES1{l}"], w["n1w"].to(dt), w["n1b"].to(dt))
        f, sf = gemm_nt(it[f"HID{l}"], w["w2"].to(dt), w["b2"].to(dt), self.mode, round_x=False)
        m2 = self.mask("res", l, 2).to(dt) * self.k.s
        # (the residual is a LayerNorm output: its error goes with the ROW's largest element, as in row_err, not with the element)
        return {f"RES2{l}": Out(f * m2 + x1f, sf * m2 + x1f.abs().amax(-1, keepdim=True))}

    def xin_next(self, l, it, dt):
        w = self.m.layers[l]
        y = layer_norm(it[f"RES2{l}"], w["n2w"].to(dt), w["n2b"].to(dt), self.perturb)
        if l + 1 < self.L:
            return {f"XIN{l + 1}": Out(y)}
        b, m = self.b, self.m
        if m.head is None:
            rows = torch.cat([torch.arange(t0, t0 + m.out_T) for t0 in b.tok0])
            return {"OUT": Out(y[rows])}
        pooled = torch.stack([y[sl].mean(0) for _, sl in _clips(b)])
        z = layer_norm(pooled, m.head[0].to(dt), m.head[1].to(dt))
        W, bias = m.head[2].to(dt), m.head[3].to(dt)
        return {"OUT": Out(z @ W.T + bias, z.abs() @ W.abs().T + bias.abs())}

    # -- backward
    def dhid(self, l, it, dt):
        w = self.m.layers[l]
        g, wr = rnd(it[f"G2{l}"], self.mode), rnd_scaled(w["w2"].to(dt), self.k.s, self.mode)
        alive = it[f"ALIVE{l}"].to(dt)
        return {f"DHID{l}": Out((g @ wr) * alive, (g.abs() @ wr.abs()) * alive, self.mode == "bf16")}

    def attn_bwd_perclip(self, l, it, dt):
        g1, qkv, b = it[f"G1{l}"], it[f"QKV{l}"], self.b
        w = self.m.layers[l]["out_w"].to(dt)
        outs = [attn_perclip_bwd(g1[sl], qkv[sl], w, self.mask("attn", l, c), self.k.s, b.H, self.mode, self.perturb) for c, sl in _clips(b)]
        o, so, ao = _cat([x["attn_o"] for x in outs])
        dq, sq, aq = _cat([x["dqkv"] for x in outs])
        return {f"ATTN_O{l}": Out(o, so, False, ao), f"DQKV{l}": Out(dq, sq, False, aq)}

    def attn_bwd_tiled(self, l, it, dt):
        g1, qkv, o, lse, b = it[f"G1{l}"], it[f"QKV{l}"], it[f"ATTN_O{l}"], it[f"LSE{l}"].reshape(-1), self.b
        w = self.m.layers[l]["out_w"].to(dt)
        outs = [attn_tiled_bwd(g1[sl], qkv[sl], o[sl], lse[b.H * sl.start:b.H * sl.stop].reshape(b.H, -1), w, self.mask("attn", l, c), self.k.s, b.H,
                               self.mode, self.perturb) for c, sl in _clips(b)]
        dq, sq, aq = _cat(outs)
        return {f"DQKV{l}": Out(dq, sq, False, aq)}

    def wgrads(self, l, it, dt):
        p, mode, pt = self.m.layer_prefix[l], self.mode, self.perturb
        out = {}

        def put(name, vs):
            out["grad:" + p + name] = Out(vs[0], vs[1])
        put(_LAYER_KEYS["in_w"], wgrad(it[f"DQKV{l}"], it[f"XIN{l}"], mode, pt))
        put(_LAYER_KEYS["in_b"], colsum(it[f"DQKV{l}"]))
        put(_LAYER_KEYS["out_w"], wgrad(it[f"G1{l}"], it[f"ATTN_O{l}"], mode, pt))
        put(_LAYER_KEYS["out_b"], colsum(it[f"G1{l}"]))
        dh, h, g2, x1 = it[f"DHID{l}"], it[f"HID{l}"], it[f"G2{l}"], it[f"X1{l}"]
        if pt == "dw1_drop_last_block":
            dh = dh.clone(); dh[:, -32:] = 0
        if pt == "dw2_drop_last_block":
            h = h.clone(); h[:, -32:] = 0
        # (the four FFN operands are held in the form the weight-gradient kernel multiplies: no further rounding in bf16 mode; f32s: exact)
        put(_LAYER_KEYS["w1"], wgrad(dh, x1, mode, None, round_g=False, round_x=False))
        put(_LAYER_KEYS["w2"], wgrad(g2, h, mode, None, round_g=False, round_x=False))
        dhb = it[f"DHID{l}"]
        if pt == "db1_without_alive":
            w = self.m.layers[l]
            dhb = rnd(rnd(g2, mode) @ rnd_scaled(w["w2"].to(dt), self.k.s, mode), mode)
        if pt == "colsum_counts_padded_row":        # one row too many in a column sum: the clip's last row twice
            dhb = torch.cat([dhb, dhb[-1:]], 0)
        put(_LAYER_KEYS["b1"], colsum(dhb))
        if mode != "bf16":      # (bf16: the column sum runs over the unrounded g2, which is not held)
            put(_LAYER_KEYS["b2"], colsum(g2))
        return out

    def proj_grads(self, it, dt):
        out = {}
        for k, (_, _, wn, bn) in enumerate(self.m.proj):
            v, s = wgrad(it[f"DSEG{k}"], self.feats[k].to(dt), self.mode, self.perturb)
            out["grad:" + wn] = Out(v, s)
            cs = colsum(it[f"DSEG{k}"])
            out["grad:" + bn] = Out(cs[0], cs[1])
        return out

    def plan(self):
        """[(stage name for the bars, function(items, dtype), input item names)] in execution order."""
        per = self.b.family == "perclip"
        P = [("pre", self.pre, []), ("xin0", self.xin0, ["PRE"])]
        for l in range(self.L):
            P.append(("qkv", _bind(self.qkv, l), [f"XIN{l}"]))
            if per:
                P.append(("res1_attn", _bind(self.res1_perclip, l), [f"QKV{l}", f"XIN{l}"]))
            else:
                P.append(("attn_tiled", _bind(self.attn_tiled, l), [f"QKV{l}"]))
                P.append(("res1", _bind(self.res1_tiled, l), [f"ATTN_O{l}", f"XIN{l}"]))
            P += [("x1", _bind(self.x1, l), [f"RES1{l}"]), ("hid", _bind(self.hid, l), [f"X1{l}"]),
                  ("res2", _bind(self.res2, l), [f"HID{l}", f"RES1{l}"]), ("ln2" if l + 1 < self.L else "out", _bind(self.xin_next, l), [f"RES2{l}"])]
        for l in range(self.L):
            P.append(("dhid", _bind(self.dhid, l), [f"G2{l}", f"ALIVE{l}"]))
            if per:
                P.append(("attn_bwd", _bind(self.attn_bwd_perclip, l), [f"G1{l}", f"QKV{l}"]))
            else:
                P.append(("attn_bwd_tiled", _bind(self.attn_bwd_tiled, l), [f"G1{l}", f"QKV{l}", f"ATTN_O{l}", f"LSE{l}"]))
            P.append(("wgrad", _bind(self.wgrads, l), [f"DQKV{l}", f"XIN{l}", f"G1{l}", f"ATTN_O{l}", f"DHID{l}", f"HID{l}", f"G2{l}", f"X1{l}"]))
        P.append(("wgrad", self.proj_grads, [f"DSEG{k}" for k in range(len(self.m.proj))]))
        return P


STAGE_NAMES = ("pre", "xin0", "qkv", "res1_attn", "attn_tiled", "res1", "x1", "hid", "res2", "ln2", "out", "dhid", "attn_bwd", "attn_bwd_tiled", "wgrad")


def _bind(fn, l):
    return lambda it, dt: fn(l, it, dt)


def _clips(b: Batch):
    return [(c, slice(b.tok0[c], b.tok0[c] + S)) for c, S in enumerate(b.lens)]


def _cat(tuples):
    return tuple(torch.cat([t[i] for t in tuples], 0) for i in range(len(tuples[0])))


def _stored(name, out: Out, mode):
    """An item as the device holds it: the bf16 items rounded, ALIVE as bits."""
    return bf16r(out.value) if (out.stored_bf16 and mode == "bf16") else out.value


def synthetic_grads(batch: Batch, masks: Masks, L: int, n_seg: int, mode: str, seed: int):
    """Upstream items of the backward stages for the CPU runs: G2, G1 behind their dropout masks (G2 as held: r(.) in bf16 mode), DSEG."""
    g = torch.Generator().manual_seed(seed)
    it = {}
    for l in range(L):
        g2 = torch.randn(batch.N, batch.d, generator=g) * 1e-2 * masks.res(l, 2) * masks.s
        it[f"G2{l}"] = bf16r(g2) if mode == "bf16" else g2
        it[f"G1{l}"] = torch.randn(batch.N, batch.d, generator=g) * 1e-2 * masks.res(l, 1) * masks.s
    for k in range(n_seg):
        it[f"DSEG{k}"] = torch.randn(len(batch.seg_tok[k]), batch.d, generator=g) * 1e-2
    return it


def simulate(st: Stages, extra: dict, dtype=F32):
    """The whole call chained in `dtype`, every item stored as the device stores it: the CPU stand-in for a device run."""
    items = dict(extra)
    for _, fn, _ in st.plan():
        for name, out in fn({k: (t if t.dtype == torch.bool else t.to(dtype)) for k, t in items.items()}, dtype).items():
            items[name] = _stored(name, out, st.mode)
    return items


def alive_check(alive_dev, alive_ref, a_ref):
    """-> (mismatches outside the margin, share of units left out, the units left out): ALIVE against the sign of the reference
    pre-activation; a byte that is neither 0 nor 1 (unwritten) is a mismatch."""
    rms = a_ref.double().pow(2).mean().sqrt()
    near = a_ref.double().abs() < ALIVE_MARGIN * rms
    dv = alive_dev.to(torch.uint8)
    bad = (((dv != alive_ref.to(torch.uint8)) & ~near) | (dv > 1)).sum().item()
    return bad, near.double().mean().item(), near


def item_err(got, out: Out, mode: str) -> float:
    """The error of one device-held item against its reference, as elem_err / row_err see it (tests/wide_ops_ref.py)."""
    ref = out.value.to(F64)
    got = got.to(F64).reshape(ref.shape)
    diff = (got - ref).abs()
    take = torch.zeros_like(ref)
    if out.stored_bf16 and mode == "bf16":
        take = take + 0.5 * bf16_ulp(ref)               # the one rounding the device-held item carries
    if out.allow is not None:
        take = take + out.allow.to(F64)
    # what is left of the difference once the stated rounding / flip allowance is taken off (a NaN or inf stays what it is)
    left = torch.where(torch.isfinite(diff), (diff - take).clamp(min=0), diff)
    moved = ref + left
    return row_err(moved, ref) if out.scale is None else elem_err(moved, ref, out.scale)


def stage_errors(st: Stages, dev: dict, dtype=F64):
    """Teacher-forced: every stage in `dtype` from the items `dev` holds, against the items `dev` holds behind it.
    -> ({stage: worst error}, {stage: [(item, error)]}, notes). An item `dev` lacks is listed in notes["missing"] (the hook reported it as not
    kept) and its stage is skipped; an unwritten (NaN) element is an infinite error."""
    worst: Dict[str, float] = {}
    detail: Dict[str, list] = {}
    notes = {"missing": [], "alive_bad": 0, "alive_skip": 0.0}
    for stage, fn, needs in st.plan():
        lack = [n for n in needs if n not in dev]
        if lack:
            notes["missing"] += [f"{stage}: {n}" for n in lack]
            continue
        inp = {n: (dev[n].detach().cpu() if dev[n].dtype in (torch.bool, torch.uint8) else dev[n].detach().cpu().to(dtype)) for n in needs}
        near = None
        _AMB_STAGE[0] = stage
        outs = fn(inp, dtype)
        _AMB_STAGE[0] = "-"
        for name in sorted(outs, key=lambda n: not n.startswith("ALIVE")):        # (ALIVE first: its margin applies to HID)
            out = outs[name]
            if name not in dev:
                notes["missing"].append(f"{stage}: {name}")
                continue
            got = dev[name].detach().cpu()
            if name.startswith("ALIVE"):
                bad, skip, near = alive_check(got, out.value, out.aux)
                notes["alive_bad"] += bad
                notes["alive_skip"] = max(notes["alive_skip"], skip)
                e = math.inf if bad else 0.0
            else:
                if name.startswith("HID") and near is not None:      # a unit within the margin of the kink may be alive on one side only
                    got = torch.where(near, out.value.to(got.dtype), got.reshape(out.value.shape))
                e = item_err(got, out, st.mode)
            worst[stage] = max(worst.get(stage, 0.0), e)
            detail.setdefault(stage, []).append((name, e))
    return worst, detail, notes


# ---- the case table --------------------------------------------------------------------------------------------------------------------------
# Built from tests/fp32_grade.py Case and its data helpers with compute="bf16"; the smallest shapes that still reach each code path.
def _cases():
    from tests.fp32_grade import CUT0, CUT1, Case
    pc = dict(family="perclip", kind="ttm3", compute="bf16", impl="fused", expect="fused")
    dr = dict(p=0.5, p_pos=0.1)
    out = []
    for tag, env in (("one", CUT0), ("cut", CUT1)):
        out += [Case(f"pc-t15-l2-p05-{tag}", B=5, T=15, L=2, env=env, seed=201, **dr, **pc),
                Case(f"pc-t15-l2-p0-{tag}", B=5, T=15, L=2, env=env, seed=202, **pc),
                Case(f"pc-s48-l1-{tag}", B=3, T=16, L=1, env=env, seed=203, **dr, **pc),
                Case(f"pc-s3-l3-{tag}", B=9, T=1, L=3, env=env, seed=204, **dr, **pc),
                Case(f"pc-s21-l2-{tag}", B=9, T=7, L=2, env=env, seed=205, **dr, **pc)]
    out += [Case("pc-det-cut-ce", B=5, T=15, L=2, env=CUT1, det=True, loss="ce_fused", seed=206, **dr, **pc),
            Case("pc-wcache-p01", B=5, T=15, L=2, p=0.1, p_pos=0.1, env=CUT0, wcache=True, seed=207, **pc),
            Case("sl-b2-x4", family="sliced", kind="ttm3", compute="bf16", B=2, impl="fused", slices=4, env=(("EGX_FFN_SLICES", 4),), seed=208, **dr),
            Case("asd-rows-b4", family="perclip", kind="asd", compute="bf16", B=4, L=2, p=0.1, p_pos=0.1, impl="fused", env=CUT0, loss="rows", seed=209),
            Case("hoi-pnr3-b2", family="hoi", kind="pnr3", compute="bf16", B=2, L=2, p=0.1, p_feat=0.2, impl="fused", env=CUT0, loss="lin", seed=210)]
    tl = dict(family="tiled", kind="ttm3", compute="bf16", L=2, expect="tiled", **dr)
    out += [Case("tl-s51", B=3, T=17, seed=211, **tl), Case("tl-s96", B=2, T=32, seed=212, **tl), Case("tl-s147", B=2, T=49, seed=213, **tl)]
    rt = dict(family="ragged_train", compute="bf16", expect="ragged", loss="ce_fused", **dr)
    out += [Case("rt-ttm3-l2", kind="ttm3", L=2, clips=((10, 10, 10), (16, 16, 16), (16, 16, 17), (32, 32, 33), (48, 1, 2)), seed=214, **rt),
            Case("rt-ttm2-l1", kind="ttm2", L=1, clips=((24, 24), (24, 25), (1, 150)), seed=215, **rt)]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
_FAMILY = {"perclip": "perclip", "sliced": "perclip", "hoi": "perclip", "tiled": "tiled", "ragged_train": "ragged"}


_PREPARED: dict = {}


def setup(case, mode: str, perturb: Optional[str] = None):
    """-> (Stages, state dict, data) of a case: weights and inputs from tests/fp32_grade.py prepare() (kept per case: they do not depend on
    the compute mode and nothing writes to them), masks from the case's seed."""
    from tests import fp32_grade as fg
    if case.id not in _PREPARED:
        sd, _, data = fg.prepare(case)
        _PREPARED[case.id] = (sd, data)
    sd, data = _PREPARED[case.id]
    fam = _FAMILY[case.family]
    H, dff = (8, 256) if case.kind == "pnr3" else (4, 2048)
    if fam == "ragged":
        seg_T = [list(t) for t in case.clips]
        feats = [torch.cat([c[k] for c in data["clips"]], 0) for k in range(len(seg_T[0]))]
    else:
        order = {"asd": [2, 0, 1]}.get(case.kind)
        fl = data["feats"] if order is None else [data["feats"][i] for i in order]
        seg_T = [[f.shape[1] for f in fl]] * case.B
        feats = [f.reshape(-1, f.shape[-1]) for f in fl]
    batch = Batch(fam, [sum(t) for t in seg_T], seg_T, H, 128, dff)
    model = build(case.kind, sd, case.L, batch)
    masks = Masks(data["seed"], batch, case.L, case.p, case.p_pos, case.p_feat)
    return Stages(model, batch, masks, feats, mode, perturb), sd, data
