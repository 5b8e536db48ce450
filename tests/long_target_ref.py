"""Gate of decode() over 9 .. 64 target tokens (DecoderMixin.egx_long_targets; egx_target_attention_fwd / _bwd of csrc/target_attn.hip): the
operator cases, the decoder cases, the masks the route draws and the bars. Shared by tests/test_cpu_long_target.py and
tests/test_gpu_long_target.py (-m gpu). Test infrastructure only; nothing here is imported by the product path.

It restates nothing: the fp64 references are tests/unit_ref.py small_attention / small_attention_grads (with attn_mask at row stride 64)
and oracle/translator_ref.py g_decode(masks=); keys and keep-scales come from tests/dropmask.py; the oracle run, the metric and the
decoder bars are those of tests/decoder_dropout_gate.py (the composed-f32 bars: logits 1e-3, gradients 1e-2).

Bars
    operator   LT_BAR[kind] = unit_ref.FACTOR * LT_FP32_ERR[kind]: the worst unit_ref.rel_err, over LT_ATTN_CASES, of the fp32 evaluation of
               the reference against its fp64 evaluation (kind "out": o; "grad": dq, dk, dv). tests/test_cpu_long_target.py measures it
               and holds the constant to what it measures (within 3x either way).
    decoder    decoder_dropout_gate.F32_BAR, unchanged.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace as NS
from typing import Dict, Tuple

import numpy as np
import torch
import torch.nn as nn

from tests import decoder_dropout_gate as ddg
from tests import dropmask as dm
from tests import unit_ref as ur
from tests.fp32_grade import kink_free
from tests.util import seeded_state_dict

LT_ROW_STRIDE = 64            # TA_MAXQ of csrc/target_attn.hip: the mask row of query i of (clip b, head h) is (b * H + h) * 64 + i
LT_MAXQ, LT_MAXK, LT_MAXDH = 64, 1024, 128
LT_GROUP, LT_CHUNK = 8, 64    # query rows per group, keys per LDS chunk

# (B, H, Sq, Sk, dh, causal, p_drop, layout): the tuple form and the layouts of unit_ref.ATTN_CASES
LT_ATTN_CASES = [
    (2, 4, 9, 9, 32, 1, 0.0, "self"),               # first row of the second query group
    (2, 4, 9, 9, 32, 1, 0.3, "self"),               # the same under dropout
    (1, 2, 16, 16, 64, 1, 0.3, "self"),             # exact groups
    (2, 2, 17, 17, 33, 1, 0.3, "odd"),              # group tail, odd head dim, unaligned rows
    (1, 2, 64, 64, 128, 1, 0.3, "self"),            # Sq limit and dh limit
    (3, 4, 9, 1, 32, 0, 0.0, "cross"),              # one key
    (3, 8, 21, 4, 64, 0, 0.3, "cross"),             # the LTA shape
    (2, 4, 10, 64, 64, 0, 0.3, "cross"),            # one full chunk
    (2, 4, 10, 65, 64, 0, 0.3, "cross_ldo4"),       # second chunk holds one key, padded output rows
    (1, 2, 33, 130, 32, 0, 0.3, "cross"),           # chunk and group tails together
    (1, 2, 64, 1024, 32, 0, 0.3, "cross"),          # both limits
    (1, 1, 12, 200, 1, 0, 0.0, "packed"),           # dh = 1
    (2, 4, 5, 5, 32, 1, 0.3, "self"),               # Sq <= 8 through the new entry point
]
LT_ATTN_SEED = 0x5EED1A77

# Measured by tests/test_cpu_long_target.py (test_fp32_reference_meets_the_operator_bar prints them with -s)
LT_FP32_ERR = {"out": 6.0e-7, "grad": 1.0e-6}
LT_BAR = {kind: ur.FACTOR * e for kind, e in LT_FP32_ERR.items()}
# Worst (smallest) error / bar of each perturbed reference over the cases it applies to, as test_perturbed_reference_misses_the_bar measures
LT_PERTURB_RATIO = {"mask_row_stride_8": 8.4e4, "causal_off_by_one": 1.15e5, "drop_last_key": 912.0, "group_boundary": 1.06e4}
PERTURBED_MIN = ddg.PERTURBED_MIN


def lt_case_id(case) -> str:
    return ur.attn_case_id(case)


def lt_site(case_index: int) -> int:
    """A site of the composed decoder's form 0x4000 + (l << 8) + k: layer l = case index, k = 1 (self) or 3 (cross)."""
    return 0x4000 + (case_index << 8) + (1 if LT_ATTN_CASES[case_index][5] else 3)


def lt_inputs(case_index: int):
    """-> fp32 q (B, Sq, d) scaled by 2 (a softmax that is not flat), k, v (B, Sk, d), d_o (B, Sq, d): unit_ref.attn_inputs' recipe."""
    B, H, Sq, Sk, dh, causal, p, layout = LT_ATTN_CASES[case_index]
    d = H * dh
    g = torch.Generator(device="cpu").manual_seed(7101 + case_index)
    q = torch.randn(B, Sq, d, generator=g) * 2
    k = torch.randn(B, Sk, d, generator=g)
    v = torch.randn(B, Sk, d, generator=g)
    d_o = torch.randn(B, Sq, d, generator=g)
    return q, k, v, d_o


def lt_mask(case_index: int, row_stride: int = LT_ROW_STRIDE, B=None):
    Bc, H, Sq, Sk, dh, causal, p, layout = LT_ATTN_CASES[case_index]
    return ur.attn_mask(LT_ATTN_SEED, lt_site(case_index), Bc if B is None else B, H, Sq, Sk, p, row_stride)


def lt_eval(case_index: int, dtype, perturb=None):
    """-> (o, (dq, dk, dv)) of the case in `dtype`. perturb: None | "mask_row_stride_8" | "causal_off_by_one" | "drop_last_key" (unit_ref's) |
    "group_boundary" (query row 8, the first of the second group, given row 7's probabilities: its output is row 7's)."""
    B, H, Sq, Sk, dh, causal, p, _ = LT_ATTN_CASES[case_index]
    q, k, v, d_o = [t.to(dtype) for t in lt_inputs(case_index)]
    mask = lt_mask(case_index, ur.SA_ROW_STRIDE if perturb == "mask_row_stride_8" else LT_ROW_STRIDE)
    if perturb == "group_boundary":
        q, k, v = [t.detach().clone().requires_grad_(True) for t in (q, k, v)]
        o = ur.small_attention(q, k, v, H, causal, mask)
        o = torch.cat((o[:, :LT_GROUP], o[:, LT_GROUP - 1:LT_GROUP], o[:, LT_GROUP + 1:]), dim=1)
        o.backward(d_o)
        return o.detach(), (q.grad, k.grad, v.grad)
    o, dq, dk, dv = ur.small_attention_grads(q, k, v, d_o, H, causal, mask, None if perturb == "mask_row_stride_8" else perturb)
    return o, (dq, dk, dv)


LT_PERTURB_APPLIES = {        # the cases a mistake can show in
    "mask_row_stride_8": lambda c: c[6] > 0 and c[0] * c[1] > 1,      # (one (clip, head): block 0's rows are i at either stride)
    "causal_off_by_one": lambda c: c[5] == 1,
    "drop_last_key": lambda c: c[3] > 1,
    "group_boundary": lambda c: c[2] > LT_GROUP and c[3] > 1,         # (one key: every probability is 1, row 7's too)
}


# ---- the masks of the route --------------------------------------------------------------------------------------------------------------
def long_decoder_masks(seed: int, B: int, sy: int, S: int, d: int, H: int, d_ff: int, L: int, p_drop: float, p_pos: float,
                       row_stride: int = LT_ROW_STRIDE):
    """The keep-scales a train-mode decode() of the composed decoder over `sy` target tokens draws with host seed `seed`, in g_decode's
    `masks` layout: every site as dropmask._decoder_masks keys the composed implementation, except the rows of the two attention sites,
    (b * H + h) * row_stride + i (64: egx_target_attention_*; 8 reproduces dropmask.decoder_masks)."""
    masks = dm._decoder_masks(seed, "composed", range(B), H, sy, S, d, d_ff, L, p_drop, p_pos)
    b, h, i = np.arange(B, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(sy, dtype=np.int64)
    rows = (b[:, None, None] * H + h[None, :, None]) * row_stride + i[None, None, :]
    for l, layer in enumerate(masks["layers"]):
        for name, cols in (("self", i), ("cross", np.arange(S, dtype=np.int64))):
            layer[name] = dm.keep_scale(dm.site_key(seed, dm.DEC_KEY_LAYER0 + l, dm._DEC_SITE_ID[name]), rows, cols, p_drop)
    return masks


# ---- the decoder cases -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class LCase:
    id: str
    d: int
    H: int
    d_ff: int
    L: int
    V: int
    B: int
    sy: int
    S: int
    p_drop: float
    p_pos: float
    seed: int
    lengths: Tuple[int, ...] = ()       # (decoder_dropout_gate's helpers read it: uniform memories only)

    @property
    def bars(self) -> dict:
        return dict(ddg.F32_BAR)

    @property
    def host_seed(self) -> int:
        return ddg.HOST_SEED + self.seed


_M256, _LTA, _DH128 = (256, 8, 256, 2, 37), (512, 8, 512, 1, 600), (256, 2, 256, 1, 37)
LT_DECODER_CASES = (
    LCase("d256-sy9", *_M256, 3, 9, 4, 0.3, 0.1, 201),
    LCase("d256-sy21", *_M256, 2, 21, 4, 0.3, 0.1, 202),
    LCase("d256-sy64-s65", *_M256, 1, 64, 65, 0.3, 0.3, 203),
    LCase("d256-sy21-p0", *_M256, 2, 21, 4, 0.0, 0.0, 204),
    LCase("lta-widths", *_LTA, 2, 21, 4, 0.3, 0.1, 205),
    LCase("head-dim-128", *_DH128, 2, 12, 48, 0.3, 0.0, 206),
)
LT_BY_ID = {c.id: c for c in LT_DECODER_CASES}
LTA_CASE = LT_BY_ID["lta-widths"]


def new_model(case: LCase, p_drop=None):
    """The reference's action / LTA EgoT2-g class at the case's widths, on the CPU: its decoder rebuilt with the case's d_ff (the class
    builds nn.TransformerDecoderLayer's default 2048) and its encoder, which no test here runs, cut to one narrow layer."""
    from egot2_amd import hoi_multitask as hm
    p = case.p_drop if p_drop is None else p_drop
    vocab = {f"w{i}": i for i in range(case.V)}
    m = hm.TaskTranslationPromptTransformerActionTask(NS(hidden_dim=case.d, num_heads=case.H, num_layers=case.L, dropout=p), vocab, v_idx=[0], n_idx=[0])
    layer = hm.CustomDecoderLayer(d_model=case.d, nhead=case.H, dropout=p)
    layer.linear1, layer.linear2 = nn.Linear(case.d, case.d_ff), nn.Linear(case.d_ff, case.d)
    m.transformer_decoder = nn.TransformerDecoder(layer, num_layers=case.L)
    m.transformer_encoder = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=case.d, nhead=case.H, dim_feedforward=8, dropout=p), num_layers=1)
    m.pos_embed.dropout.p = case.p_pos
    return m


def case_masks(case: LCase, seed: int, row_stride: int = LT_ROW_STRIDE):
    return long_decoder_masks(seed, case.B, case.sy, case.S, case.d, case.H, case.d_ff, case.L, case.p_drop, case.p_pos, row_stride)


_DATA: Dict[str, dict] = {}


def case_data(case: LCase) -> dict:
    """decoder_dropout_gate.case_data for an LCase (that one draws its masks through dropmask.decoder_masks, which refuses sy > 8): "sd",
    "dsd", "mem" (S, B, d), "y" (B, sy), "w" (sy, B, V), "masks", "margins"; the embedding scaled by EMB_SCALE and every linear1.bias
    re-chosen kink-free under the case's own masks, for that function's reasons. Computed once per case and left unchanged."""
    if case.id in _DATA:
        return _DATA[case.id]
    m = new_model(case)
    sd = seeded_state_dict(m, 400 + case.seed)
    sd["embedding.weight"] = sd["embedding.weight"] * ddg.EMB_SCALE
    rng = np.random.default_rng(7000 + case.seed)
    data = {"sd": sd, "dsd": {k: v for k, v in sd.items() if ddg.is_decoder_param(k) or k == "pos_embed.pe"},
            "mem": torch.from_numpy(rng.standard_normal((case.S, case.B, case.d), dtype=np.float32)),
            "y": torch.from_numpy(rng.integers(0, case.V, (case.B, case.sy))).long(),
            "w": torch.from_numpy(rng.standard_normal((case.sy, case.B, case.V), dtype=np.float32))}
    data["masks"] = case_masks(case, case.host_seed)
    data["dsd"], data["margins"] = kink_free(data["dsd"], lambda sd64: ddg._forward(case, data, sd64, data["masks"], torch.float64), case.L,
                                             "transformer_decoder.")
    sd.update(data["dsd"])
    _DATA[case.id] = data
    return data


_REF: Dict[str, dict] = {}


def reference(case: LCase) -> dict:
    """The fp64 oracle run of the case under its own masks ({"logits", "dmem", "grads"}), computed once."""
    if case.id not in _REF:
        _REF[case.id] = ddg.oracle_run(case, case_data(case))
    return _REF[case.id]
