"""fp64 references of the encoder's self-attention weights for the tests (no GPU, no reference tree): the gate of
tests/test_cpu_enc_attn.py and tests/test_gpu_enc_attn.py.
  * the head-averaged weights nn.MultiheadAttention gives an nn.TransformerEncoderLayer's self_attn with need_weights=True, from the
    layer's input through in_proj (tests/attn_ref.softmax_weights), layer by layer through oracle.translator_ref.encoder_layer on the
    tokens hhi_tokens / hoi_tokens prepare;
  * their per-segment sums and the attention rollout R_l = ((w_l + I) / 2) R_{l-1};
  * the cases, input makers and bars of the GPU tests, and the perturbed references every bar has to reject.
Bars (none measured on the code under test):
  kernel level (primitive, rollout, a call's own Q | K | V): 2e-6, the bar of the cross-attention primitive (tests/test_gpu_attn_weights.py
  item 1, the same formula), on the condition that stock fp32 torch on the CPU stays below bar / 8 on the same case (the project's 8 x
  yardstick rule; tests/test_cpu_enc_attn.py checks it);
  model level: e = max |w - w*| < s / 4 with s = max |w* - 1 / S| (an answer that ignores the scores fails); f32 / f32s paths also
  e < 8 x the error of this oracle run in fp32; the cases are sharpened (sharpen_self) so that s >= 0.02, and the oracle with bf16-rounded
  in_proj weights and layer inputs keeps e < s / 16: the bf16 paths have a 4 x margin by construction."""
import math
from types import SimpleNamespace as NS

import torch

from oracle import translator_ref as tr
from tests import attn_ref as ar
from tests.util import hhi_args, seeded_feats, seeded_state_dict

BAR_KERNEL = 2e-6
YARDSTICK = BAR_KERNEL / 8
S_MIN = 0.02


# ---- weights, segment sums, rollout ----
def weights_from_input(x: torch.Tensor, in_w: torch.Tensor, in_b: torch.Tensor, n_heads: int, scale: bool = True) -> torch.Tensor:
    """x (B, S, d), the layer's input -> (B, S, S) in x's dtype."""
    d = x.shape[-1]
    q, k = tr.linear(x, in_w[:d], in_b[:d]), tr.linear(x, in_w[d:2 * d], in_b[d:2 * d])
    if not scale:       # (a perturbation: no 1 / sqrt(dh))
        q = q * math.sqrt(d // n_heads)
    return ar.softmax_weights(q, k, n_heads)


def encoder_weights(sd, prefix: str, x: torch.Tensor, n_heads: int, round_bf16: bool = False):
    """The layer loop: x (B, S, d) tokens -> (weights (L, B, S, S), inputs of every layer). round_bf16: in_proj weights and layer inputs
    rounded to bf16 before the scores (what a bf16 path holds at best)."""
    ws, xs = [], []
    for i in range(tr.n_layers_of(sd, prefix)):
        p = f"{prefix}layers.{i}."
        in_w, in_b, xi = sd[p + "self_attn.in_proj_weight"], sd[p + "self_attn.in_proj_bias"], x
        if round_bf16:
            in_w, xi = in_w.bfloat16().to(x.dtype), x.bfloat16().to(x.dtype)
        xs.append(x)
        ws.append(weights_from_input(xi, in_w, in_b, n_heads))
        x = tr.encoder_layer(x, sd, p, n_heads)
    return torch.stack(ws, 0), xs


def segment_sums(w: torch.Tensor, table) -> torch.Tensor:
    """w (..., B, S, S), table (B, K) per-clip segment lengths -> (..., B, S, K)"""
    table = torch.as_tensor(table)
    B, K = table.shape
    out = torch.zeros(w.shape[:-1] + (K,), dtype=w.dtype)
    for b in range(B):
        off = 0
        for t in range(K):
            n = int(table[b, t])
            out[..., b, :, t] = w[..., b, :, off:off + n].sum(-1)
            off += n
    return out


def rollout(w: torch.Tensor, lengths=None, identity: bool = True, reverse: bool = False) -> torch.Tensor:
    """w (L, B, S, S) -> (B, S, S): R_l = ((w_l + I) / 2) R_{l-1}, R_0 = I, over each clip's own tokens (zeros beyond). identity=False and
    reverse=True are the perturbations (no identity term; multiplied in the reverse order)."""
    L, B, S, _ = w.shape
    out = torch.zeros(B, S, S, dtype=w.dtype)
    for b in range(B):
        n = S if lengths is None else int(lengths[b])
        eye = torch.eye(n, dtype=w.dtype)
        R = eye.clone()
        for l in range(L):
            A = (w[l, b, :n, :n] + eye) / 2 if identity else w[l, b, :n, :n]
            R = R @ A if reverse else A @ R
        out[b, :n, :n] = R
    return out


# ---- item 1: the primitive ----
PRIM_SHAPES = [(4, 32), (8, 16), (4, 64), (8, 96), (2, 128)]
PRIM_S, PRIM_B = (1, 15, 16, 17, 45, 48, 49, 64, 65, 150), (1, 5)
RAGGED_LENGTHS = [0, 1, 17, 48, 49, 130]


def primitive_inputs(H: int, dh: int, S: int, B: int, rows: int = 0):
    """bf16-representable fp32 q and k (rows or B * S, H * dh): randn * 1.7 from a generator seeded by the shape."""
    g = torch.Generator().manual_seed(2000003 * H + 10007 * dh + 101 * S + B)
    n = rows or B * S
    q = (torch.randn(n, H * dh, generator=g) * 1.7).bfloat16().float()
    k = (torch.randn(n, H * dh, generator=g) * 1.7).bfloat16().float()
    return q, k


def primitive_cases(H: int, dh: int):
    for S in PRIM_S:
        for B in PRIM_B:
            yield S, B
    yield 512, 1


def primitive_segments(S: int):
    """A split with a one-token segment and a boundary that is no multiple of 16 (as far as S allows)."""
    if S == 1:
        return [1]
    if S < 4:
        return [1, S - 1]
    a = max(1, (S // 3) | 1)
    return [1, a, S - 1 - a]


# Cases whose fp32 yardstick (stock fp32 torch on the CPU against fp64, measured here, rounded up) is above bar / 8 = 2.5e-7: the case's
# bar is 8 x its yardstick. All of them are the two heads of 128 (the longest dot products) and the two-layer rollout of long clips.
YARDSTICK_ABOVE = {
    ("dense", 2, 128, 45, 5): 2.8e-7,       # bar 2.24e-6
    ("dense", 2, 128, 48, 5): 4.2e-7,       # bar 3.36e-6
    ("dense", 2, 128, 49, 5): 4.2e-7,       # bar 3.36e-6
    ("dense", 2, 128, 64, 5): 2.6e-7,       # bar 2.08e-6
    ("dense", 2, 128, 65, 5): 2.6e-7,       # bar 2.08e-6
    ("dense", 2, 128, 150, 1): 2.8e-7,      # bar 2.24e-6
    ("dense", 2, 128, 512, 1): 3.0e-7,      # bar 2.4e-6
    ("ragged", 2, 128): 2.8e-7,             # bar 2.24e-6
    ("rollout", 2, 130): 2.8e-7,            # bar 2.24e-6
    ("rollout", 2, 512): 6.3e-7,            # bar 5.04e-6
}


def kernel_bar(key) -> float:
    """The kernel-level bar of a case of items 1 and 2: 2e-6, or 8 x the case's listed yardstick."""
    return max(BAR_KERNEL, 8 * YARDSTICK_ABOVE.get(key, 0.0))


def ragged_layout(lengths, gap: int = 5, lead: int = 3):
    """First rows of clips of `lengths` tokens packed with `gap` unused rows between them, and the rows the buffer needs."""
    first, r = [], lead
    for n in lengths:
        first.append(r)
        r += n + gap
    return first, r + 8


def primitive_layout_cases(H: int, dh: int):
    """Every case of item 1: (key, q, k, B, S, first rows | None, lengths | None). Dense rows; the 48-row tile grid of the d = 128 kernels
    (clip c at row c * tpc * 48, unused rows between the clips); a ragged packed batch with an empty slot."""
    for S, B in primitive_cases(H, dh):
        q, k = primitive_inputs(H, dh, S, B)
        yield ("dense", H, dh, S, B), q, k, B, S, None, None
    for S in (45, 51):
        B, tpc = 5, (S + 47) // 48
        q, k = primitive_inputs(H, dh, S, B, rows=B * tpc * 48)
        yield ("grid", H, dh, S), q, k, B, S, [c * tpc * 48 for c in range(B)], [S] * B
    S, B = max(RAGGED_LENGTHS), len(RAGGED_LENGTHS)
    first, rows = ragged_layout(RAGGED_LENGTHS)
    q, k = primitive_inputs(H, dh, S, B, rows=rows)
    yield ("ragged", H, dh), q, k, B, S, first, list(RAGGED_LENGTHS)


def ref_weights(q, k, H: int, B: int, S: int, first=None, lengths=None, dtype=torch.float64) -> torch.Tensor:
    """(B, S, S): clip b's rows first[b] .. first[b] + lengths[b] of q and k (default b * S, S); zeros beyond its tokens."""
    ref = torch.zeros(B, S, S, dtype=dtype)
    for b in range(B):
        n = S if lengths is None else min(max(int(lengths[b]), 0), S)
        r0 = b * S if first is None else int(first[b])
        if n:
            ref[b, :n, :n] = ar.softmax_weights(q[r0:r0 + n][None].to(dtype), k[r0:r0 + n][None].to(dtype), H)[0]
    return ref


# ---- item 2: the rollout ----
ROLL_L, ROLL_S = (1, 2, 6), (1, 17, 48, 130, 512)


def rollout_cases():
    for L in ROLL_L:
        for S in ROLL_S:
            yield L, (1 if S == 512 else 3), S


def rollout_inputs(L: int, B: int, S: int) -> torch.Tensor:
    """Random row-stochastic fp32 (L, B, S, S): softmax of randn * 2."""
    g = torch.Generator().manual_seed(31 * L + 7 * B + S)
    return torch.softmax(torch.randn(L, B, S, S, generator=g) * 2.0, -1)


# ---- item 3: the models ----
def sharpen_self(sd, factor: float):
    """A copy of the state dict whose self-attention q and k projection rows (weights and biases) are scaled by `factor`
    (tests/attn_ref.sharpen for the encoder): sharper softmaxes, weights far from 1 / S."""
    out = dict(sd)
    for name, v in sd.items():
        if ".self_attn.in_proj_" in name:
            d = v.shape[0] // 3
            v = v.clone()
            v[:2 * d] *= factor
            out[name] = v
    return out


def _lta_cfg(n, d, heads, layers):
    return NS(FORECASTING=NS(NUM_INPUT_CLIPS=n, NUM_ACTIONS_TO_PREDICT=3),
              MODEL=NS(TRANSLATION_HEADS=heads, TRANSLATION_LAYERS=layers, TRANSLATION_INPUT_FEATURES=d, TRANSLATION_DROPOUT=0.0,
                       NUM_CLASSES=[5, 7], DROPOUT_RATE=0.0, HEAD_ACT="softmax"), TEST=NS(NO_ACT=False))


HHI_VOCAB = ar.HHI_VOCAB
# kind, layers, batch, frames per task (HHI) / clips per task (LTA), seeds, sharpening factor of the q / k projections
MODEL_CASES = {
    "ttm3_T15": dict(kind="ttm3", L=1, B=4, T=15, wseed=511, fseed=512, sharp=1.25),
    "ttm3_B1": dict(kind="ttm3", L=1, B=1, T=15, wseed=513, fseed=514, sharp=1.25),
    "ttm3_B3": dict(kind="ttm3", L=1, B=3, T=15, wseed=515, fseed=516, sharp=1.25),
    "pnr3_L6": dict(kind="pnr3", L=6, B=2, T=0, wseed=517, fseed=518, sharp=1.25),
    "asd_L2": dict(kind="asd", L=2, B=3, T=15, wseed=519, fseed=520, sharp=1.25),
    "ttm3_T17": dict(kind="ttm3", L=2, B=2, T=17, wseed=521, fseed=522, sharp=1.25),
    "ttm3_T50": dict(kind="ttm3", L=1, B=2, T=50, wseed=523, fseed=524, sharp=1.25),
    "lta4_d256": dict(kind="lta4", L=2, B=3, T=4, d=256, h=8, wseed=525, fseed=526, sharp=1.25),
    "lta4_d768": dict(kind="lta4", L=1, B=2, T=2, d=768, h=8, wseed=527, fseed=528, sharp=1.25),
    "hhi_g": dict(kind="hhi_g", L=2, B=3, T=15, d=256, h=4, wseed=529, fseed=530, sharp=1.25),
}


# the recordings of tests/golden/make_golden_encattn.py (live/enc_attn_ref.npz): the REAL classes at the sizes and seeds of their fixtures
# (tests/golden/make_golden.py), unsharpened; every array is regenerated from the seeds
RECORDINGS = {
    "rec_ttm3": dict(kind="ttm3", L=1, B=4, T=15, wseed=11, fseed=12, sharp=1.0),
    "rec_asd": dict(kind="asd", L=2, B=3, T=15, wseed=41, fseed=42, sharp=1.0),
    "rec_pnr3": dict(kind="pnr3", L=2, B=2, T=0, wseed=71, fseed=72, sharp=1.0),
    "rec_lta4": dict(kind="lta4", L=2, B=3, T=4, F=3, d=256, h=8, wseed=61, fseed=62, sharp=1.0),
}
ALL_CASES = {**MODEL_CASES, **RECORDINGS}


def new_model(c):
    """The case's model on the CPU (sharpened seeded weights) and its fp64 state dict."""
    from egot2_amd import hhi_asd, hhi_multitask, hhi_ttm, hoi_lta, hoi_pnr
    kind = c["kind"]
    if kind == "ttm3":
        m = hhi_ttm.TaskFusionMFTransformer3Task(hhi_args(num_layers=c["L"]))
    elif kind == "asd":
        m = hhi_asd.TaskFusionMFTransformer3Task(hhi_args(num_layers=c["L"]))
    elif kind == "pnr3":
        m = hoi_pnr.TaskFusionMFTransformer3TaskDropout(NS(DATA=NS(TASK="state_change_detection"), MODEL=NS(
            TRANSLATION_INPUT_FEATURES=128, TRANSLATION_LAYERS=c["L"], FEAT_DROPOUT_RATE=0.0, TRANSFORMER_DROPOUT_RATE=0.0)))
    elif kind == "lta4":
        m = hoi_lta.TaskFusionMFTransformerLTA4Task(_lta_cfg(c["T"], c["d"], c["h"], c["L"]))
    else:
        m = hhi_multitask.TaskTranslationPromptTransformer(NS(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"], dropout=0.0,
                                                              lam_checkpoint=None, ttm_checkpoint=None, asd_checkpoint=None), HHI_VOCAB)
    # through load_state_dict and back: modules that appear under two names (the HOI heads start with the shared `ln`) end up with ONE
    # value, exactly as in the reference (tests/test_oracle_golden.py)
    m.load_state_dict(sharpen_self(seeded_state_dict(m, c["wseed"]), c["sharp"]))
    return m.eval(), {k: v.detach().clone().double() for k, v in m.state_dict().items()}


def case_feats(c):
    """Features (fp32; the lta4 recording's frame means fp64) in the argument order of the model's forward_features / encode_features."""
    B, T, kind = c["B"], c["T"], c["kind"]
    if kind == "pnr3":
        shapes = [(B, 16, 8192), (B, 16, 8192), (B, 8, 2048), (B, 8, 256)]
    elif kind == "lta4" and "F" in c:       # the fixture's raw inputs: PNR frames (the reference averages them), the OSCC stream their
        frames, action, lta = seeded_feats(c["fseed"], [(B, T, c["F"], 8192), (B, T, c["d"]), (B, T, 2048)])      # channel-reversed copy
        frames = frames.double()        # (the real class is recorded in fp64: the frame means too; the device gets them rounded to fp32)
        return [frames.mean(2), frames.flip(-1).mean(2), action, lta]
    elif kind == "lta4":
        shapes = [(B, T, 8192), (B, T, 8192), (B, T, c["d"]), (B, T, 2048)]
    else:
        shapes = [(B, T, 256)] * 3
    return seeded_feats(c["fseed"], shapes)


def case_tokens(c, sd, feats):
    """-> (tokens (B, S, d) in sd's dtype, encoder prefix, heads, the segments' lengths in TOKEN order) as the model prepares them."""
    kind = c["kind"]
    f = [x.to(next(iter(sd.values())).dtype) if x.is_floating_point() else x for x in feats]
    if kind == "ttm3":
        return tr.hhi_tokens(sd, f, ["ttm", "lam", "asd"], [0, 1, 2]), "transformer_encoder.", 4, [x.shape[1] for x in f]
    if kind == "asd":       # arguments (ttm, lam, asd); tokens asd | ttm | lam
        return tr.hhi_tokens(sd, [f[2], f[0], f[1]], ["asd", "ttm", "lam"], [2, 0, 1]), "transformer_encoder.", 4, [f[2].shape[1], f[0].shape[1], f[1].shape[1]]
    if kind == "pnr3":
        return tr.hoi_tokens(sd, f, ["proj1", "proj2", "proj3_slow", "proj3_fast"]), "transformer.", 8, [x.shape[1] for x in f]
    if kind == "lta4":
        return tr.hoi_tokens(sd, f, ["proj_pnr", "proj_oscc", None, "proj_lta"]), "transformer.", c["h"], [x.shape[1] for x in f]
    # hhi_g encode_features('ttm', lam, ttm, asd): tokens lam | ttm | asd
    return tr.hhi_tokens(sd, f, ["lam", "ttm", "asd"], [0, 1, 2]), "transformer_encoder.", c["h"], [x.shape[1] for x in f]


_ORACLE = {}


def case_oracle(name: str):
    """fp64 (weights (L, B, S, S), by_segment (L, B, S, K), rollout (B, S, S), rollout_by_segment (B, S, K), table (B, K)) of a model case,
    computed once and shared (never modified)."""
    if name not in _ORACLE:
        c = ALL_CASES[name]
        _, sd64 = new_model(c)
        with torch.no_grad():
            x, prefix, H, lens = case_tokens(c, sd64, case_feats(c))
            w, _ = encoder_weights(sd64, prefix, x, H)
        table = torch.tensor([lens] * c["B"], dtype=torch.int32)
        R = rollout(w)
        _ORACLE[name] = (w, segment_sums(w, table), R, segment_sums(R, table), table)
    return _ORACLE[name]


def case_variant(name: str, dtype=torch.float64, round_bf16: bool = False) -> torch.Tensor:
    """The case's weights from the same oracle in another arithmetic: fp32 throughout, or fp64 on bf16-rounded in_proj weights and inputs."""
    c = ALL_CASES[name]
    _, sd64 = new_model(c)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd64.items()}
    with torch.no_grad():
        x, prefix, H, _ = case_tokens(c, sd, case_feats(c))
        w, _ = encoder_weights(sd, prefix, x, H, round_bf16=round_bf16)
    return w.double()


def uniform_answer(L: int, table, S: int):
    """(weights, by_segment, rollout, rollout_by_segment) of an encoder that ignores its scores: every weight 1 / S_b."""
    table = torch.as_tensor(table)
    lens = table.sum(1).tolist()
    w = torch.zeros(L, table.shape[0], S, S, dtype=torch.float64)
    for b, n in enumerate(lens):        # (a ragged batch: 1 / S_b over the clip's own tokens, zeros beyond)
        w[:, b, :n, :n] = 1.0 / n
    R = rollout(w, lengths=lens)
    return w, segment_sums(w, table), R, segment_sums(R, table)


def model_bar(x, ref, uniform, what: str, e32=None):
    """The model-level bars on a device quantity `x` against fp64 `ref`: e = max |x - ref| < s / 4 with s = max |ref - uniform|, `uniform`
    the same quantity of an encoder that ignores its scores (uniform_answer). e32: the fp32 oracle's error (f32 / f32s paths): e < 8 e32.
    Returns (e, s)."""
    e = (x.double().cpu() - ref).abs().max().item()
    s = (ref - uniform).abs().max().item()
    print(f"[{what}] e = {e:.3e}, s = max|oracle - uniform| = {s:.3e}, e / s = {e / s:.4f}" + (f", fp32 oracle {e32:.3e}" if e32 is not None else ""))
    assert e < s / 4, (what, e, s)
    if e32 is not None:
        assert e < 8 * e32, (what, e, e32)
    return e, s


# ---- the perturbed references: each must miss the bar on every named case ----
def perturbed(name: str):
    """{perturbation: (perturbed quantity, reference quantity, index of the quantity in uniform_answer)} for a model case."""
    c = ALL_CASES[name]
    _, sd64 = new_model(c)
    w, seg, R, _, table = case_oracle(name)
    with torch.no_grad():
        x, prefix, H, lens = case_tokens(c, sd64, case_feats(c))
        _, xs = encoder_weights(sd64, prefix, x, H)
        d = x.shape[-1]
        out = {}
        if w.shape[0] > 1:
            out["neighbouring layer"] = (torch.roll(w, 1, 0), w, 0)
        p0 = f"{prefix}layers.0."
        in_w, in_b = sd64[p0 + "self_attn.in_proj_weight"], sd64[p0 + "self_attn.in_proj_bias"]
        q, k = tr.linear(xs[0], in_w[:d], in_b[:d]), tr.linear(xs[0], in_w[d:2 * d], in_b[d:2 * d])
        B, S = q.shape[:2]
        dh = d // H
        sc = (q.reshape(B, S, H, dh).permute(0, 2, 1, 3) @ k.reshape(B, S, H, dh).permute(0, 2, 3, 1)) / math.sqrt(dh)
        out["softmax of the head-mean score"] = (torch.softmax(sc.mean(1), -1), w[0], 0)
        out["no 1/sqrt(dh)"] = (weights_from_input(xs[0], in_w, in_b, H, scale=False), w[0], 0)
        if len(lens) > 1:
            shifted = table.clone()
            shifted[:, 0] += 1
            shifted[:, 1] -= 1
            out["segment boundary shifted"] = (segment_sums(w, shifted), seg, 1)
        if w.shape[0] > 1:
            out["rollout in reverse order"] = (rollout(w, reverse=True), R, 2)
        out["rollout without identity"] = (rollout(w, identity=False), R, 2)
    return out
