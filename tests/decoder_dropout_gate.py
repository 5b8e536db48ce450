"""Gate of the EgoT2-g sequence decoder's TRAIN-mode dropout: the case table, the fp64 oracle run of a case under the masks the HIP kernels
draw (tests/dropmask.py decoder_masks -> oracle/translator_ref.py g_decode(masks=)), the GPU run of a case, the metric, and the perturbed
oracles that show the metric would notice a wrong mask.

What is compared: the vocabulary logits, d(memory) and the gradient of every decoder, `fc` and `embedding` parameter under the loss
(logits * w).sum() with a fixed random w. The memory is a seeded random tensor fed straight to decode(), so no encoder error enters.
Bars (the project's own for the same paths at p = 0, not derived from what the kernels give):
    bf16 fused     logits 1.5e-2 * max(1, |ref|max)   d(memory) 6e-2 relative norm   every gradient 8e-2 relative norm
                   (tol_dec of tests/test_gpu_golden.py; test_fused_decoder_matches_the_composed_decoder of tests/test_gpu_decoder.py)
    f32 composed   logits 1e-3 * max(1, |ref|max)     every gradient, d(memory) included, 1e-2   (the f32 bars of tests/test_gpu_golden.py)
A wrong mask is an O(1) error: tests/test_cpu_decoder_dropout.py holds every perturbed oracle of perturbations() to a miss of the bf16 bar
by at least 3x, and shows that bf16-rounded weights stay within half of it.

Shared by tests/test_gpu_decoder_dropout.py (-m gpu), tests/test_cpu_decoder_dropout.py and tools/decoder_dropout_report.py. Test
infrastructure only."""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass
from types import SimpleNamespace as NS
from typing import Dict, Tuple

import numpy as np
import torch

from oracle import translator_ref as tr
from tests import dropmask as dm
from tests.fp32_grade import kink_free
from tests.util import seeded_state_dict

BF16_BAR = {"logits": 1.5e-2, "dmem": 6e-2, "grad": 8e-2}
F32_BAR = {"logits": 1e-3, "dmem": 1e-2, "grad": 1e-2}
PERTURBED_MIN = 3.0         # every perturbed oracle misses the bf16 bar by at least this factor
BF16_WEIGHTS_MAX = 0.5      # the oracle on bf16-rounded weights stays within this fraction of the bf16 bar
HOST_SEED = 0x5EEDDEC0DE
EMB_SCALE = 1.0 / 16.0      # embedding.weight of seeded_state_dict (N(0, 1)) times this: see case_data
# The embed site's keep-scale is all but invisible at p_pos = 0.1: x -> 0.9 x leaves norm1(x + SA(x)) unchanged up to the attention biases
# (LayerNorm is scale-invariant, SA is linear in x for fixed probabilities) and the embedding gradient too (mask scale x d(x) is unchanged).
# Measured miss of the bf16 bar with the scale taken as 1: 1.4 .. 4.1 at p_pos = 0.1, 5.3 .. 11.6 at p_pos = 0.3. The perturbation is
# therefore asserted on the cases with p_pos >= 0.3, which run on the GPU like the others.
EMBED_SCALE_MIN_P = 0.3


def _chunk_from_source() -> int:
    """Keys per chunk of dec_attn_long_kernel, read from the kernel (csrc/wide_decoder.hip: its `for (int j0 = 0; j0 < Sk; j0 += N)`
    loops), so that the whole-chunks-only cases follow the kernel if its chunk length changes."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egot2_amd", "csrc", "wide_decoder.hip")).read()
    body = src[src.index("void dec_attn_long_kernel("):src.index("int dec_attn_long(")]
    steps = set(re.findall(r"for \(int j0 = 0; j0 < Sk; j0 \+= (\d+)\)", body))
    assert len(steps) == 1, f"dec_attn_long_kernel: chunk loops step by {sorted(steps)}"
    return int(steps.pop())


CHUNK = _chunk_from_source()        # (64; DA_MAXK = 64 is the last length of the one-wave kernel)


# ---- the case table ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    impl: str = "fused"             # fused (compute bf16) | composed (compute f32)
    model: str = "hhi"              # hhi: hhi_multitask.TaskTranslationPromptTransformer, d = 256, V = 7; hoi: hoi_multitask
                                    # .TaskTranslationPromptTransformer6Task, d = 512, V = 12; both 2 layers
    B: int = 3
    H: int = 4
    sy: int = 2
    S: int = 45
    p_drop: float = 0.3
    p_pos: float = 0.1
    device_seed: bool = False       # enable_device_seed(): the key table derived on the stream
    lengths: Tuple[int, ...] = ()   # ragged training: memory tokens per clip (B = len(lengths))
    seed: int = 0                   # weights, memory, tokens, w

    @property
    def d(self) -> int:
        return 512 if self.model == "hoi" else 256

    @property
    def V(self) -> int:
        return 12 if self.model == "hoi" else 7

    @property
    def bars(self) -> dict:
        return dict(BF16_BAR if self.impl == "fused" else F32_BAR)

    @property
    def host_seed(self) -> int:
        return HOST_SEED + self.seed

    @property
    def mask_seed(self) -> int:
        """The seed whose masks the run draws. Device-resident seed: the value the word holds at the decode call, one lcg step past the
        one it was set to (what the encoder's forward of a step leaves behind; the decoder reads the word and does not advance it)."""
        return dm.lcg(self.host_seed) if self.device_seed else self.host_seed


L, D_FF = 2, 2048
CASES = (
    # fused, short memory: the one-wave kernel at its edges (sy = 8 = DA_MAXQ, S = 64 = DA_MAXK), head dim 64
    # (seeds: short-sy2-s1 and devseed-short moved off their first seed, at which the bf16-weights oracle sat at 0.49 of the bar)
    [Case(f"short-sy{sy}-s{S}", sy=sy, S=S, seed=10 * sy + i + (4 if (sy, S) == (2, 1) else 0)) for sy in (1, 2, 8) for i, S in enumerate((1, 45, 64))]
    # ... and head dim 32
    + [Case("short-dh32", B=5, H=8, sy=5, S=12, seed=91)]
    # fused, long memory: the chunked kernel's first length, a ragged last chunk, whole chunks only (3 of them)
    + [Case("long-s65", sy=2, S=65, seed=92), Case("long-s180", sy=3, S=180, seed=93),
       Case(f"long-s{3 * CHUNK}-sy2", sy=2, S=3 * CHUNK, seed=94), Case(f"long-s{3 * CHUNK}-sy8", sy=8, S=3 * CHUNK, seed=95)]
    # the composed decoder in exact fp32
    + [Case(f"composed-sy{sy}-s{S}", impl="composed", sy=sy, S=S, seed=100 + sy) for sy, S in ((2, 45), (8, 64), (3, 180))]
    # a positional probability at which the embed site's SCALE shows (EMBED_SCALE_MIN_P), fused and composed (whose embed key differs)
    + [Case("embed-p03-sy1", sy=1, S=1, p_pos=0.3, seed=105), Case("embed-p03-sy2", sy=2, S=45, p_pos=0.3, seed=106),
       Case("embed-p03-composed", impl="composed", sy=2, S=45, p_pos=0.3, seed=107)]
    # one probability zero: the key derivation and the capture refusal test `p_drop > 0 || p_pos > 0`
    + [Case("only-p-drop", sy=2, S=45, p_pos=0.0, seed=111), Case("only-p-pos", sy=2, S=65, p_drop=0.0, seed=112)]
    # the key table derived on the stream from the device-resident seed
    + [Case("devseed-short", sy=2, S=45, device_seed=True, seed=125), Case("devseed-long", sy=3, S=180, device_seed=True, seed=122)]
    # ragged training: both attention classes in one batch
    + [Case("ragged", sy=2, lengths=(1, 45, 64, 65, 180), B=5, S=180, seed=131)]
    # the other DecoderMixin user, at its own head count
    + [Case("hoi", model="hoi", H=8, sy=2, S=48, seed=141)]
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES) and all(c.B <= 5 for c in CASES)


# ---- one case: model, data, oracle ---------------------------------------------------------------------------------------------------
def new_model(case: Case):
    """The case's model on the CPU (weights as constructed; load case_data()["sd"])."""
    from egot2_amd.synth import HHI_G_VOCAB, HOI_G_VOCAB
    if case.model == "hoi":
        from egot2_amd import hoi_multitask
        m = hoi_multitask.TaskTranslationPromptTransformer6Task(NS(hidden_dim=512, num_heads=case.H, num_layers=L, dropout=case.p_drop), HOI_G_VOCAB)
    else:
        from egot2_amd import hhi_multitask
        args = NS(hidden_dim=256, num_heads=case.H, num_layers=L, dropout=case.p_drop, lam_checkpoint=None, ttm_checkpoint=None, asd_checkpoint=None)
        m = hhi_multitask.TaskTranslationPromptTransformer(args, HHI_G_VOCAB)
    m.pos_embed.dropout.p = case.p_pos
    return m


def is_decoder_param(name: str) -> bool:
    return name.startswith(("transformer_decoder.", "fc.", "embedding."))


_DATA: Dict[str, dict] = {}       # the last two cases' data (a case is ~40 MB of weights and masks; tests visit the table case by case)


def case_data(case: Case) -> dict:
    """Everything a run of the case needs, from the seeds alone (shared by the tests of a case and left unchanged): "sd" the full state dict
    (fp32), "dsd" its decoder / fc / embedding / pe entries, "mem" the memory ((S, B, d), ragged: packed (sum S_b, d)), "y" (B, sy) tokens,
    "w" (sy, B, V), "masks" (ragged: one per clip), "margins" {layer: (min |a| / rms(a), fraction of a > 0)} of the ReLU pre-activations.
    Two choices keep bf16 ROUNDING well inside the bf16 bar, so that what is left over is the masks (test_cpu_decoder_dropout.py: the
    oracle on bf16-rounded weights stays within half the bar; with seeded_state_dict as it comes it sits AT the bar):
      - embedding.weight is scaled by EMB_SCALE = 1 / 16: embedding * sqrt(d) + pe is then O(1) like every later layer's input, and
        layer 0's self-attention scores have unit spread instead of ~256 (a saturated softmax turns a rounding into a flipped argmax);
      - every layer's linear1.bias is re-chosen by tests/fp32_grade.py kink_free under the case's own masks, so that no ReLU
        pre-activation of the case sits within ~1e-2 rms of its kink: a unit flipped by a rounding moves linear1's gradients by
        sqrt(fraction flipped), 4 .. 6e-2 with the stock biases."""
    if case.id in _DATA:
        return _DATA[case.id]
    m = new_model(case)
    sd = seeded_state_dict(m, 400 + case.seed)
    sd["embedding.weight"] = sd["embedding.weight"] * EMB_SCALE
    rng = np.random.default_rng(7000 + case.seed)
    d, V = case.d, case.V
    rows = sum(case.lengths) if case.lengths else case.S * case.B
    mem = torch.from_numpy(rng.standard_normal((rows, d), dtype=np.float32))
    if not case.lengths:
        mem = mem.view(case.S, case.B, d)
    data = {"sd": sd, "dsd": {k: v for k, v in sd.items() if is_decoder_param(k) or k == "pos_embed.pe"}, "mem": mem,
            "y": torch.from_numpy(rng.integers(0, V, (case.B, case.sy))).long(),
            "w": torch.from_numpy(rng.standard_normal((case.sy, case.B, V), dtype=np.float32))}
    data["masks"] = case_masks(case, case.mask_seed)
    data["dsd"], data["margins"] = kink_free(data["dsd"], lambda sd64: _forward(case, data, sd64, data["masks"], torch.float64), L, "transformer_decoder.")
    sd.update(data["dsd"])
    while len(_DATA) >= 2:
        _DATA.pop(next(iter(_DATA)))
    _DATA[case.id] = data
    return data


def case_masks(case: Case, seed: int):
    """The keep-scales the case's implementation draws with host seed `seed` (ragged: a list, one g_decode `masks` per clip)."""
    if case.lengths:
        return [dm.decoder_ragged_clip_masks(seed, b, case.sy, S_b, case.d, case.H, D_FF, L, case.p_drop, case.p_pos)
                for b, S_b in enumerate(case.lengths)]
    return dm.decoder_masks(seed, case.impl, case.B, case.sy, case.S, case.d, case.H, D_FF, L, case.p_drop, case.p_pos)


def _cast(masks, dtype):
    if isinstance(masks, torch.Tensor):
        return masks.to(dtype)
    if isinstance(masks, dict):
        return {k: _cast(v, dtype) for k, v in masks.items()}
    if isinstance(masks, (list, tuple)):
        return [_cast(v, dtype) for v in masks]
    return masks


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def _forward(case: Case, data, sdd, masks, dtype, mem=None, decode=None):
    """Logits (sy, B, V) of the oracle on the state dict `sdd` (already in `dtype`); a ragged case clip by clip on its own memory rows."""
    decode = decode or tr.g_decode
    mem = data["mem"].to(dtype) if mem is None else mem
    if not case.lengths:
        return decode(sdd, case.H, data["y"], mem, masks=_cast(masks, dtype))
    outs, r0 = [], 0
    for b, S_b in enumerate(case.lengths):
        outs.append(decode(sdd, case.H, data["y"][b:b + 1], mem[r0:r0 + S_b, None, :], masks=_cast(masks[b], dtype)))
        r0 += S_b
    return torch.cat(outs, dim=1)


def oracle_run(case: Case, data, masks="case", dtype=torch.float64, bf16_weights=False, decode=None) -> dict:
    """-> {"logits" (sy, B, V), "dmem" (the memory's layout), "grads": {name: gradient}} of the oracle in `dtype` under `masks` (default: the
    case's own). bf16_weights: every weight matrix (2-D parameter) and the memory rounded to bf16 first, the arithmetic stays in `dtype`.
    decode: a replacement for tr.g_decode (the perturbed oracles)."""
    masks = data["masks"] if isinstance(masks, str) else masks

    def leaf(k, v):
        if k.endswith(".pe"):
            return v.to(dtype)
        v = bf16_round(v) if (bf16_weights and v.dim() >= 2) else v
        return v.detach().to(dtype).clone().requires_grad_(True)          # (a copy: the shared case data stays as it is)

    sdd = {k: leaf(k, v) for k, v in data["dsd"].items()}
    mem = (bf16_round(data["mem"]) if bf16_weights else data["mem"]).detach().to(dtype).clone().requires_grad_(True)
    w = data["w"].to(dtype)
    logits = _forward(case, data, sdd, masks, dtype, mem, decode)
    (logits * w).sum().backward()
    return {"logits": logits.detach(), "dmem": mem.grad, "grads": {k: v.grad for k, v in sdd.items() if v.requires_grad}}


# ---- the gate ------------------------------------------------------------------------------------------------------------------------
def _rel(a: torch.Tensor, ref: torch.Tensor) -> float:
    a, ref = a.detach().double().cpu().reshape(ref.shape), ref.detach().double().cpu()
    n = ref.norm().item()
    if n == 0.0:
        return 0.0 if a.norm().item() == 0.0 else math.inf
    return (a - ref).norm().item() / n


def gate(res: dict, ref: dict, bars: dict, clip_rows=None) -> dict:
    """Logits, d(memory) and every parameter gradient of `res` against `ref`: {"logits": max |d| / max(1, |ref|max), "dmem": relative norm
    (clip_rows [(r0, r1), ...]: the worst clip of a packed ragged memory, each on its own rows), "grads": {name: relative norm}, "grad":
    the worst of them, "worst_grad": its name, "ratio": {quantity: x bar}, "miss": the largest ratio (> 1: over a bar), "ok"}. A gradient
    the reference has and `res` has not, or the other way round, is an error of the comparison itself."""
    assert set(res["grads"]) == set(ref["grads"]), sorted(set(res["grads"]) ^ set(ref["grads"]))
    lr = ref["logits"].detach().double().cpu()
    out = {"logits": (res["logits"].detach().double().cpu().reshape(lr.shape) - lr).abs().max().item() / max(1.0, lr.abs().max().item())}
    if clip_rows:
        out["dmem"] = max(_rel(res["dmem"][r0:r1], ref["dmem"][r0:r1]) for r0, r1 in clip_rows)
    else:
        out["dmem"] = _rel(res["dmem"], ref["dmem"])
    out["grads"] = {k: _rel(res["grads"][k], g) for k, g in ref["grads"].items()}
    out["worst_grad"] = max(out["grads"], key=out["grads"].get)
    out["grad"] = out["grads"][out["worst_grad"]]
    out["ratio"] = {"logits": out["logits"] / bars["logits"], "dmem": out["dmem"] / bars["dmem"],
                    **{k: v / bars["grad"] for k, v in out["grads"].items()}}
    out["miss"] = max(out["ratio"].values())
    out["ok"] = all(math.isfinite(v) and v < 1.0 for v in out["ratio"].values())
    return out


def clip_rows(case: Case):
    if not case.lengths:
        return None
    r = np.cumsum((0,) + tuple(case.lengths))
    return [(int(r[b]), int(r[b + 1])) for b in range(len(case.lengths))]


# ---- perturbed oracles ---------------------------------------------------------------------------------------------------------------
def _site_get(masks, site, layer):
    return masks["embed"] if site == "embed" else masks["layers"][layer][site]


def _site_set(masks, site, layer, value):
    out = {"embed": masks["embed"], "layers": [dict(m) for m in masks["layers"]]}
    if site == "embed":
        out["embed"] = value
    else:
        out["layers"][layer][site] = value
    return out


def _roll_rows(t: torch.Tensor) -> torch.Tensor:
    """The mask one ROW later: rows are every axis but the last (the column), in the kernels' row-major order."""
    return torch.roll(t.reshape(-1, t.shape[-1]), 1, dims=0).reshape(t.shape)


def _decode_ffn_mask_before_bias(sd, n_heads, y, memory, masks=None):
    """g_decode with ONE misplaced site: the FFN keep-scale applied to linear1's product before the bias add and the ReLU
    (relu(m * (x W1^T) + b1) instead of m * relu(x W1^T + b1))."""
    d = sd["embedding.weight"].shape[1]
    sy = y.shape[1]
    x = tr._m(sd["embedding.weight"][y] * math.sqrt(d) + sd["pos_embed.pe"][:sy, 0, :], masks, "embed")
    mem = memory.permute(1, 0, 2)
    for i in range(tr.n_layers_of(sd, "transformer_decoder.")):
        pre = f"transformer_decoder.layers.{i}."
        g = lambda k: sd[pre + k]  # noqa: E731
        mk = masks["layers"][i]
        a = tr.attention(x, x, g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias"), g("self_attn.out_proj.weight"),
                         g("self_attn.out_proj.bias"), n_heads, True, mk["self"])
        x = tr.layer_norm(x + a * mk["sa_out"], g("norm1.weight"), g("norm1.bias"))
        c = tr.attention(x, mem, g("multihead_attn.in_proj_weight"), g("multihead_attn.in_proj_bias"), g("multihead_attn.out_proj.weight"),
                         g("multihead_attn.out_proj.bias"), n_heads, False, mk["cross"])
        x = tr.layer_norm(x + c * mk["ca_out"], g("norm2.weight"), g("norm2.bias"))
        h = torch.relu(tr.linear(x, g("linear1.weight"), None) * mk["ffn"] + g("linear1.bias"))
        f = tr.linear(h, g("linear2.weight"), g("linear2.bias"))
        x = tr.layer_norm(x + f * mk["ffn_out"], g("norm3.weight"), g("norm3.bias"))
    return tr.linear(x, sd["fc.weight"], sd["fc.bias"]).permute(1, 0, 2)


def perturbations(case: Case, data):
    """(name, masks, decode) of every perturbed oracle of a uniform case: for each of the seven sites (the per-layer ones in each layer) the
    mask of another seed, the mask shifted by one row, and the scale 1 instead of 1 / (1 - p); and the FFN mask before the bias add. Sites
    whose probability is 0 in the case have no mask to perturb and are left out, and so is the embed site's scale below EMBED_SCALE_MIN_P."""
    assert not case.lengths
    right, other = data["masks"], case_masks(case, case.mask_seed + 1)
    where = [("embed", 0)] if case.p_pos > 0 else []
    if case.p_drop > 0:
        where += [(s, l) for l in range(L) for s in dm.DEC_SITES[1:]]
    for site, layer in where:
        tag = site if site == "embed" else f"{site}.{layer}"
        m = _site_get(right, site, layer)
        yield f"other-seed/{tag}", _site_set(right, site, layer, _site_get(other, site, layer)), None
        yield f"row-shift/{tag}", _site_set(right, site, layer, _roll_rows(m)), None
        if site != "embed" or case.p_pos >= EMBED_SCALE_MIN_P:
            yield f"scale-1/{tag}", _site_set(right, site, layer, m.clamp(max=1.0)), None
    if case.p_drop > 0:
        yield "ffn-mask-before-bias", right, _decode_ffn_mask_before_bias


# ---- one case on the GPU -------------------------------------------------------------------------------------------------------------
def _signed64(v: int) -> int:
    v &= dm.M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _poison(cuda, sizes):
    """Best effort at "every element is written": the autograd Functions allocate their gradients themselves (torch.empty), so NaN-filled
    blocks of the same sizes are handed back to the caching allocator just before the run; a gradient element the library leaves unwritten
    then reads NaN and fails the comparison."""
    for n in sizes:
        t = torch.full((int(n),), float("nan"), dtype=torch.float32, device=cuda)
        del t


def gpu_run(case: Case, data, cuda) -> dict:
    """Forward and backward of the case through the HIP library, twice with the same seed -> the oracle_run layout plus "impl" (what
    last_decoder_impl() said), "repeat_equal" (the second run's logits, d(memory) and every gradient have the first run's bits) and
    "repeat_diff" ({quantity: relative norm of the difference} of those that have not)."""
    from egot2_amd import functional as F_egx
    m = new_model(case)
    m.load_state_dict(data["sd"])
    m = m.to(cuda).set_compute("bf16" if case.impl == "fused" else "f32").train()
    seed = case.mask_seed
    if case.device_seed:
        m.enable_device_seed()
        m._egx_seed_dev.fill_(_signed64(seed))
        m._egx_seed = lambda: 0            # (the host seed is not the one in use)
    else:
        m._egx_seed = lambda: seed
    y, w = data["y"].to(cuda), data["w"].to(cuda)
    names = [k for k, _ in m.named_parameters() if is_decoder_param(k)]
    n_flat = sum(p.numel() for k, p in m.named_parameters() if is_decoder_param(k))
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        mem = data["mem"].to(cuda).requires_grad_(True)
        torch.cuda.synchronize()
        _poison(cuda, [mem.numel(), n_flat] + [p.numel() for k, p in m.named_parameters() if is_decoder_param(k)])
        if case.lengths:
            logits = m.decode_ragged(y, mem, torch.tensor(case.lengths))
        else:
            logits = m.decode(y, mem)
        impl = F_egx.last_decoder_impl()
        (logits * w).sum().backward()
        torch.cuda.synchronize()
        if case.device_seed:
            assert int(m._egx_seed_dev.item()) == _signed64(seed), "the decoder advanced the device seed"
        named = dict(m.named_parameters())
        missing = [k for k in names if named[k].grad is None]
        assert not missing, f"no gradient for {missing}"
        runs.append({"logits": logits.detach().clone(), "dmem": mem.grad.detach().clone(),
                     "grads": {k: named[k].grad.detach().clone() for k in names}, "impl": impl})
    a, b = runs
    diff = {"logits": _rel(b["logits"], a["logits"]), "dmem": _rel(b["dmem"], a["dmem"]), **{k: _rel(b["grads"][k], a["grads"][k]) for k in names}}
    same = {"logits": torch.equal(a["logits"], b["logits"]), "dmem": torch.equal(a["dmem"], b["dmem"]),
            **{k: torch.equal(a["grads"][k], b["grads"][k]) for k in names}}
    a["repeat_diff"] = {k: diff[k] for k, eq in same.items() if not eq}       # {quantity: relative norm of the difference} where bits differ
    a["repeat_equal"] = not a["repeat_diff"]
    return a


def swap_diagnosis(case: Case, data, res, ref_masks) -> dict:
    """For a case over its bar: the gate's miss with each site's mask swapped for another seed's in turn. A site whose swap LOWERS the miss
    by an order of magnitude is the one the kernel keys differently; rounding does not move."""
    out = {}
    if case.lengths:
        return out
    other = case_masks(case, case.mask_seed + 1)
    for site, layer in [("embed", 0)] + [(s, l) for l in range(L) for s in dm.DEC_SITES[1:]]:
        mk = _site_set(ref_masks, site, layer, _site_get(other, site, layer))
        out[f"{site}.{layer}"] = gate(res, oracle_run(case, data, masks=mk), case.bars)["miss"]
    return out
