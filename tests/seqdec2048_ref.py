"""Shared helpers of tests/test_cpu_seqdec2048.py, tests/test_gpu_seqdec2048.py and tools/seqdec2048_eval.py: the sequence decoder at head
dim 256 / 512 (d_model up to 2048) — the three LTA sequence-decoder models of egot2_amd/hoi_lta_seq.py (reference
HOI/models/lta/lta_models_seqdecoder.py:65-240, lta_models_lta_transfer.py:531-659).

Two references, both oracle/translator_ref.py g_decode (and `encoder` for the model-level case) in fp64:
    E   on the values as they are;
    R   on weight matrices and memory rounded to bf16 and back: what the bf16 decoder multiplies with.
Weights: tests/util.py seeded_state_dict, embedding x EMB_SCALE and every layer's linear1.bias re-chosen kink-free, as
tests/decoder_dropout_gate.py case_data does and for its reasons (imported from there). The GPU model HOLDS the rounded values, so device-vs-R
is the device's own arithmetic error; it is asserted at the decoder's existing bf16 bars (decoder_dropout_gate.BF16_BAR: logits 1.5e-2,
d(memory) 6e-2, every parameter gradient 8e-2) through decoder_dropout_gate.gate. R-vs-E is recorded, not asserted: with the stock
seeded_state_dict (embedding / 16, p = 0, B = 3) R alone already sits at or above the bars against E (logits 5e-3 .. 6e-3, d(memory) 4e-2 ..
5e-2, linear1.bias 8e-2 .. 1.1e-1), which is why R and not E is the device's reference here. Test infrastructure only."""
from __future__ import annotations

import math
import os
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import translator_ref as tr
from tests import dropmask as dm
from tests.decoder_dropout_gate import BF16_BAR, EMB_SCALE, PERTURBED_MIN, bf16_round, gate      # noqa: F401  (the bars are the gate's)
from tests.fp32_grade import kink_free
from tests.util import seeded_feats, seeded_state_dict

D_FF = 2048                         # nn.TransformerEncoderLayer / DecoderLayer default, as the reference builds them
W_SEED, F_SEED = 433, 7033
REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "seqdec2048_report.txt")

# decode() against R: (kind, d, heads, L, sy, S, B)
DECODE_CASES = [("fcst", 256, 1, 2, 3, 4, 3), ("fcst", 512, 1, 1, 8, 16, 2),
                ("fcst", 2048, 8, 1, 1, 2, 3),          # the eval recipe's shapes at one layer
                ("lta2", 2048, 4, 2, 3, 4, 2)]          # the 2-task recipe
# R against E, the issue's table: (d, heads, L, sy, S), B = 3
RE_CASES = [(256, 1, 2, 3, 4), (512, 1, 1, 8, 16), (512, 2, 2, 3, 4), (2048, 8, 1, 3, 4), (2048, 4, 1, 1, 2)]
# generation: name -> (d, heads, L, V, S, B, n_steps, weight seed, feature seed, verb / noun schedule, item 4)
GEN_CASES = {
    "d512_h2_v12": (512, 2, 1, 12, 2, 24, 4, 98, 96, False, True),
    "steps40_sched": (512, 1, 2, 40, 4, 16, 40, 95, 96, True, False),
    "one_step": (256, 1, 2, 12, 16, 5, 1, 95, 96, False, False),
    "steps64": (256, 1, 2, 40, 16, 4, 64, 95, 96, False, False),
    "d2048_h8": (2048, 8, 1, 12, 2, 3, 4, 95, 96, False, False),
}


def vocab_of(V: int) -> dict:
    """A V-word vocabulary with the start words of the three models' predict() (V >= 6)."""
    words = ['</s>', '<unk>', 'lta_verb', 'lta_noun', 'action'] + [str(i) for i in range(V - 5)]       # ('action' where tests/greedy_ref.py vocab_of has it)
    return {w: i for i, w in enumerate(words)}


def idx_maps(V: int):
    """(v_idx, n_idx): the first and the second half of the words behind the five special ones, sharing the middle word."""
    mid = 5 + (V - 5) // 2
    return list(range(5, mid + 1)), list(range(mid, V))


def fcst_cfg(d, heads, L, n=2):
    return NS(MODEL=NS(TRANSFORMER_ENCODER_HEADS=heads, TRANSFORMER_ENCODER_LAYERS=L, MULTI_INPUT_FEATURES=d), FORECASTING=NS(NUM_INPUT_CLIPS=n))


def lta2_cfg(d, heads, L, n=2, p=0.0):
    return NS(MODEL=NS(TRANSLATION_HEADS=heads, TRANSLATION_LAYERS=L, TRANSLATION_INPUT_FEATURES=d, TRANSLATION_DROPOUT=p),
              FORECASTING=NS(NUM_INPUT_CLIPS=n))


def new_model(kind, d, heads, L, V=12, n=2, p=0.0, cls=None):
    """kind fcst: ForecastingEncoderSeqDecoder (or `cls`, its subclass' name); lta2: TaskFusionMFTransformer2TaskSeqDecoder. On the CPU."""
    from egot2_amd import hoi_lta_seq
    v_idx, n_idx = idx_maps(V)
    if kind == "lta2":
        return hoi_lta_seq.TaskFusionMFTransformer2TaskSeqDecoder(lta2_cfg(d, heads, L, n, p), vocab_of(V), v_idx, n_idx)
    return getattr(hoi_lta_seq, cls or "ForecastingEncoderSeqDecoder")(fcst_cfg(d, heads, L, n), vocab_of(V), v_idx, n_idx)


def is_decoder_param(name: str) -> bool:
    return name.startswith(("transformer_decoder.", "fc.", "embedding."))


def rounded(sd: dict) -> dict:
    """Weight matrices (2-D and up) rounded to bf16 and back; vectors, `pe` and integer tensors as they are."""
    return {k: (bf16_round(v) if v.is_floating_point() and v.dim() >= 2 and not k.endswith("pos_embed.pe") else v) for k, v in sd.items()}


def case_data(kind, d, heads, L, sy, S, B, V=12, wseed=W_SEED, fseed=F_SEED, masks=None, stock=False) -> dict:
    """Everything a decode case needs, from the seeds alone: "model" (CPU, the UNROUNDED weights loaded), "sd" its state dict, "dsd" the
    decoder / fc / embedding / pe entries, "mem" (S, B, d), "y" (B, sy), "w" (sy, B, V), "margins" of kink_free. stock: seeded_state_dict
    with the scaled embedding only (the issue's R-vs-E table); else linear1.bias kink-free under `masks`."""
    m = new_model(kind, d, heads, L, V)
    sd = seeded_state_dict(m, wseed)
    sd["embedding.weight"] = sd["embedding.weight"] * EMB_SCALE
    rng = np.random.default_rng(fseed + d + 17 * sy + S)
    data = {"model": m, "H": heads, "L": L,
            "mem": torch.from_numpy(rng.standard_normal((S, B, d), dtype=np.float32)),
            "y": torch.from_numpy(rng.integers(0, V, (B, sy))).long(),
            "w": torch.from_numpy(rng.standard_normal((sy, B, V), dtype=np.float32))}
    dsd = {k: v for k, v in sd.items() if is_decoder_param(k) or k == "pos_embed.pe"}
    data["margins"] = None
    if not stock:
        m64 = None if masks is None else _cast(masks, torch.float64)
        dsd, data["margins"] = kink_free(dsd, lambda sd64: tr.g_decode(sd64, heads, data["y"], data["mem"].double(), masks=m64), L,
                                         "transformer_decoder.")
        sd.update(dsd)
    m.load_state_dict(sd)
    data["sd"], data["dsd"] = sd, dsd
    return data


def _cast(masks, dtype):
    if isinstance(masks, torch.Tensor):
        return masks.to(dtype)
    if isinstance(masks, dict):
        return {k: _cast(v, dtype) for k, v in masks.items()}
    if isinstance(masks, (list, tuple)):
        return [_cast(v, dtype) for v in masks]
    return masks


# ---- perturbed decoders (the CPU self-test of the gate) --------------------------------------------------------------------------------
def decode_perturbed(sd, n_heads, y, memory, masks=None, perturb=None):
    """tr.g_decode with ONE deliberate error. "scale64": both attentions scale their scores as head dim 64 would (1 / 8) whatever the head
    dim; "no_causal": the self-attention sees every target token; "swap": each layer runs its cross-attention block before its
    self-attention block."""
    d = sd["embedding.weight"].shape[1]
    sy = y.shape[1]
    x = tr._m(sd["embedding.weight"][y] * math.sqrt(d) + sd["pos_embed.pe"][:sy, 0, :], masks, "embed")
    mem = memory.permute(1, 0, 2)
    f = math.sqrt(d // n_heads / 64.0) if perturb == "scale64" else 1.0          # scores / sqrt(dh) * f = scores / sqrt(64)

    def attn(q_in, kv_in, pre, causal, mk):
        w, b = sd[pre + "in_proj_weight"], sd[pre + "in_proj_bias"]
        if f != 1.0:
            w, b = torch.cat((w[:d] * f, w[d:])), torch.cat((b[:d] * f, b[d:]))
        return tr.attention(q_in, kv_in, w, b, sd[pre + "out_proj.weight"], sd[pre + "out_proj.bias"], n_heads, causal, mk)

    for i in range(tr.n_layers_of(sd, "transformer_decoder.")):
        pre = f"transformer_decoder.layers.{i}."
        g = lambda k: sd[pre + k]  # noqa: E731
        mk = masks["layers"][i] if masks is not None else {k: None for k in dm.DEC_SITES}
        one = lambda t, k: t if mk.get(k) is None else t * mk[k]  # noqa: E731

        def self_block(x):
            a = attn(x, x, pre + "self_attn.", perturb != "no_causal", mk.get("self"))
            return tr.layer_norm(x + one(a, "sa_out"), g("norm1.weight"), g("norm1.bias"))

        def cross_block(x):
            c = attn(x, mem, pre + "multihead_attn.", False, mk.get("cross"))
            return tr.layer_norm(x + one(c, "ca_out"), g("norm2.weight"), g("norm2.bias"))

        x = self_block(cross_block(x)) if perturb == "swap" else cross_block(self_block(x))
        h = one(torch.relu(tr.linear(x, g("linear1.weight"), g("linear1.bias"))), "ffn")
        x = tr.layer_norm(x + one(tr.linear(h, g("linear2.weight"), g("linear2.bias")), "ffn_out"), g("norm3.weight"), g("norm3.bias"))
    return tr.linear(x, sd["fc.weight"], sd["fc.bias"]).permute(1, 0, 2)


PERTURBATIONS = ("scale64", "no_causal", "swap")


# ---- the oracle of a decode case -------------------------------------------------------------------------------------------------------
def oracle_run(data, rounded_values: bool, masks=None, perturb=None, grads=True) -> dict:
    """-> {"logits" (sy, B, V), "dmem" (S, B, d), "grads": {name: gradient}} of (logits * w).sum() in fp64: R (rounded_values) or E."""
    def leaf(k, v):
        if k.endswith(".pe"):
            return v.double()
        v = bf16_round(v) if (rounded_values and v.dim() >= 2) else v
        return v.detach().double().clone().requires_grad_(grads)

    sdd = {k: leaf(k, v) for k, v in data["dsd"].items()}
    mem = (bf16_round(data["mem"]) if rounded_values else data["mem"]).detach().double().clone().requires_grad_(grads)
    m64 = None if masks is None else _cast(masks, torch.float64)
    with torch.set_grad_enabled(grads):
        if perturb is None:
            logits = tr.g_decode(sdd, data["H"], data["y"], mem, masks=m64)
        else:
            logits = decode_perturbed(sdd, data["H"], data["y"], mem, m64, perturb)
        if grads:
            (logits * data["w"].double()).sum().backward()
    return {"logits": logits.detach(), "dmem": mem.grad, "grads": {k: v.grad for k, v in sdd.items() if v.requires_grad} if grads else {}}


def gpu_decode_run(data, cuda, train=False, seed=None) -> dict:
    """Forward and backward of the case through the library on the model holding the ROUNDED weights, fed the rounded memory -> the
    oracle_run layout plus "impl" (last_decoder_impl())."""
    from egot2_amd import functional as F_egx
    m = data["model"]
    m.load_state_dict(rounded(data["sd"]))
    m = m.to(cuda).set_compute("bf16")
    m.train(train)
    if seed is not None:
        m._egx_seed = lambda: seed
    m.zero_grad(set_to_none=True)
    mem = bf16_round(data["mem"]).to(cuda).requires_grad_(True)
    logits = m.decode(data["y"].to(cuda), mem)
    impl = F_egx.last_decoder_impl()
    (logits * data["w"].to(cuda)).sum().backward()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    names = [k for k in named if is_decoder_param(k)]
    missing = [k for k in names if named[k].grad is None]
    assert not missing, f"no gradient for {missing}"
    return {"logits": logits.detach().clone(), "dmem": mem.grad.detach().clone(), "grads": {k: named[k].grad.detach().clone() for k in names}, "impl": impl}


def gate_line(tag, g) -> str:
    return (f"{tag}: logits {g['logits']:.3e} (bar {BF16_BAR['logits']:g}) d(memory) {g['dmem']:.3e} ({BF16_BAR['dmem']:g}) "
            f"worst gradient {g['grad']:.3e} ({g['worst_grad']}, {BF16_BAR['grad']:g}); worst error / bar {g['miss']:.2f}")


# ---- generation ------------------------------------------------------------------------------------------------------------------------
def build_gen_case(name):
    """(model on the CPU with the seeded weights, fp64 state dict, start token, fp64 memory (S, B, d), allowed (2, V) bool or None)."""
    d, h, L, V, S, B, n, ws, fs, sched, _ = GEN_CASES[name]
    m = new_model("fcst", d, h, L, V)
    sd = seeded_state_dict(m, ws)
    m.load_state_dict(sd)
    mem = seeded_feats(fs, [(S, B, d)])[0].double()
    allowed = None
    if sched:
        v_idx, n_idx = idx_maps(V)
        allowed = torch.zeros((2, V), dtype=torch.bool)
        allowed[0, v_idx] = True
        allowed[1, n_idx] = True
    return m, {k: v.double() for k, v in sd.items()}, vocab_of(V)["action"], mem, allowed


# ---- the report ------------------------------------------------------------------------------------------------------------------------
_RECORDS = {}


def record(section, lines):
    """Keep `lines` as `section` of profiles/seqdec2048_report.txt (the other sections of the file are kept)."""
    _RECORDS[section] = list(lines)
    old = {}
    if os.path.exists(REPORT):
        cur = None
        for ln in open(REPORT).read().splitlines():
            if ln.startswith("## "):
                cur = ln[3:].strip()
                old[cur] = []
            elif cur is not None:
                old[cur].append(ln)
    old.update(_RECORDS)
    try:
        with open(REPORT, "w") as f:
            f.write("# The sequence decoder at head dim 256 / 512 (d_model up to 2048): measured errors and times (tests/test_cpu_seqdec2048.py,\n"
                    "# tests/test_gpu_seqdec2048.py, tools/seqdec2048_eval.py). E: fp64 oracle; R: the oracle on bf16-rounded weight matrices and memory.\n")
            for sec in sorted(old):
                body = [ln for ln in old[sec] if ln.strip()]
                f.write(f"\n## {sec}\n" + "\n".join(body) + "\n")
    except OSError as e:          # a read-only checkout: the figures are still printed by the caller
        print(f"seqdec2048 report not written: {e}")


# ---- the recordings of the REAL classes (tests/golden/make_golden_seqdec.py -> tests/golden/live/seqdec_*.npz) ----------------------------
# name -> config: the real class, its width, and the seeds of the weights (seeded_state_dict, embedding x EMB_SCALE) and of the clip features.
# Small widths with big heads; outputs and config only are stored.
RECORDINGS = {
    "seqdec_fcst_d256_h1": dict(cls="ForecastingEncoderSeqDecoder", kind="fcst", d=256, h=1, L=2, n=2, B=3, V=12, sy=3, steps=40, wseed=511, fseed=611),
    "seqdec_sep_d512_h1": dict(cls="ForecastingEncoderSeparateSeqDecoder", kind="fcst", d=512, h=1, L=1, n=2, B=3, V=12, sy=1, steps=0, wseed=512, fseed=612),
    "seqdec_lta2_d512_h2": dict(cls="TaskFusionMFTransformer2TaskSeqDecoder", kind="lta2", d=512, h=2, L=1, n=2, B=3, V=12, sy=3, steps=0, wseed=513, fseed=613),
}


def recording_inputs(c):
    """(fp64 state dict of the mirror's keys, features [fp64 (B, n, d), ...] (one stream for fcst, action and lta for lta2), target (B, sy))
    of a recording, from its seeds alone. The mirror and the real class share every state_dict key, so the dict loads into either."""
    m = new_model(c["kind"], c["d"], c["h"], c["L"], c["V"], c["n"], cls=c["cls"] if c["kind"] == "fcst" else None)
    sd = seeded_state_dict(m, c["wseed"])
    sd["embedding.weight"] = sd["embedding.weight"] * EMB_SCALE
    feats = [f.double() for f in seeded_feats(c["fseed"], [(c["B"], c["n"], c["d"])] * (2 if c["kind"] == "lta2" else 1))]
    y = torch.from_numpy(np.random.default_rng(c["fseed"] + 1).integers(0, c["V"], (c["B"], c["sy"]))).long()
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, feats, y


def oracle_memory(c, sd64, feats):
    """The decoder memory (S, B, d) of the helpers' fp64 oracle: fcst ln(feats) + sinusoid positions, lta2 ln(cat(action, lta)) + pe,
    through the post-LN encoder."""
    x = torch.cat(feats, dim=1)
    pos = sd64["pe"][0] if c["kind"] == "lta2" else sd64["pos_embed.pe"][:x.shape[1], 0, :]
    x = tr.encode_prepare(x, None, None, sd64["ln.weight"], sd64["ln.bias"], None, pos)
    return tr.encoder(x, sd64, "transformer_encoder.", c["L"], c["h"]).permute(1, 0, 2)


def oracle_recording(c, sd64, feats, y):
    """What a recording holds, from the helpers' fp64 oracle: "forward" (B, V, sy); "pred_verb" / "pred_noun" as the class' predict()
    returns them; for the 40-step class also "step_logits" (steps, B, V), "step_tokens" (B, steps), "step_margins" (steps, B) of the loop
    (the next token is the argmax over the WHOLE vocabulary, as lta_models_seqdecoder.py:197 takes it)."""
    from tests import greedy_ref as gr
    v_idx, n_idx = idx_maps(c["V"])
    vocab = vocab_of(c["V"])
    B = c["B"]
    with torch.no_grad():
        mem = oracle_memory(c, sd64, feats)
        out = {"forward": tr.g_decode(sd64, c["h"], y, mem).permute(1, 2, 0)}
        if c["steps"]:
            toks, logits, margins = gr.greedy(sd64, c["h"], torch.full((B,), vocab["action"], dtype=torch.int64), mem, c["steps"])
            out.update(step_logits=logits, step_tokens=toks, step_margins=margins,
                       pred_verb=logits[0::2][:, :, v_idx].permute(1, 0, 2), pred_noun=logits[1::2][:, :, n_idx].permute(1, 0, 2))
        else:
            lv = tr.g_decode(sd64, c["h"], torch.full((B, 1), vocab["lta_verb"], dtype=torch.int64), mem)
            ln_ = tr.g_decode(sd64, c["h"], torch.full((B, 1), vocab["lta_noun"], dtype=torch.int64), mem)
            out.update(pred_verb=lv[0][:, v_idx].unsqueeze(1), pred_noun=ln_[0][:, n_idx].unsqueeze(1))
    return out
