"""fp64 reference of the decoder's cross-attention weights for the tests (no GPU, no reference tree): oracle.translator_ref.g_decode
restated so that it also returns, per decoder layer, the head-averaged weights nn.MultiheadAttention gives CustomDecoderLayer._mha_block
with need_weights=True (HHI/models/multitask/task_prompt_model.py:163-172, HOI/models/multitask/video_model_builder.py:20-30). Built on
the oracle's linear / layer_norm / attention; tests/golden/make_golden_attn.py checks it against forward hooks on the real classes."""
import math

import torch

from oracle import translator_ref as tr


def softmax_weights(q: torch.Tensor, k: torch.Tensor, n_heads: int) -> torch.Tensor:
    """q (B, Sq, d), k (B, Sk, d) -> (B, Sq, Sk): the mean over heads of softmax_j(q_h . k_h / sqrt(dh)), in the inputs' dtype."""
    B, Sq, d = q.shape
    Sk, dh = k.shape[1], d // n_heads
    qh = q.reshape(B, Sq, n_heads, dh).permute(0, 2, 1, 3)
    kh = k.reshape(B, Sk, n_heads, dh).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(dh)
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    return (p / p.sum(dim=-1, keepdim=True)).mean(dim=1)


def cross_weights(x: torch.Tensor, mem: torch.Tensor, in_w, in_b, n_heads: int) -> torch.Tensor:
    """The weights of oracle.translator_ref.attention(x, mem, ..., causal=False): x (B, Sq, d), mem (B, Sk, d) -> (B, Sq, Sk)."""
    d = x.shape[-1]
    return softmax_weights(tr.linear(x, in_w[:d], in_b[:d]), tr.linear(mem, in_w[d:2 * d], in_b[d:2 * d]), n_heads)


def g_decode_attn(sd, n_heads: int, y: torch.Tensor, memory: torch.Tensor):
    """g_decode that also returns the weights: y (B, sy) int64, memory (S, B, d) -> logits (sy, B, |V|), attn (L, B, sy, S)."""
    d = sd["embedding.weight"].shape[1]
    sy = y.shape[1]
    x = sd["embedding.weight"][y] * math.sqrt(d) + sd["pos_embed.pe"][:sy, 0, :]
    mem = memory.permute(1, 0, 2)
    attn = []
    for i in range(tr.n_layers_of(sd, "transformer_decoder.")):
        prefix = f"transformer_decoder.layers.{i}."
        g = lambda k: sd[prefix + k]  # noqa: E731
        a = tr.attention(x, x, g("self_attn.in_proj_weight"), g("self_attn.in_proj_bias"), g("self_attn.out_proj.weight"),
                         g("self_attn.out_proj.bias"), n_heads, True)
        x = tr.layer_norm(x + a, g("norm1.weight"), g("norm1.bias"))
        attn.append(cross_weights(x, mem, g("multihead_attn.in_proj_weight"), g("multihead_attn.in_proj_bias"), n_heads))
        c = tr.attention(x, mem, g("multihead_attn.in_proj_weight"), g("multihead_attn.in_proj_bias"),
                         g("multihead_attn.out_proj.weight"), g("multihead_attn.out_proj.bias"), n_heads, False)
        x = tr.layer_norm(x + c, g("norm2.weight"), g("norm2.bias"))
        f = tr.linear(torch.relu(tr.linear(x, g("linear1.weight"), g("linear1.bias"))), g("linear2.weight"), g("linear2.bias"))
        x = tr.layer_norm(x + f, g("norm3.weight"), g("norm3.bias"))
    return tr.linear(x, sd["fc.weight"], sd["fc.bias"]).permute(1, 0, 2), torch.stack(attn, 0)


def sharpen(sd64, factor: float):
    """A copy of the state dict whose cross-attention q and k projection rows (weights and biases) are scaled by `factor`: sharper
    softmaxes, so that the weights have entries far from 1 / S."""
    out = dict(sd64)
    for name, v in sd64.items():
        if ".multihead_attn.in_proj_" in name:
            d = v.shape[0] // 3
            v = v.clone()
            v[:2 * d] *= factor
            out[name] = v
    return out


# ---- the two recordings of tests/golden/make_golden_attn.py (weights and features are regenerated from the seeds) ----
RECORDINGS = {
    "attn_ref_hhi_g": dict(kind="hhi", task="ttm", d=256, h=4, L=2, B=4, T=15, sy=2, wseed=131, fseed=97, tseed=5),
    "attn_ref_hoi_g": dict(kind="hoi", task="action", d=256, h=8, L=2, B=3, sy=3, wseed=132, fseed=98, tseed=6),
}
HHI_VOCAB = {'</s>': 0, '<unk>': 1, 'ttm': 2, 'lam': 3, 'asd': 4, '0': 5, '1': 6}


def recording_inputs(c):
    """(model on the CPU, fp64 state dict, tokens (B, sy), fp64 memory (S, B, d)) of a recording's config, from its seeds."""
    from types import SimpleNamespace as NS
    from oracle import ref_harness as rh
    from tests.util import seeded_feats, seeded_state_dict
    g = torch.Generator().manual_seed(c["tseed"])
    if c["kind"] == "hhi":
        from egot2_amd import hhi_multitask
        args = NS(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"], dropout=0.0, lam_checkpoint=None, ttm_checkpoint=None, asd_checkpoint=None)
        m = hhi_multitask.TaskTranslationPromptTransformer(args, HHI_VOCAB)
        vocab = HHI_VOCAB
    else:
        from egot2_amd import hoi_multitask
        args = NS(hidden_dim=c["d"], num_heads=c["h"], num_layers=c["L"], dropout=0.0, pnr_cfg_file=None, oscc_cfg_file=None, action_cfg_file=None,
                  lta_cfg_file=None)
        m = hoi_multitask.TaskTranslationPromptTransformer6Task(args, rh.HOI_G_VOCAB)
        vocab = rh.HOI_G_VOCAB
    sd = seeded_state_dict(m, c["wseed"])
    m.load_state_dict(sd)
    sd64 = {k: v.double() for k, v in sd.items()}
    y = torch.randint(0, len(vocab), (c["B"], c["sy"]), generator=g)
    with torch.no_grad():
        if c["kind"] == "hhi":
            feats = [f.double() for f in seeded_feats(c["fseed"], [(c["B"], c["T"], 256)] * 3)]
            mem = tr.hhi_g_encode(sd64, c["h"], c["task"], *feats)
        else:
            feats = [f.double() for f in seeded_feats(c["fseed"], [(c["B"], 16, 8192), (c["B"], 16, 8192), (c["B"], 8, 2048), (c["B"], 8, 256)])]
            mem = tr.hoi_g_encode(sd64, c["h"], c["task"], *feats)
    return m, sd64, y, mem.contiguous(), feats


# ---- the inputs of the primitive's test (tests/test_gpu_attn_weights.py item 1; their condition is checked in tests/test_cpu_attn_weights.py) ----
PRIM_SHAPES = [(4, 64), (8, 32), (8, 16), (2, 128)]
PRIM_SQ, PRIM_SK, PRIM_B = (1, 3, 8), (1, 2, 63, 64, 65, 255, 256, 257, 1024), (1, 5)


def primitive_inputs(H: int, dh: int, Sq: int, Sk: int, B: int, rows: int = 0):
    """bf16-representable fp32 q (B * Sq, H * dh) and k (rows or B * Sk, H * dh): randn * 1.7 from a generator seeded by the shape."""
    g = torch.Generator().manual_seed(1000003 * H + 10007 * dh + 101 * Sq + 7 * Sk + B)
    q = (torch.randn(B * Sq, H * dh, generator=g) * 1.7).bfloat16().float()
    k = (torch.randn(rows or B * Sk, H * dh, generator=g) * 1.7).bfloat16().float()
    return q, k


def primitive_cases(H: int, dh: int):
    for Sq in PRIM_SQ:
        for Sk in PRIM_SK:
            for B in PRIM_B:
                yield Sq, Sk, B
