"""Host-side core shared by every translator class: packs nn.Parameters into the C-ABI call of
libegot2x.so. The nn.TransformerEncoder / nn.LayerNorm / nn.Linear submodules are kept only as PARAMETER
CONTAINERS so that state_dict keys, shapes and default initialisation are byte-compatible with the reference
(SURVEY.md §8b); their forward() is never called on the product path.
"""
from __future__ import annotations

import contextlib
import math
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from . import functional as F_egx
from .functional import EncoderSpec, SegmentSpec


class PositionalEncoding(nn.Module):
    """Sinusoidal table with the reference's buffer name and shape (max_len, 1, d)
    (HHI/models/ttm/model_taskspecific.py:131-151). The translator kernels read rows of `pe` directly; this
    module's forward is only used by the (torch) EgoT2-g sequence decoder."""

    def __init__(self, d_model, dropout=0.1, max_len=1000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pe = torch.zeros(max_len, d_model)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe[:, 0::2] = torch.sin(position * div_term)
        pe[:, 1::2] = torch.cos(position * div_term)
        pe = pe.unsqueeze(0).transpose(0, 1)  # (max_len, 1, d_model)
        self.register_buffer('pe', pe)

    def forward(self, x):
        x = x + self.pe[:x.size(0), :]
        return self.dropout(x)


def encoder_layer_tensors(encoder: nn.TransformerEncoder) -> List[torch.Tensor]:
    """Flatten nn.TransformerEncoder parameters in the order of egx_layer's fields."""
    out = []
    for layer in encoder.layers:
        if getattr(layer, "norm_first", False):
            raise ValueError("libegot2x implements the post-LN encoder layer only (norm_first=False)")
        sa = layer.self_attn
        if sa.in_proj_weight is None:
            raise ValueError("separate q/k/v projection weights are not supported")
        out += [sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias,
                layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias,
                layer.norm1.weight, layer.norm1.bias, layer.norm2.weight, layer.norm2.bias]
    return out


class TranslatorMixin:
    """Adds the HIP encoder call to an nn.Module. `egx_compute` in {"f32", "bf16", "f32s"}; `egx_impl` in
    {"auto", "generic", "fused"}."""

    # default arithmetic (round 6): "f32s" = fp32 operands split exactly into three bf16 parts, six bf16 MFMAs per K-block, fp32 accumulation —
    # fp32-grade results (2e-6 on the logits against fp64, tests/test_gpu_translator.py::test_split_bf16_mode_is_fp32_grade) at 2.7x the matrix
    # rate of the exact fp32 MFMA; implemented by the per-clip d = 128 kernels, everywhere else it computes as "f32". set_compute("f32") is the
    # exact v_mfma_f32_16x16x4_f32 path, "bf16" the BASELINE.json configs[2..4] arithmetic.
    egx_compute: str = "f32s"
    egx_impl: str = "auto"
    egx_defer_small: bool = False      # staged backward for the all-reduce overlap (ddp.allreduce_gradients_overlapped)
    egx_deterministic: bool = False    # fixed-order reductions in the backward (egx_config.deterministic)
    _egx_step: int = 0

    def set_compute(self, compute: str = "f32", impl: str = "auto"):
        assert compute in F_egx.COMPUTE and impl in F_egx.IMPL
        self.egx_compute, self.egx_impl = compute, impl
        return self

    def set_deterministic(self, on: bool = True):
        """Bit-identical gradients run to run (same inputs, same seed): the fused per-clip backward replaces its fp32-atomic
        cross-workgroup sums by fixed-order slab reductions, the shape-generic backward routes split-K weight gradients and
        LayerNorm / bias / pooled-head parameter gradients through partial buffers with ordered sums; the wide bf16 path is
        deterministic by construction."""
        self.egx_deterministic = bool(on)
        return self

    def enable_weight_cache(self, frozen: bool = False):
        """Keep the MFMA-fragment-packed weight copies of the per-clip / tiled kernels in a persistent buffer and skip the packing launch
        of every forward whose weights did not change since the previous one (functional.WeightCache: decided on storage addresses,
        version counters and functional.note_weights_changed(); FusedAdam and GraphedStep call the latter). Writes that bypass those
        (`p.data.add_()`) need invalidate_weight_cache(). frozen=True additionally promises that the weights stay as they are while it is
        set (inference, a forward + backward benchmark): only then is the packing launch left out of a captured hipGraph as well, and the
        device-resident dropout seed is advanced by the backward (no launch in front of the forward at all)."""
        self._egx_wcache = F_egx.WeightCache(frozen=frozen)
        return self

    def disable_weight_cache(self):
        self._egx_wcache = None
        return self

    def invalidate_weight_cache(self):
        wc = getattr(self, "_egx_wcache", None)
        if wc is not None:
            wc.invalidate()
        return self

    def enable_device_seed(self, device=None):
        """Keep the dropout seed in device memory and advance it on the stream every training forward, so that a
        captured hipGraph (torch.cuda.graph around forward+backward) draws fresh masks on every replay."""
        dev = device or next(self.parameters()).device
        self._egx_seed_dev = torch.tensor([torch.initial_seed() & (2**62 - 1)], dtype=torch.int64, device=dev)
        return self

    def _egx_seed(self) -> int:
        # counter-based: one fresh dropout key per forward, no device sync
        self._egx_step += 1
        return (torch.initial_seed() * 0x9E3779B97F4A7C15 + self._egx_step * 0xD1B54A32D192ED03) & (2**63 - 1)

    def _egx_spec(self, segments, encoder: nn.TransformerEncoder, ln: nn.LayerNorm, projs, head, **call):
        """(EncoderSpec, projection tensors, head tensors) of an encoder call: the shapes of `encoder` / `ln` / `head`, the model's compute and
        implementation, and the call's own fields (`call`)."""
        layer0 = encoder.layers[0]
        # impl "auto": functional.EncoderFn steers around the fused kernels when a learned `pe` needs a gradient
        spec = EncoderSpec(d_model=ln.normalized_shape[0], n_heads=layer0.self_attn.num_heads, d_ff=layer0.linear1.out_features,
                           n_layers=len(encoder.layers), segments=segments, ln_eps=ln.eps, compute=self.egx_compute, impl=self.egx_impl,
                           head_n_out=head[1].out_features if head is not None else 0, **call)
        proj_t = [t for s, p in zip(segments, projs) if s.has_proj for t in (p.weight, p.bias)]
        head_t = (head[0].weight, head[0].bias, head[1].weight, head[1].bias) if head is not None else ()
        return spec, proj_t, head_t

    def _egx_check_inference(self, what: str, subject: str = "ragged batches are"):
        """Inference-only features (ragged batches, greedy generation): eval mode, and no autograd graph over the parameters."""
        if self.training:
            raise ValueError(f"{subject} inference-only: call model.eval() before passing {what}")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise ValueError(f"{subject} inference-only: run them under torch.no_grad() / torch.inference_mode() "
                             "(or with every parameter frozen)")

    # ---- the encoder's self-attention weights (functional.AttentionRecorder, egx_encoder_self_weights) ----
    @contextlib.contextmanager
    def record_attention(self, weights: bool = True, by_segment: bool = True, rollout: bool = False, layers=None, max_bytes: int = 1 << 30):
        """Context manager: while active, every encoder call of this model (forward, forward_features, the EgoT2-g encode / predict*, the
        d = 128 forward_features(..., lengths=) / forward_features_ragged(..., lengths=) with host lengths) also records the head-averaged
        self-attention weights of its encoder layers, what a forward hook on a patched reference layer (self_attn(..., need_weights=True))
        sees. Yields the recorder; each call appends one functional.AttentionRecord to its `records`: weights (L', B, S, S), by_segment
        (L', B, S, K) = the weights summed over every auxiliary task's tokens, rollout (B, S, S) and rollout_by_segment (B, S, K) (attention
        rollout over all layers), segments (the per-clip segment lengths), impl. layers: the layers to return (default: all). A ragged batch:
        S = max_b S_b, zeros beyond each clip. The calls return the bits they return without it and issue the same launches, followed by one
        launch per recorded layer (and the rollout's). Inference only (eval mode, no autograd graph), as return_attention in the decoder:
        ValueError otherwise. A call whose outputs plus scratch exceed max_bytes raises ValueError naming the sizes before any device work
        (layers= and weights=False are the ways down); configurations the library does not serve raise ValueError with its text."""
        rec = F_egx.AttentionRecorder(weights, by_segment, rollout, layers, max_bytes)
        self._egx_check_recording()
        prev, self._egx_recorder = getattr(self, "_egx_recorder", None), rec
        try:
            yield rec
        finally:
            self._egx_recorder = prev

    def _egx_check_recording(self):
        if self.training:
            raise ValueError("record_attention is inference-only: call model.eval() first (the reference's train-mode weights are post-dropout "
                             "and are not modelled)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise ValueError("record_attention is inference-only: run it under torch.no_grad() / torch.inference_mode() (or with every "
                             "parameter frozen)")

    def _egx_attention_unserved(self, what: str):
        """For the encoder paths egx_encoder_self_weights does not serve: a ValueError while record_attention is active."""
        if getattr(self, "_egx_recorder", None) is not None:
            raise ValueError(f"record_attention: {what} is not served (egx_encoder_self_weights)")

    def _egx_recorded(self, feats, segments, encoder, lengths, call):
        """Run `call` (an encoder call of this model) under the model's recorder: the host checks first, no device work on a refusal."""
        rec = self._egx_recorder
        self._egx_check_recording()
        B = feats[0].shape[0]
        if lengths is None:
            S = sum(s.T for s in segments)
        elif isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            raise ValueError("record_attention: the capacity form of a ragged batch (device lengths) is not served (egx_encoder_self_weights)")
        else:
            S = int(F_egx.ragged_lengths(lengths, B, [s.T for s in segments]).sum(1).max())
        layer0 = encoder.layers[0] if len(encoder.layers) else None
        rec.plan(B, S, len(segments), len(encoder.layers), layer0.self_attn.embed_dim if layer0 is not None else 0,
                 layer0.self_attn.num_heads if layer0 is not None else 1)
        with rec:
            return call()

    def _egx_encode(self, feats: Sequence[torch.Tensor], segments: List[SegmentSpec], *, encoder: nn.TransformerEncoder,
                    ln: nn.LayerNorm, projs: Sequence[Optional[nn.Linear]], task_embed: Optional[torch.Tensor],
                    pos_table: Optional[torch.Tensor], p_drop: float, p_pos: float = 0.0, p_feat: float = 0.0,
                    head=None, out_tokens: int = 0, ce=None, token_ce=None, lengths=None) -> torch.Tensor:
        """head = (nn.LayerNorm, nn.Linear): evaluate the pooled head with the encoder and return logits (B, n_out).
        out_tokens = T > 0: return only the first T tokens of every clip, (B, T, d) (in-kernel on the fused path).
        ce = (target, class_weight | None) with a head: also evaluate nn.CrossEntropyLoss(weight)(logits, target) inside the forward
        (egx_ce) and return (logits, loss).
        token_ce = (fc_weight, fc_bias | None, target, class_weight | None) with out_tokens: return (loss, logits, probs, pred, correct) of the
        per-token classifier + weighted cross entropy on the returned tokens instead of the tokens (functional.encoder_token_ce).
        lengths: a ragged batch (inference only): (B,) or (B, K) frame counts in SEGMENT order (functional.ragged_lengths) of the padded
        feats; returns logits (B, n_out) with a head, else the first segment's rows of every clip packed, (sum_b T_{b,0}, d)
        (functional.encoder_ragged). out_tokens is then ignored: the first segment is what leaves the call."""
        if getattr(self, "_egx_recorder", None) is not None and F_egx._attention_sink is not self._egx_recorder:
            return self._egx_recorded(feats, segments, encoder, lengths, lambda: self._egx_encode(
                feats, segments, encoder=encoder, ln=ln, projs=projs, task_embed=task_embed, pos_table=pos_table, p_drop=p_drop, p_pos=p_pos,
                p_feat=p_feat, head=head, out_tokens=out_tokens, ce=ce, token_ce=token_ce, lengths=lengths))
        if lengths is not None:
            return self._egx_encode_ragged(feats, segments, lengths, encoder=encoder, ln=ln, projs=projs, task_embed=task_embed,
                                           pos_table=pos_table, head=head, ce=ce, token_ce=token_ce)
        seed_dev = getattr(self, "_egx_seed_dev", None)
        wcache = getattr(self, "_egx_wcache", None)
        # device seed: advanced by the forward's first launch (1) or, with a frozen weight cache (no launch in front of the forward), by the
        # backward behind its last reader (2)
        adv = 0 if (seed_dev is None or not self.training) else (2 if (wcache is not None and wcache.frozen and torch.is_grad_enabled()) else 1)
        spec, proj_t, head_t = self._egx_spec(segments, encoder, ln, projs, head, p_drop=p_drop, p_pos=p_pos, p_feat=p_feat,
                                              training=bool(self.training), seed=self._egx_seed() if self.training else 0,
                                              seed_ptr=seed_dev.data_ptr() if seed_dev is not None else 0,
                                              advance_seed=adv,   # fresh masks per (replayed) step
                                              defer_small=bool(self.egx_defer_small), deterministic=bool(self.egx_deterministic),
                                              out_tokens=int(out_tokens), wcache=wcache, ce=ce is not None)
        if ce is not None and head is None:
            raise ValueError("the fused cross entropy needs the pooled head")
        if token_ce is not None:
            if head is not None or not out_tokens:
                raise ValueError("the token classifier works on the first out_tokens tokens of every clip, without the pooled head")
            return F_egx.encoder_token_ce(spec, list(feats), task_embed, pos_table, ln.weight, ln.bias, proj_t,
                                          encoder_layer_tensors(encoder), *token_ce)
        return F_egx.encoder(spec, list(feats), task_embed, pos_table, ln.weight, ln.bias, proj_t,
                             encoder_layer_tensors(encoder), head_t, ce=ce)

    def _egx_encode_ragged(self, feats, segments, lengths, *, encoder, ln, projs, task_embed, pos_table, head, ce, token_ce):
        self._egx_check_inference("lengths=")
        if ce is not None or token_ce is not None:
            raise ValueError("ragged batches are inference-only: no fused loss (target= / lossav=); apply the loss to the returned outputs")
        lens = F_egx.ragged_lengths(lengths, feats[0].shape[0], [s.T for s in segments])
        spec, proj_t, head_t = self._egx_spec(segments, encoder, ln, projs, head, wcache=getattr(self, "_egx_wcache", None))
        return F_egx.encoder_ragged(spec, list(feats), lens, task_embed, pos_table, ln.weight, ln.bias, proj_t,
                                    encoder_layer_tensors(encoder), head_t)

    def _egx_train_ragged(self, feats, segments, lengths, *, encoder, ln, projs, task_embed, pos_table, p_drop, p_pos=0.0, head=None,
                          ce=None, capacity=None, status=None):
        """Ragged batch through the differentiable path (functional.encoder_ragged_train), in train and eval mode, with and without grad.
        `lengths`: (B, K) int32 host tensor in SEGMENT order (functional.ragged_lengths) - or, with capacity = (B_cap, tok_cap) and a status
        word, the (B_cap, K) int32 DEVICE tensor of the capturable form."""
        if getattr(self, "_egx_recorder", None) is not None and F_egx._attention_sink is not self._egx_recorder:
            return self._egx_recorded(feats, segments, encoder, lengths, lambda: self._egx_train_ragged(
                feats, segments, lengths, encoder=encoder, ln=ln, projs=projs, task_embed=task_embed, pos_table=pos_table, p_drop=p_drop,
                p_pos=p_pos, head=head, ce=ce, capacity=capacity, status=status))
        if self.egx_defer_small:
            raise ValueError("ragged training: the staged backward (egx_defer_small) is not supported; clear it for ragged batches")
        if ce is not None and head is None:
            raise ValueError("the fused cross entropy needs the pooled head")
        seed_dev = getattr(self, "_egx_seed_dev", None)
        training = bool(self.training)
        spec, proj_t, head_t = self._egx_spec(segments, encoder, ln, projs, head, p_drop=p_drop, p_pos=p_pos, training=training,
                                              seed=self._egx_seed() if training else 0,
                                              seed_ptr=seed_dev.data_ptr() if seed_dev is not None else 0,
                                              advance_seed=1 if (seed_dev is not None and training) else 0,     # fresh masks per call
                                              deterministic=bool(self.egx_deterministic), ce=ce is not None)
        return F_egx.encoder_ragged_train(spec, list(feats), lengths, task_embed, pos_table, ln.weight, ln.bias, proj_t,
                                          encoder_layer_tensors(encoder), head_t, ce=ce, capacity=capacity, status=status)
