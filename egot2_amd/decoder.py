"""The EgoT2-g sequence decoder + vocabulary head on libegot2x.so: decode() of
HHI/models/multitask/task_prompt_model.py:260-269 and HOI/models/multitask/video_model_builder.py:150-159.

`embedding(y) * sqrt(d)` + positional encoding -> nn.TransformerDecoder of CustomDecoderLayer (post-LN: causal
self-attention over the 2..5 target tokens, cross-attention onto the encoder memory, ReLU FFN) -> `fc`. The nn modules
are parameter containers only; projections / FFN run through the MFMA GEMM (egx_linear_*), LayerNorms through
egx_layernorm_*, the two attentions through egx_small_attention_* (at most 8 target tokens) or egx_target_attention_* (9 .. 64, behind
DecoderMixin.egx_long_targets) and the embedding through egx_embed_pos_*."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn as nn

from . import functional as F_egx

_SITE0 = 0x4000     # decoder dropout sites live above the encoder's (layer << 8 | site)


class DecoderMixin:
    # decode() of 9 .. 64 target tokens WITH autograd (the reference's training_step over 21- and 40-token targets: model(video,
    # target[:, :-1], 'lta_verb'), HOI/tasks/multitask/video_task_action.py:34-53) runs the composed fp32 decoder on egx_target_attention_*
    # when this is set (last_decoder_impl() == "composed_long"): train mode, eval mode with autograd, and eval under no_grad where
    # egx_decoder_forced does not serve the configuration. Off by default, as hoi_multitask's egx_generate is: with it off, and for at most 8
    # tokens in either state, every call is what it was, down to the exception text. Its attention masks are keyed with row stride 64.
    egx_long_targets = False

    def _egx_decoder_args(self, decoder: nn.TransformerDecoder, pos_embed, n_heads: int, p_drop: float):
        """(meta, 18 tensors per layer) of a fused decoder call (DecoderFn, RaggedDecoderFn, functional.decoder_ragged)."""
        train = bool(self.training)
        meta = dict(n_layers=len(decoder.layers), n_heads=n_heads, d_ff=decoder.layers[0].linear1.out_features, ln_eps=decoder.layers[0].norm1.eps,
                    p_drop=p_drop if train else 0.0, p_pos=pos_embed.dropout.p if train else 0.0, training=train,
                    seed=self._egx_seed() if train else 0,
                    seed_ptr=(self._egx_seed_dev.data_ptr() if train and getattr(self, "_egx_seed_dev", None) is not None else 0))
        params = []
        for layer in decoder.layers:
            sa, ca = layer.self_attn, layer.multihead_attn
            params += [sa.in_proj_weight, sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, layer.norm1.weight, layer.norm1.bias,
                       ca.in_proj_weight, ca.in_proj_bias, ca.out_proj.weight, ca.out_proj.bias, layer.norm2.weight, layer.norm2.bias,
                       layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm3.weight, layer.norm3.bias]
        return meta, params

    def _egx_fused_decoder_ok(self, decoder: nn.TransformerDecoder, d: int, n_heads: int, sy: int, S: int) -> bool:
        post_ln = not any(getattr(layer, "norm_first", False) for layer in decoder.layers)
        return (post_ln and F_egx.decoder_supported(getattr(self, "egx_compute", "f32"), d, n_heads, decoder.layers[0].linear1.out_features, sy, S,
                                                    len(decoder.layers))
                and not getattr(self, "egx_composed_decoder", False))

    def _egx_decode(self, y: torch.Tensor, encoded_x: torch.Tensor, *, embedding: nn.Embedding, pos_embed, decoder: nn.TransformerDecoder,
                    fc: nn.Linear, n_heads: int, p_drop: float, return_attention: bool = False):
        """y (B, sy) int64, encoded_x (S, B, d) decoder memory -> (sy, B, |V|) logits, as the reference's decode().
        return_attention (eval mode, no autograd): (logits, attn), attn (L, B, sy, S) fp32 the head-averaged cross-attention weights of
        every layer, what a forward hook on the reference's CustomDecoderLayer.multihead_attn sees (task_prompt_model.py:163-172). Fused
        path: egx_decoder_cross_weights on the forward's `saved`; composed path: egx_cross_attention_weights on the q / kv tensors of the
        loop. The logits are the bits of the call without the flag; last_decoder_impl() reads as without it."""
        S, B, d = encoded_x.shape
        sy = y.shape[1]
        if y.shape[0] != B:
            raise ValueError(f"target batch {y.shape[0]} != memory batch {B}")
        if return_attention:
            self._egx_check_inference("return_attention=True", subject="attention weights are")
            if n_heads < 1 or d % n_heads:
                raise ValueError(f"d_model {d} is not a multiple of {n_heads} heads")
            F_egx.check_cross_weights(d // n_heads, S)
            with torch.no_grad():
                return self._egx_decode_impl(y, encoded_x, embedding, pos_embed, decoder, fc, n_heads, p_drop, True)
        return self._egx_decode_impl(y, encoded_x, embedding, pos_embed, decoder, fc, n_heads, p_drop, False)

    def _egx_decode_impl(self, y, encoded_x, embedding, pos_embed, decoder, fc, n_heads, p_drop, want_attn: bool):
        S, B, d = encoded_x.shape
        sy = y.shape[1]
        if self._egx_fused_decoder_ok(decoder, d, n_heads, sy, S):
            # ONE library call per direction (egx_decoder_fwd / egx_decoder_bwd): bf16 MFMA GEMMs over all B * sy target rows
            meta, params = self._egx_decoder_args(decoder, pos_embed, n_heads, p_drop)
            mem2d = encoded_x.permute(1, 0, 2).contiguous().view(B * S, d)
            F_egx._last_dec_impl[0] = "fused"
            if want_attn:
                out, attn = F_egx.decoder_attention(meta, y, mem2d, embedding.weight, pos_embed.pe[:sy, 0, :], params, fc.weight, fc.bias)
                return out.view(B, sy, -1).permute(1, 0, 2), attn
            out = F_egx.DecoderFn.apply(meta, y, mem2d, embedding.weight, pos_embed.pe[:sy, 0, :], *params, fc.weight, fc.bias)
            return out.view(B, sy, -1).permute(1, 0, 2)
        if (9 <= sy <= 64 and not want_attn and not self.training and not torch.is_grad_enabled()
                and self._egx_fused_decoder_ok(decoder, d, n_heads, 1, S)
                and F_egx.decoder_forced_supported(getattr(self, "egx_compute", "f32"), d, n_heads, decoder.layers[0].linear1.out_features, S,
                                                   len(decoder.layers), embedding.weight.shape[0], sy, 1)):
            # 9 .. 64 target tokens at inference (the validation step's model(video, target[:, :-1], task)): the fused decoder stops at 8
            # rows, so the rows run one at a time through the K/V-cached step, ONE egx_decoder_forced call
            return self._egx_forced(encoded_x, y[:, None, :], None, True, embedding, pos_embed, decoder, fc, n_heads)[0].view(sy, B, -1)
        # 9 .. 64 target tokens where the forced route above did not take the call (opt-in): the loop below with the 64-row attention
        long_targets = bool(getattr(self, "egx_long_targets", False)) and sy > 8 and not want_attn
        if long_targets and not F_egx.decoder_long_supported(d, n_heads, sy, S):
            raise ValueError(f"decode() with egx_long_targets serves 9..64 target tokens, head dim <= 128 and 1..1024 memory tokens: got "
                             f"sy = {sy}, d = {d}, {n_heads} heads, S = {S}")
        self_attn, cross_attn = ((F_egx.SelfAttnTargetFn, F_egx.CrossAttnTargetFn) if long_targets
                                 else (F_egx.SelfAttnSmallFn, F_egx.CrossAttnSmallFn))
        comp = "f32"        # (B * sy)-row GEMMs: negligible work, they always run the exact fp32 MFMA path
        comp_mem = getattr(self, "egx_compute", "f32")     # the K / V projection of the (B * S)-row memory follows the encoder's compute type
        train = bool(self.training)
        # bias gradients summed in a fixed order: with the counter-based masks, a training step of this path repeats bit for bit under its seed
        lin = functools.partial(F_egx.linear, ordered_bias=True)
        seed = self._egx_seed() if train else 0
        mem2d = encoded_x.permute(1, 0, 2).contiguous().view(B * S, d)          # batch-first rows b * S + s
        x = F_egx.EmbedPosFn.apply(y, embedding.weight, pos_embed.pe[:, 0, :], math.sqrt(d),
                                   pos_embed.dropout.p if train else 0.0, seed)
        attn = []
        for li, layer in enumerate(decoder.layers):
            if getattr(layer, "norm_first", False):
                raise ValueError("libegot2x implements the post-LN decoder layer only (norm_first=False)")
            site = lambda k: _SITE0 + (li << 8) + k  # noqa: E731
            p = p_drop if train else 0.0
            sa, ca = layer.self_attn, layer.multihead_attn
            qkv = lin(x, sa.in_proj_weight, sa.in_proj_bias, comp)
            a = self_attn.apply(qkv, B, sy, n_heads, True, p, seed, site(1))
            a = F_egx.dropout(lin(a, sa.out_proj.weight, sa.out_proj.bias, comp), p_drop, train, seed, site(2))
            x = F_egx.layer_norm_residual(x, a, layer.norm1.weight, layer.norm1.bias, layer.norm1.eps)
            q = lin(x, ca.in_proj_weight[:d], ca.in_proj_bias[:d], comp)
            kv = lin(mem2d, ca.in_proj_weight[d:], ca.in_proj_bias[d:], comp_mem)
            c = cross_attn.apply(q, kv, B, sy, S, n_heads, p, seed, site(3))
            if want_attn:
                attn.append(F_egx.cross_attention_weights(q, kv[:, :d], n_heads, sy, S))
            c = F_egx.dropout(lin(c, ca.out_proj.weight, ca.out_proj.bias, comp), p_drop, train, seed, site(4))
            x = F_egx.layer_norm_residual(x, c, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps)
            h = F_egx.dropout(lin(x, layer.linear1.weight, layer.linear1.bias, comp, relu=True), p_drop, train, seed, site(5))
            f = F_egx.dropout(lin(h, layer.linear2.weight, layer.linear2.bias, comp), p_drop, train, seed, site(6))
            x = F_egx.layer_norm_residual(x, f, layer.norm3.weight, layer.norm3.bias, layer.norm3.eps)
        out = lin(x, fc.weight, fc.bias, comp)                         # (B * sy, |V|)
        F_egx._last_dec_impl[0] = "composed_long" if long_targets else "composed"
        if want_attn:
            return out.view(B, sy, -1).permute(1, 0, 2), torch.stack(attn, 0)
        return out.view(B, sy, -1).permute(1, 0, 2)

    def _egx_decode_ragged(self, y: torch.Tensor, memory: torch.Tensor, memory_lengths, *, embedding: nn.Embedding, pos_embed,
                           decoder: nn.TransformerDecoder, fc: nn.Linear, n_heads: int, p_drop: float, return_attention: bool = False):
        """Inference decode over a packed ragged memory: y (B, sy) int64, memory (sum_b S_b, d), memory_lengths (B,) with S_b rows for
        clip b -> (sy, B, |V|), each clip's logits as decode() gives them on its own (S_b, 1, d) memory. One egx_decoder_ragged_fwd call
        where the fused decoder serves the shapes (last_decoder_impl() == "ragged"); elsewhere one _egx_decode per memory length ("grouped").
        return_attention: (logits, attn (L, B, sy, max_b S_b) fp32), zeros beyond S_b: one egx_decoder_cross_weights call on the ragged
        workspace; grouped: each length group's weights scattered into place."""
        self._egx_check_inference("memory_lengths=")
        return self._egx_decode_packed(y, memory, memory_lengths, embedding=embedding, pos_embed=pos_embed, decoder=decoder, fc=fc,
                                       n_heads=n_heads, p_drop=p_drop, inference=True, want_attn=bool(return_attention))

    def _egx_decode_ragged_train(self, y: torch.Tensor, memory: torch.Tensor, memory_lengths, *, embedding: nn.Embedding, pos_embed,
                                 decoder: nn.TransformerDecoder, fc: nn.Linear, n_heads: int, p_drop: float) -> torch.Tensor:
        """Differentiable decode over a packed ragged memory, in train and eval mode: y (B, sy) int64, memory (sum_b S_b, d), memory_lengths
        (B,) -> (sy, B, |V|); gradients reach the decoder, the embedding, `fc` and the packed memory. One egx_decoder_ragged_train_fwd /
        egx_decoder_ragged_bwd pair where the fused decoder serves the shapes (last_decoder_impl() == "ragged"); elsewhere one differentiable
        _egx_decode per memory length ("grouped"), whose dropout masks differ from the ragged kernels'. Validation is host work and runs first."""
        return self._egx_decode_packed(y, memory, memory_lengths, embedding=embedding, pos_embed=pos_embed, decoder=decoder, fc=fc,
                                       n_heads=n_heads, p_drop=p_drop, inference=False)

    def _egx_decode_packed(self, y, memory, memory_lengths, *, embedding, pos_embed, decoder, fc, n_heads, p_drop, inference: bool,
                           want_attn: bool = False):
        """_egx_decode_ragged (inference: functional.decoder_ragged, no autograd) and _egx_decode_ragged_train (RaggedDecoderFn)."""
        B, sy = y.shape
        d = memory.shape[-1]
        ml = memory_lengths.detach() if isinstance(memory_lengths, torch.Tensor) else torch.as_tensor(memory_lengths)
        if ml.dtype.is_floating_point or ml.dtype.is_complex or ml.dtype == torch.bool:
            raise ValueError(f"memory_lengths must be integers, got {ml.dtype}")
        ml = ml.to("cpu", torch.int64)
        if ml.dim() != 1 or ml.shape[0] != B:
            raise ValueError(f"memory_lengths has shape {tuple(ml.shape)}: expected ({B},), one memory length per target row")
        if memory.dim() != 2 or (B and (int(ml.min()) < 1 or int(ml.sum()) != memory.shape[0])):
            raise ValueError(f"memory must be the packed (sum_b S_b, d) rows of the clips: {tuple(memory.shape)} rows, lengths sum to "
                             f"{int(ml.sum())} (each >= 1)")
        S_max = int(ml.max()) if B else 1
        if want_attn:
            if n_heads < 1 or d % n_heads:
                raise ValueError(f"d_model {d} is not a multiple of {n_heads} heads")
            F_egx.check_cross_weights(d // n_heads, S_max)
        # (head dim 256 / 512 has no ragged kernels: its clips run grouped by memory length, each group one fused call)
        if (self._egx_fused_decoder_ok(decoder, d, n_heads, sy, S_max)
                and F_egx.decoder_ragged_supported(getattr(self, "egx_compute", "f32"), d, n_heads, decoder.layers[0].linear1.out_features, sy, S_max,
                                                   len(decoder.layers))):
            meta, params = self._egx_decoder_args(decoder, pos_embed, n_heads, p_drop)
            args = (meta, y, memory, ml.to(torch.int32), embedding.weight, pos_embed.pe[:sy, 0, :])
            if want_attn:
                out, attn = F_egx.decoder_ragged(*args, params, fc.weight, fc.bias, return_attention=True)
                return out.view(B, sy, -1).permute(1, 0, 2), attn
            if inference:
                out = F_egx.decoder_ragged(*args, params, fc.weight, fc.bias)
            else:
                out = F_egx.RaggedDecoderFn.apply(*args, *params, fc.weight, fc.bias)
            return out.view(B, sy, -1).permute(1, 0, 2)
        # grouped: one decode per memory length, on (S, G, d) memories gathered from the packed rows (differentiable)
        row0 = torch.cumsum(ml, 0) - ml
        groups = {}
        for b, S in enumerate(ml.tolist()):
            groups.setdefault(S, []).append(b)
        parts, order = [], []
        attn = torch.zeros((len(decoder.layers), B, sy, S_max), dtype=torch.float32, device=memory.device) if want_attn else None
        for S, idx in groups.items():
            rows = (row0[idx][:, None] + torch.arange(S)[None, :]).reshape(-1).to(memory.device)
            mem = memory.index_select(0, rows).view(len(idx), S, d).permute(1, 0, 2)
            it = torch.tensor(idx, dtype=torch.int64, device=y.device)
            part = self._egx_decode(y.index_select(0, it), mem, embedding=embedding, pos_embed=pos_embed, decoder=decoder, fc=fc,
                                    n_heads=n_heads, p_drop=p_drop, return_attention=want_attn)
            if want_attn:
                part, w = part
                attn[:, it.to(attn.device), :, :S] = w
            parts.append(part)
            order += idx
        inv = torch.empty(B, dtype=torch.int64)
        inv[torch.tensor(order, dtype=torch.int64)] = torch.arange(B)
        out = torch.cat(parts, 1).index_select(1, inv.to(parts[0].device))
        F_egx._last_dec_impl[0] = "grouped"
        return (out, attn) if want_attn else out

    @staticmethod
    def _egx_check_generation(start, encoded_x, n_steps, embedding, pos_embed, what: str):
        """The argument checks greedy generation and beam search share (host work only); returns (S, B, d) of the memory."""
        if not isinstance(n_steps, int) or isinstance(n_steps, bool) or n_steps < 1:
            raise ValueError(f"n_steps must be a positive int, got {n_steps!r}")
        if not isinstance(encoded_x, torch.Tensor) or encoded_x.dim() != 3:
            raise ValueError("encoded_x must be the (S, B, d) decoder memory")
        S, B, d = encoded_x.shape
        if not isinstance(start, torch.Tensor) or start.dim() != 1 or start.shape[0] != B:
            raise ValueError(f"start must be a ({B},) tensor, one start token per clip of the memory: got "
                             f"{tuple(start.shape) if isinstance(start, torch.Tensor) else type(start).__name__}")
        if start.dtype != torch.int64:
            raise ValueError(f"start must be int64 tokens, got {start.dtype}")
        if n_steps > pos_embed.pe.shape[0]:
            raise ValueError(f"n_steps = {n_steps} exceeds the {pos_embed.pe.shape[0]} rows of the positional table")
        if d != embedding.weight.shape[1]:
            raise ValueError(f"memory width {d} != embedding width {embedding.weight.shape[1]}")
        if not (encoded_x.is_cuda and start.is_cuda and embedding.weight.is_cuda):
            raise ValueError(f"{what} runs on the GPU only (no CPU fallback): memory, start tokens and the model must be on the GPU")
        return S, B, d

    def _egx_greedy(self, start: torch.Tensor, encoded_x: torch.Tensor, n_steps: int, *, embedding: nn.Embedding, pos_embed,
                    decoder: nn.TransformerDecoder, fc: nn.Linear, n_heads: int, return_logits: bool = False, schedule=None,
                    return_attention: bool = False):
        """Greedy generation (inference only), the loop of predict_ac (HOI/models/multitask/video_model_builder.py:201-220, 263-274) and of
        HOI/models/lta/lta_models_seqdecoder.py:181-201: start (B,) int64 tokens, encoded_x (S, B, d) memory -> tokens (B, n_steps) int64 (the
        n_steps tokens after `start`) and, with return_logits, each step's last-row logits (n_steps, B, |V|). Ties go to the lowest index.
        One egx_decoder_generate call where it serves the configuration (last_decoder_impl() == "generate": K/V cache, argmax on the
        device, no host synchronisation); elsewhere the prefix loop over _egx_decode ("loop"). Validation is host work and runs first.
        `schedule` (a functional.TokenSchedule): step t takes its argmax over the words of row t % P, the other logits are -inf
        (egx_decoder_generate_sched; the prefix loop masks the same way).
        return_attention: a third result, attn (L, n_steps, B, S) fp32, step t's head-averaged cross-attention weights of every layer
        (egx_decoder_generate_attn; the prefix loop takes the last row of each step's decode weights)."""
        self._egx_check_inference("it to greedy_decode", subject="greedy generation is")
        V = embedding.weight.shape[0]
        if schedule is not None:
            F_egx.check_schedule(schedule, V)
        S, B, d = self._egx_check_generation(start, encoded_x, n_steps, embedding, pos_embed, "greedy generation")
        if schedule is not None:
            F_egx.check_schedule(schedule, V, encoded_x.device)
        if return_attention:
            if n_heads < 1 or d % n_heads:
                raise ValueError(f"d_model {d} is not a multiple of {n_heads} heads")
            F_egx.check_cross_weights(d // n_heads, S)
        post_ln = not any(getattr(layer, "norm_first", False) for layer in decoder.layers)
        if (post_ln and not getattr(self, "egx_composed_decoder", False)
                and F_egx.decoder_generate_supported(getattr(self, "egx_compute", "f32"), d, n_heads, decoder.layers[0].linear1.out_features, S,
                                                     len(decoder.layers), V, n_steps)):
            meta, params = self._egx_decoder_args(decoder, pos_embed, n_heads, 0.0)
            mem2d = encoded_x.permute(1, 0, 2).contiguous().view(B * S, d)
            return F_egx.decoder_generate(meta, start, mem2d, embedding.weight, pos_embed.pe[:n_steps, 0, :], params, fc.weight, fc.bias,
                                          n_steps, return_logits, schedule, return_attention)
        # the reference's prefix loop: one decode() per step over the growing prefix
        if n_steps > 8:
            raise ValueError(f"n_steps = {n_steps}: this configuration is outside egx_decoder_generate (compute bf16, vocabulary <= 1024, "
                             "n_steps <= 64, the fused decoder's shapes) and the prefix loop runs decode(), which serves at most 8 target tokens")
        with torch.no_grad():
            toks = torch.empty((B, n_steps + 1), dtype=torch.int64, device=start.device)
            toks[:, 0] = start
            rows, attn = [], []
            banned = None if schedule is None else ~schedule.allowed.to(start.device)
            for t in range(n_steps):
                last = self._egx_decode(toks[:, :t + 1], encoded_x, embedding=embedding, pos_embed=pos_embed, decoder=decoder, fc=fc,
                                        n_heads=n_heads, p_drop=0.0, return_attention=return_attention)
                if return_attention:
                    attn.append(last[1][:, :, t, :])                    # (L, B, S): the new row's weights
                    last = last[0]
                last = last[-1]
                if banned is not None:
                    last = last.masked_fill(banned[t % schedule.period], float("-inf"))
                toks[:, t + 1] = _argmax_lowest(last)
                if return_logits:
                    rows.append(last)
        F_egx._last_dec_impl[0] = "loop"
        out = (toks[:, 1:].contiguous(), (torch.stack(rows, 0).contiguous() if return_logits else None))
        return out + (torch.stack(attn, 1).contiguous(),) if return_attention else out

    def token_schedule(self, allowed: torch.Tensor) -> "F_egx.TokenSchedule":
        """A functional.TokenSchedule for greedy_decode / beam_decode on this model's device: `allowed` (P, V) bool, V the vocabulary of
        `embedding`; step t may emit the words of row t % P. Build it once (host validation, one upload) and reuse it."""
        V = self.embedding.weight.shape[0]
        if isinstance(allowed, torch.Tensor) and allowed.dim() == 2 and allowed.shape[1] != V:
            raise ValueError(f"allowed is over {allowed.shape[1]} words, the model's vocabulary has {V}")
        return F_egx.TokenSchedule(allowed, self.embedding.weight.device)

    def verb_noun_schedule(self, v_idx, n_idx) -> "F_egx.TokenSchedule":
        """The two-row schedule of the LTA outputs (HOI/models/lta/lta_models_seqdecoder.py:190-201) from the index arrays of
        vocab_idx_to_orig() (numpy arrays, lists or tensors; the sets may overlap): row 0, steps 0, 2, ..: the verb words v_idx; row 1,
        steps 1, 3, ..: the noun words n_idx."""
        V = self.embedding.weight.shape[0]
        allowed = torch.zeros((2, V), dtype=torch.bool)
        for row, (name, idx) in enumerate((("v_idx", v_idx), ("n_idx", n_idx))):
            idx = torch.as_tensor(idx).detach().to("cpu")
            if idx.numel() == 0:
                idx = idx.to(torch.int64).view(-1)                      # (an empty list arrives as float32; the empty row is refused below)
            if idx.dtype.is_floating_point or idx.dtype.is_complex or idx.dtype == torch.bool or idx.dim() != 1:
                raise ValueError(f"{name} must be a 1-D array of integer word indices, got {idx.dtype} of shape {tuple(idx.shape)}")
            idx = idx.to(torch.int64)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= V):
                raise ValueError(f"{name} holds an index outside the vocabulary of {V} words: {int(idx.min())} .. {int(idx.max())}")
            allowed[row, idx] = True
        return self.token_schedule(allowed)

    def greedy_decode(self, encoded_x: torch.Tensor, start_token, n_steps: int, return_logits: bool = False, schedule=None, *,
                      return_attention: bool = False):
        """Greedy generation from the (S, B, d) decoder memory: `start_token` an int or a (B,) int64 tensor; returns tokens (B, n_steps) and,
        with return_logits, (tokens, logits (n_steps, B, |V|)). `schedule` (token_schedule / verb_noun_schedule): step t's token is the
        argmax over the words of row t % P and the returned logits are -inf at every other word, so tokens == argmax(logits) still holds;
        the 40-step verb / noun reading of lta_models_seqdecoder.py:190-201 is verb_noun_schedule(v_idx, n_idx). One deliberate difference:
        the reference feeds back the full-vocabulary argmax and only reads the subset, a schedule feeds back the subset's argmax (the same
        word whenever the full argmax lies in the set). Without a schedule nothing changes. Eval mode only; see _egx_greedy.
        return_attention appends attn (L, n_steps, B, S) fp32 to the return value: per decoder layer and step the head-averaged
        cross-attention weights of the step's new row, what a hook on the reference's CustomDecoderLayer.multihead_attn
        (lta_models_seqdecoder.py:30-39) sees in the last row of step t; tokens and logits keep their bits. beam_decode has no such output
        (a hypothesis changes slots every step: return_trace is the tool there)."""
        start = _start_tokens(start_token, encoded_x)
        res = self._egx_greedy(start, encoded_x, n_steps, embedding=self.embedding, pos_embed=self.pos_embed,
                               decoder=self.transformer_decoder, fc=self.fc, n_heads=self.n_heads, return_logits=return_logits,
                               schedule=schedule, return_attention=bool(return_attention))
        out = (res[0],) + ((res[1],) if return_logits else ()) + ((res[2],) if return_attention else ())
        return out if len(out) > 1 else res[0]

    @staticmethod
    def attention_by_segment(attn: torch.Tensor, segment_lengths) -> torch.Tensor:
        """Sums the last axis of attention weights over consecutive memory segments: attn (..., S) -> (..., K). segment_lengths (K,) ints:
        the same split for every clip (the three T-token task blocks of the HHI 'ttm' memory: (T, T, T)); (B, K) ints: a split per clip
        for ragged memories, attn then (..., B, sy, S) as decode(..., memory_lengths=, return_attention=True) returns it. Segments start
        at key 0 and may stop short of S (the zero tail of a ragged clip). Pure torch."""
        if not isinstance(attn, torch.Tensor) or attn.dim() < 1 or not attn.dtype.is_floating_point:
            raise ValueError("attn must be a floating-point tensor whose last axis runs over the memory tokens")
        seg = segment_lengths.detach() if isinstance(segment_lengths, torch.Tensor) else torch.as_tensor(segment_lengths)
        if seg.dtype.is_floating_point or seg.dtype.is_complex or seg.dtype == torch.bool or seg.dim() not in (1, 2) or seg.shape[-1] < 1:
            raise ValueError(f"segment_lengths must be (K,) or (B, K) integers, got {seg.dtype} of shape {tuple(seg.shape)}")
        seg = seg.to("cpu", torch.int64)
        S = attn.shape[-1]
        if int(seg.min()) < 0 or int(seg.sum(dim=-1).max()) > S:
            raise ValueError(f"segment_lengths must be non-negative and sum to at most the {S} memory tokens of attn")
        if seg.dim() == 2 and (attn.dim() < 3 or attn.shape[-3] != seg.shape[0]):
            raise ValueError(f"(B, K) segment_lengths need attn of shape (..., B, sy, S) with B = {seg.shape[0]}, got {tuple(attn.shape)}")
        end = torch.cumsum(seg, dim=-1)
        first = end - seg
        j = torch.arange(S)
        member = ((j >= first[..., :, None]) & (j < end[..., :, None])).to(attn.dtype).to(attn.device)        # (K, S) or (B, K, S)
        if seg.dim() == 1:
            return attn @ member.t()
        return torch.einsum("...bis,bks->...bik", attn, member)

    def _egx_forced(self, encoded_x, y3, targets3, return_logits, embedding, pos_embed, decoder, fc, n_heads):
        """One functional.decoder_forced call on validated arguments: y3 / targets3 (B, K, sy) -> (logits (sy, B * K, |V|) or None, logprob
        (B, K, sy) or None)."""
        S, B, d = encoded_x.shape
        sy = y3.shape[2]
        meta, params = self._egx_decoder_args(decoder, pos_embed, n_heads, 0.0)
        mem2d = encoded_x.permute(1, 0, 2).contiguous().view(B * S, d)
        return F_egx.decoder_forced(meta, y3, targets3, mem2d, embedding.weight, pos_embed.pe[:sy, 0, :], params, fc.weight, fc.bias,
                                    return_logits)

    def forced_decode(self, encoded_x: torch.Tensor, y: torch.Tensor, targets: torch.Tensor = None, return_logits: bool = True, *,
                      return_attention: bool = False, memory_lengths=None):
        """Teacher-forced decoding of up to 64 target tokens from the (S, B, d) decoder memory (inference): y (B, sy) int64 input tokens on
        the GPU, 1 <= sy <= 64, or (B, K, sy) for K <= 8 sequences per clip on the clip's one memory (the K candidates of the LTA
        evaluation, the hypotheses beam_decode returns). Returns logits (sy, B, |V|), for a 3-D y (sy, B, K, |V|): row t is what decode()
        of y[..., :t + 1] gives in its last row, so forced_decode(memory, target[:, :-1]) is the reference's model(video, target[:, :-1],
        task) of a validation step (HOI/tasks/multitask/video_task.py:601-617) before its permute. With `targets` (the shape of y) also
        logprob, shaped like y: log_softmax(logits)[target] per position, exactly 0.0 where the target lies outside the vocabulary (padding
        such as -100), so -logprob.sum() / count is the cross entropy and logprob.sum(-1) a sequence's score. return_logits=False returns
        logprob alone and needs targets. One egx_decoder_forced call (last_decoder_impl() == "forced": the K/V-cached step of
        greedy_decode with the next row taken from y; fed greedy_decode's tokens it returns greedy_decode's logits bit for bit); the
        steps run one after the other, so this is for validation and scoring, not for training. Eval mode only; shapes and dtypes are
        validated on the host first, token values are never read there; outside the limits a ValueError that names them."""
        self._egx_check_inference("it to forced_decode", subject="teacher-forced decoding of up to 64 tokens is")
        if return_attention or memory_lengths is not None:
            raise ValueError("forced_decode serves neither return_attention nor memory_lengths: decode() returns attention weights and "
                             "takes ragged memories for at most 8 target tokens")
        if not isinstance(encoded_x, torch.Tensor) or encoded_x.dim() != 3:
            raise ValueError("encoded_x must be the (S, B, d) decoder memory")
        S, B, d = encoded_x.shape
        if not isinstance(y, torch.Tensor) or y.dim() not in (2, 3) or y.shape[0] != B:
            raise ValueError(f"y must be a ({B}, sy) or ({B}, K, sy) tensor of input tokens, one row (or K rows) per clip of the memory: got "
                             f"{tuple(y.shape) if isinstance(y, torch.Tensor) else type(y).__name__}")
        if y.dtype != torch.int64:
            raise ValueError(f"y must be int64 tokens, got {y.dtype}")
        K, sy = (y.shape[1] if y.dim() == 3 else 1), y.shape[-1]
        if not 1 <= K <= 8:
            raise ValueError(f"K = {K} sequences per clip: forced_decode serves 1..8")
        if not 1 <= sy <= 64:
            raise ValueError(f"sy = {sy} target tokens: forced_decode serves 1..64")
        if targets is not None:
            if not isinstance(targets, torch.Tensor) or targets.shape != y.shape:
                raise ValueError(f"targets must have the shape of y {tuple(y.shape)}, got "
                                 f"{tuple(targets.shape) if isinstance(targets, torch.Tensor) else type(targets).__name__}")
            if targets.dtype != torch.int64:
                raise ValueError(f"targets must be int64 tokens, got {targets.dtype}")
        elif not return_logits:
            raise ValueError("return_logits=False needs targets: without them nothing is left to return")
        embedding, decoder, pos_embed = self.embedding, self.transformer_decoder, self.pos_embed
        V = embedding.weight.shape[0]
        if sy > pos_embed.pe.shape[0]:
            raise ValueError(f"sy = {sy} exceeds the {pos_embed.pe.shape[0]} rows of the positional table")
        if d != embedding.weight.shape[1]:
            raise ValueError(f"memory width {d} != embedding width {embedding.weight.shape[1]}")
        if not (encoded_x.is_cuda and y.is_cuda and embedding.weight.is_cuda and (targets is None or targets.is_cuda)):
            raise ValueError("teacher-forced decoding runs on the GPU only (no CPU fallback): memory, tokens, targets and the model must be "
                             "on the GPU")
        compute, d_ff = getattr(self, "egx_compute", "f32"), decoder.layers[0].linear1.out_features
        post_ln = not any(getattr(layer, "norm_first", False) for layer in decoder.layers)
        if not (post_ln and F_egx.decoder_forced_supported(compute, d, self.n_heads, d_ff, S, len(decoder.layers), V, sy, K)):
            raise ValueError(f"teacher-forced decoding is outside egx_decoder_forced's limits (compute bf16, post-LN layers, d_model a multiple "
                             f"of 128 in [256, 1024], head dim 32 or 64 (or head dim 256 / 512 with d_model <= 2048 and S <= 16), d_ff a multiple of 128, S <= 1024, at most 16 layers, vocabulary <= "
                             f"1024, sy <= 64, K <= 8): got compute {compute}, d = {d}, {self.n_heads} heads, d_ff = {d_ff}, S = {S}, "
                             f"{len(decoder.layers)} layers, vocabulary {V}, sy = {sy}, K = {K}")
        y3, t3 = y.reshape(B, K, sy), (targets.reshape(B, K, sy) if targets is not None else None)
        logits, logprob = self._egx_forced(encoded_x, y3, t3, bool(return_logits), embedding, pos_embed, decoder, self.fc, self.n_heads)
        if logprob is not None:
            logprob = logprob.view(y.shape)
        if not return_logits:
            return logprob
        logits = logits.view((sy, B, K, V) if y.dim() == 3 else (sy, B, V))
        return (logits, logprob) if targets is not None else logits

    def beam_decode(self, encoded_x: torch.Tensor, start_token, n_steps: int, beam_width: int, return_scores: bool = False,
                    return_trace: bool = False, schedule=None):
        """Beam search from the (S, B, d) decoder memory: the `beam_width` best fixed-length continuations of `start_token` (an int or a (B,)
        int64 tensor) per clip, best first: tokens (B, beam_width, n_steps) int64; with return_scores also their scores (B, beam_width), the
        fp32 sums of log_softmax(logits)[token]; with return_trace also a functional.BeamTrace (step_tokens, step_parents, step_scores,
        step_logits). The K = 5 candidates of the LTA evaluation (HOI/tasks/lta/long_term_anticipation.py:233-388) are
        beam_decode(memory, start, 40, 5). One egx_decoder_beam call (last_decoder_impl() == "beam": K/V cache read through an ancestry
        table, ranking on the device, no host synchronisation); outside its limits a ValueError: there is no Python search to fall back on.
        `schedule` (token_schedule / verb_noun_schedule): at step t only the words of row t % P are candidates, log_softmax normalises
        over that set (as Categorical(logits=head_x[..., v_idx]) of lta_models_seqdecoder.py:190-216 does) and step_logits is -inf
        elsewhere; beam_width may not exceed the size of step 0's set. The LTA recipe is beam_decode(memory, start, 40, 5,
        schedule=model.verb_noun_schedule(v_idx, n_idx)). Unlike the reference, which feeds back the full-vocabulary argmax and only
        reads the subset, the fed-back words are the subset's. Eval mode only; validation is host work and runs first."""
        self._egx_check_inference("it to beam_decode", subject="beam search is")
        if not isinstance(beam_width, int) or isinstance(beam_width, bool) or not 1 <= beam_width <= 8:
            raise ValueError(f"beam_width must be an int in 1..8, got {beam_width!r}")
        embedding, decoder = self.embedding, self.transformer_decoder
        V = embedding.weight.shape[0]
        if beam_width > V:
            raise ValueError(f"beam_width = {beam_width} exceeds the vocabulary of {V} words")
        if schedule is not None:
            F_egx.check_schedule(schedule, V, None, beam_width)
        start = _start_tokens(start_token, encoded_x)
        S, B, d = self._egx_check_generation(start, encoded_x, n_steps, embedding, self.pos_embed, "beam search")
        compute, d_ff = getattr(self, "egx_compute", "f32"), decoder.layers[0].linear1.out_features
        post_ln = not any(getattr(layer, "norm_first", False) for layer in decoder.layers)
        if not (post_ln and F_egx.decoder_beam_supported(compute, d, self.n_heads, d_ff, S, len(decoder.layers), V, n_steps, beam_width)):
            raise ValueError(f"beam search is outside egx_decoder_beam's limits (compute bf16, post-LN layers, d_model a multiple of 128 in "
                             f"[256, 1024], head dim 32 or 64 (or head dim 256 / 512 with d_model <= 2048, S <= 16 and beam_width <= 4 at d_model 2048), d_ff a multiple of 128, S <= 1024, at most 16 layers, vocabulary <= 1024, "
                             f"n_steps <= 64, beam_width <= 8): got compute {compute}, d = {d}, {self.n_heads} heads, d_ff = {d_ff}, S = {S}, "
                             f"{len(decoder.layers)} layers, vocabulary {V}, n_steps = {n_steps}, beam_width = {beam_width}")
        if schedule is not None:
            F_egx.check_schedule(schedule, V, encoded_x.device, beam_width)          # (where its words live: the memory is a tensor by now)
        meta, params = self._egx_decoder_args(decoder, self.pos_embed, self.n_heads, 0.0)
        mem2d = encoded_x.permute(1, 0, 2).contiguous().view(B * S, d)
        tokens, scores, trace = F_egx.decoder_beam(meta, start, mem2d, embedding.weight, self.pos_embed.pe[:n_steps, 0, :], params, self.fc.weight,
                                                   self.fc.bias, n_steps, beam_width, return_trace, schedule)
        out = (tokens,) + ((scores,) if return_scores else ()) + ((trace,) if return_trace else ())
        return out if len(out) > 1 else tokens


def _start_tokens(start_token, encoded_x):
    """`start_token` of greedy_decode / beam_decode as a tensor: a (B,) tensor as it is, an int for every clip of the (S, B, d) memory."""
    if isinstance(start_token, torch.Tensor):
        start = start_token
    else:
        if not isinstance(start_token, int) or isinstance(start_token, bool):
            raise ValueError(f"start_token must be an int or a (B,) int64 tensor, got {type(start_token).__name__}")
        if not isinstance(encoded_x, torch.Tensor) or encoded_x.dim() != 3:
            raise ValueError("encoded_x must be the (S, B, d) decoder memory")
        start = torch.full((encoded_x.shape[1],), start_token, dtype=torch.int64, device=encoded_x.device)
    return start


def _argmax_lowest(logits: torch.Tensor) -> torch.Tensor:
    """Row argmax with the lowest index on ties (torch.argmax leaves ties open)."""
    V = logits.shape[-1]
    idx = torch.arange(V, device=logits.device).expand_as(logits)
    return torch.where(logits == logits.max(dim=-1, keepdim=True).values, idx, V).min(dim=-1).values
