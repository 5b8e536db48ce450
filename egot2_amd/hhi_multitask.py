"""EgoT2-g (HHI) — drop-in mirror of HHI/models/multitask/task_prompt_model.py:174-293
(`TaskTranslationPromptTransformer`). The shared task-translation ENCODER (the graded hot path)
runs in libegot2x.so; and so does the 2-token sequence decoder + vocabulary head (egot2_amd/decoder.py)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .backbones import freeze_params, make_backbone
from . import functional as F_egx
from .functional import SegmentSpec
from .decoder import DecoderMixin
from .translator import PositionalEncoding, TranslatorMixin, encoder_layer_tensors


class CustomDecoderLayer(nn.TransformerDecoderLayer):
    """task_prompt_model.py:163-172. need_weights=True is the one reason the reference subclasses the layer: a forward hook on
    `multihead_attn` then sees the head-averaged cross-attention weights (B, sy, S), which task's tokens at which time steps the task prompt
    reads. This module is a parameter container: the HIP decoder returns those weights through decode(..., return_attention=True) and
    greedy_decode(..., return_attention=True) (egot2_amd/decoder.py). The extra is_causal argument is what torch >= 2 passes."""

    def __init__(self, d_model, nhead, dropout=0.1):
        super().__init__(d_model, nhead, dropout=dropout)

    def _mha_block(self, x, mem, attn_mask, key_padding_mask, is_causal=False):
        x = self.multihead_attn(x, mem, mem, attn_mask=attn_mask, key_padding_mask=key_padding_mask, need_weights=True)[0]
        return self.dropout2(x)


class TaskTranslationPromptTransformer(nn.Module, TranslatorMixin, DecoderMixin):
    def __init__(self, args, vocab):
        super().__init__()
        self.args = args
        self.vocab = vocab
        self.n_tasks = 3
        self.dim = args.hidden_dim
        self.n_heads = args.num_heads
        self.num_layers = args.num_layers
        self.dp_rate = args.dropout
        self.max_output_length = 500
        self.transformer_encoder = nn.TransformerEncoder(   # parameter container only
            encoder_layer=nn.TransformerEncoderLayer(d_model=self.dim, nhead=self.n_heads, dropout=self.dp_rate),
            num_layers=self.num_layers
        )
        self.transformer_decoder = nn.TransformerDecoder(
            decoder_layer=CustomDecoderLayer(d_model=self.dim, nhead=self.n_heads, dropout=self.dp_rate),
            num_layers=self.num_layers
        )
        self.ln = nn.LayerNorm(self.dim)
        self.task_embed = nn.Parameter(torch.randn(1, self.n_tasks, self.dim), requires_grad=True)
        self.pos_embed = PositionalEncoding(self.dim, dropout=0.1)
        self.embedding = nn.Embedding(len(self.vocab), self.dim)
        self.proj_lam = nn.Linear(256, self.dim)
        self.proj_ttm = nn.Linear(256, self.dim)
        self.proj_asd = nn.Linear(256, self.dim)
        self.fc = nn.Linear(self.dim, len(self.vocab))
        self.seq_len = 2
        self.y_mask = self.get_tgt_mask(self.seq_len)   # plain attribute, not a buffer (as in the reference)
        self._init_parameters()
        if getattr(args, "lam_checkpoint", None):
            self.lam_model = make_backbone("lam", args.lam_checkpoint)
            freeze_params(self.lam_model)
        if getattr(args, "ttm_checkpoint", None):
            self.ttm_model = make_backbone("ttm", args.ttm_checkpoint)
            freeze_params(self.ttm_model)
        if getattr(args, "asd_checkpoint", None):
            self.asd_model = make_backbone("asd", args.asd_checkpoint)
            freeze_params(self.asd_model)

    def _init_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def get_tgt_mask(self, size) -> torch.Tensor:
        mask = torch.tril(torch.ones(size, size) == 1).float()
        mask = mask.masked_fill(mask == 0, float('-inf'))
        mask = mask.masked_fill(mask == 1, float(0.0))
        return mask

    # ---- encoder (HIP) ---------------------------------------------------------------------------------
    def encode_features(self, task, lam_feat, ttm_feat=None, asd_feat=None, lengths=None):
        """Backbone features -> decoder memory in the reference layout: (S, B, d), or (3, B*T, d) for 'asd'.

        lengths (inference only, functional.ragged_lengths): the features are padded batches of clips of their own lengths, (B,) or (B, K)
        frame counts in argument order (K = 1 for 'lam', else 3); padded frames are never read. Returns the packed memory of every clip,
        (sum_b S_b, d) with S_b = sum_k T_{b,k}, for 'ttm' / 'lam' (decode(..., memory_lengths=S_b)), and the reference's (3, sum_b T_b, d)
        for 'asd' (equal segment lengths per clip), a view of one frame-major buffer that decode() reads without a copy."""
        if lengths is not None:
            self._egx_check_inference("lengths=")
            return self._encode_ragged(task, lam_feat, ttm_feat, asd_feat, lengths, train=False)
        feats, segs, projs = self._encoder_segments(task, lam_feat, ttm_feat, asd_feat)
        x = self._egx_encode(feats, segs, encoder=self.transformer_encoder, ln=self.ln, projs=projs,
                             task_embed=self.task_embed, pos_table=self.pos_embed.pe,
                             p_drop=self.dp_rate, p_pos=self.pos_embed.dropout.p)   # (B, S, d)
        if task == 'asd':
            T = x.shape[1] // 3
            return torch.stack((x[:, 0:T].reshape(-1, self.dim), x[:, T:2 * T].reshape(-1, self.dim),
                                x[:, 2 * T:3 * T].reshape(-1, self.dim)), dim=0)
        return x.permute(1, 0, 2)

    def _encoder_segments(self, task, lam_feat, ttm_feat, asd_feat):
        """The features, their SegmentSpecs and projections of an encoder call of `task`."""
        if task == 'lam':
            feats, projs, ids = [lam_feat], [self.proj_lam], [0]
        else:
            feats, projs, ids = [lam_feat, ttm_feat, asd_feat], [self.proj_lam, self.proj_ttm, self.proj_asd], [0, 1, 2]
        segs = [SegmentSpec(T=f.shape[1], d_in=f.shape[2], has_proj=True, add_row=k, pos_row0=0) for f, k in zip(feats, ids)]
        return feats, segs, projs

    @staticmethod
    def _ragged_lengths(task, feats, lengths):
        """The (B, K) host lengths of a ragged batch of `task` (functional.ragged_lengths); 'asd' needs equal segment lengths in every clip."""
        lens = F_egx.ragged_lengths(lengths, feats[0].shape[0], [f.shape[1] for f in feats])
        if task == 'asd' and not bool((lens == lens[:, :1]).all()):
            b = int((lens != lens[:, :1]).any(1).nonzero()[0, 0])
            raise ValueError(f"task 'asd' needs lam, ttm and asd features of equal length in every clip (clip {b}: {lens[b].tolist()})")
        return lens

    def _encode_ragged(self, task, lam_feat, ttm_feat, asd_feat, lengths, *, train: bool):
        """encode_features(..., lengths=) (train False: functional.encoder_ragged_tokens) and encode_features_ragged (train True:
        functional.encoder_ragged_tokens_train). The lengths are checked (host work) before any device work."""
        self._egx_attention_unserved("a ragged batch on the wide path")
        feats, segs, projs = self._encoder_segments(task, lam_feat, ttm_feat, asd_feat)
        lens = self._ragged_lengths(task, feats, lengths)
        if train:
            if self.egx_defer_small:
                raise ValueError("ragged training: the staged backward (egx_defer_small) is not supported; clear it for ragged batches")
            seed_dev = getattr(self, "_egx_seed_dev", None)
            training = bool(self.training)
            spec, proj_t, _ = self._egx_spec(segs, self.transformer_encoder, self.ln, projs, None,
                                             p_drop=self.dp_rate if training else 0.0, p_pos=self.pos_embed.dropout.p if training else 0.0,
                                             training=training, seed=self._egx_seed() if training else 0,
                                             seed_ptr=seed_dev.data_ptr() if (seed_dev is not None and training) else 0,
                                             advance_seed=1 if (seed_dev is not None and training) else 0)      # fresh masks per call
            encode = F_egx.encoder_ragged_tokens_train
        else:
            spec, proj_t, _ = self._egx_spec(segs, self.transformer_encoder, self.ln, projs, None)
            encode = F_egx.encoder_ragged_tokens
        x = encode(spec, feats, lens, self.task_embed, self.pos_embed.pe, self.ln.weight, self.ln.bias, proj_t,
                   encoder_layer_tensors(self.transformer_encoder), out_layout=1 if task == 'asd' else 0)
        if task == 'asd':
            return x.view(-1, 3, self.dim).permute(1, 0, 2)        # (3, sum_b T_b, d): row 3 f + k of x is segment k of frame f
        return x

    def encode_features_ragged(self, task, lam_feat, ttm_feat=None, asd_feat=None, *, lengths):
        """encode_features(..., lengths=) for TRAINING: works in train and eval mode, under autograd, with dropout on every site in train
        mode. The features are padded batches of clips of their own lengths (`lengths` as encode_features); padded frames are never read and a
        clip's rows, and its contribution to every gradient, are what that clip gives alone and unpadded. Returns the packed (sum_b S_b, d)
        memory for 'ttm' / 'lam' (decode_ragged(..., memory_lengths=S_b)) and the reference's (3, sum_b T_b, d) for 'asd' (decode() reads it:
        its memory is sum_b T_b "clips" of exactly 3 rows). Gradients reach the projections, task_embed, the shared LayerNorm and the encoder;
        the (frozen) backbone features get none. One ragged forward / backward pair on the wide bf16 path (last_encoder_impl() == "ragged");
        configurations it does not cover run one differentiable uniform call per length group ("grouped", other dropout masks). In eval mode the
        result equals encode_features(..., lengths=) bit for bit."""
        assert task in ['lam', 'ttm', 'asd']
        return self._encode_ragged(task, lam_feat, ttm_feat, asd_feat, lengths, train=True)

    def decode_ragged(self, y, memory, memory_lengths):
        """decode(..., memory_lengths=) for TRAINING (train and eval mode, under autograd): (B, sy) tokens + the packed (sum_b S_b, d) memory of
        encode_features_ragged for 'ttm' / 'lam' -> (sy, B, |V|); clip b cross-attends to its own S_b rows, and the memory gradient comes back
        packed. last_decoder_impl() reports "ragged", or "grouped" where the fused decoder does not serve the shapes."""
        return self._egx_decode_ragged_train(y, memory, memory_lengths, embedding=self.embedding, pos_embed=self.pos_embed,
                                             decoder=self.transformer_decoder, fc=self.fc, n_heads=self.n_heads, p_drop=self.dp_rate)

    def forward_features_ragged(self, task, lam_feat, ttm_feat, asd_feat, target, *, lengths):
        """forward() from backbone features over a ragged batch, for the training step of HHI/tasks/multitask/video_tasktranslation.py:39-66:
        (B, |V|, sy) logits — (sum_b T_b, |V|, sy) for 'asd', one target row per frame — ready for nn.CrossEntropyLoss. The frozen backbones
        are stock PyTorch and would read padded frames: run them clip by clip (or through a feature cache) and pad their features here."""
        assert task in ['lam', 'ttm', 'asd']
        encoded_x = self.encode_features_ragged(task, lam_feat, ttm_feat, asd_feat, lengths=lengths)
        if task == 'asd':
            return self.decode(target, encoded_x).permute(1, 2, 0)
        S = self._ragged_lengths(task, self._encoder_segments(task, lam_feat, ttm_feat, asd_feat)[0], lengths).sum(1)
        return self.decode_ragged(target, encoded_x, S).permute(1, 2, 0)

    def encode(self, video, video_asd, audio, audio_asd, task):
        with torch.no_grad():
            lam_feat = self.lam_model(video, middle=True)
            if task == 'lam':
                return self.encode_features(task, lam_feat)
            ttm_feat = self.ttm_model(video, audio, middle=True)
            N, D, H, W = video_asd.shape
            audioEmbed = self.asd_model.forward_audio_frontend(audio_asd)
            visualEmbed = self.asd_model.forward_visual_frontend(video_asd)
            audioEmbed, visualEmbed = self.asd_model.forward_cross_attention(audioEmbed, visualEmbed)
            outsAV = self.asd_model.forward_audio_visual_backend(audioEmbed, visualEmbed)
            asd_feat = outsAV.view(N, D, -1)
        return self.encode_features(task, lam_feat, ttm_feat, asd_feat)

    # ---- decoder (HIP; row F1) ---------------------------------------------------------------------------
    def decode(self, y, encoded_x, memory_lengths=None, *, return_attention=False):
        """(B, sy) tokens + (S, B, d) memory -> (sy, B, |V|); on the GPU this is the HIP decoder (egot2_amd/decoder.py).
        memory_lengths (B,) (inference only): encoded_x is the packed (sum_b S_b, d) memory of encode_features(..., lengths=) for 'ttm' /
        'lam', clip b cross-attends to its own S_b rows.
        return_attention (eval mode, no autograd): (logits, attn) with attn (L, B, sy, S) fp32, per decoder layer the head-averaged
        cross-attention weights a forward hook on the reference's layer.multihead_attn sees (CustomDecoderLayer, task_prompt_model.py:163-172);
        with memory_lengths S is the longest memory and clip b's entries beyond S_b are zeros. The logits are those of the call without the
        flag, bit for bit. attention_by_segment(attn, (T, T, T)) sums the 'ttm' memory's three task blocks."""
        if memory_lengths is not None:
            return self._egx_decode_ragged(y, encoded_x, memory_lengths, embedding=self.embedding, pos_embed=self.pos_embed,
                                           decoder=self.transformer_decoder, fc=self.fc, n_heads=self.n_heads, p_drop=self.dp_rate,
                                           return_attention=return_attention)
        return self._egx_decode(y, encoded_x, embedding=self.embedding, pos_embed=self.pos_embed,
                                decoder=self.transformer_decoder, fc=self.fc, n_heads=self.n_heads, p_drop=self.dp_rate,
                                return_attention=return_attention)

    def forward(self, video, video_asd, audio, audio_asd, target, task):
        assert task in ['lam', 'ttm', 'asd']
        encoded_x = self.encode(video, video_asd, audio, audio_asd, task)
        return self.decode(target, encoded_x).permute(1, 2, 0)

    def predict(self, video, video_asd, audio, audio_asd, task):
        assert task in ['lam', 'ttm', 'asd']
        batch_size = video.shape[0] * video.shape[1] if task == 'asd' else video.shape[0]
        encoded_x = self.encode(video, video_asd, audio, audio_asd, task)
        y = torch.ones((batch_size, 1)) * self.vocab[task]
        y = y.type_as(video).long()
        output = self.decode(y, encoded_x)
        return output[0, :, -2:]

    def predict_features(self, task, lam_feat, ttm_feat=None, asd_feat=None, lengths=None):
        """predict() from backbone features: output[0, :, -2:] of decode(<task token>, encode_features(...)), (B, 2), or (B T, 2) for
        'asd'. With lengths (inference only; see encode_features) the features are padded batches of clips of their own lengths and the
        result is (B, 2), or (sum_b T_b, 2) for 'asd', in clip order: what predict() gives clip by clip, in one encoder and one decoder call.
        The frozen backbones (LAM / TTM BiLSTMs, the ASD front ends) are stock PyTorch and would read padded frames: run them clip by clip
        (or through a feature cache) and pad their features here."""
        assert task in ['lam', 'ttm', 'asd']
        if lengths is not None:
            self._egx_check_inference("lengths=")
        encoded_x = self.encode_features(task, lam_feat, ttm_feat, asd_feat, lengths=lengths)
        dev = lam_feat.device
        if task == 'asd':
            y = torch.full((encoded_x.shape[1], 1), self.vocab[task], dtype=torch.long, device=dev)
            output = self.decode(y, encoded_x)
        elif lengths is None:
            y = torch.full((lam_feat.shape[0], 1), self.vocab[task], dtype=torch.long, device=dev)
            output = self.decode(y, encoded_x)
        else:
            S = self._ragged_lengths(task, self._encoder_segments(task, lam_feat, ttm_feat, asd_feat)[0], lengths).sum(1)
            y = torch.full((lam_feat.shape[0], 1), self.vocab[task], dtype=torch.long, device=dev)
            output = self.decode(y, encoded_x, memory_lengths=S)
        return output[0, :, -2:]
