"""HOI LTA sequence-decoder models — drop-in mirrors of HOI/models/lta/lta_models_seqdecoder.py:65-240
(`ForecastingEncoderSeqDecoder`, `ForecastingEncoderSeparateSeqDecoder`) and HOI/models/lta/lta_models_lta_transfer.py:531-659
(`TaskFusionMFTransformer2TaskSeqDecoder`): a post-LN transformer encoder over the clip features and the EgoT2-g sequence decoder +
vocabulary head over its output, at d_model 2048 with 8 (or 4) heads in the shipped recipes (head dim 256 / 512).

Constructors take the reference's `(cfg, vocab)` and read the same yacs fields (MODEL.TRANSFORMER_ENCODER_{HEADS,LAYERS},
MODEL.MULTI_INPUT_FEATURES; FORECASTING.NUM_INPUT_CLIPS, MODEL.TRANSLATION_{HEADS,LAYERS,INPUT_FEATURES,DROPOUT}); attribute names and
state_dict keys are the reference's (ln, pos_embed.pe, embedding, transformer_encoder.*, transformer_decoder.*, fc, pe; backbone.* /
action_model.* / lta_model.* when built). `v_idx` / `n_idx` (utils.multitask.build_vocab.vocab_idx_to_orig) may be passed in, as
hoi_multitask.TaskTranslationPromptTransformerActionTask takes them. The frozen backbones are built through
egot2_amd.backbones.make_hoi_backbone only where the config names their checkpoints (cfg.CHECKPOINT_FILE_PATH for the forecasting
models' SlowFast, cfg.CHECKPOINT_FILE_PATH_{AR,LTA} for the 2-task model); without them the models are used at feature level:
`encode_features(...)` takes the precomputed clip features, `decode` / `forward_features` / `predict_features` go from there.

The encoder runs through TranslatorMixin._egx_encode (d 2048, head dim 256 / 512, S <= 16: the wide bf16 path), the decoder through
DecoderMixin: set_compute("bf16") is what serves these widths; under the other compute modes the first decode() raises the composed
path's refusal, which says so. Behind the off-by-default `egx_generate` switch (eval mode) the 40-step loop of predict() is ONE
greedy_decode(..., schedule=verb_noun_schedule(v_idx, n_idx)) call and generate()'s draws go through functional.lta_validate (k = 1: the row argmax; k > 1: the library's
counter generator instead of torch's). One deliberate difference of the switched predict(): the reference's loop feeds back the argmax over the
WHOLE vocabulary (lta_models_seqdecoder.py:197) and only reads the verb / noun subset, the schedule feeds back the subset's argmax. The two
agree for as long as the full argmax lies in the step's word set; from the first step where it does not, the prefixes differ and so may
every later row. The default loop decodes prefixes of up to 40 tokens: beyond 8 that is the cached step under torch.no_grad() in eval mode."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.distributions.categorical import Categorical

from . import functional as F_egx
from .backbones import cfg_get, freeze_backbone_params, freeze_params, make_hoi_backbone
from .decoder import DecoderMixin
from .functional import SegmentSpec
from .hhi_multitask import CustomDecoderLayer
from .hoi_lta import MODEL_REGISTRY
from .translator import PositionalEncoding, TranslatorMixin


def _vocab_index_maps(v_idx, n_idx):
    if v_idx is None or n_idx is None:
        try:
            import importlib
            v_idx, n_idx = importlib.import_module("utils.multitask.build_vocab").vocab_idx_to_orig()
        except ImportError:
            pass
    return v_idx, n_idx


class _SeqDecoderModel(nn.Module, TranslatorMixin, DecoderMixin):
    """What the three models share: the target mask attribute, decode(), the one-token verb / noun predict and generate()."""

    # predict() / generate() take greedy_decode and functional.lta_validate instead of the loops below when the model is in eval mode AND
    # this is set; off by default, as hoi_multitask.TaskPromptTransformer.egx_generate is
    egx_generate = False

    def get_tgt_mask(self, size) -> torch.Tensor:
        mask = torch.tril(torch.ones(size, size) == 1).float()
        mask = mask.masked_fill(mask == 0, float('-inf'))
        mask = mask.masked_fill(mask == 1, float(0.0))
        return mask

    def _init_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def decode(self, y, encoded_x, *, return_attention=False):
        """(B, sy) tokens + (S, B, d) memory -> (sy, B, |V|): the HIP decoder (egot2_amd/decoder.py)."""
        return self._egx_decode(y, encoded_x, embedding=self.embedding, pos_embed=self.pos_embed, decoder=self.transformer_decoder, fc=self.fc,
                                n_heads=self.n_heads, p_drop=self._dec_dropout, return_attention=return_attention)

    def forward_features(self, *feats_and_target):
        """forward() from precomputed clip features: (*features, target) -> (B, |V|, sy)."""
        *feats, target = feats_and_target
        return self.decode(target, self.encode_features(*feats)).permute(1, 2, 0)

    def _predict_one_token(self, encoded_x, like, only_verb=False):
        """The verb / noun heads of one 'lta_verb' / 'lta_noun' token each: [(B, 1, #verbs), (B, 1, #nouns)]."""
        B = encoded_x.shape[1]
        y_verb = (torch.ones((B, 1)) * self.vocab['lta_verb']).type_as(like).long()
        preds_verb = self.decode(y_verb, encoded_x)[0, :, self.v_idx].unsqueeze(dim=1)
        if only_verb:
            return None
        y_noun = (torch.ones((B, 1)) * self.vocab['lta_noun']).type_as(like).long()
        preds_noun = self.decode(y_noun, encoded_x)[0, :, self.n_idx].unsqueeze(dim=1)
        return [preds_verb, preds_noun]

    def _generate(self, x, k):
        if self.egx_generate and not self.training:
            return F_egx.lta_validate(x, None, k)[0]
        results = []
        for head_x in x:
            if k > 1:
                preds_dist = Categorical(logits=head_x)
                preds = [preds_dist.sample() for _ in range(k)]
            elif k == 1:
                preds = [head_x.argmax(2)]
            results.append(torch.stack(preds, dim=1))
        return results


@MODEL_REGISTRY.register()
class ForecastingEncoderSeqDecoder(_SeqDecoderModel):
    """Reference lta_models_seqdecoder.py:65-216: tokens = pos_embed(ln(clip features)) (one identity segment, sinusoid positions with
    pos_embed's dropout, no task row) -> encoder -> decoder; predict() is the 40-step greedy verb / noun loop."""

    def __init__(self, cfg, vocab, v_idx=None, n_idx=None):
        super().__init__()
        self.cfg = cfg
        self.vocab = vocab
        self.v_idx, self.n_idx = _vocab_index_maps(v_idx, n_idx)
        self.build_clip_backbone()
        self.build_encoder_decoder()

    def build_clip_backbone(self):
        cfg = self.cfg
        if not cfg_get(cfg, "CHECKPOINT_FILE_PATH"):
            return          # feature-level use
        if cfg_get(cfg, "MODEL.ARCH") == "mvit":
            raise NotImplementedError("ForecastingEncoderSeqDecoder: MODEL.ARCH = 'mvit' (the reference builds MViT here) has no backbone factory; "
                                      "attach the module as `backbone`, or use encode_features() with precomputed clip features")
        self.backbone = make_hoi_backbone("slowfast", cfg=cfg, num_classes=[cfg.MODEL.MULTI_INPUT_FEATURES], with_head=True,
                                          ckpt=cfg.CHECKPOINT_FILE_PATH, loader="lta")
        if cfg_get(cfg, "MODEL.FREEZE_BACKBONE"):
            freeze_backbone_params(self.backbone)       # never the head

    def build_encoder_decoder(self):
        self.n_heads = self.cfg.MODEL.TRANSFORMER_ENCODER_HEADS
        self.n_layers = self.cfg.MODEL.TRANSFORMER_ENCODER_LAYERS
        self.dim = self.cfg.MODEL.MULTI_INPUT_FEATURES
        self._dec_dropout = 0.1                         # (the layers' default, as the reference builds them)
        self.ln = nn.LayerNorm(self.dim)
        self.pos_embed = PositionalEncoding(self.dim, dropout=0.1, max_len=200)
        self.embedding = nn.Embedding(len(self.vocab), self.dim)
        self.y_mask = self.get_tgt_mask(200)            # plain attribute, not a buffer (as in the reference)
        self.transformer_encoder = nn.TransformerEncoder(   # parameter containers only
            encoder_layer=nn.TransformerEncoderLayer(d_model=self.dim, nhead=self.n_heads), num_layers=self.n_layers)
        self.transformer_decoder = nn.TransformerDecoder(
            decoder_layer=CustomDecoderLayer(d_model=self.dim, nhead=self.n_heads), num_layers=self.n_layers)
        self.fc = nn.Linear(self.dim, len(self.vocab))

    def encode_clips(self, x):
        assert isinstance(x, list) and len(x) >= 1
        return [self.backbone([pathway[:, i] for pathway in x]) for i in range(x[0].shape[1])]

    def encode_features(self, feats):
        """feats (B, n, d) clip features (or the list of n (B, d) encode_clips returns) -> memory (n, B, d)."""
        if isinstance(feats, (list, tuple)):
            feats = torch.stack(list(feats), dim=1)
        feats = feats.contiguous()
        segs = [SegmentSpec(T=feats.shape[1], d_in=feats.shape[2], has_proj=False, add_row=None, pos_row0=0)]
        x = self._egx_encode([feats], segs, encoder=self.transformer_encoder, ln=self.ln, projs=[None], task_embed=None,
                             pos_table=self.pos_embed.pe, p_drop=0.1, p_pos=self.pos_embed.dropout.p)
        return x.permute(1, 0, 2)

    def encode(self, x):
        return self.encode_features(x)

    def forward(self, x, target):
        return self.decode(target, self.encode(self.encode_clips(x))).permute(1, 2, 0)

    def predict_features(self, feats):
        return self._predict_from_memory(self.encode_features(feats), feats[0] if isinstance(feats, (list, tuple)) else feats)

    def predict(self, x):
        return self._predict_from_memory(self.encode(self.encode_clips(x)), x[0])

    def _predict_from_memory(self, encoded_x, like, seq_len=41):
        B = encoded_x.shape[1]
        if self.egx_generate and not self.training:
            with torch.no_grad():
                _, logits = self.greedy_decode(encoded_x, int(self.vocab['action']), seq_len - 1, return_logits=True,
                                               schedule=self.verb_noun_schedule(self.v_idx, self.n_idx))
            return [logits[0::2][:, :, self.v_idx].permute(1, 0, 2), logits[1::2][:, :, self.n_idx].permute(1, 0, 2)]
        output_tokens = torch.ones((B, seq_len)).type_as(like).long()
        output_tokens[:, 0] = self.vocab['action']
        preds_verb_list, preds_noun_list = [], []
        for sy in range(1, seq_len):
            output_prob = self.decode(output_tokens[:, :sy], encoded_x)
            if sy % 2 == 1:
                preds_verb_list.append(output_prob[-1, :, self.v_idx])
            else:
                preds_noun_list.append(output_prob[-1, :, self.n_idx])
            output_tokens[:, sy] = torch.argmax(output_prob, dim=-1)[-1, :]
        return [torch.stack(preds_verb_list, dim=1), torch.stack(preds_noun_list, dim=1)]

    def generate(self, x, k=1):
        return self._generate(self.predict(x), k)


@MODEL_REGISTRY.register()
class ForecastingEncoderSeparateSeqDecoder(ForecastingEncoderSeqDecoder):
    """Reference lta_models_seqdecoder.py:219-240: predict() decodes one 'lta_verb' and one 'lta_noun' token."""

    def _predict_from_memory(self, encoded_x, like, seq_len=41):
        with torch.no_grad():
            return self._predict_one_token(encoded_x, like)

    def predict_features(self, feats):
        with torch.no_grad():
            return super().predict_features(feats)

    def predict(self, x):
        with torch.no_grad():
            return super().predict(x)


@MODEL_REGISTRY.register()
class TaskFusionMFTransformer2TaskSeqDecoder(_SeqDecoderModel):
    """Reference lta_models_lta_transfer.py:531-659: tokens = ln(cat(action, lta)) + pe (2 n learned positions) -> encoder -> decoder over
    at most 3 target tokens (`y_mask` of size 3)."""

    def __init__(self, cfg, vocab, v_idx=None, n_idx=None):
        super().__init__()
        self.cfg = cfg
        self.vocab = vocab
        self.v_idx, self.n_idx = _vocab_index_maps(v_idx, n_idx)
        self.sequence_len = cfg.FORECASTING.NUM_INPUT_CLIPS * 2
        self.num_heads = self.n_heads = cfg.MODEL.TRANSLATION_HEADS
        self.num_layers = cfg.MODEL.TRANSLATION_LAYERS
        self.feature_dim = cfg.MODEL.TRANSLATION_INPUT_FEATURES
        self.dp_rate = self._dec_dropout = cfg.MODEL.TRANSLATION_DROPOUT
        self.transformer_encoder = nn.TransformerEncoder(   # parameter containers only
            encoder_layer=nn.TransformerEncoderLayer(d_model=self.feature_dim, nhead=self.num_heads, dropout=self.dp_rate),
            num_layers=self.num_layers)
        self.transformer_decoder = nn.TransformerDecoder(
            decoder_layer=CustomDecoderLayer(d_model=self.feature_dim, nhead=self.num_heads, dropout=self.dp_rate), num_layers=self.num_layers)
        self.ln = nn.LayerNorm(self.feature_dim)
        self.pe = nn.Parameter(torch.randn(1, self.sequence_len, self.feature_dim), requires_grad=True)
        self.pos_embed = PositionalEncoding(self.feature_dim, dropout=self.dp_rate, max_len=200)
        self.embedding = nn.Embedding(len(self.vocab), self.feature_dim)
        self.y_mask = self.get_tgt_mask(3)
        self.fc = nn.Linear(self.feature_dim, len(self.vocab))
        self._init_parameters()
        # the two frozen models (reference :561-574), attached after the xavier init above
        if cfg_get(cfg, "CHECKPOINT_FILE_PATH_AR"):
            self.action_model = make_hoi_backbone("slowfast", cfg=cfg, num_classes=[self.feature_dim], with_head=True,
                                                  ckpt=cfg.CHECKPOINT_FILE_PATH_AR, loader="lta")
            freeze_backbone_params(self.action_model)
        if cfg_get(cfg, "CHECKPOINT_FILE_PATH_LTA"):
            self.lta_model = make_hoi_backbone("lta", cfg=cfg, build_decoder=True, ckpt=cfg.CHECKPOINT_FILE_PATH_LTA)
            freeze_params(self.lta_model)

    def encode_clips(self, model, x):
        assert isinstance(x, list) and len(x) >= 1
        return torch.stack([model([pathway[:, i] for pathway in x]) for i in range(x[0].shape[1])], dim=1)

    def encode_features(self, feat_action, feat_lta):
        """action, lta (B, n, d) with 2 n == sequence_len -> memory (2n, B, d)."""
        feats = [feat_action.contiguous(), feat_lta.contiguous()]
        segs, off = [], 0
        for f in feats:
            segs.append(SegmentSpec(T=f.shape[1], d_in=f.shape[2], has_proj=False, add_row=None, pos_row0=off))
            off += f.shape[1]
        if off != self.pe.shape[1]:
            raise ValueError(f"token count {off} != {self.pe.shape[1]} learned positions")
        x = self._egx_encode(feats, segs, encoder=self.transformer_encoder, ln=self.ln, projs=[None, None], task_embed=None,
                             pos_table=self.pe[0], p_drop=self.dp_rate)
        return x.permute(1, 0, 2)

    def encode(self, x):
        feat_action = self.encode_clips(self.action_model, x)                    # (B, n, d)
        feat_lta = self.lta_model(x, None, middle=True).transpose(0, 1)
        return self.encode_features(feat_action, feat_lta)

    def forward(self, x, target):
        return self.decode(target, self.encode(x)).permute(1, 2, 0)

    def predict_features(self, feat_action, feat_lta, only_verb=False):
        return self._predict_one_token(self.encode_features(feat_action, feat_lta), feat_action, only_verb)

    def predict(self, x, only_verb=False):
        return self._predict_one_token(self.encode(x), x[0], only_verb)

    def generate(self, x, k=1):
        return self._generate(self.predict(x), k)
