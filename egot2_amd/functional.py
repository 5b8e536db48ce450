"""torch.autograd bridges onto the C ABI of libegot2x.so.

PyTorch is plumbing here (device memory, streams, autograd graph); all arithmetic of the translator runs in the
hand-written HIP kernels. There is no fallback: a missing library or a CPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import (Ce, Config, Head, HeadGrads, Layer, LayerGrads, Segment, SegmentGrads, check, ptr,
                   EGX_F32, EGX_BF16, EGX_F32_SPLIT, EGX_IMPL_AUTO, EGX_IMPL_GENERIC, EGX_IMPL_FUSED, EGX_IMPL_WIDE, EGX_IMPL_TILED)

# "f32s": fp32 operands split exactly into three bf16 parts, six bf16 MFMAs per K-block (fp32-grade results, fused d = 128
# kernels only; elsewhere it computes as "f32")
COMPUTE = {"f32": EGX_F32, "fp32": EGX_F32, "float32": EGX_F32, "bf16": EGX_BF16, "bfloat16": EGX_BF16, "f32s": EGX_F32_SPLIT}
IMPL = {"auto": EGX_IMPL_AUTO, "generic": EGX_IMPL_GENERIC, "fused": EGX_IMPL_FUSED, "wide": EGX_IMPL_WIDE, "tiled": EGX_IMPL_TILED}


@dataclass
class SegmentSpec:
    T: int
    d_in: int
    has_proj: bool
    add_row: Optional[int] = None      # row of the (1, K, d) task-embedding table, or None
    pos_row0: Optional[int] = None     # first row of the positional table used by this segment, or None
    pool: int = 1                      # > 1: the feature tensor holds T * pool frames, token t = mean of frames [t pool, (t+1) pool)


_weights_epoch = [0]


def note_weights_changed():
    """Tell the packed-weight caches (WeightCache) that parameters were written behind torch's back (raw-pointer kernels: FusedAdam, a
    replayed hipGraph that contains an optimizer update). In-place torch ops on the parameters are seen through their version counters."""
    _weights_epoch[0] += 1


class WeightCache:
    """Persistent device buffer for the MFMA-fragment-packed weight copies of the per-clip / tiled kernels (egx_config.weight_cache).
    A forward whose weights did not change since the forward that filled it skips the packing launch (6 us of the 0.38 ms TTM step).
    "Did not change" is decided on the host: storage address + version counter of every packed weight, the compute mode, the FFN keep-scale
    and note_weights_changed()'s epoch. Writes that bypass all of those (`p.data.add_()` bumps no counter) need invalidate().
    frozen=True is the caller's promise that the weights do not change while it is set (inference, a forward + backward benchmark): only
    then is the packing launch also left out of a CAPTURED step — a replay cannot re-check anything."""

    def __init__(self, frozen: bool = False):
        self.buf: Optional[torch.Tensor] = None
        self.sig = None
        self.frozen = bool(frozen)
        self.hits = 0
        self.packs = 0

    def invalidate(self):
        self.sig = None


@dataclass
class EncoderSpec:
    d_model: int
    n_heads: int
    d_ff: int
    n_layers: int
    segments: List[SegmentSpec] = field(default_factory=list)
    ln_eps: float = 1e-5
    compute: str = "f32"
    impl: str = "auto"
    p_drop: float = 0.0
    p_pos: float = 0.0
    p_feat: float = 0.0
    training: bool = False
    seed: int = 0
    seed_ptr: int = 0      # device address of a uint64 seed (hipGraph-replayable dropout), 0 = use `seed`
    head_n_out: int = 0    # > 0: pooled head (mean -> LN -> Linear) evaluated with the encoder; output = logits
    advance_seed: int = 0        # with seed_ptr: 1 = the training forward advances the device seed in its first kernel; 2 = the backward
                                 # advances it behind its last reader (egx_config.advance_seed)
    defer_small: bool = False    # backward: leave the grouped small weight gradients to run_deferred() (all-reduce overlap)
    deterministic: bool = False  # backward: fixed-order reductions instead of fp32 atomics (bit-identical gradients run to run)
    out_tokens: int = 0          # > 0: return (and take the gradient of) only the first `out_tokens` tokens of every clip
    wcache: Optional[WeightCache] = None     # persistent packed-weight cache (None: packed into `saved` every forward)
    token_ce: int = 0            # > 0 (classes): the forward also evaluates a per-token classifier + weighted cross entropy on the returned tokens
                                 # (egx_token_ce, the ASD task's lossAV); use encoder_token_ce(), which falls back where the kernels do not fuse it
    ce: bool = False             # with head_n_out: the forward also evaluates the weighted cross entropy of the logits (egx_ce); EncoderFn then
                                 # takes (target, class_weight | None) behind the head parameters and returns (logits, loss)

    def config(self) -> Config:
        return Config(self.d_model, self.n_heads, self.d_ff, self.n_layers, len(self.segments), float(self.ln_eps),
                      COMPUTE[self.compute], IMPL[self.impl], float(self.p_drop), float(self.p_pos), float(self.p_feat),
                      self.seed_ptr or None, int(self.advance_seed) if self.seed_ptr else 0, None, 0, 0,
                      int(bool(self.deterministic)), int(self.out_tokens))


# The library reads its kernel-selection switches (EGX_FFN_CUT, EGX_FFN_SLICES, EGX_SLICE_DROP) from the environment once. Tests and tuning
# tools that flip them inside one process set this (tests/conftest.py): every forward / backward then asks the library to re-read them first.
reload_tuning_each_call = False

_scratch_cache = {}
# record_attention / encoder_attention (the AttentionRecorder at the end of this file) while active, else None: the encoder forwards call it
# right behind their library call with that call's own configuration, segments and `saved`
_attention_sink = None
_last_impl = [EGX_IMPL_AUTO]
_last_slices = [1]
# last_encoder_impl() of the ragged-batch forward (encoder_ragged): the ragged tiled kernels, or the per-length-group fallback
IMPL_RAGGED, IMPL_GROUPED = 100, 101
IMPL_RAGGED_CAP = 102       # encoder_ragged_train with device lengths and a capacity (the capturable form)
_IMPL_NAMES = {**{v: k for k, v in IMPL.items()}, IMPL_RAGGED: "ragged", IMPL_GROUPED: "grouped", IMPL_RAGGED_CAP: "ragged_cap"}


def last_encoder_slices() -> int:
    """Diagnostic: workgroups per clip of the most recent encoder forward (egx_encoder_slices: > 1 = sliced mode of the per-clip
    kernels on a small batch)."""
    return _last_slices[0]


def last_encoder_impl() -> str:
    """Diagnostic: the implementation the most recent encoder forward ran ("fused" | "wide" | "generic" | ...; "ragged" / "grouped" for
    encoder_ragged and encoder_ragged_train, "ragged_cap" for encoder_ragged_train with device lengths and a capacity)."""
    return _IMPL_NAMES.get(_last_impl[0], "auto")

# EGX_POISON=1 (testing aid): every workspace handed to the library is filled with 0xFF bytes (NaN in fp32 and bf16) first,
# so that a kernel reading memory nobody wrote shows up as NaNs instead of passing on whatever the allocator left there
_POISON = bool(int(__import__("os").environ.get("EGX_POISON", "0") or 0))


def _workspace(tag: str, device: torch.device, nbytes: int) -> torch.Tensor:
    """Grow-only byte buffer per (tag, device). Safe because every call is ordered on the current stream."""
    key = (tag, device.index)
    buf = _scratch_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _scratch_cache[key] = buf
    if _POISON:
        buf.fill_(255)
    return buf


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.EgxError(f"{name} is on {t.device}: the translator runs only on the GPU through libegot2x.so "
                            "(no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.EgxError(f"{name} has dtype {t.dtype}; libegot2x stores activations and weights in fp32")
    return t.contiguous()


def _dev_feat(t: torch.Tensor, name: str) -> torch.Tensor:
    """Backbone features: fp32, or bf16 in the packed layout the wide path's projection GEMM reads."""
    if not t.is_cuda:
        raise _lib.EgxError(f"{name} is on {t.device}: the translator runs only on the GPU through libegot2x.so "
                            "(no CPU fallback)")
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.EgxError(f"{name} has dtype {t.dtype}; features are fp32 or bf16")
    return t.contiguous()


def _elem_ptr(t: torch.Tensor, row: int, row_elems: int) -> int:
    return t.data_ptr() + 4 * row * row_elems


def _dev_params(feats, proj, layer_t, head_t, ln_w, ln_b, task_embed, pos_table, feat=_dev_feat):
    """The tensors of one encoder call, on the device and contiguous: the features through `feat` (fp32 or bf16, or _dev_f32), the rest fp32.
    Returns (feats, proj, layer_t, head_t, ln_w, ln_b, task_embed, pos_table) as lists / tensors / None."""
    return ([feat(t, f"feats[{i}]") for i, t in enumerate(feats)], [_dev_f32(t, "projection weight") for t in proj],
            [_dev_f32(t, "layer weight") for t in layer_t], [_dev_f32(t, "head parameter") for t in head_t],
            _dev_f32(ln_w, "ln.weight"), _dev_f32(ln_b, "ln.bias"),
            None if task_embed is None else _dev_f32(task_embed, "task_embed"),
            None if pos_table is None else _dev_f32(pos_table, "positional table"))


def _segments(spec: EncoderSpec, feats, proj, task_embed, pos_table, B: int, grads=None):
    """The egx_segment array of a call on B clips, with the features' and projections' shapes checked. With grads = (feature gradients,
    projection gradients (w, b per projecting segment), task_embed gradient, positional-table gradient), None where not wanted, also the
    egx_segment_grads array: returns (segments, segment gradients)."""
    nseg, d = len(spec.segments), spec.d_model
    segs = (Segment * nseg)()
    sgr = (SegmentGrads * nseg)() if grads is not None else None
    pi = 0
    for i, (ss, f) in enumerate(zip(spec.segments, feats)):
        if f.shape != (B, ss.T * max(ss.pool, 1), ss.d_in):
            raise _lib.EgxError(f"feats[{i}] has shape {tuple(f.shape)}, expected ({B}, {ss.T * max(ss.pool, 1)}, {ss.d_in})")
        if not ss.has_proj and (f.dtype == torch.bfloat16 or ss.pool > 1):
            raise _lib.EgxError(f"feats[{i}]: bf16 / frame-pooled features need a projection (an identity segment enters "
                                "the shared LayerNorm as fp32 rows)")
        segs[i].feat, segs[i].T, segs[i].d_in = ptr(f), ss.T, ss.d_in
        segs[i].feat_bf16, segs[i].pool = int(f.dtype == torch.bfloat16), int(ss.pool)
        if ss.has_proj:
            w, b = proj[2 * pi], proj[2 * pi + 1]
            if w.shape != (d, ss.d_in):
                raise _lib.EgxError(f"projection {i} weight shape {tuple(w.shape)} != ({d}, {ss.d_in})")
            segs[i].proj_w, segs[i].proj_b = ptr(w), ptr(b)
        if ss.add_row is not None:
            segs[i].add_vec = _elem_ptr(task_embed, ss.add_row, d)
        if ss.pos_row0 is not None:
            segs[i].pos, segs[i].pos_stride = _elem_ptr(pos_table, ss.pos_row0, d), d
        if sgr is not None:
            d_feat, d_proj, d_te, d_pos = grads
            sgr[i].feat = ptr(d_feat[i])
            if ss.has_proj:
                sgr[i].proj_w, sgr[i].proj_b = ptr(d_proj[2 * pi]), ptr(d_proj[2 * pi + 1])
            if ss.add_row is not None and d_te is not None:
                sgr[i].add_vec = _elem_ptr(d_te, ss.add_row, d)
            if ss.pos_row0 is not None and d_pos is not None:
                sgr[i].pos = _elem_ptr(d_pos, ss.pos_row0, d)
        pi += int(ss.has_proj)
    return segs if sgr is None else (segs, sgr)


def _layers(layer_t, n_layers: int, grads=None):
    """The egx_layer array (12 tensors per layer in _LAYER_FIELDS order); with grads (the same order, None where not wanted) also the
    egx_layer_grads array: returns (layers, layer gradients)."""
    def array(struct, ts):
        return (struct * max(n_layers, 1))(*[struct(*map(ptr, ts[12 * l:12 * l + 12])) for l in range(n_layers)])
    layers = array(Layer, layer_t)
    return layers if grads is None else (layers, array(LayerGrads, grads))


class _GradPacker:
    """Allocates every requested gradient as a 16-byte-aligned view of one flat buffer. Entries marked `late` (the
    weight gradients the backward finishes last: dW_proj, dW_in, dW_o) are placed first, so that everything behind
    `late_floats` can be all-reduced while they are still being computed (ddp.allreduce_gradients_overlapped)."""

    def __init__(self):
        self.entries = []
        self.total = 0
        self.late_floats = 0

    def add(self, t: Optional[torch.Tensor], want: bool, late: bool = False, rank: int = 0) -> int:
        """`rank`: entries are laid out by ascending rank (stable): the bucketed exchange gives the tensors of the encoder layer the
        backward finishes first the lowest rank, so every layer's gradients are one contiguous slice (self.rank_span)."""
        if t is None or not want:
            self.entries.append(None)
            return -1
        self.entries.append((t.shape, (t.numel() + 3) // 4 * 4, late, rank))
        return len(self.entries) - 1

    _layouts: dict = {}          # entries signature -> (offsets, total, late_floats, rank_span, strides): a model's backward lays out the same buffer every step

    def materialise(self, device, zero: bool = True) -> List[Optional[torch.Tensor]]:
        """zero=False: the caller hands `self.flat` to the library, whose backward zero-fills it (egx_config.zero_buf)."""
        sig = tuple(self.entries)
        lay = _GradPacker._layouts.get(sig)
        if lay is None:
            offs, cur, rank_span, late_floats = {}, 0, {}, 0
            order = sorted((i for i, e in enumerate(self.entries) if e is not None), key=lambda i: self.entries[i][3])
            for want_late in (True, False):
                for i in order:
                    e = self.entries[i]
                    if e[2] == want_late:
                        offs[i] = cur
                        lo, hi = rank_span.get(e[3], (cur, cur))
                        rank_span[e[3]] = (min(lo, cur), cur + e[1])
                        cur += e[1]
                if want_late:
                    late_floats = cur
            strides = {}
            for i, e in enumerate(self.entries):
                if e is not None:
                    st, acc = [], 1
                    for k in reversed(e[0]):
                        st.append(acc)
                        acc *= k
                    strides[i] = tuple(reversed(st))
            if len(_GradPacker._layouts) > 256:
                _GradPacker._layouts.clear()
            lay = _GradPacker._layouts[sig] = (offs, cur, late_floats, rank_span, strides)
        offs, self.total, self.late_floats, rank_span, strides = lay
        self.rank_span = dict(rank_span)
        n = max(self.total, 4)
        flat = torch.zeros(n, dtype=torch.float32, device=device) if zero else torch.empty(n, dtype=torch.float32, device=device)
        if _POISON and not zero:
            flat.fill_(float("nan"))
        self.flat = flat
        # one as_strided per gradient (a slice + a view were two tensor constructions each: 50 per backward of the TTM translator)
        return [None if e is None else flat.as_strided(e[0], strides[i], offs[i]) for i, e in enumerate(self.entries)]


_deferred = []          # closures that finish a staged backward (EncoderSpec.defer_small)
# Bucketed gradient exchange (ddp.BucketedExchange): when set, bucket_hook(flat, lo, hi) is called from inside a backward as
# soon as the kernels that complete flat[lo:hi] are enqueued on the current stream (per encoder layer on the wide path, once
# per buffer elsewhere); the hook starts the all-reduce of that slice, which then overlaps the rest of the backward.
bucket_hook = None
last_grad_layout = {}   # {"flat": flat gradient buffer of the latest encoder backward, "late_floats": size of its late region}


def run_deferred():
    """Launch the grouped small weight gradients that a backward with EncoderSpec.defer_small left out."""
    while _deferred:
        _deferred.pop(0)()


def flat_storage_view(t: torch.Tensor) -> torch.Tensor:
    """1-D view over the WHOLE storage `t` lives in. Gradients handed out by _GradPacker reach `.grad` detached (autograd
    drops `_base`), so the flat buffer behind them is recovered through the storage: every gradient of one backward
    shares it, which is what lets the all-reduce and the optimizer run once per buffer."""
    st = t.untyped_storage()
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(st, 0, (st.nbytes() // t.element_size(),))


def _load():
    """The library; under reload_tuning_each_call it re-reads its kernel-selection switches first."""
    lib = _lib.load()
    if reload_tuning_each_call:
        lib.egx_tuning_reload()
    return lib


def _seed64(x: int) -> C.c_uint64:
    return C.c_uint64(int(x) & (2**64 - 1))


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """`t` as a contiguous fp32 tensor: itself where it is one already (an upstream gradient usually is: no torch op)."""
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _head(head_t, n_out: int) -> Head:
    return Head(*map(ptr, head_t), n_out)


def _saved_buffer(needs_grad: bool, tag: str, device: torch.device, nbytes: int) -> torch.Tensor:
    """The `saved` workspace of a forward: a buffer of the call's own where a backward may follow (any input needs a gradient), else the
    shared grow-only workspace `tag`. Poisoned under EGX_POISON either way."""
    if not needs_grad:
        return _workspace(tag, device, nbytes)
    saved = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    if _POISON:
        saved.fill_(255)
    return saved


def _ce_attach(spec: EncoderSpec, cfg: Config, target, weight, B: int, device):
    """The fused cross entropy of the pooled head's logits (spec.ce, egx_ce) attached to cfg: returns (loss, d_logits, keep-alive), both
    written by the forward."""
    if target.dtype != torch.int64 or tuple(target.shape) != (B,) or target.device != device:
        raise ValueError("target must be an int64 tensor of shape (B,) on the features' device")
    tgt = target.contiguous()
    cw = None if weight is None else _dev_f32(weight, "class weight")
    if cw is not None and cw.numel() != spec.head_n_out:
        raise ValueError("class weight must have one entry per class")
    loss = torch.empty((), dtype=torch.float32, device=device)
    dl = torch.empty((B, spec.head_n_out), dtype=torch.float32, device=device)
    ce_struct = Ce(ptr(tgt), ptr(cw), ptr(loss), ptr(dl))
    cfg.ce = C.cast(C.pointer(ce_struct), C.c_void_p)
    return loss, dl, (tgt, cw, ce_struct)


def _ce_upstream(ctx, d_out, d_loss):
    """Upstream gradients of the (logits, loss) outputs of a forward with spec.ce -> (d_out, dl_scale), or None when neither output has one.
    The loss's d_logits was left by the forward; its upstream gradient (loss.backward()'s ones, a loss scale) goes to the kernels as a
    device scalar. A gradient reaching the logits directly as well is the rare case: torch ops."""
    if d_loss is None:
        return None if d_out is None else (d_out, None)
    g = _f32c(d_loss)
    if d_out is None:
        return ctx.ce_dl, g
    return d_out + ctx.ce_dl * g, None


class _EncArgs:
    """The tensor arguments of the encoder Functions, in their one order: task_embed | None, pos_table | None, ln_w, ln_b, feats[n_seg],
    (proj_w, proj_b) per projecting segment, 12 tensors per layer in _LAYER_FIELDS order, (head_ln_w, head_ln_b, head_W, head_b) with
    spec.head_n_out, then the tail of a fused loss (spec.ce: target, class weight | None; spec.token_ce: classifier weight, bias | None,
    target, class weight | None). `rest` is everything behind ln_b."""

    @staticmethod
    def split(spec: EncoderSpec, rest, wide: bool = False):
        """rest -> (feats, proj, layer_t, head_t, tail). wide (RaggedWideEncoderFn): every segment projects and nothing follows the layers,
        by position and whatever the spec says."""
        nseg = len(spec.segments)
        if wide:
            return rest[:nseg], rest[nseg:3 * nseg], rest[3 * nseg:], (), ()
        nproj = sum(1 for s in spec.segments if s.has_proj)
        end = len(rest) - (4 if spec.token_ce else 2 if spec.ce else 0)
        head0 = end - (4 if spec.head_n_out else 0)
        return rest[:nseg], rest[nseg:nseg + 2 * nproj], rest[nseg + 2 * nproj:head0], rest[head0:end], rest[end:]

    @staticmethod
    def save(ctx, task_embed, pos_table, ln_w, ln_b, feats, proj, layer_t, head_t, tail=()):
        """save_for_backward of a forward's (device, contiguous) tensors; `tail`: further tensors the backward reads (the token classifier's)."""
        ctx.has_te, ctx.has_pos = task_embed is not None, pos_table is not None
        ctx.counts = (len(feats), len(proj), len(layer_t), len(head_t))
        ctx.save_for_backward(*[t for t in (task_embed, pos_table) if t is not None], ln_w, ln_b, *feats, *proj, *layer_t, *head_t, *tail)

    @staticmethod
    def load(ctx):
        """-> (task_embed, pos_table, ln_w, ln_b, feats, proj, layer_t, head_t, tail) as save() took them"""
        sv = list(ctx.saved_tensors)
        task_embed = sv.pop(0) if ctx.has_te else None
        pos_table = sv.pop(0) if ctx.has_pos else None
        a, b, c, e = (2 + sum(ctx.counts[:k]) for k in (1, 2, 3, 4))
        return task_embed, pos_table, sv[0], sv[1], sv[2:a], sv[a:b], sv[b:c], sv[c:e], sv[e:]


class _EncGrads:
    """The gradients of one encoder backward. Everything but the feature gradients is a view of ONE flat buffer (_GradPacker), registered in
    argument order; `need` is ctx.needs_input_grad, `at` the index of feats[0] in it (5, 7 or 8). bucketed (EncoderFn under bucket_hook): the
    tensors of the layer the backward finishes first (the LAST one) get rank 0, ..., layer 0 rank L - 1, everything else L, so that each
    layer's gradients are one contiguous slice; late (EncoderFn without a hook): dW_proj, dW_in, dW_o lead the buffer (_GradPacker)."""

    def __init__(self, spec: EncoderSpec, need, at: int, tensors, device, late: bool = False, bucketed: bool = False):
        task_embed, pos_table, ln_w, ln_b, feats, proj, layer_t, head_t, tail = tensors
        n_l = spec.n_layers
        rest_rank = n_l if bucketed else 0
        pk = self.pk = _GradPacker()
        for t, want in zip((task_embed, pos_table, ln_w, ln_b), need[at - 4:at]):
            pk.add(t, want, rank=rest_rank)
        # d(feature) is a per-sample ACTIVATION gradient: it must never sit in the flat buffer that the data-parallel exchange
        # all-reduces (in place, on the collective's stream, while autograd hands the same memory to the upstream module).
        # Every implementation overwrites it (input-gradient GEMM / LayerNorm backward), so it needs no zero fill either.
        self.feats = [torch.empty(f.shape, dtype=torch.float32, device=device) if need[at + i] else None for i, f in enumerate(feats)]
        k = at + len(feats)
        # proj: (w, b) pairs; layer: 12 tensors in _LAYER_FIELDS order, in_proj_w / out_proj_w are indices 0 and 2
        for i, t in enumerate(proj):
            pk.add(t, need[k + i], late=late and i % 2 == 0, rank=rest_rank)
        k += len(proj)
        for i, t in enumerate(layer_t):
            pk.add(t, need[k + i], late=late and i % 12 in (0, 2), rank=(n_l - 1 - i // 12) if bucketed else 0)
        k += len(layer_t)
        # (the token classifier's gradients, egx_token_ce, live in the flat buffer too: zero-filled, reduced and all-reduced with the rest)
        for i, t in enumerate((*head_t, *tail)):
            pk.add(t, need[k + i], rank=rest_rank)
        g = pk.materialise(device, zero=False)      # zero-filled by the backward's first launch (egx_config.zero_buf)
        self.flat, self.lead = pk.flat, at - 4
        a, b, c = 4 + len(proj), 4 + len(proj) + len(layer_t), 4 + len(proj) + len(layer_t) + len(head_t)
        self.first, self.proj, self.layers, self.head, self.tail = g[:4], g[4:a], g[a:b], g[b:c], g[c:]

    def attach(self, cfg: Config):
        cfg.zero_buf, cfg.zero_bytes = ptr(self.flat), self.flat.numel() * 4

    def segments(self):
        """The `grads` of _segments()"""
        return self.feats, self.proj, self.first[0], self.first[1]

    def head_grads(self) -> HeadGrads:
        return HeadGrads(*map(ptr, self.head))

    def result(self, trailing: int = 0):
        """The backward's return value: None for the leading non-tensor arguments and `trailing` further ones (targets, class weights)."""
        return (None,) * self.lead + (*self.first, *self.feats, *self.proj, *self.layers, *self.head, *self.tail) + (None,) * trailing


def _attach_weight_cache(lib, spec: EncoderSpec, cfg: Config, segs, proj, layer_t, device):
    """Persistent packed-weight cache (spec.wcache): valid when nothing that goes into the packed copies changed since the forward that
    filled it. Sets cfg.weight_cache / weight_cache_valid; returns (cache, signature) — the caller stores the signature in cache.sig once
    its call has succeeded — or (None, None) where the configuration packs no weights."""
    wc = spec.wcache
    if wc is None:
        return None, None
    nbytes = lib.egx_weight_cache_bytes(C.byref(cfg), segs)
    if not nbytes:
        return None, None
    packed = proj[0::2] + [layer_t[12 * l + k] for l in range(spec.n_layers) for k in (0, 2, 4, 6)]
    keep = (1.0 / (1.0 - spec.p_drop)) if (spec.training and 0.0 < spec.p_drop < 1.0) else 1.0
    wc_sig = (spec.compute, keep, _weights_epoch[0], nbytes) + tuple((t.data_ptr(), t._version) for t in packed)
    if wc.buf is None or wc.buf.numel() < nbytes or wc.buf.device != device:
        wc.buf, wc.sig = torch.zeros(nbytes, dtype=torch.uint8, device=device), None
    capturing = torch.cuda.is_current_stream_capturing()
    valid = wc.sig == wc_sig and (wc.frozen or not capturing)
    cfg.weight_cache, cfg.weight_cache_valid = wc.buf.data_ptr(), int(valid)
    wc.hits += int(valid)
    wc.packs += int(not valid)
    wc.sig = None       # (set again once the call has succeeded)
    return wc, wc_sig


def _token_ce_attach(lib, spec: EncoderSpec, cfg: Config, segs, tce_in, fused: bool, B: int, S: int, device):
    """The fused per-token classifier + weighted cross entropy (spec.token_ce, egx_token_ce) attached to cfg. tce_in = (classifier weight,
    bias | None, target, class weight | None). Returns (keep-alive, (loss, logits, probs, pred, correct), d_logits, weight, bias | None)."""
    refusal = ("EncoderSpec.token_ce: this configuration does not evaluate the token classifier in its kernels "
               "(use functional.encoder_token_ce, which falls back to linear_cross_entropy)")
    Cn, d, Mrows = int(spec.token_ce), spec.d_model, B * (spec.out_tokens or S)
    if not fused:
        raise _lib.EgxError(refusal)
    tw = _dev_f32(tce_in[0], "classifier weight")
    tb = _dev_f32(tce_in[1], "classifier bias") if tce_in[1] is not None else None
    ttgt, tcw = tce_in[2], (None if tce_in[3] is None else _dev_f32(tce_in[3], "class weight"))
    if tuple(tw.shape) != (Cn, d) or ttgt.dtype != torch.int64 or tuple(ttgt.shape) != (Mrows,) or ttgt.device != device:
        raise ValueError(f"token classifier: weight must be ({Cn}, {d}) and target an int64 tensor of shape ({Mrows},) on the features' device")
    ttgt = ttgt.contiguous()
    t_logits = torch.empty((Mrows, Cn), dtype=torch.float32, device=device)
    t_probs, t_dl = torch.empty_like(t_logits), torch.empty_like(t_logits)
    t_pred = torch.empty((Mrows,), dtype=torch.float32, device=device)
    t_loss = torch.empty((), dtype=torch.float32, device=device)
    t_correct = torch.empty((), dtype=torch.float32, device=device)
    tce_struct = _lib.TokenCe(ptr(tw), ptr(tb), ptr(ttgt), ptr(tcw), Cn, ptr(t_logits), ptr(t_probs), ptr(t_pred), ptr(t_loss),
                              ptr(t_correct), ptr(t_dl), None, None)
    cfg.token_ce = C.cast(C.pointer(tce_struct), C.c_void_p)
    if not lib.egx_encoder_token_ce_ok(C.byref(cfg), segs, B):
        raise _lib.EgxError(refusal)
    return (tw, tb, ttgt, tcw, tce_struct), (t_loss, t_logits, t_probs, t_pred, t_correct), t_dl, tw, tb


class EncoderFn(torch.autograd.Function):
    """tokens(B,S,d) = encoder(token_prep(feats)) — or, with spec.head_n_out > 0, logits(B,n_out) = head(tokens).
    Argument order: spec, then _EncArgs' (task_embed|None, pos_table|None, ln_w, ln_b, feats[n_seg], (proj_w, proj_b) per projecting
    segment, 12 tensors per layer in _LAYER_FIELDS order, then (head_ln_w, head_ln_b, head_W, head_b) when a head is requested, then
    the tail of a fused loss)."""

    @staticmethod
    def forward(ctx, spec: EncoderSpec, task_embed, pos_table, ln_w, ln_b, *rest):
        lib = _load()
        nseg = len(spec.segments)
        nhead = 4 if spec.head_n_out else 0
        if spec.token_ce and (nhead or spec.ce):
            raise _lib.EgxError("EncoderSpec.token_ce cannot be combined with the pooled head")
        if spec.ce and not nhead:
            raise _lib.EgxError("EncoderSpec.ce needs the pooled head (head_n_out > 0)")
        feats, proj, layer_t, head_t, tail = _EncArgs.split(spec, rest)
        feats, proj, layer_t, head_t, ln_w, ln_b, task_embed, pos_table = _dev_params(feats, proj, layer_t, head_t, ln_w, ln_b, task_embed,
                                                                                      pos_table)
        assert len(layer_t) == 12 * spec.n_layers, "layer parameter count mismatch"
        d = spec.d_model
        B = feats[0].shape[0]
        device = feats[0].device
        segs = _segments(spec, feats, proj, task_embed, pos_table, B)
        layers = _layers(layer_t, spec.n_layers)

        # NB: grad mode is off inside Function.forward; ctx.needs_input_grad is the reliable signal.
        # needs_input_grad order: (spec, task_embed, pos_table, ln_w, ln_b, *rest)
        nig = ctx.needs_input_grad
        if spec.impl == "auto" and (nig[2] or any(nig[5:5 + nseg])):
            feat_grad = [bool(nig[5 + i]) for i in range(nseg)]
            probe_cfg = spec.config()
            wide_ident_only = (lib.egx_encoder_impl(C.byref(probe_cfg), segs, B) == EGX_IMPL_WIDE
                               and not any(fg and ss.has_proj for fg, ss in zip(feat_grad, spec.segments)))
            if any(feat_grad) and not wide_ident_only:
                # gradients into projected features: only the shape-generic backward produces them (the wide path serves
                # identity segments — the trainable action stream of the LTA translators — from its LayerNorm backward)
                spec = dataclasses.replace(spec, impl="generic")
            # (a learned positional table - the HOI translators' `pe` - gets its gradient from every implementation)
        # first-tokens-only output: in-kernel on the fused path; elsewhere the full block is sliced here (and the gradient
        # scattered back in backward)
        py_slice = 0
        if spec.out_tokens and nhead:
            raise _lib.EgxError("out_tokens (first-tokens-only output) cannot be combined with the fused pooled head: the head pools "
                                "every token of the clip")
        if spec.out_tokens:
            full = dataclasses.replace(spec, out_tokens=0)
            probe = full.config()
            if nhead or lib.egx_encoder_impl(C.byref(probe), segs, B) != EGX_IMPL_FUSED:
                py_slice, spec = spec.out_tokens, full
        cfg = spec.config()
        sv, sc = C.c_size_t(0), C.c_size_t(0)
        ws = lib.egx_translator_workspace if nhead else lib.egx_encoder_workspace
        check(ws(C.byref(cfg), segs, B, C.byref(sv), C.byref(sc)))
        S = sum(s.T for s in spec.segments)
        saved = _saved_buffer(any(nig), "saved", device, sv.value)
        scratch = _workspace("scratch", device, sc.value)
        seed = _seed64(spec.seed)
        wc, wc_sig = _attach_weight_cache(lib, spec, cfg, segs, proj, layer_t, device)
        keep = tw = tb = None       # (keep: what cfg.ce / cfg.token_ce point to, alive across the library call)
        if spec.ce:
            loss, ctx.ce_dl, keep = _ce_attach(spec, cfg, tail[0], tail[1], B, device)
        if spec.token_ce:
            keep, tce_out, ctx.tce_dl, tw, tb = _token_ce_attach(lib, spec, cfg, segs, tail, wc is not None and not py_slice, B, S, device)
        if nhead:
            head = _head(head_t, spec.head_n_out)
            tokens = torch.empty((B, spec.head_n_out), dtype=torch.float32, device=device)   # logits
            check(lib.egx_translator_fwd(C.byref(cfg), segs, ptr(ln_w), ptr(ln_b), layers, C.byref(head), B, ptr(tokens),
                                         None, ptr(saved), ptr(scratch), int(spec.training), seed, _stream()))
        else:
            tokens = torch.empty((B, spec.out_tokens or S, d), dtype=torch.float32, device=device)
            check(lib.egx_encoder_fwd(C.byref(cfg), segs, ptr(ln_w), ptr(ln_b), layers, B, ptr(tokens), ptr(saved),
                                      ptr(scratch), int(spec.training), seed, _stream()))
            if py_slice:
                tokens = tokens[:, :py_slice].contiguous()
        del keep
        if wc is not None:
            wc.sig = wc_sig
        ctx.wcache_buf = wc.buf if wc is not None else None     # the backward reads the packed copies from the same buffer
        ctx.py_slice, ctx.S, ctx.B = py_slice, S, B
        ctx.spec = spec
        ctx.impl = lib.egx_encoder_impl(C.byref(cfg), segs, B)       # EGX_IMPL_FUSED / EGX_IMPL_TILED / EGX_IMPL_WIDE / EGX_IMPL_GENERIC
        _last_impl[0] = ctx.impl
        _last_slices[0] = lib.egx_encoder_slices(C.byref(cfg), segs, B) if ctx.impl == EGX_IMPL_FUSED else 1
        ctx.saved_buf, ctx.scratch_bytes = saved, sc.value
        if _attention_sink is not None:     # (record_attention / encoder_attention: one more launch per selected layer, behind the forward)
            _attention_sink(lib, cfg, segs, B, None, spec, saved, device)
        _EncArgs.save(ctx, task_embed, pos_table, ln_w, ln_b, feats, proj, layer_t, head_t, [t for t in (tw, tb) if t is not None])
        if spec.token_ce:
            ctx.mark_non_differentiable(*tce_out[1:])
            ctx.set_materialize_grads(False)
            return (tokens,) + tce_out
        if spec.ce:
            ctx.set_materialize_grads(False)
            return tokens, loss
        return tokens

    @staticmethod
    def backward(ctx, d_tokens, d_loss=None, *_aux):
        spec: EncoderSpec = ctx.spec
        dl_scale = None
        if spec.token_ce:
            # (tokens, loss, ...) outputs: the loss's d_logits was left by the forward; the backward's first launch rebuilds d tokens from it
            if d_tokens is not None:
                raise _lib.EgxError("EncoderSpec.token_ce: a gradient through the returned tokens as well as through the fused loss is not supported "
                                    "(compose encoder() and linear_cross_entropy() instead)")
            if d_loss is None:
                return (None,) * len(ctx.needs_input_grad)
            dl_scale = _f32c(d_loss)
            d_tokens = ctx.tce_dl       # (only its device is read below)
        if spec.ce:
            up = _ce_upstream(ctx, d_tokens, d_loss)
            if up is None:
                return (None,) * len(ctx.needs_input_grad)
            d_tokens, dl_scale = up
        if ctx.py_slice:        # gradient of the python-side slice: zeros behind the first tokens
            full = torch.zeros((d_tokens.shape[0], ctx.S, d_tokens.shape[2]), dtype=torch.float32, device=d_tokens.device)
            full[:, :ctx.py_slice] = d_tokens
            d_tokens = full
        lib = _load()
        tensors = _EncArgs.load(ctx)
        task_embed, pos_table, ln_w, ln_b, feats, proj, layer_t, head_t, tce_t = tensors
        B = ctx.B
        device = d_tokens.device
        hook = bucket_hook
        gr = _EncGrads(spec, ctx.needs_input_grad, 5, tensors, device, late=hook is None, bucketed=hook is not None)
        pk = gr.pk
        segs, sgr = _segments(spec, feats, proj, task_embed, pos_table, B, grads=gr.segments())
        layers, lgr = _layers(layer_t, spec.n_layers, gr.layers)

        cfg = spec.config()
        gr.attach(cfg)
        if ctx.wcache_buf is not None:
            cfg.weight_cache = ctx.wcache_buf.data_ptr()
        if dl_scale is not None:
            cfg.d_logits_scale = dl_scale.data_ptr()
        tce_keep = None
        if spec.token_ce:
            tce_keep = _lib.TokenCe(ptr(tce_t[0]), None, None, None, int(spec.token_ce), None, None, None, None, None, ptr(ctx.tce_dl),
                                    *map(ptr, (gr.tail + [None])[:2]))
            cfg.token_ce = C.cast(C.pointer(tce_keep), C.c_void_p)
        announced = set()
        cb_keep = None
        if hook is not None and ctx.impl == EGX_IMPL_WIDE:
            flat_for_cb, spans = pk.flat, dict(pk.rank_span)

            cb_error = []

            def _cb(_user, bucket):       # host callback from wide_encoder_bwd: layer n_l - 1 - bucket is complete on the stream
                # ctypes swallows an exception raised in a callback ("Exception ignored"): keep it, leave the bucket
                # un-announced (the remainder pass below then covers its slice) and re-raise once the launch has returned
                if cb_error or bucket not in spans or bucket in announced:
                    return
                try:
                    hook(flat_for_cb, spans[bucket][0], spans[bucket][1])
                    announced.add(bucket)
                except BaseException as e:     # noqa: BLE001
                    cb_error.append(e)
            cb_keep = _lib.BUCKET_CB(_cb)
            cfg.bucket_cb = C.cast(cb_keep, C.c_void_p)
        defer = bool(spec.defer_small) and ctx.impl == EGX_IMPL_FUSED
        cfg.bwd_stage = 1 if defer else 0
        scratch = _workspace("scratch", device, ctx.scratch_bytes)
        seed = _seed64(spec.seed)
        saved_buf = ctx.saved_buf
        # raw addresses only inside `launch`: a closure that kept the gradient VIEW tensors alive (or `gr`, which holds them) would
        # make autograd clone them instead of adopting them as .grad (they must stay views of the flat buffer)
        p_lnw, p_lnb, flat_buf = ptr(gr.first[2]), ptr(gr.first[3]), pk.flat
        if head_t:
            head, hg = _head(head_t, spec.head_n_out), gr.head_grads()
            dtok = _f32c(d_tokens)

            def launch(c):
                check(lib.egx_translator_bwd(C.byref(c), segs, ptr(ln_w), ptr(ln_b), layers, C.byref(head), B, ptr(dtok),
                                             ptr(saved_buf), ptr(scratch), sgr, p_lnw, p_lnb, lgr,
                                             C.byref(hg), int(spec.training), seed, _stream()))
        else:
            # the generic backward overwrites d_tokens (needs a private copy); the fused and wide kernels only read it
            if spec.token_ce:
                dtok = None
            else:
                dtok = _f32c(d_tokens)
                if dtok.data_ptr() == d_tokens.data_ptr() and ctx.impl == EGX_IMPL_GENERIC:
                    dtok = dtok.clone()

            def launch(c):
                check(lib.egx_encoder_bwd(C.byref(c), segs, ptr(ln_w), ptr(ln_b), layers, B, ptr(dtok), ptr(saved_buf),
                                          ptr(scratch), sgr, p_lnw, p_lnb, lgr, int(spec.training), seed,
                                          _stream()))
        launch(cfg)
        del tce_keep
        if cb_keep is not None and cb_error:
            raise cb_error[0]
        if hook is not None and not defer:
            # whatever the per-layer callbacks did not announce (other implementations: everything) is complete now
            done = sorted(pk.rank_span[b] for b in announced)
            cur = 0
            for lo, hi in done + [(pk.total, pk.total)]:
                if lo > cur:
                    hook(pk.flat, cur, lo)
                cur = max(cur, hi)
        last_grad_layout.update(flat=pk.flat, late_floats=pk.late_floats if defer else 0)
        if defer:
            # stage 2 (dW_proj, dW_in, dW_o) on request: same arguments, kept alive by this closure; the shared scratch
            # workspace must not be reused by another encoder call before run_deferred()
            cfg2 = spec.config()
            cfg2.bwd_stage = 2
            if ctx.wcache_buf is not None:
                cfg2.weight_cache = ctx.wcache_buf.data_ptr()
            keep = (flat_buf, tensors, dtok, scratch, saved_buf)   # noqa: F841  (referenced by `finish`: keeps the buffers alive)

            def finish(_keep=keep):
                launch(cfg2)
            _deferred.append(finish)
        # trailing: target, class weight (and a bias-less classifier's bias)
        return gr.result(2 if spec.ce else 4 - len(gr.tail) if spec.token_ce else 0)


def encoder(spec: EncoderSpec, feats: Sequence[torch.Tensor], task_embed, pos_table, ln_w, ln_b,
            proj: Sequence[torch.Tensor], layer_params: Sequence[torch.Tensor],
            head_params: Sequence[torch.Tensor] = (), ce=None):
    """head_params = (head_ln_w, head_ln_b, head_W, head_b) with spec.head_n_out = head_W.shape[0] -> logits.
    ce = (target (B,) int64, class_weight | None) with spec.ce: -> (logits, loss), the weighted cross entropy evaluated by the forward."""
    if spec.ce:
        return EncoderFn.apply(spec, task_embed, pos_table, ln_w, ln_b, *feats, *proj, *layer_params, *head_params, ce[0], ce[1])
    return EncoderFn.apply(spec, task_embed, pos_table, ln_w, ln_b, *feats, *proj, *layer_params, *head_params)


STAGE_ITEMS = {"PRE": 0, "XIN": 1, "QKV": 2, "RES1": 3, "X1": 4, "HID": 5, "ALIVE": 6, "RES2": 7, "G2": 8, "DHID": 9, "G1": 10, "ATTN_O": 11,
               "DQKV": 12, "DSEG": 13, "DX0": 14, "LSE": 15}        # include/egot2x.h EGX_STAGE_*
STAGE_NOT_KEPT = 2


class EncoderStages:
    """TEST INFRASTRUCTURE (tests/test_gpu_bf16_stages.py): the intermediates of ONE d = 128 encoder call, read back through the stage hooks
    (ABI v26, egx_encoder_stage_* / egx_ragged_stage_*). Construct it from any output of the call (logits, tokens or the fused loss) BEFORE the
    backward: it finds the call's autograd node (EncoderFn / RaggedEncoderFn), keeps its configuration, segments and `saved` buffer and
    rebuilds nothing else. The forward items can be read at once; the backward items live in the shared scratch workspace: read them after the
    backward and before any other encoder call. read() returns a (rows, cols) tensor (fp32; ALIVE: uint8), prefilled with NaN (255) so that
    an element the hook leaves unwritten shows, or None where the hook reports the item as not kept by this call's implementation."""

    def __init__(self, out: torch.Tensor):
        node = self._find(out.grad_fn)
        if node is None:
            raise _lib.EgxError("EncoderStages: no encoder call in the graph of this tensor")
        self._lib = _load()
        spec: EncoderSpec = node.spec
        tensors = _EncArgs.load(node)
        task_embed, pos_table, _, _, feats, proj, _, _, _ = tensors
        self.B = node.B
        self.ragged = isinstance(node, RaggedEncoderFn._backward_cls)
        self.lengths = node.lengths if self.ragged else None
        if self.ragged and (self.lengths.is_cuda or self.lengths.dtype != torch.int32):
            raise _lib.EgxError("EncoderStages: the ragged hooks read HOST lengths (the (B, K) int32 CPU tensor of ragged_lengths())")
        self.cfg = _ragged_train_config(spec) if self.ragged else spec.config()
        self.segs = _segments(spec, feats, proj, task_embed, pos_table, self.B)
        self.head_n_out = int(spec.head_n_out or spec.token_ce or 0)
        self.saved, self.scratch_bytes, self.device = node.saved_buf, node.scratch_bytes, feats[0].device
        self.spec = spec
        self._keep = tensors        # the segment array holds raw addresses

    @staticmethod
    def _find(fn):
        seen, todo = set(), [fn]
        while todo:
            f = todo.pop()
            if f is None or f in seen:
                continue
            seen.add(f)
            if isinstance(f, (EncoderFn._backward_cls, RaggedEncoderFn._backward_cls)):
                return f
            todo.extend(n for n, _ in f.next_functions)
        return None

    def _args(self):
        head = (self.B,) + ((self.lengths.data_ptr(),) if self.ragged else ()) + (self.head_n_out,)
        return (C.byref(self.cfg), self.segs) + head

    def info(self, item: str, layer: int = 0):
        """-> (rows, cols, kind) or None (not kept); kind 0 fp32, 1 bf16 values, 2 bits."""
        r, c, k = C.c_int(0), C.c_int(0), C.c_int(0)
        fn = self._lib.egx_ragged_stage_info if self.ragged else self._lib.egx_encoder_stage_info
        rc = fn(*self._args(), STAGE_ITEMS[item], layer, C.byref(r), C.byref(c), C.byref(k))
        if rc == STAGE_NOT_KEPT:
            return None
        check(rc)
        return r.value, c.value, k.value

    def read(self, item: str, layer: int = 0):
        inf = self.info(item, layer)
        if inf is None:
            return None
        rows, cols, kind = inf
        if kind == 2:
            out = torch.full((rows, cols), 255, dtype=torch.uint8, device=self.device)
        else:
            out = torch.full((rows, cols), float("nan"), dtype=torch.float32, device=self.device)
        scratch = _scratch_cache.get(("scratch", self.device.index))
        fn = self._lib.egx_ragged_stage_read if self.ragged else self._lib.egx_encoder_stage_read
        check(fn(*self._args(), ptr(self.saved), ptr(scratch) if scratch is not None else None, STAGE_ITEMS[item], layer, ptr(out), _stream()))
        return out


def ragged_lengths(lengths, B: int, T_pad: Sequence[int], order: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Frame counts of a ragged batch as the (B, K) int32 host tensor egx_ragged_fwd reads (K = len(T_pad) segments). `lengths` is a (B,)
    tensor / sequence (every segment of clip b has lengths[b] frames) or (B, K) with one column per feature argument; `order` maps segment k
    to its column (the argument order of the model method, where it differs from the token order). 1 <= T_{b,k} <= T_pad[k] (the padded
    length of feature k) or ValueError."""
    K = len(T_pad)
    t = lengths.detach() if isinstance(lengths, torch.Tensor) else torch.as_tensor(lengths)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"lengths must be integers, got {t.dtype}")
    t = t.to("cpu", torch.int64)
    if t.dim() == 1:
        t = t[:, None].expand(t.shape[0], K)
    if t.dim() != 2 or tuple(t.shape) != (B, K):
        raise ValueError(f"lengths has shape {tuple(t.shape)}: expected ({B},) or ({B}, {K}), one column per feature")
    if order is not None:
        t = t[:, list(order)]
    for k in range(K):
        col = t[:, k]
        if B and (int(col.min()) < 1 or int(col.max()) > T_pad[k]):
            raise ValueError(f"lengths of segment {k} must lie in 1 .. {T_pad[k]} (the padded length of its feature), got "
                             f"{int(col.min())} .. {int(col.max())}")
    return t.to(torch.int32).contiguous()


def _check_host_lengths(lengths, B: int, nseg: int) -> torch.Tensor:
    if not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or lengths.device.type != "cpu" or tuple(lengths.shape) != (B, nseg):
        raise ValueError(f"lengths must be the ({B}, {nseg}) int32 host tensor of ragged_lengths()")
    return lengths.contiguous()


def _length_groups(spec: EncoderSpec, feats, lengths: torch.Tensor, first_only: bool = False):
    """The clips of a ragged batch grouped by their length tuple, for the per-group fallback. Yields (clip indices, the group's spec with its
    segment lengths, the group's unpadded features); first_only: the group's spec returns the first segment's tokens only (out_tokens)."""
    groups = {}
    for b, row in enumerate(lengths.tolist()):
        groups.setdefault(tuple(row), []).append(b)
    for key, idx in groups.items():
        it = torch.tensor(idx, dtype=torch.int64, device=feats[0].device)
        fs = [f.index_select(0, it)[:, :T * max(ss.pool, 1)] for f, T, ss in zip(feats, key, spec.segments)]
        gspec = dataclasses.replace(spec, segments=[dataclasses.replace(ss, T=T) for ss, T in zip(spec.segments, key)],
                                    out_tokens=key[0] if first_only else spec.out_tokens)
        yield idx, gspec, fs


def _ragged_infer_setup(spec: EncoderSpec, feats, lengths, task_embed, pos_table, ln_w, ln_b, proj, layer_params, head_params, query: str,
                        out_layout: Optional[int] = None):
    """The shared start of encoder_ragged and encoder_ragged_tokens (call it under no_grad): the lengths (and out_layout) checked, the
    tensors on the device, segments, layers and the dropout-free configuration built, and the workspace asked for through `query`
    (egx_ragged_workspace / egx_ragged_encode_workspace). Returns (lib, lengths, the tensors as _dev_params gives them, segments, layers,
    config, workspace bytes — None where the ragged kernels do not cover the configuration and the grouped fallback has to run; the
    lengths themselves are valid: ragged_lengths() checked them)."""
    B = feats[0].shape[0]
    lengths = _check_host_lengths(lengths, B, len(spec.segments))
    if out_layout is not None:
        _check_out_layout(lengths, B, out_layout)
    lib = _load()
    params = _dev_params(feats, proj, layer_params, head_params, ln_w, ln_b, task_embed, pos_table)
    feats, proj, layer_t, _, ln_w, ln_b, task_embed, pos_table = params
    segs = _segments(spec, feats, proj, task_embed, pos_table, B)
    layers = _layers(layer_t, spec.n_layers)
    cfg = dataclasses.replace(spec, p_drop=0.0, p_pos=0.0, p_feat=0.0).config()
    nbytes = C.c_size_t(0)
    covered = getattr(lib, query)(C.byref(cfg), segs, B, lengths.data_ptr(), C.byref(nbytes)) == 0
    return lib, lengths, params, segs, layers, cfg, (nbytes.value if covered else None)


def encoder_ragged(spec: EncoderSpec, feats: Sequence[torch.Tensor], lengths: torch.Tensor, task_embed, pos_table, ln_w, ln_b,
                   proj: Sequence[torch.Tensor], layer_params: Sequence[torch.Tensor], head_params: Sequence[torch.Tensor] = ()):
    """Inference forward (no autograd) over a batch of clips of their own lengths: clip b's result is that of the same model on clip b
    alone, unpadded. feats[k] is padded (B, spec.segments[k].T, d_in); `lengths` the (B, K) int32 host tensor of ragged_lengths().
    Returns logits (B, n_out) with head_params (spec.head_n_out > 0), else the first segment's rows of every clip packed in clip order,
    (sum_b lengths[b, 0], d). Runs egx_ragged_fwd (last_encoder_impl() == "ragged") where the tiled kernels cover the configuration;
    elsewhere the clips are grouped by their length tuple and each group runs the batched forward ("grouped")."""
    if spec.training or spec.ce or spec.token_ce or spec.out_tokens:
        raise ValueError("ragged batches are inference-only: no training mode, no fused losses, no out_tokens")
    with torch.no_grad():
        lib, lengths, params, segs, layers, cfg, nbytes = _ragged_infer_setup(spec, feats, lengths, task_embed, pos_table, ln_w, ln_b, proj,
                                                                              layer_params, head_params, "egx_ragged_workspace")
        feats, proj, layer_t, head_t, ln_w, ln_b, task_embed, pos_table = params
        if nbytes is None:
            _attention_unserved("a ragged batch outside the ragged d = 128 kernels (it runs as per-length groups)")
            rows = _clip_rows([1] * len(lengths) if head_t else lengths[:, 0].tolist())
            return _encoder_grouped(spec, feats, lengths, task_embed, pos_table, ln_w, ln_b, proj, layer_t, head_t, rows, first_only=not head_t)
        B, device = feats[0].shape[0], feats[0].device
        ws = _workspace("saved", device, nbytes)
        wc, wc_sig = _attach_weight_cache(lib, spec, cfg, segs, proj, layer_t, device)
        if head_t:
            head = _head(head_t, spec.head_n_out)
            out = torch.empty((B, spec.head_n_out), dtype=torch.float32, device=device)
            check(lib.egx_ragged_fwd(C.byref(cfg), segs, lengths.data_ptr(), ptr(ln_w), ptr(ln_b), layers, C.byref(head), B, ptr(out), None,
                                     ptr(ws), _stream()))
        else:
            out = torch.empty((int(lengths[:, 0].sum()), spec.d_model), dtype=torch.float32, device=device)
            check(lib.egx_ragged_fwd(C.byref(cfg), segs, lengths.data_ptr(), ptr(ln_w), ptr(ln_b), layers, None, B, None, ptr(out),
                                     ptr(ws), _stream()))
        if wc is not None:
            wc.sig = wc_sig
    _last_impl[0] = IMPL_RAGGED
    _last_slices[0] = 1
    if _attention_sink is not None:
        _attention_sink(lib, cfg, segs, B, lengths, spec, ws, device)
    return out


def _clip_rows(counts) -> tuple:
    """Per clip the int64 host tensor of the output rows its result occupies when clip b fills counts[b] rows, clip after clip."""
    return torch.arange(sum(counts), dtype=torch.int64).split(list(counts))


def _encoder_grouped(spec: EncoderSpec, feats, lengths, task_embed, pos_table, ln_w, ln_b, proj, layer_t, head_t, rows, first_only=False):
    """The ragged entry points where the ragged kernels do not run (exact fp32, a forced implementation, deeper stacks, clips beyond the
    kernels' reach): one batched encoder() per group of clips with the same length tuple, on those clips' unpadded frames. rows[b] names the
    output rows of clip b's result (int64 host tensors: the clip index for the pooled head, the packed rows of the first segment, a slice of
    ragged_token_rows()); the rows are put in place by one cat + index_select of the inverse permutation, which autograd flows through
    unless the caller runs under no_grad."""
    parts, dst = [], []
    for idx, gspec, fs in _length_groups(spec, feats, lengths, first_only):
        r = encoder(gspec, fs, task_embed, pos_table, ln_w, ln_b, proj, layer_t, head_t)
        parts.append(r.reshape(-1, r.shape[-1]))
        dst += [rows[b] for b in idx]
    if parts:
        dst = torch.cat(dst)
        inv = torch.empty_like(dst)
        inv[dst] = torch.arange(dst.numel())
        out = torch.cat(parts, 0).index_select(0, inv.to(feats[0].device))
    else:       # (a batch of no clips)
        out = torch.empty((0, spec.head_n_out if head_t else spec.d_model), dtype=torch.float32, device=feats[0].device)
    _last_impl[0] = IMPL_GROUPED
    _last_slices[0] = 1
    return out


def _ragged_train_config(spec: EncoderSpec) -> Config:
    """The configuration of a ragged training call: the packed weight copies live in `saved` (no persistent weight cache), so a forward is
    always back-propagated with the copies it packed itself, whatever another forward re-packs in between."""
    cfg = spec.config()
    cfg.weight_cache, cfg.weight_cache_valid = None, 0
    return cfg


_NO_POS_GRAD = "ragged training: a learned positional table gets no gradient from the ragged kernels"


def _ragged_train_setup(spec: EncoderSpec, rest, ln_w, ln_b, task_embed, pos_table, wide: bool = False):
    """The start of a ragged training forward: `rest` split (_EncArgs.split; wide: RaggedWideEncoderFn's), the tensors on the device (the
    features fp32, or bf16 too on the wide path), then the segments, the layers and the ragged training configuration.
    Returns (tensors in _EncArgs.load's order, segments, layers, config)."""
    feats, proj, layer_t, head_t, tail = _EncArgs.split(spec, rest, wide)
    feats, proj, layer_t, head_t, ln_w, ln_b, task_embed, pos_table = _dev_params(feats, proj, layer_t, head_t, ln_w, ln_b, task_embed,
                                                                                  pos_table, feat=_dev_feat if wide else _dev_f32)
    segs = _segments(spec, feats, proj, task_embed, pos_table, feats[0].shape[0])
    return (task_embed, pos_table, ln_w, ln_b, feats, proj, layer_t, head_t, tail), segs, _layers(layer_t, spec.n_layers), _ragged_train_config(spec)


def _ragged_train_plan(ctx, d_out, at: int):
    """The start of a ragged training backward (ctx.spec, ctx.B, ctx.scratch_bytes and _EncArgs.save's tensors; `at`: the index of feats[0]
    among the Function's arguments): a learned positional table's gradient refused, then the gradient plan attached to the configuration.
    Returns (tensors, _EncGrads, (segments, their gradients), (layers, their gradients), config, scratch, the upstream gradient fp32)."""
    spec, need = ctx.spec, ctx.needs_input_grad
    if need[at - 3]:
        raise _lib.EgxError(_NO_POS_GRAD)
    tensors = _EncArgs.load(ctx)
    task_embed, pos_table, _, _, feats, proj, layer_t, _, _ = tensors
    gr = _EncGrads(spec, need, at, tensors, d_out.device)
    segs = _segments(spec, feats, proj, task_embed, pos_table, ctx.B, grads=gr.segments())
    layers = _layers(layer_t, spec.n_layers, gr.layers)
    cfg = _ragged_train_config(spec)
    gr.attach(cfg)
    return tensors, gr, segs, layers, cfg, _workspace("scratch", d_out.device, ctx.scratch_bytes), _f32c(d_out)


class RaggedEncoderFn(torch.autograd.Function):
    """Training forward + backward of the d = 128 translators over a ragged batch. Argument order: spec, lengths, capacity, status, then
    _EncArgs' (task_embed | None, pos_table | None, ln_w, ln_b, feats[n_seg], (proj_w, proj_b) per segment, 12 tensors per layer,
    (head_ln_w, head_ln_b, head_W, head_b) with spec.head_n_out, then (target, class_weight | None) with spec.ce).
    capacity None, the host-table form (egx_ragged_train_fwd / egx_ragged_bwd): lengths is the (B, K) int32 host tensor of ragged_lengths().
    Returns logits (B, n_out) [, loss] with a head, else the first segment's rows of every clip, packed (sum_b T_{b,0}, d).
    capacity (B_cap, tok_cap), the capturable form with the batch table built on the device (egx_ragged_cap_train_fwd / egx_ragged_cap_bwd):
    lengths is CUDA int32 (B_cap, K), all-zero rows are empty clips; status CUDA int32 (1,); one graph serves every batch that fits the
    capacity. A head is required. Returns logits (B_cap, n_out) [, loss]."""

    @staticmethod
    def forward(ctx, spec: EncoderSpec, lengths, capacity, status, task_embed, pos_table, ln_w, ln_b, *rest):
        lib = _load()
        tensors, segs, layers, cfg = _ragged_train_setup(spec, rest, ln_w, ln_b, task_embed, pos_table)
        task_embed, pos_table, ln_w, ln_b, feats, proj, layer_t, head_t, tail = tensors
        B, device = feats[0].shape[0], feats[0].device
        host = capacity is None
        sv, sc = C.c_size_t(0), C.c_size_t(0)
        if host:
            check(lib.egx_ragged_train_workspace(C.byref(cfg), segs, B, lengths.data_ptr(), C.byref(sv), C.byref(sc)))
        else:
            check(lib.egx_ragged_cap_workspace(C.byref(cfg), segs, B, capacity[1], C.byref(sv), C.byref(sc)))
        saved = _saved_buffer(any(ctx.needs_input_grad), "saved", device, sv.value)
        keep = None
        if spec.ce:
            loss, ctx.ce_dl, keep = _ce_attach(spec, cfg, tail[0], tail[1], B, device)
        if head_t:
            head = _head(head_t, spec.head_n_out)
            out = torch.empty((B, spec.head_n_out), dtype=torch.float32, device=device)
            outs = (ptr(out), None)
        else:       # (the first segment's rows: the host form only, the capacity form's checks ask for a head)
            out = torch.empty((int(lengths[:, 0].sum()), spec.d_model), dtype=torch.float32, device=device)
            outs = (None, ptr(out))
        fwd, cap, st = (lib.egx_ragged_train_fwd, (), ()) if host else (lib.egx_ragged_cap_train_fwd, (capacity[1],), (ptr(status),))
        check(fwd(C.byref(cfg), segs, lengths.data_ptr(), ptr(ln_w), ptr(ln_b), layers, C.byref(head) if head_t else None, B, *cap, *outs,
                  ptr(saved), None, *st, int(spec.training), _seed64(spec.seed), _stream()))
        del keep
        _last_impl[0] = IMPL_RAGGED if host else IMPL_RAGGED_CAP
        _last_slices[0] = 1
        if host and _attention_sink is not None:
            _attention_sink(lib, cfg, segs, B, lengths, spec, saved, device)
        # (the lengths: the backward rebuilds the same plan from them, on the host or on the device)
        ctx.spec, ctx.lengths, ctx.B, ctx.capacity, ctx.status = spec, lengths, B, capacity, status
        ctx.saved_buf, ctx.scratch_bytes = saved, sc.value
        _EncArgs.save(ctx, *tensors[:8])
        if spec.ce:
            ctx.set_materialize_grads(False)
            return out, loss
        return out

    @staticmethod
    def backward(ctx, d_out, d_loss=None):
        spec: EncoderSpec = ctx.spec
        dl_scale = None
        if spec.ce:
            up = _ce_upstream(ctx, d_out, d_loss)
            if up is None:
                return (None,) * len(ctx.needs_input_grad)
            d_out, dl_scale = up
        lib = _load()
        tensors, gr, (segs, sgr), (layers, lgr), cfg, scratch, up = _ragged_train_plan(ctx, d_out, 8)
        ln_w, ln_b, head_t = tensors[2], tensors[3], tensors[7]
        if dl_scale is not None:
            cfg.d_logits_scale = dl_scale.data_ptr()
        if head_t:
            head, hg = _head(head_t, spec.head_n_out), gr.head_grads()
            p_head, p_hg, ups = C.byref(head), C.byref(hg), (ptr(up), None)
        else:
            p_head, p_hg, ups = None, None, (None, ptr(up))
        bwd, cap, st = (lib.egx_ragged_bwd, (), ()) if ctx.capacity is None else (lib.egx_ragged_cap_bwd, (ctx.capacity[1],), (ptr(ctx.status),))
        check(bwd(C.byref(cfg), segs, ctx.lengths.data_ptr(), ptr(ln_w), ptr(ln_b), layers, p_head, ctx.B, *cap, *ups, ptr(ctx.saved_buf),
                  ptr(scratch), sgr, ptr(gr.first[2]), ptr(gr.first[3]), lgr, p_hg, *st, int(spec.training), _seed64(spec.seed), _stream()))
        return gr.result(2 if spec.ce else 0)


_cap_status: dict = {}


def ragged_cap_status_word(device: torch.device) -> torch.Tensor:
    """The sticky int32 status word (one per device) that capacity-plan ragged calls OR their refusals into when no word of the caller's own
    is passed (egx_ragged_cap_train_fwd `status`). Created outside any capture: inside one it would live in the graph's private pool."""
    key = device.index
    w = _cap_status.get(key)
    if w is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ragged capacity: run one eager step before capturing (the status word is allocated outside the graph)")
        w = _cap_status[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return w


def _check_ragged_cap(spec: EncoderSpec, feats, lengths, capacity, status, pos_table, head_params):
    """encoder_ragged_train with DEVICE lengths: the checks that need no look at the lengths (nothing here synchronises). Returns (lengths,
    capacity, status) as RaggedEncoderFn takes them. There is no fallback: a configuration the ragged kernels do not cover raises with the
    library's message."""
    K = len(spec.segments)
    if capacity is None or len(capacity) != 2:
        raise ValueError("device lengths need capacity=(B_cap, tok_cap): the clips and the tokens the captured step is sized for")
    B_cap, tok_cap = int(capacity[0]), int(capacity[1])
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (B_cap, K) or lengths.device != feats[0].device:
        raise ValueError(f"device lengths must be the ({B_cap}, {K}) int32 tensor of the capacity, on the features' device")
    if any(f.shape[0] != B_cap for f in feats):
        raise ValueError(f"the features of a capacity batch are padded to B_cap = {B_cap} clips (train.pad_ragged_batch)")
    if not head_params:
        raise ValueError("ragged capacity: a pooled head is required (head-less rows are not supported on the captured path)")
    if pos_table is not None and pos_table.requires_grad and torch.is_grad_enabled():
        raise _lib.EgxError(_NO_POS_GRAD)
    if status is None:
        status = ragged_cap_status_word(feats[0].device)
    elif status.dtype != torch.int32 or status.numel() != 1 or status.device != feats[0].device:
        raise ValueError("status must be a one-element int32 tensor on the features' device")
    return lengths.contiguous(), (B_cap, tok_cap), status


def _ragged_train_refused(spec: EncoderSpec, feats, lengths, task_embed, pos_table, proj, query: str) -> bool:
    """The pre-flight of encoder_ragged_train and encoder_ragged_tokens_train: does the call have to take the grouped path? It does where
    a learned positional table wants a gradient (the ragged kernels produce none) or where the workspace query refuses the configuration
    (the lengths themselves are valid: ragged_lengths() checked them)."""
    lib = _lib.load()
    B = feats[0].shape[0]
    segs = _segments(spec, feats, proj, task_embed, pos_table, B)
    sv, sc = C.c_size_t(0), C.c_size_t(0)
    return (pos_table is not None and pos_table.requires_grad and torch.is_grad_enabled()) or \
        getattr(lib, query)(C.byref(_ragged_train_config(spec)), segs, B, lengths.data_ptr(), C.byref(sv), C.byref(sc)) != 0


def encoder_ragged_train(spec: EncoderSpec, feats: Sequence[torch.Tensor], lengths: torch.Tensor, task_embed, pos_table, ln_w, ln_b,
                         proj: Sequence[torch.Tensor], layer_params: Sequence[torch.Tensor], head_params: Sequence[torch.Tensor] = (),
                         ce=None, capacity=None, status=None):
    """Differentiable forward over a batch of clips of their own lengths (training and evaluation): clip b's result is that of the same model
    on clip b alone, unpadded, and every clip keeps all of its frames. feats[k] is padded (B, spec.segments[k].T, d_in); `lengths` the (B, K)
    int32 host tensor of ragged_lengths(). Returns logits (B, n_out) with head_params — or (logits, loss) with ce = (target, class_weight |
    None), the weighted cross entropy over the batch — else the first segment's rows of every clip packed, (sum_b lengths[b, 0], d).
    Runs egx_ragged_train_fwd / egx_ragged_bwd (last_encoder_impl() == "ragged") where the tiled kernels cover the configuration. Elsewhere
    (exact fp32, a forced implementation, deeper stacks, clips beyond 512 tokens) the clips are grouped by their length tuple and each group
    runs the differentiable batched forward ("grouped"); its dropout masks are keyed per group and differ from the ragged kernels'.
    Capturable form: `lengths` a CUDA int32 (B_cap, K) tensor with capacity = (B_cap, tok_cap) — features, lengths and target padded to
    B_cap clips (train.pad_ragged_batch; an all-zero row of lengths is an empty clip: a zero row of logits, no part in the loss). The batch
    table is then built on the device (egx_ragged_cap_train_fwd / egx_ragged_cap_bwd, last_encoder_impl() == "ragged_cap"), nothing reads
    the lengths on the host, and one captured graph serves every batch with at most tok_cap tokens. A batch that does not fit, or lengths
    out of range, run as the empty batch and set `status` (int32 (1,), sticky; default ragged_cap_status_word()). A head is required."""
    if spec.token_ce or spec.out_tokens or spec.p_feat:
        raise ValueError("ragged training: no token loss, no out_tokens, no feature dropout")
    if spec.defer_small:
        raise ValueError("ragged training: the staged backward (defer_small) is not supported")
    if (ce is not None) != bool(spec.ce) or (ce is not None and not spec.head_n_out):
        raise ValueError("ce = (target, class_weight) goes with spec.ce and the pooled head")
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        _attention_unserved("the capacity form of a ragged batch (device lengths)")
        lengths, capacity, status = _check_ragged_cap(spec, feats, lengths, capacity, status, pos_table, head_params)
    elif capacity is not None:
        raise ValueError("capacity= goes with device lengths (a CUDA int32 tensor); host lengths size the call themselves")
    else:
        lengths, status = _check_host_lengths(lengths, feats[0].shape[0], len(spec.segments)), None
        if _ragged_train_refused(spec, feats, lengths, task_embed, pos_table, proj, "egx_ragged_train_workspace"):
            _attention_unserved("a ragged batch outside the ragged d = 128 kernels (it runs as per-length groups)")
            rows = _clip_rows([1] * len(lengths) if head_params else lengths[:, 0].tolist())
            # (the groups run without the fused loss and the weight cache: the loss is taken over the whole batch's logits)
            out = _encoder_grouped(dataclasses.replace(spec, ce=False, wcache=None), feats, lengths, task_embed, pos_table, ln_w, ln_b, proj,
                                   layer_params, head_params, rows, first_only=not head_params)
            return out if ce is None else (out, weighted_cross_entropy(out, ce[0], ce[1]))
    args = [spec, lengths, capacity, status, task_embed, pos_table, ln_w, ln_b, *feats, *proj, *layer_params, *head_params]
    if ce is not None:
        args += [ce[0], ce[1]]
    return RaggedEncoderFn.apply(*args)


def ragged_token_rows(lengths: torch.Tensor, out_layout: int = 0) -> torch.Tensor:
    """Host (B, K) int32 lengths -> int64 output row of every token of encoder_ragged_tokens(), in clip-major token order (clip b,
    segment k, frame t): packed clips (out_layout 0) or frame-major segment tuples (out_layout 1)."""
    B, K = lengths.shape
    S = lengths.to(torch.int64).sum(1)
    if out_layout == 0:
        return torch.arange(int(S.sum()), dtype=torch.int64)
    T = lengths[:, 0].to(torch.int64)
    F0 = torch.cumsum(T, 0) - T
    rows = []
    for b in range(B):
        f = F0[b] + torch.arange(int(T[b]), dtype=torch.int64)
        rows.append((K * f[None, :] + torch.arange(K, dtype=torch.int64)[:, None]).reshape(-1))
    return torch.cat(rows) if rows else torch.zeros(0, dtype=torch.int64)


def _check_out_layout(lengths: torch.Tensor, B: int, out_layout: int):
    if out_layout not in (0, 1):
        raise ValueError("out_layout must be 0 (packed clips) or 1 (frame-major segment tuples)")
    if out_layout == 1 and B and not bool((lengths == lengths[:, :1]).all()):
        b = int((lengths != lengths[:, :1]).any(1).nonzero()[0, 0])
        raise ValueError(f"out_layout 1 needs the segments of every clip to have equal lengths (clip {b}: {lengths[b].tolist()})")


def encoder_ragged_tokens(spec: EncoderSpec, feats: Sequence[torch.Tensor], lengths: torch.Tensor, task_embed, pos_table, ln_w, ln_b,
                          proj: Sequence[torch.Tensor], layer_params: Sequence[torch.Tensor], out_layout: int = 0):
    """Inference forward (no autograd) returning EVERY token of a ragged batch: feats[k] padded (B, spec.segments[k].T, d_in), `lengths` the
    (B, K) int32 host tensor of ragged_lengths(). out_layout 0: (sum_b S_b, d), clip after clip (S_b = sum_k T_{b,k}); out_layout 1 (every
    clip's segments of equal length T_b): (K sum_b T_b, d), row K f + k = segment k of frame f of the batch. Runs egx_ragged_encode on the
    wide bf16 path (last_encoder_impl() == "ragged"); configurations it does not cover run one batched forward per length tuple ("grouped")."""
    if spec.training or spec.ce or spec.token_ce or spec.out_tokens or spec.head_n_out:
        raise ValueError("ragged batches are inference-only: no training mode, no fused losses, no out_tokens, no head")
    _attention_unserved("a ragged batch on the wide path")
    with torch.no_grad():
        lib, lengths, params, segs, layers, cfg, nbytes = _ragged_infer_setup(spec, feats, lengths, task_embed, pos_table, ln_w, ln_b, proj,
                                                                              layer_params, (), "egx_ragged_encode_workspace", out_layout)
        feats, proj, layer_t, _, ln_w, ln_b, task_embed, pos_table = params
        if nbytes is None:
            rows = ragged_token_rows(lengths, out_layout).split(lengths.sum(1).tolist())
            return _encoder_grouped(spec, feats, lengths, task_embed, pos_table, ln_w, ln_b, proj, layer_t, (), rows)
        B, device = feats[0].shape[0], feats[0].device
        ws = _workspace("ragged_wide", device, nbytes)
        out = torch.empty((int(lengths.to(torch.int64).sum()), spec.d_model), dtype=torch.float32, device=device)
        check(lib.egx_ragged_encode(C.byref(cfg), segs, lengths.data_ptr(), ptr(ln_w), ptr(ln_b), layers, B, ptr(out), int(out_layout),
                                    ptr(ws), _stream()))
    _last_impl[0] = IMPL_RAGGED
    _last_slices[0] = 1
    return out


class RaggedWideEncoderFn(torch.autograd.Function):
    """Training forward + backward of the wide bf16 encoder over a ragged batch (egx_ragged_encode_train_fwd / egx_ragged_encode_bwd): every
    token of every clip, packed (out_layout 0) or in frame-major segment tuples (out_layout 1). Argument order: spec, lengths (the (B, K)
    int32 host tensor of ragged_lengths()), out_layout, then _EncArgs' (task_embed | None, pos_table | None, ln_w, ln_b, feats[n_seg],
    (proj_w, proj_b) per segment, 12 tensors per layer). The call owns its `saved` workspace (batch table, bf16 weight copies, activations,
    dropout keys): a forward of the same module in between cannot change what a pending backward reads."""

    @staticmethod
    def forward(ctx, spec: EncoderSpec, lengths, out_layout: int, task_embed, pos_table, ln_w, ln_b, *rest):
        lib = _load()
        tensors, segs, layers, cfg = _ragged_train_setup(spec, rest, ln_w, ln_b, task_embed, pos_table, wide=True)
        ln_w, ln_b, feats = tensors[2], tensors[3], tensors[4]
        B, device = feats[0].shape[0], feats[0].device
        sv, sc = C.c_size_t(0), C.c_size_t(0)
        check(lib.egx_ragged_encode_train_workspace(C.byref(cfg), segs, B, lengths.data_ptr(), C.byref(sv), C.byref(sc)))
        saved = _saved_buffer(any(ctx.needs_input_grad), "ragged_wide_saved", device, sv.value)
        out = torch.empty((int(lengths.to(torch.int64).sum()), spec.d_model), dtype=torch.float32, device=device)
        check(lib.egx_ragged_encode_train_fwd(C.byref(cfg), segs, lengths.data_ptr(), ptr(ln_w), ptr(ln_b), layers, B, ptr(out), int(out_layout),
                                              ptr(saved), int(spec.training), _seed64(spec.seed), _stream()))
        _last_impl[0] = IMPL_RAGGED
        _last_slices[0] = 1
        ctx.spec, ctx.lengths, ctx.B, ctx.out_layout = spec, lengths, B, int(out_layout)
        ctx.saved_buf, ctx.scratch_bytes = saved, sc.value
        _EncArgs.save(ctx, *tensors[:8])
        return out

    @staticmethod
    def backward(ctx, d_out):
        spec: EncoderSpec = ctx.spec
        lib = _load()
        if any(ctx.needs_input_grad[7:7 + len(spec.segments)]):
            raise _lib.EgxError("ragged training: gradients into PROJECTED features are not supported on the wide path (detach the features)")
        tensors, gr, (segs, sgr), (layers, lgr), cfg, scratch, up = _ragged_train_plan(ctx, d_out, 7)
        check(lib.egx_ragged_encode_bwd(C.byref(cfg), segs, ctx.lengths.data_ptr(), ptr(tensors[2]), layers, ctx.B, ptr(up), ctx.out_layout,
                                        ptr(ctx.saved_buf), ptr(scratch), sgr, ptr(gr.first[2]), ptr(gr.first[3]), lgr, int(spec.training),
                                        _seed64(spec.seed), _stream()))
        return gr.result()


def encoder_ragged_tokens_train(spec: EncoderSpec, feats: Sequence[torch.Tensor], lengths: torch.Tensor, task_embed, pos_table, ln_w, ln_b,
                                proj: Sequence[torch.Tensor], layer_params: Sequence[torch.Tensor], out_layout: int = 0):
    """Differentiable encoder_ragged_tokens (training and evaluation, with and without grad): every token of a ragged batch, with dropout in
    training mode and gradients for the projections, task_embed, the shared LayerNorm and the encoder layers; the features themselves get none
    (projected features stay frozen on the wide path). Runs egx_ragged_encode_train_fwd / egx_ragged_encode_bwd (last_encoder_impl() ==
    "ragged"); configurations they do not cover (compute other than bf16, a forced implementation, a clip beyond the wide attention) run one
    differentiable batched forward per length tuple ("grouped"), whose dropout masks are keyed per group and differ from the ragged kernels'.
    The bucketed gradient exchange (functional.bucket_hook / egx_config.bucket_cb) is refused."""
    if spec.ce or spec.token_ce or spec.out_tokens or spec.head_n_out or spec.p_feat:
        raise ValueError("ragged training on the wide path: no fused losses, no out_tokens, no head, no feature dropout")
    if spec.defer_small:
        raise ValueError("ragged training: the staged backward (defer_small) is not supported")
    if bucket_hook is not None:
        raise ValueError("ragged training: the bucketed per-layer gradient exchange (bucket_cb) is not supported; exchange the gradients "
                         "after the backward (ddp.allreduce_gradients)")
    _attention_unserved("a ragged batch on the wide path")
    B = feats[0].shape[0]
    lengths = _check_host_lengths(lengths, B, len(spec.segments))
    _check_out_layout(lengths, B, out_layout)
    if len(proj) != 2 * len(spec.segments):
        raise ValueError("ragged training on the wide path: every segment needs a projection")
    if _ragged_train_refused(spec, feats, lengths, task_embed, pos_table, proj, "egx_ragged_encode_train_workspace"):
        rows = ragged_token_rows(lengths, out_layout).split(lengths.sum(1).tolist())
        return _encoder_grouped(dataclasses.replace(spec, wcache=None), feats, lengths, task_embed, pos_table, ln_w, ln_b, proj, layer_params,
                                (), rows)
    feats = [f.detach() for f in feats]      # (frozen backbone features: no gradient path on the wide projections)
    return RaggedWideEncoderFn.apply(spec, lengths, int(out_layout), task_embed, pos_table, ln_w, ln_b, *feats, *proj, *layer_params)


_last_dec_impl = ["none"]


def last_decoder_impl() -> str:
    """Diagnostic: the implementation the most recent EgoT2-g decode ran: "fused" (egx_decoder_fwd), "composed" (one library call per
    operation), "ragged" (egx_decoder_ragged_fwd / egx_decoder_ragged_train_fwd), "grouped" (a ragged memory decoded one length group at a
    time), "generate" (greedy generation in one egx_decoder_generate call), "loop" (greedy generation as a prefix loop over decode()),
    "beam" (beam search in one egx_decoder_beam call), "forced" (teacher-forced decoding of up to 64 target tokens in one
    egx_decoder_forced call) or "composed_long" (the composed decoder over 9 .. 64 target tokens, egx_target_attention_*: the
    differentiable route behind egx_long_targets)."""
    return _last_dec_impl[0]


def _dec_tensors(tokens, memory, emb, pe, layer_params, fc_w, fc_b):
    """The tensors of one decoder call, on the device, fp32 and contiguous; tokens ((B, sy) int64, None: the caller checks its own) too.
    Returns (tokens, memory, emb, pe, layer_t, fc_w, fc_b)."""
    layer_t = [_dev_f32(t, "decoder layer parameter") for t in layer_params]
    fc_w, fc_b = _dev_f32(fc_w, "fc.weight"), _dev_f32(fc_b, "fc.bias")
    memory, emb, pe = _dev_f32(memory, "memory"), _dev_f32(emb, "embedding.weight"), _dev_f32(pe, "positional rows")
    if tokens is not None:
        if tokens.dtype != torch.int64 or not tokens.is_cuda:
            raise _lib.EgxError("decoder tokens must be an int64 tensor on the GPU")
        tokens = tokens.contiguous()
    return tokens, memory, emb, pe, layer_t, fc_w, fc_b


def _dec_config(meta, d: int, V: int, sy: int, S: int, train: bool):
    """egx_dec_config; train: with meta's dropout rates and device seed (a training entry point), else dropout-free (inference)."""
    drop = (meta["p_drop"], meta["p_pos"], meta.get("seed_ptr") or None) if train else (0.0, 0.0, None)
    return _lib.DecConfig(d, meta["n_heads"], meta["d_ff"], meta["n_layers"], V, sy, S, meta["ln_eps"], EGX_BF16, *drop)


def _dec_layers(layer_t, n_layers: int, grads=None):
    """The egx_dec_layer array (18 tensors per layer in _lib._DEC_LAYER_FIELDS order); with grads (the same order, None where not wanted)
    also the egx_dec_layer_grads array: returns (layers, layer gradients)."""
    def array(struct, ts):
        arr = (struct * n_layers)()
        for l in range(n_layers):
            for k, name in enumerate(_lib._DEC_LAYER_FIELDS):
                setattr(arr[l], name, ptr(ts[18 * l + k]))
        return arr
    layers = array(_lib.DecLayer, layer_t)
    return layers if grads is None else (layers, array(_lib.DecLayerGrads, grads))


def decoder_ragged(meta, tokens, memory, mem_lengths: torch.Tensor, emb, pe, layer_params: Sequence[torch.Tensor], fc_w, fc_b,
                   return_attention: bool = False):
    """Inference decode (no autograd) over a packed ragged memory: tokens (B, sy) int64, memory (sum_b S_b, d) with S_b = mem_lengths[b]
    ((B,) int32 host tensor); clip b cross-attends to its own rows only. meta as DecoderFn's (p_drop / p_pos ignored: inference).
    Returns logits (B * sy, |V|) (egx_decoder_ragged_fwd); with return_attention (logits, attn (L, B, sy, max_b S_b) fp32): one
    egx_decoder_cross_weights call on the same workspace, zeros beyond S_b."""
    with torch.no_grad():
        return _decoder_ragged_fwd(None, meta, tokens, memory, mem_lengths, emb, pe, layer_params, fc_w, fc_b, return_attention)


def _decoder_ragged_fwd(ctx, meta, tokens, memory, mem_lengths, emb, pe, layer_params, fc_w, fc_b, return_attention=False):
    """The forward of decoder_ragged (ctx None: egx_decoder_ragged_fwd in one shared workspace) and of RaggedDecoderFn
    (egx_decoder_ragged_train_fwd into a `saved` of the call's own, kept in ctx for the backward)."""
    lib = _lib.load()
    tokens, memory, emb, pe, layer_t, fc_w, fc_b = _dec_tensors(tokens, memory, emb, pe, layer_params, fc_w, fc_b)
    B, sy = tokens.shape
    V, d = emb.shape
    ml = mem_lengths.contiguous()
    cfg_args = (d, V, sy, int(ml.max()))
    cfg = _dec_config(meta, *cfg_args, ctx is not None)
    layers = _dec_layers(layer_t, meta["n_layers"])
    logits = torch.empty((B * sy, V), dtype=torch.float32, device=memory.device)
    args = (C.byref(cfg), ptr(tokens), ptr(memory), ml.data_ptr(), ptr(emb), ptr(pe), pe.stride(0), layers, ptr(fc_w), ptr(fc_b), B, ptr(logits))
    if ctx is None:
        nb = C.c_size_t(0)
        check(lib.egx_decoder_ragged_workspace(C.byref(cfg), B, ml.data_ptr(), C.byref(nb)))
        ws = _workspace("dec_ragged", memory.device, nb.value)
        check(lib.egx_decoder_ragged_fwd(*args, ptr(ws), _stream()))
        if return_attention:
            attn = torch.empty((meta["n_layers"], B, sy, cfg_args[3]), dtype=torch.float32, device=memory.device)
            check(lib.egx_decoder_cross_weights(C.byref(cfg), B, ml.data_ptr(), ptr(ws), ptr(attn), _stream()))
            _last_dec_impl[0] = "ragged"
            return logits, attn
    else:
        sv, sc = C.c_size_t(0), C.c_size_t(0)
        check(lib.egx_decoder_ragged_train_workspace(C.byref(cfg), B, ml.data_ptr(), C.byref(sv), C.byref(sc)))
        saved = _saved_buffer(any(ctx.needs_input_grad), "dec_saved", memory.device, sv.value)
        scratch = _workspace("dec_scratch", memory.device, sc.value)
        check(lib.egx_decoder_ragged_train_fwd(*args, ptr(saved), ptr(scratch), int(meta["training"]), _seed64(meta["seed"]), _stream()))
        ctx.meta, ctx.cfg_args, ctx.B, ctx.ml, ctx.saved_buf, ctx.scratch_bytes = meta, cfg_args, B, ml, saved, sc.value
        ctx.save_for_backward(tokens, memory, emb, pe, *layer_t, fc_w, fc_b)
    _last_dec_impl[0] = "ragged"
    return logits


def _token_ce_fused(spec: EncoderSpec, feats, proj, task_embed, pos_table) -> bool:
    """Does this configuration evaluate EncoderSpec.token_ce in its kernels (egx_encoder_token_ce_ok)? Probed with the real feature / projection
    tensors; the weight cache only has to exist."""
    if spec.wcache is None or spec.deterministic or not spec.out_tokens or not all(f.is_cuda and f.dim() == 3 for f in feats):
        return False
    lib = _lib.load()
    segs = _segments(spec, feats, proj, task_embed, pos_table, feats[0].shape[0])
    cfg = spec.config()
    if lib.egx_encoder_impl(C.byref(cfg), segs, feats[0].shape[0]) != EGX_IMPL_FUSED:
        return False
    cfg.weight_cache = 1        # (any non-null value: the query does not touch it)
    return bool(lib.egx_encoder_token_ce_ok(C.byref(cfg), segs, feats[0].shape[0]))


def encoder_token_ce(spec: EncoderSpec, feats: Sequence[torch.Tensor], task_embed, pos_table, ln_w, ln_b,
                     proj: Sequence[torch.Tensor], layer_params: Sequence[torch.Tensor], fc_w, fc_b, target, class_weight=None):
    """(loss, logits, probs, pred, correct) of Linear(d -> C) + weighted cross entropy on the first spec.out_tokens tokens of every clip (rows in
    clip-major order, as encoder(...).reshape(B * out_tokens, d) has them): the ASD task's lossAV on the translator's per-frame output
    (HHI/tasks/asd/video_task_taskspecific.py:24,33). Where the per-clip kernels can, the encoder launches evaluate it themselves
    (egx_token_ce: two launches less per step); elsewhere encoder() + linear_cross_entropy()."""
    if _token_ce_fused(spec, feats, proj, task_embed, pos_table):
        spec = dataclasses.replace(spec, token_ce=int(fc_w.shape[0]))
        out = EncoderFn.apply(spec, task_embed, pos_table, ln_w, ln_b, *feats, *proj, *layer_params, fc_w, fc_b, target, class_weight)
        return out[1:]
    tokens = encoder(spec, feats, task_embed, pos_table, ln_w, ln_b, proj, layer_params)
    return linear_cross_entropy(tokens.reshape(-1, tokens.shape[-1]), fc_w, fc_b, target, class_weight)


class PoolHeadFn(torch.autograd.Function):
    """out = [Linear]([LN](mean_s tokens)); ln / linear are optional (None)."""

    @staticmethod
    def forward(ctx, tokens, ln_w, ln_b, W, b, eps: float):
        lib = _lib.load()
        tokens = _dev_f32(tokens, "tokens")
        B, S, d = tokens.shape
        ln_w = _dev_f32(ln_w, "ln weight") if ln_w is not None else None
        ln_b = _dev_f32(ln_b, "ln bias") if ln_b is not None else None
        W = _dev_f32(W, "head weight") if W is not None else None
        b = _dev_f32(b, "head bias") if b is not None else None
        n_out = W.shape[0] if W is not None else d
        pooled = torch.empty((B, d), dtype=torch.float32, device=tokens.device)
        out = torch.empty((B, n_out), dtype=torch.float32, device=tokens.device)
        check(lib.egx_pool_head_fwd(ptr(tokens), B, S, d, ptr(ln_w), ptr(ln_b), float(eps), ptr(W), ptr(b), n_out,
                                    ptr(pooled), ptr(out), _stream()))
        ctx.dims = (B, S, d, n_out, float(eps))
        ctx.has = (ln_w is not None, W is not None, b is not None)
        ctx.save_for_backward(*[t for t in (pooled, ln_w, ln_b, W) if t is not None])
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        B, S, d, n_out, eps = ctx.dims
        has_ln, has_W, has_b = ctx.has
        sv = list(ctx.saved_tensors)
        pooled = sv.pop(0)
        ln_w = sv.pop(0) if has_ln else None
        ln_b = sv.pop(0) if has_ln else None
        W = sv.pop(0) if has_W else None
        d_out = _f32c(d_out)
        dev = d_out.device
        d_tokens = torch.empty((B, S, d), dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad
        pk = _GradPacker()
        i_lw = pk.add(ln_w, has_ln and need[1])
        i_lb = pk.add(ln_b, has_ln and need[2])
        i_W = pk.add(W, has_W and need[3])
        i_b = pk.add(torch.empty(n_out, device="meta") if has_b else None, has_b and need[4])
        gr = pk.materialise(dev)

        def g(i):
            return gr[i] if i >= 0 else None

        check(lib.egx_pool_head_bwd(ptr(d_out), ptr(pooled), B, S, d, ptr(ln_w), ptr(ln_b), eps, ptr(W), n_out,
                                    ptr(d_tokens), ptr(g(i_lw)), ptr(g(i_lb)), ptr(g(i_W)), ptr(g(i_b)), _stream()))
        return (d_tokens if need[0] else None), g(i_lw), g(i_lb), g(i_W), g(i_b), None


def pool_head(tokens, ln_w=None, ln_b=None, W=None, b=None, eps: float = 1e-5):
    return PoolHeadFn.apply(tokens, ln_w, ln_b, W, b, eps)


class LinearFn(torch.autograd.Function):
    """y = x W^T + b for a 2-D x, through the MFMA GEMM. ordered_bias: the bias gradient is summed in a fixed order (egx_colsum_ordered:
    the same bits on every run) instead of egx_linear_bwd's atomic column sum."""

    @staticmethod
    def forward(ctx, x, W, b, compute: str, relu: bool = False, ordered_bias: bool = False):
        lib = _lib.load()
        x = _dev_f32(x, "x")
        W = _dev_f32(W, "W")
        b = _dev_f32(b, "b") if b is not None else None
        M, K = x.shape
        N = W.shape[0]
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        check(lib.egx_linear_fwd(ptr(x), ptr(W), ptr(b), ptr(y), M, N, K, int(relu), COMPUTE[compute], _stream()))
        ctx.compute = compute
        ctx.has_b = b is not None
        ctx.relu = bool(relu)
        ctx.ordered_bias = bool(ordered_bias)
        ctx.save_for_backward(*((x, W, y) if relu else (x, W)))
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, W = ctx.saved_tensors[:2]
        dy = _f32c(dy)
        if ctx.relu:                                  # d relu: zero the gradient where the output was clamped
            dy = dy.clone()
            check(lib.egx_relu_mask(ptr(dy), ptr(ctx.saved_tensors[2]), dy.numel(), _stream()))
        M, K = x.shape
        N = W.shape[0]
        need = ctx.needs_input_grad
        dev = dy.device
        dx = torch.empty_like(x) if need[0] else None
        dW = torch.zeros_like(W) if need[1] else None
        db = torch.zeros(N, dtype=torch.float32, device=dev) if (ctx.has_b and need[2]) else None
        ordered = ctx.ordered_bias and db is not None
        nbytes = lib.egx_linear_bwd_scratch(M, N, K)
        nb_cs = lib.egx_colsum_ordered_scratch(M, N) if ordered else 0
        scratch = _workspace("linear", dev, max(nbytes, nb_cs))
        if ordered:         # (ahead of the GEMMs that use the scratch next on the stream)
            check(lib.egx_colsum_ordered(ptr(dy), M, N, ptr(db), ptr(scratch), nb_cs, _stream()))
        check(lib.egx_linear_bwd(ptr(dy), ptr(x), ptr(W), ptr(dx), ptr(dW), None if ordered else ptr(db), M, N, K, COMPUTE[ctx.compute],
                                 ptr(scratch), _stream()))
        return dx, dW, db, None, None, None


class StackedLinearFn(torch.autograd.Function):
    """y = x Wst^T + bst where Wst / bst are the row-wise stack of several nn.Linear parameters that LIVE in that stack (their `.data` are views
    of it: hoi_lta.MultiTaskHead). One GEMM forward, one backward; the weight / bias gradients come back as views of ONE stacked gradient
    buffer each — no torch.cat of twenty weight matrices per step, no split of the gradient.
    Arguments: x (M, K), Wst (N, K), bst (N), sizes, compute, then the member weights and the member biases (gradient routing only)."""

    @staticmethod
    def forward(ctx, x, Wst, bst, sizes, compute: str, *members):
        lib = _lib.load()
        x = _dev_f32(x, "x")
        M, K = x.shape
        N = Wst.shape[0]
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        check(lib.egx_linear_fwd(ptr(x), ptr(Wst), ptr(bst), ptr(y), M, N, K, 0, COMPUTE[compute], _stream()))
        ctx.compute, ctx.sizes, ctx.nm = compute, tuple(sizes), len(members) // 2
        ctx.save_for_backward(x, Wst)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, Wst = ctx.saved_tensors
        dy = _f32c(dy)
        M, K = x.shape
        N = Wst.shape[0]
        need = ctx.needs_input_grad
        dev = dy.device
        dx = torch.empty_like(x) if need[0] else None
        want_w = any(need[5:5 + ctx.nm])
        want_b = any(need[5 + ctx.nm:])
        dW = torch.zeros_like(Wst) if want_w else None
        db = torch.zeros(N, dtype=torch.float32, device=dev) if want_b else None
        scratch = _workspace("linear", dev, lib.egx_linear_bwd_scratch(M, N, K))
        check(lib.egx_linear_bwd(ptr(dy), ptr(x), ptr(Wst), ptr(dx), ptr(dW), ptr(db), M, N, K, COMPUTE[ctx.compute],
                                 ptr(scratch), _stream()))
        gw, gb, off = [], [], 0
        for i, n in enumerate(ctx.sizes):
            gw.append(dW[off:off + n] if (dW is not None and need[5 + i]) else None)
            gb.append(db[off:off + n] if (db is not None and need[5 + ctx.nm + i]) else None)
            off += n
        return (dx, None, None, None, None, *gw, *gb)


def linear(x, W, b=None, compute: str = "f32", relu: bool = False, ordered_bias: bool = False):
    shp = x.shape
    y = LinearFn.apply(x.reshape(-1, shp[-1]), W, b, compute, relu, ordered_bias)
    return y.view(*shp[:-1], W.shape[0])


class LinearResidualFn(torch.autograd.Function):
    """y = x W^T (+ b) + residual: the residual connection rides in the GEMM epilogue (pre-LN blocks)."""

    @staticmethod
    def forward(ctx, x, W, b, residual, compute: str):
        lib = _lib.load()
        x, W, residual = _dev_f32(x, "x"), _dev_f32(W, "W"), _dev_f32(residual, "residual")
        b = _dev_f32(b, "b") if b is not None else None
        M, K = x.shape
        N = W.shape[0]
        if tuple(residual.shape) != (M, N):
            raise ValueError(f"residual shape {tuple(residual.shape)} != ({M}, {N})")
        y = torch.empty((M, N), dtype=torch.float32, device=x.device)
        check(lib.egx_linear_residual_fwd(ptr(x), ptr(W), ptr(b), ptr(residual), ptr(y), M, N, K, COMPUTE[compute], _stream()))
        ctx.compute, ctx.has_b = compute, b is not None
        ctx.save_for_backward(x, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, W = ctx.saved_tensors
        dy = _f32c(dy)
        M, K = x.shape
        N = W.shape[0]
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[0] else None
        dW = torch.zeros_like(W) if need[1] else None
        db = torch.zeros(N, dtype=torch.float32, device=dy.device) if (ctx.has_b and need[2]) else None
        scratch = _workspace("linear", dy.device, lib.egx_linear_bwd_scratch(M, N, K))
        check(lib.egx_linear_bwd(ptr(dy), ptr(x), ptr(W), ptr(dx), ptr(dW), ptr(db), M, N, K, COMPUTE[ctx.compute],
                                 ptr(scratch), _stream()))
        return dx, dW, db, (dy if need[3] else None), None


def linear_residual(x, W, b, residual, compute: str = "f32"):
    return LinearResidualFn.apply(x, W, b, residual, compute)


class GeluFn(torch.autograd.Function):
    """Exact (erf) GELU; the pre-activation is kept for the backward."""

    @staticmethod
    def forward(ctx, z):
        lib = _lib.load()
        z = _dev_f32(z, "z")
        h = torch.empty_like(z)
        check(lib.egx_gelu_fwd(ptr(z), ptr(h), z.numel(), _stream()))
        ctx.save_for_backward(z)
        return h

    @staticmethod
    def backward(ctx, dh):
        lib = _lib.load()
        (z,) = ctx.saved_tensors
        dh = _f32c(dh)
        dz = torch.empty_like(z)
        check(lib.egx_gelu_bwd(ptr(z), ptr(dh), ptr(dz), z.numel(), _stream()))
        return dz


def gelu(z):
    return GeluFn.apply(z)


class AttentionFn(torch.autograd.Function):
    """softmax(Q K^T / sqrt(dh)) V per (clip, head) from packed (B * S, 3 * inner) qkv rows -> (B * S, inner), through the
    shape-generic attention kernels (any S; inner = H * dh need not equal the model width)."""

    @staticmethod
    def forward(ctx, qkv, B: int, S: int, H: int):
        lib = _lib.load()
        qkv = _dev_f32(qkv, "qkv")
        inner = qkv.shape[1] // 3
        out = torch.empty((B * S, inner), dtype=torch.float32, device=qkv.device)
        lse = torch.empty((B, H, S), dtype=torch.float32, device=qkv.device)
        check(lib.egx_attention_fwd(ptr(qkv), ptr(out), ptr(lse), B, S, H, inner, 0.0, C.c_uint64(0), _stream()))
        ctx.dims = (B, S, H, inner)
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    def backward(ctx, d_out):
        lib = _lib.load()
        qkv, out, lse = ctx.saved_tensors
        B, S, H, inner = ctx.dims
        d_out = _f32c(d_out)
        dqkv = torch.empty_like(qkv)
        check(lib.egx_attention_bwd(ptr(qkv), ptr(out), ptr(lse), ptr(d_out), ptr(dqkv), B, S, H, inner, 0.0, C.c_uint64(0), _stream()))
        return dqkv, None, None, None


def attention(qkv, B: int, S: int, H: int):
    return AttentionFn.apply(qkv, B, S, H)


_UNIT_GRAD = {}


def unit_grad(device) -> torch.Tensor:
    """A persistent scalar 1.0 on `device` for `loss.backward(gradient=unit_grad(dev))`: autograd then needs no
    ones-fill, and weighted_cross_entropy recognises it and skips the multiplication by 1 (two launches per step)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    t = _UNIT_GRAD.get(key)
    if t is None:
        t = _UNIT_GRAD[key] = torch.ones((), dtype=torch.float32, device=torch.device("cuda", key))
    return t


def _scaled_by_upstream(dl: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """d loss / d logits as the forward launch left it, times the upstream gradient `g` of the loss. `dl` itself when `g` is
    unit_grad's tensor: multiplying by that 1 would be a launch."""
    u = _UNIT_GRAD.get(dl.device.index)
    return dl if u is not None and g.data_ptr() == u.data_ptr() else dl * g


class WeightedCEFn(torch.autograd.Function):
    """loss = sum_i w[y_i] nll_i / sum_i w[y_i]; the same launch leaves d loss / d logits behind for backward."""

    @staticmethod
    def forward(ctx, logits, target, weight):
        lib = _lib.load()
        z = _dev_f32(logits, "logits")
        if z.dim() != 2:
            raise ValueError(f"weighted_cross_entropy expects (B, C) logits, got {tuple(z.shape)}")
        if target.dtype != torch.int64 or target.shape != z.shape[:1] or target.device != z.device:
            raise ValueError("target must be an int64 tensor of shape (B,) on the logits' device")
        tgt = target.contiguous()
        w = None if weight is None else _dev_f32(weight, "weight")
        if w is not None and w.numel() != z.shape[1]:
            raise ValueError("weight must have one entry per class")
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        dl = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        check(lib.egx_weighted_ce(ptr(z), ptr(tgt), ptr(w) if w is not None else None, z.shape[0], z.shape[1],
                                  ptr(loss), ptr(dl) if dl is not None else None, _stream()))
        ctx.has_dl = dl is not None
        if dl is not None:
            ctx.save_for_backward(dl)       # autograd owns it: a second backward (retain_graph) sees the same gradient,
        return loss                         # a backward after the buffers were freed raises as for any other op

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.has_dl:
            return None, None, None
        (dl,) = ctx.saved_tensors
        return _scaled_by_upstream(dl, grad_out), None, None


class DecoderFn(torch.autograd.Function):
    """The EgoT2-g sequence decoder + vocabulary head as ONE library call per direction (egx_decoder_fwd / egx_decoder_bwd, compute =
    bf16): logits (B * sy, |V|) from target tokens (B, sy) and the encoder memory (B * S, d). Inputs after `meta`: memory, embedding
    weight, positional rows (sy, d), 18 tensors per layer in _lib._DEC_LAYER_FIELDS order, fc weight, fc bias. All parameter gradients
    are views of one flat buffer (zero-filled by the library's backward)."""

    @staticmethod
    def forward(ctx, meta, tokens, memory, emb, pe, *rest):
        lib = _lib.load()
        n = 18 * meta["n_layers"]
        tokens, memory, emb, pe, layer_t, fc_w, fc_b = _dec_tensors(tokens, memory, emb, pe, rest[:n], rest[n], rest[n + 1])
        B, sy = tokens.shape
        V, d = emb.shape
        cfg_args = (d, V, sy, memory.shape[0] // B)
        cfg = _dec_config(meta, *cfg_args, True)
        sv, sc = C.c_size_t(0), C.c_size_t(0)
        check(lib.egx_decoder_workspace(C.byref(cfg), B, C.byref(sv), C.byref(sc)))
        saved = _saved_buffer(any(ctx.needs_input_grad), "dec_saved", memory.device, sv.value)
        scratch = _workspace("dec_scratch", memory.device, sc.value)
        layers = _dec_layers(layer_t, meta["n_layers"])
        logits = torch.empty((B * sy, V), dtype=torch.float32, device=memory.device)
        check(lib.egx_decoder_fwd(C.byref(cfg), ptr(tokens), ptr(memory), ptr(emb), ptr(pe), pe.stride(0), layers, ptr(fc_w), ptr(fc_b), B,
                                  ptr(logits), ptr(saved), ptr(scratch), int(meta["training"]), _seed64(meta["seed"]), _stream()))
        ctx.meta, ctx.cfg_args, ctx.B, ctx.saved_buf, ctx.scratch_bytes = meta, cfg_args, B, saved, sc.value
        ctx.save_for_backward(tokens, memory, emb, pe, *layer_t, fc_w, fc_b)
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        return _decoder_backward(ctx, d_logits, ragged=False)


class RaggedDecoderFn(torch.autograd.Function):
    """DecoderFn over a packed ragged memory (egx_decoder_ragged_train_fwd / egx_decoder_ragged_bwd): logits (B * sy, |V|) from target
    tokens (B, sy) and the (sum_b S_b, d) memory, clip b cross-attending to its own S_b = mem_lengths[b] rows. Inputs after `meta`: tokens,
    memory, mem_lengths ((B,) int32 host tensor), embedding weight, positional rows (sy, d), 18 tensors per layer, fc weight, fc bias. The
    call owns its `saved` workspace; d_memory comes back packed."""

    @staticmethod
    def forward(ctx, meta, tokens, memory, mem_lengths, emb, pe, *rest):
        n = 18 * meta["n_layers"]
        return _decoder_ragged_fwd(ctx, meta, tokens, memory, mem_lengths, emb, pe, rest[:n], rest[n], rest[n + 1])

    @staticmethod
    def backward(ctx, d_logits):
        return _decoder_backward(ctx, d_logits, ragged=True)


def _decoder_backward(ctx, d_logits, ragged: bool):
    """The backward of DecoderFn (egx_decoder_bwd, announced to bucket_hook as one slice) and of RaggedDecoderFn (egx_decoder_ragged_bwd):
    ctx as their forwards left it, with cfg_args = (d, |V|, sy, S) of _dec_config."""
    lib = _lib.load()
    meta, B = ctx.meta, ctx.B
    n_layers = meta["n_layers"]
    sv = ctx.saved_tensors
    tokens, memory, emb = sv[:3]
    layer_t, fc_w, fc_b = sv[4:4 + 18 * n_layers], sv[4 + 18 * n_layers], sv[5 + 18 * n_layers]
    # needs_input_grad: (meta, tokens, memory, [mem_lengths,] emb, pe, *layer_t, fc_w, fc_b); nothing for pe
    need = ctx.needs_input_grad
    i_emb = 4 if ragged else 3
    pk = _GradPacker()
    for t, want in zip((emb, *layer_t, fc_w, fc_b), (need[i_emb],) + need[i_emb + 2:]):
        pk.add(t, want)
    g_emb, *g_layer, g_fcw, g_fcb = pk.materialise(d_logits.device, zero=False)
    d_memory = torch.empty_like(memory) if need[2] else None
    cfg = _dec_config(meta, *ctx.cfg_args, True)
    layers, lgr = _dec_layers(layer_t, n_layers, g_layer)
    scratch = _workspace("dec_scratch", d_logits.device, ctx.scratch_bytes)
    dl = _f32c(d_logits)
    args = (layers, ptr(fc_w), B, ptr(dl), ptr(ctx.saved_buf), ptr(scratch), ptr(d_memory), ptr(g_emb), lgr, ptr(g_fcw), ptr(g_fcb),
            ptr(pk.flat), pk.flat.numel() * 4, int(meta["training"]), _seed64(meta["seed"]), _stream())
    if ragged:
        check(lib.egx_decoder_ragged_bwd(C.byref(cfg), ptr(tokens), ctx.ml.data_ptr(), *args))
    else:
        check(lib.egx_decoder_bwd(C.byref(cfg), ptr(tokens), *args))
        if bucket_hook is not None and pk.total:
            bucket_hook(pk.flat, 0, pk.total)        # the decoder's gradients are exchanged while the encoder's backward runs
    return (None, None, d_memory) + ((None,) if ragged else ()) + (g_emb, None, *g_layer, g_fcw, g_fcb)


def decoder_attention(meta, tokens, memory, emb, pe, layer_params: Sequence[torch.Tensor], fc_w, fc_b):
    """DecoderFn's forward without autograd (inference: meta's dropout rates must be 0) that also returns the cross-attention weights:
    egx_decoder_fwd, then egx_decoder_cross_weights on the same `saved`. Returns (logits (B * sy, |V|), attn (L, B, sy, S) fp32); the
    logits have the bits DecoderFn gives."""
    lib = _lib.load()
    with torch.no_grad():
        tokens, memory, emb, pe, layer_t, fc_w, fc_b = _dec_tensors(tokens, memory, emb, pe, layer_params, fc_w, fc_b)
        B, sy = tokens.shape
        V, d = emb.shape
        S = memory.shape[0] // B
        cfg = _dec_config(meta, d, V, sy, S, True)
        sv, sc = C.c_size_t(0), C.c_size_t(0)
        check(lib.egx_decoder_workspace(C.byref(cfg), B, C.byref(sv), C.byref(sc)))
        saved = _workspace("dec_saved", memory.device, sv.value)
        scratch = _workspace("dec_scratch", memory.device, sc.value)
        layers = _dec_layers(layer_t, meta["n_layers"])
        logits = torch.empty((B * sy, V), dtype=torch.float32, device=memory.device)
        attn = torch.empty((meta["n_layers"], B, sy, S), dtype=torch.float32, device=memory.device)
        check(lib.egx_decoder_fwd(C.byref(cfg), ptr(tokens), ptr(memory), ptr(emb), ptr(pe), pe.stride(0), layers, ptr(fc_w), ptr(fc_b), B,
                                  ptr(logits), ptr(saved), ptr(scratch), 0, _seed64(0), _stream()))
        check(lib.egx_decoder_cross_weights(C.byref(cfg), B, None, ptr(saved), ptr(attn), _stream()))
    return logits, attn


CROSS_WEIGHTS_HEAD_DIMS = (16, 32, 64, 128)
CROSS_WEIGHTS_MAX_KEYS = 1024


def check_cross_weights(head_dim: int, Sk: int) -> None:
    """The limits of egx_cross_attention_weights as a ValueError that names them (host work, before any device call)."""
    if head_dim not in CROSS_WEIGHTS_HEAD_DIMS or not 1 <= Sk <= CROSS_WEIGHTS_MAX_KEYS:
        raise ValueError(f"cross-attention weights are served for head dims {CROSS_WEIGHTS_HEAD_DIMS} and 1..{CROSS_WEIGHTS_MAX_KEYS} memory "
                         f"tokens per clip: got head dim {head_dim}, {Sk} memory tokens")


def cross_attention_weights(q: torch.Tensor, k: torch.Tensor, n_heads: int, Sq: int, Sk: int, mtab: Optional[torch.Tensor] = None):
    """The head-averaged attention weights w[b, i, j] = (1 / H) sum_h softmax_j(q[b, i, h] . k[b, j, h] / sqrt(dh)) that
    nn.MultiheadAttention returns with need_weights=True (egx_cross_attention_weights; no autograd). q (B * Sq, H * dh) and k (B * Sk, H * dh),
    both fp32 or both bf16, rows b * Sq + i / b * Sk + j, head h at columns h * dh; 2-D views with unit column stride and a row stride that
    is a multiple of 8 elements are read in place (the q / k columns of packed projections). mtab ((B, 2) int32 on the device: first key
    row, key rows): ragged key sets, Sk then the longest; entries beyond a clip's rows come back as zeros. dh in (16, 32, 64, 128),
    Sk <= 1024. Returns (B, Sq, Sk) fp32."""
    lib = _lib.load()
    for name, t in (("q", q), ("k", k)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"cross_attention_weights: {name} must be a 2-D fp32 or bf16 tensor on the GPU")
    if q.dtype != k.dtype or q.shape[1] != k.shape[1] or n_heads < 1 or q.shape[1] % n_heads or Sq < 1 or q.shape[0] % Sq:
        raise ValueError(f"cross_attention_weights: q {tuple(q.shape)} {q.dtype} and k {tuple(k.shape)} {k.dtype} do not fit {n_heads} heads, "
                         f"Sq = {Sq}")
    check_cross_weights(q.shape[1] // n_heads, Sk)
    B = q.shape[0] // Sq
    q, k = [t if t.stride(1) == 1 and t.stride(0) % 8 == 0 else t.contiguous() for t in (q.detach(), k.detach())]
    if mtab is None:
        if k.shape[0] != B * Sk:
            raise ValueError(f"cross_attention_weights: k has {k.shape[0]} rows, expected B * Sk = {B * Sk}")
    elif not (isinstance(mtab, torch.Tensor) and mtab.is_cuda and mtab.dtype == torch.int32 and tuple(mtab.shape) == (B, 2)):
        raise ValueError(f"cross_attention_weights: mtab must be a ({B}, 2) int32 tensor on the GPU (first key row, key rows)")
    else:
        mtab = mtab.contiguous()
    out = torch.empty((B, Sq, Sk), dtype=torch.float32, device=q.device)
    check(lib.egx_cross_attention_weights(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), int(q.dtype == torch.bfloat16), ptr(mtab),
                                          B, n_heads, q.shape[1] // n_heads, Sq, Sk, ptr(out), Sk, _stream()))
    return out


def decoder_supported(compute: str, d: int, n_heads: int, d_ff: int, sy: int, S: int, n_layers: int) -> bool:
    """Shapes egx_decoder_fwd / egx_decoder_bwd serve (include/egot2x.h); everything else stays on the composed decoder. Head dim 32 / 64:
    d <= 1024, S <= 1024; head dim 256 / 512 (the 2048-wide LTA sequence decoders): d <= 2048, S <= 16."""
    if not (compute == "bf16" and d >= 256 and d % 128 == 0 and n_heads > 0 and d % n_heads == 0):
        return False
    dh = d // n_heads
    if not ((dh in (32, 64) and d <= 1024 and 1 <= S <= 1024) or (dh in DECODER_BIG_HEAD_DIMS and d <= 2048 and 1 <= S <= DECODER_BIG_HEAD_MAX_S)):
        return False
    return d_ff >= 128 and d_ff % 128 == 0 and 1 <= sy <= 8 and 1 <= n_layers <= 16


DECODER_BIG_HEAD_DIMS = (256, 512)      # wide_decoder_bighead.hip
DECODER_BIG_HEAD_MAX_S = 16


def decoder_ragged_supported(compute: str, d: int, n_heads: int, d_ff: int, sy: int, S: int, n_layers: int) -> bool:
    """Shapes egx_decoder_ragged_* serve: the fused decoder's at head dim 32 / 64 (the 256 / 512 class runs uniform batches only)."""
    return decoder_supported(compute, d, n_heads, d_ff, sy, S, n_layers) and d // n_heads not in DECODER_BIG_HEAD_DIMS


def decoder_generate_supported(compute: str, d: int, n_heads: int, d_ff: int, S: int, n_layers: int, vocab: int, n_steps: int) -> bool:
    """Configurations egx_decoder_generate serves (include/egot2x.h): the fused decoder's limits, n_steps <= 64, vocab <= 1024."""
    return decoder_supported(compute, d, n_heads, d_ff, 1, S, n_layers) and 1 <= n_steps <= 64 and 1 <= vocab <= 1024


class TokenSchedule:
    """Per-step word sets of greedy generation and beam search: `allowed` a (P, V) bool tensor, 1 <= P <= 64, no empty row; step t
    (0-based) may emit the words of row t % P (P = 2: the verb / noun alternation of HOI/models/lta/lta_models_seqdecoder.py:190-201;
    P = n_steps: a set per step). Validated on the host HERE (a GPU tensor is copied to the host once); holds .allowed (CPU bool (P, V)),
    .counts (list of P ints) and .words: the (P, V) int32 table on `device` the library reads, row p's first counts[p] entries the set's
    indices in ascending order, the rest padded with the last index. Build it once, outside any captured region, and reuse it."""
    MAX_PERIOD = 64

    def __init__(self, allowed: torch.Tensor, device):
        if not isinstance(allowed, torch.Tensor) or allowed.dtype != torch.bool:
            raise ValueError(f"allowed must be a (P, V) bool tensor, got {allowed.dtype if isinstance(allowed, torch.Tensor) else type(allowed).__name__}")
        if allowed.dim() != 2:
            raise ValueError(f"allowed must be a (P, V) bool tensor, got shape {tuple(allowed.shape)}")
        P, V = allowed.shape
        if not 1 <= P <= self.MAX_PERIOD or V < 1:
            raise ValueError(f"allowed has {P} rows over {V} words: a schedule has 1..{self.MAX_PERIOD} rows over at least one word")
        self.allowed = allowed.detach().to("cpu").clone()
        self.counts = [int(c) for c in self.allowed.sum(dim=1).tolist()]
        empty = [p for p, c in enumerate(self.counts) if c < 1]
        if empty:
            raise ValueError(f"allowed rows {empty} are empty: every step needs at least one word")
        # a stable descending sort of the 0 / 1 row puts the allowed indices first, ascending; the tail takes the last of them
        order = torch.sort(self.allowed.to(torch.int8), dim=1, descending=True, stable=True).indices
        last = order.gather(1, torch.tensor(self.counts)[:, None] - 1)
        words = torch.where(torch.arange(V)[None, :] < torch.tensor(self.counts)[:, None], order, last)
        self.words = words.to(torch.int32).contiguous().to(device)

    @property
    def period(self) -> int:
        return self.allowed.shape[0]

    @property
    def vocab(self) -> int:
        return self.allowed.shape[1]

    def _args(self):
        """(period, counts as a C int array, words pointer): the three trailing arguments of the _sched entry points."""
        return self.period, (C.c_int * self.period)(*self.counts), ptr(self.words)


def check_schedule(schedule, vocab: int, device=None, beam_width: int = 0) -> None:
    """The host checks of a schedule against one call (no library call): its V, for beam search step 0's set, and (device given) where its
    words live."""
    if not isinstance(schedule, TokenSchedule):
        raise ValueError(f"schedule must be a functional.TokenSchedule (model.token_schedule / model.verb_noun_schedule), got {type(schedule).__name__}")
    if schedule.vocab != vocab:
        raise ValueError(f"the schedule is over {schedule.vocab} words, the model's vocabulary has {vocab}")
    if beam_width > schedule.counts[0]:
        raise ValueError(f"beam_width = {beam_width} exceeds the {schedule.counts[0]} words step 0 may emit (at step 0 only one hypothesis is "
                         f"live: it has only that many continuations)")
    if device is not None and schedule.words.device != torch.device(device):
        raise ValueError(f"the schedule's words are on {schedule.words.device}, the memory on {torch.device(device)}: build the schedule on the "
                         f"memory's device")


def _cached_step_setup(who, lead, rank, lead_desc, meta, mem2d, emb, pe, layer_params, fc_w, fc_b, n_steps, query, also=None):
    """What decoder_generate, decoder_beam and decoder_forced open with (under no_grad): the tensors on the device (_dec_tensors), the
    check of the leading token tensor `lead` (of `rank`; lead_desc: its name and shape; n_steps None: its last extent), also(), the call's
    own argument checks, the memory / positional-row fit, the dropout-free config, the layer array and the workspace query(cfg, B, n_steps,
    nb) sizes.
    Returns (lead, V, cfg, model, ws, keep): model = the seven arguments from the memory to fc_b, which every entry point takes in this
    order; keep = the tensors behind them, to be held until the call is made."""
    _, mem2d, emb, pe, layer_t, fc_w, fc_b = _dec_tensors(None, mem2d, emb, pe, layer_params, fc_w, fc_b)
    if lead.dtype != torch.int64 or not lead.is_cuda or lead.dim() != rank:
        raise _lib.EgxError(f"{who}: {lead_desc} int64 tensor on the GPU")
    if also is not None:
        also()
    lead = lead.contiguous()
    B, (V, d) = lead.shape[0], emb.shape
    n_steps = lead.shape[-1] if n_steps is None else n_steps
    if B < 1 or mem2d.dim() != 2 or mem2d.shape[0] % B or mem2d.shape[1] != d or pe.shape[0] < n_steps:
        raise _lib.EgxError(f"{who}: memory {tuple(mem2d.shape)} / positional rows {tuple(pe.shape)} do not fit B = {B}, "
                            f"d = {d}, n_steps = {n_steps}")
    cfg = _dec_config(meta, d, V, 1, mem2d.shape[0] // B, False)
    layers = _dec_layers(layer_t, meta["n_layers"])
    nb = C.c_size_t(0)
    check(query(C.byref(cfg), B, n_steps, C.byref(nb)))
    ws = torch.empty(max(nb.value, 256), dtype=torch.uint8, device=mem2d.device)
    model = (ptr(mem2d), ptr(emb), ptr(pe), pe.stride(0), layers, ptr(fc_w), ptr(fc_b))
    return lead, V, cfg, model, ws, (mem2d, emb, pe, layer_t, fc_w, fc_b)


def decoder_generate(meta, start, mem2d, emb, pe, layer_params: Sequence[torch.Tensor], fc_w, fc_b, n_steps: int, return_logits: bool = False,
                     schedule: "TokenSchedule" = None, return_attention: bool = False):
    """Greedy generation in ONE asynchronous call (egx_decoder_generate; no autograd): start (B,) int64, mem2d (B * S, d) batch-first memory
    rows, pe (>= n_steps, d) positional rows, meta as DecoderFn's (dropout ignored: inference). Returns tokens (B, n_steps) int64 and, with
    return_logits, logits (n_steps, B, |V|) fp32 (else None). The workspace comes from the caching allocator: the call can be captured.
    With a TokenSchedule: egx_decoder_generate_sched, step t's argmax over the words of row t % P, the other logits -inf.
    With return_attention: egx_decoder_generate_attn and a third result, attn (L, n_steps, B, S) fp32, step t's head-averaged
    cross-attention weights of every layer; tokens and logits keep their bits."""
    lib = _lib.load()
    with torch.no_grad():
        start, V, cfg, model, ws, keep = _cached_step_setup("decoder_generate", start, 1, "start must be a (B,)", meta, mem2d, emb, pe, layer_params,
                                                            fc_w, fc_b, n_steps, lib.egx_decoder_generate_workspace)
        B, dev = start.shape[0], ws.device
        tokens = torch.empty((B, n_steps), dtype=torch.int64, device=dev)
        logits = torch.empty((n_steps, B, V), dtype=torch.float32, device=dev) if return_logits else None
        args = (C.byref(cfg), ptr(start), *model, B, n_steps, ptr(tokens), ptr(logits), ptr(ws), _stream())
        if schedule is not None:
            check_schedule(schedule, V, dev)
        if return_attention:
            attn = torch.empty((meta["n_layers"], n_steps, B, cfg.S), dtype=torch.float32, device=dev)
            check(lib.egx_decoder_generate_attn(*args, *((0, None, None) if schedule is None else schedule._args()), ptr(attn)))
        elif schedule is None:
            check(lib.egx_decoder_generate(*args))
        else:
            check(lib.egx_decoder_generate_sched(*args, *schedule._args()))
    _last_dec_impl[0] = "generate"
    return (tokens, logits, attn) if return_attention else (tokens, logits)


def decoder_beam_supported(compute: str, d: int, n_heads: int, d_ff: int, S: int, n_layers: int, vocab: int, n_steps: int, beam_width: int) -> bool:
    """Configurations egx_decoder_beam serves (include/egot2x.h): egx_decoder_generate's limits, 1 <= beam_width <= 8, beam_width <= vocab."""
    # (the head's LDS, 64 KiB: never the limit at d <= 1024; at d = 2048 it leaves beam_width <= 4)
    return (decoder_generate_supported(compute, d, n_heads, d_ff, S, n_layers, vocab, n_steps) and 1 <= beam_width <= min(8, vocab)
            and (4 if beam_width <= 4 else 8) * (d + vocab) * 4 <= 65536)


class BeamTrace:
    """The selection trace of one decoder_beam call: step_tokens / step_parents / step_scores (n_steps, B, W) of every surviving slot
    (int64 / int32 parent slot at the step before / fp32) and step_logits (n_steps, B, W, |V|), the logits row of each PARENT slot."""
    __slots__ = ("step_tokens", "step_parents", "step_scores", "step_logits")

    def __init__(self, step_tokens, step_parents, step_scores, step_logits):
        self.step_tokens, self.step_parents, self.step_scores, self.step_logits = step_tokens, step_parents, step_scores, step_logits


def decoder_beam(meta, start, mem2d, emb, pe, layer_params: Sequence[torch.Tensor], fc_w, fc_b, n_steps: int, beam_width: int,
                 return_trace: bool = False, schedule: "TokenSchedule" = None):
    """Beam search in ONE asynchronous call (egx_decoder_beam; no autograd): start (B,) int64, mem2d (B * S, d) batch-first memory rows, pe
    (>= n_steps, d) positional rows, meta as DecoderFn's (dropout ignored: inference). Returns tokens (B, W, n_steps) int64 (best first),
    scores (B, W) fp32 and, with return_trace, a BeamTrace (else None). The workspace comes from the caching allocator: the call can be
    captured. With a TokenSchedule: egx_decoder_beam_sched, step t's log_softmax and ranking over the words of row t % P, the other logits
    -inf."""
    lib = _lib.load()
    with torch.no_grad():
        W = beam_width
        start, V, cfg, model, ws, keep = _cached_step_setup("decoder_beam", start, 1, "start must be a (B,)", meta, mem2d, emb, pe, layer_params, fc_w,
                                                            fc_b, n_steps, lambda c, B, n, nb: lib.egx_decoder_beam_workspace(c, B, n, W, nb))
        B, dev = start.shape[0], ws.device
        tokens = torch.empty((B, W, n_steps), dtype=torch.int64, device=dev)
        scores = torch.empty((B, W), dtype=torch.float32, device=dev)
        trace = None
        if return_trace:
            trace = BeamTrace(torch.empty((n_steps, B, W), dtype=torch.int64, device=dev), torch.empty((n_steps, B, W), dtype=torch.int32, device=dev),
                              torch.empty((n_steps, B, W), dtype=torch.float32, device=dev),
                              torch.empty((n_steps, B, W, V), dtype=torch.float32, device=dev))
        tr = [ptr(getattr(trace, k)) if trace is not None else None for k in BeamTrace.__slots__]
        args = (C.byref(cfg), ptr(start), *model, B, n_steps, W, ptr(tokens), ptr(scores), *tr, ptr(ws), _stream())
        if schedule is None:
            check(lib.egx_decoder_beam(*args))
        else:
            check_schedule(schedule, V, dev, W)
            check(lib.egx_decoder_beam_sched(*args, *schedule._args()))
    _last_dec_impl[0] = "beam"
    return tokens, scores, trace


def decoder_forced_supported(compute: str, d: int, n_heads: int, d_ff: int, S: int, n_layers: int, vocab: int, n_steps: int,
                             rows_per_clip: int = 1) -> bool:
    """Configurations egx_decoder_forced serves (include/egot2x.h): egx_decoder_generate's limits, 1 <= rows_per_clip <= 8."""
    return decoder_generate_supported(compute, d, n_heads, d_ff, S, n_layers, vocab, n_steps) and 1 <= rows_per_clip <= 8


def decoder_long_supported(d: int, n_heads: int, sy: int, S: int) -> bool:
    """Shapes the composed decoder serves over 9 .. 64 target tokens (decoder.py, egx_long_targets; egx_target_attention_*'s limits): head
    dim d / n_heads <= 128, 1 <= S <= 1024 memory tokens. Post-LN layers are the caller's check."""
    return n_heads >= 1 and d >= 1 and d % n_heads == 0 and d // n_heads <= 128 and 9 <= sy <= 64 and 1 <= S <= 1024


def decoder_forced(meta, tokens, targets, mem2d, emb, pe, layer_params: Sequence[torch.Tensor], fc_w, fc_b, return_logits: bool = True):
    """Teacher-forced decoding in ONE asynchronous call (egx_decoder_forced; no autograd): tokens (B, R, n_steps) int64 input tokens, R
    sequences per clip; targets the same shape or None; mem2d (B * S, d) batch-first memory rows (one memory per CLIP), pe (>= n_steps, d)
    positional rows, meta as DecoderFn's (dropout ignored: inference). Returns (logits (n_steps, B * R, |V|) fp32 or None, logprob
    (B, R, n_steps) fp32 or None): logprob[b, r, t] = log_softmax(logits[t, b * R + r])[targets[b, r, t]], 0.0 where the target is outside
    the vocabulary. The workspace comes from the caching allocator: the call can be captured."""
    lib = _lib.load()
    with torch.no_grad():
        def also():
            if targets is not None and (targets.dtype != torch.int64 or not targets.is_cuda or targets.shape != tokens.shape):
                raise _lib.EgxError(f"decoder_forced: targets must be an int64 tensor on the GPU of the tokens' shape {tuple(tokens.shape)}")
            if targets is None and not return_logits:
                raise _lib.EgxError("decoder_forced: return_logits=False without targets leaves nothing to compute")

        tokens, V, cfg, model, ws, keep = _cached_step_setup(
            "decoder_forced", tokens, 3, "tokens must be a (B, R, n_steps)", meta, mem2d, emb, pe, layer_params, fc_w, fc_b, None,
            lambda c, B, n, nb: lib.egx_decoder_forced_workspace(c, B, tokens.shape[1], n, nb), also)
        targets = targets.contiguous() if targets is not None else None
        (B, R, n_steps), dev = tokens.shape, ws.device
        logits = torch.empty((n_steps, B * R, V), dtype=torch.float32, device=dev) if return_logits else None
        logprob = torch.empty((B, R, n_steps), dtype=torch.float32, device=dev) if targets is not None else None
        check(lib.egx_decoder_forced(C.byref(cfg), ptr(tokens), ptr(targets), *model, B, R, n_steps, ptr(logits), ptr(logprob), ptr(ws),
                                     _stream()))
    _last_dec_impl[0] = "forced"
    return logits, logprob


def weighted_cross_entropy(logits, target, weight=None):
    """F.cross_entropy(logits, target, weight=weight) with mean reduction (HHI/tasks/ttm/video_task_2loader.py:21-22,34).
    Labels outside [0, C) - including F.cross_entropy's default ignore_index = -100 - contribute neither loss, weight nor
    gradient."""
    return WeightedCEFn.apply(logits, target, weight)


_SCRATCH = {}
_SCRATCH_RETIRED = []


def _zeroed_scratch(who: str, device, nbytes: int, key=(), floor: int = 0) -> torch.Tensor:
    """Scratch of a one-launch criterion (`who`: its public name): arrival counters (zero between launches) + partial sums. The rules:
    - one buffer per (operator, device, *key) - NOT per stream: a hipGraph is captured on a stream of its own and must find the buffer
      its eager warm-up created, so two streams must not run one operator concurrently on one device;
    - grown on demand (to at least `floor` bytes), and a new buffer is zero-filled once: every launch leaves its counters zero again;
    - never created inside a capture: the buffer would live in that graph's private pool, so the call raises;
    - an outgrown buffer is retired, never freed: a graph captured at the smaller size still holds its address and keeps replaying into it.
    `key` separates problem sizes whose layouts must not share memory. segmented_cross_entropy passes (Z,): its buffer begins with
    64 * (1 + Z) bytes of counters, and the partial sums behind them must not land where a launch with another Z keeps its counters."""
    key = (who, device.index if device.index is not None else torch.cuda.current_device(), *key)
    t = _SCRATCH.get(key)
    if t is None or t.numel() < nbytes:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{who}: run one eager step at this problem size before capturing it in a graph")
        if t is not None:
            _SCRATCH_RETIRED.append(t)
        t = _SCRATCH[key] = torch.zeros(max(nbytes, floor), dtype=torch.uint8, device=device)
    return t


class LinearCEFn(torch.autograd.Function):
    """(loss, logits, probs, pred, correct) of Linear(K -> C) followed by weighted cross-entropy, ONE launch forward and ONE backward
    (egx_linear_ce_*): the ASD task's lossAV, HHI/tasks/asd/loss.py:11-30. Only `loss` carries gradient."""

    @staticmethod
    def forward(ctx, x, W, b, target, weight):
        lib = _lib.load()
        x, W = _dev_f32(x, "x"), _dev_f32(W, "weight")
        if x.dim() != 2 or W.dim() != 2 or W.shape[1] != x.shape[1]:
            raise ValueError(f"linear_cross_entropy expects x (M, K) and W (C, K), got {tuple(x.shape)} and {tuple(W.shape)}")
        M, K = x.shape
        Cn = W.shape[0]
        if Cn > 8 or K not in (64, 128, 256):
            raise ValueError(f"linear_cross_entropy supports C <= 8 classes and K in (64, 128, 256), got C={Cn}, K={K}")
        if target.dtype != torch.int64 or target.shape != (M,) or target.device != x.device:
            raise ValueError("target must be an int64 tensor of shape (M,) on the input's device")
        b = _dev_f32(b, "bias") if b is not None else None
        w = _dev_f32(weight, "class weight") if weight is not None else None
        if w is not None and w.numel() != Cn:
            raise ValueError("weight must have one entry per class")
        tgt = target.contiguous()
        logits = torch.empty((M, Cn), dtype=torch.float32, device=x.device)
        probs = torch.empty_like(logits)
        need = any(ctx.needs_input_grad[:3])
        dl = torch.empty_like(logits) if need else None
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        correct = torch.empty((), dtype=torch.float32, device=x.device)
        pred = torch.empty((M,), dtype=torch.float32, device=x.device)
        scratch = _zeroed_scratch("linear_cross_entropy", x.device, lib.egx_linear_ce_scratch(M, K, Cn), floor=1 << 16)
        check(lib.egx_linear_ce_fwd(ptr(x), ptr(W), ptr(b) if b is not None else None, ptr(tgt), ptr(w) if w is not None else None,
                                    M, K, Cn, ptr(logits), ptr(probs), ptr(dl) if dl is not None else None, ptr(loss), ptr(correct),
                                    ptr(pred), ptr(scratch), _stream()))
        ctx.has_b = b is not None
        ctx.shape = (M, K, Cn)
        if need:
            ctx.save_for_backward(x, W, dl)
        ctx.mark_non_differentiable(logits, probs, pred, correct)
        ctx.set_materialize_grads(False)    # no zero-filled "gradients" for the four auxiliary outputs (a fill launch each)
        return loss, logits, probs, pred, correct

    @staticmethod
    def backward(ctx, g_loss, _gl, _gp, _gr, _gc):
        if g_loss is None:
            return None, None, None, None, None
        lib = _lib.load()
        x, W, dl = ctx.saved_tensors
        M, K, Cn = ctx.shape
        g = _f32c(g_loss)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dW = torch.empty_like(W)
        db = torch.empty((Cn,), dtype=torch.float32, device=x.device) if ctx.has_b else None
        scratch = _zeroed_scratch("linear_cross_entropy", x.device, lib.egx_linear_ce_scratch(M, K, Cn), floor=1 << 16)
        check(lib.egx_linear_ce_bwd(ptr(x), ptr(W), ptr(dl), ptr(g), M, K, Cn, ptr(dx) if dx is not None else None, ptr(dW),
                                    ptr(db) if db is not None else None, ptr(scratch), _stream()))
        return dx, dW if ctx.needs_input_grad[1] else None, db if ctx.needs_input_grad[2] else None, None, None


def linear_cross_entropy(x, W, b, target, weight=None):
    """(loss, logits, probs, pred, correct): F.cross_entropy(F.linear(x, W, b), target, weight=weight) plus softmax(logits),
    round(softmax)[:, 1] and the number of rows where that equals the label, in one launch (lossAV, HHI/tasks/asd/loss.py:17-30)."""
    return LinearCEFn.apply(x, W, b, target, weight)


# ---- the LTA criterion: per-(future step, head) cross-entropies and top-k counts in one launch (csrc/seg_ce.hip) ----------------
SEG_CE_MAX_HEADS, SEG_CE_MAX_KS, SEG_CE_MAX_CLASSES = 4, 4, 2048


def _seg_windows(preds):
    """The heads as column windows of ONE (B, Z, ld) fp32 stack -> (address of row 0, ld, col0). Zero-copy when the (B, Z, C_h) tensors
    are views of one storage with a common row stride whose windows lie side by side in a row (what `_LTATranslator.decode` returns:
    torch.split of the (B, Z, 593) stack); None otherwise (the caller concatenates)."""
    p0 = preds[0]
    B, Z = p0.shape[0], p0.shape[1]
    ld = p0.stride(1)
    base = p0.untyped_storage().data_ptr()
    if ld < 1 or any(p.untyped_storage().data_ptr() != base or p.stride() != (Z * ld, ld, 1) for p in preds):
        return None
    offs = [p.storage_offset() for p in preds]
    col0 = [o - min(offs) for o in offs]
    spans = sorted((c, c + p.shape[2]) for c, p in zip(col0, preds))
    if spans[-1][1] > ld or any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        return None
    return base + 4 * min(offs), ld, col0


def _head_stack(who: str, preds):
    """The (B, Z, C_h) heads of `who` (segmented_cross_entropy, lta_validate), checked, as the launch's stack ->
    (B, Z, H, dev, widths, addr, ld, col0, stack): in place where _seg_windows finds one, else one torch.cat - `stack` is then that tensor
    (None otherwise), which the caller holds until after the launch."""
    H = len(preds)
    if not 1 <= H <= SEG_CE_MAX_HEADS:
        raise ValueError(f"{who} takes 1 to {SEG_CE_MAX_HEADS} heads, got {H}")
    for h, p in enumerate(preds):
        _dev_f32(p[:0], f"preds[{h}]")                   # device / dtype refusal only: the heads stay the views they are
    p0 = preds[0]
    if any(p.dim() != 3 or p.shape[:2] != p0.shape[:2] or p.device != p0.device for p in preds):
        raise ValueError(f"{who} expects (B, Z, C_h) heads of one batch, got {[tuple(p.shape) for p in preds]}")
    B, Z = p0.shape[0], p0.shape[1]
    widths = [p.shape[2] for p in preds]
    win = _seg_windows(preds)
    if win is not None:
        return (B, Z, H, p0.device, widths, *win, None)
    stack = torch.cat(preds, dim=-1).contiguous()       # one concatenation builds the stack
    col0 = [sum(widths[:h]) for h in range(H)]
    return B, Z, H, p0.device, widths, stack.data_ptr(), stack.shape[2], col0, stack


def _head_labels(labels, B: int, Z: int, H: int, dev) -> torch.Tensor:
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B, Z, H) or labels.device != dev:
        raise ValueError(f"labels must be an int64 tensor of shape (B, Z, H) = {(B, Z, H)} on the predictions' device")
    return labels.contiguous()


def _c_ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def _out_tensor(out, name: str, shape, dtype, dev, wanted: bool = True):
    """A result of a one-launch criterion: the caller's preallocated out[name] (the persistent buffers of the train.py modules), else a
    new tensor; None for a result this call does not produce."""
    if not wanted:
        return None
    return out[name] if name in out else torch.empty(shape, dtype=dtype, device=dev)


def _fresh(*results):
    """New tensor objects over the result memory: a persistent buffer handed in through `out` must not become the owner of this call's
    autograd graph (it would keep the graph - and the logits' gradient accumulator, with the stream it was created on - alive into the
    next call, e.g. from an eager step on the default stream into a capture)."""
    return tuple(None if t is None else t.detach() for t in results)


class SegmentedCEFn(torch.autograd.Function):
    """(loss, loss_terms, n_valid, correct) of egx_segmented_ce; the same launch leaves d loss / d logits of the whole stack behind, and the
    backward hands out its column windows. `out` (optional dict of preallocated `loss`, `loss_terms`, `n_valid`, `correct`): where the results
    go (train.LTACriterion's persistent buffers); only `loss` carries gradient."""

    @staticmethod
    def forward(ctx, labels, ks, out, *preds):
        lib = _lib.load()
        B, Z, H, dev, widths, addr, ld, col0, _stack = _head_stack("segmented_cross_entropy", preds)     # _stack: alive until the launch
        tgt = _head_labels(labels, B, Z, H, dev)
        ks = tuple(int(k) for k in ks)
        if len(ks) > SEG_CE_MAX_KS:
            raise ValueError(f"segmented_cross_entropy takes at most {SEG_CE_MAX_KS} values of k, got {len(ks)}")
        out = out or {}
        loss = _out_tensor(out, "loss", (), torch.float32, dev)
        terms = _out_tensor(out, "loss_terms", (Z, H), torch.float32, dev)
        n_valid = _out_tensor(out, "n_valid", (Z, H), torch.int32, dev)
        correct = _out_tensor(out, "correct", (len(ks), Z, H), torch.int32, dev)
        need = any(ctx.needs_input_grad[3:])
        dl = torch.empty((B, Z, ld), dtype=torch.float32, device=dev) if need else None
        nbytes = lib.egx_segmented_ce_scratch(B, Z, H, len(ks))
        if nbytes == 0:
            check(1)
        scratch = _zeroed_scratch("segmented_cross_entropy", dev, nbytes, key=(Z,))
        check(lib.egx_segmented_ce(addr, ld, ptr(tgt), B, Z, H, _c_ints(col0), _c_ints(widths), _c_ints(ks), len(ks), ptr(loss), ptr(terms),
                                   ptr(n_valid), ptr(correct) if len(ks) else None, ptr(dl), ptr(scratch), _stream()))
        ctx.n_heads = H
        ctx.windows = list(zip(col0, widths)) if need else None
        if need:
            ctx.save_for_backward(dl)
        loss, terms, n_valid, correct = _fresh(loss, terms, n_valid, correct)
        ctx.mark_non_differentiable(terms, n_valid, correct)
        ctx.set_materialize_grads(False)
        return loss, terms, n_valid, correct

    @staticmethod
    def backward(ctx, g_loss, _gt, _gn, _gc):
        if ctx.windows is None or g_loss is None:
            return (None,) * (3 + ctx.n_heads)
        dl = _scaled_by_upstream(ctx.saved_tensors[0], g_loss)
        return (None, None, None) + tuple(dl[..., c0:c0 + w] if ctx.needs_input_grad[3 + h] else None for h, (c0, w) in enumerate(ctx.windows))


def segmented_cross_entropy(preds, labels, ks=(1, 5), out=None):
    """-> (loss, stats): the criterion of the long-term-anticipation task (HOI/tasks/lta/long_term_anticipation.py:182-203) in one launch.

    preds: list of (B, Z, C_h) fp32 tensors, one per head (1 .. 4 heads, C_h <= 2048); labels: int64 (B, Z, H).
    loss = sum over heads h and future steps z of F.cross_entropy(preds[h][:, z], labels[:, z, h]) (mean over the clips with a valid
    label). stats, all device tensors (nothing synchronises): `correct` (len(ks), Z, H) int32 - valid clips whose label is among the top k -,
    `n_valid` (Z, H) int32, `loss_terms` (Z, H) - the terms of the sum. top-k error of a pair = (1 - correct / n_valid) * 100.
    A label outside [0, C_h) (ignore index -100 included) contributes no loss, count or gradient; a (z, h) pair without a valid label adds
    0 (torch: nan); among equal logits the lower class index ranks first (torch.topk: unspecified).
    When the heads are views of one storage with a common row stride - what `forward_features` of the LTA translators returns - the kernel
    reads them in place; otherwise one torch.cat builds the stack. `out`: preallocated result tensors (train.LTACriterion)."""
    loss, terms, n_valid, correct = SegmentedCEFn.apply(labels, tuple(ks), out, *preds)
    return loss, {"correct": correct, "n_valid": n_valid, "loss_terms": terms}


# ---- the PNR keyframe criterion: BCE / masked CE, keyframe distance and accuracy in one launch (csrc/keyframe.hip) -----------------------
KEYFRAME_MAX_T, KEYFRAME_MAX_V = 64, 2048
KEYFRAME_KINDS = {"bce": 0, "cross_entropy": 1, None: 2}


def _kf_rows(t, B: int, dtype, dev, name: str):
    """A per-clip argument as a contiguous (B,) device tensor of `dtype` ((B,), (B, 1) or (1, B) in; a no-op when it already is one)."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    if t.numel() != B:
        raise ValueError(f"keyframe_criterion: {name} has {t.numel()} elements, expected one per clip ({B})")
    return t.reshape(B).to(device=dev, dtype=dtype).contiguous()


class KeyframeCriterionFn(torch.autograd.Function):
    """(loss, loss_rows, pred, label_frame, counts, dist, dist_sum) of egx_keyframe_criterion; the same launch leaves d loss / d logits of the
    whole (B, ld) block behind. `out` (optional dict of preallocated result tensors): where the results go (train.KeyframeCriterion's
    persistent buffers); only `loss` carries gradient."""

    @staticmethod
    def forward(ctx, preds, target, label, state_change, fps, start, end, pnr, kind, cols, out):
        lib = _lib.load()
        _dev_f32(preds[:0], "preds")                        # device / dtype refusal only: the logits stay the view they are
        if kind not in KEYFRAME_KINDS:
            raise ValueError(f"keyframe_criterion: kind={kind!r} (needs 'bce', 'cross_entropy' or None for the metric alone)")
        if preds.dim() == 3 and preds.shape[1] == 1:
            x = preds[:, 0]                                 # the (B, 1, T) tensor forward_features returns
        elif preds.dim() == 2:
            x = preds
        else:
            raise ValueError(f"keyframe_criterion expects (B, T), (B, 1, T) or (B, V) logits, got {tuple(preds.shape)}")
        B, V = x.shape
        if B < 1:
            raise ValueError("keyframe_criterion: empty batch")
        cols = None if cols is None else [int(c) for c in cols]
        T = V if cols is None else len(cols)
        if x.stride(1) != 1 or (B > 1 and x.stride(0) < V):
            x = x.contiguous()
        ld = x.stride(0) if B > 1 else V                    # read in place: the row stride is the launch's ld
        dev = x.device
        tgt = None
        if target is not None:
            if tuple(target.shape) != (B, T):
                raise ValueError(f"keyframe_criterion: target must have shape (B, T) = {(B, T)}, got {tuple(target.shape)}")
            tgt = target.to(device=dev, dtype=torch.float32).contiguous()
        lab = _kf_rows(label, B, torch.int64, dev, "label")
        sc = _kf_rows(state_change, B, torch.int64, dev, "state_change")
        timing = [_kf_rows(fps, B, torch.float64, dev, "fps"), _kf_rows(start, B, torch.int64, dev, "clip_start_frame"),
                  _kf_rows(end, B, torch.int64, dev, "clip_end_frame"), _kf_rows(pnr, B, torch.int64, dev, "pnr_frame")]
        if any(t is None for t in timing) and not all(t is None for t in timing):
            raise ValueError("keyframe_criterion: fps and info (clip_start_frame, clip_end_frame, pnr_frame) go together: all, or none")
        timed = timing[0] is not None
        with_loss = kind is not None
        out = out or {}
        loss = _out_tensor(out, "loss", (), torch.float32, dev, with_loss)
        loss_rows = _out_tensor(out, "loss_rows", (B,), torch.float32, dev, with_loss)
        pred = _out_tensor(out, "pred", (B,), torch.int32, dev)
        label_frame = _out_tensor(out, "label_frame", (B,), torch.int32, dev)
        counts = _out_tensor(out, "counts", (4,), torch.int32, dev)
        dist = _out_tensor(out, "dist", (B,), torch.float64, dev, timed)
        dist_sum = _out_tensor(out, "dist_sum", (), torch.float64, dev, timed)
        need = with_loss and ctx.needs_input_grad[0]
        dl = torch.empty((B, ld), dtype=torch.float32, device=dev) if need else None
        nbytes = lib.egx_keyframe_scratch(B)
        if nbytes == 0:
            check(1)
        # the size does not depend on the shape and every launch leaves the arrival counter zero, so every shape shares the buffer
        scratch = _zeroed_scratch("keyframe_criterion", dev, nbytes)
        ca = (C.c_int * T)(*cols) if cols is not None else None
        check(lib.egx_keyframe_criterion(x.data_ptr(), ld, B, T, ca, V, KEYFRAME_KINDS[kind], ptr(tgt), ptr(lab), ptr(sc), ptr(timing[0]),
                                         ptr(timing[1]), ptr(timing[2]), ptr(timing[3]), ptr(loss), ptr(loss_rows), ptr(dl), ptr(pred),
                                         ptr(label_frame), ptr(counts), ptr(dist), ptr(dist_sum), ptr(scratch), _stream()))
        ctx.grad_shape = (tuple(preds.shape), V) if need else None
        if need:
            ctx.save_for_backward(dl)
        res = _fresh(loss, loss_rows, pred, label_frame, counts, dist, dist_sum)
        ctx.mark_non_differentiable(*[t for t in res[1:] if t is not None])
        ctx.set_materialize_grads(False)
        return res

    @staticmethod
    def backward(ctx, g_loss, *_rest):
        if ctx.grad_shape is None or g_loss is None:
            return (None,) * 11
        dl = _scaled_by_upstream(ctx.saved_tensors[0], g_loss)
        shape, V = ctx.grad_shape
        return (dl[:, :V].reshape(shape),) + (None,) * 10


def keyframe_criterion(preds, target=None, label=None, state_change=None, fps=None, info=None, kind="bce", cols=None, out=None):
    """-> (loss or None, stats): the training step of the PNR keyframe task after the model (HOI/tasks/pnr/video_taskspecific_pnr.py:24-63:
    the BCE - or masked CE - loss, keyframe_distance and keyframe_accuracy of HOI/evaluation/pnr/metrics.py:23-80) in one launch, and with
    `cols` PnrOsccMetric.pnr_distance / oscc_acc (metrics.py:102-134) on decoder logits. Nothing synchronises.

    preds: fp32 (B, T), or the (B, 1, T) tensor `forward_features` returns (read in place: ld = its row stride), or (B, V) decoder logits
    with cols = the T vocabulary columns of the frames (T <= 64, V <= 2048). target: the one-hot (B, T) labels (any dtype; soft values
    allowed); label: the label frame as an int64 index (B), default argmax of target; state_change: (B) or (B, 1), default every clip counts;
    fps (B) and info = {clip_start_frame, clip_end_frame, pnr_frame} go together. kind: "bce" (BCELoss(sigmoid(x)) in logit form, mean over
    B * T), "cross_entropy" (mean over B of the state-change clips' CE) or None (metric only, loss is None).
    stats, all device tensors: `pred` (B) int32, `label_frame` (B) int32, `counts` int32 [n_sc, n_correct, n_outside, B], `loss_rows` (B),
    `dist` (B) fp64 seconds and `dist_sum` fp64 (with fps / info). keyframe_distance = dist_sum / n_sc (0.0 without a state-change clip),
    pseudo_acc = n_correct / n_sc. `out`: preallocated result tensors (train.KeyframeCriterion). For a captured step pass device tensors of
    the final dtypes (target fp32, the others int64 / fps fp64): a conversion is a copy the capture would record."""
    info = info or {}
    start, end, pnr = (info.get(k) for k in ("clip_start_frame", "clip_end_frame", "pnr_frame"))
    loss, loss_rows, pred, label_frame, counts, dist, dist_sum = KeyframeCriterionFn.apply(preds, target, label, state_change, fps, start, end,
                                                                                         pnr, kind, cols, out)
    return loss, {"pred": pred, "label_frame": label_frame, "counts": counts, "loss_rows": loss_rows, "dist": dist, "dist_sum": dist_sum}


# ---- the EgoT2-g multi-task criterion: per-task cross-entropies times their ratios + word-to-label metrics in one launch (csrc/seq_ce.hip) ---
SEQ_CE_MAX_TASKS, SEQ_CE_MAX_CLASSES, SEQ_CE_MAX_SY = 8, 2048, 64
SEQ_CE_STATS = ("loss_terms", "n_valid", "token_correct", "seq_correct", "scored", "invalid", "correct", "correct_restricted")


def sequence_ce_views(flat: torch.Tensor, T: int) -> dict:
    """The 1 + 8 T result words of egx_sequence_ce as named views: `loss` () and `loss_terms` (T,) fp32, the seven counts (T,) int32."""
    v = {"loss": flat[0:1].view(torch.float32).view(()), "loss_terms": flat[1:1 + T].view(torch.float32)}
    for i, name in enumerate(SEQ_CE_STATS[1:], start=1):
        v[name] = flat[1 + i * T:1 + (i + 1) * T]
    return v


def _seq_positions(t, B: int, sy: int, dev, name: str):
    """An int64 (B, sy) argument of sequence_cross_entropy, read in place through its strides (target[:, 1:] is no copy)."""
    if t.dtype != torch.int64 or tuple(t.shape) != (B, sy) or t.device != dev:
        raise ValueError(f"sequence_cross_entropy: {name} must be an int64 tensor of shape (B, sy) = {(B, sy)} on the logits' device")
    return t


class SequenceCEFn(torch.autograd.Function):
    """(loss, flat, *pred) of egx_sequence_ce over the tasks' (B, V, sy) logits; the same launch leaves d loss / d logits of every task behind,
    in the layout of its logits. `out` (optional {"flat": int32 (1 + 8 T,)}): where the results go (train.TranslationCriterion's persistent
    buffer); only `loss` carries gradient."""

    @staticmethod
    def forward(ctx, targets, ratios, word_labels, labels, out, want_pred, *logits):
        lib = _lib.load()
        T = len(logits)
        if not 1 <= T <= SEQ_CE_MAX_TASKS:
            raise ValueError(f"sequence_cross_entropy takes 1 to {SEQ_CE_MAX_TASKS} tasks, got {T}")
        if len(targets) != T or len(ratios) != T or len(word_labels) != T or len(labels) != T:
            raise ValueError(f"sequence_cross_entropy: {T} logits need {T} targets, ratios, word_labels and labels")
        for t, lg in enumerate(logits):
            _dev_f32(lg[:0], f"logits[{t}]")                # device / dtype refusal only: the logits stay the views they are
            if lg.dim() != 3 or lg.numel() == 0:
                raise ValueError(f"sequence_cross_entropy expects non-empty (B, V, sy) logits, got {tuple(lg.shape)} for task {t}")
        dev, V = logits[0].device, logits[0].shape[1]
        if any(lg.shape[1] != V or lg.device != dev for lg in logits):
            raise ValueError(f"sequence_cross_entropy: the tasks share one vocabulary and device, got {[tuple(lg.shape) for lg in logits]}")
        tasks = (_lib.SeqTask * T)()
        keep, dls, preds = [], [], []
        for t, lg in enumerate(logits):
            B, _, sy = lg.shape
            x = lg.permute(0, 2, 1)                         # (B, sy, V): the rows the launch reads
            if x.stride(2) != 1 or (B > 1 and x.stride(0) < V) or (sy > 1 and x.stride(1) < V):
                x = x.contiguous()                          # a class axis that is not unit-stride (or rows that overlap): one copy
            tgt = _seq_positions(targets[t], B, sy, dev, f"targets[{t}]")
            wl, lab = word_labels[t], labels[t]
            if (wl is None) != (lab is None):
                raise ValueError(f"sequence_cross_entropy: task {t} needs word_labels and labels together (the metric inputs), or neither")
            if wl is not None:
                if wl.dtype != torch.int32 or tuple(wl.shape) != (V,) or wl.device != dev:
                    raise ValueError(f"sequence_cross_entropy: word_labels[{t}] must be an int32 tensor of shape (V,) = {(V,)} on the logits' device")
                wl = wl.contiguous()
                if lab.dim() == 1 or (lab.dim() == 2 and lab.shape[1] == 1 and sy > 1):     # (B,) labels: position 0 is scored, the others are not
                    full = torch.full((B, sy), -1, dtype=torch.int64, device=dev)
                    full[:, 0] = lab.reshape(B)
                    lab = full
                lab = _seq_positions(lab, B, sy, dev, f"labels[{t}]")
            need = ctx.needs_input_grad[6 + t]
            dl = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev) if need else None
            pred = None
            if want_pred and wl is not None:
                pred = out["pred"][t] if out and out.get("pred") is not None and out["pred"][t] is not None else \
                    torch.empty((B, sy, 2), dtype=torch.int32, device=dev)
            k = tasks[t]
            k.logits, k.stride_b, k.stride_s, k.B, k.sy = x.data_ptr(), x.stride(0), x.stride(1), B, sy
            k.target, k.target_stride_b, k.target_stride_s = tgt.data_ptr(), tgt.stride(0), tgt.stride(1)
            k.ratio, k.d_logits, k.word_label = float(ratios[t]), ptr(dl), ptr(wl)
            k.labels, k.labels_stride_b, k.labels_stride_s = (lab.data_ptr(), lab.stride(0), lab.stride(1)) if lab is not None else (None, 0, 0)
            k.pred = ptr(pred)
            keep.append((x, tgt, wl, lab))                  # alive until the launch
            dls.append(dl)
            preds.append(pred)
        flat = out["flat"] if out and "flat" in out else torch.empty(1 + 8 * T, dtype=torch.int32, device=dev)
        # one layout for every T and shape, and every launch leaves the arrival counters zero: every call shares the buffer
        scratch = _zeroed_scratch("sequence_cross_entropy", dev, lib.egx_sequence_ce_scratch())
        check(lib.egx_sequence_ce(tasks, T, V, ptr(flat), ptr(scratch), _stream()))
        ctx.n_tasks = T
        ctx.read_ptrs = tuple(k[0].data_ptr() for k in keep)        # the addresses the launch read the logits at (the tests compare them)
        ctx.has_dl = [dl is not None for dl in dls]
        ctx.save_for_backward(*[dl for dl in dls if dl is not None])
        flat = flat.detach()
        loss = flat[0:1].view(torch.float32).view(()).detach()
        res = (loss, flat) + tuple(torch.empty(0, dtype=torch.int32, device=dev) if p is None else p.detach() for p in preds)
        ctx.mark_non_differentiable(*res[1:])
        ctx.set_materialize_grads(False)
        return res

    @staticmethod
    def backward(ctx, g_loss, *_rest):
        if g_loss is None or not any(ctx.has_dl):
            return (None,) * (6 + ctx.n_tasks)
        saved = iter(ctx.saved_tensors)
        grads = []
        for has in ctx.has_dl:                              # (B, sy, V) rows in the logits' own layout -> the (B, V, sy) input
            grads.append(_scaled_by_upstream(next(saved), g_loss).permute(0, 2, 1) if has else None)
        return (None,) * 6 + tuple(grads)


def sequence_cross_entropy(logits, targets, ratios, word_labels=None, labels=None, out=None, want_pred=False):
    """-> (loss, stats): the criterion of an EgoT2-g multi-task step (HHI/tasks/multitask/video_tasktranslation.py:39-66,
    HOI/tasks/multitask/video_task.py:537-577) and the integers behind its validation metrics (:683-736) in one launch; nothing synchronises.

    logits: list of 1 .. 8 fp32 (B_t, V, sy_t) tensors over ONE vocabulary (V <= 2048, sy_t <= 64) - what the EgoT2-g models return, a
    permuted view of the decoder's (sy, B, V) output, which the kernel reads in place (so does it a permuted contiguous (B, sy, V) tensor; a
    class axis that is not unit-stride costs one copy). targets: int64 (B_t, sy_t) each, read through their strides (target[:, 1:] is no
    copy); a label outside [0, V) (ignore index -100 included) contributes no loss, count or gradient. ratios: one float per task.
    loss = sum_t ratios[t] * F.cross_entropy(logits[t], targets[t]); a task without a valid label adds 0 (torch: nan).
    word_labels / labels (per task, both or None): int32 (V,) device tensor - the original label of a vocabulary word or -1
    (train.word_label_map) - and the int64 (B_t, sy_t) original labels, < 0 = not scored ((B_t,): position 0 is scored).
    stats, all device tensors: `loss_terms` (T,) fp32; `n_valid`, `token_correct` (valid positions whose argmax is the target), `seq_correct`
    (rows with a valid position and every valid position right), `scored`, `invalid` (scored positions whose argmax is no mapped word),
    `correct` (its label is the position's), `correct_restricted` (the same for the argmax over the mapped words), each (T,) int32; among
    equal logits the lower word wins. want_pred: `pred`, a list with an int32 (B_t, sy_t, 2) tensor (the label of the free and of the
    restricted argmax) per task with metric inputs, None for the others. `out`: {"flat": int32 (1 + 8 T,)} preallocated results
    (train.TranslationCriterion). The gradient of every logits tensor comes back in that tensor's own layout."""
    logits = list(logits)
    T = len(logits)
    word_labels = list(word_labels) if word_labels is not None else [None] * T
    labels = list(labels) if labels is not None else [None] * T
    res = SequenceCEFn.apply(tuple(targets), tuple(float(r) for r in ratios), tuple(word_labels), tuple(labels), out, bool(want_pred), *logits)
    stats = sequence_ce_views(res[1], T)
    loss = res[0]
    stats.pop("loss")
    stats["flat"] = res[1]
    stats["pred"] = [p if p.numel() else None for p in res[2:]] if want_pred else None
    return loss, stats


# ---- the TTM / LAM validation epoch: merged per-row scores, both classes' average precision, confusion counts (csrc/segment_ap.hip) ----
SEG_AP_TILE, SEG_AP_MAX_ROWS = 4096, 1 << 24
SEG_AP_COUNTS = ("n", "n_pos", "TP", "FN", "FP", "TN", "n_nonfinite")
SEG_AP_VALUES = ("AP0", "AP1", "mAP", "acc")


def segment_ap_views(flat: torch.Tensor) -> dict:
    """The 11 result words of egx_segment_ap (`flat`: int64 (11,)) as named 0-d views: the seven int64 counts, then AP0, AP1, mAP, acc fp64."""
    res = {name: flat[i] for i, name in enumerate(SEG_AP_COUNTS)}
    values = flat[len(SEG_AP_COUNTS):].view(torch.float64)
    res.update({name: values[i] for i, name in enumerate(SEG_AP_VALUES)})
    return res


def _seg_ap_capacity(who: str, capacity: int) -> int:
    capacity = int(capacity)
    if not 1 <= capacity <= SEG_AP_MAX_ROWS:
        raise ValueError(f"{who}: capacity={capacity} (needs 1 <= capacity <= {SEG_AP_MAX_ROWS} rows)")
    return capacity


def segment_ap_state(capacity: int, device) -> torch.Tensor:
    """The zeroed accumulator + work area of `capacity` rows (egx_segment_ap_scratch bytes). Zero it again to empty it."""
    capacity = _seg_ap_capacity("segment_ap_state", capacity)
    nbytes = _lib.load().egx_segment_ap_scratch(capacity)
    if nbytes == 0:
        check(1)
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def segment_scores_update(state: torch.Tensor, capacity: int, logits, labels, slots=None, slot0: int = 0) -> None:
    """Fold a batch of window logits into the per-row sums of `state` (PostProcessor.update / _merge_output, HHI/utils/ttm/utils.py:57-80;
    HHI/utils/lam/utils.py:34-47) in one launch; nothing synchronises.

    logits: fp32 (B, 2) on the GPU, read in place (ld = its row stride); labels: int64 (B,), a row takes its first window's; slots: int64
    (B,) device tensor of rows, non-decreasing within the call (a row may continue from an earlier call; a slot outside [0, capacity) is
    dropped), or None: window i is row slot0 + i."""
    lib = _lib.load()
    _dev_f32(logits[:0], "logits")
    if logits.dim() != 2 or logits.shape[1] != 2:
        raise ValueError(f"segment_scores_update expects (B, 2) logits, got {tuple(logits.shape)}")
    B = logits.shape[0]
    if B < 1:
        raise ValueError("segment_scores_update: empty batch")
    x = logits if logits.stride(1) == 1 and (B == 1 or logits.stride(0) >= 2) else logits.contiguous()
    ld = x.stride(0) if B > 1 else 2
    dev = x.device
    if labels.dtype != torch.int64 or labels.numel() != B or labels.device != dev:
        raise ValueError(f"segment_scores_update: labels must be an int64 tensor of {B} elements on the logits' device")
    lab = labels.reshape(B).contiguous()
    sl = None
    if slots is not None:
        if slots.dtype != torch.int64 or slots.numel() != B or slots.device != dev:
            raise ValueError(f"segment_scores_update: slots must be an int64 tensor of {B} elements on the logits' device")
        sl = slots.reshape(B).contiguous()
    check(lib.egx_segment_scores_update(x.data_ptr(), ld, B, ptr(sl), int(slot0), ptr(lab), int(capacity), ptr(state), _stream()))


def segment_ap(state: torch.Tensor, capacity: int, n: int, out=None) -> dict:
    """-> the metric of rows 0 .. n - 1 of `state` as device tensors (PostProcessor.get_mAP -> run_evaluation, HHI/utils/ttm/metrics.py:
    26-71, 138-199, 232-247); nothing synchronises. `score` (n) fp32 = softmax(mean of the row's window logits)[1]; `order1` / `order0` (n)
    int32: the rows by score descending / ascending, the lower row first among equal scores; the int64 counts `n`, `n_pos`, `TP`, `FN`, `FP`,
    `TN` (at score >= 0.5), `n_nonfinite` and fp64 `AP0`, `AP1`, `mAP`, `acc` as 0-d views of `flat` (int64 (11,)). A class without a
    positive row, or any non-finite score, gives nan. `out`: preallocated `flat`, `score`, `order1`, `order0` (train.SegmentAPValidation)."""
    lib = _lib.load()
    n, capacity = int(n), int(capacity)
    if not state.is_cuda:
        raise _lib.EgxError(f"state is on {state.device}: the metric runs only on the GPU through libegot2x.so (no CPU fallback)")
    dev = state.device
    out = out or {}
    rows = max(n, 1)
    flat = _out_tensor(out, "flat", (len(SEG_AP_COUNTS) + len(SEG_AP_VALUES),), torch.int64, dev)
    score = _out_tensor(out, "score", (rows,), torch.float32, dev)
    order1 = _out_tensor(out, "order1", (rows,), torch.int32, dev)
    order0 = _out_tensor(out, "order0", (rows,), torch.int32, dev)
    check(lib.egx_segment_ap(n, capacity, ptr(state), ptr(score), ptr(order1), ptr(order0), ptr(flat), _stream()))
    return {"flat": flat, "score": score[:n], "order1": order1[:n], "order0": order0[:n], **segment_ap_views(flat)}


# ---- the action-recognition test epoch: multi-view ensemble per video, top-k errors over the videos (csrc/view_ensemble.hip) -----------
VIEW_ENS_METHODS = {"sum": 0, "max": 1}
VIEW_ENS_MAX_BATCH = 1 << 16
VIEW_ENS_COUNTS = ("n", "n_dropped", "n_nonfinite")          # then n_invalid (H,) and correct (n_ks, H)


def view_ensemble_views(flat: torch.Tensor, H: int, n_ks: int) -> dict:
    """The result words of egx_view_ensemble_topk (`flat`: int32 (3 + H + n_ks * H,)) as named views: the 0-d counts `n`, `n_dropped`,
    `n_nonfinite`, then `n_invalid` (H,) and `correct` (n_ks, H)."""
    nc = len(VIEW_ENS_COUNTS)
    res = {name: flat[i] for i, name in enumerate(VIEW_ENS_COUNTS)}
    res["n_invalid"] = flat[nc:nc + H]
    res["correct"] = flat[nc + H:nc + H + n_ks * H].view(n_ks, H)
    return res


def _view_ens_classes(who: str, classes) -> tuple:
    classes = tuple(int(c) for c in classes)
    if not 1 <= len(classes) <= SEG_CE_MAX_HEADS or any(not 1 <= c <= SEG_CE_MAX_CLASSES for c in classes):
        raise ValueError(f"{who}: classes={classes} (needs 1 to {SEG_CE_MAX_HEADS} heads of 1 to {SEG_CE_MAX_CLASSES} classes)")
    return classes


def _view_ens_layout(who: str, capacity: int, classes):
    """-> (bytes, (labels, views, rows) byte offsets) of the state of `capacity` videos (egx_view_ensemble_state)."""
    offs = (C.c_size_t * 3)()
    nbytes = _lib.load().egx_view_ensemble_state(int(capacity), len(classes), _c_ints(classes), offs)
    if nbytes == 0:
        check(1)
    return nbytes, tuple(offs)


def view_ensemble_state(capacity: int, classes, device) -> torch.Tensor:
    """The zeroed accumulator of `capacity` videos with heads of `classes` classes (egx_view_ensemble_state bytes). Zero it again to empty
    it: zero rows are the reference's torch.zeros initialisation, for "sum" and for "max"."""
    classes = _view_ens_classes("view_ensemble_state", classes)
    nbytes, _ = _view_ens_layout("view_ensemble_state", capacity, classes)
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def view_ensemble_rows(state: torch.Tensor, capacity: int, classes) -> dict:
    """The per-video state as views of `state`: `rows` fp32 (capacity, sum classes) - the heads side by side -, `labels` int64
    (capacity, H), `views` int32 (capacity)."""
    classes = _view_ens_classes("view_ensemble_rows", classes)
    capacity, H, ld = int(capacity), len(classes), sum(classes)
    _, (o_lab, o_views, o_rows) = _view_ens_layout("view_ensemble_rows", capacity, classes)
    return {"rows": state[o_rows:o_rows + 4 * capacity * ld].view(torch.float32).view(capacity, ld),
            "labels": state[o_lab:o_lab + 8 * capacity * H].view(torch.int64).view(capacity, H),
            "views": state[o_views:o_views + 4 * capacity].view(torch.int32)}


def _clip_heads(preds):
    """The (B, C_h) heads of a clip batch as the (B, 1, C_h) views _head_stack takes: a head with unit column stride keeps its row
    stride (so heads that are column windows of one stack are read in place), any other becomes contiguous."""
    heads = []
    for p in preds:
        if p.dim() != 2:
            raise ValueError(f"view_ensemble_update expects (B, C_h) heads, got {[tuple(q.shape) for q in preds]}")
        if p.stride(1) != 1 or (p.shape[0] > 1 and p.stride(0) < p.shape[1]):
            p = p.contiguous()
        row = p.stride(0) if p.shape[0] > 1 else p.shape[1]
        heads.append(p.as_strided((p.shape[0], 1, p.shape[1]), (row, row, 1), p.storage_offset()))
    return heads


def view_ensemble_update(state: torch.Tensor, capacity: int, classes, preds, labels, slots=None, slot0: int = 0, method: str = "sum") -> None:
    """Fold a batch of clip predictions into the per-video rows of `state` (the loop of MultiTaskClassificationTask.test_epoch_end,
    HOI/tasks/lta/long_term_anticipation.py:116-140) in one launch; nothing synchronises.

    preds: the list of (B, C_h) fp32 heads `forward_features` of the AR translators returns (or one (B, sum C) tensor for one head); heads
    that are column windows of one stack are read in place, otherwise one torch.cat packs them (_head_stack's policy). labels: int64 (B, H),
    a video keeps its last clip's. slots: int32 / int64 (B,) device tensor of video slots - in any order, with repeats; a slot outside
    [0, capacity) is dropped and counted - or None: clip i is video slot0 + i. method "sum": fp32 adds in arrival order from 0; "max":
    the running maximum from 0 (the reference starts from torch.zeros: an all-negative video ends as zeros)."""
    lib = _lib.load()
    classes = _view_ens_classes("view_ensemble_update", classes)
    if method not in VIEW_ENS_METHODS:
        raise ValueError(f"view_ensemble_update: method={method!r} (needs 'sum' or 'max')")
    preds = [preds] if isinstance(preds, torch.Tensor) else list(preds)
    for h, p in enumerate(preds):
        _dev_f32(p[:0], f"preds[{h}]")
    B, _Z, H, dev, widths, addr, ld, col0, _stack = _head_stack("view_ensemble_update", _clip_heads(preds))   # _stack: alive until the launch
    if tuple(widths) != classes:
        raise ValueError(f"view_ensemble_update: heads of {tuple(widths)} classes, the accumulator holds {classes}")
    if B < 1:
        raise ValueError("view_ensemble_update: empty batch")
    if labels.dtype != torch.int64 or tuple(labels.shape) != (B, H) or labels.device != dev:
        raise ValueError(f"view_ensemble_update: labels must be an int64 tensor of shape (B, H) = {(B, H)} on the predictions' device")
    lab = labels.contiguous()
    sl, slot_bytes = None, 0
    if slots is not None:
        if slots.dtype not in (torch.int32, torch.int64) or slots.numel() != B or slots.device != dev:
            raise ValueError(f"view_ensemble_update: slots must be an int32 or int64 tensor of {B} elements on the predictions' device")
        sl = slots.reshape(B).contiguous()
        slot_bytes = sl.element_size()
    check(lib.egx_view_ensemble_update(addr, ld, B, H, _c_ints(col0), _c_ints(classes), ptr(lab), ptr(sl), slot_bytes, int(slot0),
                                       VIEW_ENS_METHODS[method], int(capacity), ptr(state), _stream()))


def view_ensemble_topk(state: torch.Tensor, capacity: int, classes, n: int, ks=(1, 5), out=None) -> dict:
    """-> the top-k counts of videos 0 .. n - 1 of `state` as device tensors (the four topk_errors calls of test_epoch_end, :142-158;
    HOI/evaluation/lta/lta_metrics.py:38-84); nothing synchronises. `rank` (n, H) int32: the rank of the video's label in its ensemble row,
    the lower class first among equal values, a NaN as the greatest value, -1 for a label outside [0, C_h); `pred` (n, H) int32: the
    class of rank 0; the int32 counts `n`, `n_dropped`, `n_nonfinite`, `n_invalid` (H,), `correct` (len(ks), H) as views of `flat`.
    top-k error = (1 - correct / n) * 100. `out`: preallocated `flat`, `rank`, `pred` (train.ViewEnsembleTest)."""
    lib = _lib.load()
    classes = _view_ens_classes("view_ensemble_topk", classes)
    ks = tuple(int(k) for k in ks)
    n, capacity, H = int(n), int(capacity), len(classes)
    if not state.is_cuda:
        raise _lib.EgxError(f"state is on {state.device}: the metric runs only on the GPU through libegot2x.so (no CPU fallback)")
    if not 1 <= len(ks) <= SEG_CE_MAX_KS:
        raise ValueError(f"view_ensemble_topk takes 1 to {SEG_CE_MAX_KS} values of k, got {len(ks)}")
    dev = state.device
    out = out or {}
    rows = max(n, 1)
    flat = _out_tensor(out, "flat", (len(VIEW_ENS_COUNTS) + H + len(ks) * H,), torch.int32, dev)
    rank = _out_tensor(out, "rank", (rows, H), torch.int32, dev)
    pred = _out_tensor(out, "pred", (rows, H), torch.int32, dev)
    check(lib.egx_view_ensemble_topk(n, capacity, H, _c_ints(classes), _c_ints(ks), len(ks), ptr(state), ptr(rank), ptr(pred), ptr(flat),
                                     _stream()))
    return {"flat": flat, "rank": rank[:n], "pred": pred[:n], **view_ensemble_views(flat, H, len(ks))}


# ---- the LTA validation step: K sampled futures per clip and head + prefix edit distances in one launch (csrc/lta_val.hip) -----------
LTA_VAL_MAX_K, LTA_VAL_MAX_Z = 8, 64
_LTA_VAL_CALLS = [0]


def _lta_val_host_seed() -> int:
    """A fresh host seed per call, counter-based like the translators' dropout seed (no device sync); torch.manual_seed makes it repeatable."""
    _LTA_VAL_CALLS[0] += 1
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + _LTA_VAL_CALLS[0] * 0xD1B54A32D192ED03 + 0x17A) & (2**63 - 1)


def lta_validate(preds, labels=None, k: int = 1, seed=None, seed_ptr=None, tokens=None, out=None):
    """-> (tokens, stats): `generate(..., k)` of the LTA models and the integers behind AUED (HOI/tasks/lta/long_term_anticipation.py:222-248,
    HOI/evaluation/lta/lta_metrics.py:86-114) in one launch (egx_lta_validate), nothing synchronises.

    preds: list of (B, Z, C_h) fp32 heads (1 .. 4, C_h <= 2048, Z <= 64), read in place when they are views of one stack (`decode()`),
    one torch.cat otherwise; labels: int64 (B, Z, H) or None (no metric); k: 1 .. 8 sequences per clip.
    tokens: list of H (B, K, Z) int64 tensors. k = 1: the row argmax (lowest index among equals); k > 1: k independent draws per row from
    the softmax of the head, by inverse cdf on words of the library's counter generator keyed by `seed` (an int; None: a fresh one per
    call) or, with `seed_ptr` (a one-element int64 device tensor or its address), by the word that holds when the launch runs. A row with a
    NaN or +inf, or without a finite logit, yields -1.
    stats (labels given): `min_dist` int32 (B, Z, H) - min over k of the Levenshtein distance of the first z + 1 tokens to the first z + 1
    labels - and `dist_sum` int64 (Z, H), its sum over the clips: ED_z = dist_sum[z, h] / (B (z + 1)).
    tokens=[(B, K, Z) int64, ...] (or one (H, B, K, Z) tensor): the metric-only entry - no sampling, `preds` may be None, the metric of these
    tokens against `labels`. out: preallocated `preds` (H, B, K, Z) int64, `min_dist`, `dist_sum` (train.LTAValidation's buffers)."""
    lib = _lib.load()
    k = int(k)
    out = out or {}
    with torch.no_grad():
        tok_in = None
        if tokens is not None:
            tok_in = tokens if isinstance(tokens, torch.Tensor) else torch.stack(list(tokens), dim=0)
            if tok_in.dim() != 4 or tok_in.dtype != torch.int64 or not tok_in.is_cuda:
                raise ValueError("lta_validate: tokens must be int64 (B, K, Z) tensors, one per head, on the GPU")
            tok_in = tok_in.contiguous()
            H, B, k, Z = tok_in.shape
            dev = tok_in.device
            if labels is None:
                raise ValueError("lta_validate: tokens= is the metric-only entry and needs labels")
            addr, ld, col0, widths = None, 0, [], []
        else:
            B, Z, H, dev, widths, addr, ld, col0, _stack = _head_stack("lta_validate", list(preds))      # _stack: alive until the launch
        if labels is not None:
            labels = _head_labels(labels, B, Z, H, dev)
        if isinstance(seed_ptr, torch.Tensor):
            if seed_ptr.dtype != torch.int64 or seed_ptr.numel() != 1 or seed_ptr.device != dev:
                raise ValueError("lta_validate: seed_ptr must be a one-element int64 tensor on the predictions' device")
            seed_ptr = seed_ptr.data_ptr()
        if seed is None:
            seed = _lta_val_host_seed() if (k > 1 and not seed_ptr and tok_in is None) else 0
        toks = _out_tensor(out, "preds", (H, B, k, Z), torch.int64, dev)
        if tuple(toks.shape) != (H, B, k, Z) or toks.dtype != torch.int64 or not toks.is_contiguous():
            raise ValueError(f"lta_validate: out['preds'] must be a contiguous int64 tensor of shape (H, B, K, Z) = {(H, B, k, Z)}")
        md = _out_tensor(out, "min_dist", (B, Z, H), torch.int32, dev, labels is not None)
        ds = _out_tensor(out, "dist_sum", (Z, H), torch.int64, dev, labels is not None)
        check(lib.egx_lta_validate(addr, ld, ptr(labels), B, Z, H, _c_ints(col0), _c_ints(widths), k, _seed64(seed), seed_ptr or None,
                                   ptr(tok_in), ptr(toks), ptr(md), ptr(ds), _stream()))
    return [toks[h] for h in range(H)], {"min_dist": md, "dist_sum": ds}


# ---- EgoT2-g sequence decoder pieces (kernels in csrc/decoder.hip) ------------------------------
class LayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x + res) * w + b over the last dimension of 2-D inputs (post-LN residual blocks)."""

    @staticmethod
    def forward(ctx, x, res, w, b, eps: float):
        lib = _lib.load()
        x = _dev_f32(x, "x")
        res = _dev_f32(res, "res") if res is not None else None
        w, b = _dev_f32(w, "ln weight"), _dev_f32(b, "ln bias")
        rows, d = x.shape
        pre = torch.empty_like(x)
        stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
        y = torch.empty_like(x)
        check(lib.egx_layernorm_fwd(ptr(x), ptr(res) if res is not None else None, ptr(w), ptr(b), float(eps), ptr(pre),
                                    ptr(stats), ptr(y), rows, d, _stream()))
        ctx.has_res = res is not None
        ctx.save_for_backward(pre, stats, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        pre, stats, w = ctx.saved_tensors
        dy = _f32c(dy)
        rows, d = pre.shape
        need = ctx.needs_input_grad
        dx = torch.empty_like(pre)
        dw = torch.zeros(d, dtype=torch.float32, device=dy.device) if need[2] else None
        db = torch.zeros(d, dtype=torch.float32, device=dy.device) if need[3] else None
        check(lib.egx_layernorm_bwd(ptr(dy), ptr(pre), ptr(stats), ptr(w), ptr(dx), ptr(dw) if dw is not None else None,
                                    ptr(db) if db is not None else None, rows, d, _stream()))
        return (dx if need[0] else None), (dx if (ctx.has_res and need[1]) else None), dw, db, None


def layer_norm_residual(x, res, w, b, eps: float = 1e-5):
    return LayerNormFn.apply(x, res, w, b, eps)


class DropoutFn(torch.autograd.Function):
    """Inverted dropout with the library's counter-based mask (seed, site, row, column); the backward regenerates it."""

    @staticmethod
    def forward(ctx, x, p: float, seed: int, site: int):
        lib = _lib.load()
        y = _dev_f32(x, "x").clone()
        rows = y.numel() // y.shape[-1]
        check(lib.egx_dropout(ptr(y), rows, y.shape[-1], float(p), _seed64(seed), site, _stream()))
        ctx.cfg = (float(p), seed, site)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        p, seed, site = ctx.cfg
        g = _f32c(dy).clone()
        rows = g.numel() // g.shape[-1]
        check(lib.egx_dropout(ptr(g), rows, g.shape[-1], p, _seed64(seed), site, _stream()))
        return g, None, None, None


def dropout(x, p: float, training: bool, seed: int, site: int):
    return DropoutFn.apply(x, p, seed, site) if (training and p > 0.0) else x


class EmbedPosFn(torch.autograd.Function):
    """(B, sy) int64 tokens -> (B * sy, d): embedding[token] * scale + pe[t] (+ dropout)."""

    @staticmethod
    def forward(ctx, tokens, emb, pe, scale: float, p: float, seed: int):
        lib = _lib.load()
        emb = _dev_f32(emb, "embedding")
        pe2 = _dev_f32(pe, "pe")
        if tokens.dtype != torch.int64 or tokens.dim() != 2 or tokens.device != emb.device:
            raise ValueError("tokens must be a (B, sy) int64 tensor on the embedding's device")
        tok = tokens.contiguous()
        B, sy = tok.shape
        V, d = emb.shape
        if sy > pe2.shape[0]:
            raise ValueError("target longer than the positional table")
        out = torch.empty((B * sy, d), dtype=torch.float32, device=emb.device)
        check(lib.egx_embed_pos_fwd(ptr(tok), ptr(emb), ptr(pe2), pe2.stride(0), float(scale), ptr(out), B, sy, d, V, float(p),
                                    _seed64(seed), _stream()))
        ctx.cfg = (float(scale), float(p), seed, V)
        ctx.save_for_backward(tok)
        return out

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        (tok,) = ctx.saved_tensors
        scale, p, seed, V = ctx.cfg
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        dy = _f32c(dy)
        B, sy = tok.shape
        d = dy.shape[-1]
        d_emb = torch.zeros((V, d), dtype=torch.float32, device=dy.device)
        check(lib.egx_embed_pos_bwd(ptr(tok), ptr(dy), ptr(d_emb), scale, B, sy, d, V, p, _seed64(seed), _stream()))
        return None, d_emb, None, None, None, None


def _attn_entry(entry: str, direction: str):
    """egx_small_attention_* (at most 8 query rows, mask row stride 8) or egx_target_attention_* (at most 64, stride 64): same arguments."""
    return getattr(_lib.load(), f"{entry}_{direction}")


def _self_attn_fwd(ctx, entry, qkv, B: int, sy: int, H: int, causal: bool, p: float, seed: int, site: int):
    fn = _attn_entry(entry, "fwd")
    qkv = _dev_f32(qkv, "qkv")
    d = qkv.shape[1] // 3
    out = torch.empty((B * sy, d), dtype=torch.float32, device=qkv.device)
    e = qkv.element_size()
    base = qkv.data_ptr()
    check(fn(base, 3 * d, base + d * e, 3 * d, base + 2 * d * e, 3 * d, ptr(out), d, B, sy, sy, H,
             d // H, int(causal), float(p), _seed64(seed), site, _stream()))
    ctx.cfg = (B, sy, H, int(causal), float(p), seed, site)
    ctx.save_for_backward(qkv)
    return out


def _self_attn_bwd(ctx, entry, d_out):
    fn = _attn_entry(entry, "bwd")
    (qkv,) = ctx.saved_tensors
    B, sy, H, causal, p, seed, site = ctx.cfg
    d = qkv.shape[1] // 3
    d_out = _f32c(d_out)
    dqkv = torch.empty_like(qkv)
    e = qkv.element_size()
    base, gb = qkv.data_ptr(), dqkv.data_ptr()
    check(fn(base, 3 * d, base + d * e, 3 * d, base + 2 * d * e, 3 * d, ptr(d_out), d,
             gb, gb + d * e, gb + 2 * d * e, B, sy, sy, H, d // H, causal, p, _seed64(seed), site, _stream()))
    return dqkv, None, None, None, None, None, None, None


def _cross_attn_fwd(ctx, entry, q, kv, B: int, sy: int, S: int, H: int, p: float, seed: int, site: int):
    fn = _attn_entry(entry, "fwd")
    q, kv = _dev_f32(q, "q"), _dev_f32(kv, "kv")
    d = q.shape[1]
    out = torch.empty((B * sy, d), dtype=torch.float32, device=q.device)
    e = kv.element_size()
    kb = kv.data_ptr()
    check(fn(ptr(q), d, kb, 2 * d, kb + d * e, 2 * d, ptr(out), d, B, sy, S, H, d // H, 0, float(p),
             _seed64(seed), site, _stream()))
    ctx.cfg = (B, sy, S, H, float(p), seed, site)
    ctx.save_for_backward(q, kv)
    return out


def _cross_attn_bwd(ctx, entry, d_out):
    fn = _attn_entry(entry, "bwd")
    q, kv = ctx.saved_tensors
    B, sy, S, H, p, seed, site = ctx.cfg
    d = q.shape[1]
    d_out = _f32c(d_out)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    e = kv.element_size()
    kb, gb = kv.data_ptr(), dkv.data_ptr()
    check(fn(ptr(q), d, kb, 2 * d, kb + d * e, 2 * d, ptr(d_out), d, ptr(dq), gb, gb + d * e,
             B, sy, S, H, d // H, 0, p, _seed64(seed), site, _stream()))
    return dq, dkv, None, None, None, None, None, None, None


class SelfAttnSmallFn(torch.autograd.Function):
    """Causal self-attention over a few target tokens from packed (B * sy, 3d) qkv rows -> (B * sy, d)."""

    @staticmethod
    def forward(ctx, qkv, B: int, sy: int, H: int, causal: bool, p: float, seed: int, site: int):
        return _self_attn_fwd(ctx, "egx_small_attention", qkv, B, sy, H, causal, p, seed, site)

    @staticmethod
    def backward(ctx, d_out):
        return _self_attn_bwd(ctx, "egx_small_attention", d_out)


class CrossAttnSmallFn(torch.autograd.Function):
    """Attention of the target's queries (B * sy, d) onto the memory's packed (B * S, 2d) key/value rows -> (B * sy, d)."""

    @staticmethod
    def forward(ctx, q, kv, B: int, sy: int, S: int, H: int, p: float, seed: int, site: int):
        return _cross_attn_fwd(ctx, "egx_small_attention", q, kv, B, sy, S, H, p, seed, site)

    @staticmethod
    def backward(ctx, d_out):
        return _cross_attn_bwd(ctx, "egx_small_attention", d_out)


class SelfAttnTargetFn(torch.autograd.Function):
    """SelfAttnSmallFn for up to 64 target tokens (egx_target_attention_*: dropout rows (b * H + h) * 64 + i)."""

    @staticmethod
    def forward(ctx, qkv, B: int, sy: int, H: int, causal: bool, p: float, seed: int, site: int):
        return _self_attn_fwd(ctx, "egx_target_attention", qkv, B, sy, H, causal, p, seed, site)

    @staticmethod
    def backward(ctx, d_out):
        return _self_attn_bwd(ctx, "egx_target_attention", d_out)


class CrossAttnTargetFn(torch.autograd.Function):
    """CrossAttnSmallFn for up to 64 target tokens (egx_target_attention_*)."""

    @staticmethod
    def forward(ctx, q, kv, B: int, sy: int, S: int, H: int, p: float, seed: int, site: int):
        return _cross_attn_fwd(ctx, "egx_target_attention", q, kv, B, sy, S, H, p, seed, site)

    @staticmethod
    def backward(ctx, d_out):
        return _cross_attn_bwd(ctx, "egx_target_attention", d_out)


# ---- the encoder's self-attention weights as an output (ABI v27: egx_self_attention_weights, egx_attention_rollout, egx_encoder_self_weights) ----
SELF_WEIGHTS_HEAD_DIMS = (16, 32, 64, 96, 128)
SELF_WEIGHTS_MAX_TOKENS = 512
SELF_WEIGHTS_MAX_SEGMENTS = 16


def check_self_weights(head_dim: int, S: int, K: int = 1) -> None:
    """The limits of the self-attention weights as a ValueError that names them (host work, before any device call)."""
    if head_dim not in SELF_WEIGHTS_HEAD_DIMS or not 1 <= S <= SELF_WEIGHTS_MAX_TOKENS or not 1 <= K <= SELF_WEIGHTS_MAX_SEGMENTS:
        raise ValueError(f"self-attention weights are served for head dims {SELF_WEIGHTS_HEAD_DIMS}, 1..{SELF_WEIGHTS_MAX_TOKENS} tokens per clip "
                         f"and 1..{SELF_WEIGHTS_MAX_SEGMENTS} segments: got head dim {head_dim}, {S} tokens, {K} segments")


def _segment_table(segments, B: int, device, who: str) -> torch.Tensor:
    """segments: K lengths shared by every clip, or (B, K) lengths per clip -> (B, K) int32 on the device"""
    t = segments.detach() if isinstance(segments, torch.Tensor) else torch.as_tensor(segments)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool or t.dim() not in (1, 2) or t.shape[-1] < 1:
        raise ValueError(f"{who}: segments must be K integer lengths or a (B, K) integer table")
    if t.dim() == 1:
        t = t[None].expand(B, t.shape[0])
    if t.shape[0] != B or t.shape[1] > SELF_WEIGHTS_MAX_SEGMENTS:
        raise ValueError(f"{who}: segments has shape {tuple(t.shape)}: expected (K,) or ({B}, K) with K <= {SELF_WEIGHTS_MAX_SEGMENTS}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def self_attention_weights(q: torch.Tensor, k: torch.Tensor, n_heads: int, S: int, rowtab: Optional[torch.Tensor] = None, segments=None,
                           B: Optional[int] = None, weights: bool = True):
    """The head-averaged self-attention weights w[b, i, j] = (1 / H) sum_h softmax_j(q[b, i, h] . k[b, j, h] / sqrt(dh)), i, j < S_b, that
    nn.MultiheadAttention returns with need_weights=True, and their per-segment sums seg[b, i, t] = sum_{j in segment t} w[b, i, j]
    (egx_self_attention_weights; no autograd). q and k (rows, H * dh), both fp32 or both bf16, head h at columns h * dh; 2-D views with unit
    column stride and a row stride that is a multiple of 8 elements are read in place (the q / k columns of a packed Q | K | V matrix).
    Clip b's tokens are rows b * S .. of q and k, or, with rowtab ((B, 2) int32 on the device: first row, S_b <= S), rows first .. first +
    S_b: ragged clips, gaps between clips, empty slots (S_b = 0: zeros). segments: K lengths, or a (B, K) table of per-clip lengths.
    dh in (16, 32, 64, 96, 128), S <= 512. Returns w (B, S, S) fp32, or (w, seg (B, S, K)) with segments; weights=False: seg alone (w is
    then never written to memory). Entries beyond a clip's S_b tokens are exact zeros."""
    lib = _lib.load()
    who = "self_attention_weights"
    for name, t in (("q", q), ("k", k)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"{who}: {name} must be a 2-D fp32 or bf16 tensor on the GPU")
    if q.dtype != k.dtype or q.shape[1] != k.shape[1] or n_heads < 1 or q.shape[1] % n_heads:
        raise ValueError(f"{who}: q {tuple(q.shape)} {q.dtype} and k {tuple(k.shape)} {k.dtype} do not fit {n_heads} heads")
    if segments is None and not weights:
        raise ValueError(f"{who}: weights=False needs segments")
    if rowtab is None:
        if S < 1 or q.shape[0] % S or k.shape[0] != q.shape[0] or (B is not None and B * S != q.shape[0]):
            raise ValueError(f"{who}: q and k have {q.shape[0]} and {k.shape[0]} rows, expected B * S with S = {S} in both")
        B = q.shape[0] // S
    else:
        if not (isinstance(rowtab, torch.Tensor) and rowtab.is_cuda and rowtab.dtype == torch.int32 and rowtab.dim() == 2 and rowtab.shape[1] == 2):
            raise ValueError(f"{who}: rowtab must be a (B, 2) int32 tensor on the GPU (first row, tokens)")
        B = rowtab.shape[0]
        rowtab = rowtab.contiguous()
    segtab = _segment_table(segments, B, q.device, who) if segments is not None else None
    K = segtab.shape[1] if segtab is not None else 0
    check_self_weights(q.shape[1] // n_heads, S, max(K, 1))
    q, k = [t if t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 else t.contiguous() for t in (q.detach(), k.detach())]
    w = torch.empty((B, S, S), dtype=torch.float32, device=q.device) if weights else None
    seg = torch.empty((B, S, K), dtype=torch.float32, device=q.device) if segtab is not None else None
    check(lib.egx_self_attention_weights(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), int(q.dtype == torch.bfloat16), ptr(rowtab),
                                         ptr(segtab), K, B, n_heads, q.shape[1] // n_heads, S, ptr(w), S, ptr(seg), _stream()))
    return w if seg is None else (w, seg) if weights else seg


def attention_rollout(w: torch.Tensor, segments=None, lengths: Optional[torch.Tensor] = None):
    """Attention rollout (Abnar & Zuidema 2020) over the layers of w (L, B, S, S) fp32 on the GPU: R_l = ((w_l + I) / 2) R_{l-1}, R_0 = I, per
    clip, in fp32 with a fixed summation order (egx_attention_rollout; no autograd); L = 1 gives exactly (w_1 + I) / 2. lengths: (B,) int32 on
    the device, clip b's tokens (zeros beyond them). Returns R (B, S, S), or (R, R_by_segment (B, S, K)) with segments (K lengths or a (B, K)
    table)."""
    lib = _lib.load()
    who = "attention_rollout"
    if not isinstance(w, torch.Tensor) or w.dim() != 4 or not w.is_cuda or w.dtype != torch.float32 or w.shape[2] != w.shape[3] or w.shape[0] < 1:
        raise ValueError(f"{who}: w must be an (L, B, S, S) fp32 tensor on the GPU")
    L, B, S, _ = w.shape
    if not 1 <= S <= SELF_WEIGHTS_MAX_TOKENS:
        raise ValueError(f"{who}: S = {S} tokens (1..{SELF_WEIGHTS_MAX_TOKENS})")
    if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda and lengths.dtype == torch.int32 and tuple(lengths.shape) == (B,)):
        raise ValueError(f"{who}: lengths must be a ({B},) int32 tensor on the GPU")
    segtab = _segment_table(segments, B, w.device, who) if segments is not None else None
    K = segtab.shape[1] if segtab is not None else 0
    w = w.detach().contiguous()
    scratch = _workspace("rollout", w.device, lib.egx_attention_rollout_scratch(L, B, S))
    out = torch.empty((B, S, S), dtype=torch.float32, device=w.device)
    seg = torch.empty((B, S, K), dtype=torch.float32, device=w.device) if segtab is not None else None
    check(lib.egx_attention_rollout(w.data_ptr(), L, B, S, ptr(lengths.contiguous()) if lengths is not None else None, ptr(segtab), K, ptr(scratch),
                                    ptr(out), ptr(seg), _stream()))
    return out if seg is None else (out, seg)


@dataclass
class AttentionRecord:
    """What one encoder call left in an AttentionRecorder (None: not asked for). weights (L', B, S, S) and by_segment (L', B, S, K) of the
    selected layers; rollout (B, S, S) and rollout_by_segment (B, S, K) over ALL layers; segments: the (B, K) int32 host table of per-clip
    segment lengths that was used; layers: the selected layers; impl: last_encoder_impl() of the call. A ragged batch: S = max_b S_b, zeros
    beyond each clip."""
    weights: Optional[torch.Tensor] = None
    by_segment: Optional[torch.Tensor] = None
    rollout: Optional[torch.Tensor] = None
    rollout_by_segment: Optional[torch.Tensor] = None
    segments: Optional[torch.Tensor] = None
    layers: tuple = ()
    impl: str = ""


class AttentionRecorder:
    """Context manager: while active, every encoder forward of this process (EncoderFn, encoder_ragged, RaggedEncoderFn) is followed by
    egx_encoder_self_weights on its own `saved`, and by the rollout if asked for; one AttentionRecord per call in `records`. The forwards
    themselves issue the launches they issue without it. Inference only; not for capture in a hipGraph across calls of different shapes."""

    def __init__(self, weights: bool = True, by_segment: bool = True, rollout: bool = False, layers=None, max_bytes: int = 1 << 30):
        if not (weights or by_segment or rollout):
            raise ValueError("record_attention: nothing to record (weights, by_segment and rollout are all off)")
        if layers is not None:
            layers = tuple(int(l) for l in layers)
            if not layers or len(set(layers)) != len(layers) or list(layers) != sorted(layers) or layers[0] < 0:
                raise ValueError(f"record_attention: layers must be distinct ascending layer indices, got {layers}")
        self.weights, self.by_segment, self.rollout, self.layers, self.max_bytes = bool(weights), bool(by_segment), bool(rollout), layers, int(max_bytes)
        self.records: List[AttentionRecord] = []
        self._prev, self.last_call = None, None

    def __enter__(self):
        global _attention_sink
        self._prev, _attention_sink = _attention_sink, self
        return self

    def __exit__(self, *exc):
        global _attention_sink
        _attention_sink = self._prev
        return False

    def plan(self, B: int, S: int, K: int, L: int, d_model: int, n_heads: int):
        """Host checks of one call (ValueError before any device work): the limits, the layer selection and the byte budget. Returns
        (selected layers, layers whose weights are computed, bytes)."""
        if L < 1:
            raise ValueError("record_attention: the encoder has no layers (its forward keeps no Q | K | V)")
        if n_heads < 1 or d_model % n_heads:
            raise ValueError(f"record_attention: d_model = {d_model} is not divisible by {n_heads} heads")
        check_self_weights(d_model // n_heads, S, K)
        sel = self.layers if self.layers is not None else tuple(range(L))
        if sel[-1] >= L:
            raise ValueError(f"record_attention: layers = {sel} but the encoder has {L} layers")
        run = tuple(range(L)) if self.rollout else sel          # (the rollout multiplies every layer)
        plane = B * S * S * 4
        out_bytes = (len(sel) * plane if self.weights else 0) + (len(sel) * B * S * K * 4 if self.by_segment else 0)
        tmp_bytes = 0
        if self.rollout:
            out_bytes += plane + (B * S * K * 4 if self.by_segment else 0)
            tmp_bytes += min(L - 1, 2) * plane + (L * plane if not (self.weights and sel == run) else 0)
        if out_bytes + tmp_bytes > self.max_bytes:
            raise ValueError(f"record_attention: B = {B}, S = {S}, K = {K}, {len(sel)} of {L} layers need {out_bytes} bytes of outputs and "
                             f"{tmp_bytes} bytes of scratch, above max_bytes = {self.max_bytes}; select fewer layers (layers=), drop the "
                             f"(L', B, S, S) weights (weights=False) or raise max_bytes")
        return sel, run, out_bytes + tmp_bytes

    def __call__(self, lib, cfg, segs, B: int, lengths, spec: EncoderSpec, saved: torch.Tensor, device):
        if spec.training:
            raise ValueError("record_attention is inference-only: the encoder call ran in training mode (the reference's train-mode weights are "
                             "post-dropout and are not modelled)")
        K, L = len(spec.segments), spec.n_layers
        if lengths is None:
            S = sum(ss.T for ss in spec.segments)
            table = torch.tensor([[ss.T for ss in spec.segments]] * B, dtype=torch.int32)
        else:
            S = int(lengths.sum(1).max())
            table = lengths.clone()
        sel, run, _ = self.plan(B, S, K, L, spec.d_model, spec.n_heads)
        cfg2 = Config.from_buffer_copy(cfg)         # the call's own configuration; eval mode: its dropout probabilities were not used
        cfg2.p_drop = cfg2.p_pos = cfg2.p_feat = 0.0
        cfg2.ce = cfg2.token_ce = None
        mask = sum(1 << l for l in run)
        need_w = self.weights or self.rollout
        w = torch.empty((len(run), B, S, S), dtype=torch.float32, device=device) if need_w else None
        seg = torch.empty((len(run), B, S, K), dtype=torch.float32, device=device) if self.by_segment else None
        try:
            check(lib.egx_encoder_self_weights(C.byref(cfg2), segs, B, lengths.data_ptr() if lengths is not None else None,
                                               int(spec.head_n_out or spec.token_ce or 0), ptr(saved), mask, ptr(w), ptr(seg), _stream()))
        except _lib.EgxError as e:
            raise ValueError(str(e)) from None
        # (test infrastructure: what the stage hooks need to read this very call's Q | K | V back, tests/test_gpu_enc_attn.py)
        self.last_call = dict(cfg=cfg2, segs=segs, B=B, lengths=lengths, head_n_out=int(spec.head_n_out or spec.token_ce or 0), saved=saved)
        rec = AttentionRecord(segments=table, layers=sel, impl=last_encoder_impl())
        pick = None if sel == run else torch.tensor([run.index(l) for l in sel], dtype=torch.int64, device=device)
        if self.rollout:
            lens = (lengths.sum(1).to(torch.int32).to(device) if lengths is not None else None)
            segtab = table.to(device) if self.by_segment else None
            r = attention_rollout(w, segments=segtab, lengths=lens)
            rec.rollout, rec.rollout_by_segment = (r if self.by_segment else (r, None))
        if self.weights:
            rec.weights = w if pick is None else w.index_select(0, pick)
        if self.by_segment:
            rec.by_segment = seg if pick is None else seg.index_select(0, pick)
        self.records.append(rec)


def _attention_unserved(what: str) -> None:
    """Called where an encoder call takes a path whose attention weights are not served: a ValueError while a recorder is active."""
    if _attention_sink is not None:
        raise ValueError(f"record_attention: {what} is not served (egx_encoder_self_weights)")


def encoder_attention(spec: EncoderSpec, feats: Sequence[torch.Tensor], task_embed, pos_table, ln_w, ln_b, proj: Sequence[torch.Tensor],
                      layer_params: Sequence[torch.Tensor], head_params: Sequence[torch.Tensor] = (), lengths: Optional[torch.Tensor] = None,
                      weights: bool = True, by_segment: bool = True, rollout: bool = False, layers=None, max_bytes: int = 1 << 30):
    """The no-autograd forward of encoder() (lengths: encoder_ragged()) followed by egx_encoder_self_weights on its `saved`, and the rollout if
    asked for. Returns (the forward's output, AttentionRecord). The output has the bits of the same call without the record."""
    if spec.training:
        raise ValueError("encoder_attention is inference-only (spec.training is set)")
    K, L, B = len(spec.segments), spec.n_layers, feats[0].shape[0]
    rec = AttentionRecorder(weights, by_segment, rollout, layers, max_bytes)
    S = sum(ss.T for ss in spec.segments) if lengths is None else int(lengths.sum(1).max())
    rec.plan(B, S, K, L, spec.d_model, spec.n_heads)            # (refusals before any device work)
    with torch.no_grad(), rec:
        if lengths is None:
            out = encoder(spec, feats, task_embed, pos_table, ln_w, ln_b, proj, layer_params, head_params)
        else:
            out = encoder_ragged(spec, feats, lengths, task_embed, pos_table, ln_w, ln_b, proj, layer_params, head_params)
    return out, rec.records[-1]
