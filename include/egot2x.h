/*
 * egot2x.h — C ABI of libegot2x.so, the MI355X (gfx950) native task-translation
 * transformer ("translator") for EgoT2's Stage-II fusion path.
 *
 * The reference has no native code: its translator is a chain of torch.nn calls.
 * Each entry point below replaces the torch.nn call sites named next to it
 * (paths relative to the reference checkout):
 *
 *   egx_encoder_fwd / egx_encoder_bwd
 *       HHI/models/ttm/model_taskspecific.py:222-226,238-242 (proj_* -> encode_prepare -> cat
 *       -> nn.TransformerEncoder), HHI/models/asd/model_taskspecific.py:133-155,
 *       HHI/models/multitask/task_prompt_model.py:224-250,
 *       HOI/models/lta/lta_models_lta_transfer.py:355-361 (proj_* -> cat -> ln + pe -> transformer),
 *       HOI/models/pnr/video_model_transfer_3task.py:249-255,
 *       HOI/models/multitask/video_model_builder.py:331-346; and their autograd backward.
 *   egx_pool_head_fwd / egx_pool_head_bwd
 *       HHI/models/ttm/model_taskspecific.py:243-244 (mean over tokens -> linear_head = LN + Linear),
 *       HOI/models/pnr/video_model_transfer_3task.py:256-257; HOI LTA mean-pool
 *       (lta_models_lta_transfer.py:362) with ln == NULL and W == NULL.
 *   egx_linear_fwd / egx_linear_bwd
 *       any nn.Linear on the path that is not inside the encoder (HOI MultiTaskHead projections,
 *       HOI/models/lta/head_helper.py:245-248,281-283).
 *   egx_gemm / egx_layernorm_* / egx_attention_*
 *       the individual ATen ops (addmm, layer_norm, multi_head_attention_forward core) for unit parity tests.
 *   egx_grad_norm + egx_counter_add_gated / egx_lr_update_gated / egx_adam_step_guarded / egx_sgd_step_guarded
 *       what pytorch_lightning.Trainer(gradient_clip_val=, track_grad_norm=) does around the optimizer step (the reference
 *       constructs its Trainer with the defaults, HHI/scripts/run_ttm.py:21, HOI/scripts/lta/run_lta.py:238) and an eager
 *       loop's torch.isfinite(loss) test, as device work a captured step replays (ABI v28 additions below).
 *
 * Conventions
 *   - All tensors are dense fp32, row-major, device memory owned by the caller (PyTorch's caching
 *     allocator). The library never allocates device memory; `saved` and `scratch` are caller-provided
 *     workspaces sized by egx_encoder_workspace().
 *   - Token layout is batch-first packed (B, S, d): one clip's S*d block is contiguous.
 *   - Weights are torch-style [out, in] row-major.
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no host sync and
 *     is hipGraph-capturable.
 *   - Return value 0 = success; non-zero = error, message via egx_last_error() (thread-local).
 *   - `compute`: EGX_F32 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32), EGX_BF16 = bf16 MFMA operands with
 *     fp32 accumulation, fp32 LayerNorm/softmax statistics, fp32 storage. EGX_F32_SPLIT = fp32 operands split exactly into
 *     three bf16 parts and multiplied by six v_mfma_f32_16x16x32_bf16 per K-block (the dropped cross terms are below fp32's
 *     own product rounding): fp32-grade results at 2.7x the matrix rate of the fp32 MFMA. Implemented by the fused d = 128
 *     kernels; everywhere else it means EGX_F32.
 */
#ifndef EGOT2X_H
#define EGOT2X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGX_ABI_VERSION 18
#define EGX_MAX_SEGMENTS 8

enum { EGX_F32 = 0, EGX_BF16 = 1, EGX_F32_SPLIT = 2 };
enum { EGX_IMPL_AUTO = 0, EGX_IMPL_GENERIC = 1, EGX_IMPL_FUSED = 2, EGX_IMPL_WIDE = 3, EGX_IMPL_TILED = 4 };

/* One contiguous run of tokens of the packed sequence, produced from one frozen-backbone feature
 * tensor: tokens[b, off + t, :] = LN(feat[b, t, :] @ proj_w^T + proj_b) + add_vec + pos[t * pos_stride + :]
 * (LN is the encoder's shared `ln`; proj_w == NULL means the feature is already d_model wide). */
typedef struct egx_segment {
    const float* feat;    /* (B, T, d_in) */
    int T;
    int d_in;
    const float* proj_w;  /* [d_model, d_in] or NULL */
    const float* proj_b;  /* [d_model] or NULL */
    const float* add_vec; /* [d_model] task-embedding row, or NULL */
    const float* pos;     /* first positional row for this segment, or NULL */
    int pos_stride;       /* floats between consecutive positional rows */
    /* Feature hand-off from the frozen backbones (wide bf16 path only, projected segments only):
     * feat_bf16 != 0: `feat` points at bf16 data (the backbone wrote its `middle=True` features in the packed bf16 layout
     *                 the projection GEMM reads; no fp32 copy, no cast pass).
     * pool > 1      : `feat` holds (B, T * pool, d_in) per-FRAME features and token t is the mean of frames
     *                 [t * pool, (t + 1) * pool): the temporal mean of HOI encode_clips_pnr
     *                 (HOI/models/lta/lta_models_lta_transfer.py:335-343, `tmp.mean(dim=1)`) fused with the cast into the
     *                 projection operand, so the pooled fp32 tensor is never written. */
    int feat_bf16;
    int pool;
} egx_segment;

/* Gradient sinks matching egx_segment; any pointer may be NULL (gradient not wanted).
 * All sinks are ACCUMULATED into (+=): the caller zero-fills them once per backward. */
typedef struct egx_segment_grads {
    float* proj_w;
    float* proj_b;
    float* add_vec;
    float* pos;       /* [T, d_model] rows with stride pos_stride (learned pe), or NULL */
    float* feat;      /* (B, T, d_in) gradient into the feature, or NULL (frozen backbones) */
} egx_segment_grads;

/* nn.TransformerEncoderLayer parameters (post-LN, ReLU). */
typedef struct egx_layer {
    const float* in_proj_w;  /* [3d, d] rows = [Wq; Wk; Wv] */
    const float* in_proj_b;  /* [3d] */
    const float* out_proj_w; /* [d, d] */
    const float* out_proj_b; /* [d] */
    const float* lin1_w;     /* [d_ff, d] */
    const float* lin1_b;     /* [d_ff] */
    const float* lin2_w;     /* [d, d_ff] */
    const float* lin2_b;     /* [d] */
    const float* norm1_w;
    const float* norm1_b;
    const float* norm2_w;
    const float* norm2_b;
} egx_layer;

typedef struct egx_layer_grads {
    float* in_proj_w;
    float* in_proj_b;
    float* out_proj_w;
    float* out_proj_b;
    float* lin1_w;
    float* lin1_b;
    float* lin2_w;
    float* lin2_b;
    float* norm1_w;
    float* norm1_b;
    float* norm2_w;
    float* norm2_b;
} egx_layer_grads;

struct egx_ce;
struct egx_token_ce;
typedef struct egx_config {
    /* d_model: a multiple of 4 up to 1024 in every compute mode. 1024 < d_model <= 2048 (the 2048-wide HOI LTA 2-task translator) runs with
     * compute EGX_BF16 on the wide path only: impl auto or wide, d_model % 128 == 0, d_ff % 128 == 0, and a token count S its attention
     * serves at head dim d_model / n_heads (S <= 128: 32 / 64 / 96 / 128; S <= 16: 256 / 512). compute f32 / f32s, impl generic / fused /
     * tiled or another (S, head dim) are refused above 1024 with an error that says "compute bf16, wide path"; ragged batches
     * (egx_ragged_encode*) stay at 1024. Nothing above 2048 is accepted. */
    int d_model;
    int n_heads;
    int d_ff;
    int n_layers;
    int n_segments;
    float ln_eps;
    int compute;      /* EGX_F32 | EGX_BF16 | EGX_F32_SPLIT */
    int impl;         /* EGX_IMPL_* */
    float p_drop;     /* encoder-layer dropout (attention probs, dropout1, FFN hidden, dropout2) */
    float p_pos;      /* dropout on the token-prep output (PositionalEncoding.dropout, fixed 0.1 in HHI) */
    float p_feat;     /* dropout on projected features before LN (HOI `dp`) */
    const uint64_t* seed_ptr; /* optional DEVICE pointer: when non-NULL the per-clip, tiled and wide bf16 kernels derive their dropout keys
                                 from *seed_ptr instead of the host `seed` argument, so a captured hipGraph draws fresh
                                 masks on every replay (advance it with egx_seed_advance inside the graph, or set
                                 advance_seed). */
    int advance_seed;         /* 1 with seed_ptr: a training-mode forward advances *seed_ptr by one LCG step before
                                 using it (folded into its first kernel), the backward of that forward reads the
                                 advanced value. 2 (ABI v15): the forward uses *seed_ptr as it is and the BACKWARD advances it
                                 behind its last reader (folded into its last launch): a forward + backward step needs no launch
                                 in front of the forward even when the packing launch is skipped (weight_cache_valid); a training
                                 forward that is never followed by its backward repeats the masks of the previous one. */
    void* zero_buf;           /* optional: a device buffer the BACKWARD zero-fills before any gradient is accumulated */
    size_t zero_bytes;        /* (the caller's flat gradient buffer: saves a separate fill launch); multiple of 16 */
    int bwd_stage;            /* backward only: 0 = everything; 1 = all but the grouped small weight gradients (dW_proj,
                                 dW_in, dW_o); 2 = only those (same arguments, zero_buf ignored). Lets the caller start the
                                 all-reduce of every other gradient while stage 2 still runs (fused path; the generic
                                 path does all its work in stage 1). */
    int deterministic;        /* != 0: every cross-workgroup sum of the BACKWARD runs in a fixed order (split-K slabs and
                                 per-clip partial rows reduced by one workgroup per output instead of fp32 atomics), so the
                                 same inputs and seed give bit-identical gradients run to run. Honoured by the fused per-clip
                                 kernels and the shape-generic kernels (split-K slabs, LayerNorm / bias / pooled-head partial
                                 buffers with ordered sums; pass the same flag to the workspace query: it sizes their scratch);
                                 the wide bf16 path is always deterministic. */
    int out_tokens;           /* 0 = the whole sequence. T > 0: only the first T tokens of every clip leave the encoder
                                 (tokens_out is (B, T, d)) and only they receive an upstream gradient (d_tokens is (B, T, d)) —
                                 the ASD translator returns its first segment, HHI/models/asd/model_taskspecific.py:156-158;
                                 without this the caller slices (copy) and autograd zero-fills and scatters the gradient.
                                 Fused per-clip kernels only (egx_encoder_impl() == EGX_IMPL_FUSED); an error elsewhere. */
    void (*bucket_cb)(void* user, int bucket);   /* BACKWARD, optional (wide bf16 path): called on the host thread right after the
                                 kernels that complete gradient bucket `bucket` have been enqueued on the stream. Bucket b in
                                 [0, n_layers) = every parameter gradient of encoder layer n_layers - 1 - b (the order the backward
                                 finishes them); everything else (projections, shared LayerNorm, embeddings) is complete when the
                                 call returns. The caller lays its flat gradient buffer out last-layer-first and starts the
                                 all-reduce of a layer's slice from the callback, so the exchange of layer l overlaps the backward
                                 of layers l - 1 .. 0 (the reference gets this from DDP's bucketed reducer,
                                 HOI/scripts/multitask/run.py:41-50). With a callback every split-K slab reduction runs right
                                 behind its GEMM (no deferred batch). Other implementations ignore it. */
    void* bucket_user;
    /* ---- ABI v15 (round 6) ---- */
    void* weight_cache;       /* optional PERSISTENT device buffer of egx_weight_cache_bytes() bytes (per-clip / tiled kernels): the
                                 MFMA-fragment-packed copies of the weights live there instead of in `saved`, so that a forward whose
                                 weights did not change since the forward that filled it can skip the packing launch
                                 (weight_cache_valid). The backward must be given the same buffer. NULL: packed into `saved` every forward.
                                 Its last 256 bytes are a control block of the library (arrival counter + accumulator of the fused
                                 cross entropy); a forward that packs resets it, so the buffer needs no initialisation. One cache
                                 serves one stream at a time. */
    int weight_cache_valid;   /* forward, with weight_cache: != 0 = the cache holds the packed copies of EXACTLY these weights in this
                                 compute mode with this FFN keep-scale (training, p_drop): nothing is packed. The caller owns that
                                 promise (egot2_amd/translator.py keys it on the parameters' storage and version counters). */
    const float* d_logits_scale; /* backward, optional DEVICE scalar: the pooled head's backward multiplies d_logits by it (the upstream
                                 gradient of a loss the forward computed itself, egx_ce; lets loss.backward() hand its ones / loss-scale
                                 tensor over without a launch). Per-clip kernels only; NULL = 1. */
    const struct egx_ce* ce;  /* forward, optional (egx_translator_fwd with a head): weighted cross entropy on the logits, see egx_ce */
    /* ---- ABI v16 (round 6) ---- */
    const struct egx_token_ce* token_ce;  /* forward + backward, optional (egx_encoder_fwd / _bwd with out_tokens): per-token classifier + weighted
                                 cross entropy on the returned tokens, see egx_token_ce. Only where egx_encoder_token_ce_ok() says so. */
} egx_config;

/* Weighted cross entropy ON the pooled head's logits, evaluated by the translator forward itself
 * (nn.CrossEntropyLoss(weight=[0.266, 0.734])(model(...), target), HHI/tasks/ttm/video_task_2loader.py:21-22,34 — the same arithmetic as
 * egx_weighted_ce, labels outside [0, n_out) contribute neither loss, weight nor gradient). On the per-clip kernels it runs in the epilogue of
 * the launch that produces the logits (the normaliser sum_i w[y_i] depends on the labels only: every workgroup sums it itself), so
 * d loss / d logits is in place when the backward starts and the step has one launch less; elsewhere (tiled / wide / generic kernels,
 * deterministic mode) the library appends the egx_weighted_ce launch. Pass `d_logits` as egx_translator_bwd's d_logits (scaled by
 * egx_config.d_logits_scale when the loss itself has an upstream gradient other than 1). */
typedef struct egx_ce {
    const int64_t* target;      /* (B) class indices */
    const float* class_weight;  /* (n_out) or NULL (= 1) */
    float* loss;                /* scalar, written */
    float* d_logits;            /* (B, n_out), written */
} egx_ce;

/* Per-token classifier + weighted cross entropy ON the tokens the encoder returns, evaluated by the encoder launches themselves: the ASD task's
 * lossAV on the translator's per-frame output (HHI/tasks/asd/video_task_taskspecific.py:24,33 -> HHI/tasks/asd/loss.py:11-30: x = FC(x);
 * nloss = CrossEntropyLoss(weight=[1, 4])(x, labels); softmax scores, rounded labels, number of correct frames). The arithmetic of
 * egx_linear_ce_fwd / _bwd; as two launches of their own they are 27 us of the 0.41 ms ASD step. Forward: the launch that normalises the last layer's
 * tokens also writes logits / probs / pred / d_logits of the clip's out_tokens rows and adds the clip's loss and correct-frame terms (the
 * normaliser sum_i w[y_i] depends on the labels only: every workgroup sums it itself). Backward (egx_encoder_bwd with d_tokens = NULL): the first
 * launch rebuilds d tokens = g * d_logits W per clip and leaves the clip's partial d W / d b rows to the step's fixed-order reduction; g =
 * *egx_config.d_logits_scale (NULL = 1). The tokens themselves are still written (tokens_out). */
typedef struct egx_token_ce {
    const float* W;             /* (C, d) classifier weight */
    const float* b;             /* (C) or NULL */
    const int64_t* target;      /* (B * out_tokens) class indices; outside [0, C): no loss, no weight, no gradient */
    const float* class_weight;  /* (C) or NULL (= 1) */
    int C;                      /* 1 <= C <= 8 */
    float* logits;              /* (B * out_tokens, C), written by the forward */
    float* probs;               /* same shape, optional: softmax(logits) */
    float* pred;                /* (B * out_tokens), optional: round(probs[:, 1]) */
    float* loss;                /* scalar, written by the forward */
    float* correct;             /* scalar, optional: rows with pred == target */
    float* d_logits;            /* (B * out_tokens, C): written by the forward, read by the backward */
    float* d_W; float* d_b;     /* backward: (C, d) and (C), each optional: the gradients are ADDED (as every parameter gradient of
                                   egx_encoder_bwd: into the caller's zero_buf-covered flat buffer, or pre-zeroed memory) */
} egx_token_ce;

int egx_abi_version(void);
/* != 0: this configuration and batch run on kernels that evaluate egx_config.token_ce themselves (one clip per workgroup, one launch per
 * direction, a persistent weight cache, no pooled head). Elsewhere the caller composes egx_linear_ce_fwd / _bwd with the encoder calls. */
int egx_encoder_token_ce_ok(const egx_config* cfg, const egx_segment* segs, int B);
/* The kernel-selection switches (EGX_FFN_CUT, EGX_FFN_SLICES, EGX_SLICE_DROP, EGX_DEC_GROUP, EGX_WIDE_TILE: development and test aids, INTEGRATION.md
 * section 4) are read from the environment once, at first use; this re-reads them (the parity tests compare the modes inside one process). */
void egx_tuning_reload(void);
/* Bytes of egx_config.weight_cache for this configuration (0: this configuration does not run on kernels that pack weights). Depends on
 * the model dimensions and the compute mode, not on the batch. */
size_t egx_weight_cache_bytes(const egx_config* cfg, const egx_segment* segs);
/* Kernel launches (and memsets) the library has enqueued on this thread's behalf since the last reset: the bench reports
 * launches per step with it. reset != 0 zeroes the counter after reading. Not thread-safe (a diagnostic). */
long long egx_launch_count(int reset);
const char* egx_last_error(void);

/* Workspace sizes in bytes for a batch of B clips of S tokens (S = sum of segment T). */
int egx_encoder_workspace(const egx_config* cfg, const egx_segment* segs, int B,
                          size_t* saved_bytes, size_t* scratch_bytes);

/* 1 when this configuration runs on the fused per-clip kernels (which leave d_tokens untouched in backward),
 * 0 for the shape-generic kernels (which consume d_tokens). */
int egx_encoder_uses_fused(const egx_config* cfg, const egx_segment* segs, int B);
/* Which kernels this configuration runs on: EGX_IMPL_FUSED (per-clip kernels: d = 128, h = 4, S <= 48), EGX_IMPL_TILED (the same
 * kernels over 48-token tiles with the attention of the whole clip between the launches: d = 128, h = 4, 48 < S <= 512, compute bf16
 * or f32s - the reference's real TTM / ASD batches of 15 .. 150 frames per task, HHI/dataset/ttm/data_loader_2task.py:119,150-162), EGX_IMPL_WIDE
 * (compute = bf16 with d_model >= 256, d_model / d_ff / projected d_in multiples of 128, d_model <= 2048, S <= 128 with head dim 32 / 64 / 96 / 128, S <= 512 with head dim 32 / 64 or S <= 16 with head dim 256 / 512: all B*S tokens
 * through bf16-storage MFMA GEMMs and MFMA attention - BASELINE.json configs[3], configs[4]) or EGX_IMPL_GENERIC; -1 on an
 * invalid configuration. */
int egx_encoder_impl(const egx_config* cfg, const egx_segment* segs, int B);
/* Workgroups per clip of the per-clip kernels (EGX_IMPL_FUSED) for this batch on the current device: 1, or 2 / 4 / 8 for small
 * batches (round_up(B, 8) * n <= compute units; the reference's own TTM batches are ~26 clips, HHI/dataset/ttm/sampler.py:41, and
 * strong scaling leaves 32 clips per GPU): every workgroup of a clip runs the clip except the FFN, of which it walks 1 / n of the
 * hidden blocks; the partial sums are exchanged through device memory. A partial sum that does not arrive within 100 us (its
 * workgroup is not resident: the device is shared) is computed by the waiting workgroup itself, so the result never depends on
 * the scheduling. EGX_FFN_SLICES=1 in the environment turns it off, =2 / 4 / 8 caps n. -1: invalid configuration. */
int egx_encoder_slices(const egx_config* cfg, const egx_segment* segs, int B);

/* tokens_out: (B, S, d). `saved` is written in forward and read in backward.
 * training != 0 applies dropout with masks derived from (seed, site, element). */
int egx_encoder_fwd(const egx_config* cfg, const egx_segment* segs,
                    const float* ln_w, const float* ln_b,
                    const egx_layer* layers, int B,
                    float* tokens_out, void* saved, void* scratch,
                    int training, uint64_t seed, void* stream);

/* d_tokens: (B, S, d) gradient w.r.t. tokens_out; it is consumed (overwritten). */
int egx_encoder_bwd(const egx_config* cfg, const egx_segment* segs,
                    const float* ln_w, const float* ln_b,
                    const egx_layer* layers, int B,
                    float* d_tokens, const void* saved, void* scratch,
                    const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b,
                    const egx_layer_grads* layer_grads,
                    int training, uint64_t seed, void* stream);

/* Encoder + pooled task head in one call: logits = Linear(LN(mean_s tokens)), the TTM / PNR head
 * (HHI/models/ttm/model_taskspecific.py:243-244). On the fused per-clip path the head runs inside the encoder
 * kernels (tokens never leave the chip unless tokens_out != NULL); on the generic path it is appended.
 * Workspaces: egx_translator_workspace(). n_out <= 64. */
typedef struct egx_head {
    const float* ln_w; const float* ln_b;   /* head LayerNorm [d] */
    const float* W; const float* b;         /* [n_out, d], [n_out] */
    int n_out;
} egx_head;
typedef struct egx_head_grads { float* ln_w; float* ln_b; float* W; float* b; } egx_head_grads;   /* accumulated (+=) */
int egx_translator_workspace(const egx_config* cfg, const egx_segment* segs, int B,
                             size_t* saved_bytes, size_t* scratch_bytes);
int egx_translator_fwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                       const egx_layer* layers, const egx_head* head, int B, float* logits_out, float* tokens_out,
                       void* saved, void* scratch, int training, uint64_t seed, void* stream);
int egx_translator_bwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                       const egx_layer* layers, const egx_head* head, int B, const float* d_logits, const void* saved,
                       void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b,
                       const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, int training,
                       uint64_t seed, void* stream);

/* ---- ABI v17: ragged batches (inference) ----
 * One forward over B clips of their own lengths: clip b's result is the result of the same model on clip b alone, unpadded (the
 * reference's batch_size=1 validation loops, HHI/tasks/ttm/video_task_2loader.py:84-97, HHI/tasks/asd/video_task_taskspecific.py:69,76).
 *   lengths    HOST int[B * n_segments], clip-major: T_{b,k} = frames of segment k of clip b, 1 <= T_{b,k} <= segs[k].T. segs[k].feat stays
 *              a padded (B, segs[k].T, d_in) tensor (segs[k].T is the row stride of a clip); rows t >= T_{b,k} are never read. Inside a
 *              clip segment k starts at token sum_{j<k} T_{b,j}; positional rows restart at segs[k].pos for every segment.
 *   head       non-NULL: logits_out (B, n_out) = Linear(LN(mean over the clip's own S_b = sum_k T_{b,k} tokens)).
 *   head NULL  tokens_out holds the FIRST segment's rows of every clip, packed: sum_b T_{b,0} rows of d floats in clip order (the ASD
 *              translator's per-frame output, HHI/models/asd/model_taskspecific.py:156-158).
 * Runs on the tiled kernels: d = 128, h = 4, d_ff % 128 == 0, 1 .. 6 layers, <= 4 projected segments (d_in % 128 == 0), fp32 features,
 * compute bf16 or f32s, impl auto or tiled, S_b <= 512 tokens per clip (clips of S_b <= 48 are single tiles). Refused: p_drop / p_pos /
 * p_feat > 0 (inference only), out_tokens, ce, token_ce, bucket_cb. weight_cache / weight_cache_valid work as in egx_translator_fwd.
 * `workspace`: egx_ragged_workspace() bytes (a function of sum_b S_b, the tile count and the model, not of B * max S_b). The call writes a
 * per-clip table built from `lengths` into the workspace on `stream`: a captured hipGraph would replay THIS call's lengths for every batch,
 * so the ragged call is not meant for graph capture. */
int egx_ragged_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* bytes);
int egx_ragged_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, int B, float* logits_out, float* tokens_out, void* workspace,
                   void* stream);

/* ---- ABI v18: ragged batches on the wide bf16 path (inference) ----
 * The EgoT2-g HHI encoder (TaskTranslationPromptTransformer.encode, HHI/models/multitask/task_prompt_model.py:230-257) over B clips of
 * their own lengths, for the reference's batch_size=1 validation (HHI/tasks/multitask/video_tasktranslation.py:83-101,176-187). Clip b's
 * rows equal those of the same model on clip b alone, unpadded.
 *   lengths     HOST int[B * n_segments], clip-major, as egx_ragged_fwd: 1 <= T_{b,k} <= segs[k].T; segs[k].feat stays padded
 *               (B, segs[k].T, d_in), rows t >= T_{b,k} are never read. Clip b has S_b = sum_k T_{b,k} tokens.
 *   out_layout  0: tokens_out holds all S_b rows of every clip, packed clip after clip (sum_b S_b rows of d floats): the decoder memory
 *               of the tasks ttm / lam. 1: every clip has T_{b,k} = T_b for all k; the row of (frame f of the batch, segment k) is
 *               K f + k (frames counted over the clips in order): the asd memory of task_prompt_model.py:250-257, i.e. the (B S, d)
 *               layout egx_decoder_fwd reads with S = K, without a copy.
 * Runs on the wide bf16 path: compute bf16, impl auto or wide, d_model % 128 == 0 in [256, 1024] (smaller with impl wide), d_ff % 128 == 0,
 * 1 .. 64 layers, projected segments (d_in % 128 == 0, pool <= 1), fp32 or bf16 features, S_b within the wide attention (S_b <= 128 for
 * head dims 32 / 64 / 96 / 128; up to 480 at head dim 64 where two K | V images fit the LDS). Refused: p_drop / p_pos / p_feat > 0,
 * ce, token_ce, out_tokens, bucket_cb, compute other than bf16 (and no head: egx_ragged_fwd has one).
 * `workspace`: egx_ragged_encode_workspace() bytes, a function of sum_b S_b and the model (not of B * max S_b). The call writes a per-clip
 * table built from `lengths` into the workspace on `stream`: a captured hipGraph would replay THIS call's lengths, so it is not for capture. */
int egx_ragged_encode_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* bytes);
int egx_ragged_encode(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                      const egx_layer* layers, int B, float* tokens_out, int out_layout, void* workspace, void* stream);

/* ---- ABI v18: ragged batches on the wide bf16 path, training (EgoT2-g HHI) ----
 * The encoder side of one training step of the EgoT2-g HHI model (HHI/tasks/multitask/video_tasktranslation.py:39-66) over B clips of their
 * own lengths: the reference cannot batch such clips, so it feeds same-length mini-batches of <= 15 clips (SequenceBatchSampler,
 * video_tasktranslation.py:144-156) through encode() (HHI/models/multitask/task_prompt_model.py:230-258). lengths, segs, out_layout and
 * tokens_out as egx_ragged_encode; a clip's rows, and its contribution to every gradient, are what that clip gives alone and unpadded.
 *   training / seed / cfg->seed_ptr / cfg->advance_seed   dropout as egx_encoder_fwd (p_drop, p_pos; p_feat on the projections). Row sites
 *               (positional, the two residual branches, FFN hidden) key on the packed token row, the feature dropout on the compacted row of its
 *               segment, the attention on (clip's index in the batch, head, query) with the row stride of the clip's kernel class (128 for
 *               S_b <= 128, 512 beyond): a batch whose clips all have the padded lengths draws the masks of egx_encoder_fwd with that seed.
 *   egx_ragged_encode_bwd takes the SAME lengths and out_layout and the forward's `saved`; d_tokens in the layout of tokens_out (out_layout 1:
 *               read back through the same row map). Gradients are ADDED into the egx_segment_grads / egx_layer_grads targets after
 *               cfg->zero_buf / zero_bytes (if set) has been zero-filled, as egx_encoder_bwd. All cross-workgroup sums run in a fixed order:
 *               the same batch and seed give bit-identical gradients.
 * Limits of egx_ragged_encode. Refused with a message: ce, token_ce, out_tokens, bucket_cb, bwd_stage != 0, compute other than bf16, a clip
 * beyond the wide attention, egx_segment_grads.feat (gradients into projected features) and egx_segment_grads.pos (a learned positional table).
 * `saved` / `scratch`: egx_ragged_encode_train_workspace() bytes, functions of sum_b S_b and the model (never of B * max S_b). The forward
 * writes a per-clip table built from `lengths` into `saved` on `stream` (the backward reads it there): a captured hipGraph would replay THIS
 * call's lengths, so the calls are not for graph capture. */
int egx_ragged_encode_train_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* saved_bytes,
                                      size_t* scratch_bytes);
int egx_ragged_encode_train_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                                const egx_layer* layers, int B, float* tokens_out, int out_layout, void* saved, int training, uint64_t seed,
                                void* stream);
int egx_ragged_encode_bwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const egx_layer* layers, int B,
                          const float* d_tokens, int out_layout, const void* saved, void* scratch, const egx_segment_grads* seg_grads,
                          float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads, int training, uint64_t seed, void* stream);

/* ---- ABI v18: ragged batches for training (d = 128 TTM / ASD translators) ----
 * One forward + backward over B clips of their own lengths, every clip keeping all of its frames: replaces the reference's sorted
 * ~400-frame batches truncated to their shortest clip (HHI/dataset/ttm/sampler.py:14-60, HHI/utils/ttm/utils.py:232-241) in the TTM
 * training step (HHI/tasks/ttm/video_task_2loader.py:30-36) and the ASD one (HHI/tasks/asd/video_task_taskspecific.py:26-37).
 *   lengths, segs, head, logits_out, tokens_out   as egx_ragged_fwd (head NULL: the first segment's rows of every clip, packed).
 *   training, seed, seed_ptr, advance_seed, deterministic, d_logits_scale, zero_buf, weight_cache   as egx_translator_fwd / _bwd.
 *   dropout (training != 0): site_key(seed, layer, site) / rand_quad as the other paths; with tok0_b = sum_{b' < b} S_b' the row of token s
 *              of clip b is tok0_b + s (POS, RES1, FFN, RES2; column = feature / hidden unit) and the ATTN row of (head h, query q) is
 *              4 tok0_b + h S_b + q (column = key). Clips of equal S > 48 thus draw exactly the masks of the tiled training call.
 *   ce         (with a head) the weighted cross entropy of the logits is appended to the forward (loss and d_logits as egx_translator_fwd).
 *   egx_ragged_bwd takes the SAME lengths and the forward's `saved`; d_logits (B, n_out) with a head, else d_tokens in the packed output
 *              shape (the other segments' rows get no upstream gradient). Gradients follow egx_translator_bwd; seg_grads[k].feat (optional)
 *              is WRITTEN as the padded (B, segs[k].T, d_in) gradient with exact zeros in the padded frames; pos gradients are refused.
 * Runs on the tiled kernels, limits of egx_ragged_fwd; refused: p_feat > 0, out_tokens, token_ce, bucket_cb, bwd_stage != 0.
 * `saved` / `scratch`: egx_ragged_train_workspace() bytes (functions of sum_b S_b and the tile count, not of B * max S_b). Each call
 * writes the batch table on `stream`: not for graph capture (egx_ragged_cap_train_fwd / egx_ragged_cap_bwd below are). */
int egx_ragged_train_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* saved_bytes,
                               size_t* scratch_bytes);
int egx_ragged_train_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                         const egx_layer* layers, const egx_head* head, int B, float* logits_out, float* tokens_out, void* saved,
                         void* scratch, int training, uint64_t seed, void* stream);
int egx_ragged_bwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, int B, const float* d_logits, const float* d_tokens, const void* saved,
                   void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads,
                   const egx_head_grads* head_grads, int training, uint64_t seed, void* stream);

/* pooled = mean_s tokens[b, s, :]; y = ln_w ? LN(pooled) : pooled; out = W ? y W^T + b : y.
 * `pooled_saved` (B, d) is kept for backward. n_out <= 64 when W != NULL; d <= 1024 (any d, multiple of 4 or not), or a multiple of 128 up to 2048 (the wide bf16 path's widths). Both are checked: a call
 * outside them returns non-zero and writes nothing.
 * Backward: d_tokens (B, S, d) is overwritten (=), the S rows of a clip all alike; d_ln_w, d_ln_b, d_W and d_b are added into (+=, the clips
 * meet in fp32 atomics) and may each be NULL. */
int egx_pool_head_fwd(const float* tokens, int B, int S, int d,
                      const float* ln_w, const float* ln_b, float ln_eps,
                      const float* W, const float* b, int n_out,
                      float* pooled_saved, float* out, void* stream);
int egx_pool_head_bwd(const float* d_out, const float* pooled_saved, int B, int S, int d,
                      const float* ln_w, const float* ln_b, float ln_eps,
                      const float* W, int n_out,
                      float* d_tokens, float* d_ln_w, float* d_ln_b, float* d_W, float* d_b,
                      void* stream);

/* y[M,N] = x[M,K] W[N,K]^T + b (+ReLU). */
int egx_linear_fwd(const float* x, const float* W, const float* b, float* y,
                   int M, int N, int K, int relu, int compute, void* stream);
/* y = x W^T + b + residual[M,N]: a projection with the residual connection in its epilogue (pre-LN blocks of
 * HOI/models/pnr/simple_vit.py:104-106: `x = attn(x) + x`, `x = ff(x) + x`). b may be NULL. */
int egx_linear_residual_fwd(const float* x, const float* W, const float* b, const float* residual, float* y, int M, int N, int K,
                            int compute, void* stream);
/* Exact (erf) GELU, nn.GELU() of simple_vit.FeedForward (HOI/models/pnr/simple_vit.py:55-65): h = z Phi(z);
 * backward dz = dh (Phi(z) + z phi(z)). n %% 4 == 0. */
int egx_gelu_fwd(const float* z, float* h, size_t n, void* stream);
int egx_gelu_bwd(const float* z, const float* dh, float* dz, size_t n, void* stream);
/* dx[M,K] = dy W ; dW[N,K] += dy^T x ; db[N] += colsum(dy). Any output may be NULL.
 * scratch must hold egx_linear_bwd_scratch(M,N,K) bytes. dW needs it (and x); dx and db alone also run with scratch = NULL. */
size_t egx_linear_bwd_scratch(int M, int N, int K);
int egx_linear_bwd(const float* dy, const float* x, const float* W,
                   float* dx, float* dW, float* db, int M, int N, int K,
                   int compute, void* scratch, void* stream);
/* db[N] += colsum(dy[M,N]) summed in a fixed order (row blocks' partial sums through scratch, added in block order): the same bits on
 * every run, where egx_linear_bwd's db meets in fp32 atomics. scratch must hold egx_colsum_ordered_scratch(M,N) bytes (0: may be NULL); a
 * call with fewer scratch_bytes is refused and leaves db alone. */
size_t egx_colsum_ordered_scratch(int M, int N);
int egx_colsum_ordered(const float* dy, int M, int N, float* db, void* scratch, size_t scratch_bytes, void* stream);

/* --- single-op entry points (unit parity tests) --- */
/* layout: 0 = NT (C = A[M,K] B[N,K]^T), 1 = NN (C = A[M,K] B[K,N]), 2 = TN (C = A[K,M]^T B[K,N]). */
int egx_gemm(int layout, const float* A, const float* B, float* C, int M, int N, int K,
             const float* bias, int relu, int compute, void* scratch, size_t scratch_bytes, void* stream);
int egx_layernorm_fwd(const float* x, const float* res, const float* w, const float* b, float eps,
                      float* pre, float* stats, float* y, int rows, int d, void* stream);
int egx_layernorm_bwd(const float* dy, const float* pre, const float* stats, const float* w,
                      float* dx, float* dw, float* db, int rows, int d, void* stream);
/* qkv: (B, S, 3d) packed in-proj output; out: (B, S, d); lse: (B, H, S). */
int egx_attention_fwd(const float* qkv, float* out, float* lse, int B, int S, int H, int d,
                      float p_drop, uint64_t seed, void* stream);
int egx_attention_bwd(const float* qkv, const float* out, const float* lse, const float* d_out,
                      float* d_qkv, int B, int S, int H, int d,
                      float p_drop, uint64_t seed, void* stream);

/* --- unit hooks of the wide bf16 path (operands are bf16 in device memory, passed as void*) ---
 * layout 0 (NT): C[M,N] = A[M,K] B[N,K]^T (+ bias) (ReLU) (+ residual[M,N] fp32): the nn.Linear forward / input gradient.
 * layout 2 (TN): C[M,N] = A[K,M]^T B[K,N]: the nn.Linear weight gradient over K = B*S tokens (M, N multiples of 128).
 * Cf (fp32) and / or Cb (bf16) receive the result (TN: Cf only). K %% 64 == 0 for NT. scratch: egx_wide_gemm_scratch() bytes. */
size_t egx_wide_gemm_scratch(int layout, int M, int N, int K);
int egx_wide_gemm(int layout, const void* A, const void* B, float* Cf, void* Cb, int M, int N, int K, const float* bias,
                  int relu, const float* residual, void* scratch, void* stream);
/* qkv: (B*S, 3d) packed bf16 in-projection rows; out: (B*S, d) bf16; lse: (B, H, S) fp32. S <= 128 with head dim 32/64/96/128,
 * or 128 < S <= 480 with head dim 32/64 (the EgoT2-g encoders on sequences of up to 3 x 150 tokens: online softmax),
 * or 1 <= S <= 16 with head dim 256/512 (the 2048-wide LTA 2-task translator: one wave per (clip, head)); a head dim of 256 / 512 with
 * S > 16 is refused.
 * Backward: d_out (B*S, d) bf16 -> d_qkv (B*S, 3d) bf16 (probabilities recomputed from lse; every element written once).
 * S > 128 also reads `out` (the forward's output) and uses `delta` ((B, H, S) fp32 scratch); both may be NULL for S <= 128. */
int egx_wide_attention_fwd(const void* qkv, void* out, float* lse, int B, int S, int H, int d, float p_drop, uint64_t seed,
                           void* stream);
int egx_wide_attention_bwd(const void* qkv, const void* out, const float* lse, const void* d_out, void* d_qkv, float* delta,
                           int B, int S, int H, int d, float p_drop, uint64_t seed, void* stream);
/* ---- ABI v25 additions (new symbols only, as v19 to v24: EGX_ABI_VERSION stays 18): every kernel of the wide bf16 path on its own -------
 * Each hook fills the parameter struct the encoder / decoder drivers fill and calls the function they call (wide_gemm_nt, wide_gemm_tn,
 * wide_tn_queue_add / _flush, wide_reduce_flush, wide_ln_fwd / _bwd and their _mapped forms, wide_row_reduce_flush, wide_colsum_bf16,
 * wide_pos_grad, wide_cast, wide_pool_cast, wide_gather_cast): no arithmetic of their own. Dropout is given as (p, seed, layer, site) and
 * keyed as the drivers key it: site_key(seed, layer, site), threshold and 1 / (1 - p) of p (sites: 1 FEAT, 2 POS, 3 ATTN, 4 RES1, 5 FFN,
 * 6 RES2). Bad arguments (null pointers, pointers that are not 16-byte aligned, leading dimensions below the width or unaligned, K % 64
 * for NT, M / N % 128 for TN, d % 4 or d > 2048, ...) are refused before anything is enqueued.
 *
 * egx_wide_gemm_ex: WideGemmParams in full.
 *   NT (layout 0)  C[m][n] = residual[m][n] + mask[m][n] ? mask_scale * v : 0, v = dropout_(m, n)(relu(sum_k A[m][k] B[n][k] + bias[n]));
 *                  Cf (fp32) and / or Cb (bf16), both (M, ldc); colsum (egx_wide_gemm_colsum_rows(M, N), N): column sums of the result per
 *                  64 output rows of every tile (of the bf16-rounded values when Cb is written); rows past M add nothing.
 *   TN (layout 2)  Cf[m][n] (+)= sum_k A[k][m] B[k][n] (accumulate = 1: +=). tn_queue: through the grouped launch (wide_tn_queue_add, then
 *                  wide_tn_queue_flush and wide_reduce_flush); tn_defer: wide_gemm_tn with its slab reduction deferred to wide_reduce_flush.
 *                  bias, relu, dropout, residual, mask, colsum and Cb are refused.
 *   scratch        egx_wide_gemm_scratch(layout, M, N, K) bytes of the problem's own (its first 1024 bytes become the zero page).
 * egx_wide_gemm_tn_batch: n <= 32 TN problems; the queued ones share ONE grouped grid per tile variant, the deferred reductions one launch.
 * egx_wide_gemm_variant: what the dispatcher picks. NT: 0 = 64 x 64 tiles, 1 = 128 x 128 with four stages, 2 = 128 x 128 with two,
 *   3 = 256 x 128, 4 = ping-pong 256 x 256, 5 = ping-pong 256 x 192 (`colsum` != 0: for a launch with column sums). TN: tile variant
 *   (0 = 128 x 128, 1 = 256 x 128, 2 = 256 x 256) + 256 * split-K count. -1: not a problem of that layout. */
typedef struct egx_wide_gemm_args {
    int layout;
    const void* A; const void* B; int M, N, K, lda, ldb;
    float* Cf; void* Cb; int ldc;
    const float* bias; int relu;
    float p_drop; uint64_t seed; uint32_t layer, site;
    const float* residual; int ldr;
    const void* mask; int ldm; float mask_scale;
    float* colsum;
    int accumulate;
    int tn_queue, tn_defer;
    void* scratch;
} egx_wide_gemm_args;
int egx_wide_gemm_ex(const egx_wide_gemm_args* args, void* stream);
int egx_wide_gemm_tn_batch(const egx_wide_gemm_args* args, int n, void* stream);
int egx_wide_gemm_colsum_rows(int M, int N);
int egx_wide_gemm_variant(int layout, int M, int N, int K, int colsum);
/* egx_wide_layernorm_fwd: y[orow] = dropout_(orow, c)(LN(x[row]) * w + b + add_vec + pos[t * pos_stride ...]), stats[row] = (mean, rstd).
 *   uniform (out_map NULL): orow = (row / T) * S + off + row % T, t = row % T; d % 4 == 0, d <= 2048.
 *   mapped (out_map given): orow = out_map[row], t = src_map[row] % T (pos needs src_map); d <= 1024.
 * egx_wide_layernorm_bwd: g = dropout_(orow, c)(dy[orow]) (p_drop / layer / site; mapped: orow = dy_map[row]); dx = LN backward of g at
 *   pre[row], stats[row]; m = dropout_(row, c)(dx) (p_out / out_layer / out_site). dx32 = mask_dx32 ? m : dx; dx16 = bf16(m);
 *   dw += sum g xhat, db += sum g, dadd += sum g, dbias += column sums of m (of the bf16-rounded values when dx16 is written).
 *   defer != 0 (uniform only): the reduction is queued and run by wide_row_reduce_flush. scratch: egx_wide_layernorm_bwd_scratch bytes. */
typedef struct egx_wide_ln_fwd_args {
    const float* x; const float* w; const float* b; float eps;
    float* stats; float* y32; void* y16;
    int rows, d, T, S, off;
    const float* add_vec; const float* pos; int pos_stride;
    float p_drop; uint64_t seed; uint32_t layer, site;
    const int* out_map; const int* src_map;
} egx_wide_ln_fwd_args;
typedef struct egx_wide_ln_bwd_args {
    const float* dy; const float* pre; const float* stats; const float* w;
    float* dx32; void* dx16;
    int rows, d, T, S, off;
    float p_drop; uint64_t seed; uint32_t layer, site;
    float p_out; uint32_t out_layer, out_site;
    int mask_dx32;
    float* dw; float* db; float* dbias; float* dadd;
    const int* dy_map;
    int defer;
    void* scratch;
} egx_wide_ln_bwd_args;
int egx_wide_layernorm_fwd(const egx_wide_ln_fwd_args* args, void* stream);
size_t egx_wide_layernorm_bwd_scratch(int rows, int d);
int egx_wide_layernorm_bwd(const egx_wide_ln_bwd_args* args, void* stream);
/* out[c] += sum_r x[r][c] over a bf16 (rows, ld) matrix, cols % 8 == 0 (defer != 0: second stage through wide_row_reduce_flush).
 * dpos[t * pos_stride + c] += sum_b dropout_(b * S + off + t, c)(dtok[(b * S + off + t) * d + c]), t < T.
 * The scratch queries return the drivers' own (wide_colsum_scratch, wide_pos_grad_scratch): a launch writes nothing beyond them. */
size_t egx_wide_colsum_scratch(int rows, int cols);
int egx_wide_colsum(const void* x, int rows, int cols, int ld, float* out, int defer, void* scratch, void* stream);
/* n_ln deferred LayerNorm backwards (uniform form) and n_cs deferred column sums, n_ln + n_cs <= 48, each with a scratch of its own: their
 * second stages run as ONE wide_row_reduce_flush launch, as at the end of a backward. */
typedef struct egx_wide_colsum_args { const void* x; int rows, cols, ld; float* out; void* scratch; } egx_wide_colsum_args;
int egx_wide_row_reduce_batch(const egx_wide_ln_bwd_args* ln, int n_ln, const egx_wide_colsum_args* cs, int n_cs, void* stream);
size_t egx_wide_pos_grad_scratch(int B, int T, int d);
int egx_wide_pos_grad(const float* dtok, int B, int S, int off, int T, int d, float* dpos, int pos_stride, float p_drop, uint64_t seed,
                      uint32_t layer, uint32_t site, void* scratch, void* stream);
/* mode 0: dst[r][c] = bf16(src[r][c]) and / or dst_t[c][r] (src fp32 (R, ld); C % 4 == 0, R % 4 == 0 with dst_t);
 * mode 1: dst[r][c] = bf16(mean_{j < pool} src[r * pool + j][c]); mode 2: dst[r][c] = bf16(src[rows[r]][c]) (src fp32 or bf16 (., C),
 * C % 8 == 0). No scratch. */
int egx_wide_cast(int mode, const void* src, int src_bf16, const int* rows, int R, int C, int ld, int pool, void* dst, void* dst_t,
                  void* stream);

/* ---- ABI v26 additions (new symbols only, as v19 to v25: EGX_ABI_VERSION stays 18): the intermediates of a d = 128 call, stage by stage ---
 * Read-only test hooks of the per-clip (one launch, cut, sliced), tiled and ragged-training calls (egx_encoder_impl() == EGX_IMPL_FUSED /
 * EGX_IMPL_TILED, egx_ragged_train_fwd / egx_ragged_bwd): what the forward leaves in `saved` and the backward in `scratch`, one item at a
 * time, as a dense row-major matrix whose rows are the batch's tokens in token order (clip by clip; a ragged batch: its packed tokens).
 * tests/test_gpu_bf16_stages.py compares every stage of a bf16 call with a reference computed from the items the device itself held going
 * into that stage. No forward or backward launch changes; the hooks add one small launch of their own per read.
 *   item                 rows x cols      from                         what
 *   EGX_STAGE_PRE        N x d            saved                        projected features (+ bias, feature dropout) before the shared LayerNorm
 *   EGX_STAGE_XIN[l]     N x d            saved                        input of layer l
 *   EGX_STAGE_QKV[l]     N x 3d           saved                        Q | K | V rows with bias
 *   EGX_STAGE_RES1[l]    N x d            saved                        x + dropout(out-projection): the input of LayerNorm1
 *   EGX_STAGE_X1[l]      N x d            saved                        LayerNorm1 output as the FFN loop multiplies it: the bf16 plane, or the three
 *                                                                      f32s planes summed (exact); exact-fp32 calls (X1 and G2): EGX_STAGE_NOT_KEPT
 *   EGX_STAGE_HID[l]     N x d_ff         saved                        dropout(relu(.)) with the keep-scale, out of its MFMA-lane tiles (bf16 in bf16 calls)
 *   EGX_STAGE_ALIVE[l]   N x d_ff bytes   saved                        1 = ReLU active and kept by the dropout
 *   EGX_STAGE_RES2[l]    N x d            saved                        x1 + dropout(FFN output): the input of LayerNorm2
 *   EGX_STAGE_G2[l]      N x d            scratch                      gradient of the FFN output behind its dropout mask (planes like X1)
 *   EGX_STAGE_DHID[l]    N x d_ff         scratch                      gradient of the FFN pre-activation (tiles like HID)
 *   EGX_STAGE_G1[l]      N x d            scratch                      gradient of the out-projection output behind its dropout mask
 *   EGX_STAGE_ATTN_O[l]  N x d            scratch (tiled, ragged: saved)   attention output, the operand of the out-projection
 *   EGX_STAGE_DQKV[l]    N x 3d           scratch                      gradient of Q | K | V
 *   EGX_STAGE_DSEG[i]    rows_i x d       scratch                      gradient of segment i's projected features (`layer` = i; ragged: packed rows)
 *   EGX_STAGE_LSE[l]     4 N x 1          saved, tiled and ragged only log-sum-exp rows of the scaled scores, (clip, head, token of the clip)
 *   EGX_STAGE_DX0        -                -                            UNSUPPORTED: written only when a learned positional table wants a gradient, which
 *                                                                      the hook is not told; it answers EGX_STAGE_NOT_KEPT whatever the call did
 * The scratch items are valid from the return of the backward until the next call that uses the same scratch. head_n_out: the pooled head's
 * outputs (egx_translator_*; egx_config.token_ce: its classes; else 0): the scratch plan depends on it. `kind` (info): EGX_STAGE_KIND_F32,
 * _BF16 (bf16 values, widened exactly to fp32), _BIT (one byte per element, 0 / 1). Return value: 0, 1 (an error: egx_last_error) or
 * EGX_STAGE_NOT_KEPT: the item does not exist when this configuration's call returns (other implementations, LSE of a per-clip call, DX0). */
enum { EGX_STAGE_PRE = 0, EGX_STAGE_XIN = 1, EGX_STAGE_QKV = 2, EGX_STAGE_RES1 = 3, EGX_STAGE_X1 = 4, EGX_STAGE_HID = 5, EGX_STAGE_ALIVE = 6,
       EGX_STAGE_RES2 = 7, EGX_STAGE_G2 = 8, EGX_STAGE_DHID = 9, EGX_STAGE_G1 = 10, EGX_STAGE_ATTN_O = 11, EGX_STAGE_DQKV = 12, EGX_STAGE_DSEG = 13,
       EGX_STAGE_DX0 = 14, EGX_STAGE_LSE = 15, EGX_STAGE_ITEMS = 16 };
enum { EGX_STAGE_KIND_F32 = 0, EGX_STAGE_KIND_BF16 = 1, EGX_STAGE_KIND_BIT = 2 };
#define EGX_STAGE_NOT_KEPT 2
int egx_encoder_stage_info(const egx_config* cfg, const egx_segment* segs, int B, int head_n_out, int item, int layer, int* rows, int* cols,
                           int* kind);
int egx_encoder_stage_read(const egx_config* cfg, const egx_segment* segs, int B, int head_n_out, const void* saved, const void* scratch,
                           int item, int layer, void* out, void* stream);
/* The same for a ragged training batch; lengths: the host (B, K) frame counts of egx_ragged_train_fwd. */
int egx_ragged_stage_info(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int head_n_out, int item, int layer,
                          int* rows, int* cols, int* kind);
int egx_ragged_stage_read(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int head_n_out, const void* saved,
                          const void* scratch, int item, int layer, void* out, void* stream);

/* ---- ABI v27 additions (new symbols only, as v19 to v26: EGX_ABI_VERSION stays 18): the encoder's self-attention weights as an output -----
 * The head-averaged self-attention weights of the translators' nn.TransformerEncoder layers: which auxiliary task's tokens, at which time
 * steps, every token reads (the interpretability claim of the translator design). The reference's nn.TransformerEncoderLayer calls
 * self_attn(..., need_weights=False) (torch/nn/modules/transformer.py _sa_block), so there a user patches the layer; here the weights are
 * recomputed from the Q | K | V rows every forward keeps in `saved`, by one launch per layer behind the forward. No forward launch changes.
 *   w[b, i, j]   = (1 / H) sum_h softmax_j(q[b, i, h, :] . k[b, j, h, :] / sqrt(dh))      i, j < S_b
 *   seg[b, i, t] = sum_{j in segment t of clip b} w[b, i, j]                                 t < K
 * Scores, max, exp, sum and normalisation in fp32; products exact (v_mfma_f32_16x16x4_f32; bf16 operands are widened first); heads added in
 * head order, then one multiplication by 1 / H; segment sums in key order; no atomics: a clip's rows do not depend on its place in the batch.
 *
 * egx_self_attention_weights: the primitive, on the caller's tensors (fp32, or bf16 with operands_bf16), addressed as in
 * egx_cross_attention_weights: row pointer + row stride in elements (>= H * dh, a multiple of 8; q and k 16-byte aligned), head h at columns
 * [h * dh, (h + 1) * dh). rowtab: DEVICE int[B][2] = (first row, S_b) of clip b in q and k alike (NULL: rows b * S, S_b = S); S_b is
 * clamped to 0 .. S; S_b = 0 is an empty slot (zeros written, nothing read). segtab: DEVICE int[B][K] segment lengths of every clip
 * (K <= 16; needed with seg_out). dh in {16, 32, 64, 96, 128}, 1 <= S <= 512. w_out: row b * S + i at w_out + (b * S + i) * ldw, S entries
 * written (entries j >= S_b and rows i >= S_b are exact zeros), ldw >= S; seg_out (B, S, K). Either output may be NULL (not both): seg_out
 * alone never writes w to memory. A workgroup owns 16 query rows of a clip, so a clip's K rows are read once per 16 query rows.
 *
 * egx_attention_rollout: R_l = ((w_l + I) / 2) R_{l-1}, R_0 = I (Abnar & Zuidema 2020) per clip over w (L, B, S, S) fp32, each product an
 * fp32 fma chain in ascending k; L = 1 gives exactly (w_1 + I) / 2. rowlen: DEVICE int[B] tokens per clip (NULL: S), zeros beyond them.
 * scratch: egx_attention_rollout_scratch(L, B, S) bytes (two (B, S, S) buffers the products ping-pong between; the last one goes straight
 * to `out`). out (B, S, S) and / or seg_out (B, S, K), the per-task sums of the rollout through the same segment sums.
 *
 * egx_encoder_self_weights: right behind a forward of the same configuration on the same stream (egx_encoder_fwd, egx_translator_fwd;
 * with `lengths`, HOST (B, K) frame counts: egx_ragged_train_fwd with training = 0), from that call's `saved`. Layer l's Q | K are found at
 * the producers' own offsets (the 48-row tile grid of the d = 128 kernels, fp32; N x 3d bf16 of the wide path; N x 3d fp32 of the generic
 * path); a ragged call's batch table is read in place from `saved`. layer_mask: bit l selects layer l; the L' selected layers are written
 * in layer order to w_out (L', B, S, S) and seg_out (L', B, S, K) (either may be NULL), K = n_segments, S = the (longest) clip's tokens, one
 * launch per selected layer. head_n_out: as in the stage hooks (the offsets in `saved` do not depend on it).
 * All three are asynchronous and capturable. Refused before any device work (egx_last_error): null pointers, dh outside the set, S outside
 * 1 .. 512, strides below H * dh or not a multiple of 8 elements, q or k not 16-byte aligned, ldw < S, p_drop / p_pos / p_feat > 0 (the
 * reference's train-mode weights are post-dropout and not modelled), a configuration whose forward keeps no Q | K | V (no layers).
 * OUT OF SCOPE here, refused likewise: the pre-LN simple_vit encoder (composed from unit operators, no `saved` of this layout), the head
 * dims 256 / 512 of the d = 2048 recipe, ragged batches on the wide path (egx_ragged_encode*), and the capacity form with device lengths
 * (egx_ragged_cap_*: `lengths` here is a host array). */
int egx_self_attention_weights(const void* q, int ldq, const void* k, int ldk, int operands_bf16, const int* rowtab /* DEVICE int[B][2] or NULL */,
                               const int* segtab /* DEVICE int[B][K] or NULL */, int K, int B, int H, int dh, int S, float* w_out, int ldw,
                               float* seg_out, void* stream);
size_t egx_attention_rollout_scratch(int L, int B, int S);
int egx_attention_rollout(const float* w /* (L, B, S, S) */, int L, int B, int S, const int* rowlen /* DEVICE int[B] or NULL */,
                          const int* segtab /* DEVICE int[B][K] or NULL */, int K, void* scratch, float* out, float* seg_out, void* stream);
int egx_encoder_self_weights(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths /* HOST (B, K) or NULL */, int head_n_out,
                             const void* saved, uint64_t layer_mask, float* w_out /* (L', B, S, S) or NULL */,
                             float* seg_out /* (L', B, S, K) or NULL */, void* stream);

/* Fused FFN weight gradients (d_model = 128): dW1 += dH^T x1, db1 += colsum(dH), dW2 += g^T H where
 * H = dropout(relu(x1 W1^T + b1)) and dH = (g W2) .* mask are recomputed on chip. x1, g: (N, 128); S = tokens per
 * clip (dropout keying). scratch: egx_ffn_dw_scratch() bytes. Replaces the autograd of linear1/ReLU/linear2 weight
 * gradients (torch.nn.TransformerEncoderLayer._ff_block). */
size_t egx_ffn_dw_scratch(int N, int d_ff, int compute);
int egx_ffn_dw(const float* x1, const float* g, const float* W1, const float* b1, const float* W2, int N, int S,
               int d_ff, float p_drop, uint64_t seed, float* dW1, float* db1, float* dW2, int compute,
               void* scratch, void* stream);
/* *seed = lcg(*seed) on the stream (one tiny kernel): the per-step dropout seed of a replayed hipGraph. */
int egx_seed_advance(uint64_t* seed, void* stream);

/* ---- training step around the translator ------------------------------------------------
 * loss = sum_i w[y_i] * nll_i / sum_i w[y_i] with nll_i = -log_softmax(logits_i)[y_i]  (weight NULL: w = 1), and
 * d_logits = d loss / d logits when d_logits != NULL - in one launch. logits (B, C) fp32, target (B) int64, weight (C).
 * Replaces nn.CrossEntropyLoss(weight=[0.266, 0.734]) and its backward, HHI/tasks/ttm/video_task_2loader.py:21-22,34. */
int egx_weighted_ce(const float* logits, const int64_t* target, const float* weight, int B, int C, float* loss,
                    float* d_logits, void* stream);
/* Classifier head of the ASD task in one launch each way: logits = x W^T + b; loss = weighted CE(logits, target) as above;
 * probs = softmax(logits) (optional), pred_label = round(probs[:, 1]) (M, optional), *correct = number of rows with
 * pred_label == target (optional), d_logits = d loss / d logits (optional). x (M, K) fp32, W (C, K), b (C) or NULL, C <= 8, K a multiple of 64. Replaces lossAV.forward,
 * HHI/tasks/asd/loss.py:11-30 (nn.Linear(dim, 2) + nn.CrossEntropyLoss(weight=[1, 4]) + softmax / round / count), whose
 * separate launches cost 15 % of the ASD translator step. `scratch`: egx_linear_ce_scratch(M, K, C) bytes, ZERO before the
 * first use (arrival counters; every launch leaves them zero again). Sums run in a fixed order (deterministic).
 * Backward: dx = g * d_logits W (optional), dW = g * d_logits^T x, db = g * colsum(d_logits) (db optional), g = *grad_scale
 * (device scalar, NULL = 1). K in {64, 128, 256}. */
size_t egx_linear_ce_scratch(int M, int K, int C);
int egx_linear_ce_fwd(const float* x, const float* W, const float* b, const int64_t* target, const float* weight, int M, int K,
                      int C, float* logits, float* probs, float* d_logits, float* loss, float* correct, float* pred_label,
                      void* scratch, void* stream);
int egx_linear_ce_bwd(const float* x, const float* W, const float* d_logits, const float* grad_scale, int M, int K, int C,
                      float* dx, float* dW, float* db, void* scratch, void* stream);
/* *counter += inc on the stream (device-resident step count of the optimizer). */
int egx_counter_add(int64_t* counter, int64_t inc, void* stream);
/* One Adam (decoupled = 0) / AdamW (decoupled = 1) update of n fp32 elements with torch.optim semantics:
 *   g = grad * grad_scale (+ weight_decay * p if !decoupled);  p *= 1 - lr * weight_decay if decoupled;
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * with t = *step (1-based, device memory: advance it with egx_counter_add first, which also makes the update
 * replayable inside a hipGraph). Replaces torch.optim.Adam(lr=5e-4) HHI/tasks/ttm/video_task_2loader.py:62-64 and
 * AdamW(lr=1e-4, weight_decay=1e-4) HOI/tasks/multitask/video_task.py:624-626 over a flat parameter buffer. */
int egx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const int64_t* step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                  void* stream);
/* ---- ABI v18, additions: per-step learning-rate schedules and SGD for the captured step ---------------------------
 * The reference schedules the learning rate per optimizer step ("interval": "step",
 * HOI/optimizers/lta/lr_scheduler.py:11-41 lr_factory; HOI/tasks/pnr/video_task.py:74-95,
 * HOI/tasks/multitask/video_task.py:265-287). A learning rate passed by value is baked into a captured hipGraph, so
 * the schedule is evaluated on the device from the step count instead. f(k), k = 0, 1, ... the 0-based update index:
 *   EGX_LR_CONSTANT          1                                                        (LambdaLR(lambda x: 1), :19-20)
 *   EGX_LR_COSINE_ANNEALING  0.5 (1 + cos(pi k / T_max))                              (CosineAnnealingLR, eta_min 0, :15-18)
 *   EGX_LR_WARMUP_COSINE     k / max(1, warmup_steps) while k < warmup_steps, then
 *                            max(0, 0.5 (1 + cos(pi cycles 2 (k - warmup_steps) / max(1, t_total - warmup_steps))))
 *                            (WarmupCosineSchedule.lr_lambda, :82-91; not clamped beyond t_total: the reference's rises again)
 *   EGX_LR_WARMUP_LINEAR     the same warm-up, then max(0, (t_total - k) / max(1, t_total - warmup_steps))
 *                            (WarmupLinearSchedule.lr_lambda, :57-64)
 *   EGX_LR_TABLE             factors[min(k, n - 1)], fp64 in device memory: any LambdaLR (get_epoch_lr policies, :35-38) */
enum { EGX_LR_CONSTANT = 0, EGX_LR_COSINE_ANNEALING = 1, EGX_LR_WARMUP_COSINE = 2, EGX_LR_WARMUP_LINEAR = 3, EGX_LR_TABLE = 4 };
#define EGX_LR_MAX_GROUPS 16
typedef struct egx_lr_schedule {
    int kind;              /* EGX_LR_* */
    int64_t warmup_steps;  /* warm-up kinds: >= 0 */
    int64_t t_total;       /* warm-up kinds: >= 0 */
    int64_t T_max;         /* cosine annealing: >= 1 */
    double cycles;         /* warm-up cosine: the reference's default is 0.5 */
    const double* factors; /* table: n factors, device memory */
    int64_t n;             /* table: >= 1 */
} egx_lr_schedule;
/* One single-thread launch: *step += 1 (the work of egx_counter_add), k = *step - 1, lr_out[g] = (float)(base_lr[g] * f(k))
 * for g < n_groups (1 .. EGX_LR_MAX_GROUPS); f in fp64. step and lr_out are device memory, base_lr is host memory and
 * is copied into the launch (a captured graph keeps the values it was captured with). */
int egx_lr_update(const egx_lr_schedule* schedule, int64_t* step, const double* base_lr, int n_groups, float* lr_out,
                  void* stream);
/* egx_adam_step with the learning rate read from device memory (*lr, as egx_lr_update left it): the same arithmetic. */
int egx_adam_step_dev_lr(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const int64_t* step,
                         const float* lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                         float grad_scale, void* stream);
/* One torch.optim.SGD update of n fp32 elements:
 *   g = grad * grad_scale + weight_decay * p;
 *   momentum > 0:  buf = g on the optimizer's first update (*step == 1: an assignment, buf's contents are not read),
 *                  else buf = momentum * buf + (1 - dampening) * g;   g = nesterov ? g + momentum * buf : buf;
 *   p -= lr * g    with lr = *lr_dev, or `lr` when lr_dev == NULL.
 * momentum == 0 takes momentum_buf == NULL (and step may be NULL); Nesterov needs momentum > 0 and dampening == 0.
 * Replaces torch.optim.SGD as HOI/optimizers/lta/optimizer.py:54-62 builds it (HOI/configs/recognition/ts_ar.yaml:39-45:
 * momentum 0.9, weight decay 1e-4; Nesterov and dampening 0 by HOI/configs/recognition/defaults.py:467-476). */
int egx_sgd_step(float* param, const float* grad, float* momentum_buf, size_t n, const int64_t* step, const float* lr_dev,
                 float lr, float momentum, float dampening, float weight_decay, int nesterov, float grad_scale,
                 void* stream);
/* ---- ABI v28 additions (new symbols only, as v19 to v27: EGX_ABI_VERSION stays 18): gradient-norm clipping and a non-finite guard for the
 * captured step ------------------------------------------------------------------------------------------------------------------------
 * A replayed hipGraph cannot test torch.isfinite(loss) or call clip_grad_norm_ on the host: the norm, the decision and the launches that obey
 * it all have to be device work. What Lightning's Trainer offers as gradient_clip_val / track_grad_norm (the reference constructs its Trainer
 * with the defaults, HHI/scripts/run_ttm.py:21, HOI/scripts/lta/run_lta.py:238) is here, over the G flat fp32 gradient buffers (g_i, n_i) of
 * one optimizer step:
 *   sqsum  = sum_i sum_j (double)g_i[j]^2   each square exact in fp64, every sum in fp64 in a FIXED order that is a function of (n_i) alone
 *                                           (not of timing, not of a buffer's alignment): no atomics on floating-point values, so ranks that
 *                                           hold the same gradient bits after the exchange take the same decision without a collective
 *   norm   = sqrt(sqsum)                    kept in fp64 (a gradient of all 3e38 has a norm above FLT_MAX and is finite)
 *   finite = isfinite(sqsum)                exactly when every element is finite: a finite fp32 cannot overflow the fp64 sum of squares
 *   coef   = c < 1 ? (float)c : 1.0f        c = max_norm / (norm + 1e-6) in fp64, the formula of torch.nn.utils.clip_grad_norm_; a comparison,
 *                                           so a NaN norm gives 1; 1.0f without a max_norm
 *   apply  = finite || !skip_nonfinite
 * The guard block lives in device memory; egx_grad_norm rewrites norm / coef / apply on every call or replay and advances the counters:
 * steps += 1, skipped += !apply, clipped += apply && coef < 1. Zero-fill it once before the first call.
 * The gated and guarded twins below read it: with apply == 0 they return before any store, so NOTHING the optimizer owns changes (parameters,
 * moments, momentum buffer, step count, learning rates: the schedule index is the number of APPLIED updates); with apply == 1 they are
 * today's launches with grad_scale = coef read from device memory, bit for bit the unguarded step when coef == 1.0f. */
typedef struct egx_guard_block {
    double norm;     /* sqrt(sqsum), fp64 */
    float coef;      /* the factor on every gradient element */
    int32_t apply;   /* 0: the step is skipped */
    int64_t steps;   /* calls of egx_grad_norm on this block */
    int64_t skipped; /* ... of which apply == 0 */
    int64_t clipped; /* ... of which apply == 1 and coef < 1 */
} egx_guard_block;
typedef struct egx_grad_norm_cfg {
    double max_norm;    /* >= 0 (not NaN); read only with has_max_norm */
    int has_max_norm;   /* 0: measure and guard, never clip */
    int skip_nonfinite; /* 0: apply = 1 always (the norm and the counters are still written) */
} egx_grad_norm_cfg;
#define EGX_GRAD_NORM_TABLE 32
/* Launch 1, grad_sqsum_kernel: one grouped launch per EGX_GRAD_NORM_TABLE buffers (a by-value table; more buffers chain further launches
 * into later ranges of the partials), at most 2048 workgroups each, split among the buffers in proportion to their sizes and grid-striding
 * over the rest; 16-byte loads where a buffer is 16-byte aligned, 4-byte loads of the same elements by the same threads otherwise; every
 * thread keeps fp64 accumulators, a fixed wave and workgroup tree follows, and each workgroup writes ONE fp64 partial to its own slot of
 * `scratch` with a plain store. Launch 2, guard_finish_kernel: one workgroup adds the partials in index order, takes the decision above and
 * writes the block. Two launches and no last-arriver ticket: nothing spins. bufs and ns are HOST arrays of n_bufs >= 1 device pointers and
 * element counts; n_i == 0 is legal (that buffer is not read, its pointer may be NULL). scratch: egx_grad_norm_scratch_bytes(ns, n_bufs)
 * bytes of device memory, no initialisation needed (0 from the query: an argument was refused). Asynchronous and capturable; max_norm is
 * copied into the launch (a captured graph keeps the value it was captured with). Refused before any device work (egx_last_error): null
 * pointers, n_bufs < 1, a scratch smaller than the query's answer, max_norm < 0 or NaN, a buffer that is not 4-byte aligned. */
size_t egx_grad_norm_scratch_bytes(const size_t* ns, int n_bufs);
int egx_grad_norm(const float* const* bufs, const size_t* ns, int n_bufs, void* scratch, size_t scratch_bytes, const egx_grad_norm_cfg* cfg,
                  egx_guard_block* guard, void* stream);
/* egx_counter_add and egx_lr_update behind a guard: no store when guard->apply == 0 (same closed forms, one device function). */
int egx_counter_add_gated(int64_t* counter, int64_t inc, const egx_guard_block* guard, void* stream);
int egx_lr_update_gated(const egx_lr_schedule* schedule, int64_t* step, const double* base_lr, int n_groups, float* lr_out,
                        const egx_guard_block* guard, void* stream);
/* egx_adam_step / egx_adam_step_dev_lr and egx_sgd_step behind a guard: grad_scale = guard->coef, no store when guard->apply == 0; the
 * learning rate is *lr_dev, or `lr` when lr_dev == NULL. The same update text as the unguarded kernels, which stay as they are. */
int egx_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const int64_t* step,
                          const float* lr_dev, float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                          const egx_guard_block* guard, void* stream);
int egx_sgd_step_guarded(float* param, const float* grad, float* momentum_buf, size_t n, const int64_t* step, const float* lr_dev,
                         float lr, float momentum, float dampening, float weight_decay, int nesterov, const egx_guard_block* guard,
                         void* stream);
/* ---- ABI v18, additions: the criterion of the long-term-anticipation task in one launch ---------------------------
 * LongTermAnticipationTask.training_step, HOI/tasks/lta/long_term_anticipation.py:182-203: on the model's [(B, Z, 115), (B, Z, 478)]
 * output it sums CrossEntropyLoss(mean)(pred_h[:, z], labels[:, z, h]) over the 2 heads and 20 future steps (40 terms) and reads
 * the top-1 / top-5 error of every (z, h) pair with .item() (evaluation/lta/lta_metrics.py:38-84). Here:
 *   logits   fp32, R = B * Z rows (row b * Z + z) of row stride `ld` floats: the (B, Z, 593) stack the translator's decode() builds.
 *            Rows need NO alignment (ld = 593 is odd). H heads (1 .. 4); head h owns columns [col0[h], col0[h] + C[h]) of every
 *            row, 1 <= C[h] <= 2048; heads are disjoint, lie inside [0, ld) and need not cover the row. col0, C, ks: HOST arrays.
 *   target   int64 (B, Z, H), contiguous. A label outside [0, C[h]) - the default ignore index -100 included - contributes no
 *            loss, no count and no gradient (the rule of egx_weighted_ce).
 *   ks       n_ks <= 4 values, each in 1 .. min_h C[h].
 *   loss       = sum_{z,h} ( sum_{b valid} nll[b,z,h] ) / n_valid[z,h]                       (scalar)
 *   loss_terms (Z, H), optional: the terms of that sum
 *   n_valid    (Z, H) int32: clips with a valid label
 *   correct    (n_ks, Z, H) int32 (NULL allowed when n_ks == 0): valid rows whose label has rank < k, where
 *              rank = #{c : z_c > z_y} + #{c < y : z_c == z_y}
 *   d_logits   (R, ld), optional, EVERY element written: (softmax - onehot) / n_valid[z,h] on the valid rows of a head; 0 on
 *              invalid rows and on columns no head covers (egx_linear_bwd of the stacked head reads whole rows).
 * Two deliberate differences from torch: (1) a (z, h) pair WITHOUT a valid label adds 0 to the loss and has zero gradient, where
 * nn.CrossEntropyLoss gives nan (0 / 0); (2) torch.topk leaves the order of equal logits unspecified - the rank rule above is this
 * library's: among equal logits the lower class index ranks first, so a row of all-equal logits is top-k correct iff y < k.
 * The softmax is max-subtracted (a row holding +80 and -80 does not overflow). One launch on `stream`; every sum runs in a fixed order
 * (per-workgroup partials in scratch, added by the last workgroup to arrive): the same bits on every run, no float atomics.
 * `scratch`: egx_segmented_ce_scratch(B, Z, H, n_ks) bytes (0: invalid arguments, see egx_last_error), ZERO before the first use
 * (it begins with 64 * (1 + Z) bytes of arrival counters; every launch leaves them zero again - so a buffer serves launches of ONE Z:
 * zero it again before a launch with another Z, whose counters lie where this one's partial sums were). Refused on the host, before any device work, with a message that names
 * the limit: null pointers; B, Z < 1 or B * Z > 2^28; H, n_ks, C[h], ks[k] or ld out of range; a head outside the row; overlapping heads. */
size_t egx_segmented_ce_scratch(int B, int Z, int H, int n_ks);
int egx_segmented_ce(const float* logits, int ld, const int64_t* target, int B, int Z, int H, const int* col0, const int* C,
                     const int* ks, int n_ks, float* loss, float* loss_terms, int* n_valid, int* correct, float* d_logits,
                     void* scratch, void* stream);
/* ---- ABI v19 (additions over v18: new symbols only, no existing signature changes, so EGX_ABI_VERSION - which a binding compares
 * for equality - stays 18): the validation step of the long-term-anticipation task in one launch -------------------------
 * LongTermAnticipationTask.validation_step, HOI/tasks/lta/long_term_anticipation.py:222-248 (and :313-341 for the sequence tasks):
 * model.generate(input, k = K) - Categorical(logits = head).sample() K times per head, argmax at K = 1,
 * HOI/models/lta/lta_models_lta_transfer.py generate() - then a permute, one .cpu() per head and AUED
 * (HOI/evaluation/lta/lta_metrics.py:86-114), a Python loop of editdistance.eval over every clip, prefix length and sequence. Here:
 *   logits   fp32, R = B * Z rows (row b * Z + z) of row stride `ld`, H heads as column windows col0[h], C[h] (HOST arrays): the layout
 *            and the rules of egx_segmented_ce (1 <= C[h] <= 2048, H <= 4, disjoint, rows unaligned). NULL allowed with preds_in.
 *   labels   int64 (B, Z, H), contiguous. NULL: no metric (min_dist and dist_sum must then be NULL too).
 *   K        1 .. 8 sequences per clip and head; Z <= 64 future steps; B * Z <= 2^28.
 *   seed     by value; with seed_ptr (device address of a uint64, as egx_config.seed_ptr) the word is read on the stream instead, so
 *            replays of a captured graph draw fresh sequences when egx_seed_advance follows the call in the graph. K > 1 with a host
 *            seed is refused inside a stream capture (every replay would repeat the draws), as the dropout seed is.
 *   preds_in optional int64 (H, B, K, Z): the metric-only entry. Sampling is skipped, the metric is computed on these tokens and
 *            `preds` (NULL allowed here) receives a copy.
 * Outputs, every element written by every call:
 *   preds    int64 (H, B, K, Z); slice h is the (B, K, Z) tensor generate() returns for head h.
 *            K = 1: the row argmax, the lowest index among equal logits.
 *            K > 1: draw k of row r = b * Z + z of head h is the class j with cdf[j - 1] <= u < cdf[j], where cdf is the running sum of
 *            the max-subtracted softmax of the head's window and u = (w + 0.5) / 2^32 with w the 32-bit word k of the row from the
 *            library's counter generator (csrc/common.h): key = site_key(seed, layer = 0x17A, site = h); (x, y) = rand_quad(key, r, k >> 1);
 *            w = x for even k, y for odd k. The K draws of a row are independent (K words), like K .sample() calls. A class with a -inf
 *            logit has probability 0 and is never drawn. The cdf is accumulated in blocks (64 contiguous chunks of <= 32 classes, chunk
 *            totals added in order: chains of <= 32 + 64 additions), is exactly non-decreasing, and the comparison u * cdf[C - 1] against
 *            the unnormalised cdf runs in fp64; against an fp64 softmax the cdf is within 1e-5 (tests/lta_val_ref.py check_draws).
 *   min_dist int32 (B, Z, H), optional: min over k of Lev(preds[h, b, k, :z + 1], labels[b, :z + 1, h]), the plain Levenshtein distance
 *            (insert, delete, substitute; integer equality, no ignore index) - what the editdistance package computes. All Z prefixes
 *            of a sequence are the diagonal of one table.
 *   dist_sum int64 (Z, H), optional: sum of min_dist over b (a memset node + 64-bit integer atomics: the same bits on every run).
 *            ED_z of the reference = dist_sum[z, h] / (B * (z + 1)); across ranks, all-reduce dist_sum and B.
 * Two deliberate differences from the reference: (1) a row that holds a NaN or +inf, or has no finite logit, yields token -1 for every
 * draw (Categorical raises), and a negative token - handed in through preds_in too - equals no label; (2) ties at K = 1 go to the
 * lowest index (torch.argmax leaves them open).
 * One launch on `stream` plus at most one memset node; no allocation, no scratch, capturable. Refused on the host, before any device
 * work, with a message that names the limit: null pointers (logits and preds_in both NULL included); B, Z, K, H, C[h] or ld out of
 * range; B * Z > 2^28; a head outside the row; overlapping heads. */
int egx_lta_validate(const float* logits, int ld, const int64_t* labels, int B, int Z, int H, const int* col0, const int* C, int K,
                     uint64_t seed, const uint64_t* seed_ptr, const int64_t* preds_in, int64_t* preds, int* min_dist,
                     int64_t* dist_sum, void* stream);
/* ---- ABI v20 additions (new symbols only, as v19: EGX_ABI_VERSION stays 18): the criterion and the metrics of the PNR keyframe task
 * in one launch -------------------------------------------------------------------------------------------------------------------
 * KeyframeLocalisation2Loader.training_step, HOI/tasks/pnr/video_taskspecific_pnr.py:24-63 (also keyframe_detection.py:23-70; recipe
 * HOI/configs/pnr/ts_pnr.yaml: LOSS_FUNC "bce", LOSS_REDUCTION "mean"): BCELoss(sigmoid(preds.squeeze(1)), labels.float()) - or, under
 * LOSS_FUNC cross_entropy, mean(state_change_label.T * CE(preds, argmax(labels))) - then keyframe_distance and keyframe_accuracy
 * (HOI/evaluation/pnr/metrics.py:23-80), two Python loops over the clips with four to six .item() reads per clip. The EgoT2-g HOI
 * validation runs the same arithmetic on decoder logits (PnrOsccMetric.pnr_distance / oscc_acc, metrics.py:102-134, called at
 * HOI/tasks/multitask/video_task.py:67,80): the argmax restricted to the vocabulary columns of '0'..'15' (or 'False' / 'True') and the
 * share of rows whose unrestricted argmax falls outside that set. Here:
 *   logits   fp32, B rows of row stride `ld` floats; rows need NO alignment. Frame t of row b is column cols[t] when `cols` (a HOST
 *            int[T], copied into the launch; distinct entries in [0, V)) is given, else column t. 1 <= T <= 64 (the recipe: 16).
 *            V = the meaningful columns of a row, T <= V <= ld, V <= 2048; without cols V == T. 1 <= B <= 2^28.
 *   kind     EGX_KF_BCE needs target; EGX_KF_CE needs target or label; EGX_KF_METRIC takes no loss (loss, loss_rows, d_logits NULL).
 *   target   fp32 (B, T) contiguous, values in [0, 1]: the one-hot labels.float() of the reference; soft values are allowed.
 *   label    int64 (B): the label frame as an index. NULL: the label frame is argmax_t target (first maximum). Both NULL: no accuracy
 *            is counted (n_correct = 0). A label outside [0, T) equals no prediction and, under CE, adds no loss and no gradient.
 *   state_change  int64 (B), or NULL = every clip counts. Compared == 1, as `sc_label.item() == 1` is.
 *   fps (fp64), clip_start, clip_end, pnr_frame (int64), each (B): all four, or none (then dist and dist_sum must be NULL).
 * Outputs, every element written by every call:
 *   loss       BCE: mean over B * T of min(softplus(-x), 100) * y + min(softplus(x), 100) * (1 - y).
 *              CE: (1 / B) sum_b [sc_b == 1] nll_b, nll_b the max-subtracted log-softmax CE over the T frames against the label frame:
 *              divided by B, NOT by the number of state-change clips, as torch.mean(state_change_label.T * loss) does.
 *              loss = (sum_b loss_rows[b]) / B under both kinds.
 *   loss_rows  (B), optional. BCE: the row's sum / T. CE: the masked nll_b.
 *   d_logits   (B, ld), optional, EVERY element written: d loss / d logits. BCE: (sigmoid(x) - y) / (B * T) (the clamp at 100, reached
 *              beyond |x| = 100, is not differentiated). CE: [sc_b == 1] (softmax - onehot) / B. Columns that are no frame: 0.
 *   pred       (B) int32: argmax over the T frames with torch.argmax's rule: the first NaN if the row holds one, otherwise the lowest
 *              index among equal maxima.
 *   label_frame (B) int32, optional: the label frame, -1 where there is none.
 *   counts     int32[4]: n_sc (clips with state_change == 1), n_correct (of those, pred == label frame), n_outside (rows whose argmax
 *              over all V columns is not one of cols; 0 without cols), B.
 *   dist       (B) fp64, optional: |((clip_end - clip_start) / T) * pred - (pnr_frame - clip_start)| / fps for a state-change clip,
 *              evaluated in fp64 in exactly that order; 0 for the other clips. The reference's literal 16 is T; its fp32 rounding of the
 *              first product is exact for every real clip (T = 16, spans below 2^20 frames), so on the recipe shape this is the
 *              reference's number bit for bit.
 *   dist_sum   fp64 scalar, optional: the sum of dist in a fixed order. keyframe_distance = dist_sum / n_sc, or 0.0 when n_sc == 0 (the
 *              reference returns np.mean(0.0)). Across ranks: all-reduce counts and dist_sum.
 * Two deliberate differences from torch: (1) the loss is evaluated in LOGIT form. BCELoss(sigmoid(x)) in fp32 rounds sigmoid to 1 for x
 * above about 16.6 and returns its clamp of 100 with a zero gradient; this library returns the true softplus (clamped at 100) and the
 * true gradient sigmoid - y. The two agree wherever fp32 sigmoid has not saturated. (2) pseudo_acc = n_correct / n_sc without a
 * state-change clip is NaN here; the reference divides by zero.
 * One launch on `stream`: a wave per clip, a lane per frame; no allocation, capturable. The clips are cut into at most 64 chunks, a
 * workgroup of four waves each (a lane of the last workgroup adds one chunk): up to B = 256 every clip has a wave of its own, beyond that
 * a wave walks ceil(B / 64) / 4 clips in turn, so the launch is sized for training batches, not for B near the 2^28 limit. Every sum runs in a fixed order (per-workgroup
 * partials in scratch, added by the last workgroup to arrive): the same bits on every run, no float atomics.
 * `scratch`: egx_keyframe_scratch(B) bytes (0: invalid B, see egx_last_error; the same size for every valid B), ZERO before the first
 * use; it begins with a 64-byte arrival counter that every launch leaves zero, so one buffer serves launches of every shape.
 * Refused on the host, before any device work, with a message that names the limit: null logits, pred, counts or scratch; B < 1 or
 * B > 2^28; T, V or ld out of range; a cols entry outside [0, V) or a duplicate (so the kernel never reads outside a row); a kind
 * whose inputs are missing; a loss output with EGX_KF_METRIC; only some of the four timing arrays; dist or dist_sum without them. */
enum { EGX_KF_BCE = 0, EGX_KF_CE = 1, EGX_KF_METRIC = 2 };
size_t egx_keyframe_scratch(int B);
int egx_keyframe_criterion(const float* logits, int ld, int B, int T, const int* cols, int V, int kind, const float* target,
                           const int64_t* label, const int64_t* state_change, const double* fps, const int64_t* clip_start,
                           const int64_t* clip_end, const int64_t* pnr_frame, float* loss, float* loss_rows, float* d_logits,
                           int* pred, int* label_frame, int* counts, double* dist, double* dist_sum, void* scratch, void* stream);
/* ---- ABI v21 additions (new symbols only, as v19 and v20: EGX_ABI_VERSION stays 18): the criterion and the metrics of an EgoT2-g
 * multi-task step in one launch ------------------------------------------------------------------------------------------------------
 * Unified3TaskTranslation.training_step (HHI/tasks/multitask/video_tasktranslation.py:39-66; accuracy :101-102) and
 * Unified6TaskTranslation.training_step / validation_step (HOI/tasks/multitask/video_task.py:537-577, :683-736):
 * loss = sum_t ratio_t * nn.CrossEntropyLoss()(logits_t (B, |V|, sy), target_t[:, 1:]) over the 3 (6) tasks of one vocabulary, every term
 * read with .item(); the validation step runs a second predict() forward per task for an argmax, and ARMetric / LTAMetric
 * (HOI/evaluation/lta/lta_metrics.py:164-211, 229-292), PNRMetric / OSCCMetric (HOI/evaluation/pnr/metrics.py:139-257) map it from the
 * vocabulary word to the task's original label in Python loops with .item() per clip. Here, for T tasks (1 .. 8; `tasks` is a HOST array,
 * copied into the launch) that share one vocabulary of V words (2 .. 2048):
 *   logits   fp32, element (b, s, c) at logits + b * stride_b + s * stride_s + c: the class axis is contiguous, the strides are in floats
 *            and rows need NO alignment. The (sy, B, V) decoder output is read in place through the (B, V, sy) view the models return
 *            (stride_b = V, stride_s = B * V), and equally a contiguous (B, sy, V) tensor. B >= 1, 1 <= sy <= 64, B * sy <= 2^22.
 *   target   int64, element (b, s) at target + b * target_stride_b + s * target_stride_s, so target[:, 1:] is read in place. A label
 *            outside [0, V) - the default ignore index -100 included - contributes no loss, no count and no gradient.
 *   ratio    the task's weight in the loss; may be 0 (the gradient is then exactly zero).
 *   d_logits optional, with the strides of logits (rows must not overlap: each stride >= V); EVERY row (b, s) is written:
 *            ratio / n_valid_t * (softmax - onehot) at a valid position, zeros at an ignored one.
 *   word_label  optional DEVICE int32[V]: the original label of a vocabulary word, or -1; goes together with
 *   labels   int64, element (b, s) at labels + b * labels_stride_b + s * labels_stride_s: the original label of the position, < 0 = the
 *            position is not scored.
 *   pred     optional int32 (B, sy, 2), contiguous (needs word_label): word_label[a] and word_label[r] of every position (-1 for r
 *            when no word is mapped), so the host can build PNRMetric.dist and the per-clip lists.
 * `result`: 1 + 8 T words of 4 bytes, every one written by every call:
 *   [0] loss = sum_t ratio_t * loss_terms[t], added for t = 0, 1, ... (fp32)
 *   loss_terms[T] fp32 = (sum of nll over the valid positions of task t) / n_valid[t]: nn.CrossEntropyLoss() on (B, V, sy) against (B, sy)
 *   n_valid[T], token_correct[T], seq_correct[T], scored[T], invalid[T], correct[T], correct_restricted[T]   (int32), where
 *   a = argmax over all V words, r = argmax over the words with word_label >= 0; among equal logits the lower index wins (the rank rule
 *   of egx_segmented_ce); token_correct = valid positions with a == target; seq_correct = rows b with at least one valid position and
 *   every valid position correct; over the scored positions invalid += word_label[a] < 0, correct += word_label[a] == label,
 *   correct_restricted += word_label[r] == label.
 * ARMetric / LTAMetric: (v_cnt, v_err, v_correct) = (scored, invalid, correct) of the verb task scored at position 0, nouns likewise;
 * OSCCMetric: (error, correct) = (invalid, correct_restricted) under {False: 0, True: 1}; PNRMetric.err = invalid under {'0'..'15': 0..15};
 * the HHI accuracy = correct_restricted under {'0': 0, '1': 1}. With the causal mask the position-0 logits of the teacher-forced forward
 * are those of predict(), so in eval mode the forward that gives the loss also gives the metrics.
 * One deliberate difference from torch: a task WITHOUT a valid label adds 0 to the loss and has zero gradient, where nn.CrossEntropyLoss
 * gives nan (0 / 0), as in egx_segmented_ce. The softmax is max-subtracted. One launch on `stream`: a wave per target row b walking its sy
 * positions; the rows of a task are cut into at most 256 chunks, a workgroup of four waves each. Every sum runs in a fixed order
 * (per-workgroup partials in scratch, added by the last workgroup to arrive): the same bits on every run, no float atomics.
 * `scratch`: egx_sequence_ce_scratch() bytes (one size for every T and shape), ZERO before the first use; it begins with nine 64-byte
 * arrival counters (the launch's and one per task, laid out for 8 tasks always) that every launch leaves zero, so one buffer serves
 * launches of every T and shape. Refused on the host, before any device work, with a message that names the limit: null tasks, result,
 * scratch, logits or target; T, V, B, sy or B * sy out of range; a negative stride; d_logits rows that overlap; labels without word_label
 * or the reverse; pred without word_label. */
typedef struct egx_seq_task {
    const float* logits; long long stride_b, stride_s;
    int B, sy;
    const int64_t* target; long long target_stride_b, target_stride_s;
    float ratio;
    float* d_logits;
    const int* word_label;
    const int64_t* labels; long long labels_stride_b, labels_stride_s;
    int* pred;
} egx_seq_task;
size_t egx_sequence_ce_scratch(void);
int egx_sequence_ce(const egx_seq_task* tasks, int T, int V, void* result, void* scratch, void* stream);
/* ---- ABI v22 additions (new symbols only, as v19 to v21: EGX_ABI_VERSION stays 18): the TTM / LAM validation epoch on the device -
 * a per-row score accumulator and the checkpoint metric val_mAP (HHI/tasks/ttm/video_task_2loader.py:19,46-50) -------------------------
 * Rows are segments (TTM) or frames (LAM). `scratch`: egx_segment_ap_scratch(capacity) bytes (0: capacity outside 1 .. 2^24, see
 * egx_last_error), 36 bytes per row of capacity plus at most 9 MiB of tile tables; it begins with the persistent per-row state (sum of the two logits,
 * window count, label) followed by the sort's work area. ZERO it to empty the accumulator; the same `capacity` goes into every call.
 *
 * egx_segment_scores_update replaces PostProcessor.update / _merge_output (HHI/utils/ttm/utils.py:57-80) and the LAM
 * PostProcessor.update (HHI/utils/lam/utils.py:34-47): the Python list of per-window outputs, torch.cat and one .item() per segment.
 *   logits   fp32, B windows of row stride `ld` >= 2 floats; columns 0 and 1 are the class logits.
 *   slots    int64 (B), DEVICE: the row of every window, NON-DECREASING within a call (the windows of a row are adjacent, as the
 *            reference's loader yields them); a row may continue from an earlier call. NULL: window i is row slot0 + i (LAM: one row per
 *            input row; slot0 + B <= capacity is checked on the host). A slot outside [0, capacity) is dropped.
 *   labels   int64 (B): a row takes the label of its FIRST window (utils.py:78); compared == 1, as label_groundtruth == 1 is.
 * One launch, a thread per window: the first window of a run of equal slots adds the run's logits, in window order, onto the row's stored
 * sum. The sum is one left fold per row and the stored score is bit-identical however a row's windows are split across calls; no atomics.
 *
 * egx_segment_ap replaces PostProcessor.save / get_mAP -> run_evaluation (utils.py:82-114; HHI/utils/ttm/metrics.py:26-71, 138-199,
 * 232-247): two CSV files per rank joined by `cat` in a subshell, a pandas merge and sort, and two Python loops over every row. Over rows
 * 0 .. N - 1 of the accumulator (1 <= N <= capacity):
 *   score    (N) fp32 = softmax(sum / count)[1], the mean and the max-subtracted softmax in fp32 as the reference computes them. A row
 *            whose score is not finite (a non-finite logit, or no window at all) holds the one NaN 0x7fc00000.
 *   order1   (N) int32: the rows by score descending; order0: by score ascending (the class-0 pass on 1 - score). Among equal scores the
 *            LOWER ROW COMES FIRST in both (the reference's pandas quicksort leaves the order of ties unspecified; and two scores that
 *            differ by less than 2^-53 of 1 tie in its 1 - score, where this orders them by their fp32 values). The NaN ranks above every
 *            number: first in order1, last in order0.
 *   result   88 bytes, every one written by every call: int64 n, n_pos, TP, FN, FP, TN, n_nonfinite, then fp64 AP0, AP1, mAP, acc.
 *            TP / FN / FP / TN at score >= 0.5 (metrics.py:232-238: exactly 0.5 is predicted positive; a NaN negative); acc = (TP + TN) / n.
 *            AP of a class (metrics.py:61-71, 138-166): tp_k = cumsum(label) in the class's order, precision tp_k / k, made non-increasing
 *            from the right, AP = sum over the positive rows of (tp_k / P - (tp_k - 1) / P) * precision_k; class 0 uses 1 - label.
 *            mAP = (AP0 + AP1) / 2. A class without a positive row has AP = NaN (the reference's 0 / 0), and with n_nonfinite > 0 both
 *            APs are NaN. Counts are integers; precisions are compared as exact rationals (tp_a k_b against tp_b k_a in 64 bits); the
 *            terms are fp64, added in a fixed order (per tile of 4096 rows, then the tiles in order): the same bits on every run.
 * NOT done here: the reference's uid handling (load_csv names fewer columns than the files hold, so its uid is start:end and
 * drop_duplicates merges segments of different videos with equal frame ranges): rows are the caller's slots and nothing is deduplicated.
 * Across ranks: all-gather the per-row state first. The test-set JSON writer stays on the host.
 * Launches on `stream`, none synchronises, their number depends on N only: a memset, the score kernel, then up to N = 4096 ONE workgroup
 * that runs the stable LSD radix sort (8-bit digits, ranks inside a wave by ballots) for both classes and both AP passes; beyond it
 * 3 launches per sort pass (tile histograms, a scan per digit in tile order, scatter), 4 passes per class - class 0 runs the passes again
 * on the plain digit where class 1 uses the complemented one, which keeps the tie rule without a tie-group pass - and 6 for the AP.
 * Refused on the host, before any device work, with a message that names the limit: a null pointer; capacity or N outside
 * 1 .. 2^24 (N also above capacity); ld < 2; B < 1; without slots, slot0 < 0 or slot0 + B > capacity. */
size_t egx_segment_ap_scratch(int capacity);
int egx_segment_scores_update(const float* logits, int ld, int B, const int64_t* slots, int slot0, const int64_t* labels, int capacity,
                              void* scratch, void* stream);
int egx_segment_ap(int N, int capacity, void* scratch, float* score, int* order1, int* order0, void* result, void* stream);
/* ---- ABI v23 additions (new symbols only, as v19 to v22: EGX_ABI_VERSION stays 18): the test epoch of the action-recognition translators
 * on the device - the multi-view ensemble per video and the top-k errors over the videos ---------------------------------------------------
 * MultiTaskClassificationTask.test_epoch_end (HOI/tasks/lta/long_term_anticipation.py:96-158; the same code in
 * long_term_anticipation_taskspecfic.py:100-162). A video is a slot 0 .. capacity - 1; the heads (H <= 4, C[h] <= 2048 classes) are packed
 * side by side in a state row of sum(C) floats.
 *
 * egx_view_ensemble_state -> the bytes of the state for `capacity` videos (0: refused, see egx_last_error): a 256-byte header (the
 * top-k launch's arrival counter, the dropped clips), the labels int64 (capacity, H), the view counts int32 (capacity), 24 KiB of count
 * partials and the rows fp32 (capacity, sum C). `offsets` (may be NULL): 3 words, the byte offsets of labels, view counts and rows.
 * ZERO the state to empty the accumulator (the reference's torch.zeros rows); the same capacity, H and C go into every call.
 *
 * egx_view_ensemble_update replaces the loop of :116-140 (three dicts of per-video tensors, one `+=` or torch.max launch per clip and head,
 * after a torch.cat of every clip of the epoch) for one batch of clips:
 *   preds    fp32, B clips of row stride `ld`; head h is columns [col0[h], col0[h] + C[h]) of a row.
 *   labels   int64 (B, H): a video takes the labels of its LAST clip (:118).
 *   slots    DEVICE, int32 (slot_bytes 4) or int64 (slot_bytes 8), (B): the video of every clip. The clips of a video need not be adjacent,
 *            may repeat within a batch and may be spread over calls. A slot outside [0, capacity) is dropped and counted. NULL: clip i is
 *            video slot0 + i (0 <= slot0, slot0 + B <= capacity is checked on the host).
 *   method   0 "sum": row = ((0 + x_1) + x_2) + ... in fp32, the clips in ARRIVAL order (row order within a call, call order across calls);
 *            1 "max": row = max(0, x_1, x_2, ...) - the running value starts from the reference's torch.zeros, so a video whose logits are
 *            all negative ends as a row of zeros; a NaN stays, as in torch.max of two tensors.
 * One launch, a workgroup per (clip, 256 columns): the workgroup of a video's first clip in the batch folds all its clips in a register and
 * stores the row once. A row has the same bits on every run and however its clips are spread over rows and calls; no float atomics.
 *
 * egx_view_ensemble_topk replaces the torch.stack of the dict values and the four topk_errors calls of :142-158
 * (HOI/evaluation/lta/lta_metrics.py:38-84) over videos 0 .. n - 1:
 *   rank     (n, H) int32: #{c : x_c > x_y} + #{c < y : x_c == x_y} of the video's label y in its head's window (the rule of
 *            egx_segmented_ce: among equal values the lower class ranks first; torch.topk leaves it unspecified). A NaN ranks as the greatest
 *            value (as torch.topk has it). -1 where the label is outside [0, C[h]).
 *   pred     (n, H) int32: the class of rank 0.
 *   result   (3 + H + n_ks * H) int32, every one written by every call: n, n_dropped (clips dropped since the state was zeroed),
 *            n_nonfinite (videos with a non-finite value in any head), n_invalid[h] (videos whose label is outside [0, C[h]): never correct),
 *            correct[k][h] (videos with 0 <= rank < ks[k]). top-k error = (1 - correct / n) * 100: topk_errors divides by preds.size(0).
 * One launch; counts go through per-workgroup partials that the last workgroup to arrive adds in a fixed order; the arrival counter
 * leaves itself zero. Nothing synchronises.
 * Refused on the host, before any device work, with a message that names the limit: a null pointer; capacity < 1; H outside 1 .. 4;
 * C[h] outside 1 .. 2048; capacity * sum(C) > 2^31 state elements; B outside 1 .. 65536; ld < 1; windows that overlap or leave the row;
 * an unknown method; slot_bytes other than 4 / 8; without slots, slot0 < 0 or slot0 + B > capacity; n outside 1 .. capacity; n_ks outside
 * 1 .. 4; ks[k] outside 1 .. the narrowest head. */
size_t egx_view_ensemble_state(int capacity, int H, const int* C, size_t* offsets);
int egx_view_ensemble_update(const float* preds, int ld, int B, int H, const int* col0, const int* C, const int64_t* labels, const void* slots,
                             int slot_bytes, int slot0, int method, int capacity, void* state, void* stream);
int egx_view_ensemble_topk(int n, int capacity, int H, const int* C, const int* ks, int n_ks, void* state, int* rank, int* pred, void* result,
                           void* stream);
/* ---- ABI v24 additions (new symbols only, as v19 to v23: EGX_ABI_VERSION stays 18): ragged d = 128 training batches with the batch table
 * built ON THE DEVICE, so that ONE captured hipGraph serves every batch that fits a declared capacity ------------------------------------
 * egx_ragged_train_fwd / egx_ragged_bwd read HOST lengths and ship the table in launch arguments: a capture would replay that call's
 * lengths for ever. The calls below take the lengths from DEVICE memory when the launches RUN and size every grid, workspace offset and
 * weight-gradient launch by a capacity: B_cap clips, tok_cap tokens, ceil(tok_cap / 48) + B_cap tiles (a bound on sum_b ceil(S_b / 48) of
 * every batch that fits, which leaves at least (tok_cap - N) / 48 surplus tiles).
 *   lengths    DEVICE int (B_cap, n_segments). A clip whose lengths are ALL 0 is empty: no tile, no token, a zero row of logits, no part
 *              in the loss (its label counts as -1, whatever `target` holds) and zero gradient; it may stand anywhere in the batch.
 *   status     DEVICE uint32, sticky: the table kernel ORs in 1 (a length outside 0 .. segs[k].T), 2 (a clip with some segments empty and
 *              others not), 4 (a clip beyond 512 tokens), 8 (sum_b S_b > tok_cap). A batch with any of them runs as the EMPTY batch - every
 *              clip empty, so that no length indexes anything: zero logits, loss 0 and zero gradients (a captured optimizer step sees zero
 *              gradients). Nothing reads the word or synchronises; the caller looks when it chooses to and clears it itself.
 *   head       required (the head-less rows, egx_ragged_train_fwd's ASD output, are refused); tokens_out / d_tokens are ignored.
 *   the rest   as egx_ragged_train_fwd / egx_ragged_bwd, whose refusals carry over (p_feat, out_tokens, token_ce, bucket_cb, bwd_stage,
 *              learned positional gradients, d = 128 / h = 4 / f32s or bf16). Under capture, train-mode dropout needs egx_config.seed_ptr.
 *              B_cap <= 2^20, tok_cap <= 2^24, tok_cap >= B_cap * n_segments.
 * Results: a clip's logits and d(feature) rows are those of egx_ragged_train_fwd / egx_ragged_bwd on the same clips (the table is the same,
 * word for word); the loss and the weight gradients are the same fixed-order sums regrouped over capacity-sized ranges (the launches run
 * over tok_cap rows; the rows no clip owns are cleared first and add exact zeros). Bit-reproducible from replay to replay.
 * egx_ragged_cap_workspace: `saved` / `scratch` bytes, functions of the capacity alone (pure host arithmetic).
 * egx_ragged_cap_table: the table kernel alone (tests, diagnostics): table = B_cap records of 16 ints | tile -> clip map of the tile
 *              capacity, -1 for surplus tiles | B_cap * 4 packed first rows | 8 totals (tokens, tiles, any clip, rows of segment 0 .. 3,
 *              status bits of this build); eff_target (B_cap) int64 or NULL. table NULL: only *n_words (host only).
 * egx_ragged_table_host: the table egx_ragged_train_fwd (train != 0: with the packed first rows) or egx_ragged_fwd builds on the host for
 *              a batch with a head, without any device work: B records | tile -> clip map | B * 4 packed first rows. out_words NULL: only
 *              *n_words. */
int egx_ragged_table_host(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int train, int* out_words, size_t* n_words);
int egx_ragged_cap_workspace(const egx_config* cfg, const egx_segment* segs, int B_cap, int tok_cap, size_t* saved_bytes, size_t* scratch_bytes);
int egx_ragged_cap_table(const egx_config* cfg, const egx_segment* segs, int B_cap, int tok_cap, const int* lengths, const int64_t* target,
                         int* table, int64_t* eff_target, unsigned* status, size_t* n_words, void* stream);
int egx_ragged_cap_train_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                             const egx_layer* layers, const egx_head* head, int B_cap, int tok_cap, float* logits_out, float* tokens_out,
                             void* saved, void* scratch, unsigned* status, int training, uint64_t seed, void* stream);
int egx_ragged_cap_bwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                       const egx_layer* layers, const egx_head* head, int B_cap, int tok_cap, const float* d_logits, const float* d_tokens,
                       const void* saved, void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b,
                       const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, unsigned* status, int training, uint64_t seed,
                       void* stream);
/* ---- EgoT2-g sequence decoder + vocabulary head --------------------------------------------
 * decode() of HHI/models/multitask/task_prompt_model.py:260-269 and HOI/models/multitask/video_model_builder.py:150-159:
 * embedding * sqrt(d) + positional encoding -> nn.TransformerDecoder of CustomDecoderLayer (causal self-attention over
 * the 2..5 target tokens, cross-attention onto the encoder memory, FFN; post-LN) -> fc. Projections, LayerNorms and the
 * FFN reuse egx_linear_* / egx_layernorm_*; the entry points below are the decoder-specific pieces.
 *
 * Attention of a few queries against a short key set, one (batch element, head) per wave: rows are tokens (row index
 * b * S + s, row stride ld* floats), head h owns columns [h * dh, (h + 1) * dh). Sq <= 8, Sk <= 1024 (one wave per (b, h) up to 64 keys, four waves and chunked K / V beyond), dh <= 128.
 * causal != 0 (needs Sq == Sk) applies the reference's lower-triangular target mask. Self-attention passes the packed
 * qkv rows three times (q, q + d, q + 2d with ld = 3d), cross-attention q and the packed kv rows of the memory.
 * p_drop > 0: dropout on the probabilities, keyed by (seed, site); the backward regenerates the same mask and
 * recomputes the probabilities (nothing is saved).
 * Any head dim from 1 to 128 (not only multiples of 32) and any row strides >= H * dh, each operand its own: rows need no alignment, and
 * nothing outside the (row, head column) windows is read or written. */
int egx_small_attention_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                            int B, int Sq, int Sk, int H, int dh, int causal, float p_drop, uint64_t seed, uint32_t site,
                            void* stream);
/* dq / dk / dv use the strides of q / k / v and are overwritten (=), every (row, head column) exactly once. */
int egx_small_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* d_o,
                            int ldo, float* dq, float* dk, float* dv, int B, int Sq, int Sk, int H, int dh, int causal,
                            float p_drop, uint64_t seed, uint32_t site, void* stream);
/* out[b, t, :] = dropout(emb[tokens[b, t]] * scale + pe[t * pe_stride ...]); tokens (B, sy) int64, emb (V, d).
 * Backward: d_emb[tokens[b, t]] += scale * mask * dy[b, t], a token's rows summed in row order (no atomics: the same bits on every run)
 * into a zero-filled or live buffer. */
int egx_embed_pos_fwd(const int64_t* tokens, const float* emb, const float* pe, int pe_stride, float scale, float* out,
                      int B, int sy, int d, int V, float p_drop, uint64_t seed, void* stream);
int egx_embed_pos_bwd(const int64_t* tokens, const float* dy, float* d_emb, float scale, int B, int sy, int d, int V,
                      float p_drop, uint64_t seed, void* stream);
/* ---- the whole decoder as ONE call per direction (round 3) ----------------------------------------------------------
 * Same reference lines as above (task_prompt_model.py:260-269, video_model_builder.py:150-159; CustomDecoderLayer
 * task_prompt_model.py:163-172). compute = EGX_BF16 only: the B * sy target rows and the B * S memory rows run through the
 * bf16 MFMA GEMMs of the wide path with fused epilogues, the LayerNorms through its row kernels, the two attentions through
 * a register-resident kernel (one wave per (clip, head)). d_model a multiple of 128 in [256, 1024], head dim 32 or 64,
 * sy <= 8 target tokens, S <= 1024 memory tokens per clip; or (ABI v29) head dim 256 or 512 with d_model a multiple of 128 in
 * [256, 2048], sy <= 8 and S <= 16 (the 2048-wide LTA sequence decoders: 8 or 4 heads over a memory of 2 or 4 clip rows). Other
 * configurations return an error (the caller composes the decoder from the entry points above instead; head dim 256 / 512 is
 * served by compute = EGX_BF16 only). Parameters are torch-layout fp32 ([out, in] row-major); `ca_in_w` /
 * `ca_in_b` are the packed in-projection of the cross-attention (rows [0, d): query, rows [d, 3d): key / value). */
typedef struct egx_dec_config {
    int d_model, n_heads, d_ff, n_layers;
    int vocab;          /* |V|: rows of the embedding, outputs of fc */
    int sy, S;          /* target tokens per clip, memory tokens per clip */
    float ln_eps;
    int compute;        /* EGX_BF16 */
    float p_drop;       /* dropout of the decoder layers (attention probabilities, the three residual branches, FFN hidden) */
    float p_pos;        /* dropout of the positional encoding */
    const uint64_t* seed_ptr;   /* optional DEVICE pointer (the translator's egx_config.seed_ptr): dropout keys are derived on the stream
                                   from *seed_ptr instead of the host `seed`, so a captured hipGraph draws fresh masks per replay */
} egx_dec_config;
typedef struct egx_dec_layer {
    const float* sa_in_w; const float* sa_in_b; const float* sa_out_w; const float* sa_out_b; const float* norm1_w; const float* norm1_b;
    const float* ca_in_w; const float* ca_in_b; const float* ca_out_w; const float* ca_out_b; const float* norm2_w; const float* norm2_b;
    const float* lin1_w; const float* lin1_b; const float* lin2_w; const float* lin2_b; const float* norm3_w; const float* norm3_b;
} egx_dec_layer;
typedef struct egx_dec_layer_grads {     /* accumulated (+=); any may be NULL */
    float* sa_in_w; float* sa_in_b; float* sa_out_w; float* sa_out_b; float* norm1_w; float* norm1_b;
    float* ca_in_w; float* ca_in_b; float* ca_out_w; float* ca_out_b; float* norm2_w; float* norm2_b;
    float* lin1_w; float* lin1_b; float* lin2_w; float* lin2_b; float* norm3_w; float* norm3_b;
} egx_dec_layer_grads;
int egx_decoder_workspace(const egx_dec_config* cfg, int B, size_t* saved_bytes, size_t* scratch_bytes);
/* tokens (B, sy) int64; memory (B * S, d) fp32, rows b * S + s (the encoder output, batch-first); emb (vocab, d); pe rows at
 * pe + t * pe_stride; logits (B * sy, vocab) fp32 out. `saved` is read by the backward; `scratch` is free afterwards. */
int egx_decoder_fwd(const egx_dec_config* cfg, const int64_t* tokens, const float* memory, const float* emb, const float* pe, int pe_stride,
                    const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, float* logits, void* saved, void* scratch,
                    int training, uint64_t seed, void* stream);
/* d_memory (B * S, d) is overwritten (=); every parameter gradient is accumulated (+=) — `zero_buf` / `zero_bytes` (optional):
 * a buffer the first operation of the call zero-fills (the caller's flat gradient buffer holding all += targets).
 * Both calls are asynchronous on `stream`; internally the K | V projections (forward) and the weight gradients (backward) run on one
 * library-owned side stream that is forked off and joined back inside the call (also under stream capture). */
int egx_decoder_bwd(const egx_dec_config* cfg, const int64_t* tokens, const egx_dec_layer* layers, const float* fc_w, int B, const float* d_logits,
                    const void* saved, void* scratch, float* d_memory, float* d_emb, const egx_dec_layer_grads* grads, float* d_fc_w,
                    float* d_fc_b, void* zero_buf, size_t zero_bytes, int training, uint64_t seed, void* stream);
/* ---- ABI v29 additions (new symbols only, as v19 to v28: EGX_ABI_VERSION stays 18): head dim 256 / 512 in the sequence decoder ----------
 * d_model above 1024 is served at head dim 256 / 512 ONLY: head dim 32 / 64 keeps d_model <= 1024 (and S <= 1024), as before; e.g. d_model 1152
 * with 18 heads of 64 is still refused.
 * egx_decoder_workspace / _fwd / _bwd, egx_decoder_generate[_sched], egx_decoder_forced and egx_decoder_beam[_sched] accept head dim 256 /
 * 512 with d_model <= 2048 and S <= 16 memory rows (forward and backward attention: one wave per (clip, head), fp32 FMAs over a wave-
 * private LDS slice of the query rows; the cached step's self-attention splits the head dim over the lanes and walks the history).
 * Everything else keeps its limits: sy <= 8, vocabulary <= 1024 and n_steps <= 64 for the cached step, the beam head's 64 KiB of LDS
 * (at d_model 2048: beam_width <= 4). Refused at head dim 256 / 512, on the host, before any launch: the ragged entry points
 * (egx_decoder_ragged_*), the cross-attention weights (egx_decoder_cross_weights, egx_cross_attention_weights,
 * egx_decoder_generate_attn), S > 16, and compute f32 / f32s.
 *
 * The unit hook pair of the decoder's attention, the decoder-side twin of egx_wide_attention_fwd / _bwd: exactly the launch
 * egx_decoder_fwd / _bwd and the cached step's cross-attention make. q rows b * Sq + i (leading dimension ldq), k / v rows b * Sk + j,
 * head h at columns [h * dh, + dh); operands_bf16 != 0: q / k / v and dq / dk / dv are bf16, else fp32 (layer 0's self-attention); o and
 * d_o are bf16. causal: key j <= query i (Sk = Sq). Scores scaled by 1 / sqrt(dh). Dropout on the probabilities keyed as the decoder keys
 * it: site_key(seed, 0x40 + layer, site) (sites: 1 self-attention, 3 cross-attention), row (b * H + h) * 8 + i, column j. The backward
 * recomputes the probabilities; every element of dq (B * Sq rows), dk and dv (B * Sk rows) within the head columns is written once.
 * dh 32 / 64: Sq <= 8, Sk <= 1024 (Sk > 64: bf16 operands, not causal). dh 256 / 512: Sq <= 8, Sk <= 16. Pointers 16-byte aligned,
 * leading dimensions multiples of 8 and >= H * dh. A refusal names the limit and launches nothing. */
typedef struct egx_dec_attn_args {
    const void* q; const void* k; const void* v; int ldq, ldk, ldv; int operands_bf16;
    void* o; int ldo;                                           /* forward: (B * Sq, ldo) bf16 out */
    const void* d_o; void* dq; void* dk; void* dv;              /* backward */
    int B, H, dh, Sq, Sk, causal;
    float p_drop; uint64_t seed; uint32_t layer, site;
    void* stream;
} egx_dec_attn_args;
int egx_decoder_attention_fwd(const egx_dec_attn_args* args);
int egx_decoder_attention_bwd(const egx_dec_attn_args* args);
/* ---- ABI v18: the decoder over ragged memories (inference) ----
 * decode() (task_prompt_model.py:260-269) of B clips whose memories differ in length: `memory` holds sum_b S_b packed rows (clip after
 * clip, S_b = mem_lengths[b], HOST int[B]; egx_ragged_encode's out_layout 0 output), clip b's target rows cross-attend to its own S_b rows
 * only. tokens (B, sy) int64, logits (B * sy, vocab) as egx_decoder_fwd. cfg->S is the longest memory (1 <= S_b <= cfg->S <= 1024); every
 * other limit is egx_decoder_fwd's. Refused: p_drop / p_pos > 0. `workspace`: egx_decoder_ragged_workspace() bytes (a function of
 * sum_b S_b). The call writes a per-clip table from `mem_lengths` into the workspace on `stream`: not for graph capture. */
int egx_decoder_ragged_workspace(const egx_dec_config* cfg, int B, const int* mem_lengths, size_t* bytes);
int egx_decoder_ragged_fwd(const egx_dec_config* cfg, const int64_t* tokens, const float* memory, const int* mem_lengths, const float* emb,
                           const float* pe, int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B,
                           float* logits, void* workspace, void* stream);
/* ---- ABI v18: the decoder over ragged memories, training ----
 * The decoder side of the same training step (decode(), task_prompt_model.py:260-269, inside video_tasktranslation.py:39-66; the
 * mixed-length batches of :144-156): egx_decoder_fwd / egx_decoder_bwd over a packed memory of sum_b S_b rows (mem_lengths as
 * egx_decoder_ragged_fwd), with dropout on every site. Clip b's target rows cross-attend to its own rows only; d_memory is packed
 * (sum_b S_b, d) and a clip's rows receive gradient from that clip's target rows alone. Dropout keys as the uniform decoder: target row, and
 * (clip's index in the batch, head, query) on the attention probabilities, so equal memories draw egx_decoder_fwd's masks. The self-attention
 * and all row-wise parts are the uniform code over B * sy target rows and sum_b S_b memory rows. egx_decoder_ragged_bwd takes the SAME
 * mem_lengths and the forward's `saved`; every other argument as egx_decoder_bwd. `saved` / `scratch`: egx_decoder_ragged_train_workspace()
 * bytes (functions of sum_b S_b). The forward writes the per-clip table into `saved` on `stream`: not for graph capture. */
int egx_decoder_ragged_train_workspace(const egx_dec_config* cfg, int B, const int* mem_lengths, size_t* saved_bytes, size_t* scratch_bytes);
int egx_decoder_ragged_train_fwd(const egx_dec_config* cfg, const int64_t* tokens, const float* memory, const int* mem_lengths, const float* emb,
                                 const float* pe, int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B,
                                 float* logits, void* saved, void* scratch, int training, uint64_t seed, void* stream);
int egx_decoder_ragged_bwd(const egx_dec_config* cfg, const int64_t* tokens, const int* mem_lengths, const egx_dec_layer* layers, const float* fc_w,
                           int B, const float* d_logits, const void* saved, void* scratch, float* d_memory, float* d_emb,
                           const egx_dec_layer_grads* grads, float* d_fc_w, float* d_fc_b, void* zero_buf, size_t zero_bytes, int training,
                           uint64_t seed, void* stream);
/* ---- ABI v18: greedy generation with a K/V cache ----
 * The inference loop of the EgoT2-g sequence models as ONE asynchronous call: predict_ac (HOI/models/multitask/video_model_builder.py:201-220,
 * 263-274: start token, then each next token the argmax over a decode() of the growing prefix) and the same loop over 40 steps in
 * HOI/models/lta/lta_models_seqdecoder.py:181-201. For t = 0 .. n_steps - 1: x_t = emb[tok_t] * sqrt(d) + pe[t] (tok_0 = start[b]) runs through
 * the post-LN decoder layers, its causal self-attention over rows 0 .. t (a per-layer K/V cache), its cross-attention over the clip's S memory
 * rows (K | V projected once per layer); logits_t = fc(x_t); tok_{t+1} = argmax(logits_t), the LOWEST index on ties. Dropout is off, so this is
 * the reference loop: row t of a causal decoder does not depend on later rows. Arithmetic as egx_decoder_fwd, choice for choice (layer 0's
 * self-attention in-projection in exact fp32 with an fp32 cache, every other GEMM bf16 with fp32 accumulation, the vocabulary head in fp32).
 * start (B,) int64; memory (B * S, d) fp32 as egx_decoder_fwd; pe needs n_steps rows; tokens_out (B, n_steps) int64 = tok_1 .. tok_n;
 * logits_out (n_steps, B, vocab) fp32 or NULL. Limits: egx_decoder_fwd's for d_model, heads, d_ff, layers and S; 1 <= n_steps <= 64;
 * 1 <= vocab <= 1024; cfg->sy is not read. Refused: p_drop / p_pos > 0, compute other than EGX_BF16, null pointers. `workspace`:
 * egx_decoder_generate_workspace() bytes (bf16 weights, the bf16 memory and its K | V per layer once; per layer a (B, n_steps, 2d) K/V cache;
 * single-row activations). No token is read on the host: the call can be captured in a hipGraph and replayed on new start / memory contents.
 * Under capture it stays on `stream`; eagerly the K | V projections run on the library's side stream (as egx_decoder_fwd). */
int egx_decoder_generate_workspace(const egx_dec_config* cfg, int B, int n_steps, size_t* bytes);
int egx_decoder_generate(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
                         const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int64_t* tokens_out,
                         float* logits_out /* may be NULL */, void* workspace, void* stream);
/* ---- ABI v18: beam search (the W best sequences per clip) with a K/V cache ----
 * The LTA evaluation scores K = 5 candidate sequences per clip (HOI/tasks/lta/long_term_anticipation.py:233-388, model.generate(x, k=5)); the
 * reference draws them by sampling every position independently from the logits of the one greedy path
 * (HOI/models/lta/lta_models_seqdecoder.py:204-216) and marks the gap at :197 ("#todo: better decoding ways"). This call is the standard
 * answer, as ONE asynchronous call on egx_decoder_generate's step: fixed-length beam search (the schedules have no end-of-sequence word: no
 * early stop, no length penalty). Rows are (B, W), row b * W + w = hypothesis slot w of clip b. A hypothesis' score is the fp32 sum over its
 * steps of log_softmax(logits)[token]. At step 0 only slot 0 is live (score 0; slots 1 .. W - 1 start at -inf). At every step the W * vocab
 * candidates score[w] + logp[w][v] of a clip are ranked and the W best survive in descending order; ties go to the LOWEST flat index
 * w * vocab + v, a NaN never wins. tokens_out (B, W, n_steps) int64: tokens_out[b][k] the k-th best final sequence (the n_steps tokens after
 * start[b]), scores_out (B, W) fp32 its score. The optional step_* outputs are the selection trace of step t, each (n_steps, B, W, ...):
 * step_tokens / step_parents (int32: the parent's slot at step t - 1) / step_scores of every surviving slot, and step_logits (n_steps, B, W,
 * vocab): for each PARENT slot w the logits row the head computed at step t (at step 0 every slot holds the start token's row).
 * Arithmetic as egx_decoder_generate (with W = 1 the same bits: tokens, logits); the memory is converted and projected once per clip, not
 * once per hypothesis; the per-layer K/V cache (B, W, n_steps, 2d) is written once and read through an ancestry table, never gathered.
 * Limits: egx_decoder_generate's (compute EGX_BF16, the fused decoder's shapes, 1 <= n_steps <= 64, 1 <= vocab <= 1024, p_drop = p_pos = 0),
 * 1 <= W <= 8 and W <= vocab; cfg->sy is not read. Every refusal is made before any device work, by the call and by the workspace query
 * alike. No value is read on the host: the call can be captured in a hipGraph and replayed on new start / memory contents; the memory's
 * K | V projections use the side stream as egx_decoder_generate's do. */
int egx_decoder_beam_workspace(const egx_dec_config* cfg, int B, int n_steps, int W, size_t* bytes);
int egx_decoder_beam(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
                     const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int W,
                     int64_t* tokens_out /* (B, W, n_steps) */, float* scores_out /* (B, W) */,
                     int64_t* step_tokens /* (n_steps, B, W) or NULL */, int32_t* step_parents /* (n_steps, B, W) or NULL */,
                     float* step_scores /* (n_steps, B, W) or NULL */, float* step_logits /* (n_steps, B, W, vocab) or NULL */,
                     void* workspace, void* stream);
/* ---- ABI v18 (additions): per-step token schedules for greedy generation and beam search ----
 * The reference reads the LTA outputs through word subsets: HOI/models/lta/lta_models_seqdecoder.py:190-201 keeps output_prob[-1, :, self.v_idx]
 * at odd steps and [..., self.n_idx] at even steps, generate() takes the argmax (or a Categorical) over that subset, and vocab_idx_to_orig()
 * supplies the two index arrays. A token schedule gives every step the set of words it may emit, enforced in the head of the step on the
 * device. `period` rows P (0 <= P <= 64; 0: no schedule, the unscheduled call); step t (0-based) uses row t % P. counts: HOST int[P], the
 * size of each row's set, 1 .. vocab. words: DEVICE int32[P][vocab], row p's first counts[p] entries the set's word indices in ascending
 * order, the rest padded with the last index. At a scheduled step the head computes the listed vocabulary rows ONLY; every other word has
 * logit -inf (so in logits_out / step_logits). A listed word's logit has the bits the unscheduled call gives for the same input row. Greedy
 * takes the argmax over the set (lowest index on ties); beam takes log_softmax over the set (the normaliser sums the set's words only, as
 * Categorical(logits=head_x[..., v_idx]) does) and ranks the W * counts finite candidates by the unscheduled tie rule. Deliberately unlike
 * the reference, which feeds back the full-vocabulary argmax and only READS the subset, the fed-back word is the subset's argmax; the two
 * agree whenever the full argmax lies in the set. Indices read from `words` are clamped to 0 .. vocab - 1 and counts to vocab on the
 * device: a corrupt list gives wrong tokens, never a read outside fc_w / fc_b / emb. Every other argument, limit and the workspace
 * (egx_decoder_generate_workspace / egx_decoder_beam_workspace) as the unscheduled calls; nothing is copied from the host per step, so the
 * calls can be captured as those can. Refused before any device work: period < 0 or > 64; period > 0 with counts or words null; a count
 * outside 1 .. vocab; for beam counts[0] < W (at step 0 only slot 0 is live: the step has only counts[0] continuations). */
int egx_decoder_generate_sched(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe,
                               int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps,
                               int64_t* tokens_out, float* logits_out /* may be NULL */, void* workspace, void* stream, int period,
                               const int* counts /* HOST int[period] */, const int32_t* words /* DEVICE int32[period][vocab] */);
/* egx_decoder_beam with a token schedule (lta_models_seqdecoder.py:190-201; see egx_decoder_generate_sched). */
int egx_decoder_beam_sched(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
                           const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int W,
                           int64_t* tokens_out /* (B, W, n_steps) */, float* scores_out /* (B, W) */,
                           int64_t* step_tokens /* (n_steps, B, W) or NULL */, int32_t* step_parents /* (n_steps, B, W) or NULL */,
                           float* step_scores /* (n_steps, B, W) or NULL */, float* step_logits /* (n_steps, B, W, vocab) or NULL */,
                           void* workspace, void* stream, int period, const int* counts /* HOST int[period] */,
                           const int32_t* words /* DEVICE int32[period][vocab] */);
/* ---- ABI v18 (additions): the decoder's cross-attention weights as an output ----
 * The reference subclasses nn.TransformerDecoderLayer as CustomDecoderLayer so that _mha_block calls the cross-attention with
 * need_weights=True (HHI/models/multitask/task_prompt_model.py:163-172, HOI/models/multitask/video_model_builder.py:20-30,
 * video_model_builder_2task.py:24, HOI/models/lta/lta_models_seqdecoder.py:30-39): a forward hook on layer.multihead_attn then sees the
 * head-averaged weights (B, sy, S) of every decoder layer: which task's tokens, at which time steps, the task prompt reads.
 *   w[b, i, j] = (1 / H) sum_h softmax_j(q[b, i, h, :] . k[b, j, h, :] / sqrt(dh))
 * Scores, max, exp, sum and normalisation in fp32; the head sum in head order 0 .. H - 1, then one multiply by 1 / H; every reduction
 * has a fixed order and there are no atomics, so a clip's rows do not depend on its position in the batch. Inference only: the
 * reference returns the weights after dropout, which these calls do not model. Beam search has no such output (a hypothesis changes
 * slots every step; egx_decoder_beam's step_* trace is the tool there).
 *
 * egx_cross_attention_weights: the primitive, on the caller's tensors. q rows b * Sq + i (row stride ldq elements), k rows b * Sk + j
 * (stride ldk), head h at columns [h * dh, (h + 1) * dh); operands_bf16 != 0: bf16 elements, else fp32. mtab (DEVICE int[B][2] or NULL):
 * clip b's keys are rows [mtab[2b], + S_b) of k with S_b = mtab[2b + 1] clamped to 0 .. Sk. out fp32, row b * Sq + i at stride ldo >= Sk:
 * Sk entries are written, entries j >= S_b as exact zeros. dh 16, 32, 64 or 128; Sq >= 1; 1 <= Sk <= 1024; any B. Refused before any
 * device work: null q / k / out, another dh, Sk outside 1 .. 1024, ldo < Sk, ldq / ldk not a multiple of 8 elements or below H * dh,
 * q / k not 16-byte aligned. One launch, asynchronous on `stream`, capturable. */
int egx_cross_attention_weights(const void* q, int ldq, const void* k, int ldk, int operands_bf16, const int* mtab /* DEVICE int[B][2] or NULL */,
                                int B, int H, int dh, int Sq, int Sk, float* out, int ldo, void* stream);
/* The weights of the decode() call (task_prompt_model.py:260-269 through CustomDecoderLayer :163-172) that egx_decoder_fwd
 * (mem_lengths NULL) or egx_decoder_ragged_fwd (mem_lengths: the SAME HOST int[B]) has just run with the same cfg and B on the same
 * stream: reads every layer's cross-attention q and k | v rows from that call's `saved` / `workspace` (for ragged calls also the table it
 * uploaded) and writes attn_out (n_layers, B, sy, S) fp32, S = cfg->S, for ragged calls the longest memory (zeros beyond S_b). n_layers
 * launches. Refused before any device work: p_drop / p_pos > 0, every limit of the forward call, null pointers. */
int egx_decoder_cross_weights(const egx_dec_config* cfg, int B, const int* mem_lengths /* HOST int[B] or NULL */, const void* saved,
                              float* attn_out, void* stream);
/* egx_decoder_generate_sched (period = 0: egx_decoder_generate) that also writes attn_out (n_layers, n_steps, B, S) fp32: after each
 * layer's cross-attention of step t one launch of the primitive with Sq = 1 on the step's q and the layer's k | v, the weights the hook on
 * the greedy loop of lta_models_seqdecoder.py:181-201 over CustomDecoderLayer (:30-39) sees in the last row of step t. Tokens and logits
 * have the bits of the call without attn_out, which issues exactly the launches it issued before this entry existed. attn_out NULL is
 * refused. Capturable as egx_decoder_generate. */
int egx_decoder_generate_attn(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe,
                              int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps,
                              int64_t* tokens_out, float* logits_out /* may be NULL */, void* workspace, void* stream, int period,
                              const int* counts /* HOST int[period] */, const int32_t* words /* DEVICE int32[period][vocab] */,
                              float* attn_out /* (n_layers, n_steps, B, S) */);
/* ---- ABI v18 (additions): teacher-forced decoding of up to 64 target tokens on the K/V-cached step ----
 * The reference runs its sequence decoders over given target tokens longer than the 8 rows egx_decoder_fwd serves: the validation step
 * model(video, target[:, :-1], 'lta_verb') over the 21 tokens [lta_verb, 20 verbs] (HOI/tasks/multitask/video_task.py:601-617,
 * HOI/tasks/multitask/video_task_action.py:83-88: val_loss_lta_verb / val_loss_lta_noun) and the 40-token teacher-forced call of
 * HOI/models/lta/lta_models_seqdecoder.py:175-179. Row t of a causal decoder without dropout sees rows 0 .. t only, so the call is
 * egx_decoder_generate's step with step t's input row taken from `tokens` instead of the argmax: x_t = emb[tokens[.., t]] * sqrt(d) + pe[t]
 * through the layers (self-attention over the per-layer K/V cache of rows 0 .. t, cross-attention onto the clip's memory), launches and
 * arithmetic as egx_decoder_generate, choice for choice: fed the tokens greedy generation chose, it returns that call's logits bit for bit.
 * Sequential over the steps (inference: validation loss, scoring of candidate sequences); nothing runs backward.
 * R target sequences per clip, 1 <= R <= 8: tokens / targets / logprob_out are (B, R, n_steps), row b * R + r = sequence r of clip b; the
 * R rows of a clip share the clip's memory (B * S rows, converted and projected once per clip; the cross-attention runs with Sq = R, as
 * egx_decoder_beam's W slots do). All B * R * n_steps input rows are embedded in one launch; a token outside [0, vocab) embeds as the
 * zero row (as egx_decoder_fwd's do). Each step's last-layer rows go into an (n_steps, B * R, d) slab and ONE launch of the fp32
 * vocabulary head after the last step writes logits_out (n_steps, B * R, vocab) when given and, with targets,
 *   logprob_out[b][r][t] = logit[target] - max - log(sum_v exp(logit[v] - max))   (fp32; the sum in a fixed order)
 * the log-probability of targets[b][r][t] under step t's logits; a target outside [0, vocab) (padding such as -100) gives exactly 0.0, a
 * NaN logit propagates. A row's logits have the bits egx_decoder_generate's head computes for the same row. Limits: egx_decoder_generate's
 * (compute EGX_BF16, the fused decoder's d_model, heads, d_ff, layers and S, 1 <= n_steps <= 64, 1 <= vocab <= 1024, p_drop = p_pos = 0);
 * cfg->sy is not read. Refused before any device work, by the call and (where it applies) the workspace query: R outside 1 .. 8, both
 * outputs null, logprob_out without targets, null pointers, a pe_stride below d_model or not a multiple of 4, B * R or B * S too large.
 * No float atomics, no value read on the host: the call can be captured in a hipGraph and replayed on new tokens, targets and memory; the
 * memory's K | V projections use the side stream as egx_decoder_generate's do. */
int egx_decoder_forced_workspace(const egx_dec_config* cfg, int B, int R, int n_steps, size_t* bytes);
int egx_decoder_forced(const egx_dec_config* cfg, const int64_t* tokens /* DEVICE (B, R, n_steps): the input tokens */,
                       const int64_t* targets /* DEVICE (B, R, n_steps) or NULL */, const float* memory, const float* emb, const float* pe,
                       int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int R, int n_steps,
                       float* logits_out /* (n_steps, B * R, vocab) fp32 or NULL */, float* logprob_out /* (B, R, n_steps) fp32 or NULL; needs targets */,
                       void* workspace, void* stream);
/* ---- ABI v18 (additions): attention of up to 64 target rows, forward and backward (training on long targets) ----
 * The reference TRAINS its HOI action / LTA sequence decoders on 21- and 40-token targets (HOI/tasks/multitask/video_task_action.py:34-53:
 * self.model(input, target_seq_verb[:, :-1], 'lta_verb') in training_step; HOI/models/lta/lta_models_seqdecoder.py:175-179);
 * egx_small_attention_* stop at 8 query rows and stay as they are. These two have their semantics, operands and layout (fp32, rows at
 * arbitrary strides >= H * dh, head h at columns [h * dh, (h + 1) * dh), self-attention passes the packed qkv rows three times,
 * cross-attention q and the packed kv rows; rows need no alignment, nothing outside the (row, head column) windows is read or written)
 * for 1 <= Sq <= 64, 1 <= Sk <= 1024, 1 <= dh <= 128, any B and H; causal != 0 needs Sq == Sk. fp32 on the VALU throughout. One
 * workgroup of four waves per (b, h) walks the query rows in groups of 8, K / V chunked by 64 rows through LDS; no float atomics, every
 * sum in a fixed order, a (b, h)'s result independent of B. The backward recomputes the probabilities and regenerates the mask (the
 * forward saves nothing); dq / dk / dv use the strides of q / k / v and are overwritten at the call level, every (row, head column)
 * exactly once per call (dk / dv: the owning thread assigns the first query group's sum and adds the later ones to it), so a zero-filled
 * buffer is not assumed. p_drop > 0: dropout on the probabilities keyed like the composed decoder's sites (key layer site >> 8, site
 * site & 0xff), row (b * H + h) * 64 + query, column key: the row stride is 64 here, 8 in egx_small_attention_*.
 * Refused before any device work: Sq outside 1..64, Sk outside 1..1024, dh outside 1..128, causal with Sq != Sk, null pointers, a row
 * stride below H * dh. */
int egx_target_attention_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo,
                             int B, int Sq, int Sk, int H, int dh, int causal, float p_drop, uint64_t seed, uint32_t site,
                             void* stream);
int egx_target_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* d_o,
                             int ldo, float* dq, float* dk, float* dv, int B, int Sq, int Sk, int H, int dh, int causal,
                             float p_drop, uint64_t seed, uint32_t site, void* stream);
/* dy[i] = y[i] > 0 ? dy[i] : 0 in place: backward of the ReLU fused into egx_linear_fwd(relu = 1). Wherever y is not > 0 (y = NaN, -0 and
 * -inf included) dy becomes +0; a denormal y > 0 keeps its dy. n = 0 touches nothing. */
int egx_relu_mask(float* dy, const float* y, size_t n, void* stream);
/* Producer side of the feature hand-off: the `middle=True` head of the frozen PNR / OSCC backbones,
 * ResNetKeyframeLocalizationHead.forward (HOI/models/pnr/head_helper.py:353-373) = AvgPool3d((kt, kh, kw), stride 1) of the res5
 * map fmap (N, C, T, H, W) [fp32, or bf16 with fmap_bf16], permute to (N, T', H', W', C), reshape to rows of H' W' C columns
 * (8192 = 2 * 2 * 2048) - optionally followed by the per-clip temporal mean of encode_clips_pnr
 * (HOI/models/lta/lta_models_lta_transfer.py:335-345; frames_mean != 0, or kt == T) - written as packed fp32 / bf16 rows:
 * out[n * out_map_stride + t' * (H' W' C) + (h' W' + w') * C + c]. With out_map_stride = n_clips * H' W' C and `out` offset by
 * i * H' W' C, call i fills token i of every sample of a (B, n_clips, 8192) translator input in place. kt must be 1 or T. */
int egx_pool_pack(const void* fmap, int fmap_bf16, int N, int C, int T, int H, int W, int kt, int kh, int kw, int frames_mean,
                  void* out, int out_bf16, long long out_map_stride, void* stream);

/* ---- gradient exchange -----------------------------------------------------------------------------
 * RCCL (ncclAllReduce over xGMI) behind plain pointers, for callers that do not use torch.distributed. Replaces what the reference
 * gets from Lightning DDP's reducer (HOI/scripts/multitask/run.py:41-50: strategy DDP, `find_unused_parameters`; HHI: the
 * `gpus=-1, accelerator='ddp'` trainers): ONE all-reduce, sum then 1 / n, over the flat gradient buffer every backward of this
 * library writes its gradients into (2.77 MB for the TTM translator, 181 MB for the LTA 4-task one).
 *   egx_comm_unique_id : rank 0 draws the 128-byte RCCL id; the caller carries it to the other ranks.
 *   egx_comm_create    : one communicator per process, on the calling thread's current HIP device (one rank per GPU).
 *   egx_allreduce      : in place over `n` elements of `buf` (dtype 0 = fp32, 1 = bf16), sum or average, asynchronous on `stream`
 *                        (hipGraph-capturable: RCCL kernels are ordinary stream work). Every rank must call it with the same n.
 *   egx_comm_size      : the rank count RCCL itself reports for the communicator (-1 on error).
 *   egx_comm_library   : the RCCL library that was resolved ("" when none): the copy already loaded in the process if there is
 *                        one (PyTorch's), else librccl.so(.1) / $EGX_RCCL_LIB. The library has no link-time dependency on RCCL.
 * egot2_amd/ddp.py keeps torch.distributed (backend "nccl" = RCCL) for the nn.Module path — Lightning's DDP hands it a process group —
 * and offers `EgxComm` over these calls for harnesses without one. */
typedef struct egx_comm egx_comm;
int egx_comm_unique_id(void* id128);
int egx_comm_create(const void* id128, int rank, int world, egx_comm** out);
int egx_comm_size(const egx_comm* comm);
int egx_allreduce(egx_comm* comm, void* buf, size_t n, int dtype, int average, void* stream);
int egx_comm_destroy(egx_comm* comm);
const char* egx_comm_library(void);

/* x[r, c] *= keep(seed, site, r, c) / (1 - p) in place (inverted dropout); calling it on the gradient with the same
 * (seed, site) is its backward. */
int egx_dropout(float* x, int rows, int cols, float p_drop, uint64_t seed, uint32_t site, void* stream);

/* Per-kernel device timing for bench.py's roofline block: hipEvents recorded on the launch stream around the
 * fused kernels while enabled (which: 0 = fused forward, 1 = fused per-clip backward, 2 = FFN weight gradients).
 * egx_timing_read synchronises on the recorded events; never call it inside a timed or captured region. */
void egx_timing_enable(int on);
int egx_timing_read(int which, double* total_ms, int* count);
/* Sliced mode (small batches, egx_encoder_slices() > 1) diagnostic: how many FFN slices waiting workgroups have computed themselves since the
 * last reset because a partner workgroup's partial sum did not arrive within 100 us (a busy GPU shared with another process — or a stray
 * EGX_SLICE_DROP in the environment). 0 on a quiet GPU; every count is ~100 us of waiting plus a recomputed slice. Synchronous (reads device
 * memory): never inside a timed or captured region. -1 on error. */
long long egx_slices_stolen(int reset);
/* development aid: phase timestamps of the fused forward (only meaningful in -DEGX_STAMPS builds) */
int egx_debug_stamps(unsigned long long* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* EGOT2X_H */
