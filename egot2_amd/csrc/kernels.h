// Internal launch interfaces shared by the translation units of libegot2x.
#pragma once
#include "common.h"

namespace egx {

struct GemmParams {
    const float* A = nullptr;
    const float* B = nullptr;
    float* C = nullptr;
    int M = 0, N = 0, K = 0;
    int lda = 0, ldb = 0, ldc = 0;
    const float* bias = nullptr;       // [N]
    const float* residual = nullptr;   // [M, ldr], added last
    int ldr = 0;
    const float* mask = nullptr;       // [M, ldm]; C = mask > 0 ? C * mask_scale : 0   (ReLU / dropout backward)
    int ldm = 0;
    float mask_scale = 1.f;
    int relu = 0;
    uint64_t drop_key = 0;             // inverted dropout on (acc + bias [relu]) keyed by (row, col)
    uint32_t drop_thresh = 0;
    float drop_inv_keep = 1.f;
    int atomic = 0;                    // split-K partials are atomically added into C (small weight gradients)
    int k_chunk = 0;                   // set by gemm()
    size_t slab_stride = 0;            // set by gemm()
};

// Deterministic mode of the shape-generic kernels (egx_config.deterministic): while a DetScope is alive on this thread, the
// cross-workgroup sums that normally use fp32 atomics (split-K weight gradients, LayerNorm / bias / head parameter gradients)
// go through partial buffers in `buf` and fixed-order reductions instead. `buf` must hold generic_det_scratch_bytes().
struct DetScope {
    DetScope(void* buf, size_t bytes);
    ~DetScope();
};
bool det_on();
size_t generic_det_scratch_bytes(int B, int d, int d_ff);

// layout: 0 NT, 1 NN, 2 TN (see gemm.hip). compute: 0 fp32 MFMA, 1 bf16 MFMA.
int gemm(int layout, GemmParams p, int compute, int accumulate, void* scratch, size_t scratch_bytes, hipStream_t st);
size_t gemm_scratch_bytes(int layout, int M, int N, int K);

// y[orow] = dropout(LN(x[row] (+ res[row])) * w + b) (+ add_vec) (+ pos[t]); row -> orow = (row / T) * S + off + row % T.
struct LnFwdParams {
    const float* x = nullptr;     // [rows, d]
    const float* res = nullptr;   // [rows, d] or null
    const float* w = nullptr;
    const float* b = nullptr;
    float eps = 1e-5f;
    float* pre = nullptr;         // [rows, d] x + res written when non-null
    float* stats = nullptr;       // [rows, 2] (mean, rstd) when non-null
    float* y = nullptr;
    int rows = 0, d = 0;
    int T = 1, S = 1, off = 0;    // output row remap (T == S == 1... identity when T == S and off == 0)
    const float* add_vec = nullptr;
    const float* pos = nullptr;
    int pos_stride = 0;
    uint64_t drop_key = 0;
    uint32_t drop_thresh = 0;
    float drop_inv_keep = 1.f;
};
int layernorm_fwd(const LnFwdParams& p, hipStream_t st);

// dx[row] = LN backward of dy[orow] (dropout mask re-applied to dy first); dw/db accumulated (+=).
struct LnBwdParams {
    const float* dy = nullptr;    // rows addressed through the remap
    const float* pre = nullptr;   // [rows, d]
    const float* stats = nullptr; // [rows, 2]
    const float* w = nullptr;
    float* dx = nullptr;          // [rows, d]
    float* dw = nullptr;          // [d] +=
    float* db = nullptr;          // [d] +=
    float* dadd = nullptr;        // [d] += sum of (masked) dy rows (task-embedding gradient) or null
    int rows = 0, d = 0;
    int T = 1, S = 1, off = 0;
    uint64_t drop_key = 0;        // mask on dy (dropout applied after LN in forward)
    uint32_t drop_thresh = 0;
    float drop_inv_keep = 1.f;
    uint64_t out_drop_key = 0;    // mask on dx (dropout applied before LN in forward: HOI feature dropout)
    uint32_t out_drop_thresh = 0;
    float out_drop_inv_keep = 1.f;
};
int layernorm_bwd(const LnBwdParams& p, hipStream_t st);

// out[c] += sum_r x[r * ld + c], r < rows, c < cols
int colsum_accum(const float* x, int rows, int cols, int ld, float* out, hipStream_t st);
// ... with the row blocks' partial sums in `part` (colsum_part_bytes(rows, cols) bytes) and added in block order: run-to-run bit-identical
size_t colsum_part_bytes(int rows, int cols);
int colsum_accum_ordered(const float* x, int rows, int cols, int ld, float* out, void* part, size_t part_bytes, hipStream_t st);
// learned positional gradient: dpos[t * pos_stride + c] += sum_b dtok[(b * S + off + t) * d + c]  (dropout mask re-applied)
int pos_grad_accum(const float* dtok, int B, int S, int off, int T, int d, float* dpos, int pos_stride,
                   uint64_t drop_key, uint32_t drop_thresh, float drop_inv_keep, hipStream_t st);
// x[i] *= dropmask(row, col) for a dense [rows, d] tensor
int apply_dropout_mask(float* x, int rows, int d, uint64_t key, uint32_t thresh, float inv_keep, hipStream_t st);

int attention_fwd(const float* qkv, float* out, float* lse, int B, int S, int H, int d,
                  uint64_t drop_key, uint32_t drop_thresh, float drop_inv_keep, hipStream_t st);
int attention_bwd(const float* qkv, const float* out, const float* lse, const float* d_out, float* d_qkv,
                  int B, int S, int H, int d,
                  uint64_t drop_key, uint32_t drop_thresh, float drop_inv_keep, hipStream_t st);

int pool_head_fwd(const float* tokens, int B, int S, int d, const float* ln_w, const float* ln_b, float eps,
                  const float* W, const float* b, int n_out, float* pooled, float* out, hipStream_t st);
// ragged batch (egx_ragged_fwd): clip b = rows [tok0_b, tok0_b + S_b) of `tokens` (the device batch table, fused.h RAGGED_REC)
int pool_head_ragged_fwd(const float* tokens, const int* rtab, int B, int d, const float* ln_w, const float* ln_b, float eps,
                         const float* W, const float* b, int n_out, float* pooled, float* out, hipStream_t st);
int pool_head_bwd(const float* d_out, const float* pooled, int B, int S, int d, const float* ln_w,
                  const float* ln_b, float eps, const float* W, int n_out, float* d_tokens, float* d_ln_w,
                  float* d_ln_b, float* d_W, float* d_b, hipStream_t st);

// train.hip
int weighted_ce(const float* logits, const int64_t* target, const float* weight, int B, int C, float* loss,
                float* dlogits, hipStream_t st);
int counter_add(int64_t* c, int64_t inc, hipStream_t st);
size_t linear_ce_scratch_bytes(int M, int K, int C);
int linear_ce_fwd(const float* x, const float* W, const float* b, const int64_t* target, const float* weight, int M, int K, int C,
                  float* logits, float* probs, float* dlogits, float* loss, float* correct, float* pred, void* scratch, hipStream_t st);
int linear_ce_bwd(const float* x, const float* W, const float* dlogits, const float* gscale, int M, int K, int C, float* dx,
                  float* dW, float* db, void* scratch, hipStream_t st);
int adam_step(float* p, const float* g, float* m, float* v, size_t n, const int64_t* step, float lr, float b1, float b2,
              float eps, float wd, int decoupled, float grad_scale, hipStream_t st);
int adam_step_dev_lr(float* p, const float* g, float* m, float* v, size_t n, const int64_t* step, const float* lr, float b1, float b2,
                     float eps, float wd, int decoupled, float grad_scale, hipStream_t st);
// schedule kinds of lr_update (the values of the C ABI's EGX_LR_* enum) and its group limit (EGX_LR_MAX_GROUPS)
enum LrKind { LR_CONSTANT = 0, LR_COSINE_ANNEALING = 1, LR_WARMUP_COSINE = 2, LR_WARMUP_LINEAR = 3, LR_TABLE = 4 };
constexpr int LR_MAX_GROUPS = 16;
int lr_update(int kind, long long warmup, long long t_total, long long T_max, double cycles, const double* factors, long long n_factors,
              int64_t* step, const double* base_lr, int n_groups, float* lr_out, hipStream_t st);
int sgd_step(float* p, const float* g, float* buf, size_t n, const int64_t* step, const float* lr_dev, float lr, float mu,
             float dampening, float wd, int nesterov, float grad_scale, hipStream_t st);
// The guard block of the clipped / guarded step (the layout of the C ABI's egx_guard_block; grad_guard.hip writes it, the twins below read it)
struct GuardBlock {
    double norm; float coef; int32_t apply; int64_t steps, skipped, clipped;
};
// train.hip: the bump and the updates behind a guard (no store when guard->apply == 0; grad_scale = guard->coef; lr = *lr_dev, or lr by value)
int counter_add_gated(int64_t* c, int64_t inc, const GuardBlock* guard, hipStream_t st);
int lr_update_gated(int kind, long long warmup, long long t_total, long long T_max, double cycles, const double* factors, long long n_factors,
                    int64_t* step, const double* base_lr, int n_groups, float* lr_out, const GuardBlock* guard, hipStream_t st);
int adam_step_guarded(float* p, const float* g, float* m, float* v, size_t n, const int64_t* step, const float* lr_dev, float lr, float b1,
                      float b2, float eps, float wd, int decoupled, const GuardBlock* guard, hipStream_t st);
int sgd_step_guarded(float* p, const float* g, float* buf, size_t n, const int64_t* step, const float* lr_dev, float lr, float mu,
                     float dampening, float wd, int nesterov, const GuardBlock* guard, hipStream_t st);
// grad_guard.hip: the fp64 norm of G flat fp32 buffers in a fixed order, and the skip / clip decision (two launches per GRAD_NORM_TABLE buffers + 1)
constexpr int GRAD_NORM_TABLE = 32, GRAD_NORM_MAX_BLOCKS = 2048;
size_t grad_norm_scratch_bytes(const size_t* ns, int n_bufs);
int grad_norm(const float* const* bufs, const size_t* ns, int n_bufs, void* scratch, size_t scratch_bytes, double max_norm, int has_max_norm,
              int skip_nonfinite, GuardBlock* guard, hipStream_t st);

// seg_ce.hip: the LTA criterion (per-(future step, head) mean cross-entropies summed, top-k counts, d loss / d logits) in one launch
constexpr int SEG_CE_MAX_HEADS = 4, SEG_CE_MAX_KS = 4, SEG_CE_MAX_CLASSES = 2048, SEG_CE_MAX_ROWS = 1 << 28;
size_t segmented_ce_scratch_bytes(int B, int Z, int H, int n_ks);
int segmented_ce(const float* logits, int ld, const int64_t* target, int B, int Z, int H, const int* col0, const int* C, const int* ks,
                 int n_ks, float* loss, float* loss_terms, int* n_valid, int* correct, float* dlogits, void* scratch, hipStream_t st);
// host helpers of the one-launch criteria (seg_ce.hip). batch_chunks: the B clips as at most max_chunks chunks of at least `waves` clips.
// check_head_windows (EGX_CHECK style, 0 or 1): every head h is a window [col0[h], col0[h] + C[h]) of 1 .. SEG_CE_MAX_CLASSES columns inside
// a row of ld, and no two windows overlap.
void batch_chunks(int B, int max_chunks, int waves, int* chunk, int* nchunks);
int check_head_windows(const char* who, int ld, int H, const int* col0, const int* C);

// lta_val.hip: the LTA validation step (K sampled futures per clip and head, prefix edit distances, their sums) in one launch
constexpr int LTA_VAL_MAX_K = 8, LTA_VAL_MAX_Z = 64;
int lta_validate(const float* logits, int ld, const int64_t* labels, int B, int Z, int H, const int* col0, const int* C, int K, uint64_t seed,
                 const uint64_t* seed_ptr, const int64_t* preds_in, int64_t* preds, int* min_dist, int64_t* dist_sum, hipStream_t st);

// keyframe.hip: the PNR keyframe criterion (BCE / masked CE on the T frame logits of a clip), keyframe distance and accuracy in one launch
constexpr int KEYFRAME_MAX_T = 64, KEYFRAME_MAX_V = 2048, KEYFRAME_MAX_ROWS = 1 << 28;
enum KeyframeKind { KEYFRAME_BCE = 0, KEYFRAME_CE = 1, KEYFRAME_METRIC = 2 };       // the values of the C ABI's EGX_KF_* enum
size_t keyframe_scratch_bytes(int B);
int keyframe_criterion(const float* logits, int ld, int B, int T, const int* cols, int V, int kind, const float* target, const int64_t* label,
                       const int64_t* state_change, const double* fps, const int64_t* clip_start, const int64_t* clip_end,
                       const int64_t* pnr_frame, float* loss, float* loss_rows, float* dlogits, int* pred, int* label_frame, int* counts,
                       double* dist, double* dist_sum, void* scratch, hipStream_t st);

// seq_ce.hip: the EgoT2-g multi-task criterion (per-task mean cross-entropies times their ratios, word-to-label metrics, d loss / d logits)
// in one launch. SeqCeTask has the fields of the C ABI's egx_seq_task.
constexpr int SEQ_CE_MAX_TASKS = 8, SEQ_CE_MAX_CLASSES = 2048, SEQ_CE_MAX_SY = 64, SEQ_CE_MAX_ROWS = 1 << 22;
struct SeqCeTask {
    const float* logits; long long stride_b, stride_s;
    int B, sy;
    const int64_t* target; long long target_stride_b, target_stride_s;
    float ratio;
    float* d_logits;
    const int* word_label;
    const int64_t* labels; long long labels_stride_b, labels_stride_s;
    int* pred;
};
size_t sequence_ce_scratch_bytes();
int sequence_ce(const SeqCeTask* tasks, int T, int V, int* result, void* scratch, hipStream_t st);

// segment_ap.hip: the TTM / LAM validation epoch (merged per-row scores, a stable radix sort, both classes' average precision, confusion
// counts). One scratch holds the persistent per-row state (zero = empty) and the sort / scan work area, carved for `capacity` rows.
constexpr int SEG_AP_TILE = 4096, SEG_AP_MAX_ROWS = 1 << 24;
constexpr size_t SEGMENT_AP_RESULT_BYTES = 7 * 8 + 4 * 8;          // int64 n, n_pos, TP, FN, FP, TN, n_nonfinite | fp64 AP0, AP1, mAP, acc
size_t segment_ap_scratch_bytes(int capacity);
int segment_scores_update(const float* logits, int ld, int B, const int64_t* slots, int slot0, const int64_t* labels, int capacity,
                          void* scratch, hipStream_t st);
int segment_ap(int N, int capacity, void* scratch, float* score, int* order1, int* order0, void* result, hipStream_t st);

// view_ensemble.hip: the test epoch of the action-recognition translators (multi-view ensemble per video, top-k errors over the videos).
// One state holds the header (arrival counter, dropped clips), the per-video labels, view counts and rows, and the count partials; all zero =
// empty. `offsets` (optional, 3 words): byte offsets of the labels (int64 (capacity, H)), the view counts (int32 (capacity)) and the rows
// (fp32 (capacity, sum C)).
constexpr int VIEW_ENS_SUM = 0, VIEW_ENS_MAX = 1, VIEW_ENS_MAX_BATCH = 1 << 16;
size_t view_ensemble_state_bytes(int capacity, int H, const int* C, size_t* offsets);
int view_ensemble_update(const float* preds, int ld, int B, int H, const int* col0, const int* C, const int64_t* labels, const void* slots,
                         int slot_bytes, int slot0, int method, int capacity, void* state, hipStream_t st);
int view_ensemble_topk(int n, int capacity, int H, const int* C, const int* ks, int n_ks, void* state, int* rank, int* pred, int* result,
                       hipStream_t st);

// decoder.hip
struct SmallAttnParams {
    const float* q; const float* k; const float* v;
    int ldq, ldk, ldv;
    float* o; int ldo;                  // forward output
    const float* d_o;                   // backward input (same ld as o)
    float* dq; float* dk; float* dv;    // backward outputs (same ld as q / k / v)
    int B, Sq, Sk, H, dh, causal;
    float scale;
    uint64_t drop_key; uint32_t drop_thresh; float drop_inv;
};
int small_attention_fwd(SmallAttnParams p, hipStream_t st);
int small_attention_bwd(SmallAttnParams p, hipStream_t st);
int embed_pos_fwd(const int64_t* tok, const float* emb, const float* pe, int pe_stride, float scale, float* out, int B, int sy,
                  int d, int V, uint64_t key, uint32_t thresh, float inv, hipStream_t st);
int embed_pos_bwd(const int64_t* tok, const float* dy, float* d_emb, float scale, int B, int sy, int d, int V, uint64_t key,
                  uint32_t thresh, float inv, hipStream_t st);
int relu_mask(float* dy, const float* y, size_t n, hipStream_t st);
int gelu_fwd(const float* z, float* h, size_t n, hipStream_t st);
int gelu_bwd(const float* z, const float* dh, float* dz, size_t n, hipStream_t st);

// Device-resident dropout seed outside the per-clip kernels: table[(layer - layer0) * 8 + site] = site_key(*seed, layer, site) for
// `nlayer` layers, computed on the stream by one small launch (advance != 0: *seed = lcg(*seed) first - the training forward).
// Kernels then receive the ADDRESS of their key (common.h resolve_key), so a captured hipGraph draws fresh masks per replay.
constexpr int DROP_KEY_SLOTS = 8;
int derive_keys(uint64_t* seed, uint64_t* table, uint32_t layer0, int nlayer, int advance, hipStream_t st);
static inline uint64_t key_slot(const uint64_t* table, uint32_t layer_rel, uint32_t site) {
    return (uint64_t)(uintptr_t)(table + (size_t)layer_rel * DROP_KEY_SLOTS + site);
}

}  // namespace egx
