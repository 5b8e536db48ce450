// The encoder's self-attention weights as an output (enc_attn_weights.hip) as the host drivers see them.
#pragma once
#include "common.h"

namespace egx {

constexpr int SW_ROWS = 16;         // query rows of a workgroup
constexpr int SW_MAXS = 512;        // tokens of a clip (the limit of the tiled and wide attention)
constexpr int SW_MAXSEG = 16;       // segments of a clip in the per-task sums

// One layer of a batch. Clip b's S_b = clamp(rowtab[b * tab_stride + 1], 0, S) tokens are rows [rowtab[b * tab_stride] * row_mul, + S_b) of
// q and k (null table: rows b * clip_rows, S_b = S). The public table is int[B][2] (tab_stride 2, row_mul 1); the d = 128 ragged batch table
// is read in place (tab_stride = its record length, row_mul 48: the record holds the clip's first 48-row tile). segtab[b * seg_stride + t] is
// the length of clip b's segment t (public: seg_stride K).
struct SelfWParams {
    const void* q; const void* k; int ldq, ldk;     // row stride in elements; head h at columns [h * dh, (h + 1) * dh)
    const int* rowtab; int tab_stride, row_mul;
    long long clip_rows;
    const int* segtab; int seg_stride, K;
    int fixed_segs, seg_fixed[SW_MAXSEG];           // null segtab with fixed_segs: every clip has these K lengths (a uniform encoder call)
    float* w; int ldw;                              // row b * S + i, S entries written; null: not written
    float* seg;                                     // (B, S, K); null: not computed
    int B, H, S;
    float scale, inv_h;
};
int self_weights(SelfWParams p, int dh, bool f32, hipStream_t st);      // host checks first (no device work on a refusal), then one launch
// one launch per layer selected by `layer_mask` (bit l), in layer order: layer l's Q rows at qkv0 + l * layer_bytes, its K rows d_model
// elements behind them; the n-th selected layer writes w_out + n * B * S * S and seg_out + n * B * S * K (p.w / p.seg: null or the bases)
int self_weights_layers(SelfWParams p, const void* qkv0, size_t layer_bytes, int d_model, int L, uint64_t layer_mask, bool f32, hipStream_t st);

// One product of the attention rollout: out = A_l . prev with A_l = (w_l + I) / 2 (prev null: out = A_l), per clip, over the clip's
// rowlen[b] tokens (null: S); zeros beyond them.
struct RolloutParams {
    const float* w; const float* prev; float* out;  // (B, S, S) each; out null: not written
    float* seg;                                     // (B, S, K) or null
    const int* rowlen; int len_stride;              // DEVICE lengths (entry b * len_stride) or null
    const int* segtab; int seg_stride, K;
    int seg_fixed[SW_MAXSEG];                       // null segtab: every clip has these K lengths
    int B, S;
};
int rollout_step(const RolloutParams& p, hipStream_t st);
size_t rollout_scratch_bytes(int L, int B, int S);
int rollout(const float* w, int L, int B, int S, const int* rowlen, int len_stride, const int* segtab, int seg_stride, const int* seg_fixed, int K,
            void* scratch, float* out, float* seg_out, hipStream_t st);

}  // namespace egx
