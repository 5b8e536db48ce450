// Host side of the d = 128 kernels (one-launch, cut, sliced, tiled, ragged) as encoder.hip sees it (see fused_host.hip).
#pragma once
#include "../../include/egot2x.h"
#include "common.h"

namespace egx {

// ---- workspace plan (make_plan, encoder.hip) ---------------------------------------------------------------------
struct LayerOff {
    size_t x_in, qkv, lse, attn_o, res1, stats1, x1, hid, res2, stats2;
};
struct Plan {
    int B = 0, S = 0, d = 0, H = 0, dff = 0, L = 0, nseg = 0;
    int vB = 0, tpc = 1;    // fused kernels: workgroups ("virtual clips") and 48-token tiles per clip; vB = B unless the tiled mode (S > 48) is planned
    size_t N = 0;
    int seg_off[EGX_MAX_SEGMENTS];
    size_t seg_pre[EGX_MAX_SEGMENTS], seg_stats[EGX_MAX_SEGMENTS];
    LayerOff layer[64];
    size_t saved_bytes = 0;
    // scratch
    size_t s_dA = 0, s_dB = 0, s_dqkv = 0, s_dhid = 0, s_slab = 0, slab_bytes = 0, s_det = 0, det_bytes = 0;
    size_t scratch_bytes = 0;
};
int make_plan(const egx_config* cfg, const egx_segment* segs, int B, Plan& pl);

static inline float* fptr(void* base, size_t off) { return (float*)((char*)base + off); }
static inline const float* cfptr(const void* base, size_t off) { return (const float*)((const char*)base + off); }

struct Drop {
    uint64_t key = 0;
    uint32_t thresh = 0;
    float inv_keep = 1.f;
};
static inline Drop make_drop(int training, float p, uint64_t seed, uint32_t layer, uint32_t site) {
    Drop dr;
    if (training && p > 0.f) {
        dr.key = site_key(seed, layer, site);
        dr.thresh = drop_threshold(p);
        dr.inv_keep = p < 1.f ? 1.f / (1.f - p) : 0.f;
    }
    return dr;
}
// dx[M,K] = dy[M,N] W[N,K]  (+ mask/scale, + residual) on the generic GEMM (encoder.hip): the ragged backward's feature gradient
int linear_dx(const float* dy, const float* W, float* dx, int M, int N, int K, const float* mask, float mask_scale,
              const float* residual, int compute, hipStream_t st, void* slab = nullptr, size_t slab_bytes = 0);

// ---- what the dispatch and the queries of encoder.hip ask of the d = 128 paths -----------------------------------------------
bool packed_feats(const egx_segment* segs, int nseg);
bool fused_ok(const egx_config* cfg, const egx_segment* segs, const Plan& pl);      // per-clip kernels: S <= 48
bool tiled_ok(const egx_config* cfg, const egx_segment* segs, const Plan& pl);      // the same kernels over 48-token tiles: 48 < S <= 512
int fused_slices(const Plan& pl, int compute);
bool fused_token_ce_ok(const egx_config* cfg, const Plan& pl);      // egx_config.token_ce, given that the per-clip kernels run
size_t fused_weight_cache_bytes(const egx_config* cfg, const egx_segment* segs, const Plan& pl);
// the larger of the per-clip and the tiled workspace, 0 where neither runs
void fused_workspace(const egx_config* cfg, const egx_segment* segs, const Plan& pl, size_t* saved, size_t* scratch);
int check_head(const egx_head* head);                                       // 0 without a head
int check_ce(const egx_ce* ce, bool with_head, const char* entry);          // 0 without egx_config.ce
int fused_path_fwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool tiled, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, float* tokens_out, float* logits_out, void* saved, int training,
                   uint64_t seed, hipStream_t st);
int fused_path_bwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool tiled, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, float* d_tokens, const float* d_logits, const void* saved, void* scratch,
                   const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads,
                   const egx_head_grads* head_grads, int training, uint64_t seed, hipStream_t st);
// the self-attention weights of a d = 128 call from the Q | K | V rows its forward left in `saved` (egx_encoder_self_weights, encoder.hip):
// a uniform per-clip / tiled call, and a ragged call (egx_ragged_train_fwd's layout; *S_out: the longest clip)
int fused_self_weights(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool tiled, const void* saved, uint64_t layer_mask,
                       float* w_out, float* seg_out, hipStream_t st);
int ragged_self_weights(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, const void* saved, uint64_t layer_mask,
                        float* w_out, float* seg_out, hipStream_t st);

}  // namespace egx
