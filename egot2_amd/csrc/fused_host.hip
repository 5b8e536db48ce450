// Host side of the d = 128 kernels: workspace layouts, mode policy and launch sequences of the per-clip (one-launch, cut, sliced) and the
// tiled mode, and the ragged batches, which are tiled batches with a batch table and their own workspace view. Like encoder.hip it only
// enqueues kernels on the caller's stream: no allocation, no synchronisation.
#include <string.h>
#include <vector>

#include "../../include/egot2x.h"
#include "common.h"
#include "kernels.h"
#include "fused.h"
#include "fused_host.h"
#include "enc_attn_weights.h"

namespace egx {

// ---- fused per-clip path (fused.hip) ---------------------------------------------------------------
bool packed_feats(const egx_segment* segs, int nseg) {
    for (int i = 0; i < nseg; ++i)
        if (segs[i].feat_bf16 || segs[i].pool > 1) return true;
    return false;
}
bool fused_ok(const egx_config* cfg, const egx_segment* segs, const Plan& pl) {
    if (pl.nseg > FUSED_MAX_SEG || pl.L > FUSED_MAX_LAYERS || pl.L < 1) return false;
    if (packed_feats(segs, pl.nseg)) return false;
    int d_in[EGX_MAX_SEGMENTS], T[EGX_MAX_SEGMENTS];
    bool hp[EGX_MAX_SEGMENTS];
    for (int i = 0; i < pl.nseg; ++i) { d_in[i] = segs[i].d_in; T[i] = segs[i].T; hp[i] = segs[i].proj_w != nullptr; }
    return fused_supported(pl.d, pl.H, pl.dff, pl.S, pl.nseg, d_in, T, hp);
}
// Fragment-packed weight copies (written by the forward, reused by the backward): per segment the projection, per layer each matrix in
// both orientations. They live in the caller's persistent weight cache (egx_config.weight_cache, ABI v15) or in the `packs` section of `saved`.
struct FusedPackLayout {
    void* proj[EGX_MAX_SEGMENTS];
    struct Layer { void* in_w; void* in_wt; void* out_w; void* out_wt; void* lin1_w; void* lin1_wt; void* lin2_w; void* lin2_wt; } layer[FUSED_MAX_LAYERS];
    size_t bytes;
};
static FusedPackLayout fused_pack_layout(const egx_config* cfg, const egx_segment* segs, const Plan& pl, char* base) {
    FusedPackLayout L;
    memset(&L, 0, sizeof(L));
    int bf = cfg->compute;      // packed element format follows the compute mode (fused_dev.h)
    size_t cur = 0;
    auto take_p = [&](int R, int K) -> void* { void* q = base ? base + cur : nullptr; cur += align_up(packed_bytes(R, K, bf), 256); return q; };
    for (int i = 0; i < pl.nseg; ++i) L.proj[i] = take_p(pl.d, segs[i].d_in);
    for (int l = 0; l < pl.L && l < FUSED_MAX_LAYERS; ++l) {
        L.layer[l].in_w = take_p(3 * pl.d, pl.d);
        L.layer[l].in_wt = take_p(pl.d, 3 * pl.d);
        L.layer[l].out_w = take_p(pl.d, pl.d);
        L.layer[l].out_wt = take_p(pl.d, pl.d);
        L.layer[l].lin1_w = take_p(pl.dff, pl.d);
        L.layer[l].lin1_wt = take_p(pl.d, pl.dff);
        L.layer[l].lin2_w = take_p(pl.d, pl.dff);
        L.layer[l].lin2_wt = take_p(pl.dff, pl.d);
    }
    L.bytes = cur;
    return L;
}
// The FFN hidden activation H (forward, `saved`) and its gradient dH (backward, scratch) are handed to the weight-gradient kernel as operand
// tiles instead of being recomputed there (ffn_dw_kernel, the recompute variant, is kept as the egx_ffn_dw unit hook): the FFN loops of the
// clip kernels store them unconditionally.
static size_t fused_hid_total(const egx_config* cfg, const Plan& pl) { return align_up((size_t)pl.L * fused_hid_bytes(pl.vB, pl.dff, cfg->compute == EGX_BF16), 256); }
// split / bf16 mode: the FFN input x1 of every layer is kept as bf16 planes
static bool split_planes(const egx_config* cfg) { return cfg->compute == EGX_F32_SPLIT || cfg->compute == EGX_BF16; }
static size_t plane_elem_bytes(const egx_config* cfg) { return cfg->compute == EGX_BF16 ? 2 : 6; }   // one bf16 plane, or the three parts
constexpr int SLICE_LAYOUT_CUS = 304;       // the largest compute-unit count of the supported parts (gfx942: 304, gfx950: 256) bounds the slice count the layout
                                            // provides for (512 reserved a two-slice exchange buffer, 12.6 MB per layer, for the B = 256 headline batch)
static int fused_slices_layout(const Plan& pl) {
    const int nit = pl.dff / 128, bq = (pl.B + 7) / 8 * 8;
    int n = 1;
    while (n * 2 <= 8 && nit % (n * 2) == 0 && bq * n * 2 <= SLICE_LAYOUT_CUS) n *= 2;
    return n;
}
// the exchange buffer of the sliced mode (L, B, n, 48, d): one in `saved` for the forward, one in the backward's scratch
static size_t sliced_xchg_bytes(const Plan& pl) {
    const int n = fused_slices_layout(pl);
    return n > 1 ? align_up((size_t)pl.L * pl.B * n * FUSED_TOK_PAD * pl.d * 4, 256) : 0;
}

// ---- the `saved` block of every d = 128 call ----------------------------------------------------------------------------------------------
// One layout for the one-launch, cut, sliced, tiled and ragged calls, built once per call by saved_layout() and read by every launch
// sequence, workspace query and test hook below. vB: workgroups (clips, or 48-token tiles), grid = 48 vB rows, N: tokens (B S; ragged: sum_b S_b).
// The sections in order, each 256-byte aligned; one a layout does not have takes no bytes, its offset stays 0 and nothing reads it:
//   res          fp32 [pre][res1, res2 per layer], (N, d) each: the pre-LN rows and the residual sums (res_index)
//   relu_bits    ReLU / dropout sign bits of the FFN hidden: one u32 per (layer, workgroup, hidden block, lane)
//   packs        the fragment-packed weights; reserved also when they live in egx_config.weight_cache
//   hid          the FFN hidden tiles H of every layer (fused_hid_bytes: fp32, or bf16 in bf16 mode)
//   x1p          f32s / bf16 only: the FFN input x1 of every layer as bf16 planes (L, 3 or 1, grid, d)
//   xin          the input of every layer, fp32 (L, N, d)                    } the backward loads them
//   qkv          its Q | K | V rows on the tile grid, fp32 (L, grid, 3d)     } instead of recomputing
//  per-clip layout (S <= 48) only:
//   x1f          x1 = LayerNorm1 output of every layer as fp32 rows (L, N, d): what the cut mode's attention-side launch hands to ffn_fwd_kernel
//   xchg         where the shape admits slices: the forward's exchange buffer (L, B, n, 48, d)
//   xflags_fwd, xflags_bwd   then the "published" words of the forward and of the backward, (L, B, 8) each (one per layer, clip and slice: SLICE_MAX = 8)
//  tiled and ragged layouts only (attention runs between the tile launches):
//   attn         every layer's attention output, fp32 (L, N, d)
//   lse          every layer's log-sum-exp rows, H per token: (L, H, N); a uniform batch reads it as (L, B, H, S), N = B S
//   tokens       the last layer's dense tokens (N, d), then the token means (B, d) of a translator call
//  ragged layouts only:
//   tab, efft    the device copy of the batch table (fused.h RAGGED_REC); capacity plan only: the effective targets, int64 (B)
struct SavedLayout {
    char* base;                 // the caller's block (null in a size query)
    size_t res, relu_bits, packs, hid, x1p, xin, qkv, x1f, xchg, xflags_fwd, xflags_bwd, attn, lse, tokens, tab, efft, bytes;
    size_t relu_layer_words, hid_layer, x1p_layer, qkv_layer, lse_layer_floats;     // one layer of the section (bytes unless named otherwise)
    size_t res_block, flag_words;       // floats of one (N, d) block of `res`; words of xflags_fwd and of xflags_bwd each
    FusedPackLayout pack;               // resolved: in the weight cache, else in `packs` (null pointers in a size query)
    char* at(size_t off) const { return base + off; }
    size_t res_index(int l, int which) const { return (size_t)(1 + 2 * l + which) * res_block; }    // floats in front of block `which` (0 = res1, 1 = res2) of layer l
};
// tiled: the layout of the tile grid (vp planned by plan_tiled, or a ragged plan: tab_words > 0, and efft_rows > 0 for the capacity plan)
static SavedLayout saved_layout(const egx_config* cfg, const egx_segment* segs, const Plan& vp, bool tiled, const void* saved = nullptr,
                                size_t tab_words = 0, size_t efft_rows = 0) {
    SavedLayout s;
    memset(&s, 0, sizeof(s));
    s.base = (char*)const_cast<void*>(saved);
    const size_t nd = vp.N * vp.d * 4, grid = (size_t)vp.vB * FUSED_TOK_PAD;
    s.res_block = vp.N * vp.d;
    s.relu_layer_words = (size_t)vp.vB * (vp.dff / 32) * 64;
    s.hid_layer = fused_hid_bytes(vp.vB, vp.dff, cfg->compute == EGX_BF16);
    s.x1p_layer = split_planes(cfg) ? grid * vp.d * plane_elem_bytes(cfg) : 0;
    s.qkv_layer = grid * 3 * vp.d * 4;
    size_t cur = 0;
    s.res = take(cur, (1 + 2 * vp.L) * nd);
    s.relu_bits = take(cur, vp.L * s.relu_layer_words * 4);
    s.pack = fused_pack_layout(cfg, segs, vp, cfg->weight_cache ? (char*)cfg->weight_cache : saved ? s.base + cur : nullptr);
    s.packs = take(cur, s.pack.bytes);
    s.hid = take(cur, fused_hid_total(cfg, vp));
    s.x1p = take(cur, vp.L * s.x1p_layer);
    s.xin = take(cur, vp.L * nd);
    s.qkv = take(cur, vp.L * s.qkv_layer);
    const bool per_clip = !tiled, sliced = per_clip && fused_slices_layout(vp) > 1, ragged = tab_words > 0, capacity = efft_rows > 0;
    if (per_clip) s.x1f = take(cur, vp.L * nd);
    if (sliced) {
        // The exchange buffer and the flag words are laid out for the LARGEST slice count the shape admits on any device and under any
        // EGX_FFN_SLICES (fused_slices_layout: a function of the shape alone), so that the workspace query, the forward and the backward —
        // which each pick their own run-time count <= that bound (fused_slices) — agree on every offset whatever the environment or the
        // current device did between the calls (a changed count used to move the flag words past the caller's buffer).
        s.flag_words = (size_t)vp.L * vp.B * 8;
        s.xchg = take(cur, sliced_xchg_bytes(vp));
        s.xflags_fwd = take(cur, 2 * s.flag_words * 4);
        s.xflags_bwd = s.xflags_fwd + s.flag_words * 4;
    }
    if (tiled) {
        s.lse_layer_floats = (size_t)vp.H * vp.N;
        s.attn = take(cur, vp.L * nd);
        s.lse = take(cur, vp.L * s.lse_layer_floats * 4);
        s.tokens = take(cur, (vp.N + (size_t)vp.B) * vp.d * 4);
    }
    if (ragged) s.tab = take(cur, tab_words * sizeof(int));
    if (capacity) s.efft = take(cur, efft_rows * sizeof(int64_t));
    s.bytes = cur;
    return s;
}
// Cut mode (ffn_cut.hip): the per-clip kernels cut at the FFN, whose loops run as launches of their own with eight waves per clip. One
// workgroup per clip only (the sliced mode of small batches keeps the one-launch kernels). Policy = where it measured faster on MI355X
// (profiles/r05_cut_ab.txt): the f32s arithmetic (six MFMAs per K-block: the hidden loops are 55 % of the one-launch kernels and gain
// 25 % from the second wave per SIMD) with one layer per launch pair and the reference's d_ff; bf16's short loops and deeper / narrower
// stacks pay more for the two extra launches per layer than the loops gain. EGX_FFN_CUT=1 forces it wherever it is supported (the
// parity tests run every mode through it), =0 keeps the one-launch kernels.
static bool use_cut(const Plan& pl, int n_slices, bool tiled, int compute) {
    if (tiled || n_slices != 1 || !ffn_cut_supported(pl.dff)) return false;
    if (tuning().ffn_cut >= 0) return tuning().ffn_cut != 0;
    return compute == EGX_F32_SPLIT && pl.L == 1 && pl.dff >= 1024;
}
// ---- sliced mode (small batches): n workgroups per clip, each 1 / n of the FFN hidden blocks (FusedFwdParams::n_slices). Only when
// the workgroups of the launch can all be resident at once: round_up(B, 8) * n <= CUs (a performance rule, not a protocol: a slice
// whose partial sum does not arrive within 100 us is computed by the waiting workgroup itself, fused_dev.h).
// EGX_FFN_SLICES=1 turns it off, =2 / 4 / 8 caps n.
static int device_cus() {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (!cus[dev]) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cus[dev] = v;
    }
    return cus[dev];
}
// EGX_SLICE_DROP=<hex mask> (testing aid): the workgroups of those slices leave at once; the others must compute their share
static int slice_drop_mask(int n) {
    if (!tuning().has_drop) return 0;
    const int m = (int)tuning().slice_drop & ((1 << n) - 1);
    return m == (1 << n) - 1 ? 0 : m;      // at least one slice has to run
}
// The exchange is built on gfx942 / gfx950 behaviour (write-through relaxed agent-scope atomics, s_waitcnt ordering; fused_dev.h): any other
// device runs one workgroup per clip.
static bool device_slicing_ok() {
    static int ok[64] = {0};        // 0 unknown, 1 yes, 2 no
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (!ok[dev]) {
        hipDeviceProp_t pr;
        ok[dev] = (hipGetDeviceProperties(&pr, dev) == hipSuccess && (strncmp(pr.gcnArchName, "gfx950", 6) == 0 || strncmp(pr.gcnArchName, "gfx942", 6) == 0)) ? 1 : 2;
    }
    return ok[dev] == 1;
}
int fused_slices(const Plan& pl, int compute) {
    if (!device_slicing_ok()) return 1;
    const bool e = tuning().has_slices;            // (EGX_FFN_SLICES; the LAYOUT does not depend on it)
    // measured at B = 32 (profiles/r04_sliced.txt): the exchange costs ~10 us per kernel; with bf16's short FFN loop eight slices lose to four
    int cap = e ? tuning().slices_cap : (compute == EGX_BF16 ? 4 : 8);
    if (cap < 1) cap = 1;
    const int cus = device_cus(), nit = pl.dff / 128, bq = (pl.B + 7) / 8 * 8;
    int n = 1;
    while (n * 2 <= cap && n * 2 <= 8 && nit % (n * 2) == 0 && bq * n * 2 <= cus) n *= 2;
    if (compute == EGX_BF16 && n == 2 && !e) n = 1;     // two slices of the short bf16 loop do not pay for the exchange (B = 128: +3 % / -3 %)
    const int cap_layout = fused_slices_layout(pl);
    return n < cap_layout ? n : cap_layout;
}

// ---- tiled mode (d = 128, 48 < S <= 512): the same kernels over 48-token tiles, attention between the launches
// sizes of the tile grid: vB workgroups ("virtual clips"); B / N stay the real clips / tokens
static Plan plan_tiled(Plan pl) { pl.tpc = cdiv(pl.S, FUSED_TOK_PAD); pl.vB = pl.B * pl.tpc; return pl; }
bool tiled_ok(const egx_config* cfg, const egx_segment* segs, const Plan& pl) {
    if (pl.d != 128 || pl.H != 4 || pl.dff % 128 != 0 || pl.dff < 128) return false;
    if (pl.S <= FUSED_TOK_PAD || pl.S > TILED_MAX_S) return false;
    if (pl.nseg > FUSED_MAX_SEG || pl.L > FUSED_MAX_LAYERS || pl.L < 1) return false;
    if (packed_feats(segs, pl.nseg) || cfg->p_feat > 0.f) return false;
    if (cfg->compute != EGX_BF16 && cfg->compute != EGX_F32_SPLIT) return false;     // exact-fp32 MFMA: the generic kernels
    if (cfg->out_tokens != 0 && cfg->out_tokens != pl.S) return false;
    for (int i = 0; i < pl.nseg; ++i)
        if (!segs[i].proj_w || segs[i].d_in % 128 != 0) return false;
    return true;
}

// scratch of the fused backward: per layer the operands of the weight-gradient kernels, then d(seg), the per-clip
// partial sums, and the slab area shared by ffn_dw and the split-K GEMMs.
struct FusedBwdScratch {
    size_t x1[FUSED_MAX_LAYERS], g2[FUSED_MAX_LAYERS], attn_o[FUSED_MAX_LAYERS], g1[FUSED_MAX_LAYERS], dqkv[FUSED_MAX_LAYERS];
    size_t dseg[EGX_MAX_SEGMENTS];
    size_t partials, slabs, slab_bytes, dhid, bytes, dx0;
    size_t sdw_tiles, sdw_bytes;            // round 6: the tiles small_dw leaves for the fixed-order tail launch (NOT the shared slab area: layer 0's FFN slabs live there)
    size_t dy1, dxin;                       // cut mode: what the FFN-side and the attention-side launches of the backward hand each other
    size_t xchg;                            // sliced mode only
    size_t datt, dres, delta, dtok;         // tiled mode only
    size_t ffn_slab[FUSED_MAX_LAYERS];      // slab area of each layer's FFN weight gradient (layer 0: `slabs`): one reduction launch sums them all
    int P;
};
// The prefix both backwards share, up to dH; returns the cursor. seg_rows[i]: rows of d(seg i) (uniform: B T_i; ragged: the packed sum_b T_{b,i}).
static size_t bwd_scratch_prefix(FusedBwdScratch& s, const egx_config* cfg, const egx_segment* segs, const Plan& pl, const size_t* seg_rows, int head_n_out) {
    memset(&s, 0, sizeof(s));
    size_t cur = 0;
    const size_t nd = pl.N * pl.d * 4;
    const size_t nd3 = (size_t)pl.vB * FUSED_TOK_PAD * pl.d * 6;        // g2 leaves as three bf16 planes on the 48-row clip / tile grid in split mode
    for (int l = 0; l < pl.L && l < FUSED_MAX_LAYERS; ++l) {
        s.x1[l] = take(cur, nd); s.g2[l] = take(cur, nd3); s.attn_o[l] = take(cur, nd);
        s.g1[l] = take(cur, nd); s.dqkv[l] = take(cur, 3 * nd);
    }
    for (int i = 0; i < pl.nseg; ++i) s.dseg[i] = take(cur, seg_rows[i] * pl.d * 4);
    s.P = fused_partial_len(pl.L, pl.nseg) + fused_head_partial_len(head_n_out);
    s.partials = take(cur, (size_t)pl.vB * s.P * 4);
    size_t slab = ffn_dw_scratch_bytes((int)pl.N, pl.dff, nullptr);
    slab = size_max(slab, gemm_scratch_bytes(2, 3 * pl.d, pl.d, (int)pl.N));
    slab = size_max(slab, gemm_scratch_bytes(2, pl.d, pl.d, (int)pl.N));
    for (int i = 0; i < pl.nseg; ++i) slab = size_max(slab, gemm_scratch_bytes(2, pl.d, segs[i].d_in, (int)seg_rows[i]));
    const size_t sdw_bytes = (size_t)(512 + SMALL_DW_MAX * 16) * 64 * 128 * sizeof(float);   // small_dw's tiles: one per workgroup
    slab = size_max(slab, sdw_bytes);       // (deterministic small_dw of the staged backward leaves them in the slab area)
    s.slab_bytes = slab;
    s.slabs = take(cur, slab);
    s.ffn_slab[0] = s.slabs;
    for (int l = 1; l < pl.L && l < FUSED_MAX_LAYERS; ++l) s.ffn_slab[l] = take(cur, ffn_dw_scratch_bytes((int)pl.N, pl.dff, nullptr));
    s.sdw_bytes = sdw_bytes;
    s.sdw_tiles = take(cur, s.sdw_bytes);
    s.dhid = take(cur, fused_hid_total(cfg, pl));
    return cur;
}
static FusedBwdScratch fused_bwd_scratch(const egx_config* cfg, const egx_segment* segs, const Plan& pl, int head_n_out = 0) {
    FusedBwdScratch s;
    size_t seg_rows[EGX_MAX_SEGMENTS];
    for (int i = 0; i < pl.nseg; ++i) seg_rows[i] = (size_t)pl.B * segs[i].T;
    size_t cur = bwd_scratch_prefix(s, cfg, segs, pl, seg_rows, head_n_out);
    const size_t nd = pl.N * pl.d * 4;
    s.dx0 = take(cur, nd);         // d(token-prep output) behind its dropout mask (learned positional table gradient)
    s.dy1 = take(cur, nd); s.dxin = take(cur, nd);
    if (pl.tpc > 1 || pl.S > FUSED_TOK_PAD) {       // tiled mode: d(attention output), the residual gradient, delta, d(tokens) of a translator call
        s.datt = take(cur, nd); s.dres = take(cur, nd);
        s.delta = take(cur, (size_t)pl.B * pl.H * pl.S * 4);
        s.dtok = take(cur, nd);
    } else {
        s.xchg = take(cur, sliced_xchg_bytes(pl));
    }
    s.bytes = cur;
    return s;
}

// ---- parameters of the clip / tile kernels, shared by the uniform calls (fused_path_fwd / fused_path_bwd) and the ragged ones -------
// The descriptor list of the packing launch: a weight-cache hit (egx_config.weight_cache_valid) packs nothing, the copy is in place.
struct Packer {
    PackParams& pk;
    bool cache_hit;
    const void* operator()(const float* src, void* dst, int R, int K, int ld, int transpose, float scale = 1.f) {
        if (cache_hit) return dst;
        PackDesc& dsc = pk.d[pk.n++];
        dsc.src = src; dsc.dst = dst; dsc.R = R; dsc.K = K; dsc.ld = ld; dsc.transpose = transpose; dsc.scale = scale;
        return dst;
    }
};
// segment i as both directions read it; the forward (proj_wp: its packed projection) reads the features and the projection too
static void fill_seg(FusedSeg& fs, const egx_segment& s, int i, const void* proj_wp = nullptr) {
    if (proj_wp) { fs.feat = s.feat; fs.proj_wp = proj_wp; fs.proj_b = s.proj_b; }
    fs.add_vec = s.add_vec; fs.pos = s.pos; fs.T = s.T; fs.d_in = s.d_in; fs.pos_stride = s.pos_stride;
    fs.Tfull = s.T; fs.seg_id = i;
}
// a forward layer: packed weights and their transposed copies for the backward kernels (also when a weight cache is filled: a later
// backward reads them from there); the keep-scale of the FFN hidden dropout rides on the packed W1 (forward: relu(s (W1 x + b1)) =
// s relu(W1 x + b1)) and W2^T (backward: dH = alive ? s W2^T g : 0): the FFN epilogues of the clip kernels have no multiply
static void fill_layer(FusedLayer& fl, const egx_layer& w, const FusedPackLayout::Layer& P, int d, int dff, float ffn_scale, Packer& pack) {
    fl.in_proj_wp = pack(w.in_proj_w, P.in_w, 3 * d, d, d, 0); fl.in_proj_b = w.in_proj_b;
    fl.out_proj_wp = pack(w.out_proj_w, P.out_w, d, d, d, 0); fl.out_proj_b = w.out_proj_b;
    fl.lin1_wp = pack(w.lin1_w, P.lin1_w, dff, d, d, 0, ffn_scale); fl.lin1_b = w.lin1_b;
    fl.lin2_wp = pack(w.lin2_w, P.lin2_w, d, dff, dff, 0); fl.lin2_b = w.lin2_b;
    pack(w.in_proj_w, P.in_wt, d, 3 * d, d, 1);
    pack(w.out_proj_w, P.out_wt, d, d, d, 1);
    pack(w.lin1_w, P.lin1_wt, d, dff, d, 1);
    pack(w.lin2_w, P.lin2_wt, dff, d, dff, 1, ffn_scale);
    fl.norm1_w = w.norm1_w; fl.norm1_b = w.norm1_b; fl.norm2_w = w.norm2_w; fl.norm2_b = w.norm2_b;
}
// a backward layer's weights: the packed copies the forward left
static void fill_bwd_layer(FusedBwdLayer& fl, const egx_layer& w, const FusedPackLayout::Layer& P) {
    fl.in_proj_wp = P.in_w; fl.in_proj_wtp = P.in_wt; fl.out_proj_wtp = P.out_wt;
    fl.lin1_wp = P.lin1_w; fl.lin2_wtp = P.lin2_wt; fl.lin1_wtp = P.lin1_wt;
    fl.in_proj_b = w.in_proj_b; fl.lin1_b = w.lin1_b;
    fl.norm1_w = w.norm1_w; fl.norm1_b = w.norm1_b; fl.norm2_w = w.norm2_w; fl.norm2_b = w.norm2_b;
}
// the dropout sites of layer l (FusedLayer, FusedBwdLayer): one threshold and keep-scale, a key per site
template <class LayerT>
static void set_layer_drop(LayerT& fl, int training, float p, uint64_t seed, int l) {
    const Drop da = make_drop(training, p, seed, (uint32_t)l, SITE_ATTN);
    fl.attn_key = da.key; fl.attn_thresh = da.thresh; fl.drop_inv = da.inv_keep;
    fl.res_thresh = da.thresh; fl.ffn_thresh = da.thresh;
    fl.res1_key = make_drop(training, p, seed, (uint32_t)l, SITE_RES1).key;
    fl.ffn_key = make_drop(training, p, seed, (uint32_t)l, SITE_FFN).key;
    fl.res2_key = make_drop(training, p, seed, (uint32_t)l, SITE_RES2).key;
}

// ---- what encoder.hip asks -------------------------------------------------------------------------------------------------------
// egx_config.token_ce is evaluated by the per-clip kernels of the one-launch mode only (one workgroup per clip, no cut, no slices, no pooled head),
// with the arrival counter of the weight cache's control block
bool fused_token_ce_ok(const egx_config* cfg, const Plan& pl) {
    if (!cfg->weight_cache || cfg->deterministic) return false;
    if (pl.B > 4095) return false;      // (the arrival word: 12 bits of clips, 20 bits of correct frames)
    const int ns = fused_slices(pl, cfg->compute);
    return ns == 1 && !use_cut(pl, ns, false, cfg->compute);
}
// Bytes of the persistent packed-weight cache (egx_config.weight_cache): the fragment-packed copies of the per-clip / tiled kernels. The layout
// is a function of the model dimensions and the compute mode only (fused_pack_layout), so one buffer serves every batch size.
size_t fused_weight_cache_bytes(const egx_config* cfg, const egx_segment* segs, const Plan& pl) {
    if (pl.d != 128 || pl.nseg > FUSED_MAX_SEG || pl.L > FUSED_MAX_LAYERS || pl.L < 1 || pl.dff % 128 != 0) return 0;
    for (int i = 0; i < pl.nseg; ++i)
        if (!segs[i].proj_w || segs[i].d_in % 128 != 0) return 0;
    return align_up(fused_pack_layout(cfg, segs, pl, nullptr).bytes, 256) + 256;      // + the control block (FusedFwdParams::ce_ticket / tce_ticket)
}
void fused_workspace(const egx_config* cfg, const egx_segment* segs, const Plan& pl, size_t* saved, size_t* scratch) {
    *saved = 0; *scratch = 0;
    if (tiled_ok(cfg, segs, pl)) {
        const Plan vp = plan_tiled(pl);
        *saved = saved_layout(cfg, segs, vp, true).bytes;
        *scratch = fused_bwd_scratch(cfg, segs, vp, FUSED_HEAD_MAX_OUT).bytes;       // (the pooled head's partial-row section: sized for the largest head)
    }
    if (fused_ok(cfg, segs, pl)) {
        *saved = size_max(*saved, saved_layout(cfg, segs, pl, false).bytes);
        *scratch = size_max(*scratch, fused_bwd_scratch(cfg, segs, pl, FUSED_HEAD_MAX_OUT).bytes);
    }
}
int check_head(const egx_head* head) {
    EGX_CHECK(!(head && head->W) || (head->ln_w && head->ln_b && head->b && head->n_out >= 1 && head->n_out <= FUSED_HEAD_MAX_OUT),
              "head needs ln_w, ln_b, W, b and 1 <= n_out <= %d", FUSED_HEAD_MAX_OUT);
    return 0;
}
int check_ce(const egx_ce* ce, bool with_head, const char* entry) {
    EGX_CHECK(!ce || with_head, "egx_config.ce: the fused cross entropy needs the pooled head%s", entry);
    EGX_CHECK(!ce || (ce->target && ce->loss && ce->d_logits), "egx_config.ce: target, loss and d_logits must be set");
    return 0;
}

// ---- one driver for uniform and ragged batches -------------------------------------------------------------------------------------------
// What differs between the callers of the clip / tile kernels. A ragged batch is a tiled batch with a batch table and another workspace view.
struct TiledView {
    const SavedLayout* sl;                  // the saved block of the uniform call / the ragged workspace
    const int* rtab;                        // device batch table (fused.h RAGGED_REC); nullptr = uniform. Selects the pooled-head launch too
    int B_clips, tpc, S_clip;               // clips, tiles per clip (ragged: 0, the table has them), tokens of the (longest) clip
    bool tiled;
    int rot_mode;                           // hidden-block walk order of the FFN loops
    bool keys;                              // the forward hands on dropout keys, the device seed and its advance (all but ragged inference)
};
static TiledView uniform_view(const Plan& vp, const SavedLayout& SL, bool tiled) {
    TiledView v;
    memset(&v, 0, sizeof(v));
    v.sl = &SL;
    v.B_clips = vp.B; v.tpc = vp.tpc; v.S_clip = vp.S; v.tiled = tiled;
    v.rot_mode = FFN_ROT_XCD_STAGGER;
    v.keys = true;
    return v;
}

// The part of FusedFwdParams and of the packing launch every forward fills alike. Left to the caller: the output pointers, and of the
// uniform call seg[i].off / row0, the feature-dropout keys, out_T, the fused head and losses, the slices.
static void fill_fwd(FusedFwdParams& fp, PackParams& pk, const TiledView& v, const egx_config* cfg, const egx_segment* segs,
                     const Plan& vp, const float* ln_w, const float* ln_b, const egx_layer* layers, int training, uint64_t seed) {
    const int d = vp.d;
    const SavedLayout& SL = *v.sl;
    const FusedPackLayout& PL = SL.pack;
    memset(&fp, 0, sizeof(fp));
    // rewrite the weights into MFMA-fragment order (once per forward; they live behind the saved activations or in the weight cache)
    memset(&pk, 0, sizeof(pk));
    pk.mode = cfg->compute;
    fp.seed_ptr = v.keys ? cfg->seed_ptr : nullptr;
    pk.seed_advance = (cfg->advance_seed == 1 && fp.seed_ptr && training) ? const_cast<uint64_t*>(fp.seed_ptr) : nullptr;
    // weight cache valid (egx_config.weight_cache_valid): the packed copies of exactly these weights are in place, nothing is packed
    Packer pack{pk, cfg->weight_cache && cfg->weight_cache_valid};
    const Drop dffn = make_drop(training, cfg->p_drop, seed, 0, SITE_FFN);
    const float ffn_scale = dffn.thresh ? dffn.inv_keep : 1.f;      // (fill_layer)
    for (int i = 0; i < vp.nseg; ++i)
        fill_seg(fp.seg[i], segs[i], i, pack(segs[i].proj_w, PL.proj[i], d, segs[i].d_in, segs[i].d_in, 0));
    fp.n_heads = vp.H;
    for (int l = 0; l < vp.L; ++l) {
        fill_layer(fp.layer[l], layers[l], PL.layer[l], d, vp.dff, ffn_scale, pack);
        if (v.keys) set_layer_drop(fp.layer[l], training, cfg->p_drop, seed, l);
    }
    fp.ln_w = ln_w; fp.ln_b = ln_b; fp.eps = cfg->ln_eps;
    fp.nseg = vp.nseg; fp.n_layers = vp.L; fp.B = vp.vB; fp.S = v.tiled ? FUSED_TOK_PAD : vp.S; fp.d_ff = vp.dff;
    fp.tpc = v.tpc; fp.S_clip = v.S_clip; fp.Ntok = vp.N; fp.mode = FUSED_MODE_FULL;
    fp.saved_pre = (float*)SL.at(SL.res);
    fp.saved_res = fp.saved_pre + SL.res_index(0, 0);
    fp.relu_bits = (uint32_t*)SL.at(SL.relu_bits);
    fp.hid_out = SL.at(SL.hid);
    fp.x1p_out = split_planes(cfg) ? (unsigned short*)SL.at(SL.x1p) : nullptr;
    fp.xin_out = (float*)SL.at(SL.xin);
    fp.qkv_out = (float*)SL.at(SL.qkv);
    if (v.keys) {
        Drop dpz = make_drop(training, cfg->p_pos, seed, 0, SITE_POS);
        fp.pos_key = dpz.key; fp.pos_thresh = dpz.thresh; fp.pos_inv = dpz.inv_keep;
    }
    fp.rot_mode = v.rot_mode;
    fp.n_slices = 1;
    if (v.rtab) { fp.rtab = v.rtab; fp.B_clips = v.B_clips; }
    if (cfg->weight_cache && pk.n) pk.zero_ctl = (unsigned*)((char*)cfg->weight_cache + align_up(PL.bytes, 256));     // a launch that fills the cache also resets its control block
}

// the attention launch of layer l between the tile launches, both directions
static TiledAttnParams tiled_attn_params(const TiledView& v, int l, const float* qkv, float* attn_o, uint64_t key, uint32_t thresh,
                                         float inv, const uint64_t* seed_ptr) {
    TiledAttnParams ap;
    memset(&ap, 0, sizeof(ap));
    ap.qkv = qkv + l * (v.sl->qkv_layer / 4);
    ap.attn_o = attn_o;
    ap.lse = (float*)v.sl->at(v.sl->lse) + l * v.sl->lse_layer_floats;
    ap.B = v.B_clips; ap.S = v.S_clip; ap.tpc = v.tpc;
    ap.drop_key = key; ap.drop_thresh = thresh; ap.drop_inv = inv;
    ap.seed_ptr = seed_ptr; ap.layer = l;
    ap.rtab = v.rtab;
    return ap;
}

// tiled mode: token preparation + Q | K | V of layer 0, then per layer [attention of every clip] [out-projection .. LayerNorm2
// + Q | K | V of the next layer] (2 L + 1 launches), then the pooled head on the output tokens and the cross entropy on its logits
static int tiled_forward(FusedFwdParams& fp, const TiledView& v, const egx_config* cfg, const Plan& vp, const egx_head* head, float* logits_out, hipStream_t st) {
    const int d = vp.d, comp = cfg->compute;
    float* attn = (float*)v.sl->at(v.sl->attn);
    fp.attn_in = attn;
    fp.mode = FUSED_MODE_PRE;
    if (fused_forward(fp, comp, st)) return 1;
    for (int l = 0; l < vp.L; ++l) {
        const FusedLayer& fl = fp.layer[l];
        const TiledAttnParams ap = tiled_attn_params(v, l, fp.qkv_out, attn + (size_t)l * vp.N * d, fl.attn_key, fl.attn_thresh, fl.drop_inv, fp.seed_ptr);
        if (tiled_attn_fwd(ap, comp, st)) return 1;
        fp.mode = FUSED_MODE_POST; fp.l0 = l;
        if (fused_forward(fp, comp, st)) return 1;
    }
    if (head && head->W) {
        float* pooled = (float*)v.sl->at(v.sl->tokens) + vp.N * d;
        if (v.rtab ? pool_head_ragged_fwd(fp.tokens_out, v.rtab, v.B_clips, d, head->ln_w, head->ln_b, cfg->ln_eps, head->W, head->b, head->n_out, pooled, logits_out, st)
                   : pool_head_fwd(fp.tokens_out, v.B_clips, v.S_clip, d, head->ln_w, head->ln_b, cfg->ln_eps, head->W, head->b, head->n_out, pooled, logits_out, st)) return 1;
        const egx_ce* ce = cfg->ce;
        if (ce) return weighted_ce(logits_out, ce->target, ce->class_weight, v.B_clips, head->n_out, ce->loss, ce->d_logits, st);
    }
    return 0;
}

// The part of FusedBwdParams every backward fills alike. Left to the caller: of the uniform call seg[i].off / row0, the feature-dropout
// keys, out_T, dx0_out, token_ce and the slices; of the ragged call rseg.
static int fill_bwd(FusedBwdParams& bp, const FusedBwdScratch& SC, const TiledView& v, const egx_config* cfg,
                    const egx_segment* segs, const Plan& vp, const float* ln_w, const float* ln_b, const egx_layer* layers, const egx_head* head,
                    const float* d_logits, const float* d_tokens, void* scratch, int training, uint64_t seed) {
    const size_t N = vp.N, d = vp.d;
    const SavedLayout& SL = *v.sl;
    memset(&bp, 0, sizeof(bp));
    for (int i = 0; i < vp.nseg; ++i) {
        fill_seg(bp.seg[i], segs[i], i);
        bp.dseg_out[i] = fptr(scratch, SC.dseg[i]);
    }
    bp.n_heads = vp.H;
    for (int l = 0; l < vp.L; ++l) {
        FusedBwdLayer& fl = bp.layer[l];
        fill_bwd_layer(fl, layers[l], SL.pack.layer[l]);
        set_layer_drop(fl, training, cfg->p_drop, seed, l);
        fl.x1_out = fptr(scratch, SC.x1[l]); fl.g2_out = fptr(scratch, SC.g2[l]);
        fl.g1_out = fptr(scratch, SC.g1[l]); fl.dqkv_out = fptr(scratch, SC.dqkv[l]);
        fl.x_in_out = (float*)SL.at(SL.xin) + l * N * d;      // saved by the forward
        // tiled mode: the attention output was saved by the forward too (the per-clip kernels recompute it in P10)
        fl.attn_o_out = v.tiled ? (float*)SL.at(SL.attn) + l * N * d : fptr(scratch, SC.attn_o[l]);
    }
    bp.ln_w = ln_w; bp.ln_b = ln_b; bp.eps = cfg->ln_eps;
    bp.nseg = vp.nseg; bp.n_layers = vp.L; bp.B = vp.vB; bp.S = v.tiled ? FUSED_TOK_PAD : vp.S; bp.d_ff = vp.dff;
    bp.tiled = v.tiled ? 1 : 0; bp.tpc = v.tpc; bp.S_clip = v.S_clip; bp.Ntok = N;
    if (v.rtab) { bp.rtab = v.rtab; bp.B_clips = v.B_clips; }
    bp.d_tokens = d_tokens;
    if (head && head->W) {        // (tiled mode since round 5 too: the first tile launch runs the head backward from the saved token means)
        bp.head.ln_w = head->ln_w; bp.head.ln_b = head->ln_b; bp.head.W = head->W; bp.head.b = head->b; bp.head.n_out = head->n_out;
        bp.d_logits = d_logits;
        bp.d_logits_scale = cfg->d_logits_scale;
        bp.head_off = fused_partial_len(vp.L, vp.nseg);
        if (v.tiled) bp.pooled = (const float*)SL.at(SL.tokens) + N * d;
    }
    bp.saved_pre = (const float*)SL.at(SL.res);
    bp.saved_res = bp.saved_pre + SL.res_index(0, 0);
    bp.saved_qkv = (const float*)SL.at(SL.qkv);
    bp.relu_bits = (const uint32_t*)SL.at(SL.relu_bits);
    bp.dhid_out = (char*)scratch + SC.dhid;
    bp.xg_planes = split_planes(cfg) ? 1 : 0;
    EGX_CHECK(cfg->zero_bytes % 16 == 0 && (((uintptr_t)cfg->zero_buf) & 15) == 0, "zero_buf must be 16-byte aligned and sized");
    bp.zero_buf = (float*)cfg->zero_buf; bp.zero_n = cfg->zero_buf ? cfg->zero_bytes / 4 : 0;
    bp.partials = fptr(scratch, SC.partials); bp.P = SC.P;
    Drop dpz = make_drop(training, cfg->p_pos, seed, 0, SITE_POS);
    bp.pos_key = dpz.key; bp.pos_thresh = dpz.thresh; bp.pos_inv = dpz.inv_keep;
    bp.seed_ptr = cfg->seed_ptr;
    bp.rot_mode = v.rot_mode;
    bp.n_slices = 1;
    return 0;
}

// tiled mode: L + 1 launches of the tile kernel with the attention backward of every clip between them
static int tiled_backward(FusedBwdParams& bp, const FusedBwdScratch& SC, const TiledView& v, const egx_config* cfg, const Plan& vp, void* scratch, hipStream_t st) {
    const int comp = cfg->compute;
    bp.datt = fptr(scratch, SC.datt); bp.dres = fptr(scratch, SC.dres);
    for (int l = vp.L - 1; l >= 0; --l) {
        bp.l_back = l; bp.l_front = l + 1 < vp.L ? l + 1 : -1;
        if (fused_backward(bp, comp, st)) return 1;
        bp.zero_buf = nullptr;
        const FusedBwdLayer& fl = bp.layer[l];
        TiledAttnParams ap = tiled_attn_params(v, l, bp.saved_qkv, fl.attn_o_out, fl.attn_key, fl.attn_thresh, fl.drop_inv, cfg->seed_ptr);
        ap.d_o = bp.datt; ap.delta = fptr(scratch, SC.delta); ap.dqkv = fl.dqkv_out;
        if (tiled_attn_bwd(ap, comp, st)) return 1;
    }
    bp.l_back = -1; bp.l_front = 0;
    return fused_backward(bp, comp, st);
}

// ---- the backward's tail: the cross-workgroup sums ----------------------------------------------------------------------------------------
// small parameter gradients: where the sums of the per-clip (per-tile) partial rows go (fused.h FUSED_P_LAYER has the row's layout)
static void partial_dsts(ReducePartialsParams& rp, const FusedBwdParams& bp, const egx_layer_grads* layer_grads, float* d_ln_w, float* d_ln_b,
                         const egx_segment_grads* seg_grads, const egx_head* head, const egx_head_grads* head_grads, const egx_token_ce* tce) {
    memset(&rp, 0, sizeof(rp));
    rp.B = bp.B; rp.P = bp.P; rp.partials = bp.partials;
    auto add_dst = [&](float* dst, int off, int len) { if (dst) { rp.d[rp.n].dst = dst; rp.d[rp.n].off = off; rp.d[rp.n].len = len; ++rp.n; } };
    for (int l = 0; l < bp.n_layers; ++l) {
        const egx_layer_grads& gw = layer_grads[l];
        int o = l * FUSED_P_LAYER;
        add_dst(gw.norm2_w, o + 0, 128); add_dst(gw.norm2_b, o + 128, 128); add_dst(gw.lin2_b, o + 256, 128);
        add_dst(gw.norm1_w, o + 384, 128); add_dst(gw.norm1_b, o + 512, 128); add_dst(gw.out_proj_b, o + 640, 128);
        add_dst(gw.in_proj_b, o + 768, 384);
    }
    const int og = bp.n_layers * FUSED_P_LAYER, oh = fused_partial_len(bp.n_layers, bp.nseg);
    add_dst(d_ln_w, og, 128); add_dst(d_ln_b, og + 128, 128);
    for (int i = 0; i < bp.nseg && seg_grads; ++i) {
        add_dst(seg_grads[i].add_vec, og + 256 + i * 256, 128);
        add_dst(seg_grads[i].proj_b, og + 256 + i * 256 + 128, 128);
    }
    if (head && head->W && head_grads) {
        add_dst(head_grads->ln_w, oh, 128); add_dst(head_grads->ln_b, oh + 128, 128);
        add_dst(head_grads->b, oh + 256, head->n_out);
        add_dst(head_grads->W, oh + 256 + FUSED_HEAD_MAX_OUT, head->n_out * 128);
    }
    if (tce) {
        add_dst(tce->d_b, oh + 256, tce->C);
        add_dst(tce->d_W, oh + 256 + FUSED_HEAD_MAX_OUT, tce->C * 128);
    }
}

// FFN weight gradient of layer l (dW1, db1, dW2 from the stored H / dH tiles and the x1 / g2 planes); every layer's slabs are summed by ONE
// launch behind the last one. (Round 6 tried it right behind ffn_bwd_kernel of the same layer, while dH and g2 are still in the Infinity
// Cache: three same-box pairs 372.1 / 374.9 / 371.9 vs 372.2 / 370.3 / 376.1 us, no difference; and the exact-fp32 mode needs x1 from the
// attention-side launch first. It stays behind the whole backward.)
static int launch_ffn_dw(int l, const FusedBwdParams& bp, const FusedBwdScratch& SC, const TiledView& v, const egx_config* cfg,
                         const Plan& vp, const egx_layer* layers, const egx_layer_grads* layer_grads, void* scratch,
                         SlabReduce& red, hipStream_t st) {
    const egx_layer_grads& gw = layer_grads[l];
    if (!(gw.lin1_w || gw.lin1_b || gw.lin2_w)) return 0;
    const int comp = cfg->compute;
    const SavedLayout& SL = *v.sl;
    FfnDwParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.x1 = bp.layer[l].x1_out; fp.g = bp.layer[l].g2_out;
    fp.w1p = SL.pack.layer[l].lin1_w; fp.w2tp = SL.pack.layer[l].lin2_wt; fp.b1 = layers[l].lin1_b;
    fp.N = (int)vp.N; fp.S = vp.S; fp.d_ff = vp.dff;
    fp.drop_key = bp.layer[l].ffn_key; fp.drop_thresh = bp.layer[l].ffn_thresh; fp.drop_inv = bp.layer[l].drop_inv;
    fp.seed_ptr = cfg->seed_ptr; fp.layer = l;
    fp.hs = SL.at(SL.hid + l * SL.hid_layer);
    fp.dhs = (const char*)scratch + SC.dhid + l * SL.hid_layer;
    fp.B = vp.vB;
    fp.xg_planes = bp.xg_planes;
    if (fp.xg_planes) fp.x1 = (const float*)SL.at(SL.x1p + l * SL.x1p_layer);
    return ffn_dw(fp, comp, gw.lin1_w, gw.lin1_b, gw.lin2_w, (char*)scratch + SC.ffn_slab[l], st, nullptr, cfg->deterministic != 0, &red);
}

// The queue of the grouped small-weight-gradient launches (dW_o, dW_in per layer, dW_proj per segment), SMALL_DW_MAX problems each.
// With a tail (the one-stage backwards): small_dw leaves tiles and ONE fixed-order launch sums them, the FFN slabs and the partial rows
// (tail_reduce, fused_bwd.hip): no float atomics, bit-reproducible in every mode; the slabs, the rows, the seed advance and the weight
// prefetch ride in the first tail launch only. Without one (stage 2 of the staged backward) small_dw reduces by itself.
struct TailArgs { const SlabReduce* red; const ReducePartialsParams* rp; uint64_t* adv; const TouchList* tl; };
struct SmallDwQueue {
    int comp; hipStream_t st;
    void* slabs; size_t slab_bytes;         // small_dw's tiles (null: atomic accumulation)
    const TailArgs* tail;
    SmallDwParams sp;
    bool first;
    SmallDwQueue(int comp_, hipStream_t st_, void* slabs_, size_t slab_bytes_, const TailArgs* tail_)
        : comp(comp_), st(st_), slabs(slabs_), slab_bytes(slab_bytes_), tail(tail_), first(true) { memset(&sp, 0, sizeof(sp)); }
    int flush() {
        if (sp.n && small_dw(sp, comp, st, slabs, slab_bytes, !tail)) return 1;
        const int rc = (tail && (sp.n || first)) ? tail_reduce(sp.n ? &sp : nullptr, first ? tail->red : nullptr, first ? tail->rp : nullptr,
                                                               first ? tail->adv : nullptr, first ? tail->tl : nullptr, st) : 0;
        first = false;
        memset(&sp, 0, sizeof(sp));
        return rc;
    }
    // dW[R][C] += G^T X over K token rows (K <= 0: a ragged batch may leave a problem no rows; never so on uniform shapes)
    int add(const float* G, int ldg, const float* X, int ldx, float* out, int R, int Cc, int K) {
        if (!out || K <= 0) return 0;
        if (sp.n == SMALL_DW_MAX && flush()) return 1;
        SmallDwProblem& q = sp.pr[sp.n++];
        q.G = G; q.X = X; q.out = out; q.R = R; q.C = Cc; q.K = K; q.ldg = ldg; q.ldx = ldx;
        return 0;
    }
};
// every dense weight gradient through the queue; feat[i] / seg_rows[i]: the feature rows of segment i that match the rows of d(seg i)
static int small_dw_all(SmallDwQueue& q, const FusedBwdParams& bp, const Plan& vp, const egx_layer_grads* layer_grads, const egx_segment* segs,
                        const egx_segment_grads* seg_grads, const float* const* feat, const size_t* seg_rows) {
    const int d = vp.d, N = (int)vp.N;
    for (int l = 0; l < vp.L; ++l) {
        const egx_layer_grads& gw = layer_grads[l];
        if (q.add(bp.layer[l].g1_out, d, bp.layer[l].attn_o_out, d, gw.out_proj_w, d, d, N)) return 1;
        if (q.add(bp.layer[l].dqkv_out, 3 * d, bp.layer[l].x_in_out, d, gw.in_proj_w, 3 * d, d, N)) return 1;
    }
    for (int i = 0; i < vp.nseg && seg_grads; ++i)
        if (q.add(bp.dseg_out[i], d, feat[i], segs[i].d_in, seg_grads[i].proj_w, d, segs[i].d_in, (int)seg_rows[i])) return 1;
    return q.flush();
}

// ---- the uniform batch: per-clip kernels (S <= 48: one launch, cut, sliced) or the tiled mode -----------------------------------------------
int fused_path_fwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool tiled, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, float* tokens_out, float* logits_out, void* saved, int training,
                   uint64_t seed, hipStream_t st) {
    const int d = pl.d, S = pl.S, B = pl.B, comp = cfg->compute;
    const bool with_head = head && head->W;
    const egx_ce* ce = cfg->ce;
    const egx_token_ce* tce = cfg->token_ce;
    const Plan vp = tiled ? plan_tiled(pl) : pl;
    const SavedLayout SL = saved_layout(cfg, segs, vp, tiled, saved);
    const FusedPackLayout& PL = SL.pack;
    const TiledView v = uniform_view(vp, SL, tiled);
    FusedFwdParams fp;
    PackParams pk;
    fill_fwd(fp, pk, v, cfg, segs, vp, ln_w, ln_b, layers, training, seed);
    for (int i = 0; i < pl.nseg; ++i) {
        fp.seg[i].off = pl.seg_off[i]; fp.seg[i].row0 = 0;
        Drop df = make_drop(training, cfg->p_feat, seed, (uint32_t)i, SITE_FEAT);
        fp.feat_key[i] = df.key; fp.feat_thresh = df.thresh; fp.feat_inv = df.inv_keep;
    }
    fp.tokens_out = tokens_out;
    fp.out_T = cfg->out_tokens > 0 ? cfg->out_tokens : S;
    if (tiled) {
        if (!fp.tokens_out) fp.tokens_out = (float*)SL.at(SL.tokens);
        if (pack_weights(pk, st)) return 1;
        return tiled_forward(fp, v, cfg, vp, head, logits_out, st);
    }
    if (with_head) {
        fp.head.ln_w = head->ln_w; fp.head.ln_b = head->ln_b; fp.head.W = head->W; fp.head.b = head->b; fp.head.n_out = head->n_out;
        fp.logits_out = logits_out;
    }
    fp.n_slices = fused_slices(pl, comp);
    if (fp.n_slices > 1) {
        fp.xchg = (float*)SL.at(SL.xchg); fp.xflags = (unsigned*)SL.at(SL.xflags_fwd);
        pk.zero_words = fp.xflags; pk.n_zero = (int)SL.flag_words;        // the packing launch (always in front) zeroes the flags
        fp.slice_drop = slice_drop_mask(fp.n_slices);
    }
    fp.x1f_out = (float*)SL.at(SL.x1f);
    const bool cut = use_cut(pl, fp.n_slices, false, comp);
    // fused weighted cross entropy (egx_ce): in the epilogue of the launch that writes the logits; every clip adds its term into *loss,
    // which the packing launch zeroes when there is one, else the first launch of a cut-mode forward, else a memset node
    const bool ce_fused = ce && with_head && !cfg->deterministic;
    if (ce_fused) {
        fp.ce_target = ce->target; fp.ce_weight = ce->class_weight; fp.ce_loss = ce->loss; fp.ce_dlogits = ce->d_logits; fp.ce_B = B;
        if (pk.n || pk.seed_advance || pk.zero_words) pk.zero_word2 = ce->loss;
        else if (cut) fp.zero_word = ce->loss;
        else if (cfg->weight_cache) fp.ce_ticket = (unsigned*)((char*)cfg->weight_cache + align_up(PL.bytes, 256));   // no earlier launch: arrival counter instead of a memset node
        else EGX_HIP(hipMemsetAsync(ce->loss, 0, sizeof(float), st));
    }
    if (tce) {
        fp.tce_W = tce->W; fp.tce_b = tce->b; fp.tce_target = tce->target; fp.tce_cw = tce->class_weight; fp.tce_C = tce->C;
        fp.tce_logits = tce->logits; fp.tce_probs = tce->probs; fp.tce_pred = tce->pred; fp.tce_loss = tce->loss; fp.tce_correct = tce->correct;
        fp.tce_dlogits = tce->d_logits;
        fp.tce_ticket = (unsigned*)((char*)cfg->weight_cache + align_up(PL.bytes, 256)) + 4;      // words 4..6 of the control block
    }
    if (pack_weights(pk, st)) return 1;
    // With a persistent weight cache nothing has just written the packed copies: every launch brings the streams its successor reads
    // first into the Infinity Cache (TouchList, fused.h)
    const bool touch = cfg->weight_cache != nullptr;
    const size_t ffn_pb = packed_bytes(pl.dff, d, comp), in_pb = packed_bytes(3 * d, d, comp), out_pb = packed_bytes(d, d, comp);
    if (cut) {
        // cut mode: per layer [token preparation | layer input .. LayerNorm1] (4 waves per clip) + [FFN .. LayerNorm2 (+ pooled head)] (8 waves)
        fp.mode = FUSED_MODE_ATTN;
        for (int l = 0; l < pl.L; ++l) {
            fp.l0 = l;
            memset(&fp.touch, 0, sizeof(fp.touch));
            if (touch) { touch_add(fp.touch, PL.layer[l].lin1_w, ffn_pb); touch_add(fp.touch, PL.layer[l].lin2_w, ffn_pb); }
            if (fused_forward(fp, comp, st)) return 1;
            fp.zero_word = nullptr;
            memset(&fp.touch, 0, sizeof(fp.touch));
            if (touch && l + 1 < pl.L) { touch_add(fp.touch, PL.layer[l + 1].in_w, in_pb); touch_add(fp.touch, PL.layer[l + 1].out_w, out_pb); }
            else if (touch && training) { touch_add(fp.touch, PL.layer[l].lin2_wt, ffn_pb); touch_add(fp.touch, PL.layer[l].lin1_wt, ffn_pb); }
            if (ffn_cut_forward(fp, l, comp, st)) return 1;
        }
    } else {
        if (touch) {        // one launch: its own FFN streams (read ~25 us in) and, in training, the backward's first
            touch_add(fp.touch, PL.layer[0].lin1_w, ffn_pb); touch_add(fp.touch, PL.layer[0].lin2_w, ffn_pb);
            if (training) { touch_add(fp.touch, PL.layer[pl.L - 1].lin2_wt, ffn_pb); touch_add(fp.touch, PL.layer[pl.L - 1].lin1_wt, ffn_pb); }
        }
        if (fused_forward(fp, comp, st)) return 1;
    }
    // deterministic mode keeps the cross entropy out of the epilogue: its own launch on the logits
    if (ce && with_head && !ce_fused) return weighted_ce(logits_out, ce->target, ce->class_weight, B, head->n_out, ce->loss, ce->d_logits, st);
    return 0;
}

int fused_path_bwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool tiled, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, float* d_tokens, const float* d_logits, const void* saved, void* scratch,
                   const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads,
                   const egx_head_grads* head_grads, int training, uint64_t seed, hipStream_t st) {
    const int d = pl.d, S = pl.S, B = pl.B, comp = cfg->compute;
    const bool with_head = head && head->W;
    const Plan vp = tiled ? plan_tiled(pl) : pl;
    const SavedLayout SL = saved_layout(cfg, segs, vp, tiled, saved);
    const FusedPackLayout& PL = SL.pack;
    const TiledView v = uniform_view(vp, SL, tiled);
    const egx_token_ce* tce = cfg->token_ce;
    if (tce) {
        EGX_CHECK(!with_head && !tiled && fused_token_ce_ok(cfg, pl), "egx_config.token_ce: not on this configuration (egx_encoder_token_ce_ok)");
        EGX_CHECK(tce->W && tce->d_logits && tce->C >= 1 && tce->C <= 8, "egx_config.token_ce: W, d_logits and 1 <= C <= 8 must be set");
    }
    FusedBwdScratch SC = fused_bwd_scratch(cfg, segs, vp, with_head ? head->n_out : tce ? tce->C : 0);
    FusedBwdParams bp;
    if (fill_bwd(bp, SC, v, cfg, segs, vp, ln_w, ln_b, layers, head, d_logits, d_tokens, scratch, training, seed)) return 1;
    const bool touch = cfg->weight_cache != nullptr && !tiled;      // (see the forward)
    const size_t ffn_pb = packed_bytes(pl.dff, d, comp), in_pb = packed_bytes(3 * d, d, comp), out_pb = packed_bytes(d, d, comp);
    for (int i = 0; i < pl.nseg; ++i) {
        bp.seg[i].off = pl.seg_off[i]; bp.seg[i].row0 = 0;
        Drop df = make_drop(training, cfg->p_feat, seed, (uint32_t)i, SITE_FEAT);
        bp.feat_key[i] = df.key; bp.feat_thresh = df.thresh; bp.feat_inv = df.inv_keep;
    }
    bool want_pos = false;
    for (int i = 0; i < pl.nseg && seg_grads; ++i) want_pos = want_pos || seg_grads[i].pos;
    bp.dx0_out = want_pos ? fptr(scratch, SC.dx0) : nullptr;
    bp.out_T = cfg->out_tokens > 0 ? cfg->out_tokens : S;
    if (tce) {
        bp.tce_W = tce->W; bp.tce_dlogits = tce->d_logits; bp.tce_C = tce->C;
        bp.d_logits_scale = cfg->d_logits_scale;
        bp.head_off = fused_partial_len(pl.L, pl.nseg);
    }
    const int stage = cfg->bwd_stage;
    EGX_CHECK(stage >= 0 && stage <= 2, "bwd_stage=%d", stage);
    if (stage == 2) bp.zero_buf = nullptr;
    if (!tiled) bp.n_slices = fused_slices(pl, comp);
    if (bp.n_slices > 1 && stage != 2) {
        bp.xchg = fptr(scratch, SC.xchg);
        bp.xflags = (unsigned*)SL.at(SL.xflags_bwd);
        EGX_HIP(hipMemsetAsync(bp.xflags, 0, SL.flag_words * 4, st));
        bp.slice_drop = slice_drop_mask(bp.n_slices);
    }
    if (stage != 2 && tiled) {
        if (tiled_backward(bp, SC, v, cfg, vp, scratch, st)) return 1;
    } else if (stage != 2 && use_cut(pl, bp.n_slices, tiled, comp)) {
        // cut mode: per layer, top down, [LayerNorm2 backward + FFN input gradient] (8 waves per clip) + [LayerNorm1 backward .. the layer
        // input's gradient, or the token-preparation backward] (4 waves)
        bp.cut = 1; bp.dy1 = fptr(scratch, SC.dy1); bp.dxin = fptr(scratch, SC.dxin);
        for (int l = pl.L - 1; l >= 0; --l) {
            bp.cut_layer = l;
            memset(&bp.touch, 0, sizeof(bp.touch));
            if (touch) { touch_add(bp.touch, PL.layer[l].out_wt, out_pb); touch_add(bp.touch, PL.layer[l].in_wt, in_pb); }
            if (ffn_cut_backward(bp, l, comp, st)) return 1;
            bp.zero_buf = nullptr;
            memset(&bp.touch, 0, sizeof(bp.touch));
            if (touch && l > 0) { touch_add(bp.touch, PL.layer[l - 1].lin2_wt, ffn_pb); touch_add(bp.touch, PL.layer[l - 1].lin1_wt, ffn_pb); }
            if (fused_backward(bp, comp, st)) return 1;
        }
    } else if (stage != 2) {
        if (touch) { touch_add(bp.touch, PL.layer[pl.L - 1].out_wt, out_pb); touch_add(bp.touch, PL.layer[pl.L - 1].in_wt, in_pb); }
        if (fused_backward(bp, comp, st)) return 1;
    }

    for (int i = 0; i < pl.nseg && seg_grads; ++i)
        EGX_CHECK(!seg_grads[i].feat, "fused backward: feature gradients are not supported (use impl=generic)");
    ReducePartialsParams rp;
    partial_dsts(rp, bp, layer_grads, d_ln_w, d_ln_b, seg_grads, head, head_grads, tce);
    // learned positional table (the HOI translators' `pe`): sum d(token-prep output) over the clips, per segment
    if (bp.dx0_out && stage != 2)
        for (int i = 0; i < pl.nseg; ++i)
            if (seg_grads[i].pos && pos_grad_accum(bp.dx0_out, B, S, pl.seg_off[i], segs[i].T, d, seg_grads[i].pos, segs[i].pos_stride, 0, 0, 1.f, st)) return 1;
    // the partial-row reduction rides in the slab-reduction launch of the first FFN weight gradient
    bool rp_pending = stage != 2;
    SlabReduce red;
    red.narr = 0; red.nslab = 0;
    for (int l = 0; l < pl.L && stage != 2; ++l)
        if (launch_ffn_dw(l, bp, SC, v, cfg, vp, layers, layer_grads, scratch, red, st)) return 1;
    // egx_config.advance_seed == 2: the backward advances the device seed behind its last reader (the last launch that can run here)
    uint64_t* adv = (cfg->advance_seed == 2 && cfg->seed_ptr && training && stage != 1) ? const_cast<uint64_t*>(cfg->seed_ptr) : nullptr;
    const float* feat[EGX_MAX_SEGMENTS];
    size_t seg_rows[EGX_MAX_SEGMENTS];
    for (int i = 0; i < pl.nseg; ++i) { feat[i] = segs[i].feat; seg_rows[i] = (size_t)(B * segs[i].T); }
    // One-stage backward: every sum in the tail launch. The staged backward (stage 1 / 2) keeps the launches of its own below.
    if (stage == 0) {
        TouchList tl;
        memset(&tl, 0, sizeof(tl));
        if (touch) {    // the next forward starts with the projections and layer 0's in-projection (one contiguous run of the cache) and out-projection
            touch_add(tl, PL.proj[0], (size_t)((const char*)PL.layer[0].in_wt - (const char*)PL.proj[0]));
            touch_add(tl, PL.layer[0].out_w, out_pb);
        }
        const TailArgs tail = {&red, &rp, adv, &tl};
        SmallDwQueue q(comp, st, (char*)scratch + SC.sdw_tiles, SC.sdw_bytes, &tail);
        return small_dw_all(q, bp, vp, layer_grads, segs, seg_grads, feat, seg_rows);
    }
    // two-stage backward: the late region must be complete when the exchange starts, so the reductions get a launch of their own
    if (red.narr) {
        if (ffn_dw_reduce(red, rp_pending ? &rp : nullptr, cfg->deterministic != 0, st)) return 1;
        rp_pending = false;
    }
    if (rp_pending && reduce_partials(rp, st, cfg->deterministic != 0)) return 1;
    // every remaining weight gradient (dW_o, dW_in per layer, dW_proj per segment) in grouped launches
    if (stage != 1) {
        SmallDwQueue q(comp, st, cfg->deterministic ? (char*)scratch + SC.slabs : nullptr, SC.slab_bytes, nullptr);
        if (small_dw_all(q, bp, vp, layer_grads, segs, seg_grads, feat, seg_rows)) return 1;
    }
    if (adv && seed_advance(adv, st)) return 1;
    return 0;
}

}  // namespace egx

using namespace egx;

// ---- ragged batches (egx_ragged_fwd): inference over clips of their own lengths on the tiled kernels ---------------------------------
// The tile grid of the tiled mode with per-clip offsets: clip b has S_b = sum_k T_{b,k} tokens in ceil(S_b / 48) tiles; its tiles, dense token
// rows, log-sum-exp rows and output rows start at the prefix sums of the clips before it (fused.h RAGGED_REC). The workspace is the tiled
// forward's layout sized for N = sum_b S_b tokens and sum_b ceil(S_b / 48) tiles, then the device copy of the batch table.
namespace {
struct RaggedPlan {
    Plan vp;                    // vp.B clips, vp.vB tiles, vp.N = sum_b S_b tokens, vp.S = the longest clip
    size_t out_rows = 0;        // head-less output rows: sum_b T_{b,0}
    SavedLayout sl;             // the workspace (inference) / `saved` (training) of the call the plan was made for
    std::vector<int> tab;       // host copy of the batch table (empty in a capacity plan: the device builds it, ragged_table.hip)
    size_t tab_words = 0;       // ints of the device table
    int tiles = 0;
    size_t seg_rows[FUSED_MAX_SEG] = {0, 0, 0, 0};    // training plan: sum_b T_{b,k}, the packed rows of segment k
};

// what a ragged call asks of its configuration, whatever the lengths (the host plan and the capacity plan)
int ragged_config_ok(const egx_config* cfg, const egx_segment* segs, int B, const Plan& vp, bool train) {
    EGX_CHECK(B <= (1 << 20), "ragged batch: B=%d clips (at most %d)", B, 1 << 20);
    if (train) {
        EGX_CHECK(cfg->p_feat == 0.f, "ragged training: feature dropout (p_feat > 0) is not supported (got %g)", cfg->p_feat);
        EGX_CHECK(cfg->out_tokens == 0, "ragged training: out_tokens is not supported (head-less, the first segment of every clip is returned)");
        EGX_CHECK(!cfg->token_ce, "ragged training: the fused token loss (egx_config.token_ce) is not supported; apply the loss to the returned rows");
        EGX_CHECK(!cfg->bucket_cb && cfg->bwd_stage == 0, "ragged training: bucket_cb and the staged backward (bwd_stage) are not supported");
    } else {
        EGX_CHECK(cfg->p_drop == 0.f && cfg->p_pos == 0.f && cfg->p_feat == 0.f,
                  "ragged batches are inference-only: p_drop, p_pos and p_feat must be 0 (got %g, %g, %g)", cfg->p_drop, cfg->p_pos, cfg->p_feat);
        EGX_CHECK(cfg->out_tokens == 0, "ragged batch: out_tokens is not supported (head-less, the first segment of every clip is returned)");
        EGX_CHECK(!cfg->ce && !cfg->token_ce, "ragged batch: the fused losses (egx_config.ce / token_ce) are not supported; apply the loss to the outputs");
        EGX_CHECK(!cfg->bucket_cb, "ragged batch: bucket_cb is a backward option (the ragged call is a forward only)");
    }
    EGX_CHECK(!cfg->weight_cache_valid || cfg->weight_cache, "weight_cache_valid without a weight_cache");
    EGX_CHECK(cfg->impl == EGX_IMPL_AUTO || cfg->impl == EGX_IMPL_TILED, "ragged batch: runs on the tiled kernels (impl auto or tiled, got %d)", cfg->impl);
    // what tiled_ok() asks of the configuration, the clip length apart
    EGX_CHECK(vp.d == 128 && vp.H == 4 && vp.dff % 128 == 0 && vp.dff >= 128 && vp.nseg <= FUSED_MAX_SEG && vp.L >= 1 && vp.L <= FUSED_MAX_LAYERS &&
              !packed_feats(segs, vp.nseg) && (cfg->compute == EGX_F32_SPLIT || cfg->compute == EGX_BF16),
              "ragged batch: needs d=128, h=4, d_ff%%128==0, <= %d segments, 1..%d layers, fp32 features, compute bf16 or f32s", FUSED_MAX_SEG, FUSED_MAX_LAYERS);
    for (int k = 0; k < vp.nseg; ++k)
        EGX_CHECK(segs[k].proj_w && segs[k].d_in % 128 == 0, "ragged batch: segment %d needs a projection with d_in %% 128 == 0", k);
    return 0;
}
// train (egx_ragged_train_*): dropout (but FEAT) and the weighted cross entropy are allowed; the table gets the packed first row of every
// clip's segments behind the tile map (FusedBwdParams::rseg). saved: the call's block, null in a size query
int ragged_plan(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, const void* saved, RaggedPlan& rp, bool train = false) {
    Plan& vp = rp.vp;
    if (make_plan(cfg, segs, B, vp)) return 1;
    EGX_CHECK(lengths, "ragged batch: null lengths");
    if (ragged_config_ok(cfg, segs, B, vp, train)) return 1;
    const int K = vp.nseg;
    rp.tab.assign((size_t)B * RAGGED_REC, 0);
    int tiles = 0, S_max = 0;
    size_t tok = 0, out = 0;
    for (int b = 0; b < B; ++b) {
        int* rec = rp.tab.data() + (size_t)b * RAGGED_REC;
        int S = 0;
        for (int k = 0; k < K; ++k) {
            const int T = lengths[(size_t)b * K + k];
            EGX_CHECK(T >= 1 && T <= segs[k].T, "ragged batch: clip %d segment %d has %d frames (1 .. %d, the padded length)", b, k, T, segs[k].T);
            rec[RG_T + k] = T; rec[RG_OFF + k] = S;
            S += T;
        }
        EGX_CHECK(S <= TILED_MAX_S, "ragged batch: clip %d has S=%d tokens (at most %d)", b, S, TILED_MAX_S);
        rec[RG_TILE0] = tiles; rec[RG_S] = S; rec[RG_TOK0] = (int)tok;
        rec[RG_OUT0] = (int)out; rec[RG_OUTN] = rec[RG_T];      // head-less output: the first segment; with a head the call rewrites these
        tiles += cdiv(S, FUSED_TOK_PAD);
        tok += S; out += rec[RG_T];
        S_max = S > S_max ? S : S_max;
    }
    rp.tab.resize((size_t)B * RAGGED_REC + tiles + (train ? (size_t)B * FUSED_MAX_SEG : 0));
    for (int b = 0; b < B; ++b) {
        const int* rec = rp.tab.data() + (size_t)b * RAGGED_REC;
        for (int j = 0; j < cdiv(rec[RG_S], FUSED_TOK_PAD); ++j) rp.tab[(size_t)B * RAGGED_REC + rec[RG_TILE0] + j] = b;
    }
    if (train) {
        int* rseg = rp.tab.data() + (size_t)B * RAGGED_REC + tiles;
        for (int k = 0; k < K; ++k) {
            size_t r = 0;
            for (int b = 0; b < B; ++b) { rseg[(size_t)b * FUSED_MAX_SEG + k] = (int)r; r += lengths[(size_t)b * K + k]; }
            rp.seg_rows[k] = r;
        }
    }
    rp.tiles = tiles;
    vp.vB = tiles; vp.tpc = 0; vp.N = tok; vp.S = S_max;
    rp.out_rows = out;
    rp.tab_words = rp.tab.size();
    rp.sl = saved_layout(cfg, segs, vp, true, saved, rp.tab_words);
    return 0;
}
// with a head the last layer leaves EVERY token of a clip (rows tok0 .. tok0 + S_b of the dense array); head-less its first segment, packed
void ragged_head_rows(RaggedPlan& rp, int B, bool with_head) {
    if (!with_head) return;
    for (int b = 0; b < B; ++b) {
        int* rec = rp.tab.data() + (size_t)b * RAGGED_REC;
        rec[RG_OUT0] = rec[RG_TOK0]; rec[RG_OUTN] = rec[RG_S];
    }
}

TiledView ragged_view(const RaggedPlan& rp, int B, const int* tab, bool keys) {
    TiledView v;
    memset(&v, 0, sizeof(v));
    v.sl = &rp.sl;
    v.rtab = tab;
    v.B_clips = B; v.tpc = 0; v.S_clip = rp.vp.S; v.tiled = true;
    // every tile walks the FFN hidden blocks from block 0 (rot_mode 1, +2.5 % of the tiled launches' time against the staggered default):
    // the staggered start depends on the tile's place in the grid, so a clip's result would depend on where the batch puts it
    v.rot_mode = 1;
    v.keys = keys;
    return v;
}

// The forward of egx_ragged_fwd (`train` false) and egx_ragged_train_fwd (`train`) over the caller's plan (ragged_plan(..., train)) and the
// workspace it was made for. Only the train call hands the kernels dropout keys, the device seed (and its advance) and runs the cross entropy; the
// inference call's keys stay zero and its FFN keep-scale 1.
int ragged_forward(const egx_config* cfg, const egx_segment* segs, RaggedPlan& rp, const float* ln_w, const float* ln_b, const egx_layer* layers,
                   const egx_head* head, int B, float* logits_out, float* tokens_out, bool train, int training, uint64_t seed,
                   hipStream_t st, bool dev_table = false) {
    const Plan& vp = rp.vp;
    const bool with_head = head && head->W;
    // the batch table to the device, stream-ordered, in the arguments of upload launches (no host buffer has to outlive the call). Its
    // contents depend on the lengths of THIS call: a captured hipGraph would replay them for every batch, so the call is not for capture.
    // (dev_table: the capacity plan's table, already built in place by ragged_table_build on this stream.)
    const SavedLayout& SL = rp.sl;
    int* tab = (int*)SL.at(SL.tab);
    if (!dev_table) {
        ragged_head_rows(rp, B, with_head);
        if (upload_words(tab, rp.tab.data(), rp.tab.size(), st)) return 1;
    }
    const TiledView v = ragged_view(rp, B, tab, train);
    FusedFwdParams fp;
    PackParams pk;
    fill_fwd(fp, pk, v, cfg, segs, vp, ln_w, ln_b, layers, training, seed);     // (the clip's own segment pieces come from the batch table)
    // with a head: every token of the last layer (N, d) in the workspace, then the token means (B, d)
    fp.tokens_out = with_head ? (float*)SL.at(SL.tokens) : tokens_out;
    if (pack_weights(pk, st)) return 1;
    return tiled_forward(fp, v, cfg, vp, head, logits_out, st);     // (the inference plan refuses egx_config.ce)
}
}  // namespace

extern "C" {

int egx_ragged_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* bytes) {
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, nullptr, rp)) return 1;
    if (bytes) *bytes = rp.sl.bytes;
    return 0;
}

int egx_ragged_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, int B, float* logits_out, float* tokens_out, void* workspace, void* stream) {
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, workspace, rp)) return 1;
    EGX_CHECK(workspace && ln_w && ln_b && layers, "ragged batch: null pointer argument");
    const bool with_head = head && head->W;
    EGX_CHECK(with_head ? logits_out != nullptr : tokens_out != nullptr, "ragged batch: null output pointer");
    if (check_head(head)) return 1;
    return ragged_forward(cfg, segs, rp, ln_w, ln_b, layers, head, B, logits_out, tokens_out, false, 0, 0, (hipStream_t)stream);
}

}  // extern "C"

// ---- ragged batches for training (egx_ragged_train_fwd / egx_ragged_bwd): the tiled training mode over clips of their own lengths -------
// `saved` is egx_ragged_fwd's workspace layout for the same batch (the RAGGED forward launches already write everything the tiled backward
// reads: layer inputs, Q | K | V, the residual sums, the FFN hidden tiles and ReLU / dropout bits, x1 planes, attention outputs, log-sum-exp
// rows, the last layer's tokens and the per-clip token means). The backward's scratch is the tiled backward's, sized by N = sum_b S_b tokens
// and the tile count, with d(seg) packed (sum_b T_{b,k} rows per segment), then its own copy of the batch table and the packed operands of
// the projection-weight and feature gradients.
namespace {
struct RaggedTrainScratch {
    FusedBwdScratch sc;
    size_t tab = 0, featp[FUSED_MAX_SEG] = {0, 0, 0, 0}, dfeat = 0, bytes = 0;
};
RaggedTrainScratch ragged_train_scratch(const egx_config* cfg, const egx_segment* segs, const RaggedPlan& rp, int head_n_out) {
    RaggedTrainScratch r;
    FusedBwdScratch& s = r.sc;
    const Plan& pl = rp.vp;
    size_t cur = bwd_scratch_prefix(s, cfg, segs, pl, rp.seg_rows, head_n_out);
    const size_t nd = pl.N * pl.d * 4;
    s.dx0 = take(cur, nd);
    s.datt = take(cur, nd); s.dres = take(cur, nd);
    s.delta = take(cur, (size_t)pl.H * pl.N * 4);
    s.bytes = cur;
    r.tab = take(cur, rp.tab_words * sizeof(int));
    size_t dfeat = 0;
    for (int i = 0; i < pl.nseg; ++i) {
        r.featp[i] = take(cur, rp.seg_rows[i] * segs[i].d_in * 4);
        dfeat = size_max(dfeat, rp.seg_rows[i] * segs[i].d_in * 4);
    }
    r.dfeat = take(cur, dfeat);
    r.bytes = cur;
    return r;
}
int ragged_backward(const egx_config* cfg, const egx_segment* segs, const RaggedPlan& rp, const RaggedTrainScratch& RS, const int* tab,
                    const int* rseg, const int* cap_meta, const float* ln_w, const float* ln_b, const egx_layer* layers, const egx_head* head, int B,
                    const float* d_logits, const float* d_tokens, void* scratch, const egx_segment_grads* seg_grads,
                    float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, int training,
                    uint64_t seed, hipStream_t st);
}  // namespace

extern "C" {

int egx_ragged_train_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* saved_bytes,
                               size_t* scratch_bytes) {
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, nullptr, rp, true)) return 1;
    if (saved_bytes) *saved_bytes = rp.sl.bytes;
    if (scratch_bytes) *scratch_bytes = ragged_train_scratch(cfg, segs, rp, FUSED_HEAD_MAX_OUT).bytes;
    return 0;
}

int egx_ragged_train_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                         const egx_layer* layers, const egx_head* head, int B, float* logits_out, float* tokens_out, void* saved,
                         void* scratch, int training, uint64_t seed, void* stream) {
    (void)scratch;
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, saved, rp, true)) return 1;
    EGX_CHECK(saved && ln_w && ln_b && layers, "ragged training: null pointer argument");
    const bool with_head = head && head->W;
    EGX_CHECK(with_head ? logits_out != nullptr : tokens_out != nullptr, "ragged training: null output pointer");
    if (check_head(head) || check_ce(cfg->ce, with_head, "")) return 1;
    return ragged_forward(cfg, segs, rp, ln_w, ln_b, layers, head, B, logits_out, tokens_out, true, training, seed, (hipStream_t)stream);
}

int egx_ragged_bwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                   const egx_layer* layers, const egx_head* head, int B, const float* d_logits, const float* d_tokens, const void* saved,
                   void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads,
                   const egx_head_grads* head_grads, int training, uint64_t seed, void* stream) {
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, saved, rp, true)) return 1;
    const bool with_head = head && head->W;
    EGX_CHECK((with_head ? (const void*)d_logits : (const void*)d_tokens) && saved && scratch && ln_w && ln_b && layers && layer_grads,
              "ragged training: null pointer argument");
    if (check_head(head)) return 1;
    hipStream_t st = (hipStream_t)stream;
    RaggedTrainScratch RS = ragged_train_scratch(cfg, segs, rp, with_head ? head->n_out : 0);
    // the batch table again (the backward's own copy: nothing of the forward's call is trusted but `saved`)
    ragged_head_rows(rp, B, with_head);
    int* tab = (int*)((char*)scratch + RS.tab);
    if (upload_words(tab, rp.tab.data(), rp.tab.size(), st)) return 1;
    return ragged_backward(cfg, segs, rp, RS, tab, tab + (size_t)B * RAGGED_REC + rp.tiles, nullptr, ln_w, ln_b, layers, head, B, d_logits, d_tokens,
                           scratch, seg_grads, d_ln_w, d_ln_b, layer_grads, head_grads, training, seed, st);
}

}  // extern "C"

namespace {
// The backward of egx_ragged_bwd and egx_ragged_cap_bwd behind their table (`tab` on the device, `rseg` inside it). cap_meta (the capacity
// plan: the totals of the device-built table): every size below is the CAPACITY's, and the rows no clip of this batch owns are cleared first.
int ragged_backward(const egx_config* cfg, const egx_segment* segs, const RaggedPlan& rp, const RaggedTrainScratch& RS, const int* tab,
                    const int* rseg, const int* cap_meta, const float* ln_w, const float* ln_b, const egx_layer* layers, const egx_head* head, int B,
                    const float* d_logits, const float* d_tokens, void* scratch, const egx_segment_grads* seg_grads,
                    float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, int training,
                    uint64_t seed, hipStream_t st) {
    const Plan& vp = rp.vp;
    const int d = vp.d, comp = cfg->compute, L = vp.L;
    const FusedBwdScratch& SC = RS.sc;
    bool want_pos = false;
    for (int i = 0; i < vp.nseg && seg_grads; ++i) want_pos = want_pos || seg_grads[i].pos;
    EGX_CHECK(!want_pos, "ragged training: learned positional tables (egx_segment_grads.pos) are not supported");
    const SavedLayout& SL = rp.sl;
    const TiledView v = ragged_view(rp, B, tab, true);
    FusedBwdParams bp;
    if (fill_bwd(bp, SC, v, cfg, segs, vp, ln_w, ln_b, layers, head, d_logits, d_tokens, scratch, training, seed)) return 1;
    bp.rseg = rseg;
    const float* featp[FUSED_MAX_SEG];
    for (int i = 0; i < vp.nseg; ++i) featp[i] = fptr(scratch, RS.featp[i]);
    if (cap_meta) {
        // Capacity plan: the weight-gradient launches below run over tok_cap token rows, the tile capacity and capacity-sized packed segment
        // rows. What no clip of THIS batch owns — token rows [N, tok_cap), the per-tile arrays of the surplus tiles, the packed rows beyond
        // sum_b T_{b,k} — is written by no launch (a surplus workgroup leaves at once, fused_bwd.hip), so it is cleared here, both operands of
        // every product (a stale NaN times zero is a NaN): those launches then add exact zeros. `saved` is the forward's of this very step.
        // (Arrival counters: none of this call's launches has one. The tile and attention launches leave per-tile rows; ffn_dw, small_dw and
        // the tail launch that sums them in a fixed order have grids of the capacity's sizes, which the host knows.)
        RaggedSlackParams sl;
        memset(&sl, 0, sizeof(sl));
        sl.meta = cap_meta;
        const int parts = comp == EGX_BF16 ? 1 : 3;
        const size_t tile_rows = (size_t)FUSED_TOK_PAD * d * 2, plane = (size_t)vp.vB * tile_rows;      // a tile / all tiles of one bf16 plane
        const size_t hid_tile = SL.hid_layer / vp.vB, row = (size_t)d * 4;
        int rc = 0;
        for (int l = 0; l < L; ++l) {
            rc |= ragged_slack_add(sl, SL.at(SL.hid + l * SL.hid_layer), hid_tile, vp.vB, RS_TILES);
            rc |= ragged_slack_add(sl, (char*)scratch + SC.dhid + l * SL.hid_layer, hid_tile, vp.vB, RS_TILES);
            for (int j = 0; j < parts; ++j) {
                rc |= ragged_slack_add(sl, SL.at(SL.x1p + l * SL.x1p_layer + j * plane), tile_rows, vp.vB, RS_TILES);
                rc |= ragged_slack_add(sl, (char*)bp.layer[l].g2_out + j * plane, tile_rows, vp.vB, RS_TILES);
            }
            rc |= ragged_slack_add(sl, bp.layer[l].g1_out, row, vp.N, RS_TOKENS);
            rc |= ragged_slack_add(sl, bp.layer[l].attn_o_out, row, vp.N, RS_TOKENS);
            rc |= ragged_slack_add(sl, bp.layer[l].dqkv_out, 3 * row, vp.N, RS_TOKENS);
            rc |= ragged_slack_add(sl, bp.layer[l].x_in_out, row, vp.N, RS_TOKENS);
        }
        for (int i = 0; i < vp.nseg; ++i) {
            rc |= ragged_slack_add(sl, bp.dseg_out[i], row, rp.seg_rows[i], RS_SEG0 + i);
            rc |= ragged_slack_add(sl, const_cast<float*>(featp[i]), (size_t)segs[i].d_in * 4, rp.seg_rows[i], RS_SEG0 + i);
        }
        rc |= ragged_slack_add(sl, bp.partials, (size_t)bp.P * 4, vp.vB, RS_TILES);
        if (rc || ragged_slack_zero(sl, st)) return 1;
    }
    if (tiled_backward(bp, SC, v, cfg, vp, scratch, st)) return 1;

    // the small parameter gradients: the per-tile partial rows (padding rows of a clip's last tile add nothing: they are zero there)
    ReducePartialsParams rpp;
    partial_dsts(rpp, bp, layer_grads, d_ln_w, d_ln_b, seg_grads, head, head_grads, nullptr);
    // FFN weight gradients from the stored H / dH tiles and the x1 / g2 planes of the tile grid; their slabs are summed by the tail launch
    SlabReduce red;
    red.narr = 0; red.nslab = 0;
    for (int l = 0; l < L; ++l)
        if (launch_ffn_dw(l, bp, SC, v, cfg, vp, layers, layer_grads, scratch, red, st)) return 1;
    // the projection-weight gradients read the valid feature frames only: gathered into packed rows that match the packed d(seg) rows
    for (int i = 0; i < vp.nseg && seg_grads; ++i)
        if (seg_grads[i].proj_w && ragged_rows(const_cast<float*>(segs[i].feat), fptr(scratch, RS.featp[i]), tab, rseg, B, segs[i].T, segs[i].d_in, i, 1, st))
            return 1;
    // every dense weight gradient (dW_o, dW_in per layer, dW_proj per segment) and the sums in the tail launch. tail_reduce's touch list
    // stays null here (the uniform call hands it its own, which is empty in tiled mode)
    uint64_t* adv = (cfg->advance_seed == 2 && cfg->seed_ptr && training) ? const_cast<uint64_t*>(cfg->seed_ptr) : nullptr;
    const TailArgs tail = {&red, &rpp, adv, nullptr};
    SmallDwQueue q(comp, st, (char*)scratch + SC.sdw_tiles, SC.sdw_bytes, &tail);
    if (small_dw_all(q, bp, vp, layer_grads, segs, seg_grads, featp, rp.seg_rows)) return 1;
    // d(feature) (unfrozen backbones): packed d(seg) W_proj, then scattered to the padded tensor with its padded frames zeroed
    for (int i = 0; i < vp.nseg && seg_grads; ++i) {
        if (!seg_grads[i].feat) continue;
        float* dfp = fptr(scratch, RS.dfeat);
        if (linear_dx(bp.dseg_out[i], segs[i].proj_w, dfp, (int)rp.seg_rows[i], d, segs[i].d_in, nullptr, 1.f, nullptr, comp, st)) return 1;
        if (ragged_rows(seg_grads[i].feat, dfp, tab, rseg, B, segs[i].T, segs[i].d_in, i, 0, st)) return 1;
    }
    return 0;
}

// ---- capacity plan (egx_ragged_cap_*, ABI v24): one captured hipGraph for every batch that fits a declared capacity --------------------------
// The layout of the host plan for B_cap clips, tok_cap tokens and ceil(tok_cap / 48) + B_cap tiles (which bounds sum_b ceil(S_b / 48) of every
// batch that fits and leaves at least (tok_cap - N) / 48 surplus tiles); packed segment rows at min(tok_cap, B_cap T_k). Nothing here reads
// a length: the table is built on the device (ragged_table.hip), stream-ordered, in front of each call's launches.
constexpr int RAGGED_CAP_MAX_TOKENS = 1 << 24;
int ragged_cap_plan(const egx_config* cfg, const egx_segment* segs, int B_cap, int tok_cap, const void* saved, RaggedPlan& rp) {
    EGX_CHECK(cfg && segs, "ragged capacity: null pointer argument");
    EGX_CHECK(B_cap >= 1 && tok_cap >= 1, "ragged capacity: B_cap=%d clips and tok_cap=%d tokens must be at least 1", B_cap, tok_cap);
    Plan& vp = rp.vp;
    if (make_plan(cfg, segs, B_cap, vp)) return 1;
    if (ragged_config_ok(cfg, segs, B_cap, vp, true)) return 1;
    EGX_CHECK(tok_cap <= RAGGED_CAP_MAX_TOKENS, "ragged capacity: tok_cap=%d tokens (at most %d)", tok_cap, RAGGED_CAP_MAX_TOKENS);
    EGX_CHECK((long long)tok_cap >= (long long)B_cap * vp.nseg,
              "ragged capacity: tok_cap=%d tokens cannot hold B_cap=%d clips of %d segments (one frame per segment at least)", tok_cap, B_cap, vp.nseg);
    long long s_pad = 0;
    for (int k = 0; k < vp.nseg; ++k) {
        s_pad += segs[k].T;
        const long long r = (long long)B_cap * segs[k].T;
        rp.seg_rows[k] = (size_t)(r < tok_cap ? r : tok_cap);
    }
    const int S_longest = (int)(s_pad < tok_cap ? s_pad : tok_cap);
    rp.tiles = cdiv(tok_cap, FUSED_TOK_PAD) + B_cap;
    vp.vB = rp.tiles; vp.tpc = 0; vp.N = (size_t)tok_cap; vp.S = S_longest < TILED_MAX_S ? S_longest : TILED_MAX_S;
    rp.tab_words = ragged_cap_table_words(B_cap, rp.tiles);
    rp.sl = saved_layout(cfg, segs, vp, true, saved, rp.tab_words, (size_t)B_cap);
    return 0;
}
// what the two capacity calls refuse alike
int ragged_cap_checks(const egx_config* cfg, const egx_head* head, int training, hipStream_t st) {
    EGX_CHECK(head && head->W, "ragged capacity: a pooled head is required (the head-less rows of a captured batch are not supported yet)");
    if (check_head(head) || check_ce(cfg->ce, true, "")) return 1;
    // (as egx_translator_fwd: a host seed would be baked into the captured graph and every replay would repeat its masks)
    if (training && !cfg->seed_ptr && (cfg->p_drop > 0.f || cfg->p_pos > 0.f)) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
        EGX_CHECK(cs == hipStreamCaptureStatusNone, "training-mode dropout (p > 0) with a host seed cannot be captured in a hipGraph: every replay would "
                  "repeat the same masks; pass egx_config.seed_ptr (model.enable_device_seed()), capture with p = 0, or launch eagerly");
    }
    return 0;
}
RaggedTableParams ragged_cap_table_params(const egx_segment* segs, const RaggedPlan& rp, int tok_cap, const int* lengths, const int64_t* target,
                                          int64_t* eff_target, int* tab, unsigned* status) {
    RaggedTableParams tp;
    memset(&tp, 0, sizeof(tp));
    tp.lengths = lengths; tp.K = rp.vp.nseg; tp.B_cap = rp.vp.B; tp.tok_cap = tok_cap; tp.tile_cap = rp.tiles;
    for (int k = 0; k < rp.vp.nseg; ++k) tp.T_pad[k] = segs[k].T;
    tp.target = target; tp.eff_target = eff_target; tp.tab = tab; tp.status = status;
    return tp;
}
}  // namespace

extern "C" {

int egx_ragged_table_host(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int train, int* out_words, size_t* n_words) {
    EGX_CHECK(cfg && segs && n_words, "ragged table: null pointer argument");
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, nullptr, rp, train != 0)) return 1;
    ragged_head_rows(rp, B, true);
    *n_words = rp.tab.size();
    if (out_words) memcpy(out_words, rp.tab.data(), rp.tab.size() * sizeof(int));
    return 0;
}

int egx_ragged_cap_workspace(const egx_config* cfg, const egx_segment* segs, int B_cap, int tok_cap, size_t* saved_bytes, size_t* scratch_bytes) {
    RaggedPlan rp;
    if (ragged_cap_plan(cfg, segs, B_cap, tok_cap, nullptr, rp)) return 1;
    if (saved_bytes) *saved_bytes = rp.sl.bytes;
    if (scratch_bytes) *scratch_bytes = ragged_train_scratch(cfg, segs, rp, FUSED_HEAD_MAX_OUT).bytes;
    return 0;
}

int egx_ragged_cap_table(const egx_config* cfg, const egx_segment* segs, int B_cap, int tok_cap, const int* lengths, const int64_t* target,
                         int* table, int64_t* eff_target, unsigned* status, size_t* n_words, void* stream) {
    RaggedPlan rp;
    if (ragged_cap_plan(cfg, segs, B_cap, tok_cap, nullptr, rp)) return 1;
    if (n_words) *n_words = rp.tab_words;
    if (!table) return 0;       // (the size query)
    EGX_CHECK(lengths, "ragged capacity: null pointer argument");
    return ragged_table_build(ragged_cap_table_params(segs, rp, tok_cap, lengths, target, eff_target, table, status), (hipStream_t)stream);
}

int egx_ragged_cap_train_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                             const egx_layer* layers, const egx_head* head, int B_cap, int tok_cap, float* logits_out, float* tokens_out,
                             void* saved, void* scratch, unsigned* status, int training, uint64_t seed, void* stream) {
    (void)scratch; (void)tokens_out;
    RaggedPlan rp;
    if (ragged_cap_plan(cfg, segs, B_cap, tok_cap, saved, rp)) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (ragged_cap_checks(cfg, head, training, st)) return 1;
    EGX_CHECK(lengths && saved && ln_w && ln_b && layers && logits_out && status, "ragged capacity: null pointer argument");
    int* tab = (int*)rp.sl.at(rp.sl.tab);
    const int* meta = tab + rp.tab_words - RAGGED_META;
    int64_t* efft = (int64_t*)rp.sl.at(rp.sl.efft);
    const egx_ce* ce = cfg->ce;
    if (ragged_table_build(ragged_cap_table_params(segs, rp, tok_cap, lengths, ce ? ce->target : nullptr, efft, tab, status), st)) return 1;
    // the cross entropy reads the EFFECTIVE targets: an empty clip (and every clip of a refused batch) is -1 there, whatever the caller left
    egx_config c2 = *cfg;
    egx_ce ce2;
    if (ce) { ce2 = *ce; ce2.target = efft; c2.ce = &ce2; }
    if (ragged_forward(&c2, segs, rp, ln_w, ln_b, layers, head, B_cap, logits_out, nullptr, true, training, seed, st, true)) return 1;
    return ce ? ragged_empty_loss(meta, ce->loss, st) : 0;
}

int egx_ragged_cap_bwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                       const egx_layer* layers, const egx_head* head, int B_cap, int tok_cap, const float* d_logits, const float* d_tokens,
                       const void* saved, void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b,
                       const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, unsigned* status, int training, uint64_t seed,
                       void* stream) {
    RaggedPlan rp;
    if (ragged_cap_plan(cfg, segs, B_cap, tok_cap, saved, rp)) return 1;
    hipStream_t st = (hipStream_t)stream;
    if (ragged_cap_checks(cfg, head, training, st)) return 1;
    EGX_CHECK(lengths && d_logits && saved && scratch && ln_w && ln_b && layers && layer_grads && status, "ragged capacity: null pointer argument");
    RaggedTrainScratch RS = ragged_train_scratch(cfg, segs, rp, head->n_out);
    // the table again, from the same device lengths (the backward's own copy, as egx_ragged_bwd's)
    int* tab = (int*)((char*)scratch + RS.tab);
    if (ragged_table_build(ragged_cap_table_params(segs, rp, tok_cap, lengths, nullptr, nullptr, tab, status), st)) return 1;
    const int* rseg = tab + (size_t)B_cap * RAGGED_REC + rp.tiles;
    return ragged_backward(cfg, segs, rp, RS, tab, rseg, rseg + (size_t)B_cap * FUSED_MAX_SEG, ln_w, ln_b, layers, head, B_cap, d_logits, d_tokens,
                           scratch, seg_grads, d_ln_w, d_ln_b, layer_grads, head_grads, training, seed, st);
}

}  // extern "C"

// ---- stage read (ABI v26, test hooks): the intermediates a d = 128 call leaves in `saved` and in the backward's scratch ---------------------
// Read-only: where an item lives comes from the SavedLayout and the scratch plans the launches above use; stage_read.hip turns it into a
// dense matrix in token order. An item the chosen implementation does not hold when its call returns is EGX_STAGE_NOT_KEPT, never a stale read:
//   forward (in `saved` from the forward on, every d = 128 mode): PRE, XIN, QKV, RES1, RES2, HID, ALIVE, and X1 as the bf16 plane(s) the FFN
//     loop multiplied (bf16: one plane, f32s: three, summed exactly); exact-fp32 calls: X1 and G2 are not served (NOT_KEPT);
//   backward (in `scratch` once the backward has returned; per layer and disjoint, bwd_scratch_prefix): G2 (planes like X1), DHID, G1, DQKV,
//     DSEG, and ATTN_O, which the per-clip kernels recompute in the backward and the tiled / ragged calls save in the forward;
//   LSE leaves the attention kernel of the tiled / ragged calls only. DX0 (written only when a learned positional table wants a gradient, which
//   the hook is not told) is UNSUPPORTED: it answers NOT_KEPT whatever the call did.
namespace {
struct StageWhere { bool in_scratch; size_t off; StageReadParams sr; int kind; };
int stage_locate(const egx_config* cfg, const Plan& vp, const TiledView& v, const FusedBwdScratch& SC, const size_t* seg_rows,
                 int item, int layer, StageWhere& w) {
    memset(&w, 0, sizeof(w));
    const SavedLayout& SL = *v.sl;
    const bool bf = cfg->compute == EGX_BF16, planes = split_planes(cfg);
    const size_t N = vp.N, d = vp.d, nd = N * d * 4;
    StageReadParams& sr = w.sr;
    sr.out_bytes = 4; sr.rows = (int)N; sr.cols = (int)d; sr.layout = SR_DENSE;
    sr.S_clip = vp.S; sr.tpc = v.tiled ? v.tpc : 1; sr.rtab = v.rtab; sr.B_clips = v.B_clips;
    w.kind = EGX_STAGE_KIND_F32;
    const bool per_seg = item == EGX_STAGE_DSEG;
    EGX_CHECK(item >= 0 && item < EGX_STAGE_ITEMS, "stage read: item %d (0 .. %d)", item, EGX_STAGE_ITEMS - 1);
    EGX_CHECK(item == EGX_STAGE_PRE || item == EGX_STAGE_DX0 || (layer >= 0 && layer < (per_seg ? vp.nseg : vp.L)),
              "stage read: %s %d out of range", per_seg ? "segment" : "layer", layer);
    const size_t grid = (size_t)vp.vB * FUSED_TOK_PAD;
    auto operand_planes = [&](size_t off) {      // x1 / g2 as the weight-gradient kernel reads them
        sr.layout = SR_PLANES; sr.n_planes = bf ? 1 : 3; sr.plane_stride = grid * d; w.off = off;
        if (bf) w.kind = EGX_STAGE_KIND_BF16;
    };
    switch (item) {
    case EGX_STAGE_PRE: w.off = SL.res; break;
    case EGX_STAGE_RES1: w.off = SL.res + SL.res_index(layer, 0) * 4; break;
    case EGX_STAGE_RES2: w.off = SL.res + SL.res_index(layer, 1) * 4; break;
    case EGX_STAGE_XIN: w.off = SL.xin + layer * nd; break;
    case EGX_STAGE_QKV: sr.layout = SR_GRID; sr.cols = 3 * (int)d; w.off = SL.qkv + layer * SL.qkv_layer; break;
    case EGX_STAGE_X1:
        if (!planes) return EGX_STAGE_NOT_KEPT;         // exact fp32: dense rows in the backward's scratch, not served (no test reads them)
        operand_planes(SL.x1p + layer * SL.x1p_layer);
        break;
    case EGX_STAGE_HID: case EGX_STAGE_DHID:
        sr.layout = SR_HID; sr.cols = vp.dff; sr.bf16 = bf;
        if (bf) w.kind = EGX_STAGE_KIND_BF16;
        w.in_scratch = item == EGX_STAGE_DHID;
        w.off = (w.in_scratch ? SC.dhid : SL.hid) + layer * SL.hid_layer;
        break;
    case EGX_STAGE_ALIVE:
        sr.layout = SR_ALIVE; sr.cols = vp.dff; sr.out_bytes = 1; w.kind = EGX_STAGE_KIND_BIT;
        w.off = SL.relu_bits + layer * SL.relu_layer_words * 4;
        break;
    case EGX_STAGE_G2:
        if (!planes) return EGX_STAGE_NOT_KEPT;         // (as X1)
        w.in_scratch = true;
        operand_planes(SC.g2[layer]);
        break;
    case EGX_STAGE_G1: w.in_scratch = true; w.off = SC.g1[layer]; break;
    case EGX_STAGE_DQKV: w.in_scratch = true; sr.cols = 3 * (int)d; w.off = SC.dqkv[layer]; break;
    case EGX_STAGE_ATTN_O:
        if (v.tiled) w.off = SL.attn + layer * nd;
        else { w.in_scratch = true; w.off = SC.attn_o[layer]; }
        break;
    case EGX_STAGE_DSEG: w.in_scratch = true; sr.rows = (int)seg_rows[layer]; w.off = SC.dseg[layer]; break;
    case EGX_STAGE_LSE:         // (clip, head, token of the clip); a ragged clip's rows start at 4 tok0
        if (!v.tiled) return EGX_STAGE_NOT_KEPT;
        sr.rows = (int)SL.lse_layer_floats; sr.cols = 1; w.off = SL.lse + layer * SL.lse_layer_floats * 4;
        break;
    default: return EGX_STAGE_NOT_KEPT;      // EGX_STAGE_DX0: unsupported (the hook is not told whether a position gradient was requested)
    }
    return 0;
}
int stage_run(const egx_config* cfg, const Plan& vp, const TiledView& v, const FusedBwdScratch& SC, const size_t* seg_rows,
              const void* scratch, int item, int layer, int* rows, int* cols, int* kind, void* out, hipStream_t st) {
    StageWhere w;
    const int rc = stage_locate(cfg, vp, v, SC, seg_rows, item, layer, w);
    if (rc) return rc;
    if (rows) *rows = w.sr.rows;
    if (cols) *cols = w.sr.cols;
    if (kind) *kind = w.kind;
    if (!out) return 0;         // (the shape query)
    const void* base = w.in_scratch ? scratch : v.sl->base;
    EGX_CHECK(base, "stage read: the item lives in `%s`, which is null", w.in_scratch ? "scratch" : "saved");
    EGX_CHECK(w.off < (w.in_scratch ? SC.bytes : v.sl->bytes), "stage read: offset beyond the workspace");
    w.sr.src = (const char*)base + w.off;
    w.sr.out = out;
    return stage_read(w.sr, st);
}
int stage_uniform(const egx_config* cfg, const egx_segment* segs, int B, int head_n_out, const void* saved, const void* scratch, int item, int layer,
                  int* rows, int* cols, int* kind, void* out, void* stream) {
    EGX_CHECK(cfg && segs, "stage read: null config / segments");
    EGX_CHECK(head_n_out >= 0 && head_n_out <= FUSED_HEAD_MAX_OUT, "stage read: head_n_out=%d (0 .. %d)", head_n_out, FUSED_HEAD_MAX_OUT);
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return 1;
    const int impl = egx_encoder_impl(cfg, segs, B);
    if (impl < 0) return 1;
    if (impl != EGX_IMPL_FUSED && impl != EGX_IMPL_TILED) return EGX_STAGE_NOT_KEPT;       // the generic and the wide kernels have workspaces of their own
    const bool tiled = impl == EGX_IMPL_TILED;
    const Plan vp = tiled ? plan_tiled(pl) : pl;
    const SavedLayout SL = saved_layout(cfg, segs, vp, tiled, saved);
    const TiledView v = uniform_view(vp, SL, tiled);
    const FusedBwdScratch SC = fused_bwd_scratch(cfg, segs, vp, head_n_out);
    size_t seg_rows[EGX_MAX_SEGMENTS];
    for (int i = 0; i < pl.nseg; ++i) seg_rows[i] = (size_t)B * segs[i].T;
    return stage_run(cfg, vp, v, SC, seg_rows, scratch, item, layer, rows, cols, kind, out, (hipStream_t)stream);
}
int stage_ragged(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int head_n_out, const void* saved, const void* scratch,
                 int item, int layer, int* rows, int* cols, int* kind, void* out, void* stream) {
    EGX_CHECK(cfg && segs, "stage read: null config / segments");
    EGX_CHECK(head_n_out >= 0 && head_n_out <= FUSED_HEAD_MAX_OUT, "stage read: head_n_out=%d (0 .. %d)", head_n_out, FUSED_HEAD_MAX_OUT);
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, saved, rp, true)) return 1;
    const RaggedTrainScratch RS = ragged_train_scratch(cfg, segs, rp, head_n_out);
    // the forward's copy of the batch table (in `saved`): tile0, tok0 and S of every clip are the same with and without a head
    const int* tab = saved ? (const int*)rp.sl.at(rp.sl.tab) : nullptr;
    EGX_CHECK(!out || tab, "stage read: the ragged batch table lives in `saved`, which is null");
    const TiledView v = ragged_view(rp, B, tab, true);
    return stage_run(cfg, rp.vp, v, RS.sc, rp.seg_rows, scratch, item, layer, rows, cols, kind, out, (hipStream_t)stream);
}
}  // namespace

extern "C" {

int egx_encoder_stage_info(const egx_config* cfg, const egx_segment* segs, int B, int head_n_out, int item, int layer, int* rows, int* cols, int* kind) {
    return stage_uniform(cfg, segs, B, head_n_out, nullptr, nullptr, item, layer, rows, cols, kind, nullptr, nullptr);
}
int egx_encoder_stage_read(const egx_config* cfg, const egx_segment* segs, int B, int head_n_out, const void* saved, const void* scratch, int item,
                           int layer, void* out, void* stream) {
    EGX_CHECK(out, "stage read: null output");
    return stage_uniform(cfg, segs, B, head_n_out, saved, scratch, item, layer, nullptr, nullptr, nullptr, out, stream);
}
int egx_ragged_stage_info(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int head_n_out, int item, int layer, int* rows,
                          int* cols, int* kind) {
    return stage_ragged(cfg, segs, B, lengths, head_n_out, nullptr, nullptr, item, layer, rows, cols, kind, nullptr, nullptr);
}
int egx_ragged_stage_read(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int head_n_out, const void* saved,
                          const void* scratch, int item, int layer, void* out, void* stream) {
    EGX_CHECK(out, "stage read: null output");
    return stage_ragged(cfg, segs, B, lengths, head_n_out, saved, scratch, item, layer, nullptr, nullptr, nullptr, out, stream);
}

}  // extern "C"

// ---- the self-attention weights of a d = 128 call (ABI v27, egx_encoder_self_weights) -------------------------------------------------------
// Every d = 128 forward keeps each layer's fp32 Q | K | V rows on the 48-row tile grid in SavedLayout::qkv (what EGX_STAGE_QKV reads): clip c
// of a uniform call starts at row c * tpc * 48, a ragged clip at 48 x the first tile of its batch-table record, which enc_self_weights_kernel
// reads in place (first tile, S_b and the segments' frame counts), so nothing is built or uploaded here.
namespace egx {
static void self_weights_common(SelfWParams& p, const Plan& vp, float* w_out, float* seg_out, int B, int S) {
    memset(&p, 0, sizeof(p));
    p.ldq = p.ldk = 3 * vp.d; p.K = vp.nseg; p.w = w_out; p.ldw = S; p.seg = seg_out; p.B = B; p.H = vp.H; p.S = S;
}
int fused_self_weights(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool tiled, const void* saved, uint64_t layer_mask,
                       float* w_out, float* seg_out, hipStream_t st) {
    const Plan vp = tiled ? plan_tiled(pl) : pl;
    SelfWParams p;
    self_weights_common(p, vp, w_out, seg_out, pl.B, pl.S);
    p.clip_rows = (long long)vp.tpc * FUSED_TOK_PAD;
    p.fixed_segs = 1;
    for (int i = 0; i < vp.nseg; ++i) p.seg_fixed[i] = segs[i].T;
    const SavedLayout SL = saved_layout(cfg, segs, vp, tiled, saved);
    return self_weights_layers(p, SL.at(SL.qkv), SL.qkv_layer, vp.d, vp.L, layer_mask, true, st);
}
int ragged_self_weights(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, const void* saved, uint64_t layer_mask,
                        float* w_out, float* seg_out, hipStream_t st) {
    RaggedPlan rp;
    if (ragged_plan(cfg, segs, B, lengths, saved, rp, true)) return 1;
    const Plan& vp = rp.vp;
    const SavedLayout& SL = rp.sl;
    const int* tab = (const int*)SL.at(SL.tab);     // the forward's device copy of the batch table
    SelfWParams p;
    self_weights_common(p, vp, w_out, seg_out, B, vp.S);
    p.rowtab = tab; p.tab_stride = RAGGED_REC; p.row_mul = FUSED_TOK_PAD;       // record: RG_TILE0, RG_S
    p.segtab = tab + RG_T; p.seg_stride = RAGGED_REC;
    static_assert(RG_TILE0 == 0 && RG_S == 1, "enc_self_weights_kernel reads (first tile, S_b) at the head of a record");
    return self_weights_layers(p, SL.at(SL.qkv), SL.qkv_layer, vp.d, vp.L, layer_mask, true, st);
}
}  // namespace egx
