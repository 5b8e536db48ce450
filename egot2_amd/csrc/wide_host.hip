// Host orchestration of the wide bf16 path (see wide.h): token preparation + L post-LN encoder layers over all B*S tokens
// as large bf16 MFMA GEMMs with fused epilogues, MFMA attention per (clip, head), row kernels with bf16 side outputs.
// Same call sites as the generic path (include/egot2x.h: egx_encoder_fwd / egx_encoder_bwd); only enqueues kernels.
#include <string.h>
#include <vector>

#include "../../include/egot2x.h"
#include "common.h"
#include "kernels.h"
#include "wide.h"
#include "wide_host.h"
#include "wide_run.h"
#include "fused.h"      // (upload_words: the ragged batch table)

namespace egx {

namespace {

struct WLayer {
    size_t w_in, w_in_t, w_o, w_o_t, w1, w1_t, w2, w2_t;                     // bf16 weight copies
    size_t qkv, lse, attn, res1, stats1, x1_32, x1_16, hid, res2, stats2;    // saved activations
    size_t x16;                                                               // bf16 copy of the layer input
    size_t x32;                                                               // fp32 layer input (layer 0: x0; else previous output)
};
struct WPlan {
    int B, S, d, H, dff, L, nseg;
    size_t N;
    int seg_off[EGX_MAX_SEGMENTS];
    size_t tab;         // ragged training: the device copy of the batch table (the backward reads what the forward uploaded)
    size_t keys;        // dropout keys derived from a device-resident seed (derive_keys): (max(L, nseg) layers) x 8 slots
    size_t zero, seg_w[EGX_MAX_SEGMENTS], seg_feat16[EGX_MAX_SEGMENTS], seg_pre[EGX_MAX_SEGMENTS], seg_stats[EGX_MAX_SEGMENTS];
    WLayer layer[64];
    size_t saved_bytes;
    // scratch
    size_t gA, gB, dres, dy16, dhid16, dattn16, dqkv16, adelta, dseg16, slabs, slab_all, slab_all_bytes, lnpart, cspart, rowpart, rowpart_bytes, scratch_bytes;
};

// a ragged batch (see "ragged batches" below): the host copy of its table
struct WRagged {
    int B = 0, K = 0, layout = 0;
    bool train = false;     // the training entry points; else egx_ragged_encode, whose workspace make_wplan lays out for inference
    size_t N = 0, R[EGX_MAX_SEGMENTS] = {}, Rmax = 0;
    // host copy of the batch table (ints): B clip records (WIDE_RG_REC), the clips of attention class 0 | 1 | 2, per segment the source
    // row (b * segs[k].T + t) and the token row of every compacted row, and (out_layout 1) the output row of every token row
    std::vector<int> tab;
    size_t cls0 = 0, gmap[EGX_MAX_SEGMENTS] = {}, omap[EGX_MAX_SEGMENTS] = {}, outmap = 0;
    int ncls[3] = {0, 0, 0}, Smax[3] = {0, 0, 0};
};

// rg: a ragged batch — N = sum_b S_b packed token rows and R_k compacted rows of segment k instead of B * S and B * T_k; nothing is sized by B * max S_b.
// An inference batch (rg->train false: egx_ragged_encode) keeps nothing for a backward: one set of activation buffers serves every layer and every
// segment, res2 / stats2 reuse res1 / stats1, and no W^T is laid out (offset 0, the zero page's); only `saved` is used.
void make_wplan(const egx_config* cfg, const egx_segment* segs, int B, WPlan& pl, const WRagged* rg = nullptr) {
    memset(&pl, 0, sizeof(pl));
    pl.B = B; pl.d = cfg->d_model; pl.H = cfg->n_heads; pl.dff = cfg->d_ff; pl.L = cfg->n_layers; pl.nseg = cfg->n_segments;
    int S = 0;
    for (int i = 0; i < pl.nseg; ++i) { pl.seg_off[i] = S; S += segs[i].T; }
    pl.S = S; pl.N = rg ? rg->N : (size_t)B * S;
    const bool infer = rg && !rg->train;
    size_t din_max = 0;
    for (int i = 0; i < pl.nseg; ++i) din_max = size_max(din_max, (size_t)segs[i].d_in);
    auto seg_rows = [&](int i) { return rg ? rg->R[i] : (size_t)B * segs[i].T; };
    const size_t d = pl.d, N = pl.N, dff = pl.dff;
    size_t cur = 0;
    auto take_wt = [&](size_t bytes) { return infer ? (size_t)0 : take(cur, bytes); };
    pl.zero = take(cur, 1024);
    pl.keys = take(cur, (size_t)64 * DROP_KEY_SLOTS * sizeof(uint64_t));
    for (int i = 0; i < pl.nseg; ++i) {
        if (segs[i].proj_w) pl.seg_w[i] = take(cur, d * segs[i].d_in * 2);
        if (infer && i > 0) {
            pl.seg_feat16[i] = pl.seg_feat16[0]; pl.seg_pre[i] = pl.seg_pre[0]; pl.seg_stats[i] = pl.seg_stats[0];
            continue;
        }
        const size_t rows = infer ? rg->Rmax : seg_rows(i), din = infer ? din_max : (size_t)segs[i].d_in;
        if (segs[i].proj_w) {
            // bf16 copy of the features (the projection GEMM's operand); features that arrive in bf16 and un-pooled are used in place
            if (rg || !(segs[i].feat_bf16 && segs[i].pool <= 1)) pl.seg_feat16[i] = take(cur, rows * din * 2);
            pl.seg_pre[i] = take(cur, rows * d * 4);
        }
        pl.seg_stats[i] = take(cur, rows * 2 * 4);
    }
    size_t x0_32 = take(cur, N * d * 4);
    for (int l = 0; l < pl.L; ++l) {
        WLayer& o = pl.layer[l];
        if (infer && l > 0) o = pl.layer[0];        // (its weights are replaced below)
        o.w_in = take(cur, 3 * d * d * 2); o.w_in_t = take_wt(3 * d * d * 2);
        o.w_o = take(cur, d * d * 2); o.w_o_t = take_wt(d * d * 2);
        o.w1 = take(cur, dff * d * 2); o.w1_t = take_wt(dff * d * 2);
        o.w2 = take(cur, dff * d * 2); o.w2_t = take_wt(dff * d * 2);
        if (infer && l > 0) continue;
        o.x32 = l == 0 ? x0_32 : take(cur, N * d * 4);
        o.x16 = take(cur, N * d * 2);
        o.qkv = take(cur, N * 3 * d * 2);
        o.lse = take(cur, N * pl.H * 4);        // (B, H, S); ragged: (clip, head) rows from H tok0_b + h S_b
        o.attn = take(cur, N * d * 2);
        o.res1 = take(cur, N * d * 4);
        o.stats1 = take(cur, N * 2 * 4);
        o.x1_32 = take(cur, N * d * 4);
        o.x1_16 = take(cur, N * d * 2);
        o.hid = take(cur, N * dff * 2);
        o.res2 = infer ? o.res1 : take(cur, N * d * 4);
        o.stats2 = infer ? o.stats1 : take(cur, N * 2 * 4);
    }
    if (rg) pl.tab = take(cur, (rg->outmap ? rg->tab.size() : rg->tab.size() + N) * sizeof(int));     // (sized for out_layout 1 either way)
    pl.saved_bytes = cur;

    size_t sc = 0;
    pl.gA = take(sc, N * d * 4);
    pl.gB = take(sc, N * d * 4);
    pl.dres = take(sc, N * d * 4);
    pl.dy16 = take(sc, N * d * 2);
    pl.dhid16 = take(sc, N * dff * 2);
    pl.dattn16 = take(sc, N * d * 2);
    pl.dqkv16 = take(sc, N * 3 * d * 2);
    pl.adelta = take(sc, rg ? (rg->ncls[2] ? N * pl.H * sizeof(float) : 0) : wide_attn_delta_bytes(B, pl.H, S));
    size_t segrows = 0;
    for (int i = 0; i < pl.nseg; ++i) segrows = size_max(segrows, seg_rows(i));
    pl.dseg16 = take(sc, segrows * d * 2);
    size_t slab = 0;
    slab = size_max(slab, wide_gemm_tn_scratch(3 * pl.d, pl.d, (int)N));
    slab = size_max(slab, wide_gemm_tn_scratch(pl.d, pl.d, (int)N));
    slab = size_max(slab, wide_gemm_tn_scratch(pl.dff, pl.d, (int)N));
    slab = size_max(slab, wide_gemm_tn_scratch(pl.d, pl.dff, (int)N));
    for (int i = 0; i < pl.nseg; ++i)
        if (segs[i].proj_w) slab = size_max(slab, wide_gemm_tn_scratch(pl.d, segs[i].d_in, (int)seg_rows(i)));
    pl.slabs = take(sc, slab);
    // one slab region per weight gradient of a backward (their reductions run as ONE launch at its end)
    size_t all = pl.L * wide_slab_bytes({{pl.d, pl.dff, N}, {pl.dff, pl.d, N}, {pl.d, pl.d, N}, {3 * pl.d, pl.d, N}});
    for (int i = 0; i < pl.nseg; ++i)
        if (segs[i].proj_w) all += wide_slab_bytes({{pl.d, segs[i].d_in, seg_rows(i)}});
    if (all > ((size_t)400 << 20)) all = 0;      // measured break-even (wide_encoder_bwd): 283 MB pays, 764 MB does not
    pl.slab_all = take(sc, all);
    pl.slab_all_bytes = all;
    pl.lnpart = take(sc, wide_ln_bwd_scratch((int)N, pl.d));
    const size_t cs_ffn = wide_ffn_colsum_bytes((int)N, pl.dff), cs_in = wide_colsum_scratch((int)N, 3 * pl.d);
    size_t cs = size_max(cs_in, cs_ffn);
    if (!rg) for (int i = 0; i < pl.nseg; ++i) cs = size_max(cs, wide_pos_grad_scratch(B, segs[i].T, pl.d));      // (ragged: no learned-position gradient)
    pl.cspart = take(sc, cs);
    // a partial buffer per deferred row reduction of a backward (wide_row_reduce_flush: ONE launch sums them all at its end):
    // two LayerNorm backwards + the lin1 / in-projection bias column sums per layer
    size_t all_r = wide_rowpart_bytes(pl.L, 2, (int)N, pl.d, {cs_ffn, cs_in});
    if (all_r > ((size_t)256 << 20)) all_r = 0;
    pl.rowpart = take(sc, all_r);
    pl.rowpart_bytes = all_r;
    pl.scratch_bytes = sc;
}

}  // namespace

bool wide_ok(const egx_config* cfg, const egx_segment* segs, int B) {
    (void)B;
    if (cfg->compute != EGX_BF16) return false;
    const int d = cfg->d_model, dff = cfg->d_ff;
    // impl = auto keeps d_model = 128 on the per-clip / fp32-storage kernels (the wide path's extra bf16 roundings sit at the
    // 1e-2 bound there); impl = wide may force it
    if ((d < 256 && cfg->impl != EGX_IMPL_WIDE) || d % 128 != 0 || dff % 128 != 0 || d > 2048 || cfg->n_layers < 1 || cfg->n_layers > 64) return false;
    if (cfg->n_heads <= 0 || d % cfg->n_heads != 0) return false;
    int S = 0;
    for (int i = 0; i < cfg->n_segments; ++i) {
        if (segs[i].proj_w ? (segs[i].d_in % 128 != 0) : (segs[i].d_in != d)) return false;
        S += segs[i].T;
    }
    return wide_attn_supported(S, d / cfg->n_heads);
}

void wide_workspace(const egx_config* cfg, const egx_segment* segs, int B, size_t* saved, size_t* scratch) {
    WPlan pl;
    make_wplan(cfg, segs, B, pl);
    *saved = pl.saved_bytes;
    *scratch = pl.scratch_bytes;
}

// where wide_encoder_fwd leaves layer l's bf16 Q | K | V rows (N x 3d) in `saved` (egx_encoder_self_weights reads them there)
void wide_qkv_offsets(const egx_config* cfg, const egx_segment* segs, int B, size_t* off) {
    WPlan pl;
    make_wplan(cfg, segs, B, pl);
    for (int l = 0; l < pl.L; ++l) off[l] = pl.layer[l].qkv;
}

namespace {
// the context of one encoder call over `pl`: with a device-resident seed the kernels read their keys from the table in `saved` (the forward
// derives it there, the backward finds it)
WideRun encoder_run(const egx_config* cfg, const WPlan& pl, const void* saved, void* scratch, int training, uint64_t seed, hipStream_t st) {
    WideRun r;
    r.saved = (char*)const_cast<void*>(saved); r.scratch = (char*)scratch; r.st = st; r.zero = r.sv<char>(pl.zero);
    r.ln_eps = cfg->ln_eps; r.p_drop = cfg->p_drop; r.training = training; r.seed = seed;
    const bool dev_keys = cfg->seed_ptr && training && (cfg->p_drop > 0.f || cfg->p_pos > 0.f || cfg->p_feat > 0.f);
    r.keys = dev_keys ? r.sv<uint64_t>(pl.keys) : nullptr;
    return r;
}
// layer l's two post-LN sublayers over the plan's buffers; y32 / y16: where the forward's last LayerNorm writes
void encoder_sublayers(const WideRun& r, const WPlan& pl, int l, const egx_layer& w, float* y32, bf16_t* y16, WideProjLn& attn_out, WideFfn& ffn) {
    const WLayer& o = pl.layer[l];
    auto wt = [&](size_t off) { return off ? r.sv<bf16_t>(off) : nullptr; };       // (0: the plan laid out no W^T)
    attn_out = {r.sv<bf16_t>(o.attn), pl.d, r.sv<bf16_t>(o.w_o), wt(o.w_o_t), w.out_proj_b, r.sv<float>(o.x32), r.sv<float>(o.res1),
                r.sv<float>(o.stats1), w.norm1_w, w.norm1_b, r.sv<float>(o.x1_32), r.sv<bf16_t>(o.x1_16), SITE_RES1};
    ffn = {r.sv<bf16_t>(o.x1_16), r.sv<bf16_t>(o.w1), wt(o.w1_t), w.lin1_b, pl.dff, SITE_FFN,
           {r.sv<bf16_t>(o.hid), pl.dff, r.sv<bf16_t>(o.w2), wt(o.w2_t), w.lin2_b, r.sv<float>(o.x1_32), r.sv<float>(o.res2), r.sv<float>(o.stats2),
            w.norm2_w, w.norm2_b, y32, y16, SITE_RES2}};
}
// the self-attention of layer l, forward or (BWD) backward: uniform, or a ragged batch's one launch per attention kernel class
template <bool BWD>
int encoder_attn(const WideRun& r, const WPlan& pl, int l, int B, const WRagged* rg, const int* tab) {
    const WLayer& o = pl.layer[l];
    WideAttnParams a;
    a.qkv = r.sv<bf16_t>(o.qkv); a.out = r.sv<bf16_t>(o.attn); a.lse = r.sv<float>(o.lse);
    if (BWD) { a.delta = r.sc<float>(pl.adelta); a.d_out = r.sc<bf16_t>(pl.dattn16); a.d_qkv = r.sc<bf16_t>(pl.dqkv16); }
    a.B = B; a.S = pl.S; a.H = pl.H; a.d = pl.d;
    const WideDrop da = r.drop(r.p_drop, (uint32_t)l, SITE_ATTN);
    a.drop_key = da.key; a.drop_thresh = da.thresh; a.drop_inv = da.inv;
    if (!rg) return BWD ? wide_attn_bwd(a, r.st) : wide_attn_fwd(a, r.st);
    a.rtab = tab;
    for (int c = 0, first = 0; c < 3; first += rg->ncls[c], ++c) {
        if (!rg->ncls[c]) continue;
        a.B = rg->ncls[c]; a.S = rg->Smax[c]; a.clips = tab + rg->cls0 + first;
        if (BWD ? wide_attn_ragged_bwd(a, r.st) : wide_attn_ragged_fwd(a, r.st)) return 1;
    }
    return 0;
}

// the wide forward over `pl`. rg (with `tab`, the device copy of its table): a ragged batch — token preparation through the row maps, the attention
// one launch per kernel class over the batch table, and (rg->layout 1) the last LayerNorm's rows scattered to the frame-major output; every other
// launch is the uniform one over the pl.N packed token rows.
int encoder_fwd_run(const egx_config* cfg, const WPlan& pl, const egx_segment* segs, const float* ln_w, const float* ln_b, const egx_layer* layers,
                    int B, float* tokens_out, void* saved, int training, uint64_t seed, hipStream_t st, const WRagged* rg, const int* tab) {
    const int d = pl.d, S = pl.S, dff = pl.dff, N = (int)pl.N;
    const WideRun r = encoder_run(cfg, pl, saved, nullptr, training, seed, st);
    // device-resident seed: one small launch advances it (training forward with advance_seed) and derives every key of this
    // call into `saved`; the kernels below read their keys from there, and so does the backward
    if (r.keys && derive_keys(const_cast<uint64_t*>(cfg->seed_ptr), r.sv<uint64_t>(pl.keys), 0, 64, cfg->advance_seed, st)) return 1;
    EGX_HIP(hipMemsetAsync(r.sv<char>(pl.zero), 0, 1024, st));

    // token preparation
    float* x0 = r.sv<float>(pl.layer[0].x32);
    bf16_t* x0_16 = r.sv<bf16_t>(pl.layer[0].x16);
    {   // every weight of this forward -> bf16 (W for the forward, W^T for the input gradients), one launch
        WideCastBatch cb;
        for (int i = 0; i < pl.nseg; ++i)
            if (segs[i].proj_w && wide_cast_add(cb, segs[i].proj_w, d, segs[i].d_in, segs[i].d_in, r.sv<bf16_t>(pl.seg_w[i]), nullptr, st)) return 1;
        auto wt = [&](size_t off) { return off ? r.sv<bf16_t>(off) : nullptr; };       // (0: the plan laid out no W^T)
        for (int l = 0; l < pl.L; ++l) {
            const WLayer& o = pl.layer[l];
            const egx_layer& w = layers[l];
            if (wide_cast_add(cb, w.in_proj_w, 3 * d, d, d, r.sv<bf16_t>(o.w_in), wt(o.w_in_t), st)) return 1;
            if (wide_cast_add(cb, w.out_proj_w, d, d, d, r.sv<bf16_t>(o.w_o), wt(o.w_o_t), st)) return 1;
            if (wide_cast_add(cb, w.lin1_w, dff, d, d, r.sv<bf16_t>(o.w1), wt(o.w1_t), st)) return 1;
            if (wide_cast_add(cb, w.lin2_w, d, dff, dff, r.sv<bf16_t>(o.w2), wt(o.w2_t), st)) return 1;
        }
        if (wide_cast_flush(cb, st)) return 1;
    }
    for (int i = 0; i < pl.nseg; ++i) {
        const egx_segment& sg = segs[i];
        const int rows = rg ? (int)rg->R[i] : B * sg.T;
        const float* pre = sg.feat;
        if (sg.proj_w) {
            const bool in_place = !rg && sg.feat_bf16 && sg.pool <= 1;
            bf16_t* f16 = r.sv<bf16_t>(pl.seg_feat16[i]);
            float* po = r.sv<float>(pl.seg_pre[i]);
            // ragged: the valid frames only, compacted (kept in `saved`: the operand of the projection's weight gradient)
            if (rg && wide_gather_cast(sg.feat, sg.feat_bf16, tab + rg->gmap[i], rows, sg.d_in, f16, st)) return 1;
            if (!rg && !in_place && wide_pool_cast(sg.feat, sg.feat_bf16, rows, sg.pool > 1 ? sg.pool : 1, sg.d_in, f16, st)) return 1;
            if (r.nt(in_place ? reinterpret_cast<const bf16_t*>(sg.feat) : f16, r.sv<bf16_t>(pl.seg_w[i]), rows, d, sg.d_in, sg.proj_b, po, nullptr, 0,
                     r.drop(cfg->p_feat, (uint32_t)i, SITE_FEAT), nullptr)) return 1;
            pre = po;
        }
        WideLnFwdParams lp;
        lp.x = pre; lp.w = ln_w; lp.b = ln_b; lp.eps = cfg->ln_eps;
        lp.stats = r.sv<float>(pl.seg_stats[i]);
        lp.y32 = x0; lp.y16 = x0_16; lp.rows = rows; lp.d = d; lp.T = sg.T; lp.S = S; lp.off = pl.seg_off[i];
        lp.add_vec = sg.add_vec; lp.pos = sg.pos; lp.pos_stride = sg.pos_stride;
        const WideDrop dp = r.drop(cfg->p_pos, 0, SITE_POS);
        lp.drop_key = dp.key; lp.drop_thresh = dp.thresh; lp.drop_inv = dp.inv;
        if (rg) {       // compacted row -> its token row (the positional dropout keys on that row, as in the uniform layout)
            lp.out_map = tab + rg->omap[i]; lp.src_map = tab + rg->gmap[i];
            if (wide_ln_fwd_mapped(lp, st)) return 1;
        } else if (wide_ln_fwd(lp, st)) return 1;
    }

    for (int l = 0; l < pl.L; ++l) {
        const WLayer& o = pl.layer[l];
        const bool last = l + 1 == pl.L;
        WideProjLn attn_out;
        WideFfn ffn;
        encoder_sublayers(r, pl, l, layers[l], last ? tokens_out : r.sv<float>(pl.layer[l + 1].x32), last ? nullptr : r.sv<bf16_t>(pl.layer[l + 1].x16),
                          attn_out, ffn);
        // packed in-projection
        if (r.nt(r.sv<bf16_t>(o.x16), r.sv<bf16_t>(o.w_in), N, 3 * d, d, layers[l].in_proj_b, nullptr, r.sv<bf16_t>(o.qkv), 0, WideDrop(), nullptr)) return 1;
        if (encoder_attn<false>(r, pl, l, B, rg, tab)) return 1;
        if (wide_proj_ln_fwd(r, attn_out, (uint32_t)l, N, d)) return 1;        // out-projection + dropout1 + residual -> res1 -> LayerNorm1
        // linear1 + ReLU + dropout -> hidden; linear2 + dropout2 + residual -> res2 -> LayerNorm2 (the last one of a ragged batch with
        // rg->layout 1: the output in frame-major segment tuples)
        if (wide_ffn_fwd(r, ffn, (uint32_t)l, N, d, last && rg && rg->layout == 1 ? tab + rg->outmap : nullptr)) return 1;
    }
    return 0;
}
}  // namespace

int wide_encoder_fwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b, const egx_layer* layers,
                     int B, float* tokens_out, void* saved, int training, uint64_t seed, hipStream_t st) {
    WPlan pl;
    make_wplan(cfg, segs, B, pl);
    return encoder_fwd_run(cfg, pl, segs, ln_w, ln_b, layers, B, tokens_out, saved, training, seed, st, nullptr, nullptr);
}

namespace {
// the wide backward over `pl`; rg / tab as encoder_fwd_run: the attention backward per kernel class, d_tokens read through the output map
// (rg->layout 1) and the token-preparation backward through the maps the forward scattered with. All other launches are row-wise over pl.N rows.
int encoder_bwd_run(const egx_config* cfg, const WPlan& pl, const egx_segment* segs, const float* ln_w, const egx_layer* layers, int B,
                    const float* d_tokens, const void* saved, void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w,
                    float* d_ln_b, const egx_layer_grads* layer_grads, int training, uint64_t seed, hipStream_t st, const WRagged* rg,
                    const int* tab) {
    const int d = pl.d, S = pl.S, N = (int)pl.N;
    WideRun r = encoder_run(cfg, pl, saved, scratch, training, seed, st);      // (device-resident seed: the forward left this step's keys in `saved`)
    if (cfg->zero_buf && cfg->zero_bytes) EGX_HIP(hipMemsetAsync(cfg->zero_buf, 0, cfg->zero_bytes, st));
    float* gA = r.sc<float>(pl.gA);
    float* gB = r.sc<float>(pl.gB);
    float* dres = r.sc<float>(pl.dres);
    bf16_t* dy16 = r.sc<bf16_t>(pl.dy16);
    bf16_t* dattn16 = r.sc<bf16_t>(pl.dattn16);
    bf16_t* dqkv16 = r.sc<bf16_t>(pl.dqkv16);
    const float* g = d_tokens;

    // weight gradients: when the split-K slabs of the whole backward are small (the d = 256 EgoT2-g encoder: 283 MB, 15
    // reductions of 8 us in 1.6 ms of work) every gradient gets a slab region of its own and ALL slab reductions run as one
    // launch at the end (-2.5 %); for larger problems that reduction reads its slabs back from HBM instead of the Infinity
    // Cache (d = 512: 764 MB, +1.5 %; C4: 1.1 GB, +0.8 %), so they keep the reduction right behind each GEMM on the shared slab.
    // The second stages of the two-stage column sums (LayerNorm / bias gradients) are queued likewise, each with a partial buffer of its
    // own out of `rowpart` (none left: the shared buffer and its own launch). A bucketed exchange defers neither: a layer's gradients
    // must be final when its bucket is announced.
    WideLedger led;
    led.st = led.tn_stream = st; led.zero = r.zero;
    led.slab = r.sc<char>(pl.slab_all); led.slab_bytes = cfg->bucket_cb ? 0 : pl.slab_all_bytes;
    led.rows = r.sc<char>(pl.rowpart); led.rows_bytes = cfg->bucket_cb ? 0 : pl.rowpart_bytes;
    led.lnpart = r.sc<char>(pl.lnpart); led.cspart = r.sc<float>(pl.cspart); led.shared_slab = r.sc<char>(pl.slabs);
    r.led = &led;
    auto no_fork = []() { return 0; };

    for (int l = pl.L - 1; l >= 0; --l) {
        const WLayer& o = pl.layer[l];
        const egx_layer_grads& gw = layer_grads[l];
        WideProjLn attn_out;
        WideFfn ffn;
        encoder_sublayers(r, pl, l, layers[l], nullptr, nullptr, attn_out, ffn);
        // LayerNorm2 and the FFN: g1 = d(x1). d_tokens of a ragged batch in the frame-major layout is read back through the forward's map
        float* g1 = (g == gA) ? gB : gA;
        if (wide_ffn_bwd(r, ffn, {gw.lin1_w, gw.lin1_b, {gw.lin2_w, gw.lin2_b, gw.norm2_w, gw.norm2_b}}, (uint32_t)l, N, d, g, dres, dy16,
                         r.sc<bf16_t>(pl.dhid16), g1, no_fork, rg && rg->layout == 1 && l == pl.L - 1 ? tab + rg->outmap : nullptr)) return 1;
        // LayerNorm1 and the out-projection: dres = d(res1), dy16 = dropout1-mask .* d(res1); d(attention output) = dy W_o
        if (wide_proj_ln_bwd(r, attn_out, {gw.out_proj_w, gw.out_proj_b, gw.norm1_w, gw.norm1_b}, (uint32_t)l, N, d, g1, dres, dy16, no_fork)) return 1;
        if (r.nt_bwd(dy16, attn_out.w_t, N, d, d, nullptr, dattn16, nullptr)) return 1;
        if (encoder_attn<true>(r, pl, l, B, rg, tab)) return 1;
        if (gw.in_proj_b && led.colsum(dqkv16, N, 3 * d, gw.in_proj_b, led.cspart, st)) return 1;
        if (led.dw_tn(dqkv16, r.sv<bf16_t>(o.x16), gw.in_proj_w, 3 * d, d, N)) return 1;
        // d(layer input) = dqkv W_in + d(res1)
        float* g0 = (g1 == gA) ? gB : gA;
        if (r.nt_bwd(dqkv16, r.sv<bf16_t>(o.w_in_t), N, d, 3 * d, g0, nullptr, dres)) return 1;
        g = g0;
        if (cfg->bucket_cb) cfg->bucket_cb(cfg->bucket_user, pl.L - 1 - l);     // every gradient of layer l is enqueued
    }

    // token preparation backward
    const WideDrop dp = r.drop(cfg->p_pos, 0, SITE_POS);
    bf16_t* dseg16 = r.sc<bf16_t>(pl.dseg16);
    for (int i = 0; i < pl.nseg; ++i) {
        const egx_segment& sg = segs[i];
        egx_segment_grads sgr;
        memset(&sgr, 0, sizeof(sgr));
        if (seg_grads) sgr = seg_grads[i];
        // d(features): an identity segment's feature gradient IS the LayerNorm backward's fp32 input gradient (the trainable
        // SlowFast head of the LTA translators feeds such a segment); projected features stay frozen on this path
        EGX_CHECK(!sgr.feat || !sg.proj_w, "wide path: gradients into PROJECTED features are not supported (use impl = generic)");
        const int rows = rg ? (int)rg->R[i] : B * sg.T;
        EGX_CHECK(!rg || !sgr.pos, "ragged encode: a learned positional table gets no gradient from the ragged kernels");
        if (sgr.pos && wide_pos_grad(g, B, S, pl.seg_off[i], sg.T, d, sgr.pos, sg.pos_stride, dp.key, dp.thresh, dp.inv, led.cspart, st)) return 1;
        const bool need = (sg.proj_w && (sgr.proj_w || sgr.proj_b)) || d_ln_w || d_ln_b || sgr.add_vec || sgr.feat;
        if (!need) continue;
        WideLnBwdParams b;
        b.dy = g; b.pre = sg.proj_w ? r.sv<float>(pl.seg_pre[i]) : sg.feat; b.stats = r.sv<float>(pl.seg_stats[i]);
        b.w = ln_w; b.dx16 = sg.proj_w ? dseg16 : nullptr; b.dx32 = sg.proj_w ? nullptr : sgr.feat; b.rows = rows; b.d = d; b.T = sg.T; b.S = S; b.off = pl.seg_off[i];
        b.drop_key = dp.key; b.drop_thresh = dp.thresh; b.drop_inv = dp.inv;
        if (sg.proj_w) {
            const WideDrop df = r.drop(cfg->p_feat, (uint32_t)i, SITE_FEAT);
            b.out_key = df.key; b.out_thresh = df.thresh; b.out_inv = df.inv;
        }
        b.dw = d_ln_w; b.db = d_ln_b; b.dadd = sgr.add_vec; b.dbias = sg.proj_w ? sgr.proj_b : nullptr;
        // (not queued: every segment adds into the SAME shared-LayerNorm gradient; queued reductions run concurrently and must have targets of their own)
        if (rg) {       // compacted row r reads the gradient of its token row (and that row's positional mask)
            b.dy_map = tab + rg->omap[i];
            if (wide_ln_bwd_mapped(b, led.lnpart, st)) return 1;
        } else if (wide_ln_bwd(b, led.lnpart, st)) return 1;
        const bf16_t* f16 = (!rg && sg.feat_bf16 && sg.pool <= 1) ? reinterpret_cast<const bf16_t*>(sg.feat) : r.sv<bf16_t>(pl.seg_feat16[i]);
        if (sg.proj_w && led.dw_tn(dseg16, f16, sgr.proj_w, d, sg.d_in, rows)) return 1;
    }
    return led.flush();
}
}  // namespace

int wide_encoder_bwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const egx_layer* layers, int B,
                     const float* d_tokens, const void* saved, void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w,
                     float* d_ln_b, const egx_layer_grads* layer_grads, int training, uint64_t seed, hipStream_t st) {
    WPlan pl;
    make_wplan(cfg, segs, B, pl);
    return encoder_bwd_run(cfg, pl, segs, ln_w, layers, B, d_tokens, saved, scratch, seg_grads, d_ln_w, d_ln_b, layer_grads, training, seed, st,
                           nullptr, nullptr);
}

// ---- ragged batches (egx_ragged_encode, egx_ragged_encode_train_*) ---------------------------------------------------------------------
// Clip b has T_{b,k} frames per segment and S_b = sum_k T_{b,k} tokens; its tokens are rows [tok0_b, tok0_b + S_b) of every (N, .) array,
// N = sum_b S_b, segment k from row tok0_b + off_{b,k}. Token preparation gathers the valid frames of segment k into R_k = sum_b T_{b,k}
// compacted rows (wide_gather_cast), projects them with one GEMM and scatters them to their token rows in the shared LayerNorm
// (wide_ln_fwd_mapped); GEMMs and row kernels then run over the N token rows as in the uniform forward; the attention runs one launch per
// kernel class over the clips of that class (wide_attn_ragged_fwd). Nothing in the workspace is sized by B * max S_b.
namespace {
// train: the training entry points (dropout allowed). make_wplan lays the workspace out over the table.
int ragged_encode_plan(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int out_layout, WRagged& rp, bool train = false) {
    EGX_CHECK(cfg && segs && lengths, "ragged encode: null argument");
    EGX_CHECK(B >= 1 && B <= (1 << 20), "ragged encode: B=%d clips (1 .. %d)", B, 1 << 20);
    EGX_CHECK(train || (cfg->p_drop == 0.f && cfg->p_pos == 0.f && cfg->p_feat == 0.f),
              "ragged batches are inference-only: p_drop, p_pos and p_feat must be 0 (got %g, %g, %g)", cfg->p_drop, cfg->p_pos, cfg->p_feat);
    EGX_CHECK(!cfg->ce && !cfg->token_ce, "ragged encode: the fused losses (egx_config.ce / token_ce) are not supported; apply the loss to the outputs");
    EGX_CHECK(cfg->out_tokens == 0 && !cfg->bucket_cb, "ragged encode: out_tokens and bucket_cb are not supported");
    EGX_CHECK(!train || cfg->bwd_stage == 0, "ragged encode: the staged backward (bwd_stage) is not supported");
    EGX_CHECK(cfg->compute == EGX_BF16, "ragged encode: runs on the wide bf16 path (compute bf16, got %d)", cfg->compute);
    EGX_CHECK(cfg->impl == EGX_IMPL_AUTO || cfg->impl == EGX_IMPL_WIDE, "ragged encode: runs on the wide path (impl auto or wide, got %d)", cfg->impl);
    EGX_CHECK(out_layout == 0 || out_layout == 1, "ragged encode: out_layout %d (0: packed clips, 1: frame-major segment tuples)", out_layout);
    const int d = cfg->d_model, K = cfg->n_segments, dff = cfg->d_ff, L = cfg->n_layers;
    EGX_CHECK((d >= 256 || cfg->impl == EGX_IMPL_WIDE) && d % 128 == 0 && d <= 1024 && dff % 128 == 0 && dff >= 128 && L >= 1 && L <= 64 &&
              cfg->n_heads > 0 && d % cfg->n_heads == 0 && K >= 1 && K <= EGX_MAX_SEGMENTS,
              "ragged encode: needs d_model %% 128 == 0 in [256, 1024], d_ff %% 128 == 0, 1 .. 64 layers, 1 .. %d segments", EGX_MAX_SEGMENTS);
    const int dh = d / cfg->n_heads;
    for (int k = 0; k < K; ++k)
        EGX_CHECK(segs[k].proj_w && segs[k].d_in % 128 == 0 && segs[k].pool <= 1 && segs[k].T >= 1,
                  "ragged encode: segment %d needs a projection with d_in %% 128 == 0 and no frame pooling", k);
    rp.B = B; rp.K = K; rp.layout = out_layout; rp.train = train;
    rp.tab.assign((size_t)B * WIDE_RG_REC + B, 0);
    size_t tok = 0;
    for (int b = 0; b < B; ++b) {
        int* rec = rp.tab.data() + (size_t)b * WIDE_RG_REC;
        int S = 0;
        for (int k = 0; k < K; ++k) {
            const int T = lengths[(size_t)b * K + k];
            EGX_CHECK(T >= 1 && T <= segs[k].T, "ragged encode: clip %d segment %d has %d frames (1 .. %d, the padded length)", b, k, T, segs[k].T);
            EGX_CHECK(out_layout == 0 || T == lengths[(size_t)b * K], "ragged encode: out_layout 1 needs equal segment lengths in every clip "
                      "(clip %d: segment %d has %d frames, segment 0 %d)", b, k, T, lengths[(size_t)b * K]);
            rec[WRG_T + k] = T; rec[WRG_OFF + k] = S;
            S += T;
            rp.R[k] += T;
        }
        const int c = wide_attn_ragged_class(S, dh);
        EGX_CHECK(c >= 0, "ragged encode: clip %d has S=%d tokens, beyond the wide attention (head dim %d)", b, S, dh);
        rec[WRG_S] = S; rec[WRG_TOK0] = (int)tok;
        rp.ncls[c]++; rp.Smax[c] = S > rp.Smax[c] ? S : rp.Smax[c];
        tok += S;
        EGX_CHECK(tok <= ((size_t)1 << 28), "ragged encode: %zu tokens in one call", tok);
    }
    rp.N = tok;
    rp.cls0 = (size_t)B * WIDE_RG_REC;
    {
        int at[3] = {0, rp.ncls[0], rp.ncls[0] + rp.ncls[1]};
        for (int b = 0; b < B; ++b) {
            const int* rec = rp.tab.data() + (size_t)b * WIDE_RG_REC;
            rp.tab[rp.cls0 + at[wide_attn_ragged_class(rec[WRG_S], dh)]++] = b;
        }
    }
    for (int k = 0; k < K; ++k) {
        rp.gmap[k] = rp.tab.size();
        rp.omap[k] = rp.gmap[k] + rp.R[k];
        rp.tab.resize(rp.omap[k] + rp.R[k]);
        size_t r = 0;
        for (int b = 0; b < B; ++b) {
            const int* rec = rp.tab.data() + (size_t)b * WIDE_RG_REC;
            for (int t = 0; t < rec[WRG_T + k]; ++t, ++r) {
                rp.tab[rp.gmap[k] + r] = b * segs[k].T + t;
                rp.tab[rp.omap[k] + r] = rec[WRG_TOK0] + rec[WRG_OFF + k] + t;
            }
        }
        rp.Rmax = size_max(rp.Rmax, rp.R[k]);
    }
    if (out_layout == 1) {      // token (clip b, segment k, frame t) -> row K (F0_b + t) + k, F0_b = frames of the clips before b
        rp.outmap = rp.tab.size();
        rp.tab.resize(rp.outmap + rp.N);
        size_t F0 = 0;
        for (int b = 0; b < B; ++b) {
            const int* rec = rp.tab.data() + (size_t)b * WIDE_RG_REC;
            for (int k = 0; k < K; ++k)
                for (int t = 0; t < rec[WRG_T + k]; ++t) rp.tab[rp.outmap + rec[WRG_TOK0] + rec[WRG_OFF + k] + t] = (int)(K * (F0 + t) + k);
            F0 += rec[WRG_T];
        }
    }
    return 0;
}

// the forward of a ragged batch (egx_ragged_encode, egx_ragged_encode_train_fwd): table and arguments checked before the first device call
int ragged_encode_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b, const egx_layer* layers,
                      int B, float* tokens_out, int out_layout, void* saved, int training, uint64_t seed, void* stream, bool train, const char* who) {
    WRagged rp;
    if (ragged_encode_plan(cfg, segs, B, lengths, out_layout, rp, train)) return 1;
    EGX_CHECK(ln_w && ln_b && layers && tokens_out && saved, "%s: null pointer argument", who);
    WPlan pl;
    make_wplan(cfg, segs, B, pl, &rp);
    hipStream_t st = (hipStream_t)stream;
    // the batch table into `saved` (a training backward reads it there), stream-ordered in the arguments of upload launches: a captured hipGraph
    // would replay THIS call's lengths for every batch, so the call is not meant for capture
    int* tab = at<int>(saved, pl.tab);
    if (upload_words(tab, rp.tab.data(), rp.tab.size(), st)) return 1;
    return encoder_fwd_run(cfg, pl, segs, ln_w, ln_b, layers, B, tokens_out, saved, training, seed, st, &rp, tab);
}
}  // namespace

}  // namespace egx

using namespace egx;

extern "C" {

int egx_ragged_encode_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* bytes) {
    WRagged rp;
    if (ragged_encode_plan(cfg, segs, B, lengths, 0, rp)) return 1;
    WPlan pl;
    make_wplan(cfg, segs, B, pl, &rp);
    if (bytes) *bytes = pl.saved_bytes;
    return 0;
}

int egx_ragged_encode(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                      const egx_layer* layers, int B, float* tokens_out, int out_layout, void* workspace, void* stream) {
    return ragged_encode_fwd(cfg, segs, lengths, ln_w, ln_b, layers, B, tokens_out, out_layout, workspace, 0, 0, stream, false, "egx_ragged_encode");
}

/* ---- training (the encoder side of HHI/tasks/multitask/video_tasktranslation.py:39-66 on the mixed-length batches its SequenceBatchSampler,
 * :144-156, cannot form; encode() of HHI/models/multitask/task_prompt_model.py:230-258) ---- */
int egx_ragged_encode_train_workspace(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, size_t* saved_bytes,
                                      size_t* scratch_bytes) {
    WRagged rp;
    if (ragged_encode_plan(cfg, segs, B, lengths, 0, rp, true)) return 1;
    WPlan pl;
    make_wplan(cfg, segs, B, pl, &rp);
    if (saved_bytes) *saved_bytes = pl.saved_bytes;
    if (scratch_bytes) *scratch_bytes = pl.scratch_bytes;
    return 0;
}

int egx_ragged_encode_train_fwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const float* ln_b,
                                const egx_layer* layers, int B, float* tokens_out, int out_layout, void* saved, int training, uint64_t seed,
                                void* stream) {
    return ragged_encode_fwd(cfg, segs, lengths, ln_w, ln_b, layers, B, tokens_out, out_layout, saved, training, seed, stream, true,
                             "egx_ragged_encode_train_fwd");
}

int egx_ragged_encode_bwd(const egx_config* cfg, const egx_segment* segs, const int* lengths, const float* ln_w, const egx_layer* layers, int B,
                          const float* d_tokens, int out_layout, const void* saved, void* scratch, const egx_segment_grads* seg_grads,
                          float* d_ln_w, float* d_ln_b, const egx_layer_grads* layer_grads, int training, uint64_t seed, void* stream) {
    WRagged rp;
    if (ragged_encode_plan(cfg, segs, B, lengths, out_layout, rp, true)) return 1;
    EGX_CHECK(ln_w && layers && d_tokens && saved && scratch && layer_grads, "egx_ragged_encode_bwd: null pointer argument");
    for (int k = 0; k < rp.K; ++k) {
        EGX_CHECK(!seg_grads || !seg_grads[k].feat, "ragged encode: gradients into PROJECTED features are not supported");
        EGX_CHECK(!seg_grads || !seg_grads[k].pos, "ragged encode: a learned positional table gets no gradient from the ragged kernels");
    }
    WPlan pl;
    make_wplan(cfg, segs, B, pl, &rp);
    // (the host copy of the table rebuilt from the same lengths gives the offsets; the device copy is the forward's)
    return encoder_bwd_run(cfg, pl, segs, ln_w, layers, B, d_tokens, saved, scratch, seg_grads, d_ln_w, d_ln_b, layer_grads, training, seed,
                           (hipStream_t)stream, &rp, cat<int>(saved, pl.tab));
}

}  // extern "C"
