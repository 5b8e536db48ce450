// C ABI + host orchestration of the translator (see include/egot2x.h for the reference call sites each
// entry point replaces). Everything here only enqueues kernels on the caller's stream: no allocation,
// no synchronisation, hipGraph-capturable.
#include <stdarg.h>
#include <string.h>
#include <stdlib.h>
#include <vector>

#include "../../include/egot2x.h"
#include "common.h"
#include "kernels.h"
#include "fused.h"
#include "fused_host.h"
#include "wide.h"
#include "wide_host.h"
#include "enc_attn_weights.h"

namespace egx {

static thread_local char g_err[1024] = "";

static long long g_launches = 0;
void count_launch() { ++g_launches; }
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- workspace plan (struct Plan: fused_host.h) ------------------------------------------------------------------
int make_plan(const egx_config* cfg, const egx_segment* segs, int B, Plan& pl) {
    EGX_CHECK(cfg && segs, "null config/segments");
    EGX_CHECK(cfg->n_segments >= 1 && cfg->n_segments <= EGX_MAX_SEGMENTS, "n_segments=%d out of range", cfg->n_segments);
    EGX_CHECK(cfg->n_layers >= 0 && cfg->n_layers <= 64, "n_layers=%d out of range", cfg->n_layers);
    EGX_CHECK(cfg->d_model > 0 && cfg->d_model % 4 == 0 && cfg->d_model <= 2048, "d_model=%d unsupported (multiple of 4, <= 1024; <= 2048 with compute bf16, wide path)", cfg->d_model);
    EGX_CHECK(cfg->n_heads > 0 && cfg->d_model % cfg->n_heads == 0, "d_model=%d not divisible by n_heads=%d", cfg->d_model, cfg->n_heads);
    EGX_CHECK(cfg->d_ff > 0 && cfg->d_ff % 4 == 0, "d_ff=%d must be a positive multiple of 4", cfg->d_ff);
    EGX_CHECK(cfg->compute == EGX_F32 || cfg->compute == EGX_BF16 || cfg->compute == EGX_F32_SPLIT, "compute=%d unknown", cfg->compute);
    EGX_CHECK(B > 0, "empty batch (B=%d)", B);
    EGX_CHECK(cfg->out_tokens >= 0, "out_tokens=%d", cfg->out_tokens);
    pl.B = B; pl.vB = B; pl.tpc = 1; pl.d = cfg->d_model; pl.H = cfg->n_heads; pl.dff = cfg->d_ff; pl.L = cfg->n_layers; pl.nseg = cfg->n_segments;
    int S = 0;
    for (int i = 0; i < pl.nseg; ++i) {
        EGX_CHECK(segs[i].T > 0, "segment %d has T=%d", i, segs[i].T);
        EGX_CHECK(segs[i].d_in > 0, "segment %d has d_in=%d", i, segs[i].d_in);
        EGX_CHECK(segs[i].proj_w || segs[i].d_in == pl.d, "segment %d: identity projection needs d_in == d_model", i);
        EGX_CHECK(segs[i].pool >= 0 && (segs[i].proj_w || (!segs[i].feat_bf16 && segs[i].pool <= 1)),
                  "segment %d: bf16 / frame-pooled features need a projection", i);
        pl.seg_off[i] = S;
        S += segs[i].T;
    }
    pl.S = S;
    pl.N = (size_t)B * S;
    // 1024 < d_model <= 2048 (the 2048-wide HOI LTA 2-task translator): the wide bf16 path alone has kernels that wide
    if (cfg->d_model > 1024) {
        const int dh = cfg->d_model / cfg->n_heads;
        EGX_CHECK(cfg->compute == EGX_BF16, "d_model=%d above 1024 needs compute bf16, wide path (got compute %d: f32 / f32s stop at 1024)", cfg->d_model, cfg->compute);
        EGX_CHECK(cfg->impl == EGX_IMPL_AUTO || cfg->impl == EGX_IMPL_WIDE, "d_model=%d above 1024 needs compute bf16, wide path (impl auto or wide, got %d)", cfg->d_model, cfg->impl);
        EGX_CHECK(wide_attn_supported(S, dh),
                  "d_model=%d above 1024 needs compute bf16, wide path, whose attention has no kernel for S=%d tokens at head dim %d "
                  "(S <= 128: head dim 32 / 64 / 96 / 128; S <= %d: head dim 256 / 512)", cfg->d_model, S, dh, WIDE_ATTN_BIGHEAD_MAX_S);
        EGX_CHECK(wide_ok(cfg, segs, B), "d_model=%d above 1024 needs compute bf16, wide path: d_model, d_ff and every projected d_in multiples of 128, "
                  "1 .. 64 layers, identity segments d_model wide", cfg->d_model);
    }
    size_t d = pl.d, N = pl.N;
    size_t cur = 0;
    for (int i = 0; i < pl.nseg; ++i) {
        size_t rows = (size_t)B * segs[i].T;
        pl.seg_pre[i] = take(cur, rows * d * 4);
        pl.seg_stats[i] = take(cur, rows * 2 * 4);
    }
    for (int l = 0; l < pl.L; ++l) {
        LayerOff& o = pl.layer[l];
        o.x_in = take(cur, N * d * 4);
        o.qkv = take(cur, N * 3 * d * 4);
        o.lse = take(cur, (size_t)B * pl.H * S * 4);
        o.attn_o = take(cur, N * d * 4);
        o.res1 = take(cur, N * d * 4);
        o.stats1 = take(cur, N * 2 * 4);
        o.x1 = take(cur, N * d * 4);
        o.hid = take(cur, N * (size_t)pl.dff * 4);
        o.res2 = take(cur, N * d * 4);
        o.stats2 = take(cur, N * 2 * 4);
    }
    pl.saved_bytes = cur;

    size_t sc = 0;
    pl.s_dA = take(sc, N * d * 4);
    pl.s_dB = take(sc, N * d * 4);
    pl.s_dqkv = take(sc, N * 3 * d * 4);
    pl.s_dhid = take(sc, N * (size_t)pl.dff * 4);
    size_t slab = 0;
    auto upd = [&](int M, int Nn, int K) { slab = size_max(slab, gemm_scratch_bytes(2, M, Nn, K)); };
    upd(3 * pl.d, pl.d, (int)N);
    upd(pl.d, pl.d, (int)N);
    upd(pl.dff, pl.d, (int)N);
    upd(pl.d, pl.dff, (int)N);
    for (int i = 0; i < pl.nseg; ++i)
        if (segs[i].proj_w) upd(pl.d, segs[i].d_in, B * segs[i].T);
    pl.slab_bytes = slab;
    pl.s_slab = take(sc, slab);
    pl.det_bytes = cfg->deterministic ? generic_det_scratch_bytes(B, pl.d, pl.dff) : 0;
    pl.s_det = take(sc, pl.det_bytes);
    pl.scratch_bytes = sc;
    return 0;
}

// The one reader of the kernel-selection switches (struct Tuning, common.h); comm.hip reads EGX_RCCL_LIB, a library path, when RCCL is first resolved.
static Tuning g_tuning;
static bool g_tuning_loaded = false;
static void tuning_load() {
    Tuning t;
    if (const char* e = getenv("EGX_FFN_CUT")) t.ffn_cut = e[0] != '0' ? 1 : 0;
    if (const char* e = getenv("EGX_FFN_SLICES")) { t.has_slices = true; t.slices_cap = atoi(e); }
    if (const char* e = getenv("EGX_SLICE_DROP")) { t.has_drop = true; t.slice_drop = strtol(e, nullptr, 16); }
    if (const char* e = getenv("EGX_DEC_GROUP")) t.dec_group = atoi(e);
    if (const char* e = getenv("EGX_WIDE_TILE")) t.wide_tile = atoi(e);
    if (const char* e = getenv("EGX_DEC_SIDE")) t.dec_side = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;
    g_tuning = t;
    g_tuning_loaded = true;
}
const Tuning& tuning() { if (!g_tuning_loaded) tuning_load(); return g_tuning; }

static bool use_tiled(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool* err) {
    *err = false;
    const bool ok = tiled_ok(cfg, segs, pl);
    if (cfg->impl == EGX_IMPL_TILED) {
        if (!ok) { set_error("tiled implementation does not support this configuration (needs d=128, h=4, 48 < S <= %d, compute bf16 or f32s, d_ff%%128==0, projected segments, <=4 layers)", TILED_MAX_S); *err = true; }
        return ok;
    }
    return cfg->impl == EGX_IMPL_AUTO && ok;
}

static bool use_fused(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool* err) {
    *err = false;
    bool ok = fused_ok(cfg, segs, pl);
    if (cfg->impl == EGX_IMPL_FUSED) {
        if (!ok) { set_error("fused implementation does not support this configuration (needs d=128, h=4 or 8, S<=48, d_ff%%128==0, projected segments, <=%d layers)", FUSED_MAX_LAYERS); *err = true; }
        return ok;
    }
    return cfg->impl == EGX_IMPL_AUTO && ok;   // auto: fused per-clip kernels whenever the shape allows
}

// wide bf16 path (wide_host.hip): bf16 compute outside the fused kernels' shape, whenever its alignment rules hold
static bool use_wide(const egx_config* cfg, const egx_segment* segs, const Plan& pl, bool* err) {
    *err = false;
    const bool ok = wide_ok(cfg, segs, pl.B);
    if (cfg->impl == EGX_IMPL_WIDE) {
        if (!ok) { set_error("wide implementation does not support this configuration (needs compute = bf16, d_model >= 256, d_model / d_ff / projected d_in multiples of 128, S <= 128 with head dim 32 / 64 / 96 / 128, S <= 480 with head dim 32 / 64 or S <= 16 with head dim 256 / 512; d_model <= 2048)"); *err = true; }
        return ok;
    }
    return cfg->impl == EGX_IMPL_AUTO && ok && !fused_ok(cfg, segs, pl);
}

static int linear_nt(const float* x, const float* W, const float* bias, float* y, int M, int N, int K, int relu,
                     const Drop& dr, const float* residual, int compute, hipStream_t st) {
    GemmParams g;
    g.A = x; g.B = W; g.C = y;
    g.M = M; g.N = N; g.K = K;
    g.lda = K; g.ldb = K; g.ldc = N;
    g.bias = bias;
    g.relu = relu;
    g.drop_key = dr.key; g.drop_thresh = dr.thresh; g.drop_inv_keep = dr.inv_keep;
    g.residual = residual; g.ldr = N;
    return gemm(0, g, compute, 0, nullptr, 0, st);
}

// dx[M,K] = dy[M,N] W[N,K]  (+ mask/scale, + residual)
int linear_dx(const float* dy, const float* W, float* dx, int M, int N, int K, const float* mask, float mask_scale,
              const float* residual, int compute, hipStream_t st, void* slab, size_t slab_bytes) {
    GemmParams g;
    g.A = dy; g.B = W; g.C = dx;
    g.M = M; g.N = K; g.K = N;
    g.lda = N; g.ldb = K; g.ldc = K;
    g.mask = mask; g.ldm = K; g.mask_scale = mask_scale;
    g.residual = residual; g.ldr = K;
    return gemm(1, g, compute, 0, slab, slab_bytes, st);    // slab scratch (optional): lets a skinny dx split its reduction
}

// dW[N,K] += dy[M,N]^T x[M,K]
static int linear_dw(const float* dy, const float* x, float* dW, int M, int N, int K, int compute, void* slab,
                     size_t slab_bytes, hipStream_t st) {
    GemmParams g;
    g.A = dy; g.B = x; g.C = dW;
    g.M = N; g.N = K; g.K = M;
    g.lda = N; g.ldb = K; g.ldc = K;
    return gemm(2, g, compute, 1, slab, slab_bytes, st);
}

int debug_read_ppstamps(unsigned long long* out);       // wide_gemm.hip (development aid)
int debug_read_cstamps(unsigned long long* out);        // ffn_cut.hip (development aid)
int debug_read_sstamps(unsigned long long* out);        // small_dw_kernel (development aid)

}  // namespace egx

using namespace egx;

extern "C" {

int egx_abi_version(void) { return EGX_ABI_VERSION; }
void egx_tuning_reload(void) { tuning_load(); }
long long egx_launch_count(int reset) { long long n = g_launches; if (reset) g_launches = 0; return n; }
int egx_debug_stamps(unsigned long long* out, int n) { return n == -1000 ? debug_read_ppstamps(out) : n == -3000 ? debug_read_cstamps(out) : n == -4000 ? debug_read_sstamps(out) : (n < 0 ? debug_read_bstamps(out, -n) : debug_read_stamps(out, n)); }
long long egx_slices_stolen(int reset) {
    const long long a = slices_stolen_fwd(reset), b = slices_stolen_bwd(reset);
    return a < 0 || b < 0 ? -1 : a + b;
}
int egx_seed_advance(uint64_t* seed, void* stream) { EGX_CHECK(seed, "null seed"); return seed_advance(seed, (hipStream_t)stream); }
void egx_timing_enable(int on) { timing_enable(on); }
int egx_timing_read(int which, double* total_ms, int* count) { return timing_read(which, total_ms, count); }

// Unit-test hook for the fused FFN weight-gradient kernel. scratch: packed W1 + packed W2^T + slabs.
size_t egx_ffn_dw_scratch(int N, int d_ff, int compute) {
    int bf = compute;
    return 2 * align_up(packed_bytes(d_ff, 128, bf), 256) + ffn_dw_scratch_bytes(N, d_ff, nullptr);
}
int egx_ffn_dw(const float* x1, const float* g, const float* W1, const float* b1, const float* W2, int N, int S, int d_ff,
               float p_drop, uint64_t seed, float* dW1, float* db1, float* dW2, int compute, void* scratch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int bf = compute;
    PackParams pk;
    memset(&pk, 0, sizeof(pk));
    pk.mode = bf;
    char* cur = (char*)scratch;
    pk.d[0].src = W1; pk.d[0].dst = cur; pk.d[0].R = d_ff; pk.d[0].K = 128; pk.d[0].ld = 128; pk.d[0].transpose = 0;
    cur += align_up(packed_bytes(d_ff, 128, bf), 256);
    pk.d[1].src = W2; pk.d[1].dst = cur; pk.d[1].R = d_ff; pk.d[1].K = 128; pk.d[1].ld = d_ff; pk.d[1].transpose = 1;
    cur += align_up(packed_bytes(d_ff, 128, bf), 256);
    pk.n = 2;
    if (pack_weights(pk, st)) return 1;
    FfnDwParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.x1 = x1; fp.g = g; fp.w1p = pk.d[0].dst; fp.w2tp = pk.d[1].dst; fp.b1 = b1;
    fp.N = N; fp.S = S; fp.d_ff = d_ff;
    Drop dh = make_drop(p_drop > 0.f, p_drop, seed, 0, SITE_FFN);
    fp.drop_key = dh.key; fp.drop_thresh = dh.thresh; fp.drop_inv = dh.inv_keep;
    return ffn_dw(fp, compute, dW1, db1, dW2, cur, st);
}
const char* egx_last_error(void) { return g_err; }

// ---- unit hooks of the wide bf16 path ----------------------------------------------------------------------------
size_t egx_wide_gemm_scratch(int layout, int M, int N, int K) { return 1024 + (layout == 2 ? wide_gemm_tn_scratch(M, N, K) : 0); }
int egx_wide_gemm(int layout, const void* A, const void* B, float* Cf, void* Cb, int M, int N, int K, const float* bias,
                  int relu, const float* residual, void* scratch, void* stream) {
    EGX_CHECK(layout == 0 || layout == 2, "egx_wide_gemm: layout %d (0 = NT, 2 = TN)", layout);
    EGX_CHECK(scratch, "egx_wide_gemm: null scratch");
    hipStream_t st = (hipStream_t)stream;
    EGX_HIP(hipMemsetAsync(scratch, 0, 1024, st));
    WideGemmParams g;
    g.A = (const bf16_t*)A; g.B = (const bf16_t*)B; g.M = M; g.N = N; g.K = K;
    g.Cf = Cf; g.Cb = (bf16_t*)Cb; g.ldc = N; g.bias = bias; g.relu = relu; g.residual = residual; g.ldr = N;
    g.zero_page = scratch;
    if (layout == 0) { g.lda = K; g.ldb = K; return wide_gemm_nt(g, st); }
    g.lda = M; g.ldb = N;
    return wide_gemm_tn(g, (char*)scratch + 1024, st);
}
static int wide_attn_hook(const void* qkv, void* out, float* lse, const void* d_out, void* d_qkv, float* delta, int B, int S, int H, int d,
                          float p_drop, uint64_t seed, void* stream, bool bwd) {
    WideAttnParams a;
    a.qkv = (const bf16_t*)qkv; a.out = (bf16_t*)out; a.lse = lse; a.d_out = (const bf16_t*)d_out; a.d_qkv = (bf16_t*)d_qkv; a.delta = delta;
    a.B = B; a.S = S; a.H = H; a.d = d;
    if (p_drop > 0.f) { a.drop_key = site_key(seed, 0, SITE_ATTN); a.drop_thresh = drop_threshold(p_drop); a.drop_inv = p_drop < 1.f ? 1.f / (1.f - p_drop) : 0.f; }
    return bwd ? wide_attn_bwd(a, (hipStream_t)stream) : wide_attn_fwd(a, (hipStream_t)stream);
}
int egx_wide_attention_fwd(const void* qkv, void* out, float* lse, int B, int S, int H, int d, float p_drop, uint64_t seed, void* stream) {
    return wide_attn_hook(qkv, out, lse, nullptr, nullptr, nullptr, B, S, H, d, p_drop, seed, stream, false);
}
int egx_wide_attention_bwd(const void* qkv, const void* out, const float* lse, const void* d_out, void* d_qkv, float* delta, int B, int S,
                           int H, int d, float p_drop, uint64_t seed, void* stream) {
    return wide_attn_hook(qkv, const_cast<void*>(out), const_cast<float*>(lse), d_out, d_qkv, delta, B, S, H, d, p_drop, seed, stream, true);
}

// ABI v25: every kernel of the wide path on its own. The hooks check their arguments, fill the production parameter structs and call the
// production functions; the dropout triple is the one wide_host.hip's mkdrop forms from a host seed.
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static int hook_drop(const char* who, float p, uint64_t seed, uint32_t layer, uint32_t site, uint64_t* key, uint32_t* thresh, float* inv) {
    EGX_CHECK(p >= 0.f && p <= 1.f, "%s: dropout probability %g outside [0, 1]", who, (double)p);
    *key = 0; *thresh = 0; *inv = 1.f;
    if (p > 0.f) { *key = site_key(seed, layer, site); *thresh = drop_threshold(p); *inv = p < 1.f ? 1.f / (1.f - p) : 0.f; }
    return 0;
}
static int wide_gemm_fill(const egx_wide_gemm_args* a, WideGemmParams& g) {
    EGX_CHECK(a, "egx_wide_gemm_ex: null arguments");
    EGX_CHECK(a->layout == 0 || a->layout == 2, "egx_wide_gemm_ex: layout %d (0 = NT, 2 = TN)", a->layout);
    EGX_CHECK(a->A && a->B && a->scratch, "egx_wide_gemm_ex: null operand or scratch");
    EGX_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "egx_wide_gemm_ex: empty problem %dx%dx%d", a->M, a->N, a->K);
    EGX_CHECK(al16(a->A) && al16(a->B) && al16(a->Cf) && al16(a->Cb) && al16(a->bias) && al16(a->residual) && al16(a->mask) && al16(a->colsum) &&
              al16(a->scratch), "egx_wide_gemm_ex: pointers must be 16-byte aligned");
    EGX_CHECK(a->lda % 8 == 0 && a->ldb % 8 == 0 && a->ldc % 4 == 0 && a->ldc >= a->N, "egx_wide_gemm_ex: lda %d, ldb %d (multiples of 8), ldc %d (multiple of 4, >= N)",
              a->lda, a->ldb, a->ldc);
    if (a->layout == 0) {
        EGX_CHECK(a->Cf || a->Cb, "egx_wide_gemm_ex: NT needs Cf or Cb");
        EGX_CHECK(a->K % 64 == 0 && a->N % 4 == 0, "egx_wide_gemm_ex: NT %dx%dx%d needs K %% 64 == 0 and N %% 4 == 0", a->M, a->N, a->K);
        EGX_CHECK(a->lda >= a->K && a->ldb >= a->K, "egx_wide_gemm_ex: NT lda %d, ldb %d below K", a->lda, a->ldb);
        EGX_CHECK(!a->residual || (a->ldr >= a->N && a->ldr % 4 == 0), "egx_wide_gemm_ex: ldr %d (multiple of 4, >= N)", a->ldr);
        EGX_CHECK(!a->mask || (a->ldm >= a->N && a->ldm % 4 == 0), "egx_wide_gemm_ex: ldm %d (multiple of 4, >= N)", a->ldm);
        EGX_CHECK(!a->accumulate && !a->tn_queue && !a->tn_defer, "egx_wide_gemm_ex: accumulate / tn_queue / tn_defer are TN switches");
    } else {
        EGX_CHECK(a->Cf && !a->Cb, "egx_wide_gemm_ex: TN writes Cf only");
        EGX_CHECK(a->M % 128 == 0 && a->N % 128 == 0, "egx_wide_gemm_ex: TN %dx%dx%d needs M, N multiples of 128", a->M, a->N, a->K);
        EGX_CHECK(a->lda >= a->M && a->ldb >= a->N, "egx_wide_gemm_ex: TN lda %d below M or ldb %d below N", a->lda, a->ldb);
        EGX_CHECK(!a->bias && !a->relu && a->p_drop == 0.f && !a->residual && !a->mask && !a->colsum, "egx_wide_gemm_ex: TN has no epilogue");
    }
    g.A = (const bf16_t*)a->A; g.B = (const bf16_t*)a->B; g.M = a->M; g.N = a->N; g.K = a->K; g.lda = a->lda; g.ldb = a->ldb;
    g.Cf = a->Cf; g.Cb = (bf16_t*)a->Cb; g.ldc = a->ldc; g.bias = a->bias; g.relu = a->relu;
    if (hook_drop("egx_wide_gemm_ex", a->p_drop, a->seed, a->layer, a->site, &g.drop_key, &g.drop_thresh, &g.drop_inv)) return 1;
    g.residual = a->residual; g.ldr = a->ldr; g.mask = (const bf16_t*)a->mask; g.ldm = a->ldm; g.mask_scale = a->mask_scale;
    g.colsum = a->colsum; g.accumulate = a->accumulate; g.zero_page = a->scratch;
    return 0;
}
int egx_wide_gemm_tn_batch(const egx_wide_gemm_args* args, int n, void* stream) {
    EGX_CHECK(args && n >= 1 && n <= 32, "egx_wide_gemm_tn_batch: %d problems (1 .. 32)", n);
    hipStream_t st = (hipStream_t)stream;
    std::vector<WideGemmParams> g(n);
    for (int i = 0; i < n; ++i) {
        if (wide_gemm_fill(args + i, g[i])) return 1;
        EGX_CHECK(args[i].layout == 2, "egx_wide_gemm_tn_batch: problem %d is not TN", i);
    }
    WideTnQueue Q;
    WideReduceBatch red;
    for (int i = 0; i < n; ++i) {
        EGX_HIP(hipMemsetAsync(args[i].scratch, 0, 1024, st));
        void* slabs = (char*)args[i].scratch + 1024;
        if (args[i].tn_queue ? wide_tn_queue_add(Q, g[i], slabs, st, &red) : wide_gemm_tn(g[i], slabs, st, args[i].tn_defer ? &red : nullptr)) return 1;
    }
    if (wide_tn_queue_flush(Q, st)) return 1;
    return wide_reduce_flush(red, st);
}
int egx_wide_gemm_ex(const egx_wide_gemm_args* args, void* stream) {
    WideGemmParams g;
    if (wide_gemm_fill(args, g)) return 1;
    if (args->layout == 2) return egx_wide_gemm_tn_batch(args, 1, stream);
    EGX_HIP(hipMemsetAsync(args->scratch, 0, 1024, (hipStream_t)stream));
    return wide_gemm_nt(g, (hipStream_t)stream);
}
int egx_wide_gemm_colsum_rows(int M, int N) { return M > 0 && N > 0 ? wide_gemm_nt_colsum_rows(M, N) : 0; }
int egx_wide_gemm_variant(int layout, int M, int N, int K, int colsum) {
    if (M <= 0 || N <= 0 || K <= 0) return -1;
    if (layout == 0) return K % 64 == 0 && N % 4 == 0 ? wide_gemm_nt_launch(M, N, colsum != 0) : -1;
    return layout == 2 ? wide_gemm_tn_launch(M, N, K) : -1;
}

int egx_wide_layernorm_fwd(const egx_wide_ln_fwd_args* a, void* stream) {
    EGX_CHECK(a, "egx_wide_layernorm_fwd: null arguments");
    EGX_CHECK(a->x && a->w && a->b && (a->y32 || a->y16), "egx_wide_layernorm_fwd: null pointer");
    EGX_CHECK(a->rows >= 0 && a->d > 0 && a->d % 4 == 0 && a->d <= (a->out_map ? 1024 : 2048), "egx_wide_layernorm_fwd: d=%d unsupported (multiple of 4, <= %d)",
              a->d, a->out_map ? 1024 : 2048);
    EGX_CHECK(al16(a->x) && al16(a->w) && al16(a->b) && al16(a->y32) && al16(a->y16) && al16(a->add_vec) && al16(a->pos) && ((uintptr_t)a->stats & 7) == 0,
              "egx_wide_layernorm_fwd: pointers must be 16-byte aligned");
    EGX_CHECK(a->T >= 1 && a->S >= 1 && (a->out_map || (a->off >= 0 && a->off + a->T <= a->S)), "egx_wide_layernorm_fwd: T=%d, S=%d, off=%d", a->T, a->S, a->off);
    EGX_CHECK(!a->pos || (a->pos_stride >= a->d && a->pos_stride % 4 == 0), "egx_wide_layernorm_fwd: pos_stride %d (multiple of 4, >= d)", a->pos_stride);
    EGX_CHECK(a->out_map || !a->src_map, "egx_wide_layernorm_fwd: src_map without out_map");
    WideLnFwdParams p;
    p.x = a->x; p.w = a->w; p.b = a->b; p.eps = a->eps; p.stats = a->stats; p.y32 = a->y32; p.y16 = (bf16_t*)a->y16;
    p.rows = a->rows; p.d = a->d; p.T = a->T; p.S = a->S; p.off = a->off; p.add_vec = a->add_vec; p.pos = a->pos; p.pos_stride = a->pos_stride;
    if (hook_drop("egx_wide_layernorm_fwd", a->p_drop, a->seed, a->layer, a->site, &p.drop_key, &p.drop_thresh, &p.drop_inv)) return 1;
    p.out_map = a->out_map; p.src_map = a->src_map;
    return a->out_map ? wide_ln_fwd_mapped(p, (hipStream_t)stream) : wide_ln_fwd(p, (hipStream_t)stream);
}
size_t egx_wide_layernorm_bwd_scratch(int rows, int d) { return rows > 0 && d > 0 ? wide_ln_bwd_scratch(rows, d) : 0; }
static int ln_bwd_fill(const egx_wide_ln_bwd_args* a, WideLnBwdParams& p) {
    EGX_CHECK(a, "egx_wide_layernorm_bwd: null arguments");
    EGX_CHECK(a->dy && a->pre && a->stats && a->w && a->scratch, "egx_wide_layernorm_bwd: null pointer");
    EGX_CHECK(a->rows >= 0 && a->d > 0 && a->d % 4 == 0 && a->d <= (a->dy_map ? 1024 : 2048), "egx_wide_layernorm_bwd: d=%d unsupported (multiple of 4, <= %d)",
              a->d, a->dy_map ? 1024 : 2048);
    EGX_CHECK(al16(a->dy) && al16(a->pre) && al16(a->w) && al16(a->dx32) && al16(a->dx16) && al16(a->scratch) && ((uintptr_t)a->stats & 7) == 0,
              "egx_wide_layernorm_bwd: pointers must be 16-byte aligned");
    EGX_CHECK(a->T >= 1 && a->S >= 1 && (a->dy_map || (a->off >= 0 && a->off + a->T <= a->S)), "egx_wide_layernorm_bwd: T=%d, S=%d, off=%d", a->T, a->S, a->off);
    EGX_CHECK(!a->defer || !a->dy_map, "egx_wide_layernorm_bwd: the mapped form never defers its reduction");
    p.dy = a->dy; p.pre = a->pre; p.stats = a->stats; p.w = a->w; p.dx32 = a->dx32; p.dx16 = (bf16_t*)a->dx16;
    p.rows = a->rows; p.d = a->d; p.T = a->T; p.S = a->S; p.off = a->off;
    if (hook_drop("egx_wide_layernorm_bwd", a->p_drop, a->seed, a->layer, a->site, &p.drop_key, &p.drop_thresh, &p.drop_inv)) return 1;
    if (hook_drop("egx_wide_layernorm_bwd", a->p_out, a->seed, a->out_layer, a->out_site, &p.out_key, &p.out_thresh, &p.out_inv)) return 1;
    p.mask_dx32 = a->mask_dx32; p.dw = a->dw; p.db = a->db; p.dbias = a->dbias; p.dadd = a->dadd; p.dy_map = a->dy_map;
    return 0;
}
static int colsum_args_ok(const void* x, int rows, int cols, int ld, const float* out, const void* scratch) {
    EGX_CHECK(x && out && scratch, "egx_wide_colsum: null pointer");
    EGX_CHECK(rows >= 0 && cols > 0 && cols % 8 == 0 && ld % 8 == 0 && ld >= cols, "egx_wide_colsum: %dx%d, ld %d (cols, ld multiples of 8, ld >= cols)", rows, cols, ld);
    EGX_CHECK(al16(x) && al16(scratch), "egx_wide_colsum: pointers must be 16-byte aligned");
    return 0;
}
int egx_wide_row_reduce_batch(const egx_wide_ln_bwd_args* ln, int n_ln, const egx_wide_colsum_args* cs, int n_cs, void* stream) {
    EGX_CHECK(n_ln >= 0 && n_cs >= 0 && n_ln + n_cs >= 1 && n_ln + n_cs <= WIDE_ROWRED_MAX && (ln || !n_ln) && (cs || !n_cs),
              "egx_wide_row_reduce_batch: %d + %d reductions (1 .. %d)", n_ln, n_cs, WIDE_ROWRED_MAX);
    std::vector<WideLnBwdParams> p(n_ln);
    for (int i = 0; i < n_ln; ++i) {
        if (ln_bwd_fill(ln + i, p[i])) return 1;
        EGX_CHECK(!ln[i].dy_map, "egx_wide_row_reduce_batch: the mapped LayerNorm backward never defers its reduction");
    }
    for (int i = 0; i < n_cs; ++i)
        if (colsum_args_ok(cs[i].x, cs[i].rows, cs[i].cols, cs[i].ld, cs[i].out, cs[i].scratch)) return 1;
    hipStream_t st = (hipStream_t)stream;
    WideRowReduceBatch red;
    for (int i = 0; i < n_ln; ++i)
        if (wide_ln_bwd(p[i], ln[i].scratch, st, &red)) return 1;
    for (int i = 0; i < n_cs; ++i)
        if (wide_colsum_bf16((const bf16_t*)cs[i].x, cs[i].rows, cs[i].cols, cs[i].ld, cs[i].out, cs[i].scratch, st, &red)) return 1;
    return wide_row_reduce_flush(red, st);
}
int egx_wide_layernorm_bwd(const egx_wide_ln_bwd_args* a, void* stream) {
    WideLnBwdParams p;
    if (ln_bwd_fill(a, p)) return 1;
    if (a->dy_map) return wide_ln_bwd_mapped(p, a->scratch, (hipStream_t)stream);
    if (!a->defer) return wide_ln_bwd(p, a->scratch, (hipStream_t)stream);
    return egx_wide_row_reduce_batch(a, 1, nullptr, 0, stream);
}

size_t egx_wide_colsum_scratch(int rows, int cols) { return rows > 0 && cols > 0 ? wide_colsum_scratch(rows, cols) : 0; }
int egx_wide_colsum(const void* x, int rows, int cols, int ld, float* out, int defer, void* scratch, void* stream) {
    if (colsum_args_ok(x, rows, cols, ld, out, scratch)) return 1;
    if (!defer) return wide_colsum_bf16((const bf16_t*)x, rows, cols, ld, out, scratch, (hipStream_t)stream);
    const egx_wide_colsum_args one = {x, rows, cols, ld, out, scratch};
    return egx_wide_row_reduce_batch(nullptr, 0, &one, 1, stream);
}
size_t egx_wide_pos_grad_scratch(int B, int T, int d) { return B > 0 && T > 0 && d > 0 ? wide_pos_grad_scratch(B, T, d) : 0; }
int egx_wide_pos_grad(const float* dtok, int B, int S, int off, int T, int d, float* dpos, int pos_stride, float p_drop, uint64_t seed,
                      uint32_t layer, uint32_t site, void* scratch, void* stream) {
    EGX_CHECK(dtok && dpos && scratch, "egx_wide_pos_grad: null pointer");
    EGX_CHECK(B >= 1 && T >= 1 && off >= 0 && off + T <= S && d > 0 && d % 4 == 0 && pos_stride >= d, "egx_wide_pos_grad: B=%d, S=%d, off=%d, T=%d, d=%d, pos_stride=%d",
              B, S, off, T, d, pos_stride);
    EGX_CHECK(al16(dtok) && al16(scratch), "egx_wide_pos_grad: pointers must be 16-byte aligned");
    uint64_t key; uint32_t thresh; float inv;
    if (hook_drop("egx_wide_pos_grad", p_drop, seed, layer, site, &key, &thresh, &inv)) return 1;
    return wide_pos_grad(dtok, B, S, off, T, d, dpos, pos_stride, key, thresh, inv, scratch, (hipStream_t)stream);
}
int egx_wide_cast(int mode, const void* src, int src_bf16, const int* rows, int R, int C, int ld, int pool, void* dst, void* dst_t, void* stream) {
    EGX_CHECK(mode >= 0 && mode <= 2, "egx_wide_cast: mode %d (0 = plain / transposed, 1 = pooled, 2 = gathered)", mode);
    EGX_CHECK(src && (dst || (mode == 0 && dst_t)), "egx_wide_cast: null pointer");
    EGX_CHECK(R >= 0 && C > 0 && al16(src) && al16(dst) && al16(dst_t), "egx_wide_cast: %dx%d, pointers must be 16-byte aligned", R, C);
    hipStream_t st = (hipStream_t)stream;
    if (mode == 0) {
        EGX_CHECK(!src_bf16 && C % 4 == 0 && ld % 4 == 0 && ld >= C && (!dst_t || R % 4 == 0), "egx_wide_cast: %dx%d, ld %d: fp32 source, multiples of 4", R, C, ld);
        return wide_cast((const float*)src, R, C, ld, (bf16_t*)dst, (bf16_t*)dst_t, st);
    }
    EGX_CHECK(C % 8 == 0 && !dst_t, "egx_wide_cast: pooled / gathered need C %% 8 == 0 and have no transposed output");
    if (mode == 1) {
        EGX_CHECK(pool >= 1, "egx_wide_cast: pool %d", pool);
        return wide_pool_cast(src, src_bf16, R, pool, C, (bf16_t*)dst, st);
    }
    EGX_CHECK(rows, "egx_wide_cast: gathered needs the row list");
    return wide_gather_cast(src, src_bf16, rows, R, C, (bf16_t*)dst, st);
}

int egx_encoder_workspace(const egx_config* cfg, const egx_segment* segs, int B, size_t* saved_bytes, size_t* scratch_bytes) {
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return 1;
    size_t wsv = 0, wsc = 0;
    if (wide_ok(cfg, segs, B)) wide_workspace(cfg, segs, B, &wsv, &wsc);
    size_t fsv = 0, fsc = 0;
    fused_workspace(cfg, segs, pl, &fsv, &fsc);
    if (saved_bytes) *saved_bytes = size_max(size_max(pl.saved_bytes, wsv), fsv);
    if (scratch_bytes) *scratch_bytes = size_max(size_max(pl.scratch_bytes, wsc), fsc);
    return 0;
}

static bool token_ce_ok(const egx_config* cfg, const egx_segment* segs, const Plan& pl) {
    bool ferr;
    return use_fused(cfg, segs, pl, &ferr) && fused_token_ce_ok(cfg, pl);
}

size_t egx_weight_cache_bytes(const egx_config* cfg, const egx_segment* segs) {
    if (!cfg || !segs) return 0;
    Plan pl;
    if (make_plan(cfg, segs, 1, pl)) return 0;
    return fused_weight_cache_bytes(cfg, segs, pl);
}

int egx_encoder_token_ce_ok(const egx_config* cfg, const egx_segment* segs, int B) {
    Plan pl;
    if (!cfg || !segs || make_plan(cfg, segs, B, pl)) return 0;
    return token_ce_ok(cfg, segs, pl) ? 1 : 0;
}

int egx_encoder_uses_fused(const egx_config* cfg, const egx_segment* segs, int B) {
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return 0;
    bool ferr;
    return use_fused(cfg, segs, pl, &ferr) ? 1 : 0;
}

int egx_encoder_slices(const egx_config* cfg, const egx_segment* segs, int B) {
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return -1;
    bool ferr;
    return use_fused(cfg, segs, pl, &ferr) ? fused_slices(pl, cfg->compute) : 1;
}

int egx_encoder_impl(const egx_config* cfg, const egx_segment* segs, int B) {
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return -1;
    bool ferr;
    if (use_fused(cfg, segs, pl, &ferr)) return EGX_IMPL_FUSED;
    if (ferr) return -1;
    if (use_tiled(cfg, segs, pl, &ferr)) return EGX_IMPL_TILED;
    if (ferr) return -1;
    if (use_wide(cfg, segs, pl, &ferr)) return EGX_IMPL_WIDE;
    if (ferr) return -1;
    return EGX_IMPL_GENERIC;
}

}  // extern "C"

// wide bf16 path (wide_host.hip) of the forward; with a head, tokens and the pooled vector live behind the wide path's saved block
static int wide_path_fwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, const float* ln_w, const float* ln_b, const egx_layer* layers,
                         const egx_head* head, float* tokens_out, float* logits_out, void* saved, int training, uint64_t seed, hipStream_t st) {
    const int B = pl.B, S = pl.S, d = pl.d, N = (int)pl.N;
    const bool with_head = head && head->W;
    const egx_ce* ce = cfg->ce;
    size_t wsv = 0, wsc = 0;
    wide_workspace(cfg, segs, B, &wsv, &wsc);
    float* tk = tokens_out;
    float* pooled = nullptr;
    if (with_head) {
        float* extra = fptr(saved, align_up(wsv, 256));
        pooled = extra + (size_t)N * d;
        if (!tk) tk = extra;
    }
    if (wide_encoder_fwd(cfg, segs, ln_w, ln_b, layers, B, tk, saved, training, seed, st)) return 1;
    if (with_head) {
        if (pool_head_fwd(tk, B, S, d, head->ln_w, head->ln_b, cfg->ln_eps, head->W, head->b, head->n_out, pooled, logits_out, st)) return 1;
        if (ce) return weighted_ce(logits_out, ce->target, ce->class_weight, B, head->n_out, ce->loss, ce->d_logits, st);
    }
    return 0;
}

// shape-generic path of the forward: one kernel per operation
static int generic_fwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, const float* ln_w, const float* ln_b, const egx_layer* layers,
                       const egx_head* head, float* tokens_out, float* logits_out, void* saved, int training, uint64_t seed, hipStream_t st) {
    const int B = pl.B, S = pl.S, d = pl.d, N = (int)pl.N, comp = cfg->compute;
    const bool with_head = head && head->W;
    const egx_ce* ce = cfg->ce;
    EGX_CHECK(!(cfg->seed_ptr && training && (cfg->p_drop > 0.f || cfg->p_pos > 0.f || cfg->p_feat > 0.f)),
              "device-resident dropout seed (seed_ptr) is only supported by the fused kernels");
    EGX_CHECK(!packed_feats(segs, pl.nseg), "bf16 / frame-pooled features (egx_segment.feat_bf16 / pool) are only supported by the wide bf16 path");

    // generic path with a head: tokens and the pooled vector live behind the layer intermediates in `saved`
    float* head_pooled = nullptr;
    if (with_head) {
        float* tk = fptr(saved, align_up(pl.saved_bytes, 256));
        head_pooled = tk + (size_t)N * d;
        if (!tokens_out) tokens_out = tk;
    }
    float* x0 = pl.L > 0 ? fptr(saved, pl.layer[0].x_in) : tokens_out;
    for (int i = 0; i < pl.nseg; ++i) {
        const egx_segment& sg = segs[i];
        int rows = B * sg.T;
        const float* pre = sg.feat;
        if (sg.proj_w) {
            float* po = fptr(saved, pl.seg_pre[i]);
            Drop df = make_drop(training, cfg->p_feat, seed, (uint32_t)i, SITE_FEAT);
            if (linear_nt(sg.feat, sg.proj_w, sg.proj_b, po, rows, d, sg.d_in, 0, df, nullptr, comp, st)) return 1;
            pre = po;
        }
        LnFwdParams lp;
        lp.x = pre; lp.w = ln_w; lp.b = ln_b; lp.eps = cfg->ln_eps;
        lp.stats = fptr(saved, pl.seg_stats[i]);
        lp.y = x0; lp.rows = rows; lp.d = d;
        lp.T = sg.T; lp.S = S; lp.off = pl.seg_off[i];
        lp.add_vec = sg.add_vec; lp.pos = sg.pos; lp.pos_stride = sg.pos_stride;
        Drop dp = make_drop(training, cfg->p_pos, seed, 0, SITE_POS);
        lp.drop_key = dp.key; lp.drop_thresh = dp.thresh; lp.drop_inv_keep = dp.inv_keep;
        if (layernorm_fwd(lp, st)) return 1;
    }

    for (int l = 0; l < pl.L; ++l) {
        const LayerOff& o = pl.layer[l];
        const egx_layer& w = layers[l];
        const float* x_in = cfptr(saved, o.x_in);
        float* x_out = (l + 1 < pl.L) ? fptr(saved, pl.layer[l + 1].x_in) : tokens_out;
        Drop none;
        if (linear_nt(x_in, w.in_proj_w, w.in_proj_b, fptr(saved, o.qkv), N, 3 * d, d, 0, none, nullptr, comp, st)) return 1;
        Drop da = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_ATTN);
        if (attention_fwd(cfptr(saved, o.qkv), fptr(saved, o.attn_o), fptr(saved, o.lse), B, S, pl.H, d, da.key, da.thresh,
                          da.inv_keep, st)) return 1;
        Drop d1 = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_RES1);
        if (linear_nt(cfptr(saved, o.attn_o), w.out_proj_w, w.out_proj_b, fptr(saved, o.res1), N, d, d, 0, d1, x_in, comp, st)) return 1;
        LnFwdParams l1;
        l1.x = cfptr(saved, o.res1); l1.w = w.norm1_w; l1.b = w.norm1_b; l1.eps = cfg->ln_eps;
        l1.stats = fptr(saved, o.stats1); l1.y = fptr(saved, o.x1); l1.rows = N; l1.d = d;
        if (layernorm_fwd(l1, st)) return 1;
        Drop dh = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_FFN);
        if (linear_nt(cfptr(saved, o.x1), w.lin1_w, w.lin1_b, fptr(saved, o.hid), N, pl.dff, d, 1, dh, nullptr, comp, st)) return 1;
        Drop d2 = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_RES2);
        if (linear_nt(cfptr(saved, o.hid), w.lin2_w, w.lin2_b, fptr(saved, o.res2), N, d, pl.dff, 0, d2, cfptr(saved, o.x1), comp, st)) return 1;
        LnFwdParams l2;
        l2.x = cfptr(saved, o.res2); l2.w = w.norm2_w; l2.b = w.norm2_b; l2.eps = cfg->ln_eps;
        l2.stats = fptr(saved, o.stats2); l2.y = x_out; l2.rows = N; l2.d = d;
        if (layernorm_fwd(l2, st)) return 1;
    }
    if (with_head) {
        if (pool_head_fwd(tokens_out, B, S, d, head->ln_w, head->ln_b, cfg->ln_eps, head->W, head->b, head->n_out,
                          head_pooled, logits_out, st)) return 1;
        if (ce) return weighted_ce(logits_out, ce->target, ce->class_weight, B, head->n_out, ce->loss, ce->d_logits, st);
    }
    return 0;
}

// Shared body of egx_encoder_fwd (head == null) and egx_translator_fwd (pooled head fused or appended).
static int encoder_fwd_impl(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                            const egx_layer* layers, const egx_head* head, int B, float* tokens_out, float* logits_out,
                            void* saved, void* scratch, int training, uint64_t seed, void* stream) {
    (void)scratch;
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return 1;
    EGX_CHECK(saved && ln_w && ln_b, "null pointer argument");
    EGX_CHECK(pl.L == 0 || layers, "null layers");
    hipStream_t st = (hipStream_t)stream;
    const bool with_head = head && head->W;
    EGX_CHECK(with_head ? (logits_out != nullptr) : (tokens_out != nullptr), "null output pointer");
    if (check_ce(cfg->ce, with_head, " (egx_translator_fwd)")) return 1;
    EGX_CHECK(!cfg->weight_cache_valid || cfg->weight_cache, "weight_cache_valid without a weight_cache");
    const egx_token_ce* tce = cfg->token_ce;
    if (tce) {
        EGX_CHECK(!with_head && token_ce_ok(cfg, segs, pl), "egx_config.token_ce: not on this configuration (egx_encoder_token_ce_ok)");
        EGX_CHECK(tce->W && tce->target && tce->logits && tce->loss && tce->d_logits && tce->C >= 1 && tce->C <= 8,
                  "egx_config.token_ce: W, target, logits, loss, d_logits and 1 <= C <= 8 must be set");
    }
    if (check_head(head)) return 1;
    // A HOST seed is baked into a captured graph: every replay would draw the SAME dropout masks — training that runs, converges worse and
    // says nothing. Refused (as the decoder does, wide_decoder.hip refuse_captured_dropout); with egx_config.seed_ptr the seed lives in device
    // memory and is advanced on the stream, so replays draw fresh masks (model.enable_device_seed(), train.GraphedStep).
    if (training && !cfg->seed_ptr && (cfg->p_drop > 0.f || cfg->p_pos > 0.f || cfg->p_feat > 0.f)) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
        EGX_CHECK(cs == hipStreamCaptureStatusNone, "training-mode dropout (p > 0) with a host seed cannot be captured in a hipGraph: every replay would "
                  "repeat the same masks; pass egx_config.seed_ptr (model.enable_device_seed()), capture with p = 0, or launch eagerly");
    }
    bool ferr, terr = false, werr;
    const bool fused = use_fused(cfg, segs, pl, &ferr);
    const bool tiled = !fused && !ferr && use_tiled(cfg, segs, pl, &terr);
    if (fused || tiled) return fused_path_fwd(cfg, segs, pl, tiled, ln_w, ln_b, layers, head, tokens_out, logits_out, saved, training, seed, st);
    if (ferr || terr) return 1;
    EGX_CHECK(cfg->out_tokens == 0 || cfg->out_tokens == pl.S, "out_tokens is implemented by the fused per-clip kernels only (egx_encoder_impl() == EGX_IMPL_FUSED)");
    if (use_wide(cfg, segs, pl, &werr)) return wide_path_fwd(cfg, segs, pl, ln_w, ln_b, layers, head, tokens_out, logits_out, saved, training, seed, st);
    if (werr) return 1;
    return generic_fwd(cfg, segs, pl, ln_w, ln_b, layers, head, tokens_out, logits_out, saved, training, seed, st);
}

// wide bf16 path (wide_host.hip) of the backward
static int wide_path_bwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, const float* ln_w, const egx_layer* layers, const egx_head* head,
                         const float* d_tokens, const float* d_logits, const void* saved, void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w,
                         float* d_ln_b, const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, int training, uint64_t seed, hipStream_t st) {
    const int B = pl.B;
    const bool with_head = head && head->W;
    EGX_CHECK(layers && layer_grads, "null layers / layer_grads");
    if (cfg->bwd_stage == 2) return 0;      // no deferred part
    size_t wsv = 0, wsc = 0;
    wide_workspace(cfg, segs, B, &wsv, &wsc);
    const float* dtok = d_tokens;
    bool zeroed = false;
    if (with_head) {
        const float* extra = cfptr(saved, align_up(wsv, 256));
        const float* pooled = extra + (size_t)pl.N * pl.d;
        float* dt = fptr(scratch, align_up(wsc, 256));
        if (cfg->zero_buf && cfg->zero_bytes) { EGX_HIP(hipMemsetAsync(cfg->zero_buf, 0, cfg->zero_bytes, st)); zeroed = true; }
        if (pool_head_bwd(d_logits, pooled, B, pl.S, pl.d, head->ln_w, head->ln_b, cfg->ln_eps, head->W, head->n_out, dt,
                          head_grads ? head_grads->ln_w : nullptr, head_grads ? head_grads->ln_b : nullptr,
                          head_grads ? head_grads->W : nullptr, head_grads ? head_grads->b : nullptr, st)) return 1;
        dtok = dt;
    }
    egx_config c2 = *cfg;
    if (zeroed) { c2.zero_buf = nullptr; c2.zero_bytes = 0; }
    return wide_encoder_bwd(&c2, segs, ln_w, layers, B, dtok, saved, scratch, seg_grads, d_ln_w, d_ln_b, layer_grads, training, seed, st);
}

// shape-generic path of the backward
static int generic_bwd(const egx_config* cfg, const egx_segment* segs, const Plan& pl, const float* ln_w, const egx_layer* layers, const egx_head* head,
                       float* d_tokens, const float* d_logits, const void* saved, void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w,
                       float* d_ln_b, const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, int training, uint64_t seed, hipStream_t st) {
    const int B = pl.B;
    const bool with_head = head && head->W;
    EGX_CHECK(pl.L == 0 || (layers && layer_grads), "null layers / layer_grads");
    if (cfg->bwd_stage == 2) return 0;      // the generic path has no deferred part
    const int d = pl.d, S = pl.S, comp = cfg->compute, dff = pl.dff;
    const int N = (int)pl.N;
    if (cfg->zero_buf && cfg->zero_bytes) EGX_HIP(hipMemsetAsync(cfg->zero_buf, 0, cfg->zero_bytes, st));
    // deterministic mode: every cross-workgroup sum below goes through partial buffers and fixed-order reductions
    DetScope det_scope(cfg->deterministic ? (char*)scratch + pl.s_det : nullptr, pl.det_bytes);
    if (with_head) {
        const float* tk = cfptr(saved, align_up(pl.saved_bytes, 256));
        const float* pooled = tk + (size_t)N * d;
        d_tokens = fptr(scratch, align_up(pl.scratch_bytes, 256));
        if (pool_head_bwd(d_logits, pooled, B, S, d, head->ln_w, head->ln_b, cfg->ln_eps, head->W, head->n_out, d_tokens,
                          head_grads ? head_grads->ln_w : nullptr, head_grads ? head_grads->ln_b : nullptr,
                          head_grads ? head_grads->W : nullptr, head_grads ? head_grads->b : nullptr, st)) return 1;
    }
    float* dA = fptr(scratch, pl.s_dA);
    float* dBm = fptr(scratch, pl.s_dB);
    float* dqkv = fptr(scratch, pl.s_dqkv);
    float* dhid = fptr(scratch, pl.s_dhid);
    void* slab = (char*)scratch + pl.s_slab;
    float* g = d_tokens;

    for (int l = pl.L - 1; l >= 0; --l) {
        const LayerOff& o = pl.layer[l];
        const egx_layer& w = layers[l];
        const egx_layer_grads& gw = layer_grads[l];
        // LayerNorm2 backward: dA = d(res2)
        LnBwdParams b2;
        b2.dy = g; b2.pre = cfptr(saved, o.res2); b2.stats = cfptr(saved, o.stats2); b2.w = w.norm2_w;
        b2.dx = dA; b2.dw = gw.norm2_w; b2.db = gw.norm2_b; b2.rows = N; b2.d = d;
        if (layernorm_bwd(b2, st)) return 1;
        // dropout2 on the FFN branch
        const float* dbr = dA;
        Drop d2 = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_RES2);
        if (d2.thresh) {
            EGX_HIP(hipMemcpyAsync(dBm, dA, (size_t)N * d * 4, hipMemcpyDeviceToDevice, st));
            if (apply_dropout_mask(dBm, N, d, d2.key, d2.thresh, d2.inv_keep, st)) return 1;
            dbr = dBm;
        }
        if (gw.lin2_b && colsum_accum(dbr, N, d, d, gw.lin2_b, st)) return 1;
        if (gw.lin2_w && linear_dw(dbr, cfptr(saved, o.hid), gw.lin2_w, N, d, dff, comp, slab, pl.slab_bytes, st)) return 1;
        Drop dh = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_FFN);
        if (linear_dx(dbr, w.lin2_w, dhid, N, d, dff, cfptr(saved, o.hid), dh.inv_keep, nullptr, comp, st)) return 1;
        if (gw.lin1_b && colsum_accum(dhid, N, dff, dff, gw.lin1_b, st)) return 1;
        if (gw.lin1_w && linear_dw(dhid, cfptr(saved, o.x1), gw.lin1_w, N, dff, d, comp, slab, pl.slab_bytes, st)) return 1;
        // dx1 = dhid W1 + d(res2)  -> g
        if (linear_dx(dhid, w.lin1_w, g, N, dff, d, nullptr, 1.f, dA, comp, st)) return 1;
        // LayerNorm1 backward: dA = d(res1)
        LnBwdParams b1;
        b1.dy = g; b1.pre = cfptr(saved, o.res1); b1.stats = cfptr(saved, o.stats1); b1.w = w.norm1_w;
        b1.dx = dA; b1.dw = gw.norm1_w; b1.db = gw.norm1_b; b1.rows = N; b1.d = d;
        if (layernorm_bwd(b1, st)) return 1;
        dbr = dA;
        Drop d1 = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_RES1);
        if (d1.thresh) {
            EGX_HIP(hipMemcpyAsync(dBm, dA, (size_t)N * d * 4, hipMemcpyDeviceToDevice, st));
            if (apply_dropout_mask(dBm, N, d, d1.key, d1.thresh, d1.inv_keep, st)) return 1;
            dbr = dBm;
        }
        if (gw.out_proj_b && colsum_accum(dbr, N, d, d, gw.out_proj_b, st)) return 1;
        if (gw.out_proj_w && linear_dw(dbr, cfptr(saved, o.attn_o), gw.out_proj_w, N, d, d, comp, slab, pl.slab_bytes, st)) return 1;
        // d(attn_o) -> g
        if (linear_dx(dbr, w.out_proj_w, g, N, d, d, nullptr, 1.f, nullptr, comp, st)) return 1;
        Drop da = make_drop(training, cfg->p_drop, seed, (uint32_t)l, SITE_ATTN);
        if (attention_bwd(cfptr(saved, o.qkv), cfptr(saved, o.attn_o), cfptr(saved, o.lse), g, dqkv, B, S, pl.H, d, da.key,
                          da.thresh, da.inv_keep, st)) return 1;
        if (gw.in_proj_b && colsum_accum(dqkv, N, 3 * d, 3 * d, gw.in_proj_b, st)) return 1;
        if (gw.in_proj_w && linear_dw(dqkv, cfptr(saved, o.x_in), gw.in_proj_w, N, 3 * d, d, comp, slab, pl.slab_bytes, st)) return 1;
        // dx_in = dqkv Win + d(res1) -> g
        if (linear_dx(dqkv, w.in_proj_w, g, N, 3 * d, d, nullptr, 1.f, dA, comp, st)) return 1;
    }

    // token preparation backward
    Drop dp = make_drop(training, cfg->p_pos, seed, 0, SITE_POS);
    for (int i = 0; i < pl.nseg; ++i) {
        const egx_segment& sg = segs[i];
        egx_segment_grads sgr;
        memset(&sgr, 0, sizeof(sgr));
        if (seg_grads) sgr = seg_grads[i];
        int rows = B * sg.T;
        if (sgr.pos && pos_grad_accum(g, B, S, pl.seg_off[i], sg.T, d, sgr.pos, sg.pos_stride, dp.key, dp.thresh, dp.inv_keep, st)) return 1;
        bool need_dx = (sg.proj_w && (sgr.proj_w || sgr.proj_b || sgr.feat)) || (!sg.proj_w && sgr.feat);
        bool need_any = need_dx || d_ln_w || d_ln_b || sgr.add_vec;
        if (!need_any) continue;
        float* dseg = (!sg.proj_w && sgr.feat) ? sgr.feat : dA;
        LnBwdParams bp;
        bp.dy = g;
        bp.pre = sg.proj_w ? cfptr(saved, pl.seg_pre[i]) : sg.feat;
        bp.stats = cfptr(saved, pl.seg_stats[i]);
        bp.w = ln_w; bp.dx = dseg; bp.dw = d_ln_w; bp.db = d_ln_b; bp.dadd = sgr.add_vec;
        bp.rows = rows; bp.d = d; bp.T = sg.T; bp.S = S; bp.off = pl.seg_off[i];
        bp.drop_key = dp.key; bp.drop_thresh = dp.thresh; bp.drop_inv_keep = dp.inv_keep;
        if (sg.proj_w) {
            Drop df = make_drop(training, cfg->p_feat, seed, (uint32_t)i, SITE_FEAT);
            bp.out_drop_key = df.key; bp.out_drop_thresh = df.thresh; bp.out_drop_inv_keep = df.inv_keep;
        }
        if (layernorm_bwd(bp, st)) return 1;
        if (sg.proj_w) {
            if (sgr.proj_b && colsum_accum(dseg, rows, d, d, sgr.proj_b, st)) return 1;
            if (sgr.proj_w && linear_dw(dseg, sg.feat, sgr.proj_w, rows, d, sg.d_in, comp, slab, pl.slab_bytes, st)) return 1;
            if (sgr.feat && linear_dx(dseg, sg.proj_w, sgr.feat, rows, d, sg.d_in, nullptr, 1.f, nullptr, comp, st)) return 1;
        }
    }
    return 0;
}

static int encoder_bwd_impl(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                            const egx_layer* layers, const egx_head* head, int B, float* d_tokens, const float* d_logits,
                            const void* saved, void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w,
                            float* d_ln_b, const egx_layer_grads* layer_grads, const egx_head_grads* head_grads,
                            int training, uint64_t seed, void* stream) {
    (void)ln_b;
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return 1;
    const bool with_head = head && head->W;
    EGX_CHECK((with_head ? (const void*)d_logits : cfg->token_ce ? (const void*)cfg->token_ce->d_logits : (const void*)d_tokens) && saved && scratch && ln_w, "null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    bool ferr, terr = false, werr;
    const bool fused = use_fused(cfg, segs, pl, &ferr);
    const bool tiled = !fused && !ferr && use_tiled(cfg, segs, pl, &terr);
    if (fused || tiled) return fused_path_bwd(cfg, segs, pl, tiled, ln_w, ln_b, layers, head, d_tokens, d_logits, saved, scratch, seg_grads, d_ln_w, d_ln_b,
                                              layer_grads, head_grads, training, seed, st);
    if (ferr || terr) return 1;
    if (use_wide(cfg, segs, pl, &werr)) return wide_path_bwd(cfg, segs, pl, ln_w, layers, head, d_tokens, d_logits, saved, scratch, seg_grads, d_ln_w, d_ln_b,
                                                             layer_grads, head_grads, training, seed, st);
    if (werr) return 1;
    return generic_bwd(cfg, segs, pl, ln_w, layers, head, d_tokens, d_logits, saved, scratch, seg_grads, d_ln_w, d_ln_b, layer_grads, head_grads, training, seed, st);
}

extern "C" {

int egx_encoder_fwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                    const egx_layer* layers, int B, float* tokens_out, void* saved, void* scratch, int training,
                    uint64_t seed, void* stream) {
    return encoder_fwd_impl(cfg, segs, ln_w, ln_b, layers, nullptr, B, tokens_out, nullptr, saved, scratch, training, seed, stream);
}

int egx_encoder_bwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                    const egx_layer* layers, int B, float* d_tokens, const void* saved, void* scratch,
                    const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b,
                    const egx_layer_grads* layer_grads, int training, uint64_t seed, void* stream) {
    return encoder_bwd_impl(cfg, segs, ln_w, ln_b, layers, nullptr, B, d_tokens, nullptr, saved, scratch, seg_grads, d_ln_w,
                            d_ln_b, layer_grads, nullptr, training, seed, stream);
}

int egx_translator_workspace(const egx_config* cfg, const egx_segment* segs, int B, size_t* saved_bytes, size_t* scratch_bytes) {
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return 1;
    size_t sv = 0, sc = 0;
    if (egx_encoder_workspace(cfg, segs, B, &sv, &sc)) return 1;
    // generic path extras: tokens + pooled behind `saved`, d_tokens behind `scratch`
    size_t wsv = 0, wsc = 0;
    if (wide_ok(cfg, segs, B)) wide_workspace(cfg, segs, B, &wsv, &wsc);
    size_t extra_sv = align_up(size_max(pl.saved_bytes, wsv), 256) + (pl.N + (size_t)B) * pl.d * 4 + 256;
    size_t extra_sc = align_up(size_max(pl.scratch_bytes, wsc), 256) + pl.N * pl.d * 4 + 256;
    if (saved_bytes) *saved_bytes = size_max(sv, extra_sv);
    if (scratch_bytes) *scratch_bytes = size_max(sc, extra_sc);
    return 0;
}

int egx_translator_fwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                       const egx_layer* layers, const egx_head* head, int B, float* logits_out, float* tokens_out,
                       void* saved, void* scratch, int training, uint64_t seed, void* stream) {
    EGX_CHECK(head && head->W, "egx_translator_fwd needs a head (use egx_encoder_fwd otherwise)");
    return encoder_fwd_impl(cfg, segs, ln_w, ln_b, layers, head, B, tokens_out, logits_out, saved, scratch, training, seed, stream);
}

int egx_translator_bwd(const egx_config* cfg, const egx_segment* segs, const float* ln_w, const float* ln_b,
                       const egx_layer* layers, const egx_head* head, int B, const float* d_logits, const void* saved,
                       void* scratch, const egx_segment_grads* seg_grads, float* d_ln_w, float* d_ln_b,
                       const egx_layer_grads* layer_grads, const egx_head_grads* head_grads, int training,
                       uint64_t seed, void* stream) {
    EGX_CHECK(head && head->W, "egx_translator_bwd needs a head (use egx_encoder_bwd otherwise)");
    return encoder_bwd_impl(cfg, segs, ln_w, ln_b, layers, head, B, nullptr, d_logits, saved, scratch, seg_grads, d_ln_w,
                            d_ln_b, layer_grads, head_grads, training, seed, stream);
}

int egx_pool_head_fwd(const float* tokens, int B, int S, int d, const float* ln_w, const float* ln_b, float ln_eps,
                      const float* W, const float* b, int n_out, float* pooled_saved, float* out, void* stream) {
    EGX_CHECK(tokens && pooled_saved && out, "null pointer argument");
    return pool_head_fwd(tokens, B, S, d, ln_w, ln_b, ln_eps, W, b, n_out, pooled_saved, out, (hipStream_t)stream);
}

int egx_pool_head_bwd(const float* d_out, const float* pooled_saved, int B, int S, int d, const float* ln_w,
                      const float* ln_b, float ln_eps, const float* W, int n_out, float* d_tokens, float* d_ln_w,
                      float* d_ln_b, float* d_W, float* d_b, void* stream) {
    EGX_CHECK(d_out && pooled_saved && d_tokens, "null pointer argument");
    return pool_head_bwd(d_out, pooled_saved, B, S, d, ln_w, ln_b, ln_eps, W, n_out, d_tokens, d_ln_w, d_ln_b, d_W, d_b,
                         (hipStream_t)stream);
}

int egx_linear_fwd(const float* x, const float* W, const float* b, float* y, int M, int N, int K, int relu, int compute,
                   void* stream) {
    EGX_CHECK(x && W && y, "null pointer argument");
    Drop none;
    return linear_nt(x, W, b, y, M, N, K, relu, none, nullptr, compute, (hipStream_t)stream);
}
int egx_linear_residual_fwd(const float* x, const float* W, const float* b, const float* residual, float* y, int M, int N, int K,
                            int compute, void* stream) {
    EGX_CHECK(x && W && y && residual, "null pointer argument");
    Drop none;
    return linear_nt(x, W, b, y, M, N, K, 0, none, residual, compute, (hipStream_t)stream);
}
int egx_gelu_fwd(const float* z, float* h, size_t n, void* stream) { return gelu_fwd(z, h, n, (hipStream_t)stream); }
int egx_gelu_bwd(const float* z, const float* dh, float* dz, size_t n, void* stream) { return gelu_bwd(z, dh, dz, n, (hipStream_t)stream); }

// db[N] += colsum(dy[M, N]) with the row blocks' partial sums added in block order through `scratch` (no atomics between row blocks):
// the same bits on every run. egx_linear_bwd's own column sum meets in atomicAdd; callers that need repeatable bias gradients (the
// composed EgoT2-g decoder) pass db = NULL there and call this.
size_t egx_colsum_ordered_scratch(int M, int N) { return colsum_part_bytes(M, N); }
int egx_colsum_ordered(const float* dy, int M, int N, float* db, void* scratch, size_t scratch_bytes, void* stream) {
    EGX_CHECK(dy && db, "egx_colsum_ordered: null pointer argument");
    EGX_CHECK(scratch_bytes >= colsum_part_bytes(M, N) && (scratch || !colsum_part_bytes(M, N)),
              "egx_colsum_ordered: scratch of %zu bytes, egx_colsum_ordered_scratch(%d, %d) = %zu", scratch_bytes, M, N, colsum_part_bytes(M, N));
    return colsum_accum_ordered(dy, M, N, N, db, scratch, scratch_bytes, (hipStream_t)stream);
}

size_t egx_linear_bwd_scratch(int M, int N, int K) { return size_max(gemm_scratch_bytes(2, N, K, M), gemm_scratch_bytes(1, M, K, N)); }

int egx_linear_bwd(const float* dy, const float* x, const float* W, float* dx, float* dW, float* db, int M, int N, int K,
                   int compute, void* scratch, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    EGX_CHECK(dy, "null dy");
    if (db && colsum_accum(dy, M, N, N, db, st)) return 1;
    if (dW) {
        EGX_CHECK(x && scratch, "linear_bwd: dW needs x and scratch");
        if (linear_dw(dy, x, dW, M, N, K, compute, scratch, gemm_scratch_bytes(2, N, K, M), st)) return 1;
    }
    if (dx) {
        EGX_CHECK(W, "linear_bwd: dx needs W");
        if (linear_dx(dy, W, dx, M, N, K, nullptr, 1.f, nullptr, compute, st, scratch, scratch ? egx_linear_bwd_scratch(M, N, K) : 0)) return 1;
    }
    return 0;
}

int egx_gemm(int layout, const float* A, const float* Bm, float* C, int M, int N, int K, const float* bias, int relu,
             int compute, void* scratch, size_t scratch_bytes, void* stream) {
    EGX_CHECK(A && Bm && C, "null pointer argument");
    GemmParams g;
    g.A = A; g.B = Bm; g.C = C; g.M = M; g.N = N; g.K = K;
    g.lda = (layout == 2) ? M : K;
    g.ldb = (layout == 0) ? K : N;
    g.ldc = N;
    g.bias = bias; g.relu = relu;
    return gemm(layout, g, compute, 0, scratch, scratch_bytes, (hipStream_t)stream);
}

int egx_layernorm_fwd(const float* x, const float* res, const float* w, const float* b, float eps, float* pre,
                      float* stats, float* y, int rows, int d, void* stream) {
    EGX_CHECK(x && w && b && y, "null pointer argument");
    LnFwdParams p;
    p.x = x; p.res = res; p.w = w; p.b = b; p.eps = eps; p.pre = pre; p.stats = stats; p.y = y; p.rows = rows; p.d = d;
    return layernorm_fwd(p, (hipStream_t)stream);
}

int egx_layernorm_bwd(const float* dy, const float* pre, const float* stats, const float* w, float* dx, float* dw,
                      float* db, int rows, int d, void* stream) {
    EGX_CHECK(dy && pre && stats && w && dx, "null pointer argument");
    LnBwdParams p;
    p.dy = dy; p.pre = pre; p.stats = stats; p.w = w; p.dx = dx; p.dw = dw; p.db = db; p.rows = rows; p.d = d;
    return layernorm_bwd(p, (hipStream_t)stream);
}

int egx_attention_fwd(const float* qkv, float* out, float* lse, int B, int S, int H, int d, float p_drop, uint64_t seed,
                      void* stream) {
    EGX_CHECK(qkv && out && lse, "null pointer argument");
    Drop da = make_drop(p_drop > 0.f, p_drop, seed, 0, SITE_ATTN);
    return attention_fwd(qkv, out, lse, B, S, H, d, da.key, da.thresh, da.inv_keep, (hipStream_t)stream);
}

int egx_attention_bwd(const float* qkv, const float* out, const float* lse, const float* d_out, float* d_qkv, int B,
                      int S, int H, int d, float p_drop, uint64_t seed, void* stream) {
    EGX_CHECK(qkv && out && lse && d_out && d_qkv, "null pointer argument");
    Drop da = make_drop(p_drop > 0.f, p_drop, seed, 0, SITE_ATTN);
    return attention_bwd(qkv, out, lse, d_out, d_qkv, B, S, H, d, da.key, da.thresh, da.inv_keep, (hipStream_t)stream);
}

int egx_weighted_ce(const float* logits, const int64_t* target, const float* weight, int B, int C, float* loss,
                    float* d_logits, void* stream) {
    return weighted_ce(logits, target, weight, B, C, loss, d_logits, (hipStream_t)stream);
}

size_t egx_linear_ce_scratch(int M, int K, int C) { return linear_ce_scratch_bytes(M, K, C); }
int egx_linear_ce_fwd(const float* x, const float* W, const float* b, const int64_t* target, const float* weight, int M, int K,
                      int C, float* logits, float* probs, float* d_logits, float* loss, float* correct, float* pred_label,
                      void* scratch, void* stream) {
    return linear_ce_fwd(x, W, b, target, weight, M, K, C, logits, probs, d_logits, loss, correct, pred_label, scratch, (hipStream_t)stream);
}
int egx_linear_ce_bwd(const float* x, const float* W, const float* d_logits, const float* grad_scale, int M, int K, int C,
                      float* dx, float* dW, float* db, void* scratch, void* stream) {
    return linear_ce_bwd(x, W, d_logits, grad_scale, M, K, C, dx, dW, db, scratch, (hipStream_t)stream);
}

int egx_counter_add(int64_t* counter, int64_t inc, void* stream) { return counter_add(counter, inc, (hipStream_t)stream); }

int egx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const int64_t* step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                  void* stream) {
    EGX_CHECK(lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "adam_step: invalid hyper-parameters");
    return adam_step(param, grad, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale,
                     (hipStream_t)stream);
}

// ABI v18, additions: the arguments are checked on the host (train.hip lr_update / sgd_step), before any device work
int egx_lr_update(const egx_lr_schedule* schedule, int64_t* step, const double* base_lr, int n_groups, float* lr_out, void* stream) {
    EGX_CHECK(schedule, "lr_update: null schedule");
    return lr_update(schedule->kind, schedule->warmup_steps, schedule->t_total, schedule->T_max, schedule->cycles, schedule->factors,
                     schedule->n, step, base_lr, n_groups, lr_out, (hipStream_t)stream);
}

int egx_adam_step_dev_lr(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const int64_t* step,
                         const float* lr, float beta1, float beta2, float eps, float weight_decay, int decoupled, float grad_scale,
                         void* stream) {
    EGX_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f, "adam_step_dev_lr: invalid hyper-parameters (needs 0 <= beta < 1, eps >= 0)");
    return adam_step_dev_lr(param, grad, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay, decoupled, grad_scale,
                            (hipStream_t)stream);
}

int egx_sgd_step(float* param, const float* grad, float* momentum_buf, size_t n, const int64_t* step, const float* lr_dev, float lr,
                 float momentum, float dampening, float weight_decay, int nesterov, float grad_scale, void* stream) {
    return sgd_step(param, grad, momentum_buf, n, step, lr_dev, lr, momentum, dampening, weight_decay, nesterov, grad_scale,
                    (hipStream_t)stream);
}

// ABI v18, additions: the LTA criterion (seg_ce.hip); every argument is checked on the host before any device work
size_t egx_segmented_ce_scratch(int B, int Z, int H, int n_ks) { return segmented_ce_scratch_bytes(B, Z, H, n_ks); }
int egx_segmented_ce(const float* logits, int ld, const int64_t* target, int B, int Z, int H, const int* col0, const int* C, const int* ks,
                     int n_ks, float* loss, float* loss_terms, int* n_valid, int* correct, float* d_logits, void* scratch, void* stream) {
    return segmented_ce(logits, ld, target, B, Z, H, col0, C, ks, n_ks, loss, loss_terms, n_valid, correct, d_logits, scratch,
                        (hipStream_t)stream);
}

// ABI v19 addition: the LTA validation step (lta_val.hip); every argument is checked on the host before any device work
int egx_lta_validate(const float* logits, int ld, const int64_t* labels, int B, int Z, int H, const int* col0, const int* C, int K,
                     uint64_t seed, const uint64_t* seed_ptr, const int64_t* preds_in, int64_t* preds, int* min_dist, int64_t* dist_sum,
                     void* stream) {
    return lta_validate(logits, ld, labels, B, Z, H, col0, C, K, seed, seed_ptr, preds_in, preds, min_dist, dist_sum, (hipStream_t)stream);
}

// ABI v20 additions: the PNR keyframe criterion and metrics (keyframe.hip); every argument is checked on the host before any device work
size_t egx_keyframe_scratch(int B) { return keyframe_scratch_bytes(B); }
int egx_keyframe_criterion(const float* logits, int ld, int B, int T, const int* cols, int V, int kind, const float* target,
                           const int64_t* label, const int64_t* state_change, const double* fps, const int64_t* clip_start,
                           const int64_t* clip_end, const int64_t* pnr_frame, float* loss, float* loss_rows, float* d_logits, int* pred,
                           int* label_frame, int* counts, double* dist, double* dist_sum, void* scratch, void* stream) {
    return keyframe_criterion(logits, ld, B, T, cols, V, kind, target, label, state_change, fps, clip_start, clip_end, pnr_frame, loss,
                              loss_rows, d_logits, pred, label_frame, counts, dist, dist_sum, scratch, (hipStream_t)stream);
}

// ABI v21 additions: the EgoT2-g multi-task sequence criterion and metrics (seq_ce.hip); every argument is checked on the host before any
// device work
static_assert(sizeof(egx_seq_task) == 112, "egx_seq_task: the layout the bindings declare");
size_t egx_sequence_ce_scratch(void) { return sequence_ce_scratch_bytes(); }
int egx_sequence_ce(const egx_seq_task* tasks, int T, int V, void* result, void* scratch, void* stream) {
    SeqCeTask k[SEQ_CE_MAX_TASKS];
    for (int t = 0; tasks && t < T && t < SEQ_CE_MAX_TASKS; ++t) {
        const egx_seq_task& a = tasks[t];
        k[t] = SeqCeTask{a.logits, a.stride_b, a.stride_s, a.B, a.sy, a.target, a.target_stride_b, a.target_stride_s, a.ratio, a.d_logits,
                         a.word_label, a.labels, a.labels_stride_b, a.labels_stride_s, a.pred};
    }
    return sequence_ce(tasks ? k : nullptr, T, V, (int*)result, scratch, (hipStream_t)stream);
}

// ABI v22 additions: the TTM / LAM validation accumulator and metric (segment_ap.hip); every argument is checked on the host before any
// device work
size_t egx_segment_ap_scratch(int capacity) { return segment_ap_scratch_bytes(capacity); }
int egx_segment_scores_update(const float* logits, int ld, int B, const int64_t* slots, int slot0, const int64_t* labels, int capacity,
                              void* scratch, void* stream) {
    return segment_scores_update(logits, ld, B, slots, slot0, labels, capacity, scratch, (hipStream_t)stream);
}
int egx_segment_ap(int N, int capacity, void* scratch, float* score, int* order1, int* order0, void* result, void* stream) {
    return segment_ap(N, capacity, scratch, score, order1, order0, result, (hipStream_t)stream);
}

// ABI v23 additions: the multi-view ensemble of the action-recognition test epoch and its top-k errors (view_ensemble.hip); every argument
// is checked on the host before any device work
size_t egx_view_ensemble_state(int capacity, int H, const int* C, size_t* offsets) { return view_ensemble_state_bytes(capacity, H, C, offsets); }
int egx_view_ensemble_update(const float* preds, int ld, int B, int H, const int* col0, const int* C, const int64_t* labels, const void* slots,
                             int slot_bytes, int slot0, int method, int capacity, void* state, void* stream) {
    return view_ensemble_update(preds, ld, B, H, col0, C, labels, slots, slot_bytes, slot0, method, capacity, state, (hipStream_t)stream);
}
int egx_view_ensemble_topk(int n, int capacity, int H, const int* C, const int* ks, int n_ks, void* state, int* rank, int* pred, void* result,
                           void* stream) {
    return view_ensemble_topk(n, capacity, H, C, ks, n_ks, state, rank, pred, (int*)result, (hipStream_t)stream);
}

// ---- EgoT2-g sequence decoder pieces (decoder.hip) ---------------------------------------------------------------
static SmallAttnParams small_attn_params(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int B, int Sq,
                                         int Sk, int H, int dh, int causal, float p_drop, uint64_t seed, uint32_t site) {
    SmallAttnParams p;
    memset(&p, 0, sizeof(p));
    p.q = q; p.k = k; p.v = v; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv;
    p.B = B; p.Sq = Sq; p.Sk = Sk; p.H = H; p.dh = dh; p.causal = causal;
    Drop dr = make_drop(p_drop > 0.f, p_drop, seed, site >> 8, site & 0xffu);
    p.drop_key = dr.key; p.drop_thresh = dr.thresh; p.drop_inv = dr.inv_keep;
    return p;
}

int egx_small_attention_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, int B,
                            int Sq, int Sk, int H, int dh, int causal, float p_drop, uint64_t seed, uint32_t site, void* stream) {
    SmallAttnParams p = small_attn_params(q, ldq, k, ldk, v, ldv, B, Sq, Sk, H, dh, causal, p_drop, seed, site);
    p.o = o; p.ldo = ldo;
    return small_attention_fwd(p, (hipStream_t)stream);
}

int egx_small_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* d_o, int ldo,
                            float* dq, float* dk, float* dv, int B, int Sq, int Sk, int H, int dh, int causal, float p_drop,
                            uint64_t seed, uint32_t site, void* stream) {
    SmallAttnParams p = small_attn_params(q, ldq, k, ldk, v, ldv, B, Sq, Sk, H, dh, causal, p_drop, seed, site);
    p.d_o = d_o; p.ldo = ldo; p.dq = dq; p.dk = dk; p.dv = dv;
    return small_attention_bwd(p, (hipStream_t)stream);
}

int egx_embed_pos_fwd(const int64_t* tokens, const float* emb, const float* pe, int pe_stride, float scale, float* out, int B,
                      int sy, int d, int V, float p_drop, uint64_t seed, void* stream) {
    Drop dr = make_drop(p_drop > 0.f, p_drop, seed, 0xDECu, SITE_POS);
    return embed_pos_fwd(tokens, emb, pe, pe_stride, scale, out, B, sy, d, V, dr.key, dr.thresh, dr.inv_keep, (hipStream_t)stream);
}

int egx_embed_pos_bwd(const int64_t* tokens, const float* dy, float* d_emb, float scale, int B, int sy, int d, int V, float p_drop,
                      uint64_t seed, void* stream) {
    Drop dr = make_drop(p_drop > 0.f, p_drop, seed, 0xDECu, SITE_POS);
    return embed_pos_bwd(tokens, dy, d_emb, scale, B, sy, d, V, dr.key, dr.thresh, dr.inv_keep, (hipStream_t)stream);
}

int egx_relu_mask(float* dy, const float* y, size_t n, void* stream) { return relu_mask(dy, y, n, (hipStream_t)stream); }

int egx_dropout(float* x, int rows, int cols, float p_drop, uint64_t seed, uint32_t site, void* stream) {
    EGX_CHECK(x || rows * cols == 0, "egx_dropout: null pointer");
    Drop dr = make_drop(p_drop > 0.f, p_drop, seed, site >> 8, site & 0xffu);
    return apply_dropout_mask(x, rows, cols, dr.key, dr.thresh, dr.inv_keep, (hipStream_t)stream);
}

}  // extern "C"

// ---- ABI v27: the encoder's self-attention weights from the Q | K | V rows a forward left in `saved` (enc_attn_weights.hip) ----------------
extern "C" {

int egx_encoder_self_weights(const egx_config* cfg, const egx_segment* segs, int B, const int* lengths, int head_n_out, const void* saved,
                             uint64_t layer_mask, float* w_out, float* seg_out, void* stream) {
    const char* who = "egx_encoder_self_weights";
    EGX_CHECK(cfg && segs, "%s: null config / segments", who);
    EGX_CHECK(saved, "%s: null pointer argument (saved)", who);
    EGX_CHECK(w_out || seg_out, "%s: null pointer argument (w_out and seg_out are both null)", who);
    EGX_CHECK(head_n_out >= 0, "%s: head_n_out = %d", who, head_n_out);
    EGX_CHECK(cfg->p_drop == 0.f && cfg->p_pos == 0.f && cfg->p_feat == 0.f,
              "%s: inference only: p_drop, p_pos and p_feat must be 0 (got %g, %g, %g); the weights behind the attention dropout are not modelled",
              who, cfg->p_drop, cfg->p_pos, cfg->p_feat);
    Plan pl;
    if (make_plan(cfg, segs, B, pl)) return 1;
    EGX_CHECK(pl.L >= 1, "%s: a configuration without encoder layers keeps no Q | K | V", who);
    EGX_CHECK(layer_mask != 0 && (pl.L >= 64 || (layer_mask >> pl.L) == 0), "%s: layer_mask = 0x%llx selects no layer or one beyond the %d layers",
              who, (unsigned long long)layer_mask, pl.L);
    const int dh = pl.d / pl.H;
    EGX_CHECK(dh == 16 || dh == 32 || dh == 64 || dh == 96 || dh == 128,
              "%s: head dim %d (16, 32, 64, 96 or 128; the head dims 256 / 512 of the d = 2048 recipe are not served)", who, dh);
    EGX_CHECK(pl.nseg <= SW_MAXSEG, "%s: %d segments (at most %d)", who, pl.nseg, SW_MAXSEG);
    hipStream_t st = (hipStream_t)stream;
    if (lengths) {
        EGX_CHECK(pl.d == 128, "%s: ragged batches are served on the d = 128 kernels only (egx_ragged_train_fwd with training = 0); the wide path's "
                  "ragged batches (egx_ragged_encode*) are not", who);
        return ragged_self_weights(cfg, segs, B, lengths, saved, layer_mask, w_out, seg_out, st);
    }
    EGX_CHECK(pl.S <= SW_MAXS, "%s: S = %d (1..%d)", who, pl.S, SW_MAXS);
    const int impl = egx_encoder_impl(cfg, segs, B);
    if (impl < 0) return 1;
    if (impl == EGX_IMPL_FUSED || impl == EGX_IMPL_TILED) return fused_self_weights(cfg, segs, pl, impl == EGX_IMPL_TILED, saved, layer_mask, w_out, seg_out, st);
    SelfWParams p;
    memset(&p, 0, sizeof(p));
    p.ldq = p.ldk = 3 * pl.d; p.clip_rows = pl.S; p.K = pl.nseg; p.w = w_out; p.ldw = pl.S; p.seg = seg_out; p.B = B; p.H = pl.H; p.S = pl.S;
    p.fixed_segs = 1;
    for (int i = 0; i < pl.nseg; ++i) p.seg_fixed[i] = segs[i].T;
    if (impl == EGX_IMPL_WIDE) {
        size_t off[64];
        wide_qkv_offsets(cfg, segs, B, off);
        // (the wide plan's layers are laid out at one stride; checked, not assumed)
        const size_t stride = pl.L > 1 ? off[1] - off[0] : 0;
        for (int l = 1; l < pl.L; ++l) EGX_CHECK(off[l] == off[0] + l * stride, "%s: wide plan: layer %d not at the common stride", who, l);
        return self_weights_layers(p, (const char*)saved + off[0], stride, pl.d, pl.L, layer_mask, false, st);
    }
    const size_t stride = pl.L > 1 ? pl.layer[1].qkv - pl.layer[0].qkv : 0;
    return self_weights_layers(p, (const char*)saved + pl.layer[0].qkv, stride, pl.d, pl.L, layer_mask, true, st);
}

}  // extern "C"
