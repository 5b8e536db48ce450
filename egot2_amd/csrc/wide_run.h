// The launch kit of the wide bf16 host drivers: wide_host.hip (the encoder) and wide_decoder.hip (the decoder and its cached step).
// What a driver does with it:
//   plan      lays `saved` / `scratch` / `ws` out (make_wplan, make_dplan, step_layout) and sizes the regions of a backward's deferred
//             reductions with wide_slab_bytes() / wide_rowpart_bytes();
//   context   builds ONE WideRun per forward or backward call: the base pointers, the stream, the zero page, the LayerNorm epsilon and all
//             that dropout needs (training, host seed, device key table, layer base of the keys). Its members fill the launch parameters:
//             drop(), nt() / nt_on() / nt_bwd(), ln(), ln_bwd(). A backward hangs a WideLedger over the plan's regions on it;
//   sublayers runs wide_proj_ln_fwd / _bwd ("projection + dropout + residual -> LayerNorm") and wide_ffn_fwd / _bwd (the post-LN FFN)
//             over small structs of buffer pointers, between the launches only it has (token preparation, attention, fp32 layer 0);
//   flush     WideLedger::flush(): every queued row sum, every queued weight gradient and every slab sum, one launch each.
// Nothing here owns memory or state between calls, and nothing is virtual or type-erased: a launch costs what filling its struct costs.
#pragma once
#include <initializer_list>

#include "common.h"
#include "kernels.h"
#include "wide.h"

namespace egx {

template <class T> T* at(void* base, size_t off) { return reinterpret_cast<T*>((char*)base + off); }
template <class T> const T* cat(const void* base, size_t off) { return reinterpret_cast<const T*>((const char*)base + off); }

struct WideDrop { uint64_t key = 0; uint32_t thresh = 0; float inv = 1.f; };

// ---- deferred reductions of a backward -------------------------------------------------------------------------------------------------
// Sizing: one slab region per weight gradient, whose split-K sums run as ONE launch at the end ...
struct WideTnShape { int M, N; size_t K; };     // dW (M, N) over K token rows
inline size_t wide_slab_bytes(std::initializer_list<WideTnShape> products) {
    size_t all = 0;
    for (const WideTnShape& p : products) all += align_up(wide_gemm_tn_scratch(p.M, p.N, (int)p.K), 256);
    return all;
}
// ... and one partial buffer per deferred row reduction (wide.h WideRowReduceBatch): per layer n_ln LayerNorm backwards over `rows` rows
// and one column sum of each listed size
inline size_t wide_rowpart_bytes(int L, int n_ln, int rows, int d, std::initializer_list<size_t> colsums) {
    size_t per = (size_t)n_ln * align_up(wide_ln_bwd_scratch(rows, d), 256);
    for (size_t c : colsums) per += align_up(c, 256);
    return (size_t)L * per;
}
inline size_t wide_ffn_colsum_bytes(int rows, int dff) { return (size_t)(4 * cdiv(rows, 256) + 4) * dff * 4; }      // lin1's bias sums

// The bookkeeping of one backward. The encoder and the decoder differ in four ways, all of them members:
//   fallback    shared_slab given (encoder): a gradient that finds no region (slab_bytes 0: nothing is deferred) takes the shared slab and
//               is reduced right behind its GEMM; null (decoder): it is refused;
//   accumulate  fresh / fresh_bytes (decoder): a target inside the buffer the call has just zero-filled is overwritten, not added to;
//   issue path  a weight gradient runs on tn_stream (the decoder's side stream) or, grouped, is queued for one launch per tile variant;
//   sizing      the callers' regions come from wide_slab_bytes / wide_rowpart_bytes above (the encoder's cut-offs: make_wplan).
struct WideLedger {
    WideReduceBatch rb; WideRowReduceBatch rrb; WideTnQueue tq;
    hipStream_t st = nullptr, tn_stream = nullptr;
    const void* zero = nullptr;
    char* slab = nullptr; size_t slab_bytes = 0, slab_cur = 0;
    char* rows = nullptr; size_t rows_bytes = 0, rows_cur = 0;      // (0 bytes: every row reduction runs at once on the shared buffers)
    void* lnpart = nullptr; float* cspart = nullptr;                // the shared partial buffers
    void* shared_slab = nullptr;
    const char* fresh = nullptr; size_t fresh_bytes = 0;
    bool grouped = false;

    // a partial buffer of its own for a row reduction that is then QUEUED (null: none left)
    void* row_region(size_t need) {
        need = align_up(need, 256);
        if (!rows_bytes || rows_cur + need > rows_bytes) return nullptr;
        void* r = rows + rows_cur;
        rows_cur += need;
        return r;
    }
    // out[c] += the column sums of the bf16 rows x (rows, cols), on stream s; `shared`: the partial buffer when no region is left
    int colsum(const bf16_t* x, int nrows, int cols, float* out, void* shared, hipStream_t s) {
        void* reg = row_region(wide_colsum_scratch(nrows, cols));
        return wide_colsum_bf16(x, nrows, cols, cols, out, reg ? reg : shared, s, reg ? &rrb : nullptr);
    }
    // dW (n_out, k_in) (+)= dy^T x over `tokens` rows; dW null: nothing
    int dw_tn(const bf16_t* dy, const bf16_t* x, float* dW, int n_out, int k_in, int tokens) {
        if (!dW) return 0;
        WideGemmParams t;
        t.A = dy; t.B = x; t.M = n_out; t.N = k_in; t.K = tokens; t.lda = n_out; t.ldb = k_in; t.Cf = dW; t.ldc = k_in; t.zero_page = zero;
        // a target inside the freshly zero-filled buffer is overwritten (saves the read of the +=), anything else keeps the += contract
        // of the header
        const bool zeroed = fresh && (const char*)dW >= fresh && (const char*)(dW + (size_t)n_out * k_in) <= fresh + fresh_bytes;
        t.accumulate = zeroed ? 0 : 1;
        const size_t need = align_up(wide_gemm_tn_scratch(n_out, k_in, tokens), 256);
        if (!slab_bytes || slab_cur + need > slab_bytes) {
            EGX_CHECK(shared_slab, "decoder backward: slab region exhausted");
            return wide_gemm_tn(t, shared_slab, tn_stream);
        }
        void* region = slab + slab_cur;
        slab_cur += need;
        return grouped ? wide_tn_queue_add(tq, t, region, st, &rb) : wide_gemm_tn(t, region, tn_stream, &rb);
    }
    // every queued LayerNorm / bias column sum; every queued weight gradient (one grid per tile variant); then all slab sums
    int flush() {
        if (wide_row_reduce_flush(rrb, st)) return 1;
        if (wide_tn_queue_flush(tq, st)) return 1;
        return wide_reduce_flush(rb, st);
    }
};

// ---- the context of one forward or backward call ------------------------------------------------------------------------------------------
struct WideRun {
    char* saved = nullptr; char* scratch = nullptr;     // (a cached step: its one workspace as `saved`)
    hipStream_t st = nullptr;
    const void* zero = nullptr;
    float ln_eps = 1e-5f, p_drop = 0.f;                 // p_drop: the sublayers' dropout
    int training = 0; uint64_t seed = 0;
    const uint64_t* keys = nullptr;                     // device-resident seed: the table derive_keys() filled on the stream, else null
    uint32_t layer_base = 0;                            // of the host keys: 0 the encoder, 0x40 the decoder (the table is relative to it)
    WideLedger* led = nullptr;                          // a backward's

    template <class T> T* sv(size_t off) const { return reinterpret_cast<T*>(saved + off); }
    template <class T> T* sc(size_t off) const { return reinterpret_cast<T*>(scratch + off); }

    // with a key table the key is the ADDRESS of its slot (resolve_key, common.h)
    WideDrop drop(float p, uint32_t layer, uint32_t site) const {
        WideDrop dr;
        if (training && p > 0.f) {
            dr.key = keys ? key_slot(keys, layer, site) : site_key(seed, layer_base + layer, site);
            dr.thresh = drop_threshold(p); dr.inv = p < 1.f ? 1.f / (1.f - p) : 0.f;
        }
        return dr;
    }
    // forward NT GEMM: C (M, N) = dropout(relu(A (M, K) W (N, K)^T + bias)) + residual, fp32 (Cf) or bf16 (Cb) rows
    int nt_on(hipStream_t s, const bf16_t* A, const bf16_t* W, int M, int N, int K, const float* bias, float* Cf, bf16_t* Cb, int relu,
              const WideDrop& dr, const float* residual) const {
        WideGemmParams g;
        g.A = A; g.B = W; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.Cf = Cf; g.Cb = Cb; g.ldc = N; g.bias = bias; g.relu = relu;
        g.drop_key = dr.key; g.drop_thresh = dr.thresh; g.drop_inv = dr.inv; g.residual = residual; g.ldr = N; g.zero_page = zero;
        return wide_gemm_nt(g, s);
    }
    int nt(const bf16_t* A, const bf16_t* W, int M, int N, int K, const float* bias, float* Cf, bf16_t* Cb, int relu, const WideDrop& dr,
           const float* residual) const { return nt_on(st, A, W, M, N, K, bias, Cf, Cb, relu, dr, residual); }
    // backward NT GEMM: C (M, N) = (A (M, K) Wt (N, K)^T) .* (mask != 0) * mask_scale + residual; colsum: per-tile column sums of C
    int nt_bwd(const bf16_t* A, const bf16_t* Wt, int M, int N, int K, float* Cf, bf16_t* Cb, const float* residual, const bf16_t* mask = nullptr,
               float mask_scale = 1.f, float* colsum = nullptr) const {
        WideGemmParams g;
        g.A = A; g.B = Wt; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.Cf = Cf; g.Cb = Cb; g.ldc = N;
        g.residual = residual; g.ldr = N; g.mask = mask; g.ldm = N; g.mask_scale = mask_scale; g.colsum = colsum; g.zero_page = zero;
        return wide_gemm_nt(g, st);
    }
    // y = LN(x) w + b over `rows` rows; out_map (ragged batches): row r leaves at y[out_map[r]]
    int ln(const float* x, const float* w, const float* b, float* stats, float* y32, bf16_t* y16, int rows, int d, const int* out_map = nullptr) const {
        WideLnFwdParams lp;
        lp.x = x; lp.w = w; lp.b = b; lp.eps = ln_eps; lp.stats = stats; lp.y32 = y32; lp.y16 = y16; lp.rows = rows; lp.d = d; lp.out_map = out_map;
        return out_map ? wide_ln_fwd_mapped(lp, st) : wide_ln_fwd(lp, st);
    }
    // dx32 = d(pre), dx16 = outm .* dx32; dw / db / dbias += the parameter gradients, queued on the ledger where it has a region left.
    // dy_map (ragged batches): row r reads dy[dy_map[r]]; summed at once (the mapped kernel is not queued)
    int ln_bwd(const float* dy, const float* pre, const float* stats, const float* w, const WideDrop& outm, float* dw, float* db, float* dbias,
               float* dx32, bf16_t* dx16, int rows, int d, const int* dy_map = nullptr) const {
        WideLnBwdParams b;
        b.dy = dy; b.pre = pre; b.stats = stats; b.w = w; b.dx32 = dx32; b.dx16 = dx16; b.rows = rows; b.d = d;
        b.out_key = outm.key; b.out_thresh = outm.thresh; b.out_inv = outm.inv;
        b.dw = dw; b.db = db; b.dbias = dbias; b.dy_map = dy_map;
        if (dy_map) return wide_ln_bwd_mapped(b, led->lnpart, st);
        void* reg = led->row_region(wide_ln_bwd_scratch(rows, d));
        return reg ? wide_ln_bwd(b, reg, st, &led->rrb) : wide_ln_bwd(b, led->lnpart, st);
    }
};

// ---- the post-LN sublayers ----------------------------------------------------------------------------------------------------------------
// y = LN(res), res = dropout_site(a16 W^T + bias) + resid: the out-projection of an attention, or linear2 of the FFN, over `rows` rows
struct WideProjLn {
    bf16_t* a16; int K;                             // the projection's operand rows (rows, K): written by whatever runs ahead of it
    const bf16_t* w; const bf16_t* w_t;             // W (d, K); W^T (backward)
    const float* bias; const float* resid;
    float* res; float* stats;                       // kept for the backward: the pre-LN sum and its statistics
    const float* ln_w; const float* ln_b;
    float* y32; bf16_t* y16;                        // (forward)
    uint32_t site;                                  // dropout site of the branch
};
struct WideProjLnGrads { float* w; float* bias; float* ln_w; float* ln_b; };
// y = LN(x + dropout_out(linear2(dropout_site(relu(linear1(x)))))): out.a16 is the hidden, out.resid is x
struct WideFfn {
    const bf16_t* x16; const bf16_t* w1; const bf16_t* w1_t; const float* b1; int dff; uint32_t site;
    WideProjLn out;
};
struct WideFfnGrads { float* w1; float* b1; WideProjLnGrads out; };

inline int wide_proj_ln_fwd(const WideRun& r, const WideProjLn& p, uint32_t layer, int rows, int d, const int* out_map = nullptr) {
    if (r.nt(p.a16, p.w, rows, d, p.K, p.bias, p.res, nullptr, 0, r.drop(r.p_drop, layer, p.site), p.resid)) return 1;
    return r.ln(p.res, p.ln_w, p.ln_b, p.stats, p.y32, p.y16, rows, d, out_map);
}
inline int wide_ffn_fwd(const WideRun& r, const WideFfn& f, uint32_t layer, int rows, int d, const int* out_map = nullptr) {
    if (r.nt(f.x16, f.w1, rows, f.dff, d, f.b1, nullptr, f.out.a16, 1, r.drop(r.p_drop, layer, f.site), nullptr)) return 1;
    return wide_proj_ln_fwd(r, f.out, layer, rows, d, out_map);
}
// LayerNorm backward of dy: dres = d(res), dy16 = the branch's dropout mask .* d(res), with d(ln_w), d(ln_b), d(bias); then d(W) from dy16.
// fork(): the decoder's side-stream fork ahead of the weight gradient (the encoder passes a no-op). The caller takes dy16 on to d(a16).
template <class Fork>
int wide_proj_ln_bwd(const WideRun& r, const WideProjLn& p, const WideProjLnGrads& g, uint32_t layer, int rows, int d, const float* dy, float* dres,
                     bf16_t* dy16, Fork&& fork, const int* dy_map = nullptr) {
    if (r.ln_bwd(dy, p.res, p.stats, p.ln_w, r.drop(r.p_drop, layer, p.site), g.ln_w, g.ln_b, g.bias, dres, dy16, rows, d, dy_map)) return 1;
    return fork() || r.led->dw_tn(dy16, p.a16, g.w, d, p.K, rows);
}
// The FFN backward chain: LayerNorm backward and d(W2); d(hidden) = (dy16 W2) .* alive / keep with its column sums -> d(b1); d(W1);
// dx = d(hidden) W1 + dres
template <class Fork>
int wide_ffn_bwd(const WideRun& r, const WideFfn& f, const WideFfnGrads& g, uint32_t layer, int rows, int d, const float* dy, float* dres,
                 bf16_t* dy16, bf16_t* dhid16, float* dx, Fork&& fork, const int* dy_map = nullptr) {
    WideLedger& led = *r.led;
    if (wide_proj_ln_bwd(r, f.out, g.out, layer, rows, d, dy, dres, dy16, fork, dy_map)) return 1;
    const int cs_rows = wide_gemm_nt_colsum_rows(rows, f.dff);
    float* cs_reg = g.b1 ? (float*)led.row_region((size_t)cs_rows * f.dff * 4) : nullptr;
    float* cs = g.b1 ? (cs_reg ? cs_reg : led.cspart) : nullptr;
    if (r.nt_bwd(dy16, f.out.w_t, rows, f.dff, d, nullptr, dhid16, nullptr, f.out.a16, r.drop(r.p_drop, layer, f.site).inv, cs)) return 1;
    if (g.b1 && wide_reduce_rows(cs, cs_rows, f.dff, g.b1, r.st, cs_reg ? &led.rrb : nullptr)) return 1;
    if (fork() || led.dw_tn(dhid16, f.x16, g.w1, f.dff, d, rows)) return 1;
    return r.nt_bwd(dhid16, f.w1_t, rows, d, f.dff, dx, nullptr, dres);
}

}  // namespace egx
