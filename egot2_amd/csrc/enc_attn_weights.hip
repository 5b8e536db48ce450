// The encoder's self-attention weights as an output (ABI v27 additions: egx_self_attention_weights, egx_attention_rollout,
// egx_encoder_self_weights): what nn.MultiheadAttention returns with need_weights=True for the self_attn of an nn.TransformerEncoderLayer
// (the reference's layers call it with need_weights=False; a user patches the layer to see them), their per-task sums, and the attention
// rollout over the layers (Abnar & Zuidema 2020):
//   w[b, i, j]   = (1 / H) sum_h softmax_j(q[b, i, h, :] . k[b, j, h, :] / sqrt(DH))          i, j < S_b
//   seg[b, i, t] = sum_{j in segment t of clip b} w[b, i, j]
//   R_l          = ((w_l + I) / 2) . R_{l-1},  R_0 = I
//
// enc_self_weights_kernel: a 256-thread workgroup owns 16 query rows of one clip and walks the heads in order 0 .. H - 1. Per head the four
// waves share the clip's key tiles of 16 (wave w: tiles w, w + 4, ...): a tile's 16 x 16 scores are DH / 4 v_mfma_f32_16x16x4_f32 on operands
// read straight from global memory (every lane one 16-byte load per 16 columns of its row: lane (r, g) holds columns 16 t + 4 g .. + 3 of row
// r, the same k order in both operands), so the clip's K rows are read once per 16 query rows. bf16 operands are widened to fp32 (exact) and
// take the same instruction: every product is exact, the sum an fp32 fma chain. The scaled scores go to LDS (16 x 516 floats: the row
// stride spreads the four row groups of an accumulator tile over the banks); after a barrier wave w owns rows 4 w .. 4 w + 3: lane l holds keys
// l, l + 64, ... (eight accumulators per row), maximum and sum by the wave's xor tree, exp and the division in fp32, and adds e / sum to
// its head sum: heads in head order, one multiplication by 1 / H at the end. The finished tile goes to global memory (if asked for) and to
// LDS, where thread (row, segment) adds its segment's entries one after the other in key order. No atomics; the clip's index enters
// addresses only, so a clip's rows have the same bits wherever the clip sits in the batch. Rows i >= S_b and entries j >= S_b of the S
// written ones are exact zeros; an empty slot (S_b = 0) writes zeros and reads nothing, its table entries apart.
//
// enc_rollout_kernel: the same tile ownership. The 16 x S_b tile of A = (w + I) / 2 is staged in LDS; without a predecessor it IS the
// result (L = 1: exactly (w + I) / 2), else wave w accumulates column tiles w, w + 4, ... (up to eight 16 x 16 accumulators) over k = 0, 4, ...
// with the same fp32 MFMA: an fma chain in ascending k. The result tile passes through LDS for coalesced stores and the segment sums.
#include <math.h>

#include "../../include/egot2x.h"
#include "enc_attn_weights.h"

namespace egx {

namespace {

constexpr int SW_LD = SW_MAXS + 4;          // LDS row stride in floats: 4 rows apart = 16 banks apart
constexpr int SW_THREADS = 256;
constexpr int SW_KEYS = SW_MAXS / 64;       // keys per lane in the softmax pass

template <bool F32>
__device__ __forceinline__ void load4(const void* p, size_t idx, float (&v)[4]) {
    if (F32) {
        const float4 x = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + idx);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        const uint2 x = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(p) + idx);
        v[0] = __uint_as_float(x.x << 16); v[1] = __uint_as_float(x.x & 0xffff0000u);
        v[2] = __uint_as_float(x.y << 16); v[3] = __uint_as_float(x.y & 0xffff0000u);
    }
}

// clip b's token count and (self weights) first row
__device__ __forceinline__ int clip_len(const int* tab, int stride, int at, int b, int S) {
    if (!tab) return S;
    const int n = tab[(size_t)b * stride + at];
    return n < 0 ? 0 : (n > S ? S : n);
}

// rows [i0, i0 + 16) of a clip without tokens there: zeros over the S written entries
__device__ __forceinline__ void zero_tile(float* out, size_t ld, float* seg, int K, size_t orow0, int i0, int S, int t) {
    const int rows = S - i0 < SW_ROWS ? S - i0 : SW_ROWS;
    if (out)
        for (int rr = 0; rr < rows; ++rr)
            for (int j = t; j < S; j += SW_THREADS) out[(orow0 + rr) * ld + j] = 0.f;
    if (seg)
        for (int e = t; e < rows * K; e += SW_THREADS) seg[orow0 * K + e] = 0.f;
}

// sT: the finished 16 x S_b tile. Thread (row = t & 15, segment = t >> 4) adds the entries of its segment in key order.
__device__ __forceinline__ void segment_sums(const float* sT, const int* lens /* LDS */, int K, int Sb, int S, int i0, float* seg_rows, int t) {
    if (t >= SW_ROWS * K) return;
    const int row = t & 15, sg = t >> 4;
    int lo = 0;
    for (int u = 0; u < sg; ++u) {
        const int n = lens[u];
        lo = (n > 0 && n < Sb - lo) ? lo + n : (n > 0 ? Sb : lo);
    }
    const int n = lens[sg];
    const int hi = (n > 0 && n < Sb - lo) ? lo + n : (n > 0 ? Sb : lo);
    float s = 0.f;
#pragma unroll 4
    for (int j = lo; j < hi; ++j) s += sT[row * SW_LD + j];
    if (i0 + row < S) seg_rows[row * K + sg] = i0 + row < Sb ? s : 0.f;
}

// lane (r, g) of a key tile: columns col0 + 16 t .. + 3 (col0 = h DH + 4 g) of key row j, zeros behind the clip's last key (nothing is read there)
template <int DH, bool F32>
__device__ __forceinline__ void load_key_tile(const void* k, size_t row0, int ldk, int col0, int j, int Sb, float (&kf)[DH / 4]) {
    const size_t koff = (row0 + j) * (size_t)ldk + col0;
#pragma unroll
    for (int tt = 0; tt < DH / 16; ++tt) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (j < Sb) load4<F32>(k, koff + 16 * tt, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) kf[4 * tt + e] = v[e];
    }
}
// 16 x 16 scores of one key tile: an fp32 fma chain over the head's DH columns; accumulator element e is query row 4 g + e, key column r
template <int DH>
__device__ __forceinline__ void score_tile(const float (&qf)[DH / 4], const float (&kf)[DH / 4], float* dst, float scale) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < DH / 4; ++e) c = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[e], kf[e], c, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[e * SW_LD] = c[e] * scale;
}

template <int DH, bool F32>
__global__ __launch_bounds__(SW_THREADS) void enc_self_weights_kernel(SelfWParams p) {
    __shared__ float sS[SW_ROWS * SW_LD];
    __shared__ int sLens[SW_MAXSEG];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    const int tiles = (p.S + SW_ROWS - 1) / SW_ROWS;
    const int b = blockIdx.x / tiles, i0 = (blockIdx.x - b * tiles) * SW_ROWS;
    const int Sb = clip_len(p.rowtab, p.tab_stride, 1, b, p.S);
    const size_t orow0 = (size_t)b * p.S + i0;
    if (i0 >= Sb) {         // (uniform over the workgroup, before any barrier)
        zero_tile(p.w, (size_t)p.ldw, p.seg, p.K, orow0, i0, p.S, t);
        return;
    }
    size_t row0 = (size_t)b * (size_t)p.clip_rows;
    if (p.rowtab) {
        const int first = p.rowtab[(size_t)b * p.tab_stride];
        row0 = (size_t)(first < 0 ? 0 : first) * (size_t)p.row_mul;
    }
    if (p.seg && t < p.K) sLens[t] = p.segtab ? p.segtab[(size_t)b * p.seg_stride + t] : p.seg_fixed[t];     // (visible behind the barriers below)
    const int nkt = (Sb + 15) >> 4;
    const bool qok = i0 + r < Sb;
    const size_t qoff = (row0 + i0 + r) * (size_t)p.ldq + 4 * g;
    float acc[4][SW_KEYS];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int c = 0; c < SW_KEYS; ++c) acc[rr][c] = 0.f;

    for (int h = 0; h < p.H; ++h) {             // (uniform trip count: every barrier below is reached by all 256 threads)
        float qf[DH / 4];
#pragma unroll
        for (int tt = 0; tt < DH / 16; ++tt) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (qok) load4<F32>(p.q, qoff + h * DH + 16 * tt, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) qf[4 * tt + e] = v[e];
        }
        // two key tiles per trip: the loads of both are in flight before the first product
        for (int kt = wave; kt < nkt; kt += 8) {
            const bool two = kt + 4 < nkt;          // (uniform over the wave)
            float kf0[DH / 4], kf1[DH / 4];
            load_key_tile<DH, F32>(p.k, row0, p.ldk, h * DH + 4 * g, kt * 16 + r, Sb, kf0);
            if (two) load_key_tile<DH, F32>(p.k, row0, p.ldk, h * DH + 4 * g, (kt + 4) * 16 + r, Sb, kf1);
            score_tile<DH>(qf, kf0, sS + 4 * g * SW_LD + kt * 16 + r, p.scale);
            if (two) score_tile<DH>(qf, kf1, sS + 4 * g * SW_LD + (kt + 4) * 16 + r, p.scale);
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const float* srow = sS + (4 * wave + rr) * SW_LD;
            float s[SW_KEYS];
            float m = -INFINITY;
#pragma unroll
            for (int c = 0; c < SW_KEYS; ++c) {
                const int j = lane + 64 * c;
                s[c] = j < Sb ? srow[j] : -INFINITY;
                m = fmaxf(m, s[c]);
            }
            m = wave_max(m);
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < SW_KEYS; ++c) {
                s[c] = lane + 64 * c < Sb ? __expf(s[c] - m) : 0.f;
                sum += s[c];
            }
            sum = wave_sum(sum);
#pragma unroll
            for (int c = 0; c < SW_KEYS; ++c) acc[rr][c] += s[c] / sum;
        }
        __syncthreads();
    }

#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int row = 4 * wave + rr, i = i0 + row;
#pragma unroll
        for (int c = 0; c < SW_KEYS; ++c) {
            const int j = lane + 64 * c;
            const float v = (i < Sb && j < Sb) ? acc[rr][c] * p.inv_h : 0.f;
            if (j < Sb) sS[row * SW_LD + j] = v;
            if (p.w && i < p.S && j < p.S) p.w[(orow0 + row) * (size_t)p.ldw + j] = v;
        }
    }
    if (!p.seg) return;
    __syncthreads();
    segment_sums(sS, sLens, p.K, Sb, p.S, i0, p.seg + orow0 * p.K, t);
}

__global__ __launch_bounds__(SW_THREADS) void enc_rollout_kernel(RolloutParams p) {
    __shared__ float sA[SW_ROWS * SW_LD];
    __shared__ int sLens[SW_MAXSEG];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, r = lane & 15, g = lane >> 4;
    const int tiles = (p.S + SW_ROWS - 1) / SW_ROWS;
    const int b = blockIdx.x / tiles, i0 = (blockIdx.x - b * tiles) * SW_ROWS;
    const int Sb = clip_len(p.rowlen, p.len_stride, 0, b, p.S);
    const size_t orow0 = (size_t)b * p.S + i0;
    if (i0 >= Sb) {
        zero_tile(p.out, (size_t)p.S, p.seg, p.K, orow0, i0, p.S, t);
        return;
    }
    const size_t base = (size_t)b * p.S * p.S;
    if (p.seg && t < p.K) sLens[t] = p.segtab ? p.segtab[(size_t)b * p.seg_stride + t] : p.seg_fixed[t];     // (visible behind the barrier below)
    const int S4 = (Sb + 3) & ~3;               // the k loop's extent: zeros behind the clip's tokens (S4 <= 512 < SW_LD)
    for (int row = wave; row < SW_ROWS; row += 4) {
        const int i = i0 + row;
        for (int k = lane; k < S4; k += 64)
            sA[row * SW_LD + k] = (i < Sb && k < Sb) ? (p.w[base + (size_t)i * p.S + k] + (i == k ? 1.f : 0.f)) * 0.5f : 0.f;
    }
    __syncthreads();
    if (p.prev) {
        const int nct = (Sb + 15) >> 4;
        f32x4 c[SW_MAXS / 64];
#pragma unroll
        for (int u = 0; u < SW_MAXS / 64; ++u) c[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int k0 = 0; k0 < S4; k0 += 4) {
            const int kk = k0 + g;
            const float a = sA[r * SW_LD + kk];
            const float* prow = p.prev + base + (size_t)kk * p.S;
#pragma unroll
            for (int u = 0; u < SW_MAXS / 64; ++u) {
                const int ct = wave + 4 * u;
                if (ct < nct) {         // (uniform over the wave)
                    const int j = ct * 16 + r;
                    const float bv = (kk < Sb && j < Sb) ? prow[j] : 0.f;
                    c[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, c[u], 0, 0, 0);
                }
            }
        }
        __syncthreads();        // every wave has read its last A operands
#pragma unroll
        for (int u = 0; u < SW_MAXS / 64; ++u) {
            const int ct = wave + 4 * u;
            if (ct < nct)
#pragma unroll
                for (int e = 0; e < 4; ++e) sA[(4 * g + e) * SW_LD + ct * 16 + r] = c[u][e];
        }
        __syncthreads();
    }
    if (p.out)
        for (int row = wave; row < SW_ROWS; row += 4) {
            const int i = i0 + row;
            if (i < p.S)
                for (int j = lane; j < p.S; j += 64) p.out[base + (size_t)i * p.S + j] = (i < Sb && j < Sb) ? sA[row * SW_LD + j] : 0.f;
        }
    if (p.seg) segment_sums(sA, sLens, p.K, Sb, p.S, i0, p.seg + orow0 * p.K, t);
}

}  // namespace

int self_weights(SelfWParams p, int dh, bool f32, hipStream_t st) {
    const char* who = "egx_self_attention_weights";
    EGX_CHECK(p.q && p.k, "%s: null pointer argument (q, k)", who);
    EGX_CHECK(p.w || p.seg, "%s: null pointer argument (w_out and seg_out are both null)", who);
    EGX_CHECK(dh == 16 || dh == 32 || dh == 64 || dh == 96 || dh == 128, "%s: head dim %d (16, 32, 64, 96 or 128)", who, dh);
    EGX_CHECK(p.S >= 1 && p.S <= SW_MAXS, "%s: S = %d (1..%d)", who, p.S, SW_MAXS);
    EGX_CHECK(p.H >= 1 && p.B >= 0, "%s: B = %d, H = %d", who, p.B, p.H);
    EGX_CHECK(!p.w || p.ldw >= p.S, "%s: ldw = %d < S = %d", who, p.ldw, p.S);
    EGX_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldq >= p.H * dh && p.ldk >= p.H * dh,
              "%s: ldq = %d, ldk = %d (multiples of 8 elements, at least H * dh = %d)", who, p.ldq, p.ldk, p.H * dh);
    EGX_CHECK(((uintptr_t)p.q | (uintptr_t)p.k) % 16 == 0, "%s: q and k must be 16-byte aligned", who);
    EGX_CHECK(!p.seg || ((p.segtab || p.fixed_segs) && p.K >= 1 && p.K <= SW_MAXSEG), "%s: seg_out needs a segment table and K = %d in 1..%d", who, p.K, SW_MAXSEG);
    const long long grid = (long long)p.B * cdiv(p.S, SW_ROWS);
    EGX_CHECK(grid <= 0x7fffffffLL, "%s: B * ceil(S / 16) = %lld workgroups", who, grid);
    if (p.B == 0) return 0;
    p.scale = 1.f / sqrtf((float)dh); p.inv_h = 1.f / (float)p.H;
    const dim3 gd((unsigned)grid), block(SW_THREADS);
#define EGX_SW_LAUNCH(DH_) \
    do { if (f32) hipLaunchKernelGGL((enc_self_weights_kernel<DH_, true>), gd, block, 0, st, p); \
         else hipLaunchKernelGGL((enc_self_weights_kernel<DH_, false>), gd, block, 0, st, p); } while (0)
    if (dh == 16) EGX_SW_LAUNCH(16);
    else if (dh == 32) EGX_SW_LAUNCH(32);
    else if (dh == 64) EGX_SW_LAUNCH(64);
    else if (dh == 96) EGX_SW_LAUNCH(96);
    else EGX_SW_LAUNCH(128);
#undef EGX_SW_LAUNCH
    EGX_LAUNCH_CHECK();
    return 0;
}

int self_weights_layers(SelfWParams p, const void* qkv0, size_t layer_bytes, int d_model, int L, uint64_t layer_mask, bool f32, hipStream_t st) {
    float* w0 = p.w;
    float* seg0 = p.seg;
    const size_t esz = f32 ? 4 : 2;
    int n = 0;
    for (int l = 0; l < L; ++l) {
        if (!((layer_mask >> l) & 1)) continue;
        p.q = (const char*)qkv0 + (size_t)l * layer_bytes;
        p.k = (const char*)p.q + (size_t)d_model * esz;
        p.w = w0 ? w0 + (size_t)n * p.B * p.S * p.ldw : nullptr;
        p.seg = seg0 ? seg0 + (size_t)n * p.B * p.S * p.K : nullptr;
        if (self_weights(p, d_model / p.H, f32, st)) return 1;
        ++n;
    }
    return 0;
}

int rollout_step(const RolloutParams& p, hipStream_t st) {
    const dim3 gd((unsigned)(p.B * cdiv(p.S, SW_ROWS))), block(SW_THREADS);
    hipLaunchKernelGGL(enc_rollout_kernel, gd, block, 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

static size_t rollout_buf_bytes(int B, int S) { return align_up((size_t)B * S * S * 4, 256); }
size_t rollout_scratch_bytes(int L, int B, int S) {
    if (L < 2 || B < 1 || S < 1) return 0;
    return (L == 2 ? 1 : 2) * rollout_buf_bytes(B, S);
}

// R_1 = A_1 goes to the first scratch buffer (L = 1: to the output), every further product to the other one, the last to the output
int rollout(const float* w, int L, int B, int S, const int* rowlen, int len_stride, const int* segtab, int seg_stride, const int* seg_fixed, int K, void* scratch,
            float* out, float* seg_out, hipStream_t st) {
    const char* who = "egx_attention_rollout";
    EGX_CHECK(w, "%s: null pointer argument (w)", who);
    EGX_CHECK(out || seg_out, "%s: null pointer argument (out and seg_out are both null)", who);
    EGX_CHECK(L >= 1 && L <= 64, "%s: L = %d layers (1..64)", who, L);
    EGX_CHECK(S >= 1 && S <= SW_MAXS, "%s: S = %d (1..%d)", who, S, SW_MAXS);
    EGX_CHECK(B >= 0, "%s: B = %d", who, B);
    EGX_CHECK(!seg_out || ((segtab || seg_fixed) && K >= 1 && K <= SW_MAXSEG), "%s: seg_out needs a segment table and K = %d in 1..%d", who, K, SW_MAXSEG);
    EGX_CHECK(L == 1 || scratch, "%s: null scratch with L = %d layers (egx_attention_rollout_scratch)", who, L);
    EGX_CHECK((long long)B * cdiv(S, SW_ROWS) <= 0x7fffffffLL, "%s: B * ceil(S / 16) workgroups", who);
    if (B == 0) return 0;
    float* buf[2] = {(float*)scratch, (float*)((char*)scratch + rollout_buf_bytes(B, S))};
    const size_t layer = (size_t)B * S * S;
    const float* prev = nullptr;
    for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        RolloutParams p;
        p.w = w + l * layer; p.prev = prev; p.out = last ? out : buf[l & 1]; p.seg = last ? seg_out : nullptr;
        p.rowlen = rowlen; p.len_stride = len_stride; p.segtab = segtab; p.seg_stride = seg_stride; p.K = K; p.B = B; p.S = S;
        for (int u = 0; u < SW_MAXSEG; ++u) p.seg_fixed[u] = (!segtab && seg_fixed && u < K) ? seg_fixed[u] : 0;
        if (rollout_step(p, st)) return 1;
        prev = p.out;
    }
    return 0;
}

}  // namespace egx

using namespace egx;

extern "C" {

int egx_self_attention_weights(const void* q, int ldq, const void* k, int ldk, int operands_bf16, const int* rowtab, const int* segtab, int K, int B,
                               int H, int dh, int S, float* w_out, int ldw, float* seg_out, void* stream) {
    SelfWParams p;
    p.q = q; p.k = k; p.ldq = ldq; p.ldk = ldk; p.rowtab = rowtab; p.tab_stride = 2; p.row_mul = 1; p.clip_rows = S;
    p.segtab = segtab; p.seg_stride = K; p.K = K; p.w = w_out; p.ldw = ldw; p.seg = seg_out; p.B = B; p.H = H; p.S = S;
    p.scale = 0.f; p.inv_h = 0.f; p.fixed_segs = 0;
    for (int u = 0; u < SW_MAXSEG; ++u) p.seg_fixed[u] = 0;
    return self_weights(p, dh, !operands_bf16, (hipStream_t)stream);
}

size_t egx_attention_rollout_scratch(int L, int B, int S) { return rollout_scratch_bytes(L, B, S); }

int egx_attention_rollout(const float* w, int L, int B, int S, const int* rowlen, const int* segtab, int K, void* scratch, float* out, float* seg_out,
                          void* stream) {
    return rollout(w, L, B, S, rowlen, 1, segtab, K, nullptr, K, scratch, out, seg_out, (hipStream_t)stream);
}

}  // extern "C"
