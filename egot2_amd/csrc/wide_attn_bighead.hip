// MFMA attention of the wide path for LARGE heads over SHORT sequences: head dim 256 / 512, 1 <= S <= 16 tokens per clip. The 2048-wide HOI LTA
// 2-task translator (HOI/configs/lta/ts_lta_2task.yaml:79-82: TRANSLATION_INPUT_FEATURES 2048, TRANSLATION_HEADS 4 -> head dim 512, two streams of
// NUM_INPUT_CLIPS 2 -> S = 4; the config defaults' 8 heads -> head dim 256) inside nn.TransformerEncoderLayer
// (HOI/models/lta/lta_models_lta_transfer.py:429-526). Same operands, log-sum-exp and dropout keying as wide_attn.hip's S <= 128 class.
//
// One WAVE per (clip, head), four to a workgroup, nothing shared between them. The whole score matrix of a head is ONE 16 x 16 tile (the
// sequence padded to 16), accumulated over dh / 32 steps of mfma_f32_16x16x32_bf16 from row fragments; the softmax runs on the four
// accumulator registers of a lane plus two cross-lane steps. Every product against the padded key tile (O = P V forward; dQ = dS K,
// dK = dS^T Q, dV = P^T dO backward) is ONE mfma_f32_16x16x16_bf16 per 16 output columns with a zero accumulator: its probability operand
// is the score tile as it sits in the registers, its other operand a transposed read (ds_read_b64_tr_b16) of a wave-private token-major
// LDS image in wide_attn.hip's row format (16 rows of 2 dh + 32 bytes). No accumulator lives across column tiles, so the register count does
// not grow with the head dim.
// Forward: one image (V) per wave. Backward: two image slots per wave, K | Q for the scores, dQ and dK, then dO over K's slot for dV
// (three images of four waves would not fit the LDS at head dim 512). The backward recomputes P from the log-sum-exp in BOTH orientations
// (key on the accumulator rows for delta and dQ, query on the rows for dK and dV) from the same row fragments, A and B operand swapped.
// Rows >= S of a tile: their probabilities are exact zeros, their images zero rows, and they are never written. Every output element is
// written by exactly one wave: no atomics, bitwise reproducible.
// A wave past the last (clip, head) of a partial workgroup recomputes the last pair and writes nothing (it still meets the barriers).
#include "common.h"
#include "wide.h"
#include "fused.h"

namespace egx {

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int BGH_NW = 4, BGH_NTH = BGH_NW * 64, BGH_SP = WIDE_ATTN_BIGHEAD_MAX_S;      // waves per workgroup; rows of an image

__device__ __forceinline__ bf16x8 lds128(const unsigned char* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x8 ldg128(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }
// lanes 16 j .. 16 j + 15 address a 4 (row) x 16 (column) block, four bf16 each; lane r of the group receives column r's four rows
__device__ __forceinline__ s16x4 lds_tr(const unsigned char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
}
// an accumulator tile (rows 4g + e on the registers) as the B operand of a 16-deep product
__device__ __forceinline__ s16x4 pk4(const f32x4& t) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 u = {pack_bf16x2(t[0], t[1]), pack_bf16x2(t[2], t[3])};
    return __builtin_bit_cast(s16x4, u);
}
__device__ __forceinline__ f32x4 mfma32(const bf16x8& a, const bf16x8& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(const s16x4& a, const s16x4& b) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, f32x4{0, 0, 0, 0}, 0, 0, 0);
}
__device__ __forceinline__ void st4(bf16_t* o, const f32x4& t) {
    *reinterpret_cast<uint2*>(o) = make_uint2(pack_bf16x2(t[0], t[1]), pack_bf16x2(t[2], t[3]));
}

// one wave copies `rows` token rows of a head (DH bf16 each, global row stride ld elements) into its image; rows [rows, 16) are zero-filled.
// Eight 16-byte loads in flight per lane.
template <int DH>
__device__ __forceinline__ void stage16(unsigned char* img, const bf16_t* src, int ld, int rows, int lane) {
    constexpr int RS = DH * 2 + 32, CH = DH / 8, NIT = BGH_SP * CH / 64;
    static_assert(NIT % 8 == 0, "stage16: eight chunks per step");
#pragma unroll
    for (int i0 = 0; i0 < NIT; i0 += 8) {
        uint4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = lane + (i0 + u) * 64, row = i / CH, c = i % CH;
            v[u] = make_uint4(0, 0, 0, 0);
            if (row < rows) v[u] = *reinterpret_cast<const uint4*>(src + (size_t)row * ld + c * 8);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = lane + (i0 + u) * 64, row = i / CH, c = i % CH;
            *reinterpret_cast<uint4*>(img + row * RS + c * 16) = v[u];
        }
    }
}

}  // namespace

// ---- forward ----------------------------------------------------------------------------------------------------
// lane (r = lane & 15, g = lane >> 4): query r, keys 4g .. 4g + 3 (scores transposed, S^T = K Q^T, as in wide_attn_fwd_kernel)
template <int DH>
__global__ __launch_bounds__(BGH_NTH) void wide_attn_bighead_fwd_kernel(WideAttnParams p) {
    const uint64_t dkey = p.drop_thresh ? resolve_key(p.drop_key) : 0ull;
    constexpr int RS = DH * 2 + 32, NKB = DH / 32, NCT = DH / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int npair = p.B * p.H, pair = blockIdx.x * BGH_NW + wave;
    const bool active = pair < npair;
    const int bh = active ? pair : npair - 1, h = bh % p.H, b = bh / p.H;
    const int S = p.S, d = p.d, ld = 3 * d;
    const size_t row0 = (size_t)b * S;
    const bf16_t* base = p.qkv + row0 * ld + h * DH;
    unsigned char* Vimg = smem + wave * BGH_SP * RS;
    stage16<DH>(Vimg, base + 2 * d, ld, S, lane);
    const int rrow = r < S ? r : S - 1;                       // rows >= S read the last token: finite, masked below, never written
    const bf16_t* qp = base + (size_t)rrow * ld + 8 * g;
    const bf16_t* kp = qp + d;
    f32x4 sc = f32x4{0, 0, 0, 0};
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) sc = mfma32(ldg128(kp + kb * 32), ldg128(qp + kb * 32), sc);
    const float scale = rsqrtf((float)DH);
    float m = -INFINITY;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float s = 4 * g + e < S ? sc[e] * scale : -INFINITY;
        sc[e] = s;
        m = fmaxf(m, s);
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float pv = __expf(sc[e] - m); sc[e] = pv; sum += pv; }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    const bool wr = active && r < S;
    if (wr && g == 0) p.lse[(size_t)bh * S + r] = m + __logf(sum);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pv = sc[e] * inv;
        if (p.drop_thresh) pv *= drop_scale(dkey, (uint32_t)(bh * 128 + r), (uint32_t)(4 * g + e), p.drop_thresh, p.drop_inv);
        sc[e] = pv;
    }
    const s16x4 pf = pk4(sc);
    __syncthreads();                                           // the image is complete
    const unsigned char* v0 = Vimg + (4 * g + (r >> 2)) * RS + 8 * (r & 3);
    bf16_t* o = p.out + (row0 + rrow) * d + h * DH + 4 * g;
#pragma unroll 8
    for (int ct = 0; ct < NCT; ++ct) {
        const f32x4 oc = mfma16(lds_tr(v0 + ct * 32), pf);    // O^T: columns ct * 16 + 4g + e of query r
        if (wr) st4(o + ct * 16, oc);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------
// orientation T (key on the accumulator rows, query on the lane): delta = rowsum(P .* dP) and dQ; orientation N (query on the rows, key on
// the lane): dK and dV. Both from the same row fragments.
template <int DH>
__global__ __launch_bounds__(BGH_NTH) void wide_attn_bighead_bwd_kernel(WideAttnParams p) {
    const uint64_t dkey = p.drop_thresh ? resolve_key(p.drop_key) : 0ull;
    constexpr int RS = DH * 2 + 32, NKB = DH / 32, NCT = DH / 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int npair = p.B * p.H, pair = blockIdx.x * BGH_NW + wave;
    const bool active = pair < npair;
    const int bh = active ? pair : npair - 1, h = bh % p.H, b = bh / p.H;
    const int S = p.S, d = p.d, ld = 3 * d;
    const size_t row0 = (size_t)b * S;
    const bf16_t* base = p.qkv + row0 * ld + h * DH;
    const bf16_t* dout = p.d_out + row0 * d + h * DH;
    unsigned char* img0 = smem + wave * 2 * BGH_SP * RS;       // K, later dO
    unsigned char* img1 = img0 + BGH_SP * RS;                  // Q
    stage16<DH>(img0, base + d, ld, S, lane);
    stage16<DH>(img1, base, ld, S, lane);
    const int rrow = r < S ? r : S - 1;
    const float lqT = p.lse[(size_t)bh * S + rrow];            // log-sum-exp of query r
    // The keep-scales of both orientations are drawn HERE, ahead of the score products, and pinned: between the last MFMA of the score loop
    // and the first read of its accumulators there must be no branch target. With the `p.drop_thresh ?` branches behind the loop hipcc laid
    // the no-dropout side out as a block entered by a jump, counted the other side's instructions as its wait states and read the LAST
    // product's fourth register three instructions after issuing it: at head dim 256 dP^T of keys 3, 7, 11, 15 missed its last 32 columns.
    float ksT[4] = {1.f, 1.f, 1.f, 1.f}, ksN[4] = {1.f, 1.f, 1.f, 1.f};
    if (p.drop_thresh) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            ksT[e] = drop_scale(dkey, (uint32_t)(bh * 128 + r), (uint32_t)(4 * g + e), p.drop_thresh, p.drop_inv);
            ksN[e] = drop_scale(dkey, (uint32_t)(bh * 128 + 4 * g + e), (uint32_t)r, p.drop_thresh, p.drop_inv);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(ksT[e]), "+v"(ksN[e]));
    const bf16_t* vp = base + 2 * d + (size_t)rrow * ld + 8 * g;
    const bf16_t* dp = dout + (size_t)rrow * d + 8 * g;
    __syncthreads();
    f32x4 aT = f32x4{0, 0, 0, 0}, cT = aT, aN = aT, cN = aT;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        const bf16x8 kf = lds128(img0 + r * RS + (kb * 32 + 8 * g) * 2), qf = lds128(img1 + r * RS + (kb * 32 + 8 * g) * 2);
        const bf16x8 vf = ldg128(vp + kb * 32), df = ldg128(dp + kb * 32);
        aT = mfma32(kf, qf, aT);        // S^T [key 4g + e][query r]
        aN = mfma32(qf, kf, aN);        // S   [query 4g + e][key r]
        cT = mfma32(vf, df, cT);        // dP^T
        cN = mfma32(df, vf, cN);        // dP
    }
    asm volatile("" : "+v"(aT), "+v"(cT), "+v"(aN), "+v"(cN));       // read out in the block of the MFMAs (see above); straight-line code from here
    const float scale = rsqrtf((float)DH);
    // orientation T
    float dl = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int key = 4 * g + e;
        const float pv = (key < S && r < S) ? __expf(aT[e] * scale - lqT) : 0.f;
        const float dm = cT[e] * ksT[e];
        dl += pv * dm;
        aT[e] = pv; cT[e] = dm;
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);                              // delta of query r, on all four lanes of it
#pragma unroll
    for (int e = 0; e < 4; ++e) cT[e] = aT[e] * (cT[e] - dl) * scale;      // dS^T
    // orientation N: query 4g + e, key r; the query's statistics sit on lane 4g + e
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int query = 4 * g + e;
        const float lq = __shfl(lqT, query, 64), dq = __shfl(dl, query, 64);
        const float pv = (r < S && query < S) ? __expf(aN[e] * scale - lq) : 0.f;
        aN[e] = pv * ksN[e];                                   // dropped P
        cN[e] = pv * (ksN[e] * cN[e] - dq) * scale;            // dS
    }
    const s16x4 sT = pk4(cT), pN = pk4(aN), sN = pk4(cN);
    const bool wr = active && r < S;
    const int toff = (4 * g + (r >> 2)) * RS + 8 * (r & 3);
    bf16_t* gq = p.d_qkv + (row0 + rrow) * ld + h * DH + 4 * g;        // row r of this head: query r (dQ), key r (dK, dV)
#pragma unroll 4
    for (int ct = 0; ct < NCT; ++ct) {
        const f32x4 dq = mfma16(lds_tr(img0 + toff + ct * 32), sT);    // dQ^T = K^T dS^T
        const f32x4 dk = mfma16(lds_tr(img1 + toff + ct * 32), sN);    // dK^T = Q^T dS
        if (wr) { st4(gq + ct * 16, dq); st4(gq + d + ct * 16, dk); }
    }
    __syncthreads();                                           // K's image has been read
    stage16<DH>(img0, dout, d, S, lane);
    __syncthreads();
#pragma unroll 8
    for (int ct = 0; ct < NCT; ++ct) {
        const f32x4 dv = mfma16(lds_tr(img0 + toff + ct * 32), pN);    // dV^T = dO^T P
        if (wr) st4(gq + 2 * d + ct * 16, dv);
    }
}

bool wide_attn_bighead_dim(int dh) { return dh == 256 || dh == 512; }
bool wide_attn_bighead_supported(int S, int dh) { return S >= 1 && S <= WIDE_ATTN_BIGHEAD_MAX_S && wide_attn_bighead_dim(dh); }

template <int DH>
static int launch_bighead(const WideAttnParams& p, bool bwd, hipStream_t st) {
    constexpr int RS = DH * 2 + 32;
    const size_t lds = (size_t)(bwd ? 2 : 1) * BGH_NW * BGH_SP * RS;
    static_assert((size_t)2 * BGH_NW * BGH_SP * RS <= 160 * 1024, "LDS budget");
    static bool attr[2] = {false, false};
    if (!attr[bwd]) {
        const void* fn = bwd ? reinterpret_cast<const void*>(&wide_attn_bighead_bwd_kernel<DH>) : reinterpret_cast<const void*>(&wide_attn_bighead_fwd_kernel<DH>);
        EGX_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr[bwd] = true;
    }
    const dim3 grid(cdiv(p.B * p.H, BGH_NW));
    timing_begin(bwd ? TIMER_WIDE_ATTN_BWD : TIMER_WIDE_ATTN_FWD, st);
    if (bwd) hipLaunchKernelGGL(wide_attn_bighead_bwd_kernel<DH>, grid, dim3(BGH_NTH), lds, st, p);
    else hipLaunchKernelGGL(wide_attn_bighead_fwd_kernel<DH>, grid, dim3(BGH_NTH), lds, st, p);
    timing_end(bwd ? TIMER_WIDE_ATTN_BWD : TIMER_WIDE_ATTN_FWD, st);
    EGX_LAUNCH_CHECK();
    return 0;
}

// the caller (dispatch_attn, wide_attn.hip) has checked the pointers, d % H and d % 8
int wide_attn_bighead(const WideAttnParams& p, bool bwd, hipStream_t st) {
    const int dh = p.d / p.H;
    EGX_CHECK(wide_attn_bighead_supported(p.S, dh), "wide attention: head dim 256 / 512 serves S <= %d (got S=%d, head dim %d)", WIDE_ATTN_BIGHEAD_MAX_S, p.S, dh);
    EGX_CHECK((long long)p.B * p.H <= (1ll << 24), "wide attention: %d x %d (clip, head) pairs in one call", p.B, p.H);      // (bh * 128 + query: 32-bit dropout rows)
    return dh == 256 ? launch_bighead<256>(p, bwd, st) : launch_bighead<512>(p, bwd, st);
}

}  // namespace egx
