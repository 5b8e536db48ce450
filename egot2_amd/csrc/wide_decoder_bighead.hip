// The sequence decoder's attention for LARGE heads: head dim 256 / 512, Sq <= 8 target rows (DA_MAXQ) onto Sk <= 16 keys (DA_BIGHEAD_MAXK). The
// three LTA sequence-decoder models of the reference (HOI/models/lta/lta_models_seqdecoder.py:65-240, lta_models_lta_transfer.py:531-659:
// d_model 2048 with 8 or 4 heads, a memory of 2 or 4 clip rows, 1 .. 3 target tokens). Causal self-attention (Sk = Sq) and cross-attention onto
// the clip's memory rows; DecAttnParams, operand types (bf16, or fp32 for layer 0's self-attention) and dropout keying as dec_attn_kernel
// (wide_decoder.hip), so decoder_fwd_run / decoder_bwd_run and tests/dropmask.py decoder_masks serve both classes unchanged.
//
// dec_attn_kernel keeps one key row of DH floats per lane; at DH = 256 / 512 that is the whole register file. Here no lane holds a row:
//   scores   the 8 x 16 score tile is spread over the wave, lane (j = lane & 15, g = lane >> 4) owns key j and queries g and g + 4. It walks
//            key row j (and, backward, value row j) in 8-element steps straight from memory against the query (dO) rows staged in a wave-
//            private fp32 LDS slice: four running sums per lane whatever DH is. Softmax, dropout, delta and dS are 16-lane reductions.
//   products O = P V, dQ = dS K, dK = dS^T Q and dV = P^T dO run lane = column: 64 columns per pass, DH / 64 passes, 8 (forward) or 8 + 2
//            (backward) accumulators per pass, P and dS broadcast from LDS. Each pass ends in its stores: nothing lives across passes.
// The arithmetic is fp32 FMAs, not MFMA: layer 0's self-attention reads fp32 q / k / v precisely so that its near-saturated scores are NOT
// rounded to bf16 (decoder_layer_fwd), which a bf16 MFMA score tile would undo, and an 8 x 16 tile of at most 128 scores gives a matrix
// unit nothing to amortise. The backward recomputes P (nothing saved). One wave per (clip, head), four to a workgroup; every output element
// is written by exactly one lane, once: no atomics, two runs give the same bits. A wave past the last (clip, head) recomputes the last pair
// and writes nothing (it still meets the barriers); rows >= Sq and keys >= Sk are exact zeros of P / dS and are never written.
#include "dec_attn.h"

namespace egx {

namespace {

constexpr int DAB_NW = 4, DAB_NP = DA_MAXQ * DA_BIGHEAD_MAXK;       // waves per workgroup; entries of a wave's P (dS) tile

template <int DH, bool BWD>
constexpr int dab_wave_floats() { return (BWD ? 2 : 1) * (DA_MAXQ * (DH + 4) + DAB_NP); }      // Q (| dO) rows, padded by 4 floats, and P (| dS)

__device__ __forceinline__ float grp16_max(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float grp16_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float dot8(const float* __restrict__ s, const float (&x)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + 4);
    return ((a.x * x[0] + a.y * x[1]) + (a.z * x[2] + a.w * x[3])) + ((b.x * x[4] + b.y * x[5]) + (b.z * x[6] + b.w * x[7]));
}

template <int DH, bool BWD, bool F32>
__global__ __launch_bounds__(64 * DAB_NW) void dec_attn_bighead_kernel(DecAttnParams p) {
    const uint64_t dkey = p.drop_thresh ? resolve_key(p.drop_key) : 0ull;
    constexpr int QS = DH + 4, CH = DH / 8, MK = DA_BIGHEAD_MAXK;
    extern __shared__ __attribute__((aligned(16))) float dab_sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int npair = p.B * p.H, pair = blockIdx.x * DAB_NW + wave;
    const bool active = pair < npair;
    const int bh = active ? pair : npair - 1, b = bh / p.H, h = bh % p.H;
    const int Sq = p.Sq, Sk = p.Sk;
    float* sQ = dab_sm + wave * dab_wave_floats<DH, BWD>();
    float* sG = sQ + DA_MAXQ * QS;                                  // backward only
    float* sP = sQ + (BWD ? 2 : 1) * DA_MAXQ * QS;                  // probabilities after dropout
    float* sD = sP + DAB_NP;                                        // dS (backward only)
    const size_t q0 = (size_t)b * Sq, k0 = (size_t)b * Sk;          // the clip's first query / key row
    // the Sq query (and dO) rows -> LDS as fp32
    for (int i = lane; i < Sq * CH; i += 64) {
        const int r = i / CH, c = (i - r * CH) * 8;
        float t8[8];
        load8<F32>(p.q, (q0 + r) * p.ldq + h * DH + c, t8);
        *reinterpret_cast<float4*>(sQ + r * QS + c) = make_float4(t8[0], t8[1], t8[2], t8[3]);
        *reinterpret_cast<float4*>(sQ + r * QS + c + 4) = make_float4(t8[4], t8[5], t8[6], t8[7]);
        if constexpr (BWD) {
            load8<false>(p.d_o, (q0 + r) * p.ldo + h * DH + c, t8);
            *reinterpret_cast<float4*>(sG + r * QS + c) = make_float4(t8[0], t8[1], t8[2], t8[3]);
            *reinterpret_cast<float4*>(sG + r * QS + c + 4) = make_float4(t8[4], t8[5], t8[6], t8[7]);
        }
    }
    __syncthreads();
    {   // scores (and dP) of key j against queries g and g + 4
        const int j = lane & 15, g = lane >> 4;
        const int i0 = g < Sq ? g : 0, i1 = g + 4 < Sq ? g + 4 : 0;         // rows >= Sq read row 0: finite, masked below, never written
        const size_t krow = (k0 + (j < Sk ? j : 0)) * p.ldk + h * DH, vrow = (k0 + (j < Sk ? j : 0)) * p.ldv + h * DH;
        float s[2] = {0.f, 0.f}, dp[2] = {0.f, 0.f};
#pragma unroll 4
        for (int c = 0; c < DH; c += 8) {
            float x8[8];
            load8<F32>(p.k, krow + c, x8);
            s[0] += dot8(sQ + i0 * QS + c, x8);
            s[1] += dot8(sQ + i1 * QS + c, x8);
            if constexpr (BWD) {
                load8<F32>(p.v, vrow + c, x8);
                dp[0] += dot8(sG + i0 * QS + c, x8);
                dp[1] += dot8(sG + i1 * QS + c, x8);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = g + 4 * u;
            const bool live = i < Sq && j < Sk && !(p.causal && j > i);
            const float sc = live ? s[u] * p.scale : -INFINITY;
            const float m = grp16_max(sc);
            const float e = live ? __expf(sc - m) : 0.f;
            const float sum = grp16_sum(e);
            const float prob = live ? e / sum : 0.f;
            float mask = 1.f;
            if (p.drop_thresh) mask = drop_scale(dkey, (uint32_t)(bh * DA_MAXQ + i), (uint32_t)j, p.drop_thresh, p.drop_inv);
            sP[i * MK + j] = prob * mask;
            if constexpr (BWD) {
                const float dm = live ? dp[u] * mask : 0.f;
                const float delta = grp16_sum(prob * dm);
                sD[i * MK + j] = live ? prob * (dm - delta) * p.scale : 0.f;
            }
        }
    }
    __syncthreads();
    if constexpr (!BWD) {
        // lane = column: O[i][c] = sum_j P[i][j] V[j][c]
        for (int c = lane; c < DH; c += 64) {
            float acc[DA_MAXQ];
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i) acc[i] = 0.f;
            const size_t v0 = k0 * p.ldv + h * DH + c;
            for (int j = 0; j < Sk; ++j) {
                const float vv = load1<F32>(p.v, v0 + (size_t)j * p.ldv);
#pragma unroll
                for (int i = 0; i < DA_MAXQ; ++i) acc[i] += sP[i * MK + j] * vv;
            }
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i)
                if (active && i < Sq) p.o[(q0 + i) * p.ldo + h * DH + c] = f2bf(acc[i]);
        }
    } else {
        // lane = column: dQ[i][c] = sum_j dS[i][j] K[j][c]; dK[j][c] = sum_i dS[i][j] Q[i][c]; dV[j][c] = sum_i P[i][j] dO[i][c]
        for (int c = lane; c < DH; c += 64) {
            float accq[DA_MAXQ], qc[DA_MAXQ], gc[DA_MAXQ];
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i) {
                accq[i] = 0.f;
                qc[i] = i < Sq ? sQ[i * QS + c] : 0.f;
                gc[i] = i < Sq ? sG[i * QS + c] : 0.f;
            }
            const size_t kc = k0 * p.ldk + h * DH + c, vc = k0 * p.ldv + h * DH + c;
            for (int j = 0; j < Sk; ++j) {
                const float kk = load1<F32>(p.k, kc + (size_t)j * p.ldk);
                float ak = 0.f, av = 0.f;
#pragma unroll
                for (int i = 0; i < DA_MAXQ; ++i) {
                    const float dsv = sD[i * MK + j];
                    accq[i] += dsv * kk;
                    ak += dsv * qc[i];
                    av += sP[i * MK + j] * gc[i];
                }
                if (active) {
                    store1<F32>(p.dk, kc + (size_t)j * p.ldk, ak);
                    store1<F32>(p.dv, vc + (size_t)j * p.ldv, av);
                }
            }
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i)
                if (active && i < Sq) store1<F32>(p.dq, (q0 + i) * p.ldq + h * DH + c, accq[i]);
        }
    }
}

template <int DH, bool BWD, bool F32>
int launch_dab(const DecAttnParams& p, hipStream_t st) {
    constexpr size_t lds = (size_t)DAB_NW * dab_wave_floats<DH, BWD>() * sizeof(float);
    static_assert(lds <= 160 * 1024, "LDS budget");
    static bool attr = false;
    if (!attr) {
        EGX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_attn_bighead_kernel<DH, BWD, F32>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr = true;
    }
    hipLaunchKernelGGL((dec_attn_bighead_kernel<DH, BWD, F32>), dim3(cdiv(p.B * p.H, DAB_NW)), dim3(64 * DAB_NW), lds, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}
template <int DH>
int launch_dab_dh(const DecAttnParams& p, bool f32, bool bwd, hipStream_t st) {
    if (bwd) return f32 ? launch_dab<DH, true, true>(p, st) : launch_dab<DH, true, false>(p, st);
    return f32 ? launch_dab<DH, false, true>(p, st) : launch_dab<DH, false, false>(p, st);
}

bool al16(const void* x) { return ((uintptr_t)x & 15) == 0; }

}  // namespace

bool dec_attn_bighead_dim(int dh) { return dh == 256 || dh == 512; }

int dec_attn_bighead(const DecAttnParams& p, int dh, bool f32, bool bwd, const char* who, hipStream_t st) {
    EGX_CHECK(dec_attn_bighead_dim(dh), "%s: head dim %d is not of the big-head class (256 / 512)", who, dh);
    EGX_CHECK(p.Sq >= 1 && p.Sq <= DA_MAXQ, "%s: head dim 256 / 512 serves Sq <= %d target rows (got Sq=%d, head dim %d)", who, DA_MAXQ, p.Sq, dh);
    EGX_CHECK(p.Sk >= 1 && p.Sk <= DA_BIGHEAD_MAXK, "%s: head dim 256 / 512 serves Sk <= %d keys (got Sk=%d, head dim %d)", who, DA_BIGHEAD_MAXK, p.Sk, dh);
    EGX_CHECK(!p.causal || p.Sk == p.Sq, "%s: causal self-attention has Sk = Sq (got Sq=%d, Sk=%d)", who, p.Sq, p.Sk);
    EGX_CHECK(!p.mtab && !p.clips, "%s: ragged memories serve head dim 32 / 64 only (head dim %d runs uniform batches)", who, dh);
    EGX_CHECK(p.B >= 1 && p.H >= 1 && (long long)p.B * p.H <= (1ll << 24), "%s: %d x %d (clip, head) pairs in one call", who, p.B, p.H);   // (bh * 8 + query: 32-bit dropout rows)
    EGX_CHECK(p.q && p.k && p.v && (bwd ? p.d_o && p.dq && p.dk && p.dv : p.o != nullptr), "%s: null pointer argument", who);
    const int w = p.H * dh;
    EGX_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldv % 8 == 0 && p.ldo % 8 == 0 && p.ldq >= w && p.ldk >= w && p.ldv >= w && p.ldo >= w,
              "%s: ldq = %d, ldk = %d, ldv = %d, ldo = %d (multiples of 8, >= H * head dim = %d)", who, p.ldq, p.ldk, p.ldv, p.ldo, w);
    EGX_CHECK(al16(p.q) && al16(p.k) && al16(p.v) && al16(p.o) && al16(p.d_o) && al16(p.dq) && al16(p.dk) && al16(p.dv), "%s: pointers must be 16-byte aligned", who);
    return dh == 256 ? launch_dab_dh<256>(p, f32, bwd, st) : launch_dab_dh<512>(p, f32, bwd, st);
}

}  // namespace egx
