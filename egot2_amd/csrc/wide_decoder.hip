// The EgoT2-g sequence decoder + vocabulary head as ONE call per direction:
// decode() of HHI/models/multitask/task_prompt_model.py:260-269 and HOI/models/multitask/video_model_builder.py:150-159 —
// `embedding(y) * sqrt(d)` + positional encoding -> nn.TransformerDecoder of CustomDecoderLayer (post-LN: causal
// self-attention over the 2..8 target tokens, cross-attention onto the S <= 1024 memory tokens of the clip, ReLU FFN) -> `fc`.
//
// Round 2 composed it from ~40 autograd functions per layer (60 small fp32 GEMMs, 75 zero-fills and 41 copies per step:
// launch-bound, 60 % of the EgoT2-g step). Here the whole stack is orchestrated in C++ like the wide encoder
// (wide_host.hip): all B * sy target rows go through the bf16 MFMA GEMMs with fused epilogues (bias, ReLU, dropout,
// residual, column sums), LayerNorms through the row kernels with bf16 side outputs, the two tiny attentions through a
// register-resident kernel (one wave per (clip, head)), every gradient accumulates into ONE caller-provided flat buffer
// that the first memset zeroes, and the split-K slabs of all weight gradients are summed by one launch at the end.
// Supported: compute = bf16, d_model a multiple of 128 in [256, 1024], head dim 32 or 64, sy <= 8, S <= 1024 (one wave per (clip, head) up to 64 memory tokens, a chunked four-wave kernel beyond),
// or head dim 256 / 512 with d_model <= 2048, sy <= 8, S <= 16 (wide_decoder_bighead.hip; the cached step's big-head self-attention below); anything else
// stays on the composed path (egot2_amd/decoder.py).
#include <string.h>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/egot2x.h"
#include "common.h"
#include "kernels.h"
#include "wide.h"
#include "wide_run.h"
#include "dec_attn.h"
#include "fused.h"      // (upload_words: the ragged batch table)

namespace egx {

namespace {

// One wave per (clip, head), four per workgroup. Lane j holds key row j (and, in the backward, value row j) in registers,
// lane c holds column c of V (forward) / of K and dO (backward); the Sq <= 8 query rows and the probabilities go through a
// per-wave LDS slice as broadcast reads. Probabilities are recomputed in the backward (nothing saved).
// RAGGED (ragged memories, bf16 operands): wave (i, h) serves clip p.clips[i] with its own memory rows [mtab[2c], + mtab[2c + 1]); its query / output
// rows and its dropout rows are those of the clip's batch position, as in a uniform batch. A flag on the kernel template, so that the uniform
// kernels keep their code: see the note at wide_attn_fwd_kernel (wide_attn.hip).
template <int DH, bool BWD, bool F32, bool RAGGED>
__global__ __launch_bounds__(256) void dec_attn_kernel(DecAttnParams p) {
    const uint64_t dkey = p.drop_thresh ? resolve_key(p.drop_key) : 0ull;
    __shared__ float sQ[4][DA_MAXQ][DH];        // query rows (fp32)
    __shared__ float sG[4][DA_MAXQ][DH];        // dO rows (backward)
    __shared__ float sP[4][DA_MAXQ][64];        // probabilities after dropout
    __shared__ float sD[4][DA_MAXQ][64];        // dS (backward)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wi = blockIdx.x * 4 + wave;
    if (wi >= p.B * p.H) return;                // (no barrier below: every wave works alone)
    const int b = RAGGED ? p.clips[wi / p.H] : wi / p.H, h = wi % p.H, bh = RAGGED ? b * p.H + h : wi;      // bh: the dropout rows
    const int Sq = p.Sq, Sk = RAGGED ? p.mtab[2 * b + 1] : p.Sk;
    const size_t m0 = RAGGED ? (size_t)p.mtab[2 * b] : (size_t)b * Sk;                                      // the clip's first memory row
    const bool kv_lane = lane < Sk;
    // key row of this lane
    float kr[DH], vr[BWD ? DH : 1];
    {
        const size_t krow = (m0 + (kv_lane ? lane : 0)) * p.ldk + h * DH;
#pragma unroll
        for (int c = 0; c < DH; c += 8) {
            float t8[8];
            load8<F32>(p.k, krow + c, t8);
#pragma unroll
            for (int e = 0; e < 8; ++e) kr[c + e] = t8[e];
        }
        if constexpr (BWD) {
            const size_t vrow = (m0 + (kv_lane ? lane : 0)) * p.ldv + h * DH;
#pragma unroll
            for (int c = 0; c < DH; c += 8) {
                float t8[8];
                load8<F32>(p.v, vrow + c, t8);
#pragma unroll
                for (int e = 0; e < 8; ++e) vr[c + e] = t8[e];
            }
        }
    }
    // query (and dO) rows -> LDS
    for (int i = lane; i < Sq * DH; i += 64) {
        const int r = i / DH, c = i - r * DH;
        sQ[wave][r][c] = load1<F32>(p.q, ((size_t)b * Sq + r) * p.ldq + h * DH + c);
        if constexpr (BWD) sG[wave][r][c] = bf1(p.d_o[((size_t)b * Sq + r) * p.ldo + h * DH + c]);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float ds_reg[BWD ? DA_MAXQ : 1];            // dS[i][lane]
#pragma unroll
    for (int i = 0; i < DA_MAXQ; ++i) {         // (static indices: a runtime-indexed register array would live in scratch)
        if (i >= Sq) break;
        const bool live = kv_lane && !(p.causal && lane > i);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < DH; c += 4) {
            const float4 qv = *reinterpret_cast<const float4*>(&sQ[wave][i][c]);
            s += (qv.x * kr[c] + qv.y * kr[c + 1]) + (qv.z * kr[c + 2] + qv.w * kr[c + 3]);
        }
        s = live ? s * p.scale : -INFINITY;
        const float m = wave_max(s);
        const float e = live ? __expf(s - m) : 0.f;
        const float prob = e / wave_sum(e);
        float mask = 1.f;
        if (p.drop_thresh) mask = drop_scale(dkey, (uint32_t)(bh * DA_MAXQ + i), (uint32_t)lane, p.drop_thresh, p.drop_inv);
        sP[wave][i][lane] = prob * mask;
        if constexpr (BWD) {
            float dp = 0.f;
#pragma unroll
            for (int c = 0; c < DH; c += 4) {
                const float4 gv = *reinterpret_cast<const float4*>(&sG[wave][i][c]);
                dp += (gv.x * vr[c] + gv.y * vr[c + 1]) + (gv.z * vr[c + 2] + gv.w * vr[c + 3]);
            }
            dp = live ? dp * mask : 0.f;
            const float delta = wave_sum(prob * dp);
            const float dsv = live ? prob * (dp - delta) * p.scale : 0.f;
            ds_reg[i] = dsv;
            sD[wave][i][lane] = dsv;
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (!BWD) {
        // lane c: O[i][c] = sum_j P[i][j] V[j][c]
        if (lane < DH) {
            float acc[DA_MAXQ];
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i) acc[i] = 0.f;
            const size_t v0 = m0 * p.ldv + h * DH + lane;
            for (int j = 0; j < Sk; ++j) {
                const float vv = load1<F32>(p.v, v0 + (size_t)j * p.ldv);
#pragma unroll
                for (int i = 0; i < DA_MAXQ; ++i)
                    if (i < Sq) acc[i] += sP[wave][i][j] * vv;
            }
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i)
                if (i < Sq) p.o[((size_t)b * Sq + i) * p.ldo + h * DH + lane] = f2bf(acc[i]);
        }
    } else {
        // lane j: dK[j][:] = sum_i dS[i][j] Q[i][:]  (row store)
        if (kv_lane) {
            const size_t dk0 = (m0 + lane) * p.ldk + h * DH;
#pragma unroll
            for (int c = 0; c < DH; c += 8) {
                float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int i = 0; i < DA_MAXQ; ++i) {
                    if (i >= Sq) break;
                    const float4 q0 = *reinterpret_cast<const float4*>(&sQ[wave][i][c]);
                    const float4 q1 = *reinterpret_cast<const float4*>(&sQ[wave][i][c + 4]);
                    const float dsv = ds_reg[i];
                    a[0] += dsv * q0.x; a[1] += dsv * q0.y; a[2] += dsv * q0.z; a[3] += dsv * q0.w;
                    a[4] += dsv * q1.x; a[5] += dsv * q1.y; a[6] += dsv * q1.z; a[7] += dsv * q1.w;
                }
                store8<F32>(p.dk, dk0 + c, a);
            }
        }
        // lane c: dQ[i][c] = sum_j dS[i][j] K[j][c];  dV[j][c] = sum_i P[i][j] dO[i][c]
        if (lane < DH) {
            float accq[DA_MAXQ], go[DA_MAXQ];
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i) { accq[i] = 0.f; go[i] = i < Sq ? sG[wave][i][lane] : 0.f; }
            const size_t k0 = m0 * p.ldk + h * DH + lane, dv0 = m0 * p.ldv + h * DH + lane;
            for (int j = 0; j < Sk; ++j) {
                const float kk = load1<F32>(p.k, k0 + (size_t)j * p.ldk);
                float av = 0.f;
#pragma unroll
                for (int i = 0; i < DA_MAXQ; ++i)
                    if (i < Sq) { accq[i] += sD[wave][i][j] * kk; av += sP[wave][i][j] * go[i]; }
                store1<F32>(p.dv, dv0 + (size_t)j * p.ldv, av);
            }
#pragma unroll
            for (int i = 0; i < DA_MAXQ; ++i)
                if (i < Sq) store1<F32>(p.dq, ((size_t)b * Sq + i) * p.ldq + h * DH + lane, accq[i]);
        }
    }
}

// Cross-attention onto a memory of more than 64 tokens (EgoT2-g HHI on real-length TTM / ASD sequences: up to 3 x 150): one
// workgroup of four waves per (clip, head); K and V stream through ONE 64-row LDS buffer (fp32, padded rows) chunk by chunk,
// all Sq x Sk probabilities stay in LDS. bf16 operands and gradients; same dropout keying as dec_attn_kernel.
constexpr int DAL_MAXK = 1024;
template <int DH, bool BWD, bool RAGGED>
__global__ __launch_bounds__(256) void dec_attn_long_kernel(DecAttnParams p) {
    const uint64_t dkey = p.drop_thresh ? resolve_key(p.drop_key) : 0ull;
    constexpr int LDK = DH + 1;
    extern __shared__ float dal_sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (the ragged side divides the unsigned workgroup index, the uniform side the signed one, as each always did)
    const int b = RAGGED ? p.clips[blockIdx.x / p.H] : (int)blockIdx.x / p.H, h = RAGGED ? blockIdx.x % p.H : (int)blockIdx.x % p.H;
    const int bh = RAGGED ? b * p.H + h : blockIdx.x;                                                       // the dropout rows
    const int Sq = p.Sq, Sk = RAGGED ? p.mtab[2 * b + 1] : p.Sk, SKP = (Sk + 63) & ~63;
    const size_t m0 = RAGGED ? (size_t)p.mtab[2 * b] : (size_t)b * Sk;                                      // the clip's first memory row
    float* Cs = dal_sm;                     // K or V chunk [64][DH + 1]
    float* Qs = Cs + 64 * LDK;
    float* Gs = Qs + DA_MAXQ * DH;
    float* Ps = Gs + DA_MAXQ * DH;          // [Sq][SKP]
    float* Ds = Ps + DA_MAXQ * SKP;         // backward only
    const bf16_t* kb = reinterpret_cast<const bf16_t*>(p.k) + m0 * p.ldk + h * DH;
    const bf16_t* vb = reinterpret_cast<const bf16_t*>(p.v) + m0 * p.ldv + h * DH;
    auto stage = [&](const bf16_t* src, int ld, int j0) {
        __syncthreads();
        for (int i = tid; i < 64 * (DH / 8); i += 256) {
            const int j = i / (DH / 8), c = (i - j * (DH / 8)) * 8;
            float t8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (j0 + j < Sk) load8<false>(src, (size_t)(j0 + j) * ld + c, t8);
#pragma unroll
            for (int e = 0; e < 8; ++e) Cs[j * LDK + c + e] = t8[e];
        }
        __syncthreads();
    };
    for (int i = tid; i < Sq * DH; i += 256) {
        const int r = i / DH, c = i - r * DH;
        Qs[i] = load1<false>(p.q, ((size_t)b * Sq + r) * p.ldq + h * DH + c);
        if constexpr (BWD) Gs[i] = bf1(p.d_o[((size_t)b * Sq + r) * p.ldo + h * DH + c]);
    }
    for (int j0 = 0; j0 < Sk; j0 += 64) {          // scores: wave w owns queries w, w + 4; lane = key within the chunk
        stage(kb, p.ldk, j0);
        for (int i = wave; i < Sq; i += 4) {
            float sc = 0.f;
#pragma unroll
            for (int c = 0; c < DH; ++c) sc += Qs[i * DH + c] * Cs[lane * LDK + c];
            Ps[i * SKP + j0 + lane] = j0 + lane < Sk ? sc * p.scale : -INFINITY;
        }
    }
    __syncthreads();
    for (int i = wave; i < Sq; i += 4) {
        float m = -INFINITY;
        for (int j = lane; j < SKP; j += 64) m = fmaxf(m, Ps[i * SKP + j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < SKP; j += 64) { const float e = __expf(Ps[i * SKP + j] - m); Ps[i * SKP + j] = e; sum += e; }
        sum = 1.f / wave_sum(sum);
        for (int j = lane; j < SKP; j += 64) Ps[i * SKP + j] *= sum;
    }
    auto keep = [&](int i, int j) { return p.drop_thresh ? drop_scale(dkey, (uint32_t)(bh * DA_MAXQ + i), (uint32_t)j, p.drop_thresh, p.drop_inv) : 1.f; };
    constexpr int NE = DA_MAXQ * DH / 256;          // (query, column) accumulators per thread: 1 (DH = 32) or 2 (DH = 64)
    float acc[NE];
#pragma unroll
    for (int u = 0; u < NE; ++u) acc[u] = 0.f;
    if constexpr (BWD) {
        for (int j0 = 0; j0 < Sk; j0 += 64) {      // dP = dO V^T
            stage(vb, p.ldv, j0);
            for (int i = wave; i < Sq; i += 4) {
                float dp = 0.f;
#pragma unroll
                for (int c = 0; c < DH; ++c) dp += Gs[i * DH + c] * Cs[lane * LDK + c];
                Ds[i * SKP + j0 + lane] = dp;
            }
        }
        __syncthreads();
        for (int i = wave; i < Sq; i += 4) {
            float delta = 0.f;
            for (int j = lane; j < SKP; j += 64) {
                const float dp = Ds[i * SKP + j] * keep(i, j);
                Ds[i * SKP + j] = dp;
                delta += Ps[i * SKP + j] * dp;
            }
            delta = wave_sum(delta);
            for (int j = lane; j < SKP; j += 64) {
                const float pr = Ps[i * SKP + j];
                Ds[i * SKP + j] = pr * (Ds[i * SKP + j] - delta) * p.scale;
                Ps[i * SKP + j] = pr * keep(i, j);
            }
        }
        bf16_t* dkb = reinterpret_cast<bf16_t*>(p.dk) + m0 * p.ldk + h * DH;
        bf16_t* dvb = reinterpret_cast<bf16_t*>(p.dv) + m0 * p.ldv + h * DH;
        for (int j0 = 0; j0 < Sk; j0 += 64) {      // dQ += dS K; dK = dS^T Q, dV = P^T dO for the chunk's keys
            stage(kb, p.ldk, j0);
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = tid + u * 256, i = e / DH, c = e - i * DH;
                if (i < Sq) {
                    float a = 0.f;
                    for (int j = 0; j < 64; ++j) a += Ds[i * SKP + j0 + j] * Cs[j * LDK + c];
                    acc[u] += a;
                }
            }
            for (int e = tid; e < 64 * (DH / 8); e += 256) {
                const int j = e / (DH / 8), c = (e - j * (DH / 8)) * 8;
                if (j0 + j < Sk) {
                    float ak[8] = {0, 0, 0, 0, 0, 0, 0, 0}, av[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    for (int i = 0; i < Sq; ++i) {
                        const float dsv = Ds[i * SKP + j0 + j], pv = Ps[i * SKP + j0 + j];
#pragma unroll
                        for (int x = 0; x < 8; ++x) { ak[x] += dsv * Qs[i * DH + c + x]; av[x] += pv * Gs[i * DH + c + x]; }
                    }
                    store8<false>(dkb, (size_t)(j0 + j) * p.ldk + c, ak);
                    store8<false>(dvb, (size_t)(j0 + j) * p.ldv + c, av);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int e = tid + u * 256, i = e / DH, c = e - i * DH;
            if (i < Sq) store1<false>(p.dq, ((size_t)b * Sq + i) * p.ldq + h * DH + c, acc[u]);
        }
    } else {
        if (p.drop_thresh) {
            for (int i = wave; i < Sq; i += 4)
                for (int j = lane; j < SKP; j += 64) Ps[i * SKP + j] *= keep(i, j);
        }
        for (int j0 = 0; j0 < Sk; j0 += 64) {
            stage(vb, p.ldv, j0);
#pragma unroll
            for (int u = 0; u < NE; ++u) {
                const int e = tid + u * 256, i = e / DH, c = e - i * DH;
                if (i < Sq) {
                    float a = 0.f;
                    for (int j = 0; j < 64; ++j) a += Ps[i * SKP + j0 + j] * Cs[j * LDK + c];
                    acc[u] += a;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NE; ++u) {
            const int e = tid + u * 256, i = e / DH, c = e - i * DH;
            if (i < Sq) p.o[((size_t)b * Sq + i) * p.ldo + h * DH + c] = f2bf(acc[u]);
        }
    }
}
template <int DH, bool BWD, bool RAGGED>
int dec_attn_long(const DecAttnParams& p, hipStream_t st) {
    // Cs, Qs, Gs, Ps and Ds. The ragged forward does not reserve Ds (backward only), which would cut the workgroups per CU at long memories; the
    // uniform forward still does.
    constexpr int NPS = RAGGED && !BWD ? 1 : 2;
    auto lds = [](int Sk) { return ((size_t)64 * (DH + 1) + (size_t)2 * DA_MAXQ * DH + (size_t)NPS * DA_MAXQ * ((Sk + 63) & ~63)) * sizeof(float); };
    static bool attr = false;
    if (!attr) {
        EGX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_attn_long_kernel<DH, BWD, RAGGED>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds(DAL_MAXK)));
        attr = true;
    }
    hipLaunchKernelGGL((dec_attn_long_kernel<DH, BWD, RAGGED>), dim3(p.B * p.H), dim3(256), lds(p.Sk), st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

template <bool BWD>
int dec_attn(DecAttnParams p, int dh, bool f32, hipStream_t st) {
    p.scale = 1.f / sqrtf((float)dh);
    if (dec_attn_bighead_dim(dh)) return dec_attn_bighead(p, dh, f32, BWD, "decoder attention", st);       // (wide_decoder_bighead.hip)
    if (p.Sk > DA_MAXK) {
        EGX_CHECK(!f32 && !p.causal && (dh == 32 || dh == 64), "decoder attention: a memory of %d tokens needs bf16 operands and head dim 32 / 64", p.Sk);
        return dh == 64 ? dec_attn_long<64, BWD, false>(p, st) : dec_attn_long<32, BWD, false>(p, st);
    }
    const dim3 grid(cdiv(p.B * p.H, 4)), block(256);
    if (dh == 64 && !f32) hipLaunchKernelGGL((dec_attn_kernel<64, BWD, false, false>), grid, block, 0, st, p);
    else if (dh == 32 && !f32) hipLaunchKernelGGL((dec_attn_kernel<32, BWD, false, false>), grid, block, 0, st, p);
    else if (dh == 64) hipLaunchKernelGGL((dec_attn_kernel<64, BWD, true, false>), grid, block, 0, st, p);
    else if (dh == 32) hipLaunchKernelGGL((dec_attn_kernel<32, BWD, true, false>), grid, block, 0, st, p);
    else EGX_CHECK(false, "decoder attention: head dim %d (32 or 64)", dh);
    EGX_LAUNCH_CHECK();
    return 0;
}

// ---- ragged memories (egx_decoder_ragged_fwd, egx_decoder_ragged_train_fwd / egx_decoder_ragged_bwd) ----
// dec_attn_kernel (bf16 operands) and dec_attn_long_kernel with RAGGED set: forward with dropout on the probabilities (none at drop_thresh 0: the
// inference call) and backward (dq for the clip's Sq target rows, dk / dv for the clip's own memory rows, written packed: every memory row
// belongs to one clip). One launch per kernel class: p.clips / p.B the clips of the class, p.Sk their longest memory.
template <bool BWD>
int dec_attn_ragged_train(DecAttnParams p, int dh, bool long_class, hipStream_t st) {
    EGX_CHECK(dh == 32 || dh == 64, "decoder attention: head dim %d (32 or 64)", dh);
    EGX_CHECK(!p.causal && p.Sk >= 1 && p.Sk <= DAL_MAXK && p.mtab && p.clips, "decoder attention (ragged training): bad arguments");
    if (p.B <= 0) return 0;
    p.scale = 1.f / sqrtf((float)dh);
    if (long_class) return dh == 64 ? dec_attn_long<64, BWD, true>(p, st) : dec_attn_long<32, BWD, true>(p, st);
    EGX_CHECK(p.Sk <= DA_MAXK, "decoder attention (ragged): short class with Sk = %d", p.Sk);
    const dim3 grid(cdiv(p.B * p.H, 4)), block(256);
    if (dh == 64) hipLaunchKernelGGL((dec_attn_kernel<64, BWD, false, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((dec_attn_kernel<32, BWD, false, true>), grid, block, 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

// ---- the cross-attention weights as an output (egx_cross_attention_weights, egx_decoder_cross_weights, egx_decoder_generate_attn) ----
// What CustomDecoderLayer._mha_block asks nn.MultiheadAttention for with need_weights=True (HHI/models/multitask/task_prompt_model.py:163-172,
// HOI/models/multitask/video_model_builder.py:20-30, HOI/models/lta/lta_models_seqdecoder.py:30-39): the head-averaged probabilities
//   w[b, i, j] = (1 / H) sum_h softmax_j(q[b, i, h, :] . k[b, j, h, :] / sqrt(DH)).
// One 256-thread workgroup per (clip, query row), a loop over the heads in order 0 .. H - 1. Thread t owns keys t, t + 256, t + 512, t + 768
// (Sk <= 1024: four accumulators); it reads its key's head slice with 16-byte loads and the query slice from LDS as broadcast reads. Per head
// a block maximum and a block sum: the wave's xor tree, then the four wave partials in wave order. Scores, max, exp, sum and the
// normalisation are fp32; the head sum runs in head order and is multiplied by 1 / H once. No atomics: a clip's rows have the same bits
// wherever the clip sits in the batch. Ragged (mtab): clip b's S_b = clamp(mtab[2b + 1], 0, Sk) keys are rows [mtab[2b], + S_b) of k;
// entries j >= S_b of the Sk written ones are exact zeros.
struct CrossWParams {
    const void* q; const void* k; int ldq, ldk;     // rows b * Sq + i / b * Sk + j (or the table's); head h at columns h * DH
    const int* mtab;                                // DEVICE int[B][2] or null
    float* out; int ldo;                            // row b * Sq + i, Sk entries written
    int B, H, Sq, Sk;
    float scale, inv_h;
};
constexpr int CW_MAXK = 1024, CW_THREADS = 256, CW_KEYS = CW_MAXK / CW_THREADS;

template <int DH, bool F32>
__global__ __launch_bounds__(CW_THREADS) void dec_cross_weights_kernel(CrossWParams p) {
    __shared__ __align__(16) float sQ[DH];      // (read as float4)
    __shared__ float sMax[4], sSum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x / p.Sq, i = blockIdx.x - b * p.Sq;
    int Sb = p.Sk;
    size_t m0 = (size_t)b * p.Sk;
    if (p.mtab) {
        const int first = p.mtab[2 * b], rows = p.mtab[2 * b + 1];
        Sb = rows < 0 ? 0 : (rows > p.Sk ? p.Sk : rows);
        m0 = (size_t)(first < 0 ? 0 : first);
    }
    const size_t qrow = ((size_t)b * p.Sq + i) * p.ldq;
    float acc[CW_KEYS];
#pragma unroll
    for (int c = 0; c < CW_KEYS; ++c) acc[c] = 0.f;
    for (int h = 0; h < p.H; ++h) {             // (uniform trip count: every barrier below is reached by all 256 threads)
        if (t < DH) sQ[t] = load1<F32>(p.q, qrow + h * DH + t);
        __syncthreads();
        float s[CW_KEYS];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < CW_KEYS; ++c) {
            const int j = t + c * CW_THREADS;
            s[c] = -INFINITY;
            if (j < Sb) {
                const size_t krow = (m0 + j) * p.ldk + h * DH;
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
                for (int e = 0; e < DH; e += 8) {
                    float k8[8];
                    load8<F32>(p.k, krow + e, k8);
                    const float4 q0 = *reinterpret_cast<const float4*>(&sQ[e]);
                    const float4 q1 = *reinterpret_cast<const float4*>(&sQ[e + 4]);
                    a0 += q0.x * k8[0] + q1.x * k8[4]; a1 += q0.y * k8[1] + q1.y * k8[5];
                    a2 += q0.z * k8[2] + q1.z * k8[6]; a3 += q0.w * k8[3] + q1.w * k8[7];
                }
                s[c] = ((a0 + a1) + (a2 + a3)) * p.scale;
            }
            m = fmaxf(m, s[c]);
        }
        m = wave_max(m);
        if (lane == 0) sMax[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3]));
        float e[CW_KEYS];
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CW_KEYS; ++c) {
            e[c] = t + c * CW_THREADS < Sb ? __expf(s[c] - m) : 0.f;
            sum += e[c];
        }
        sum = wave_sum(sum);
        if (lane == 0) sSum[wave] = sum;
        __syncthreads();
        sum = ((sSum[0] + sSum[1]) + sSum[2]) + sSum[3];     // wave order
#pragma unroll
        for (int c = 0; c < CW_KEYS; ++c) acc[c] += e[c] / sum;     // (Sb = 0: 0 / 0 is never stored)
    }
    float* orow = p.out + ((size_t)b * p.Sq + i) * p.ldo;
#pragma unroll
    for (int c = 0; c < CW_KEYS; ++c) {
        const int j = t + c * CW_THREADS;
        if (j < p.Sk) orow[j] = j < Sb ? acc[c] * p.inv_h : 0.f;
    }
}

// host checks first (no device work on a refusal), then one launch
int cross_weights(CrossWParams p, int dh, bool f32, hipStream_t st) {
    EGX_CHECK(p.q && p.k && p.out, "egx_cross_attention_weights: null pointer argument");
    EGX_CHECK(dh == 16 || dh == 32 || dh == 64 || dh == 128, "egx_cross_attention_weights: head dim %d (16, 32, 64 or 128)", dh);
    EGX_CHECK(p.Sk >= 1 && p.Sk <= CW_MAXK, "egx_cross_attention_weights: Sk = %d (1..%d)", p.Sk, CW_MAXK);
    EGX_CHECK(p.Sq >= 1 && p.H >= 1 && p.B >= 0, "egx_cross_attention_weights: B = %d, H = %d, Sq = %d", p.B, p.H, p.Sq);
    EGX_CHECK(p.ldo >= p.Sk, "egx_cross_attention_weights: ldo = %d < Sk = %d", p.ldo, p.Sk);
    EGX_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldq >= p.H * dh && p.ldk >= p.H * dh,
              "egx_cross_attention_weights: ldq = %d, ldk = %d (multiples of 8 elements, at least H * dh = %d)", p.ldq, p.ldk, p.H * dh);
    EGX_CHECK(((uintptr_t)p.q | (uintptr_t)p.k) % 16 == 0, "egx_cross_attention_weights: q and k must be 16-byte aligned");
    EGX_CHECK((long long)p.B * p.Sq <= 0x7fffffffLL, "egx_cross_attention_weights: B * Sq = %lld workgroups", (long long)p.B * p.Sq);
    if (p.B == 0) return 0;
    p.scale = 1.f / sqrtf((float)dh); p.inv_h = 1.f / (float)p.H;
    const dim3 grid((unsigned)(p.B * p.Sq)), block(CW_THREADS);
#define EGX_CW_LAUNCH(DH_) \
    do { if (f32) hipLaunchKernelGGL((dec_cross_weights_kernel<DH_, true>), grid, block, 0, st, p); \
         else hipLaunchKernelGGL((dec_cross_weights_kernel<DH_, false>), grid, block, 0, st, p); } while (0)
    if (dh == 16) EGX_CW_LAUNCH(16);
    else if (dh == 32) EGX_CW_LAUNCH(32);
    else if (dh == 64) EGX_CW_LAUNCH(64);
    else EGX_CW_LAUNCH(128);
#undef EGX_CW_LAUNCH
    EGX_LAUNCH_CHECK();
    return 0;
}

// x32 / x16 [row] = dropout(emb[tok[row]] * scale + pe[row % sy])
__global__ __launch_bounds__(256) void dec_embed_kernel(const int64_t* __restrict__ tok, const float* __restrict__ emb, const float* __restrict__ pe,
                                                        int pe_stride, float scale, float* __restrict__ x32, bf16_t* __restrict__ x16, int rows,
                                                        int sy, int d, int V, uint64_t key, uint32_t thresh, float inv) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // one float4 each
    if (i >= (size_t)rows * (d / 4)) return;
    const int row = (int)(i / (d / 4)), c = (int)(i % (d / 4)) * 4;
    const int64_t t = tok[row];
    float4 e = make_float4(0, 0, 0, 0);
    if (t >= 0 && t < V) e = *reinterpret_cast<const float4*>(emb + (size_t)t * d + c);
    const float4 pp = *reinterpret_cast<const float4*>(pe + (size_t)(row % sy) * pe_stride + c);
    float o[4] = {e.x * scale + pp.x, e.y * scale + pp.y, e.z * scale + pp.z, e.w * scale + pp.w};
    if (thresh) {
        float ds[4];
        drop_scale4(resolve_key(key), (uint32_t)row, (uint32_t)c, thresh, inv, ds);
        o[0] *= ds[0]; o[1] *= ds[1]; o[2] *= ds[2]; o[3] *= ds[3];
    }
    *reinterpret_cast<float4*>(x32 + (size_t)row * d + c) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint2*>(x16 + (size_t)row * d + c) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
}
// d_emb[v][c] += scale * sum over the rows whose token is v of mask * dy[row][c]: one workgroup per (v, 64 columns), four
// row groups summed through LDS in a fixed order (deterministic; replaces one atomic add per element onto a handful of
// vocabulary rows)
__global__ __launch_bounds__(256) void dec_embed_grad_kernel(const int64_t* __restrict__ tok, const float* __restrict__ dy, float* __restrict__ d_emb,
                                                             float scale, int rows, int d, int V, uint64_t key, uint32_t thresh, float inv) {
    __shared__ float part[4][64];
    const int v = blockIdx.y, lane = threadIdx.x & 63, grp = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    float acc = 0.f;
    if (c < d) {
        for (int row = grp; row < rows; row += 4) {
            if (tok[row] != v) continue;                                 // wave-uniform
            float g = dy[(size_t)row * d + c];
            if (thresh) g *= drop_scale(resolve_key(key), (uint32_t)row, (uint32_t)c, thresh, inv);
            acc += g;
        }
    }
    part[grp][lane] = acc;
    __syncthreads();
    if (grp == 0 && c < d) d_emb[(size_t)v * d + c] += ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) * scale;
}

// Small vocabularies (V <= 64: the EgoT2-g task vocabularies): one workgroup per 64 columns walks ALL rows once, every row's
// gradient is loaded unconditionally (eight rows in flight per wave) and added to the LDS accumulator row of its token; four
// up to 16 waves take a slice of the rows each and are summed in wave order (deterministic). The per-(token, column) kernel above
// scans the token list once per vocabulary entry with a dependent load per match: 43-61 us at B * sy = 512 against 6 here.
constexpr int EMB_VMAX = 64;
__global__ __launch_bounds__(1024) void dec_embed_grad_small_kernel(const int64_t* __restrict__ tok, const float* __restrict__ dy, float* __restrict__ d_emb,
                                                                    float scale, int rows, int d, int V, uint64_t key, uint32_t thresh, float inv) {
    extern __shared__ float acc[];          // [G row groups][V][64], G = blockDim.x / 64 (as many as 64 KB hold, at most 16)
    const int G = blockDim.x >> 6;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    float* mine = acc + (size_t)grp * V * 64;
    for (int v = 0; v < V; ++v) mine[v * 64 + lane] = 0.f;
    const int cc = c < d ? c : d - 1;
    const int per = (rows + G - 1) / G, r0 = grp * per, r1 = r0 + per < rows ? r0 + per : rows;
    for (int row = r0; row < r1; row += 8) {
        float g[8];
        int t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int rr = row + u < r1 ? row + u : r1 - 1;
            g[u] = dy[(size_t)rr * d + cc];
            t[u] = (int)tok[rr];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (row + u >= r1) break;
            float gv = g[u];
            if (thresh) gv *= drop_scale(resolve_key(key), (uint32_t)(row + u), (uint32_t)cc, thresh, inv);
            if (t[u] >= 0 && t[u] < V) mine[t[u] * 64 + lane] += gv;      // lane-private column: no conflict, row order kept
        }
    }
    __syncthreads();
    if (c < d)
        for (int v = grp; v < V; v += G) {
            float sum = 0.f;
            for (int k = 0; k < G; ++k) sum += acc[((size_t)k * V + v) * 64 + lane];     // group order
            d_emb[(size_t)v * d + c] += sum * scale;
        }
}

struct DecW { size_t sa_in, sa_o, q, kv, ca_o, w1, w2; };      // a layer's bf16 weights (ca_in_w as its q and k | v rows)
struct DLayer {
    DecW w, wt;                                                 // W and W^T
    size_t x32, x16, qkv, sa, res1, st1, x1_32, x1_16, q, kv, ca, res2, st2, x2_32, x2_16, hid, res3, st3;
};
struct DPlan {
    int B, sy, S, d, H, dff, L, V;
    size_t Md, Nm;
    size_t zero, mem16, xL32, qkv32, keys;
    DLayer layer[16];
    size_t saved_bytes;
    size_t gA, gB, dres, dattn16, dqkv32, slab_all, slab_all_bytes, lnpart, cspart, cspart_side, rowpart, rowpart_bytes, fcslab, fcslab_bytes, scratch_bytes;
    // operands of the weight-gradient GEMMs: one buffer per (layer, use) — those GEMMs run on a side stream beside the input-gradient
    // chain (decoder_bwd), so the chain must not overwrite an operand while its weight gradient may still be reading it
    struct { size_t dy16[3], dhid16, dqkv16, dq16, dkv16; } g[16];
};

// mem_rows > 0 (ragged memories): the memory is that many packed rows instead of B * S
int make_dplan(const egx_dec_config* c, int B, DPlan& pl, size_t mem_rows = 0) {
    EGX_CHECK(c, "null decoder config");
    EGX_CHECK(c->compute == EGX_BF16, "the fused decoder runs compute = bf16 (the composed path serves the other modes)");
    // head dim 32 / 64: d_model <= 1024, S <= 1024 (dec_attn_kernel, dec_attn_long_kernel); head dim 256 / 512: d_model <= 2048, S <= 16
    // (wide_decoder_bighead.hip)
    const int dh_ = c->n_heads > 0 && c->d_model % c->n_heads == 0 ? c->d_model / c->n_heads : 0;
    const bool big = dec_attn_bighead_dim(dh_);
    EGX_CHECK(c->d_model >= 256 && c->d_model <= (big ? 2048 : 1024) && c->d_model % 128 == 0,
              "fused decoder: d_model = %d (multiples of 128 in [256, 1024]; up to 2048 with head dim 256 / 512)", c->d_model);
    EGX_CHECK(dh_ == 32 || dh_ == 64 || big, "fused decoder: head dim %d (32 or 64; 256 or 512 with S <= %d)", c->n_heads > 0 ? c->d_model / c->n_heads : 0,
              DA_BIGHEAD_MAXK);
    EGX_CHECK(c->d_ff >= 128 && c->d_ff % 128 == 0, "fused decoder: d_ff = %d (multiples of 128)", c->d_ff);
    EGX_CHECK(c->n_layers >= 1 && c->n_layers <= 16, "fused decoder: %d layers (1..16)", c->n_layers);
    EGX_CHECK(c->sy >= 1 && c->sy <= DA_MAXQ && c->S >= 1 && c->S <= DAL_MAXK, "fused decoder: sy = %d (1..%d), S = %d (1..%d)", c->sy, DA_MAXQ, c->S, DAL_MAXK);
    EGX_CHECK(!big || c->S <= DA_BIGHEAD_MAXK, "fused decoder: head dim 256 / 512 serves S <= %d memory rows (got S=%d, head dim %d)", DA_BIGHEAD_MAXK,
              c->S, dh_);
    EGX_CHECK(c->vocab >= 1 && B >= 1, "fused decoder: vocab = %d, B = %d", c->vocab, B);
    memset(&pl, 0, sizeof(pl));
    pl.B = B; pl.sy = c->sy; pl.S = c->S; pl.d = c->d_model; pl.H = c->n_heads; pl.dff = c->d_ff; pl.L = c->n_layers; pl.V = c->vocab;
    pl.Md = (size_t)B * c->sy; pl.Nm = mem_rows ? mem_rows : (size_t)B * c->S;
    const size_t d = pl.d, dff = pl.dff, Md = pl.Md, Nm = pl.Nm;
    size_t cur = 0;
    pl.zero = take(cur, 1024);
    pl.keys = take(cur, (size_t)16 * DROP_KEY_SLOTS * sizeof(uint64_t));
    pl.mem16 = take(cur, Nm * d * 2);
    for (int l = 0; l < pl.L; ++l) {
        DLayer& o = pl.layer[l];
        o.w.sa_in = take(cur, 3 * d * d * 2); o.wt.sa_in = take(cur, 3 * d * d * 2);
        o.w.sa_o = take(cur, d * d * 2); o.wt.sa_o = take(cur, d * d * 2);
        o.w.q = take(cur, d * d * 2); o.wt.q = take(cur, d * d * 2);
        o.w.kv = take(cur, 2 * d * d * 2); o.wt.kv = take(cur, 2 * d * d * 2);
        o.w.ca_o = take(cur, d * d * 2); o.wt.ca_o = take(cur, d * d * 2);
        o.w.w1 = take(cur, dff * d * 2); o.wt.w1 = take(cur, dff * d * 2);
        o.w.w2 = take(cur, dff * d * 2); o.wt.w2 = take(cur, dff * d * 2);
        o.x32 = take(cur, Md * d * 4); o.x16 = take(cur, Md * d * 2);
        o.qkv = take(cur, Md * 3 * d * 2); o.sa = take(cur, Md * d * 2);
        o.res1 = take(cur, Md * d * 4); o.st1 = take(cur, Md * 8);
        o.x1_32 = take(cur, Md * d * 4); o.x1_16 = take(cur, Md * d * 2);
        o.q = take(cur, Md * d * 2); o.kv = take(cur, Nm * 2 * d * 2); o.ca = take(cur, Md * d * 2);
        o.res2 = take(cur, Md * d * 4); o.st2 = take(cur, Md * 8);
        o.x2_32 = take(cur, Md * d * 4); o.x2_16 = take(cur, Md * d * 2);
        o.hid = take(cur, Md * dff * 2);
        o.res3 = take(cur, Md * d * 4); o.st3 = take(cur, Md * 8);
    }
    pl.xL32 = take(cur, Md * d * 4);
    pl.qkv32 = take(cur, Md * 3 * d * 4);
    pl.saved_bytes = cur;

    size_t sc = 0;
    pl.gA = take(sc, Md * d * 4); pl.gB = take(sc, Md * d * 4); pl.dres = take(sc, Md * d * 4);
    pl.dattn16 = take(sc, Md * d * 2); pl.dqkv32 = take(sc, Md * 3 * d * 4);
    for (int l = 0; l < pl.L; ++l) {
        for (int u = 0; u < 3; ++u) pl.g[l].dy16[u] = take(sc, Md * d * 2);
        pl.g[l].dhid16 = take(sc, Md * dff * 2); pl.g[l].dqkv16 = take(sc, Md * 3 * d * 2);
        pl.g[l].dq16 = take(sc, Md * d * 2); pl.g[l].dkv16 = take(sc, Nm * 2 * d * 2);
    }
    pl.slab_all_bytes = pl.L * wide_slab_bytes({{pl.d, pl.dff, Md}, {pl.dff, pl.d, Md}, {pl.d, pl.d, Md}, {pl.d, pl.d, Md}, {pl.d, pl.d, Md},
                                                {3 * pl.d, pl.d, Md}, {2 * pl.d, pl.d, Nm}});
    pl.slab_all = take(sc, pl.slab_all_bytes);
    pl.lnpart = take(sc, wide_ln_bwd_scratch((int)Md, pl.d));
    size_t cs = size_max(wide_colsum_scratch((int)Md, 3 * pl.d), wide_colsum_scratch((int)Nm, 2 * pl.d));
    cs = size_max(cs, wide_ffn_colsum_bytes((int)Md, pl.dff));
    pl.cspart = take(sc, cs);
    pl.cspart_side = take(sc, cs);
    // a partial buffer per deferred row reduction of the backward (wide.h WideRowReduceBatch): per layer three LayerNorm backwards,
    // the lin1 bias sums and three bf16 column sums (self-attention in-projection, cross-attention q and k | v)
    pl.rowpart_bytes = wide_rowpart_bytes(pl.L, 3, (int)Md, pl.d, {cs, cs, cs, cs});
    pl.rowpart = take(sc, pl.rowpart_bytes);
    pl.fcslab_bytes = size_max(gemm_scratch_bytes(2, pl.V, pl.d, (int)Md), gemm_scratch_bytes(1, (int)Md, pl.d, pl.V));
    pl.fcslab_bytes = size_max(pl.fcslab_bytes, size_max(gemm_scratch_bytes(2, 3 * pl.d, pl.d, (int)Md), gemm_scratch_bytes(1, (int)Md, pl.d, 3 * pl.d)));
    pl.fcslab = take(sc, pl.fcslab_bytes);
    pl.scratch_bytes = sc;
    return 0;
}

enum { DS_SELF = 1, DS_SA_OUT = 2, DS_CROSS = 3, DS_CA_OUT = 4, DS_FFN = 5, DS_FFN_OUT = 6, DS_EMBED = 7 };

// The decoder's weight gradients (small TN GEMMs over B * sy target rows, bias column sums) are off the critical path of its
// backward: the input-gradient chain is ~16 dependent launches per layer that each occupy 16-64 CUs. They run on a library-owned
// side stream, forked off the caller's stream by an event after the kernel that produces their operand and joined before the
// slab reduction (works the same under stream capture: the side stream's launches become a parallel branch of the graph).
// EGX_DEC_SIDE=0 keeps everything on the caller's stream. Under stream CAPTURE the fork is not taken either (side_wanted()): as
// branches of a hipGraph the side launches cost more than they hide — measured on one box, C5 HHI step as one graph 2.71 ms with
// the branches, 2.42 ms without (eager: 2.55 with the side stream, 2.50 without); C5 HOI 4.14 vs 3.88 (eager 3.82 / 3.98).
// EGX_DEC_SIDE=2 forks under capture as well.
struct SideStream {
    hipStream_t s = nullptr;
    hipEvent_t ev[8] = {};
    hipEvent_t kv_ev[16] = {};      // forward: layer l's K | V projection of the memory is done
    int next = 0;
    bool on = false, on_captured = false;
    std::mutex mu;                  // forward and (autograd-thread) backward share the event ring
    // `to` continues behind everything enqueued on `from` so far. Record + wait of one ring event under the lock: two threads
    // picking the same event between the record and the wait would wait for each other's position.
    int order(hipStream_t from, hipStream_t to) {
        std::lock_guard<std::mutex> lk(mu);
        hipEvent_t e = ev[next]; next = (next + 1) % 8;
        EGX_HIP(hipEventRecord(e, from));
        EGX_HIP(hipStreamWaitEvent(to, e, 0));
        return 0;
    }
};
// one side stream per DEVICE, created on that device the first time a decoder call runs there (a process-global stream made
// on whichever device was current first would be the wrong device's stream for every other one)
SideStream& side_stream() {
    enum { MAXDEV = 16 };
    static SideStream S[MAXDEV];
    static std::once_flag once[MAXDEV];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) dev = 0;
    std::call_once(once[dev], [dev]() {
        SideStream& T = S[dev];
        const int mode = tuning().dec_side;
        if (mode != 0 && hipStreamCreateWithFlags(&T.s, hipStreamNonBlocking) == hipSuccess) {
            T.on = true; T.on_captured = mode == 2;
            for (auto& v : T.ev) if (hipEventCreateWithFlags(&v, hipEventDisableTiming) != hipSuccess) T.on = false;
            for (auto& v : T.kv_ev) if (hipEventCreateWithFlags(&v, hipEventDisableTiming) != hipSuccess) T.on = false;
        }
    });
    return S[dev];
}
// does this call fork? (never while `st` is being captured, unless EGX_DEC_SIDE=2)
bool side_wanted(const SideStream& SS, hipStream_t st) {
    if (!SS.on || SS.on_captured) return SS.on;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return true; }
    return cs == hipStreamCaptureStatusNone;
}
// joins the side stream back into the caller's stream when a call leaves — on the error paths too: an un-joined fork
// would invalidate an active stream capture (and leave work running that the caller's next launch may overwrite)
struct SideJoin {
    SideStream& SS; hipStream_t st; bool forked = false;
    SideJoin(SideStream& ss, hipStream_t s) : SS(ss), st(s) {}
    int join() { if (!forked) return 0; forked = false; return SS.order(SS.s, st); }
    ~SideJoin() { if (forked) (void)SS.order(SS.s, st); }
};
// a host seed is baked into a captured graph: every replay would redraw the SAME masks. The encoder's fused kernels have the
// device-resident seed (egx_config.seed_ptr) for that; the decoder has not, so training-mode dropout under capture is refused.
int refuse_captured_dropout(const egx_dec_config* cfg, int training, hipStream_t st) {
    if (!training || !(cfg->p_drop > 0.f || cfg->p_pos > 0.f) || cfg->seed_ptr) return 0;      // with seed_ptr every replay draws fresh masks
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return 0; }
    EGX_CHECK(cs == hipStreamCaptureStatusNone, "egx_decoder: training-mode dropout (p > 0) cannot be captured in a hipGraph: the host seed "
              "would be baked in and every replay would repeat the same masks; launch eagerly, capture with p = 0, or pass egx_dec_config.seed_ptr");
    return 0;
}

}  // namespace

}  // namespace egx

using namespace egx;

extern "C" {

int egx_decoder_workspace(const egx_dec_config* cfg, int B, size_t* saved_bytes, size_t* scratch_bytes) {
    DPlan pl;
    if (make_dplan(cfg, B, pl)) return 1;
    if (saved_bytes) *saved_bytes = pl.saved_bytes;
    if (scratch_bytes) *scratch_bytes = pl.scratch_bytes;
    return 0;
}

}  // extern "C"

namespace {
// ragged memories (egx_decoder_ragged_fwd): the device copy of the per-clip table and the clips of the two cross-attention kernel classes
struct DecRagged {
    const int* mtab;                // [B][2]: first memory row, memory rows
    const int* clips[2]; int n[2], Sk_max[2];      // class 0: Sk <= 64 (dec_attn_kernel), class 1: the chunked kernel
};

// the context of one decoder call over `pl` (wide_run.h): the decoder's keys are those of layers 0x40 + l; with a device-resident seed the
// kernels read them from the table in `saved` (the forward derives it there, the backward finds it)
WideRun decoder_run(const egx_dec_config* cfg, const DPlan& pl, const void* saved, void* scratch, int training, uint64_t seed, hipStream_t st) {
    WideRun r;
    r.saved = (char*)const_cast<void*>(saved); r.scratch = (char*)scratch; r.st = st; r.zero = r.sv<char>(pl.zero);
    r.ln_eps = cfg->ln_eps; r.p_drop = cfg->p_drop; r.training = training; r.seed = seed; r.layer_base = 0x40u;
    const bool dev_keys = cfg->seed_ptr && training && (cfg->p_drop > 0.f || cfg->p_pos > 0.f);
    r.keys = dev_keys ? r.sv<uint64_t>(pl.keys) : nullptr;
    return r;
}

// One layer's weights -> bf16 at `o`, with the transposes at `ot` for a call that runs backward; skip_in: not the self-attention
// in-projection (the cached step's layer 0 runs it in fp32 on the caller's weight and lays no copy out)
int dec_cast_layer(WideCastBatch& cb, const WideRun& r, const egx_dec_layer& w, const DecW& o, const DecW* ot, bool skip_in, int d, int dff) {
    auto t = [&](size_t DecW::*m) { return ot ? r.sv<bf16_t>(ot->*m) : nullptr; };
    if (!skip_in && wide_cast_add(cb, w.sa_in_w, 3 * d, d, d, r.sv<bf16_t>(o.sa_in), t(&DecW::sa_in), r.st)) return 1;
    if (wide_cast_add(cb, w.sa_out_w, d, d, d, r.sv<bf16_t>(o.sa_o), t(&DecW::sa_o), r.st)) return 1;
    if (wide_cast_add(cb, w.ca_in_w, d, d, d, r.sv<bf16_t>(o.q), t(&DecW::q), r.st)) return 1;
    if (wide_cast_add(cb, w.ca_in_w + (size_t)d * d, 2 * d, d, d, r.sv<bf16_t>(o.kv), t(&DecW::kv), r.st)) return 1;
    if (wide_cast_add(cb, w.ca_out_w, d, d, d, r.sv<bf16_t>(o.ca_o), t(&DecW::ca_o), r.st)) return 1;
    if (wide_cast_add(cb, w.lin1_w, dff, d, d, r.sv<bf16_t>(o.w1), t(&DecW::w1), r.st)) return 1;
    return wide_cast_add(cb, w.lin2_w, d, dff, dff, r.sv<bf16_t>(o.w2), t(&DecW::w2), r.st);
}

// What one decoder layer reads and writes: filled per layer from a DPlan (every layer its own buffers, kept for the backward) or from a
// StepPlan (one shared set). The cross-attention's K | V and the caches belong to the callers' attention callables.
struct DecLayerView {
    const float* x32; const bf16_t* x16;            // the layer's input rows (layer 0 reads the fp32 ones only)
    const bf16_t* w_sa_in; const bf16_t* w_q;       // (the other weights: in the sublayers)
    float* qkv32; bf16_t* qkv16; bf16_t* q;         // the self-attention's q | k | v (fp32: layer 0) and the cross-attention's queries
    WideProjLn sa_out, ca_out;                      // behind the two attentions, whose outputs are their a16
    WideFfn ffn;
};
// the weights W at `o` (W^T at `ot`, or none), the sublayers' three (pre-LN sum, statistics) pairs and outputs; y: the layer's output rows
void dec_view_sublayers(DecLayerView& v, const WideRun& r, const egx_dec_layer& w, const DecW& o, const DecW* ot, int d, int dff, bf16_t* sa, bf16_t* ca,
                        bf16_t* hid, float* const (&res)[3], float* const (&stats)[3], float* x1_32, bf16_t* x1_16, float* x2_32, bf16_t* x2_16,
                        float* y32, bf16_t* y16) {
    auto t = [&](size_t DecW::*m) { return ot ? r.sv<bf16_t>(ot->*m) : nullptr; };
    v.w_sa_in = r.sv<bf16_t>(o.sa_in); v.w_q = r.sv<bf16_t>(o.q);
    v.sa_out = {sa, d, r.sv<bf16_t>(o.sa_o), t(&DecW::sa_o), w.sa_out_b, v.x32, res[0], stats[0], w.norm1_w, w.norm1_b, x1_32, x1_16, DS_SA_OUT};
    v.ca_out = {ca, d, r.sv<bf16_t>(o.ca_o), t(&DecW::ca_o), w.ca_out_b, x1_32, res[1], stats[1], w.norm2_w, w.norm2_b, x2_32, x2_16, DS_CA_OUT};
    v.ffn = {x2_16, r.sv<bf16_t>(o.w1), t(&DecW::w1), w.lin1_b, dff, DS_FFN,
             {hid, dff, r.sv<bf16_t>(o.w2), t(&DecW::w2), w.lin2_b, x2_32, res[2], stats[2], w.norm3_w, w.norm3_b, y32, y16, DS_FFN_OUT}};
}
DecLayerView dplan_view(const WideRun& r, const DPlan& pl, int l, const egx_dec_layer& w) {
    const DLayer& o = pl.layer[l];
    const bool last = l + 1 == pl.L;
    DecLayerView v;
    v.x32 = r.sv<float>(o.x32); v.x16 = r.sv<bf16_t>(o.x16);
    v.qkv32 = r.sv<float>(pl.qkv32); v.qkv16 = r.sv<bf16_t>(o.qkv); v.q = r.sv<bf16_t>(o.q);
    float* const res[3] = {r.sv<float>(o.res1), r.sv<float>(o.res2), r.sv<float>(o.res3)};
    float* const stats[3] = {r.sv<float>(o.st1), r.sv<float>(o.st2), r.sv<float>(o.st3)};
    dec_view_sublayers(v, r, w, o.w, &o.wt, pl.d, pl.dff, r.sv<bf16_t>(o.sa), r.sv<bf16_t>(o.ca), r.sv<bf16_t>(o.hid), res, stats, r.sv<float>(o.x1_32),
                       r.sv<bf16_t>(o.x1_16), r.sv<float>(o.x2_32), r.sv<bf16_t>(o.x2_16), r.sv<float>(last ? pl.xL32 : pl.layer[l + 1].x32),
                       last ? nullptr : r.sv<bf16_t>(pl.layer[l + 1].x16));
    return v;
}

// the cross-attention of Sq query rows per clip onto the clip's Sk memory rows (k | v rows of 2d); the callers add dropout, ragged
// tables and the backward's gradients
DecAttnParams cross_attn_params(const bf16_t* q, const bf16_t* kv, bf16_t* o, int d, int B, int H, int Sq, int Sk) {
    DecAttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.ldq = d; a.k = kv; a.v = kv + d; a.ldk = a.ldv = 2 * d; a.o = o; a.ldo = d;
    a.B = B; a.H = H; a.Sq = Sq; a.Sk = Sk; a.causal = 0;
    return a;
}

// ONE decoder layer's forward over M target rows, for training (decoder_fwd_run) and for the cached step (StepRun::layers): nine launches
// around the callers' two attentions. self_attn(l, v, f32) reads v.qkv32 (f32) or v.qkv16 and writes v.sa_out.a16; cross_attn(l, v) reads v.q and
// writes v.ca_out.a16, behind whatever makes the memory's K | V ready. Dropout is the context's (a cached step's draws none).
// Causal self-attention over the target tokens: layer 0 sees the embeddings scaled by sqrt(d): its q / k are an order of magnitude larger
// than a LayerNorm output's and bf16-rounded scores would move the (near-saturated) softmax, so its in-projection runs on the exact
// fp32 MFMA GEMM and its attention reads fp32 q / k / v (three small GEMMs per step).
template <class SelfAttn, class CrossAttn>
int decoder_layer_fwd(const WideRun& r, const egx_dec_layer& w, const DecLayerView& v, int l, int M, int d, SelfAttn&& self_attn, CrossAttn&& cross_attn) {
    const bool f32_self = l == 0;
    if (f32_self) {
        GemmParams g;
        g.A = v.x32; g.B = w.sa_in_w; g.C = v.qkv32; g.M = M; g.N = 3 * d; g.K = d; g.lda = d; g.ldb = d; g.ldc = 3 * d; g.bias = w.sa_in_b;
        if (gemm(0, g, 0, 0, nullptr, 0, r.st)) return 1;
    } else if (r.nt(v.x16, v.w_sa_in, M, 3 * d, d, w.sa_in_b, nullptr, v.qkv16, 0, WideDrop(), nullptr)) return 1;
    if (self_attn(l, v, f32_self)) return 1;
    if (wide_proj_ln_fwd(r, v.sa_out, (uint32_t)l, M, d)) return 1;
    // cross-attention onto the memory
    if (r.nt(v.sa_out.y16, v.w_q, M, d, d, w.ca_in_b, nullptr, v.q, 0, WideDrop(), nullptr)) return 1;
    if (cross_attn(l, v)) return 1;
    if (wide_proj_ln_fwd(r, v.ca_out, (uint32_t)l, M, d)) return 1;
    return wide_ffn_fwd(r, v.ffn, (uint32_t)l, M, d);
}

int decoder_fwd_run(const egx_dec_config* cfg, const DPlan& pl, const int64_t* tokens, const float* memory, const float* emb, const float* pe,
                    int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, float* logits, void* saved,
                    int training, uint64_t seed, hipStream_t st, const DecRagged* rg) {
    if (refuse_captured_dropout(cfg, training, st)) return 1;
    const int d = pl.d, Md = (int)pl.Md, Nm = (int)pl.Nm, dh = d / pl.H;
    const WideRun r = decoder_run(cfg, pl, saved, nullptr, training, seed, st);
    // device-resident seed (the encoder's forward of this step has advanced it): this call's keys, derived on the stream
    if (r.keys && derive_keys(const_cast<uint64_t*>(cfg->seed_ptr), r.sv<uint64_t>(pl.keys), 0x40u, 16, 0, st)) return 1;
    EGX_HIP(hipMemsetAsync(r.sv<char>(pl.zero), 0, 1024, st));
    bf16_t* mem16 = r.sv<bf16_t>(pl.mem16);
    if (wide_cast(memory, Nm, d, d, mem16, nullptr, st)) return 1;
    {   // every weight -> bf16 (W and W^T), one launch
        WideCastBatch cb;
        for (int l = 0; l < pl.L; ++l)
            if (dec_cast_layer(cb, r, layers[l], pl.layer[l].w, &pl.layer[l].wt, false, d, pl.dff)) return 1;
        if (wide_cast_flush(cb, st)) return 1;
    }
    {   // embedding * sqrt(d) + positional encoding (+ dropout)
        const WideDrop de = r.drop(cfg->p_pos, 0, DS_EMBED);
        const size_t n4 = pl.Md * (d / 4);
        hipLaunchKernelGGL(dec_embed_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, tokens, emb, pe, pe_stride, sqrtf((float)d),
                           r.sv<float>(pl.layer[0].x32), r.sv<bf16_t>(pl.layer[0].x16), Md, pl.sy, d, pl.V, de.key, de.thresh, de.inv);
        EGX_LAUNCH_CHECK();
    }
    // the K | V projection of the memory for layer l (the one large GEMM of a layer), on stream s
    auto project_kv = [&](int l, hipStream_t s) {
        return r.nt_on(s, mem16, r.sv<bf16_t>(pl.layer[l].w.kv), Nm, 2 * d, d, layers[l].ca_in_b + d, nullptr, r.sv<bf16_t>(pl.layer[l].kv), 0, WideDrop(), nullptr);
    };
    // these depend on nothing the target-token chain computes: all of them go to the side stream now, beside the chain's 16-WG
    // launches; a layer's cross-attention waits for its own
    SideStream& SS = side_stream();
    SideJoin sj(SS, st);        // error paths: join whatever was forked
    const bool side = side_wanted(SS, st);
    if (side) {
        if (SS.order(st, SS.s)) return 1;
        sj.forked = true;
        for (int l = 0; l < pl.L; ++l) {
            if (project_kv(l, SS.s)) return 1;
            EGX_HIP(hipEventRecord(SS.kv_ev[l], SS.s));
        }
    }
    auto self_attn = [&](int l, const DecLayerView& v, bool f32) -> int {
        DecAttnParams a;
        memset(&a, 0, sizeof(a));
        if (f32) { a.q = v.qkv32; a.k = v.qkv32 + d; a.v = v.qkv32 + 2 * d; }
        else { a.q = v.qkv16; a.k = v.qkv16 + d; a.v = v.qkv16 + 2 * d; }
        a.ldq = a.ldk = a.ldv = 3 * d; a.o = v.sa_out.a16; a.ldo = d;
        a.B = B; a.H = pl.H; a.Sq = pl.sy; a.Sk = pl.sy; a.causal = 1;
        const WideDrop da = r.drop(cfg->p_drop, (uint32_t)l, DS_SELF);
        a.drop_key = da.key; a.drop_thresh = da.thresh; a.drop_inv = da.inv;
        return dec_attn<false>(a, dh, f32, st);
    };
    auto cross_attn = [&](int l, const DecLayerView& v) -> int {
        if (side) EGX_HIP(hipStreamWaitEvent(st, SS.kv_ev[l], 0));
        else if (project_kv(l, st)) return 1;
        DecAttnParams a = cross_attn_params(v.q, r.sv<bf16_t>(pl.layer[l].kv), v.ca_out.a16, d, B, pl.H, pl.sy, pl.S);
        const WideDrop da = r.drop(cfg->p_drop, (uint32_t)l, DS_CROSS);
        a.drop_key = da.key; a.drop_thresh = da.thresh; a.drop_inv = da.inv;
        if (!rg) return dec_attn<false>(a, dh, false, st);
        a.mtab = rg->mtab;
        for (int c = 0; c < 2; ++c) {
            a.clips = rg->clips[c]; a.B = rg->n[c]; a.Sk = rg->Sk_max[c];
            if (dec_attn_ragged_train<false>(a, dh, c == 1, st)) return 1;
        }
        return 0;
    };
    for (int l = 0; l < pl.L; ++l)
        if (decoder_layer_fwd(r, layers[l], dplan_view(r, pl, l, layers[l]), l, Md, d, self_attn, cross_attn)) return 1;
    {   // vocabulary head (|V| is 7..12: the shape-generic GEMM, fp32 rows in, fp32 logits out)
        GemmParams g;
        g.A = r.sv<float>(pl.xL32); g.B = fc_w; g.C = logits; g.M = Md; g.N = pl.V; g.K = d; g.lda = d; g.ldb = d; g.ldc = pl.V; g.bias = fc_b;
        if (gemm(0, g, 0, 0, nullptr, 0, st)) return 1;
    }
    sj.forked = false;      // joined already: every layer's cross-attention waited for its kv_ev, the last side-stream operation
    return 0;
}

// the ragged call's plan: DPlan over sum_b S_b memory rows, then the batch table (host copy in `tab`)
// (train: the training entry points, which take dropout; `bytes` is then the size of `saved`, the table behind the uniform plan's saved region)
int decoder_ragged_plan(const egx_dec_config* cfg, int B, const int* mem_lengths, DPlan& pl, std::vector<int>& tab, int (&n)[2], int (&smax)[2],
                        size_t& off_tab, size_t& bytes, bool train = false) {
    EGX_CHECK(cfg && mem_lengths, "egx_decoder_ragged: null argument");
    EGX_CHECK(B >= 1 && B <= (1 << 20), "egx_decoder_ragged: B=%d clips (1 .. %d)", B, 1 << 20);
    EGX_CHECK(!(cfg->n_heads > 0 && cfg->d_model % cfg->n_heads == 0 && dec_attn_bighead_dim(cfg->d_model / cfg->n_heads)),
              "egx_decoder_ragged: ragged memories serve head dim 32 / 64 (head dim %d: the 256 / 512 class runs uniform batches only, egx_decoder_fwd)",
              cfg->d_model / cfg->n_heads);
    EGX_CHECK(train || (cfg->p_drop == 0.f && cfg->p_pos == 0.f), "egx_decoder_ragged: inference only: p_drop and p_pos must be 0 (got %g, %g)", cfg->p_drop, cfg->p_pos);
    size_t rows = 0;
    n[0] = n[1] = 0; smax[0] = smax[1] = 0;
    tab.assign((size_t)3 * B, 0);       // [B][2] table, then the clips of class 0 and of class 1
    for (int b = 0; b < B; ++b) {
        const int S = mem_lengths[b];
        EGX_CHECK(S >= 1 && S <= cfg->S, "egx_decoder_ragged: clip %d has a memory of %d rows (1 .. %d = egx_dec_config.S)", b, S, cfg->S);
        tab[2 * b] = (int)rows; tab[2 * b + 1] = S;
        rows += S;
        const int c = S > DA_MAXK;
        n[c]++; smax[c] = S > smax[c] ? S : smax[c];
    }
    EGX_CHECK(rows <= (size_t)1 << 30, "egx_decoder_ragged: %zu memory rows", rows);
    int i0 = 0, i1 = n[0];
    for (int b = 0; b < B; ++b) tab[(size_t)2 * B + (tab[2 * b + 1] > DA_MAXK ? i1++ : i0++)] = b;
    if (make_dplan(cfg, B, pl, rows)) return 1;
    off_tab = align_up(pl.saved_bytes, 256);
    bytes = off_tab + align_up(tab.size() * sizeof(int), 256);
    return 0;
}
DecRagged dec_ragged_view(const int* dtab, int B, const int (&n)[2], const int (&smax)[2]) {
    DecRagged rg;
    rg.mtab = dtab;
    rg.clips[0] = dtab + 2 * (size_t)B; rg.clips[1] = rg.clips[0] + n[0];
    for (int c = 0; c < 2; ++c) { rg.n[c] = n[c]; rg.Sk_max[c] = smax[c] ? smax[c] : 1; }
    return rg;
}
}  // namespace

extern "C" {

int egx_decoder_fwd(const egx_dec_config* cfg, const int64_t* tokens, const float* memory, const float* emb, const float* pe, int pe_stride,
                    const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, float* logits, void* saved, void* scratch,
                    int training, uint64_t seed, void* stream) {
    DPlan pl;
    if (make_dplan(cfg, B, pl)) return 1;
    EGX_CHECK(tokens && memory && emb && pe && layers && fc_w && logits && saved && scratch, "egx_decoder_fwd: null pointer argument");
    return decoder_fwd_run(cfg, pl, tokens, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, logits, saved, training, seed, (hipStream_t)stream, nullptr);
}

int egx_decoder_ragged_workspace(const egx_dec_config* cfg, int B, const int* mem_lengths, size_t* bytes) {
    DPlan pl;
    std::vector<int> tab;
    int n[2], smax[2];
    size_t off_tab = 0, nb = 0;
    if (decoder_ragged_plan(cfg, B, mem_lengths, pl, tab, n, smax, off_tab, nb)) return 1;
    if (bytes) *bytes = nb;
    return 0;
}

int egx_decoder_ragged_fwd(const egx_dec_config* cfg, const int64_t* tokens, const float* memory, const int* mem_lengths, const float* emb,
                           const float* pe, int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, float* logits,
                           void* workspace, void* stream) {
    DPlan pl;
    std::vector<int> tab;
    int n[2], smax[2];
    size_t off_tab = 0, nb = 0;
    if (decoder_ragged_plan(cfg, B, mem_lengths, pl, tab, n, smax, off_tab, nb)) return 1;
    EGX_CHECK(tokens && memory && emb && pe && layers && fc_w && logits && workspace, "egx_decoder_ragged_fwd: null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    // the table goes to the device in the arguments of upload launches (stream-ordered; a captured graph would replay THESE lengths)
    int* dtab = at<int>(workspace, off_tab);
    if (upload_words(dtab, tab.data(), tab.size(), st)) return 1;
    const DecRagged rg = dec_ragged_view(dtab, B, n, smax);
    return decoder_fwd_run(cfg, pl, tokens, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, logits, workspace, 0, 0, st, &rg);
}

int egx_cross_attention_weights(const void* q, int ldq, const void* k, int ldk, int operands_bf16, const int* mtab, int B, int H, int dh, int Sq,
                                int Sk, float* out, int ldo, void* stream) {
    CrossWParams p;
    memset(&p, 0, sizeof(p));
    p.q = q; p.k = k; p.ldq = ldq; p.ldk = ldk; p.mtab = mtab; p.out = out; p.ldo = ldo; p.B = B; p.H = H; p.Sq = Sq; p.Sk = Sk;
    return cross_weights(p, dh, !operands_bf16, (hipStream_t)stream);
}

int egx_decoder_cross_weights(const egx_dec_config* cfg, int B, const int* mem_lengths, const void* saved, float* attn_out, void* stream) {
    EGX_CHECK(cfg, "egx_decoder_cross_weights: null decoder config");
    EGX_CHECK(cfg->p_drop == 0.f && cfg->p_pos == 0.f, "egx_decoder_cross_weights: inference only: p_drop and p_pos must be 0 (got %g, %g)",
              cfg->p_drop, cfg->p_pos);
    EGX_CHECK(!(cfg->n_heads > 0 && cfg->d_model % cfg->n_heads == 0 && dec_attn_bighead_dim(cfg->d_model / cfg->n_heads)),
              "egx_decoder_cross_weights: head dim %d (16, 32, 64 or 128: the weights of the 256 / 512 class are not served)", cfg->d_model / cfg->n_heads);
    DPlan pl;
    size_t off_tab = 0;
    int S = cfg->S;
    if (mem_lengths) {      // the plan of egx_decoder_ragged_fwd: the table that call uploaded sits behind the plan's saved region
        std::vector<int> tab;
        int n[2], smax[2];
        size_t nb = 0;
        if (decoder_ragged_plan(cfg, B, mem_lengths, pl, tab, n, smax, off_tab, nb)) return 1;
        S = smax[0] > smax[1] ? smax[0] : smax[1];
    } else if (make_dplan(cfg, B, pl)) return 1;
    EGX_CHECK(saved && attn_out, "egx_decoder_cross_weights: null pointer argument");
    const int* mtab = mem_lengths ? cat<int>(saved, off_tab) : nullptr;
    for (int l = 0; l < pl.L; ++l) {
        CrossWParams p;
        memset(&p, 0, sizeof(p));
        p.q = cat<bf16_t>(saved, pl.layer[l].q); p.ldq = pl.d; p.k = cat<bf16_t>(saved, pl.layer[l].kv); p.ldk = 2 * pl.d; p.mtab = mtab;
        p.out = attn_out + (size_t)l * B * pl.sy * S; p.ldo = S; p.B = B; p.H = pl.H; p.Sq = pl.sy; p.Sk = S;
        if (cross_weights(p, pl.d / pl.H, false, (hipStream_t)stream)) return 1;
    }
    return 0;
}

}  // extern "C"

namespace {
// the decoder backward over `pl` (uniform: B * S memory rows; rg: the packed rows of a ragged memory, whose cross-attention backward runs per
// kernel class over the batch table — everything else is row-wise over the B * sy target rows and the pl.Nm memory rows)
int decoder_bwd_run(const egx_dec_config* cfg, const DPlan& pl, const int64_t* tokens, const egx_dec_layer* layers, const float* fc_w, int B,
                    const float* d_logits, const void* saved, void* scratch, float* d_memory, float* d_emb, const egx_dec_layer_grads* grads,
                    float* d_fc_w, float* d_fc_b, void* zero_buf, size_t zero_bytes, int training, uint64_t seed, hipStream_t st,
                    const DecRagged* rg) {
    if (refuse_captured_dropout(cfg, training, st)) return 1;
    const int d = pl.d, Md = (int)pl.Md, Nm = (int)pl.Nm, dh = d / pl.H;
    WideRun r = decoder_run(cfg, pl, saved, scratch, training, seed, st);
    if (zero_buf && zero_bytes) EGX_HIP(hipMemsetAsync(zero_buf, 0, zero_bytes, st));
    float* gA = r.sc<float>(pl.gA);
    float* gB = r.sc<float>(pl.gB);
    float* dres = r.sc<float>(pl.dres);
    bf16_t* dattn16 = r.sc<bf16_t>(pl.dattn16);
    float* cspart_side = r.sc<float>(pl.cspart_side);
    // side stream for the weight gradients: fork() orders it behind everything enqueued on `st` so far
    SideStream& SS = side_stream();
    const bool side = side_wanted(SS, st);
    hipStream_t sd = side ? SS.s : st;
    SideJoin sj(SS, st);
    auto fork = [&]() -> int {
        if (!side) return 0;
        if (SS.order(st, sd)) return 1;
        sj.forked = true;
        return 0;
    };
    const bf16_t* mem16 = r.sv<bf16_t>(pl.mem16);

    // The ledger (wide_run.h): every weight gradient has a slab region of its own (none left: refused) and their split-K sums run as one
    // launch at the end; the second stages of the two-stage column sums (LayerNorm / bias gradients) are queued with a partial buffer of
    // their own each and summed by ONE launch at the end (every target is a different parameter: concurrent sums never meet).
    // Round 5: the weight gradients are QUEUED and leave as one grouped launch per tile variant at the end of the call (wide_gemm.hip
    // wide_tn_queue_*): 35 launches of 14 us each over 512 target rows become one or two grids that fill the chip. Their operands sit in
    // per-(layer, use) buffers until then. Used where the side stream is not (a captured step, EGX_DEC_SIDE=0): with eager launches the
    // side stream already hides these GEMMs beside the target-token chain and grouping them at the end measured 1.4 % slower (C5 HOI
    // 3.80 -> 3.86 ms); captured, C5 HHI 2.42 -> 2.26 ms (profiles/r05_dec_group.txt). EGX_DEC_GROUP=0 / 1 forces either.
    // (ungrouped: enqueued on the side stream; the caller forks first)
    // (Writing straight into dW with one split over <= 1024 target rows - no slab, no batched reduction of 55-73 us - lengthened the side
    // stream: same-box C5 HOI 3.95 = 3.95 ms, C5 HHI 2.46 -> 2.62 ms. That variant last existed at 3b19ffd.)
    WideLedger led;
    led.st = st; led.tn_stream = sd; led.zero = r.zero;
    led.slab = r.sc<char>(pl.slab_all); led.slab_bytes = pl.slab_all_bytes;
    led.rows = r.sc<char>(pl.rowpart); led.rows_bytes = pl.rowpart_bytes;
    led.lnpart = r.sc<char>(pl.lnpart); led.cspart = r.sc<float>(pl.cspart);
    led.fresh = (const char*)zero_buf; led.fresh_bytes = zero_bytes;
    const int group_env = tuning().dec_group;
    led.grouped = group_env >= 0 ? group_env != 0 : !side;
    r.led = &led;

    // vocabulary head: d(fc_w) += d_logits^T x, d(fc_b) += colsum, g = d_logits fc_w
    float* g = gA;
    {
        const float* xL = r.sv<float>(pl.xL32);
        if (d_fc_w) {
            GemmParams t;
            t.A = d_logits; t.B = xL; t.C = d_fc_w; t.M = pl.V; t.N = d; t.K = Md; t.lda = pl.V; t.ldb = d; t.ldc = d;
            if (gemm(2, t, 0, 1, r.sc<char>(pl.fcslab), pl.fcslab_bytes, st)) return 1;
        }
        if (d_fc_b && colsum_accum(d_logits, Md, pl.V, pl.V, d_fc_b, st)) return 1;
        GemmParams q;
        q.A = d_logits; q.B = fc_w; q.C = g; q.M = Md; q.N = d; q.K = pl.V; q.lda = pl.V; q.ldb = d; q.ldc = d;
        if (gemm(1, q, 0, 0, r.sc<char>(pl.fcslab), pl.fcslab_bytes, st)) return 1;
    }
    bool mem_started = false;
    for (int l = pl.L - 1; l >= 0; --l) {
        const DLayer& o = pl.layer[l];
        const egx_dec_layer_grads& gw = grads[l];
        const DecLayerView v = dplan_view(r, pl, l, layers[l]);
        bf16_t* dy16a = r.sc<bf16_t>(pl.g[l].dy16[0]);
        bf16_t* dy16b = r.sc<bf16_t>(pl.g[l].dy16[1]);
        bf16_t* dy16c = r.sc<bf16_t>(pl.g[l].dy16[2]);
        bf16_t* dqkv16 = r.sc<bf16_t>(pl.g[l].dqkv16);
        bf16_t* dq16 = r.sc<bf16_t>(pl.g[l].dq16);
        bf16_t* dkv16 = r.sc<bf16_t>(pl.g[l].dkv16);
        // FFN
        float* g1 = (g == gA) ? gB : gA;
        if (wide_ffn_bwd(r, v.ffn, {gw.lin1_w, gw.lin1_b, {gw.lin2_w, gw.lin2_b, gw.norm3_w, gw.norm3_b}}, (uint32_t)l, Md, d, g, dres, dy16a,
                         r.sc<bf16_t>(pl.g[l].dhid16), g1, fork)) return 1;
        // cross-attention
        if (wide_proj_ln_bwd(r, v.ca_out, {gw.ca_out_w, gw.ca_out_b, gw.norm2_w, gw.norm2_b}, (uint32_t)l, Md, d, g1, dres, dy16b, fork)) return 1;
        if (r.nt_bwd(dy16b, v.ca_out.w_t, Md, d, d, nullptr, dattn16, nullptr)) return 1;
        {
            DecAttnParams a = cross_attn_params(v.q, r.sv<bf16_t>(o.kv), nullptr, d, B, pl.H, pl.sy, pl.S);
            a.d_o = dattn16; a.dq = dq16; a.dk = dkv16; a.dv = dkv16 + d;
            const WideDrop da = r.drop(cfg->p_drop, (uint32_t)l, DS_CROSS);
            a.drop_key = da.key; a.drop_thresh = da.thresh; a.drop_inv = da.inv;
            if (rg) {
                a.mtab = rg->mtab;
                for (int c = 0; c < 2; ++c) {
                    a.clips = rg->clips[c]; a.B = rg->n[c]; a.Sk = rg->Sk_max[c];
                    if (dec_attn_ragged_train<true>(a, dh, c == 1, st)) return 1;
                }
            } else if (dec_attn<true>(a, dh, false, st)) return 1;
        }
        if (fork()) return 1;
        if (gw.ca_in_b && (led.colsum(dq16, Md, d, gw.ca_in_b, cspart_side, sd) || led.colsum(dkv16, Nm, 2 * d, gw.ca_in_b + d, cspart_side, sd))) return 1;
        if (led.dw_tn(dq16, v.sa_out.y16, gw.ca_in_w, d, d, Md)) return 1;
        if (led.dw_tn(dkv16, mem16, gw.ca_in_w ? gw.ca_in_w + (size_t)d * d : nullptr, 2 * d, d, Nm)) return 1;
        if (d_memory) {     // d(memory) (+)= d(kv) W_kv, summed over the layers
            if (r.nt_bwd(dkv16, r.sv<bf16_t>(o.wt.kv), Nm, d, 2 * d, d_memory, nullptr, mem_started ? d_memory : nullptr)) return 1;
            mem_started = true;
        }
        float* g2 = (g1 == gA) ? gB : gA;
        if (r.nt_bwd(dq16, r.sv<bf16_t>(o.wt.q), Md, d, d, g2, nullptr, dres)) return 1;
        // self-attention
        if (wide_proj_ln_bwd(r, v.sa_out, {gw.sa_out_w, gw.sa_out_b, gw.norm1_w, gw.norm1_b}, (uint32_t)l, Md, d, g2, dres, dy16c, fork)) return 1;
        if (r.nt_bwd(dy16c, v.sa_out.w_t, Md, d, d, nullptr, dattn16, nullptr)) return 1;
        const bool f32_self = l == 0;
        float* dqkv32 = r.sc<float>(pl.dqkv32);
        {
            DecAttnParams a;
            memset(&a, 0, sizeof(a));
            if (f32_self) {
                a.q = v.qkv32; a.k = v.qkv32 + d; a.v = v.qkv32 + 2 * d; a.dq = dqkv32; a.dk = dqkv32 + d; a.dv = dqkv32 + 2 * d;
            } else {
                a.q = v.qkv16; a.k = v.qkv16 + d; a.v = v.qkv16 + 2 * d; a.dq = dqkv16; a.dk = dqkv16 + d; a.dv = dqkv16 + 2 * d;
            }
            a.ldq = a.ldk = a.ldv = 3 * d; a.ldo = d; a.d_o = dattn16;
            a.B = B; a.H = pl.H; a.Sq = pl.sy; a.Sk = pl.sy; a.causal = 1;
            const WideDrop da = r.drop(cfg->p_drop, (uint32_t)l, DS_SELF);
            a.drop_key = da.key; a.drop_thresh = da.thresh; a.drop_inv = da.inv;
            if (dec_attn<true>(a, dh, f32_self, st)) return 1;
        }
        float* g0 = (g2 == gA) ? gB : gA;
        if (f32_self) {     // exact fp32 in-projection gradients (see the forward); these stay on the caller's stream (they share
                            // the fp32 slab with the vocabulary head's GEMMs)
            if (gw.sa_in_b && colsum_accum(dqkv32, Md, 3 * d, 3 * d, gw.sa_in_b, st)) return 1;
            if (gw.sa_in_w) {
                GemmParams t;
                t.A = dqkv32; t.B = v.x32; t.C = gw.sa_in_w; t.M = 3 * d; t.N = d; t.K = Md; t.lda = 3 * d; t.ldb = d; t.ldc = d;
                if (gemm(2, t, 0, 1, r.sc<char>(pl.fcslab), pl.fcslab_bytes, st)) return 1;
            }
            // d(layer input): only the embedding gradient reads it -> the bf16 GEMM like the other layers, on a bf16 copy of dqkv
            if (wide_cast(dqkv32, Md, 3 * d, 3 * d, dqkv16, nullptr, st)) return 1;
        } else {
            if (fork()) return 1;
            if (gw.sa_in_b && led.colsum(dqkv16, Md, 3 * d, gw.sa_in_b, cspart_side, sd)) return 1;
            if (led.dw_tn(dqkv16, v.x16, gw.sa_in_w, 3 * d, d, Md)) return 1;
        }
        if (r.nt_bwd(dqkv16, r.sv<bf16_t>(o.wt.sa_in), Md, d, 3 * d, g0, nullptr, dres)) return 1;
        g = g0;
    }
    if (sj.join()) return 1;    // the slab reduction below (and whatever the caller enqueues next) comes after the side stream's work
    if (d_memory && !mem_started) EGX_HIP(hipMemsetAsync(d_memory, 0, pl.Nm * d * sizeof(float), st));
    if (d_emb) {
        const WideDrop de = r.drop(cfg->p_pos, 0, DS_EMBED);
        if (pl.V <= EMB_VMAX)
        {
            int G = 65536 / (pl.V * 256);
            G = G > 16 ? 16 : (G < 1 ? 1 : G);
            hipLaunchKernelGGL(dec_embed_grad_small_kernel, dim3(cdiv(d, 64)), dim3(64 * G), (size_t)G * pl.V * 256, st, tokens, g, d_emb,
                               sqrtf((float)d), Md, d, pl.V, de.key, de.thresh, de.inv);
        }
        else
            hipLaunchKernelGGL(dec_embed_grad_kernel, dim3(cdiv(d, 64), pl.V), dim3(256), 0, st, tokens, g, d_emb, sqrtf((float)d), Md, d, pl.V,
                               de.key, de.thresh, de.inv);
        EGX_LAUNCH_CHECK();
    }
    return led.flush();
}
}  // namespace

extern "C" {

int egx_decoder_bwd(const egx_dec_config* cfg, const int64_t* tokens, const egx_dec_layer* layers, const float* fc_w, int B, const float* d_logits,
                    const void* saved, void* scratch, float* d_memory, float* d_emb, const egx_dec_layer_grads* grads, float* d_fc_w,
                    float* d_fc_b, void* zero_buf, size_t zero_bytes, int training, uint64_t seed, void* stream) {
    DPlan pl;
    if (make_dplan(cfg, B, pl)) return 1;
    EGX_CHECK(tokens && layers && fc_w && d_logits && saved && scratch && grads, "egx_decoder_bwd: null pointer argument");
    return decoder_bwd_run(cfg, pl, tokens, layers, fc_w, B, d_logits, saved, scratch, d_memory, d_emb, grads, d_fc_w, d_fc_b, zero_buf, zero_bytes,
                           training, seed, (hipStream_t)stream, nullptr);
}

/* ---- training over ragged memories (the decoder side of HHI/tasks/multitask/video_tasktranslation.py:39-66 on the mixed-length batches its
 * SequenceBatchSampler, :144-156, cannot form; decode() of HHI/models/multitask/task_prompt_model.py:260-269) ---- */
int egx_decoder_ragged_train_workspace(const egx_dec_config* cfg, int B, const int* mem_lengths, size_t* saved_bytes, size_t* scratch_bytes) {
    DPlan pl;
    std::vector<int> tab;
    int n[2], smax[2];
    size_t off_tab = 0, nb = 0;
    if (decoder_ragged_plan(cfg, B, mem_lengths, pl, tab, n, smax, off_tab, nb, true)) return 1;
    if (saved_bytes) *saved_bytes = nb;
    if (scratch_bytes) *scratch_bytes = pl.scratch_bytes;
    return 0;
}

int egx_decoder_ragged_train_fwd(const egx_dec_config* cfg, const int64_t* tokens, const float* memory, const int* mem_lengths, const float* emb,
                                 const float* pe, int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B,
                                 float* logits, void* saved, void* scratch, int training, uint64_t seed, void* stream) {
    DPlan pl;
    std::vector<int> tab;
    int n[2], smax[2];
    size_t off_tab = 0, nb = 0;
    if (decoder_ragged_plan(cfg, B, mem_lengths, pl, tab, n, smax, off_tab, nb, true)) return 1;
    EGX_CHECK(tokens && memory && emb && pe && layers && fc_w && logits && saved, "egx_decoder_ragged_train_fwd: null pointer argument");
    (void)scratch;
    hipStream_t st = (hipStream_t)stream;
    int* dtab = at<int>(saved, off_tab);       // (kept in `saved`: the backward reads the same table)
    if (upload_words(dtab, tab.data(), tab.size(), st)) return 1;
    const DecRagged rg = dec_ragged_view(dtab, B, n, smax);
    return decoder_fwd_run(cfg, pl, tokens, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, logits, saved, training, seed, st, &rg);
}

int egx_decoder_ragged_bwd(const egx_dec_config* cfg, const int64_t* tokens, const int* mem_lengths, const egx_dec_layer* layers, const float* fc_w,
                           int B, const float* d_logits, const void* saved, void* scratch, float* d_memory, float* d_emb,
                           const egx_dec_layer_grads* grads, float* d_fc_w, float* d_fc_b, void* zero_buf, size_t zero_bytes, int training,
                           uint64_t seed, void* stream) {
    DPlan pl;
    std::vector<int> tab;
    int n[2], smax[2];
    size_t off_tab = 0, nb = 0;
    if (decoder_ragged_plan(cfg, B, mem_lengths, pl, tab, n, smax, off_tab, nb, true)) return 1;
    EGX_CHECK(tokens && layers && fc_w && d_logits && saved && scratch && grads, "egx_decoder_ragged_bwd: null pointer argument");
    // (the forward left the table in `saved`; the host copy rebuilt from the same lengths gives its layout)
    const DecRagged rg = dec_ragged_view(cat<int>(saved, off_tab), B, n, smax);
    return decoder_bwd_run(cfg, pl, tokens, layers, fc_w, B, d_logits, saved, scratch, d_memory, d_emb, grads, d_fc_w, d_fc_b, zero_buf, zero_bytes,
                           training, seed, (hipStream_t)stream, &rg);
}

}  // extern "C"

// ---- greedy generation with a K/V cache (egx_decoder_generate) ----
// The inference loop of the EgoT2-g sequence models (predict_ac, HOI/models/multitask/video_model_builder.py:201-220, 263-274; the 40-step
// verb / noun loop of HOI/models/lta/lta_models_seqdecoder.py:181-201) as ONE call: weights and memory to bf16 once, the memory's K | V
// projected once per layer, then per step ONE new target row per clip through the layers (self-attention over a per-layer K/V cache), the
// fp32 vocabulary head, the argmax and the next token's embedding on the device. Arithmetic as decoder_fwd_run, choice for choice.
namespace {

constexpr int GEN_MAX_STEPS = 64, BEAM_MAX_W = DA_MAXQ, BEAM_DEPTH = GEN_MAX_STEPS;

// rows that each read their own history (greedy, forced): row b's history is cache rows (b, 0 .. t - 1)
struct GenAttnParams {
    const void* qkv;        // (B, 3d): the new row's q | k | v (fp32 or bf16)
    void* cache;            // (B, n_steps, 2d): k | v of rows 0 .. t - 1; row t is appended
    bf16_t* o;              // (B, d)
    int B, H, d, t, n_steps;
    float scale;
};
// beam search: hypothesis slot w of clip b (row b * W + w) reads its history through an ancestry table instead of a gathered cache
struct BeamAttnParams {
    const void* qkv;        // (B * W, 3d): the new rows' q | k | v (fp32 or bf16)
    void* cache;            // (B, W, n_steps, 2d): row (b, s, j) = k | v of the row slot s of clip b ran at step j; written once
    const int* anc;         // (B, W, BEAM_DEPTH): anc[b][w][j], j < t = the slot that ran row j of hypothesis w's history
    bf16_t* o;              // (B * W, d)
    int B, W, H, d, t, n_steps;
    float scale;
};
template <bool ANC>
using CachedAttnParams = std::conditional_t<ANC, BeamAttnParams, GenAttnParams>;

// One wave per (row, head), four per workgroup. Lane j holds key row j (j < t from the cache, j == t the new row, which lanes c < DH also
// append to the cache); the query goes through a per-wave LDS slice as broadcast reads; lane c accumulates column c of the output. Sums run
// in dec_attn_kernel's order, so a step sees the scores and the output a causal decode() of the same rows computes. t < 64 = one key per
// lane. ANC: history row j of row (b, w) is cache row (b, anc[b][w][j], j) instead of (row, j); same lane roles and summation order, so
// with W = 1 (every slot 0) the same bits. (The two forms of every cache address are kept apart as written: each instance's instruction
// stream is the one of the kernel it had to itself.)
template <int DH, bool F32, bool ANC>
__global__ __launch_bounds__(256) void cached_self_attn_kernel(CachedAttnParams<ANC> p) {
    __shared__ __align__(16) float sQ[4][DH];   // (read as float4)
    __shared__ float sP[4][64];
    __shared__ int sS[ANC ? 4 : 1][64];         // ANC: slot of history row j
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rh = blockIdx.x * 4 + wave;
    int W = 1;
    if constexpr (ANC) W = p.W;
    if (rh >= p.B * W * p.H) return;            // (no barrier below: every wave works alone)
    const int r = rh / p.H, h = rh % p.H, t = p.t, d = p.d, b = r / W;
    const size_t nrow = (size_t)r * 3 * d + h * DH;                         // q; k at + d, v at + 2d
    // cache row (b, s, j) at ((b * W + s) * n_steps + j) * 2d + ccol: k; v at + d. Without ancestry s = w: row r's rows follow crow
    size_t ccol = 0, cnew = 0, crow = 0;
    if constexpr (ANC) {
        ccol = (size_t)h * DH;
        cnew = ((size_t)r * p.n_steps + t) * 2 * d + ccol;
    } else {
        crow = (size_t)r * p.n_steps * 2 * d + h * DH;
    }
    const bool cached = lane < t;
    int slot = 0;
    if constexpr (ANC) {
        slot = cached ? p.anc[(size_t)r * BEAM_DEPTH + lane] : 0;
        slot = slot < 0 ? 0 : (slot >= p.W ? p.W - 1 : slot);               // (the head writes 0 .. W - 1)
        sS[wave][lane] = slot;
    }
    float kr[DH];
    {
        const void* kb = cached ? (const void*)p.cache : p.qkv;
        size_t krow;
        if constexpr (ANC) krow = cached ? (((size_t)b * p.W + slot) * p.n_steps + lane) * 2 * d + ccol : nrow + d;
        else krow = cached ? crow + (size_t)lane * 2 * d : nrow + d;
#pragma unroll
        for (int c = 0; c < DH; c += 8) {
            float t8[8];
            load8<F32>(kb, krow + c, t8);
#pragma unroll
            for (int e = 0; e < 8; ++e) kr[c + e] = t8[e];
        }
    }
    float vnew = 0.f;
    if (lane < DH) {                            // append row t (read by later steps only)
        const float knew = load1<F32>(p.qkv, nrow + d + lane);
        vnew = load1<F32>(p.qkv, nrow + 2 * d + lane);
        if constexpr (ANC) {
            store1<F32>(p.cache, cnew + lane, knew);
            store1<F32>(p.cache, cnew + d + lane, vnew);
        } else {
            store1<F32>(p.cache, crow + (size_t)t * 2 * d + lane, knew);
            store1<F32>(p.cache, crow + (size_t)t * 2 * d + d + lane, vnew);
        }
        sQ[wave][lane] = load1<F32>(p.qkv, nrow + lane);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const bool live = lane <= t;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < DH; c += 4) {
        const float4 qv = *reinterpret_cast<const float4*>(&sQ[wave][c]);
        s += (qv.x * kr[c] + qv.y * kr[c + 1]) + (qv.z * kr[c + 2] + qv.w * kr[c + 3]);
    }
    s = live ? s * p.scale : -INFINITY;
    const float m = wave_max(s);
    const float e = live ? __expf(s - m) : 0.f;
    sP[wave][lane] = e / wave_sum(e);
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < DH) {
        float acc = 0.f;
        if constexpr (ANC) {
            const size_t v0 = (size_t)b * p.W * p.n_steps * 2 * d + ccol + d + lane;
            for (int j = 0; j < t; ++j) acc += sP[wave][j] * load1<F32>(p.cache, v0 + ((size_t)sS[wave][j] * p.n_steps + j) * 2 * d);
        } else {
            const size_t v0 = crow + d + lane;
            for (int j = 0; j < t; ++j) acc += sP[wave][j] * load1<F32>(p.cache, v0 + (size_t)j * 2 * d);
        }
        acc += sP[wave][t] * vnew;
        p.o[(size_t)r * d + h * DH + lane] = f2bf(acc);
    }
}

// Head dim 256 / 512 (the 2048-wide LTA sequence decoders): a key row per lane would be the whole register file, so here the LANES SPLIT THE
// HEAD DIM, NC = DH / 64 consecutive columns each, and the wave walks the history: row j's score is the wave sum of the lanes' partial
// products and stays on lane j; the softmax runs across the lanes as above; the output is the walk again, P[j] broadcast from lane j. No
// LDS, no barrier; NC-element registers whatever the history's length. Cache layout, appended row and ancestry as cached_self_attn_kernel.
template <bool F32, int NC>
__device__ __forceinline__ void loadc(const void* base, size_t idx, float (&o)[NC]) {
    if constexpr (NC == 8) {
        load8<F32>(base, idx, o);
    } else if constexpr (F32) {
        const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + idx);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    } else {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16_t*>(base) + idx);
        o[0] = bf_lo(u.x); o[1] = bf_hi(u.x); o[2] = bf_lo(u.y); o[3] = bf_hi(u.y);
    }
}
template <bool F32, int NC>
__device__ __forceinline__ void storec(void* base, size_t idx, const float (&a)[NC]) {
    if constexpr (NC == 8) {
        store8<F32>(base, idx, a);
    } else if constexpr (F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + idx) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(base) + idx) = make_uint2(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]));
    }
}
template <int DH, bool F32, bool ANC>
__global__ __launch_bounds__(256) void cached_self_attn_bighead_kernel(CachedAttnParams<ANC> p) {
    constexpr int NC = DH / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rh = blockIdx.x * 4 + wave;
    int W = 1;
    if constexpr (ANC) W = p.W;
    if (rh >= p.B * W * p.H) return;            // (no barrier below: every wave works alone)
    const int r = rh / p.H, h = rh % p.H, t = p.t, d = p.d, b = r / W;
    const size_t col = (size_t)h * DH + lane * NC;                          // this lane's columns of a d-wide row
    const size_t nrow = (size_t)r * 3 * d + col;                            // q; k at + d, v at + 2d
    int slot = 0;
    if constexpr (ANC) {
        slot = lane < t ? p.anc[(size_t)r * BEAM_DEPTH + lane] : 0;
        slot = slot < 0 ? 0 : (slot >= p.W ? p.W - 1 : slot);               // (the head writes 0 .. W - 1)
    }
    // cache row (row, j): k at crow(j), v at + d
    auto crow = [&](int j) -> size_t {
        size_t row = (size_t)r;
        if constexpr (ANC) row = (size_t)b * W + __shfl(slot, j, 64);
        return (row * p.n_steps + j) * 2 * d + col;
    };
    float q[NC], kn[NC], vn[NC];
    loadc<F32, NC>(p.qkv, nrow, q);
    loadc<F32, NC>(p.qkv, nrow + d, kn);
    loadc<F32, NC>(p.qkv, nrow + 2 * d, vn);
    {   // append row t (read by later steps only)
        const size_t cnew = ((size_t)r * p.n_steps + t) * 2 * d + col;
        storec<F32, NC>(p.cache, cnew, kn);
        storec<F32, NC>(p.cache, cnew + d, vn);
    }
    float s = -INFINITY;
    for (int j = 0; j <= t; ++j) {
        float kj[NC];
        if (j < t) {
            loadc<F32, NC>(p.cache, crow(j), kj);
        } else {
#pragma unroll
            for (int e = 0; e < NC; ++e) kj[e] = kn[e];
        }
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < NC; ++e) part = fmaf(q[e], kj[e], part);
        const float tot = wave_sum(part);
        if (lane == j) s = tot * p.scale;
    }
    const bool live = lane <= t;
    const float m = wave_max(s);
    const float e = live ? __expf(s - m) : 0.f;
    const float prob = e / wave_sum(e);
    float acc[NC];
#pragma unroll
    for (int x = 0; x < NC; ++x) acc[x] = 0.f;
    for (int j = 0; j < t; ++j) {
        float vj[NC];
        loadc<F32, NC>(p.cache, crow(j) + d, vj);
        const float pj = __shfl(prob, j, 64);
#pragma unroll
        for (int x = 0; x < NC; ++x) acc[x] = fmaf(pj, vj[x], acc[x]);
    }
    {
        const float pt = __shfl(prob, t, 64);
#pragma unroll
        for (int x = 0; x < NC; ++x) acc[x] = fmaf(pt, vn[x], acc[x]);
    }
    storec<false, NC>(p.o, (size_t)r * d + col, acc);
}

template <bool ANC>
int cached_self_attn(CachedAttnParams<ANC> p, int dh, bool f32, hipStream_t st) {
    const char* who = ANC ? "beam self-attention" : "cached self-attention";
    EGX_CHECK(p.t >= 0 && p.t < p.n_steps && p.n_steps <= GEN_MAX_STEPS, "%s: step %d of %d (at most %d)", who, p.t, p.n_steps, GEN_MAX_STEPS);
    int W = 1;
    if constexpr (ANC) {
        EGX_CHECK(p.W >= 1 && p.W <= BEAM_MAX_W, "%s: W = %d (1..%d)", who, p.W, BEAM_MAX_W);
        W = p.W;
    }
    p.scale = 1.f / sqrtf((float)dh);
    const dim3 grid(cdiv(p.B * W * p.H, 4)), block(256);
    if (dh == 512 && !f32) hipLaunchKernelGGL((cached_self_attn_bighead_kernel<512, false, ANC>), grid, block, 0, st, p);
    else if (dh == 256 && !f32) hipLaunchKernelGGL((cached_self_attn_bighead_kernel<256, false, ANC>), grid, block, 0, st, p);
    else if (dh == 512) hipLaunchKernelGGL((cached_self_attn_bighead_kernel<512, true, ANC>), grid, block, 0, st, p);
    else if (dh == 256) hipLaunchKernelGGL((cached_self_attn_bighead_kernel<256, true, ANC>), grid, block, 0, st, p);
    else if (dh == 64 && !f32) hipLaunchKernelGGL((cached_self_attn_kernel<64, false, ANC>), grid, block, 0, st, p);
    else if (dh == 32 && !f32) hipLaunchKernelGGL((cached_self_attn_kernel<32, false, ANC>), grid, block, 0, st, p);
    else if (dh == 64) hipLaunchKernelGGL((cached_self_attn_kernel<64, true, ANC>), grid, block, 0, st, p);
    else if (dh == 32) hipLaunchKernelGGL((cached_self_attn_kernel<32, true, ANC>), grid, block, 0, st, p);
    else EGX_CHECK(false, "%s: head dim %d (32, 64, 256 or 512)", who, dh);
    EGX_LAUNCH_CHECK();
    return 0;
}

// The greedy head of one step: logits = x fc_w^T + fc_b in fp32 for GH_CLIPS clips per workgroup (fc_w streams once per workgroup; GH_WAVES
// waves, each with GH_ROWS vocabulary rows in flight per pass; the clips' rows in LDS), then one wave per clip: argmax (lowest index on ties; a NaN never wins), the token to tokens_out,
// the logits to logits_out when given, and the next step's input row emb[tok] * scale + pe_next as fp32 and bf16 (dec_embed_kernel's
// expression). pe_next null: the last step. With a word list (words, n_words) the head computes the listed rows only and every other logit
// is -inf: the argmax runs over the set.
constexpr int GH_CLIPS = 4, GH_WAVES = 8, GH_ROWS = 4, GEN_MAX_VOCAB = 1024;
struct GenHeadParams {
    const float* x; const float* fc_w; const float* fc_b; const float* emb; const float* pe_next;
    int64_t* tok; int tok_stride;               // clip b's token of this step at tok[b * tok_stride]
    float* logits;                              // (B, V) rows of this step, or null
    float* x32; bf16_t* x16;                    // (B, d): next step's input rows
    int B, d, V;
    float scale;
    const int32_t* words; int n_words;          // the step's word list (ascending indices, the count by value), or null: every word
};
// The fp32 vocabulary head of R target rows held in LDS (sx [R][d]) -> sl [R][V] = x fc_w^T + fc_b, shared by the greedy and the beam
// head: GH_WAVES waves, each with GH_ROWS vocabulary rows in flight per pass; per (vocabulary row, target row) one explicit fma chain over
// the lane's columns, then the wave sum. A row's logits depend on neither R nor its slot r. LISTED: entry k of the pass is vocabulary row
// list[k] (clamped to 0 .. V - 1), k < nv: only the listed rows of fc_w are read, and a listed word's logit is the chain and wave sum the
// unlisted loop runs for it: the same bits. Not LISTED: nv = V and entry k is row k.
template <int R, bool LISTED>
__device__ __forceinline__ void head_logits_rows(const float* fc_w, const float* fc_b, const float* sx, float* sl,
                                                 int d, int V, const int32_t* list, int nv, int lane, int wave) {
    // GH_ROWS vocabulary rows per wave and pass: their fc_w loads and wave reductions are independent and overlap (one row at a time the loop
    // is a chain of load and shuffle latencies: 206 us per launch at V = 600, d = 512)
    for (int v0 = wave; v0 < nv; v0 += GH_WAVES * GH_ROWS) {
        float a[GH_ROWS][R];
        int vr[GH_ROWS];
#pragma unroll
        for (int u = 0; u < GH_ROWS; ++u) {
            const int k = v0 + u * GH_WAVES < nv ? v0 + u * GH_WAVES : v0;          // (an entry past the end re-reads entry v0; its sums are dropped)
            int v = k;
            if (LISTED) {
                v = __builtin_amdgcn_readfirstlane(list[k]);             // (k is the wave's: one scalar index, as the unlisted row is)
                v = v < 0 ? 0 : (v >= V ? V - 1 : v);
            }
            vr[u] = v;
#pragma unroll
            for (int r = 0; r < R; ++r) a[u][r] = 0.f;
        }
        for (int c = lane * 4; c < d; c += 256) {
            float4 w[GH_ROWS];
#pragma unroll
            for (int u = 0; u < GH_ROWS; ++u) w[u] = *reinterpret_cast<const float4*>(fc_w + (size_t)vr[u] * d + c);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 xv = *reinterpret_cast<const float4*>(sx + r * d + c);
                // one explicit fma chain per (row, clip): left to the compiler's contraction (and its packed fp32 pairs) the clips of a
                // workgroup rounded differently by their slot, and permuting a batch moved logits by an ulp
#pragma unroll
                for (int u = 0; u < GH_ROWS; ++u)
                    a[u][r] = fmaf(w[u].w, xv.w, fmaf(w[u].z, xv.z, fmaf(w[u].y, xv.y, fmaf(w[u].x, xv.x, a[u][r]))));
            }
        }
#pragma unroll
        for (int u = 0; u < GH_ROWS; ++u) {
            const bool on = v0 + u * GH_WAVES < nv;
            const int v = vr[u];
            const float bias = fc_b && on ? fc_b[v] : 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float sum = wave_sum(a[u][r]);
                if (lane == 0 && on) sl[r * V + v] = sum + bias;
            }
        }
    }
}
// Every thread of the workgroup calls it. list null: sl = the logits of all V words. list given: the `count` (clamped to 0 .. V) listed
// words' logits, every other entry of sl -inf (filled first, behind a barrier of its own: the argmax, log-softmax and ranking read sl whole).
template <int R>
__device__ __forceinline__ void head_logits(const float* fc_w, const float* fc_b, const float* sx, float* sl, int d, int V,
                                            const int32_t* list, int count, int lane, int wave) {
    if (list) {
        for (int i = threadIdx.x; i < R * V; i += 64 * GH_WAVES) sl[i] = -INFINITY;
        __syncthreads();
        head_logits_rows<R, true>(fc_w, fc_b, sx, sl, d, V, list, count < 0 ? 0 : (count > V ? V : count), lane, wave);
    } else {
        head_logits_rows<R, false>(fc_w, fc_b, sx, sl, d, V, nullptr, V, lane, wave);
    }
}

__global__ __launch_bounds__(64 * GH_WAVES) void gen_head_kernel(GenHeadParams p) {
    extern __shared__ __align__(16) float gh_sm[];
    float* sx = gh_sm;                          // [GH_CLIPS][d]
    float* sl = gh_sm + GH_CLIPS * p.d;         // [GH_CLIPS][V]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = p.d, V = p.V;
    const int b0 = blockIdx.x * GH_CLIPS, nb = p.B - b0 < GH_CLIPS ? p.B - b0 : GH_CLIPS;
    for (int i = tid * 4; i < GH_CLIPS * d; i += 256 * GH_WAVES) {
        const int r = i / d;
        float4 v = make_float4(0, 0, 0, 0);
        if (r < nb) v = *reinterpret_cast<const float4*>(p.x + (size_t)b0 * d + i);
        *reinterpret_cast<float4*>(sx + i) = v;
    }
    __syncthreads();
    head_logits<GH_CLIPS>(p.fc_w, p.fc_b, sx, sl, d, V, p.words, p.n_words, lane, wave);
    __syncthreads();
    if (wave >= nb) return;
    const int b = b0 + wave;
    const float* row = sl + wave * V;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {        // ascending within a lane: `>` keeps the lowest index
        float x = row[v];
        if (!(x == x)) x = -INFINITY;
        if (x > best || idx == 0x7fffffff) { best = x; idx = v; }
        if (p.logits) p.logits[(size_t)b * V + v] = row[v];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane == 0) p.tok[(size_t)b * p.tok_stride] = (int64_t)idx;
    if (p.pe_next) {
        const float scale = p.scale;
        for (int c = lane * 4; c < d; c += 256) {
            const float4 e = *reinterpret_cast<const float4*>(p.emb + (size_t)idx * d + c);
            const float4 pp = *reinterpret_cast<const float4*>(p.pe_next + c);
            float o[4] = {e.x * scale + pp.x, e.y * scale + pp.y, e.z * scale + pp.z, e.w * scale + pp.w};
            *reinterpret_cast<float4*>(p.x32 + (size_t)b * d + c) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<uint2*>(p.x16 + (size_t)b * d + c) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        }
    }
}

struct GLayer { DecW w; size_t kv, cache; };

// The host checks of a token schedule (egx_decoder_generate_sched / egx_decoder_beam_sched), before any device work: period rows (0: no
// schedule), counts a HOST int[period] with every count in 1 .. vocab, words the DEVICE int32[period][vocab] table (not read here). W > 0:
// beam search, whose step 0 has only counts[0] continuations of the one live slot.
constexpr int SCHED_MAX_PERIOD = 64;
int check_sched(const char* who, int period, const int* counts, const int32_t* words, int vocab, int W) {
    EGX_CHECK(period >= 0 && period <= SCHED_MAX_PERIOD, "%s: period = %d (0..%d)", who, period, SCHED_MAX_PERIOD);
    if (period == 0) return 0;
    EGX_CHECK(counts && words, "%s: period = %d with a null counts or words", who, period);
    for (int p = 0; p < period; ++p)
        EGX_CHECK(counts[p] >= 1 && counts[p] <= vocab, "%s: counts[%d] = %d (1..vocab = %d)", who, p, counts[p], vocab);
    EGX_CHECK(W <= counts[0], "%s: W = %d exceeds counts[0] = %d (at step 0 only slot 0 is live: the step has only counts[0] continuations)",
              who, W, counts[0]);
    return 0;
}

// The plan of one cached-step call (greedy, beam search, teacher-forced): egx_decoder_generate's layout over M = B * rows target rows per
// step (rows per clip: 1, W or R; the memory and its K | V stay B * S rows). Every per-row buffer except greedy's LN statistics takes a
// multiple of 256 bytes per row, so the beam and forced workspaces are exactly linear in M and in n_steps (the caches and the slabs only).
struct StepPlan {
    int B, rows, n, S, d, H, dff, L, V;
    size_t M, Nm;
    size_t zero, mem16, x32, x16, qkv32, qkv16, sa, res, st, x1_32, x1_16, q, ca, x2_32, x2_16, hid, xL32;
    size_t xin32, score, anc[2], hist[2];       // a call's own buffers, taken behind the shared layout (beam_plan, forced_plan)
    GLayer layer[16];
    size_t bytes;                               // the running total: take(pl.bytes, ...) appends
};

// The checks every cached-step entry point and workspace query opens with, under its own name; the call's own range checks follow.
int step_checks(const char* who, const egx_dec_config* c, int n_steps) {
    EGX_CHECK(c, "null decoder config");
    EGX_CHECK(c->p_drop == 0.f && c->p_pos == 0.f, "%s: inference only: p_drop and p_pos must be 0 (got %g, %g)", who, c->p_drop, c->p_pos);
    EGX_CHECK(n_steps >= 1 && n_steps <= GEN_MAX_STEPS, "%s: n_steps = %d (1..%d)", who, n_steps, GEN_MAX_STEPS);
    EGX_CHECK(c->vocab >= 1 && c->vocab <= GEN_MAX_VOCAB, "%s: vocab = %d (1..%d)", who, c->vocab, GEN_MAX_VOCAB);
    return 0;
}

// (beam and forced) B * rows target rows and B * S memory rows within the kernels' int indices; `letter` names the rows per clip
int step_rows_fit(const char* who, char letter, const egx_dec_config* c, int B, int rows) {
    EGX_CHECK((size_t)B * rows <= (size_t)0x7fffffff / (size_t)(3 * c->d_model) && (size_t)B * c->S <= (size_t)0x7fffffff / (size_t)(2 * c->d_model),
              "%s: B = %d with %c = %d, S = %d is too large", who, B, letter, rows, c->S);
    return 0;
}

// d, heads, d_ff, layers, S and compute: egx_decoder_fwd's limits with `rows` target rows per clip (cfg->sy is not read), then the layout.
// st_row: bytes of LN statistics per row (greedy 8, else 256); xL_steps: the steps whose last-layer rows are kept (1: a head per step).
int step_layout(const egx_dec_config* c, int B, int rows, int n_steps, size_t st_row, int xL_steps, StepPlan& pl) {
    {
        egx_dec_config one = *c;
        one.sy = rows;
        DPlan dp;
        if (make_dplan(&one, B, dp)) return 1;
    }
    memset(&pl, 0, sizeof(pl));
    pl.B = B; pl.rows = rows; pl.n = n_steps; pl.S = c->S; pl.d = c->d_model; pl.H = c->n_heads; pl.dff = c->d_ff; pl.L = c->n_layers; pl.V = c->vocab;
    pl.M = (size_t)B * rows; pl.Nm = (size_t)B * c->S;
    const size_t d = pl.d, dff = pl.dff, Nm = pl.Nm, M = pl.M;
    size_t& cur = pl.bytes;
    pl.zero = take(cur, 1024);
    pl.mem16 = take(cur, Nm * d * 2);
    for (int l = 0; l < pl.L; ++l) {
        GLayer& o = pl.layer[l];
        o.w.sa_in = l ? take(cur, 3 * d * d * 2) : 0;      // (layer 0's in-projection runs in fp32 on the caller's weight)
        o.w.sa_o = take(cur, d * d * 2); o.w.q = take(cur, d * d * 2); o.w.kv = take(cur, 2 * d * d * 2); o.w.ca_o = take(cur, d * d * 2);
        o.w.w1 = take(cur, dff * d * 2); o.w.w2 = take(cur, dff * d * 2);
        o.kv = take(cur, Nm * 2 * d * 2);
        o.cache = take(cur, M * n_steps * 2 * d * (l ? 2 : 4));
    }
    pl.x32 = take(cur, M * d * 4); pl.x16 = take(cur, M * d * 2);
    pl.qkv32 = take(cur, M * 3 * d * 4); pl.qkv16 = take(cur, M * 3 * d * 2); pl.sa = take(cur, M * d * 2);
    pl.res = take(cur, M * d * 4); pl.st = take(cur, M * st_row);
    pl.x1_32 = take(cur, M * d * 4); pl.x1_16 = take(cur, M * d * 2); pl.q = take(cur, M * d * 2); pl.ca = take(cur, M * d * 2);
    pl.x2_32 = take(cur, M * d * 4); pl.x2_16 = take(cur, M * d * 2); pl.hid = take(cur, M * dff * 2);
    pl.xL32 = take(cur, M * xL_steps * d * 4);
    return 0;
}

// One cached-step call in flight, what the three decoders share: begin(), the caller's input kernel, fork_kv(), then layers() per step and
// joined() behind the last one. The caller keeps its input kernel, its loop over t and its head. From fork_kv() on, `sj` joins the side
// stream on every error return.
struct StepRun {
    const egx_dec_config* cfg; const StepPlan& pl; const egx_dec_layer* lw; void* ws; hipStream_t st;
    WideRun r;                  // no dropout, no keys: inference
    SideStream& SS; SideJoin sj; bool side = false;
    StepRun(const egx_dec_config* c, const StepPlan& p, const egx_dec_layer* layers, void* workspace, hipStream_t s)
        : cfg(c), pl(p), lw(layers), ws(workspace), st(s), SS(side_stream()), sj(SS, s) {
        r.saved = (char*)ws; r.st = st; r.zero = r.sv<char>(pl.zero); r.ln_eps = cfg->ln_eps;
    }

    // the zero page, the memory -> bf16, every weight -> bf16 once (no transposed copies: nothing runs backward), one launch
    int begin(const float* memory) {
        EGX_HIP(hipMemsetAsync(r.sv<char>(pl.zero), 0, 1024, st));
        if (wide_cast(memory, (int)pl.Nm, pl.d, pl.d, r.sv<bf16_t>(pl.mem16), nullptr, st)) return 1;
        WideCastBatch cb;
        for (int l = 0; l < pl.L; ++l)
            if (dec_cast_layer(cb, r, lw[l], pl.layer[l].w, nullptr, l == 0, pl.d, pl.dff)) return 1;
        return wide_cast_flush(cb, st);
    }

    // the memory's K | V, once per layer and per CLIP (B * S rows): on the side stream beside step 0 (eager), on the caller's stream under capture
    int fork_kv() {
        const int d = pl.d;
        side = side_wanted(SS, st);
        if (side) {
            if (SS.order(st, SS.s)) return 1;
            sj.forked = true;
        }
        for (int l = 0; l < pl.L; ++l) {
            const GLayer& o = pl.layer[l];
            if (r.nt_on(side ? SS.s : st, r.sv<bf16_t>(pl.mem16), r.sv<bf16_t>(o.w.kv), (int)pl.Nm, 2 * d, d, lw[l].ca_in_b + d, nullptr, r.sv<bf16_t>(o.kv), 0,
                        WideDrop(), nullptr)) return 1;
            if (side) EGX_HIP(hipEventRecord(SS.kv_ev[l], SS.s));
        }
        return 0;
    }

    // Step t's M new rows through the layers (decoder_layer_fwd over the one shared buffer set). xin: layer 0's fp32 input rows (and the
    // residual of its out-projection); xL: where the last layer's LN3 writes; self_attn(qkv, cache, o, f32, t, st): the call's cached
    // self-attention of one layer; attn_out, when given, (L, n_steps, B, S): every layer's cross-attention is followed by one
    // dec_cross_weights_kernel launch on the same q and k.
    template <class SelfAttn>
    int layers(int t, const float* xin, float* xL, SelfAttn&& self_attn, float* attn_out) {
        const int d = pl.d, dh = d / pl.H;
        auto self = [&](int l, const DecLayerView& v, bool f32) -> int {
            return self_attn(f32 ? (const void*)v.qkv32 : (const void*)v.qkv16, r.sv<char>(pl.layer[l].cache), v.sa_out.a16, f32, t, st);
        };
        // cross-attention of the clip's new rows onto its S memory rows: dec_attn with Sq = the rows per clip
        auto cross = [&](int l, const DecLayerView& v) -> int {
            if (side && t == 0) EGX_HIP(hipStreamWaitEvent(st, SS.kv_ev[l], 0));
            const bf16_t* kv = r.sv<bf16_t>(pl.layer[l].kv);
            const DecAttnParams a = cross_attn_params(v.q, kv, v.ca_out.a16, d, pl.B, pl.H, pl.rows, pl.S);
            if (dec_attn<false>(a, dh, false, st)) return 1;
            if (!attn_out) return 0;
            // (egx_decoder_generate_attn, one row per clip) this step's head-averaged weights of the layer: attn_out[l][t] (B, S)
            CrossWParams cw;
            memset(&cw, 0, sizeof(cw));
            cw.q = a.q; cw.ldq = d; cw.k = kv; cw.ldk = 2 * d; cw.out = attn_out + ((size_t)l * pl.n + t) * pl.B * pl.S; cw.ldo = pl.S;
            cw.B = pl.B; cw.H = pl.H; cw.Sq = 1; cw.Sk = pl.S;
            return cross_weights(cw, dh, false, st);
        };
        float* const res[3] = {r.sv<float>(pl.res), r.sv<float>(pl.res), r.sv<float>(pl.res)};
        float* const stats[3] = {r.sv<float>(pl.st), r.sv<float>(pl.st), r.sv<float>(pl.st)};
        for (int l = 0; l < pl.L; ++l) {
            const bool last = l + 1 == pl.L;
            DecLayerView v;
            v.x32 = l == 0 ? xin : r.sv<float>(pl.x32); v.x16 = r.sv<bf16_t>(pl.x16);
            v.qkv32 = r.sv<float>(pl.qkv32); v.qkv16 = r.sv<bf16_t>(pl.qkv16); v.q = r.sv<bf16_t>(pl.q);
            dec_view_sublayers(v, r, lw[l], pl.layer[l].w, nullptr, d, pl.dff, r.sv<bf16_t>(pl.sa), r.sv<bf16_t>(pl.ca), r.sv<bf16_t>(pl.hid), res, stats,
                               r.sv<float>(pl.x1_32), r.sv<bf16_t>(pl.x1_16), r.sv<float>(pl.x2_32), r.sv<bf16_t>(pl.x2_16),
                               last ? xL : r.sv<float>(pl.x32), last ? nullptr : r.sv<bf16_t>(pl.x16));
            if (decoder_layer_fwd(r, lw[l], v, l, (int)pl.M, d, self, cross)) return 1;
        }
        return 0;
    }

    // behind the last step: joined already, every layer's step-0 cross-attention waited for its kv_ev, the last side-stream operation
    void joined() { sj.forked = false; }
};

// the cached self-attention of rows that each read their own history (greedy, forced): the cached self-attention without ancestry over the M rows
auto own_history_attn(const StepPlan& pl) {
    return [&pl](const void* qkv, void* cache, bf16_t* o, bool f32, int t, hipStream_t st) -> int {
        GenAttnParams a;
        a.qkv = qkv; a.cache = cache; a.o = o;
        a.B = (int)pl.M; a.H = pl.H; a.d = pl.d; a.t = t; a.n_steps = pl.n; a.scale = 0.f;
        return cached_self_attn<false>(a, pl.d / pl.H, f32, st);
    };
}

// The greedy and the forced head keep GH_CLIPS rows of d inputs and V logits in dynamic LDS and set no limit of their own on the launch: the
// default 64 KiB must hold them (49152 bytes at d = 2048, V = 1024, the widest configuration step_layout and step_checks let through)
constexpr int GEN_HEAD_LDS_LIMIT = 64 * 1024;
size_t gen_head_lds(int d, int V) { return (size_t)GH_CLIPS * ((size_t)d + V) * sizeof(float); }
int gen_head_fits(const char* who, int d, int V) {
    EGX_CHECK(gen_head_lds(d, V) <= (size_t)GEN_HEAD_LDS_LIMIT, "%s: the head needs %zu bytes of LDS for d = %d, V = %d (at most %d)", who, gen_head_lds(d, V), d,
              V, GEN_HEAD_LDS_LIMIT);
    return 0;
}

int generate_plan(const egx_dec_config* c, int B, int n_steps, StepPlan& pl) {
    if (step_checks("egx_decoder_generate", c, n_steps)) return 1;
    if (step_layout(c, B, 1, n_steps, 8, 1, pl)) return 1;
    return gen_head_fits("egx_decoder_generate", pl.d, pl.V);
}

// The one body of egx_decoder_generate (period = 0), egx_decoder_generate_sched and egx_decoder_generate_attn: step t's head takes row
// t % period of the schedule; with attn_out (L, n_steps, B, S) every layer's cross-attention of a step is followed by one
// dec_cross_weights_kernel launch on the same q and k (attn_out null: the launches of the calls without it, nothing else).
int generate_run(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
                 const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int64_t* tokens_out,
                 float* logits_out, void* workspace, void* stream, int period, const int* counts, const int32_t* words, float* attn_out) {
    StepPlan pl;
    if (generate_plan(cfg, B, n_steps, pl)) return 1;
    if (check_sched("egx_decoder_generate_sched", period, counts, words, pl.V, 0)) return 1;
    EGX_CHECK(start && memory && emb && pe && layers && fc_w && fc_b && tokens_out && workspace, "egx_decoder_generate: null pointer argument");
    EGX_CHECK(pe_stride >= pl.d && pe_stride % 4 == 0, "egx_decoder_generate: pe_stride = %d (>= d_model, a multiple of 4)", pe_stride);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    const int d = pl.d;
    StepRun run(cfg, pl, layers, ws, st);
    if (run.begin(memory)) return 1;
    // step 0's input rows: emb[start] * sqrt(d) + pe[0]
    float* x32 = at<float>(ws, pl.x32);
    bf16_t* x16 = at<bf16_t>(ws, pl.x16);
    hipLaunchKernelGGL(dec_embed_kernel, dim3((unsigned)(((size_t)B * (d / 4) + 255) / 256)), dim3(256), 0, st, start, emb, pe, pe_stride,
                       sqrtf((float)d), x32, x16, B, 1, d, pl.V, (uint64_t)0, (uint32_t)0, 1.f);
    EGX_LAUNCH_CHECK();
    if (run.fork_kv()) return 1;
    for (int t = 0; t < n_steps; ++t) {
        if (run.layers(t, x32, at<float>(ws, pl.xL32), own_history_attn(pl), attn_out)) return 1;
        GenHeadParams hp;
        hp.x = cat<float>(ws, pl.xL32); hp.fc_w = fc_w; hp.fc_b = fc_b; hp.emb = emb;
        hp.pe_next = t + 1 < n_steps ? pe + (size_t)(t + 1) * pe_stride : nullptr;
        hp.tok = tokens_out + t; hp.tok_stride = n_steps;
        hp.logits = logits_out ? logits_out + (size_t)t * B * pl.V : nullptr;
        hp.x32 = x32; hp.x16 = x16; hp.B = B; hp.d = d; hp.V = pl.V; hp.scale = sqrtf((float)d);
        hp.words = period ? words + (size_t)(t % period) * pl.V : nullptr; hp.n_words = period ? counts[t % period] : 0;
        hipLaunchKernelGGL(gen_head_kernel, dim3(cdiv(B, GH_CLIPS)), dim3(64 * GH_WAVES), gen_head_lds(d, pl.V), st, hp);
        EGX_LAUNCH_CHECK();
    }
    run.joined();
    return 0;
}

}  // namespace

extern "C" {

int egx_decoder_generate_workspace(const egx_dec_config* cfg, int B, int n_steps, size_t* bytes) {
    StepPlan pl;
    if (generate_plan(cfg, B, n_steps, pl)) return 1;
    if (bytes) *bytes = pl.bytes;
    return 0;
}

int egx_decoder_generate(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
                         const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int64_t* tokens_out,
                         float* logits_out, void* workspace, void* stream) {
    return generate_run(cfg, start, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, n_steps, tokens_out, logits_out, workspace, stream, 0,
                        nullptr, nullptr, nullptr);
}

int egx_decoder_generate_sched(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe,
                               int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps,
                               int64_t* tokens_out, float* logits_out, void* workspace, void* stream, int period, const int* counts,
                               const int32_t* words) {
    return generate_run(cfg, start, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, n_steps, tokens_out, logits_out, workspace, stream,
                        period, counts, words, nullptr);
}

int egx_decoder_generate_attn(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe,
                              int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps,
                              int64_t* tokens_out, float* logits_out, void* workspace, void* stream, int period, const int* counts,
                              const int32_t* words, float* attn_out) {
    EGX_CHECK(attn_out, "egx_decoder_generate_attn: null attn_out (egx_decoder_generate / egx_decoder_generate_sched are the calls without it)");
    EGX_CHECK(!(cfg && cfg->n_heads > 0 && cfg->d_model % cfg->n_heads == 0 && dec_attn_bighead_dim(cfg->d_model / cfg->n_heads)),
              "egx_decoder_generate_attn: head dim %d (16, 32, 64 or 128: the weights of the 256 / 512 class are not served)", cfg->d_model / cfg->n_heads);
    return generate_run(cfg, start, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, n_steps, tokens_out, logits_out, workspace, stream,
                        period, counts, words, attn_out);
}

}  // extern "C"

// ---- beam search with a K/V cache (egx_decoder_beam) ----
// egx_decoder_generate's step over B * W rows (row b * W + w: hypothesis slot w of clip b, decode()'s (B, sy) layout, so every row-wise stage
// and the cross-attention with Sq = W serve it unchanged) with two kernels of its own: the ANC instance of the cached self-attention reads a hypothesis'
// history through an ancestry table instead of gathering the cache, and the head ranks the W * V candidates of a clip and writes the next step's rows.
namespace {

constexpr int BEAM_LDS_LIMIT = 64 * 1024;

// step 0's rows: x32 / x16 [b * W + w] = emb[start[b]] * scale + pe[0] (dec_embed_kernel's expression) for every slot, and the scores
// 0 for slot 0, -inf for the others: only slot 0 is live
__global__ __launch_bounds__(256) void beam_init_kernel(const int64_t* __restrict__ start, const float* __restrict__ emb, const float* __restrict__ pe,
                                                        float scale, float* __restrict__ x32, bf16_t* __restrict__ x16, float* __restrict__ score,
                                                        int rows, int W, int d, int V) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // one float4 each
    if (i >= (size_t)rows * (d / 4)) return;
    const int row = (int)(i / (d / 4)), c = (int)(i % (d / 4)) * 4;
    const int64_t t = start[row / W];
    float4 e = make_float4(0, 0, 0, 0);
    if (t >= 0 && t < V) e = *reinterpret_cast<const float4*>(emb + (size_t)t * d + c);
    const float4 pp = *reinterpret_cast<const float4*>(pe + c);
    float o[4] = {e.x * scale + pp.x, e.y * scale + pp.y, e.z * scale + pp.z, e.w * scale + pp.w};
    *reinterpret_cast<float4*>(x32 + (size_t)row * d + c) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint2*>(x16 + (size_t)row * d + c) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
    if (c == 0) score[row] = row % W == 0 ? 0.f : -INFINITY;
}

// The beam head of one step, one workgroup per clip: the W rows' logits (head_logits, as the greedy head), per row the fp32 log-softmax
// and candidate scores score[w] + logp[w][v] in LDS, then W rounds of a block-wide arg-max with removal over the W * V candidates (ties to
// the lowest flat index w * V + v; a NaN ranks as -inf and never wins), then the survivors' token / parent / score, their ancestry and
// token histories copied from the parents' (double-buffered: a survivor reads another slot's row), and the next step's input rows
// emb[tok] * scale + pe_next. pe_next null: the last step. With a word list the other words' logits are -inf: exp gives them 0, so the
// log-softmax normalises over the set, and their candidates (-inf) lose to the W * n_words finite ones.
struct BeamHeadParams {
    const float* x; const float* fc_w; const float* fc_b; const float* emb; const float* pe_next;
    const float* score_in; float* score_out;            // (B, W); may alias: a clip's scores are read before the ranking, written after it
    const int* anc_in; int* anc_out;                    // (B, W, BEAM_DEPTH)
    const int64_t* hist_in; int64_t* hist_out;          // (B, W, ld): tokens 0 .. t of each hypothesis
    int hist_in_ld, hist_out_ld;
    int64_t* step_tok; int32_t* step_par; float* step_score;        // (B, W) of this step, or null
    float* step_logits;                                 // (B, W, V) of this step, or null
    float* x32; bf16_t* x16;                            // (B * W, d): next step's input rows
    int B, W, d, V, t;
    float scale;
    const int32_t* words; int n_words;                  // the step's word list as GenHeadParams', or null: every word
};
constexpr int BH_THREADS = 64 * GH_WAVES;
template <int R>
__global__ __launch_bounds__(BH_THREADS) void beam_head_kernel(BeamHeadParams p) {
    extern __shared__ __align__(16) float bh_sm[];
    float* sx = bh_sm;                          // [R][d]; free after the logits: the ranking's scratch
    float* sl = bh_sm + R * p.d;                // [R][V]: logits, then candidate scores (flat index w * V + v for the W live rows)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = p.d, V = p.V, W = p.W, t = p.t, b = blockIdx.x;
    const size_t r0 = (size_t)b * W;
    for (int i = tid * 4; i < R * d; i += 4 * BH_THREADS) {
        const int r = i / d;
        float4 v = make_float4(0, 0, 0, 0);
        if (r < W) v = *reinterpret_cast<const float4*>(p.x + r0 * d + i);
        *reinterpret_cast<float4*>(sx + i) = v;
    }
    __syncthreads();
    head_logits<R>(p.fc_w, p.fc_b, sx, sl, d, V, p.words, p.n_words, lane, wave);
    __syncthreads();
    float* rv = sx;                             // [2][GH_WAVES] the waves' bests of a round (by round parity)
    int* ri = reinterpret_cast<int*>(sx + 2 * GH_WAVES);
    float* selv = sx + 4 * GH_WAVES;            // [BEAM_MAX_W] the winners
    int* seli = reinterpret_cast<int*>(sx + 4 * GH_WAVES + BEAM_MAX_W);
    if (wave < W) {                             // wave w: row w -> score[w] + log_softmax(logits[w]) in place
        float* row = sl + wave * V;
        const float prev = p.score_in[r0 + wave];
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) {
            const float x = row[v];
            if (p.step_logits) p.step_logits[(r0 + wave) * V + v] = x;
            if (x == x) m = fmaxf(m, x);
        }
        m = wave_max(m);
        float sum = 0.f;
        for (int v = lane; v < V; v += 64) {
            const float x = row[v];
            if (x == x) sum += expf(x - m);
        }
        const float lse = logf(wave_sum(sum));
        for (int v = lane; v < V; v += 64) {
            const float x = row[v];
            row[v] = x == x ? prev + ((x - m) - lse) : -INFINITY;
        }
    }
    __syncthreads();
    const int n = W * V;                        // <= 8192: candidate k of this thread is flat index tid + k * BH_THREADS, k < 16
    uint32_t removed = 0;
    for (int round = 0; round < W; ++round) {
        float best = -INFINITY;
        int idx = 0x7fffffff;
        for (int k = 0, i = tid; i < n; ++k, i += BH_THREADS) {     // ascending within a thread: `>` keeps the lowest index
            if ((removed >> k) & 1u) continue;
            float x = sl[i];
            if (!(x == x)) x = -INFINITY;
            if (x > best || idx == 0x7fffffff) { best = x; idx = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(idx, o, 64);
            if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
        }
        float* rvp = rv + (round & 1) * GH_WAVES;
        int* rip = ri + (round & 1) * GH_WAVES;
        if (lane == 0) { rvp[wave] = best; rip[wave] = idx; }
        __syncthreads();
        best = rvp[0]; idx = rip[0];
#pragma unroll
        for (int w = 1; w < GH_WAVES; ++w) {
            const float ob = rvp[w];
            const int oi = rip[w];
            if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
        }
        if (idx >= n) idx = 0;                  // (cannot happen: W <= W * V candidates are left in every round)
        if ((idx & (BH_THREADS - 1)) == tid) removed |= 1u << (idx / BH_THREADS);
        if (tid == 0) { selv[round] = best; seli[round] = idx; }
    }
    __syncthreads();
    if (tid < W) {
        const int flat = seli[tid], par = flat / V;
        p.score_out[r0 + tid] = selv[tid];
        if (p.step_tok) p.step_tok[r0 + tid] = (int64_t)(flat - par * V);
        if (p.step_par) p.step_par[r0 + tid] = par;
        if (p.step_score) p.step_score[r0 + tid] = selv[tid];
    }
    // survivor k: history rows 0 .. t - 1 from its parent, row t the parent's slot (ancestry) / the new token (history)
    for (int i = tid; i < W * (t + 1); i += BH_THREADS) {
        const int k = i / (t + 1), j = i - k * (t + 1);
        const int flat = seli[k], par = flat / V;
        p.anc_out[(r0 + k) * BEAM_DEPTH + j] = j < t ? p.anc_in[(r0 + par) * BEAM_DEPTH + j] : par;
        p.hist_out[(r0 + k) * p.hist_out_ld + j] = j < t ? p.hist_in[(r0 + par) * p.hist_in_ld + j] : (int64_t)(flat - par * V);
    }
    if (p.pe_next && wave < W) {
        const int flat = seli[wave], tok = flat - (flat / V) * V;
        const float scale = p.scale;
        for (int c = lane * 4; c < d; c += 256) {
            const float4 e = *reinterpret_cast<const float4*>(p.emb + (size_t)tok * d + c);
            const float4 pp = *reinterpret_cast<const float4*>(p.pe_next + c);
            float o[4] = {e.x * scale + pp.x, e.y * scale + pp.y, e.z * scale + pp.z, e.w * scale + pp.w};
            *reinterpret_cast<float4*>(p.x32 + (r0 + wave) * d + c) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<uint2*>(p.x16 + (r0 + wave) * d + c) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        }
    }
}

size_t beam_head_lds(int W, int d, int V) { return (size_t)(W <= 4 ? 4 : 8) * (d + V) * sizeof(float); }

int beam_head(const BeamHeadParams& p, hipStream_t st) {
    const size_t lds = beam_head_lds(p.W, p.d, p.V);
    EGX_CHECK(lds <= (size_t)BEAM_LDS_LIMIT, "beam head: %zu bytes of LDS for W = %d, d = %d, V = %d (at most %d)", lds, p.W, p.d, p.V, BEAM_LDS_LIMIT);
    if (p.W <= 4) hipLaunchKernelGGL(beam_head_kernel<4>, dim3(p.B), dim3(BH_THREADS), lds, st, p);
    else hipLaunchKernelGGL(beam_head_kernel<8>, dim3(p.B), dim3(BH_THREADS), lds, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

// The checks of the call and of the workspace query, then the shared layout over M = B * W target rows plus the beam's state.
int beam_plan(const egx_dec_config* c, int B, int n_steps, int W, StepPlan& pl) {
    if (step_checks("egx_decoder_beam", c, n_steps)) return 1;
    EGX_CHECK(W >= 1 && W <= BEAM_MAX_W, "egx_decoder_beam: W = %d (1..%d)", W, BEAM_MAX_W);
    EGX_CHECK(W <= c->vocab, "egx_decoder_beam: W = %d exceeds vocab = %d (a step has only vocab distinct continuations of the start token)", W, c->vocab);
    if (step_layout(c, B, W, n_steps, 256, 1, pl)) return 1;
    EGX_CHECK(beam_head_lds(W, c->d_model, c->vocab) <= (size_t)BEAM_LDS_LIMIT, "egx_decoder_beam: the head needs %zu bytes of LDS (at most %d)",
              beam_head_lds(W, c->d_model, c->vocab), BEAM_LDS_LIMIT);
    if (step_rows_fit("egx_decoder_beam", 'W', c, B, W)) return 1;
    pl.score = take(pl.bytes, pl.M * 256);
    for (int u = 0; u < 2; ++u) {
        pl.anc[u] = take(pl.bytes, pl.M * BEAM_DEPTH * sizeof(int));
        pl.hist[u] = take(pl.bytes, pl.M * BEAM_DEPTH * sizeof(int64_t));
    }
    return 0;
}

// The one body of egx_decoder_beam (period = 0) and egx_decoder_beam_sched: step t's head takes row t % period of the schedule.
int beam_run(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
             const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int W, int64_t* tokens_out,
             float* scores_out, int64_t* step_tokens, int32_t* step_parents, float* step_scores, float* step_logits, void* workspace,
             void* stream, int period, const int* counts, const int32_t* words) {
    StepPlan pl;
    if (beam_plan(cfg, B, n_steps, W, pl)) return 1;
    if (check_sched("egx_decoder_beam_sched", period, counts, words, pl.V, W)) return 1;
    EGX_CHECK(start && memory && emb && pe && layers && fc_w && fc_b && tokens_out && scores_out && workspace, "egx_decoder_beam: null pointer argument");
    EGX_CHECK(pe_stride >= pl.d && pe_stride % 4 == 0, "egx_decoder_beam: pe_stride = %d (>= d_model, a multiple of 4)", pe_stride);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    const int d = pl.d, M = (int)pl.M;
    StepRun run(cfg, pl, layers, ws, st);
    if (run.begin(memory)) return 1;
    float* x32 = at<float>(ws, pl.x32);
    bf16_t* x16 = at<bf16_t>(ws, pl.x16);
    float* score = at<float>(ws, pl.score);
    hipLaunchKernelGGL(beam_init_kernel, dim3((unsigned)(((size_t)M * (d / 4) + 255) / 256)), dim3(256), 0, st, start, emb, pe, sqrtf((float)d), x32,
                       x16, score, M, W, d, pl.V);
    EGX_LAUNCH_CHECK();
    if (run.fork_kv()) return 1;
    // a hypothesis' history is read through the ancestry table the previous step's head wrote
    auto self_attn = [&](const void* qkv, void* cache, bf16_t* o, bool f32, int t, hipStream_t s_) -> int {
        BeamAttnParams a;
        a.qkv = qkv; a.cache = cache; a.anc = cat<int>(ws, pl.anc[t & 1]); a.o = o;
        a.B = B; a.W = W; a.H = pl.H; a.d = d; a.t = t; a.n_steps = n_steps; a.scale = 0.f;
        return cached_self_attn<true>(a, d / pl.H, f32, s_);
    };
    for (int t = 0; t < n_steps; ++t) {
        const bool last_step = t + 1 == n_steps;
        if (run.layers(t, x32, at<float>(ws, pl.xL32), self_attn, nullptr)) return 1;
        BeamHeadParams hp;
        memset(&hp, 0, sizeof(hp));
        hp.x = cat<float>(ws, pl.xL32); hp.fc_w = fc_w; hp.fc_b = fc_b; hp.emb = emb;
        hp.pe_next = last_step ? nullptr : pe + (size_t)(t + 1) * pe_stride;
        hp.score_in = score; hp.score_out = last_step ? scores_out : score;
        hp.anc_in = cat<int>(ws, pl.anc[t & 1]); hp.anc_out = at<int>(ws, pl.anc[(t + 1) & 1]);
        hp.hist_in = cat<int64_t>(ws, pl.hist[t & 1]); hp.hist_in_ld = BEAM_DEPTH;
        hp.hist_out = last_step ? tokens_out : at<int64_t>(ws, pl.hist[(t + 1) & 1]); hp.hist_out_ld = last_step ? n_steps : BEAM_DEPTH;
        const size_t so = (size_t)t * M;
        hp.step_tok = step_tokens ? step_tokens + so : nullptr; hp.step_par = step_parents ? step_parents + so : nullptr;
        hp.step_score = step_scores ? step_scores + so : nullptr; hp.step_logits = step_logits ? step_logits + so * pl.V : nullptr;
        hp.x32 = x32; hp.x16 = x16; hp.B = B; hp.W = W; hp.d = d; hp.V = pl.V; hp.t = t; hp.scale = sqrtf((float)d);
        hp.words = period ? words + (size_t)(t % period) * pl.V : nullptr; hp.n_words = period ? counts[t % period] : 0;
        if (beam_head(hp, st)) return 1;
    }
    run.joined();
    return 0;
}

}  // namespace

extern "C" {

int egx_decoder_beam_workspace(const egx_dec_config* cfg, int B, int n_steps, int W, size_t* bytes) {
    StepPlan pl;
    if (beam_plan(cfg, B, n_steps, W, pl)) return 1;
    if (bytes) *bytes = pl.bytes;
    return 0;
}

int egx_decoder_beam(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
                     const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int W, int64_t* tokens_out,
                     float* scores_out, int64_t* step_tokens, int32_t* step_parents, float* step_scores, float* step_logits, void* workspace,
                     void* stream) {
    return beam_run(cfg, start, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, n_steps, W, tokens_out, scores_out, step_tokens, step_parents,
                    step_scores, step_logits, workspace, stream, 0, nullptr, nullptr);
}

int egx_decoder_beam_sched(const egx_dec_config* cfg, const int64_t* start, const float* memory, const float* emb, const float* pe, int pe_stride,
                           const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int n_steps, int W, int64_t* tokens_out,
                           float* scores_out, int64_t* step_tokens, int32_t* step_parents, float* step_scores, float* step_logits,
                           void* workspace, void* stream, int period, const int* counts, const int32_t* words) {
    return beam_run(cfg, start, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, n_steps, W, tokens_out, scores_out, step_tokens, step_parents,
                    step_scores, step_logits, workspace, stream, period, counts, words);
}

}  // extern "C"

// ---- teacher-forced decoding on the K/V-cached step (egx_decoder_forced) ----
// egx_decoder_generate's step over B * R rows (row b * R + r: target sequence r of clip b, as the beam's slots: the cross-attention runs with
// Sq = R on the clip's memory) with the next input row taken from the caller's tokens instead of the argmax: every input row is embedded in
// one launch up front, each step's last-layer rows go into an (n_steps, B * R, d) slab, and ONE head launch after the last step turns the
// slab into logits and log-probabilities. The validation step of HOI/tasks/multitask/video_task.py:601-617 and video_task_action.py:83-88
// (model(video, target[:, :-1], 'lta_verb') over 21 tokens) and the 40-token call of HOI/models/lta/lta_models_seqdecoder.py:175-179.
namespace {

constexpr int FORCED_MAX_R = DA_MAXQ;

// x32[t * M + m] = emb[tok[m * n + t]] * scale + pe[t] (dec_embed_kernel's expression; a token outside [0, V) embeds as the zero row):
// tokens are (M, n) row-major, the rows leave in step-major order so that step t reads M contiguous rows. Layer 0 reads the fp32 rows only.
__global__ __launch_bounds__(256) void forced_embed_kernel(const int64_t* __restrict__ tok, const float* __restrict__ emb, const float* __restrict__ pe,
                                                           int pe_stride, float scale, float* __restrict__ x32, int M, int n, int d, int V) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // one float4 each
    if (i >= (size_t)M * n * (d / 4)) return;
    const size_t row = i / (d / 4);                                    // output row t * M + m
    const int c = (int)(i % (d / 4)) * 4;
    const int t = (int)(row / M), m = (int)(row % M);
    const int64_t w = tok[(size_t)m * n + t];
    float4 e = make_float4(0, 0, 0, 0);
    if (w >= 0 && w < V) e = *reinterpret_cast<const float4*>(emb + (size_t)w * d + c);
    const float4 pp = *reinterpret_cast<const float4*>(pe + (size_t)t * pe_stride + c);
    *reinterpret_cast<float4*>(x32 + row * d + c) = make_float4(e.x * scale + pp.x, e.y * scale + pp.y, e.z * scale + pp.z, e.w * scale + pp.w);
}

// The vocabulary head over the slab, GH_CLIPS rows per workgroup: logits by head_logits<GH_CLIPS>, unlisted (a row's logits depend on
// neither its slot nor its neighbours: the bits gen_head_kernel computes for the row), then one wave per row: the logits row to logits_out
// when given, and with targets logprob = logit[target] - max - log(sum exp(logit - max)) in fp32, the sum lane-strided ascending, then
// the xor butterfly. A target outside [0, V) gives exactly 0.0; a NaN logit reaches the sum and so the row's logprob.
struct ForcedHeadParams {
    const float* x;             // (n * M, d): row t * M + m
    const float* fc_w; const float* fc_b;
    const int64_t* targets;     // (M, n) or null
    float* logits;              // (n * M, V) or null
    float* logprob;             // (M, n) or null
    int rows, M, n, d, V;
};
__global__ __launch_bounds__(64 * GH_WAVES) void forced_head_kernel(ForcedHeadParams p) {
    extern __shared__ __align__(16) float fh_sm[];
    float* sx = fh_sm;                          // [GH_CLIPS][d]
    float* sl = fh_sm + GH_CLIPS * p.d;         // [GH_CLIPS][V]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int d = p.d, V = p.V;
    const int g0 = blockIdx.x * GH_CLIPS, nb = p.rows - g0 < GH_CLIPS ? p.rows - g0 : GH_CLIPS;
    for (int i = tid * 4; i < GH_CLIPS * d; i += 256 * GH_WAVES) {
        const int r = i / d;
        float4 v = make_float4(0, 0, 0, 0);
        if (r < nb) v = *reinterpret_cast<const float4*>(p.x + (size_t)g0 * d + i);
        *reinterpret_cast<float4*>(sx + i) = v;
    }
    __syncthreads();
    head_logits<GH_CLIPS>(p.fc_w, p.fc_b, sx, sl, d, V, nullptr, 0, lane, wave);
    __syncthreads();
    if (wave >= nb) return;
    const int g = g0 + wave;
    const float* row = sl + wave * V;
    float mx = -INFINITY;
    for (int v = lane; v < V; v += 64) {
        const float x = row[v];
        if (p.logits) p.logits[(size_t)g * V + v] = x;
        mx = fmaxf(mx, x);                      // (a NaN is skipped here and caught by the sum)
    }
    if (!p.logprob) return;
    mx = wave_max(mx);
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += expf(row[v] - mx);
    const float lse = logf(wave_sum(sum));
    if (lane == 0) {
        const int t = g / p.M, m = g - t * p.M;
        const size_t o = (size_t)m * p.n + t;
        const int64_t w = p.targets[o];
        p.logprob[o] = w >= 0 && w < V ? (row[(int)w] - mx) - lse : 0.f;
    }
}

// The checks of the call and of the workspace query, then the shared layout over M = B * R target rows with the last layer's rows of every
// step kept, plus the (n_steps, M, d) fp32 slab of embedded input rows.
int forced_plan(const egx_dec_config* c, int B, int R, int n_steps, StepPlan& pl) {
    if (step_checks("egx_decoder_forced", c, n_steps)) return 1;
    EGX_CHECK(R >= 1 && R <= FORCED_MAX_R, "egx_decoder_forced: R = %d (1..%d)", R, FORCED_MAX_R);
    if (step_layout(c, B, R, n_steps, 256, n_steps, pl)) return 1;
    if (gen_head_fits("egx_decoder_forced", pl.d, pl.V)) return 1;
    if (step_rows_fit("egx_decoder_forced", 'R', c, B, R)) return 1;
    pl.xin32 = take(pl.bytes, pl.M * n_steps * pl.d * 4);
    return 0;
}

int forced_run(const egx_dec_config* cfg, const int64_t* tokens, const int64_t* targets, const float* memory, const float* emb, const float* pe,
               int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int R, int n_steps, float* logits_out,
               float* logprob_out, void* workspace, void* stream) {
    StepPlan pl;
    if (forced_plan(cfg, B, R, n_steps, pl)) return 1;
    EGX_CHECK(logits_out || logprob_out, "egx_decoder_forced: logits_out and logprob_out are both null: nothing to compute");
    EGX_CHECK(!logprob_out || targets, "egx_decoder_forced: logprob_out without targets");
    EGX_CHECK(tokens && memory && emb && pe && layers && fc_w && fc_b && workspace, "egx_decoder_forced: null pointer argument");
    EGX_CHECK(pe_stride >= pl.d && pe_stride % 4 == 0, "egx_decoder_forced: pe_stride = %d (>= d_model, a multiple of 4)", pe_stride);
    hipStream_t st = (hipStream_t)stream;
    void* ws = workspace;
    const int d = pl.d, M = (int)pl.M;
    StepRun run(cfg, pl, layers, ws, st);
    if (run.begin(memory)) return 1;
    // every step's input rows in one launch: all B * R * n_steps tokens are known up front
    hipLaunchKernelGGL(forced_embed_kernel, dim3((unsigned)(((size_t)M * n_steps * (d / 4) + 255) / 256)), dim3(256), 0, st, tokens, emb, pe, pe_stride,
                       sqrtf((float)d), at<float>(ws, pl.xin32), M, n_steps, d, pl.V);
    EGX_LAUNCH_CHECK();
    if (run.fork_kv()) return 1;
    // step t: layer 0 reads the caller's tokens of step t, the last layer writes row block t of the slab
    for (int t = 0; t < n_steps; ++t)
        if (run.layers(t, cat<float>(ws, pl.xin32) + (size_t)t * M * d, at<float>(ws, pl.xL32) + (size_t)t * M * d, own_history_attn(pl), nullptr)) return 1;
    run.joined();
    ForcedHeadParams hp;
    hp.x = cat<float>(ws, pl.xL32); hp.fc_w = fc_w; hp.fc_b = fc_b; hp.targets = targets; hp.logits = logits_out; hp.logprob = logprob_out;
    hp.rows = M * n_steps; hp.M = M; hp.n = n_steps; hp.d = d; hp.V = pl.V;
    hipLaunchKernelGGL(forced_head_kernel, dim3(cdiv(hp.rows, GH_CLIPS)), dim3(64 * GH_WAVES), gen_head_lds(d, pl.V), st, hp);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int egx_decoder_forced_workspace(const egx_dec_config* cfg, int B, int R, int n_steps, size_t* bytes) {
    StepPlan pl;
    if (forced_plan(cfg, B, R, n_steps, pl)) return 1;
    if (bytes) *bytes = pl.bytes;
    return 0;
}

int egx_decoder_forced(const egx_dec_config* cfg, const int64_t* tokens, const int64_t* targets, const float* memory, const float* emb,
                       const float* pe, int pe_stride, const egx_dec_layer* layers, const float* fc_w, const float* fc_b, int B, int R,
                       int n_steps, float* logits_out, float* logprob_out, void* workspace, void* stream) {
    return forced_run(cfg, tokens, targets, memory, emb, pe, pe_stride, layers, fc_w, fc_b, B, R, n_steps, logits_out, logprob_out, workspace, stream);
}

}  // extern "C"

// ---- unit hooks of the decoder's attention (ABI v29): exactly the launches decoder_fwd_run / decoder_bwd_run and the cached step's
// cross-attention make (dec_attn), on the caller's operands. Every check runs before the launch.
namespace {
int dec_attn_hook(const char* who, const egx_dec_attn_args* a, bool bwd) {
    EGX_CHECK(a, "%s: null arguments", who);
    EGX_CHECK(a->p_drop >= 0.f && a->p_drop <= 1.f, "%s: dropout probability %g outside [0, 1]", who, (double)a->p_drop);
    EGX_CHECK(a->B >= 1 && a->H >= 1 && a->Sq >= 1 && a->Sk >= 1, "%s: B = %d, H = %d, Sq = %d, Sk = %d", who, a->B, a->H, a->Sq, a->Sk);
    EGX_CHECK(a->dh == 32 || a->dh == 64 || dec_attn_bighead_dim(a->dh), "%s: head dim %d (32 or 64; 256 / 512 with Sk <= %d)", who, a->dh, DA_BIGHEAD_MAXK);
    DecAttnParams p;
    memset(&p, 0, sizeof(p));
    p.q = a->q; p.k = a->k; p.v = a->v; p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.o = (bf16_t*)a->o; p.ldo = a->ldo;
    p.d_o = (const bf16_t*)a->d_o; p.dq = a->dq; p.dk = a->dk; p.dv = a->dv;
    p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.Sk = a->Sk; p.causal = a->causal ? 1 : 0;
    if (a->p_drop > 0.f) {
        p.drop_key = site_key(a->seed, 0x40u + a->layer, a->site);
        p.drop_thresh = drop_threshold(a->p_drop); p.drop_inv = a->p_drop < 1.f ? 1.f / (1.f - a->p_drop) : 0.f;
    }
    if (!dec_attn_bighead_dim(a->dh)) {       // (the big-head class checks its own operands: dec_attn_bighead)
        const int w = a->H * a->dh;
        EGX_CHECK(a->Sq <= DA_MAXQ && a->Sk <= DAL_MAXK && (!a->causal || a->Sq == a->Sk), "%s: Sq = %d (1..%d), Sk = %d (1..%d; causal: Sk = Sq)", who,
                  a->Sq, DA_MAXQ, a->Sk, DAL_MAXK);
        EGX_CHECK(p.q && p.k && p.v && (bwd ? p.d_o && p.dq && p.dk && p.dv : p.o != nullptr), "%s: null pointer argument", who);
        EGX_CHECK(p.ldq % 8 == 0 && p.ldk % 8 == 0 && p.ldv % 8 == 0 && p.ldo % 8 == 0 && p.ldq >= w && p.ldk >= w && p.ldv >= w && p.ldo >= w,
                  "%s: ldq = %d, ldk = %d, ldv = %d, ldo = %d (multiples of 8, >= H * head dim = %d)", who, p.ldq, p.ldk, p.ldv, p.ldo, w);
        EGX_CHECK((((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.o | (uintptr_t)p.d_o | (uintptr_t)p.dq | (uintptr_t)p.dk | (uintptr_t)p.dv) & 15) == 0,
                  "%s: pointers must be 16-byte aligned", who);
        EGX_CHECK(a->Sk <= DA_MAXK || (a->operands_bf16 && !a->causal), "%s: a memory of %d tokens needs bf16 operands", who, a->Sk);
    }
    hipStream_t st = (hipStream_t)a->stream;
    return bwd ? dec_attn<true>(p, a->dh, !a->operands_bf16, st) : dec_attn<false>(p, a->dh, !a->operands_bf16, st);
}
}  // namespace

extern "C" {

int egx_decoder_attention_fwd(const egx_dec_attn_args* a) { return dec_attn_hook("egx_decoder_attention_fwd", a, false); }
int egx_decoder_attention_bwd(const egx_dec_attn_args* a) { return dec_attn_hook("egx_decoder_attention_bwd", a, true); }

}  // extern "C"
