// The sequence decoder's attention launches (wide_decoder.hip: head dim 32 / 64; wide_decoder_bighead.hip: head dim 256 / 512): one
// parameter struct and the operand accessors both classes share.
#pragma once
#include "common.h"
#include "wide.h"

namespace egx {

constexpr int DA_MAXQ = 8, DA_MAXK = 64;
constexpr int DA_BIGHEAD_MAXK = WIDE_ATTN_BIGHEAD_MAX_S;         // keys of the head dim 256 / 512 class

__device__ __forceinline__ float bf_lo(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
__device__ __forceinline__ float bf1(bf16_t v) { return __builtin_bit_cast(float, (uint32_t)v << 16); }

struct DecAttnParams {
    const void* q; const void* k; const void* v; int ldq, ldk, ldv;           // rows b * Sq + i / b * Sk + j; head h at columns h * DH
    bf16_t* o; int ldo;                                                        // (q / k / v and their gradients: bf16, or fp32 with F32 = true)
    const bf16_t* d_o; void* dq; void* dk; void* dv;                           // backward (same strides as o / q / k / v)
    int B, H, Sq, Sk, causal;
    float scale;
    uint64_t drop_key; uint32_t drop_thresh; float drop_inv;
    // ragged memories (dec_attn_ragged_train, RAGGED kernels): the B clips of `clips`; clip c's Sk_c = mtab[2c + 1] keys are rows [mtab[2c], + Sk_c)
    // of k / v, its query / output rows c * Sq + i. Sk = the longest memory of the launch.
    const int* mtab; const int* clips;
};

// 8 consecutive elements of a q / k / v row as fp32
template <bool F32>
__device__ __forceinline__ void load8(const void* base, size_t idx, float (&o)[8]) {
    if constexpr (F32) {
        const float4 a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + idx);
        const float4 b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + idx + 4);
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
    } else {
        const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(base) + idx);
        o[0] = bf_lo(u.x); o[1] = bf_hi(u.x); o[2] = bf_lo(u.y); o[3] = bf_hi(u.y);
        o[4] = bf_lo(u.z); o[5] = bf_hi(u.z); o[6] = bf_lo(u.w); o[7] = bf_hi(u.w);
    }
}
template <bool F32>
__device__ __forceinline__ float load1(const void* base, size_t idx) {
    if constexpr (F32) return reinterpret_cast<const float*>(base)[idx];
    else return bf1(reinterpret_cast<const bf16_t*>(base)[idx]);
}
template <bool F32>
__device__ __forceinline__ void store1(void* base, size_t idx, float v) {
    if constexpr (F32) reinterpret_cast<float*>(base)[idx] = v;
    else reinterpret_cast<bf16_t*>(base)[idx] = f2bf(v);
}
template <bool F32>
__device__ __forceinline__ void store8(void* base, size_t idx, const float (&a)[8]) {
    if constexpr (F32) {
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + idx) = make_float4(a[0], a[1], a[2], a[3]);
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(base) + idx + 4) = make_float4(a[4], a[5], a[6], a[7]);
    } else {
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(base) + idx) =
            make_uint4(pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(a[4], a[5]), pack_bf16x2(a[6], a[7]));
    }
}

// wide_decoder_bighead.hip: head dim 256 / 512, Sq <= DA_MAXQ target rows, Sk <= DA_BIGHEAD_MAXK keys; p.scale is set by the caller. The
// checks run before the launch; `who` names the entry point in a refusal.
bool dec_attn_bighead_dim(int dh);
int dec_attn_bighead(const DecAttnParams& p, int dh, bool f32, bool bwd, const char* who, hipStream_t st);

}  // namespace egx
