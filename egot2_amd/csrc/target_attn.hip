// Attention of a LONG target (up to 64 query rows) for the composed decoder's training route (egot2_amd/decoder.py, egx_long_targets): the
// reference trains the HOI action / LTA EgoT2-g model on 21- and 40-token targets (HOI/tasks/multitask/video_task_action.py:34-53,
// HOI/models/lta/lta_models_seqdecoder.py:175-179), the small kernels of decoder.hip stop at 8 rows. Same operands, layout and arithmetic
// as small_attention_fwd/bwd (fp32 on the VALU, separate Q and K / V operands at their own row strides, head h at columns [h * dh, (h + 1) * dh)):
//   target_attention_fwd/bwd  1 <= Sq <= 64 queries against 1 <= Sk <= 1024 keys, 1 <= dh <= 128. One workgroup of four waves per (b, h)
//                             walks the query rows in GROUPS of 8 with the arithmetic of long_memory_attention_kernel: K / V pass
//                             through one 64-row LDS buffer in chunks, the 8 x round_up(Sk, 64) probabilities of the group stay in LDS.
//                             (A causal call has Sk = Sq <= 64: one chunk, so there is no chunk above the diagonal to skip.)
//   backward                  recomputes the probabilities and regenerates the mask per group; nothing is saved by the forward. dQ rows
//                             belong to one group and are written once. dK / dV: the thread that owns (key j, column c) — the same
//                             thread in every group — ASSIGNS the first group's sum and ADDS each later group's to what it wrote
//                             itself, so the order of the sum is fixed, no buffer is assumed zero and no atomic is needed.
//   dropout                   row (b * H + h) * 64 + query, column key: the row stride is 64 (TA_MAXQ), not the small kernels' 8, whose
//                             rows of neighbouring (b, h) would collide from query 8 on.
// A (b, h)'s arithmetic depends on nothing but its own operands and its block index (through the mask row).
#include "../../include/egot2x.h"
#include "common.h"
#include "kernels.h"
#include "fused_host.h"

namespace egx {

constexpr int TA_MAXQ = 64, TA_MAXK = 1024, TA_MAXDH = 128, TA_GROUP = 8, TA_CHUNK = 64, TA_NTH = 256;

// grid = B * H, block = 256. LDS: K or V chunk [64][dh + 1]; Q, dO of the group [8][dh]; P, dS of the group [8][round_up(Sk, 64)].
// acc[u] is indexed by unrolled loops only: a runtime-indexed register array would go to scratch.
template <bool BWD>
__global__ __launch_bounds__(TA_NTH) void target_attention_kernel(SmallAttnParams p) {
    extern __shared__ float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int dh = p.dh, LDK = dh + 1, Sq = p.Sq, Sk = p.Sk, SKP = (Sk + TA_CHUNK - 1) & ~(TA_CHUNK - 1);
    float* Cs = sm;                         // K or V chunk [64][dh + 1], zero beyond Sk
    float* Qs = Cs + TA_CHUNK * LDK;
    float* Gs = Qs + TA_GROUP * dh;         // dO (backward only)
    float* Ps = Gs + TA_GROUP * dh;         // [8][SKP]
    float* Ds = Ps + TA_GROUP * SKP;        // backward only
    const float* kb = p.k + (size_t)b * Sk * p.ldk + h * dh;
    const float* vb = p.v + (size_t)b * Sk * p.ldv + h * dh;
    const float* qb = p.q + (size_t)b * Sq * p.ldq + h * dh;
    const uint32_t row0 = (uint32_t)blockIdx.x * TA_MAXQ;
    auto stage = [&](const float* src, int ld, int j0) {
        __syncthreads();
        for (int i = tid; i < TA_CHUNK * dh; i += TA_NTH) {
            const int j = i / dh, c = i - j * dh;
            Cs[j * LDK + c] = j0 + j < Sk ? src[(size_t)(j0 + j) * ld + c] : 0.f;
        }
        __syncthreads();
    };
    for (int i0 = 0; i0 < Sq; i0 += TA_GROUP) {
        const int ng = min(TA_GROUP, Sq - i0);          // rows of this group: local r = 0 .. ng - 1 is query i0 + r
        __syncthreads();                                // the previous group has read Qs / Gs / Ps / Ds
        for (int i = tid; i < ng * dh; i += TA_NTH) {
            const int r = i / dh, c = i - r * dh;
            Qs[i] = qb[(size_t)(i0 + r) * p.ldq + c];
            if constexpr (BWD) Gs[i] = p.d_o[((size_t)b * Sq + i0 + r) * p.ldo + h * dh + c];
        }
        // scores: wave w owns local rows w, w + 4; lane = key within the chunk
        for (int j0 = 0; j0 < Sk; j0 += TA_CHUNK) {
            stage(kb, p.ldk, j0);
            for (int r = wave; r < ng; r += 4) {
                float sc = 0.f;
                for (int c = 0; c < dh; ++c) sc += Qs[r * dh + c] * Cs[lane * LDK + c];
                const int j = j0 + lane;
                Ps[r * SKP + j] = (j < Sk && !(p.causal && j > i0 + r)) ? sc * p.scale : -INFINITY;
            }
        }
        __syncthreads();
        for (int r = wave; r < ng; r += 4) {
            float m = -INFINITY;
            for (int j = lane; j < SKP; j += 64) m = fmaxf(m, Ps[r * SKP + j]);
            m = wave_max(m);
            float sum = 0.f;
            for (int j = lane; j < SKP; j += 64) { const float e = __expf(Ps[r * SKP + j] - m); Ps[r * SKP + j] = e; sum += e; }
            sum = 1.f / wave_sum(sum);
            for (int j = lane; j < SKP; j += 64) Ps[r * SKP + j] *= sum;        // the plain probabilities (0 where masked and beyond Sk)
        }
        if constexpr (BWD) {
            // dP = dO V^T into Ds
            for (int j0 = 0; j0 < Sk; j0 += TA_CHUNK) {
                stage(vb, p.ldv, j0);
                for (int r = wave; r < ng; r += 4) {
                    float dp = 0.f;
                    for (int c = 0; c < dh; ++c) dp += Gs[r * dh + c] * Cs[lane * LDK + c];
                    Ds[r * SKP + j0 + lane] = dp;
                }
            }
            __syncthreads();
            for (int r = wave; r < ng; r += 4) {
                const uint32_t mrow = row0 + (uint32_t)(i0 + r);
                float delta = 0.f;
                for (int j = lane; j < SKP; j += 64) {
                    float mask = 1.f;
                    if (p.drop_thresh) mask = drop_scale(p.drop_key, mrow, (uint32_t)j, p.drop_thresh, p.drop_inv);
                    const float dp = Ds[r * SKP + j] * mask;
                    Ds[r * SKP + j] = dp;
                    delta += Ps[r * SKP + j] * dp;
                }
                delta = wave_sum(delta);
                for (int j = lane; j < SKP; j += 64) {
                    float mask = 1.f;
                    if (p.drop_thresh) mask = drop_scale(p.drop_key, mrow, (uint32_t)j, p.drop_thresh, p.drop_inv);
                    const float pr = Ps[r * SKP + j];
                    Ds[r * SKP + j] = pr * (Ds[r * SKP + j] - delta) * p.scale;
                    Ps[r * SKP + j] = pr * mask;
                }
            }
            // dQ = dS K (accumulated over the chunks); dK = dS^T Q, dV = P^T dO per chunk, carried over the groups by their owner
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < Sk; j0 += TA_CHUNK) {
                stage(kb, p.ldk, j0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = tid + u * TA_NTH;
                    if (e < ng * dh) {
                        const int r = e / dh, c = e - r * dh;
                        float a = 0.f;
                        for (int j = 0; j < TA_CHUNK; ++j) a += Ds[r * SKP + j0 + j] * Cs[j * LDK + c];
                        acc[u] += a;
                    }
                }
                for (int e = tid; e < TA_CHUNK * dh; e += TA_NTH) {
                    const int j = e / dh, c = e - j * dh;
                    if (j0 + j < Sk) {
                        float ak = 0.f, av = 0.f;
                        for (int r = 0; r < ng; ++r) {
                            ak += Ds[r * SKP + j0 + j] * Qs[r * dh + c];
                            av += Ps[r * SKP + j0 + j] * Gs[r * dh + c];
                        }
                        float* dkp = p.dk + ((size_t)b * Sk + j0 + j) * p.ldk + h * dh + c;
                        float* dvp = p.dv + ((size_t)b * Sk + j0 + j) * p.ldv + h * dh + c;
                        if (i0 == 0) { *dkp = ak; *dvp = av; }
                        else { *dkp += ak; *dvp += av; }            // this thread wrote the element in every earlier group
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = tid + u * TA_NTH;
                if (e < ng * dh) { const int r = e / dh, c = e - r * dh; p.dq[((size_t)b * Sq + i0 + r) * p.ldq + h * dh + c] = acc[u]; }
            }
        } else {
            if (p.drop_thresh) {
                for (int r = wave; r < ng; r += 4)
                    for (int j = lane; j < SKP; j += 64)
                        Ps[r * SKP + j] *= drop_scale(p.drop_key, row0 + (uint32_t)(i0 + r), (uint32_t)j, p.drop_thresh, p.drop_inv);
            }
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j0 = 0; j0 < Sk; j0 += TA_CHUNK) {
                stage(vb, p.ldv, j0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = tid + u * TA_NTH;
                    if (e < ng * dh) {
                        const int r = e / dh, c = e - r * dh;
                        float a = 0.f;
                        for (int j = 0; j < TA_CHUNK; ++j) a += Ps[r * SKP + j0 + j] * Cs[j * LDK + c];
                        acc[u] += a;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int e = tid + u * TA_NTH;
                if (e < ng * dh) { const int r = e / dh, c = e - r * dh; p.o[((size_t)b * Sq + i0 + r) * p.ldo + h * dh + c] = acc[u]; }
            }
        }
    }
}

static size_t target_attn_lds(int dh, int Sk) {
    return ((size_t)TA_CHUNK * (dh + 1) + (size_t)2 * TA_GROUP * dh + (size_t)2 * TA_GROUP * ((Sk + TA_CHUNK - 1) & ~(TA_CHUNK - 1))) * sizeof(float);
}

// every refusal of the two entry points: host work only, before any device call
static int target_attention_check(const char* who, const SmallAttnParams& p, int ldo) {
    EGX_CHECK(p.B >= 1 && p.H >= 1, "%s: B=%d H=%d", who, p.B, p.H);
    EGX_CHECK(p.Sq >= 1 && p.Sq <= TA_MAXQ, "%s: Sq=%d outside 1..%d (target tokens)", who, p.Sq, TA_MAXQ);
    EGX_CHECK(p.Sk >= 1 && p.Sk <= TA_MAXK, "%s: Sk=%d outside 1..%d", who, p.Sk, TA_MAXK);
    EGX_CHECK(p.dh >= 1 && p.dh <= TA_MAXDH, "%s: head dim %d outside 1..%d", who, p.dh, TA_MAXDH);
    EGX_CHECK(!p.causal || p.Sq == p.Sk, "%s: the causal mask needs Sq == Sk, got Sq=%d Sk=%d", who, p.Sq, p.Sk);
    const long long w = (long long)p.H * p.dh;
    EGX_CHECK(p.ldq >= w && p.ldk >= w && p.ldv >= w && ldo >= w, "%s: row strides %d / %d / %d / %d below H * dh = %lld", who, p.ldq, p.ldk,
              p.ldv, ldo, w);
    EGX_CHECK((long long)p.B * p.H <= 0x7fffffffLL / TA_MAXQ, "%s: B * H = %lld too large", who, (long long)p.B * p.H);
    return 0;
}

template <bool BWD>
static int launch_target_attention(SmallAttnParams p, hipStream_t st) {
    p.scale = 1.f / sqrtf((float)p.dh);
    static bool attr = false;
    if (!attr) {
        EGX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&target_attention_kernel<BWD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)target_attn_lds(TA_MAXDH, TA_MAXK)));
        attr = true;
    }
    hipLaunchKernelGGL(target_attention_kernel<BWD>, dim3(p.B * p.H), dim3(TA_NTH), target_attn_lds(p.dh, p.Sk), st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

static SmallAttnParams target_attn_params(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int ldo, int B, int Sq,
                                          int Sk, int H, int dh, int causal, float p_drop, uint64_t seed, uint32_t site) {
    SmallAttnParams p = {};
    p.q = q; p.k = k; p.v = v; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo;
    p.B = B; p.Sq = Sq; p.Sk = Sk; p.H = H; p.dh = dh; p.causal = causal;
    Drop dr = make_drop(p_drop > 0.f, p_drop, seed, site >> 8, site & 0xffu);
    p.drop_key = dr.key; p.drop_thresh = dr.thresh; p.drop_inv = dr.inv_keep;
    return p;
}

}  // namespace egx

using namespace egx;

extern "C" {

int egx_target_attention_fwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* o, int ldo, int B, int Sq,
                             int Sk, int H, int dh, int causal, float p_drop, uint64_t seed, uint32_t site, void* stream) {
    SmallAttnParams p = target_attn_params(q, ldq, k, ldk, v, ldv, ldo, B, Sq, Sk, H, dh, causal, p_drop, seed, site);
    p.o = o;
    EGX_CHECK(q && k && v && o, "egx_target_attention_fwd: null pointer argument");
    if (target_attention_check("egx_target_attention_fwd", p, ldo)) return 1;
    return launch_target_attention<false>(p, (hipStream_t)stream);
}

int egx_target_attention_bwd(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* d_o, int ldo, float* dq,
                             float* dk, float* dv, int B, int Sq, int Sk, int H, int dh, int causal, float p_drop, uint64_t seed,
                             uint32_t site, void* stream) {
    SmallAttnParams p = target_attn_params(q, ldq, k, ldk, v, ldv, ldo, B, Sq, Sk, H, dh, causal, p_drop, seed, site);
    p.d_o = d_o; p.dq = dq; p.dk = dk; p.dv = dv;
    EGX_CHECK(q && k && v && d_o && dq && dk && dv, "egx_target_attention_bwd: null pointer argument");
    if (target_attention_check("egx_target_attention_bwd", p, ldo)) return 1;
    return launch_target_attention<true>(p, (hipStream_t)stream);
}

}  // extern "C"
