// The criterion of the long-term-anticipation task in one launch: HOI/tasks/lta/long_term_anticipation.py:182-203,
//   loss = sum over heads h, future steps z of CrossEntropyLoss(mean)(pred_h[:, z], labels[:, z, h])       (2 x 20 = 40 terms)
//   top-k errors of every (z, h) pair (evaluation/lta/lta_metrics.py:38-84 topks_correct), each read with .item()
// on the (B, Z, ld) stack of the MultiTaskHead's outputs, whose heads are column windows [col0[h], col0[h] + C[h]) of a row.
//
//   grid    : a workgroup per (future step z, chunk of clips); 4 waves, a wave per row (b, z) of the chunk, its heads one after the other.
//             Every workgroup first counts the valid labels of ITS z over all B clips (the normaliser depends on the labels only), so the
//             loss terms and d loss / d logits of its rows are final in the same pass.
//   segment : C <= 512: lane-strided dword loads (rows have no alignment: ld = 593 is odd), the segment stays in up to 8 registers per
//             lane; wave butterflies for max, exp-sum and the label's rank; the gradient is written from the registers, so every logit
//             is read once. C > 512: a per-lane online max / exp-sum pass, then one re-read (from L2) that writes the gradient.
//   sums    : per-workgroup partials (nll per head, correct counts per k and head) go to scratch; the last workgroup to arrive sums
//             the chunks of every (z, h) pair by a fixed butterfly, divides by n_valid and adds the terms in a fixed order: the same bits
//             on every run, no float atomics. The arrival counters leave themselves zero.
#include "common.h"
#include "kernels.h"

namespace egx {

constexpr int SEG_WAVES = 4;
constexpr int SEG_COUNTER_WORDS = 16;     // an arrival counter per 64 bytes: [launch][future step 0][future step 1] ...
constexpr int SEG_RED_U = 4;              // (z, h) pairs a wave of the last workgroup sums per pass
constexpr int SEG_MAX_CHUNKS = 64;      // chunks of clips per future step: bounds the label count every workgroup repeats

struct SegCeParams {
    const float* logits; const int64_t* target;
    int B, Z, H, ld, nks, chunk, nchunks, gaps;
    int col0[SEG_CE_MAX_HEADS], C[SEG_CE_MAX_HEADS], ks[SEG_CE_MAX_KS];
    float* loss; float* loss_terms; int* n_valid; int* correct; float* dlogits;
    float* fpart;           // [Z * nchunks][H]        sum of nll over the chunk's valid rows
    int* ipart;             // [Z * nchunks][nks][H]   rows of the chunk whose label has rank < k
    unsigned* counter;      // arrival counters, zero before the first launch
};

struct SegOut { float nll; int rank; };

// C <= 64 * NR: element c = lane + 64 j lives in register j
template <int NR>
__device__ __forceinline__ SegOut seg_regs(const float* __restrict__ seg, float* __restrict__ dseg, int C, int y, float inv, int lane) {
    float v[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) v[j] = lane + 64 * j < C ? seg[lane + 64 * j] : -INFINITY;
    float m = v[0], zy = -INFINITY;
#pragma unroll
    for (int j = 0; j < NR; ++j) { m = fmaxf(m, v[j]); zy = lane + 64 * j == y ? v[j] : zy; }
    m = wave_max(m);
    zy = __shfl(zy, y & 63, 64);
    float s = 0.f;
    int r = 0;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int c = lane + 64 * j;
        const bool in = c < C;
        r += in ? outranks(v[j], zy, c, y) : 0;
        v[j] = in ? expf(v[j] - m) : 0.f;       // max-subtracted: the largest term is 1
        s += v[j];
    }
    s = wave_sum(s);
    r = wave_sum(r);
    if (dseg) {
        const float rs = 1.f / s;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int c = lane + 64 * j;
            if (c < C) dseg[c] = (v[j] * rs - (c == y ? 1.f : 0.f)) * inv;
        }
    }
    SegOut o;
    o.nll = (m - zy) + logf(s);
    o.rank = r;
    return o;
}

// C > 512: per-lane online max / exp-sum over the lane's elements, combined across the wave; the gradient pass reads the segment again
__device__ __forceinline__ SegOut seg_loop(const float* __restrict__ seg, float* __restrict__ dseg, int C, int y, float inv, int lane) {
    const float zy = seg[y];
    float ml = seg[lane], sl = 1.f;             // C > 512: every lane owns an element
    int r = outranks(ml, zy, lane, y);
#pragma unroll 4
    for (int c = lane + 64; c < C; c += 64) {
        const float x = seg[c];
        r += outranks(x, zy, c, y);
        if (x > ml) { sl = sl * expf(ml - x) + 1.f; ml = x; }
        else sl += expf(x - ml);
    }
    const float m = wave_max(ml);
    const float s = wave_sum(sl * expf(ml - m));
    r = wave_sum(r);
    if (dseg) {
        const float rs = 1.f / s;
#pragma unroll 4
        for (int c = lane; c < C; c += 64) dseg[c] = (expf(seg[c] - m) * rs - (c == y ? 1.f : 0.f)) * inv;
    }
    SegOut o;
    o.nll = (m - zy) + logf(s);
    o.rank = r;
    return o;
}

// 6 waves per SIMD (77 VGPRs, no scratch): the kernel is a chain of memory round trips per wave, so it lives off waves in flight
__global__ __launch_bounds__(256, 6) void segmented_ce_kernel(SegCeParams p) {
    __shared__ int cnt_s[SEG_WAVES][SEG_CE_MAX_HEADS];
    __shared__ float nll_s[SEG_WAVES][SEG_CE_MAX_HEADS];
    __shared__ int cor_s[SEG_WAVES][SEG_CE_MAX_KS][SEG_CE_MAX_HEADS];
    __shared__ float red_s[SEG_WAVES];
    __shared__ int col0_s[SEG_CE_MAX_HEADS], C_s[SEG_CE_MAX_HEADS], ks_s[SEG_CE_MAX_KS];      // indexed by a run-time head / k below
    __shared__ float inv_s[SEG_CE_MAX_HEADS];
    __shared__ bool last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int z = blockIdx.x / p.nchunks, chunk_id = blockIdx.x % p.nchunks;
    if (tid == 0) {
#pragma unroll
        for (int h = 0; h < SEG_CE_MAX_HEADS; ++h) { col0_s[h] = p.col0[h]; C_s[h] = p.C[h]; }
#pragma unroll
        for (int k = 0; k < SEG_CE_MAX_KS; ++k) ks_s[k] = p.ks[k];
    }
    if (lane < SEG_CE_MAX_HEADS) {          // the wave's accumulators: lane 0 adds a row's results in row order
        nll_s[wave][lane] = 0.f;
#pragma unroll
        for (int k = 0; k < SEG_CE_MAX_KS; ++k) cor_s[wave][k][lane] = 0;
    }

    // n_valid[z, h] over ALL clips: every workgroup of this z counts it itself
    int cnt[SEG_CE_MAX_HEADS] = {0, 0, 0, 0};
    for (int b = tid; b < p.B; b += 256) {
        const int64_t* t = p.target + ((size_t)b * p.Z + z) * p.H;
#pragma unroll
        for (int h = 0; h < SEG_CE_MAX_HEADS; ++h)
            if (h < p.H) { const int64_t y = t[h]; cnt[h] += (y >= 0 && y < p.C[h]) ? 1 : 0; }
    }
#pragma unroll
    for (int h = 0; h < SEG_CE_MAX_HEADS; ++h) {
        cnt[h] = wave_sum(cnt[h]);
        if (lane == 0) cnt_s[wave][h] = cnt[h];
    }
    __syncthreads();
    if (tid < SEG_CE_MAX_HEADS) {
        const int n = (cnt_s[0][tid] + cnt_s[1][tid]) + (cnt_s[2][tid] + cnt_s[3][tid]);
        inv_s[tid] = n > 0 ? 1.f / (float)n : 0.f;
    }
    __syncthreads();

    const int b_end = min(p.B, (chunk_id + 1) * p.chunk);
    for (int b = chunk_id * p.chunk + wave; b < b_end; b += SEG_WAVES) {     // wave w: rows w, w + 4, ... of the chunk, in this order
        const size_t row = (size_t)b * p.Z + z;
        const float* lrow = p.logits + row * p.ld;
        float* drow = p.dlogits ? p.dlogits + row * p.ld : nullptr;
        const int64_t* t = p.target + row * p.H;
        if (drow && p.gaps)                                                    // columns no head covers: zero gradient
            for (int c = lane; c < p.ld; c += 64) {
                bool covered = false;
                for (int h = 0; h < p.H; ++h) covered |= c >= col0_s[h] && c < col0_s[h] + C_s[h];
                if (!covered) drow[c] = 0.f;
            }
#pragma unroll 1
        for (int h = 0; h < p.H; ++h) {
            const int C = C_s[h];
            const int64_t y64 = t[h];
            // ignore_index (-100) / out-of-range label: no loss, no count, no gradient. The label is the same in every lane.
            const int y = __builtin_amdgcn_readfirstlane((y64 < 0 || y64 >= C) ? -1 : (int)y64);
            const float* seg = lrow + col0_s[h];
            float* dseg = drow ? drow + col0_s[h] : nullptr;
            if (y < 0) {
                if (dseg)
                    for (int c = lane; c < C; c += 64) dseg[c] = 0.f;
                continue;
            }
            const float inv = inv_s[h];
            SegOut o;
            if (C <= 64) o = seg_regs<1>(seg, dseg, C, y, inv, lane);
            else if (C <= 128) o = seg_regs<2>(seg, dseg, C, y, inv, lane);
            else if (C <= 256) o = seg_regs<4>(seg, dseg, C, y, inv, lane);
            else if (C <= 512) o = seg_regs<8>(seg, dseg, C, y, inv, lane);
            else o = seg_loop(seg, dseg, C, y, inv, lane);
            if (lane == 0) {
                nll_s[wave][h] += o.nll;
                for (int k = 0; k < p.nks; ++k) cor_s[wave][k][h] += o.rank < ks_s[k] ? 1 : 0;
            }
        }
    }
    __syncthreads();
    // Workgroup partials -> scratch, the last workgroup to arrive sums them. The hand-off (wave 0 stores and signals): every handed-off word
    // is stored write-through at agent scope, the wave drains its stores, then ONE relaxed agent-scope add draws the ticket; the reader loads
    // every such word at agent scope (past its CU's L1). No release fence, so no L2 write-back per workgroup.
    if (wave == 0) {
        if (lane < p.H)
            __hip_atomic_store(p.fpart + (size_t)blockIdx.x * p.H + lane, (nll_s[0][lane] + nll_s[1][lane]) + (nll_s[2][lane] + nll_s[3][lane]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane < p.nks * p.H) {
            const int k = lane / p.H, h = lane % p.H;
            __hip_atomic_store(p.ipart + ((size_t)blockIdx.x * p.nks + k) * p.H + h,
                               (cor_s[0][k][h] + cor_s[1][k][h]) + (cor_s[2][k][h] + cor_s[3][k][h]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (chunk_id == 0 && lane < p.H)
            __hip_atomic_store(p.n_valid + (size_t)z * p.H + lane, (cnt_s[0][lane] + cnt_s[1][lane]) + (cnt_s[2][lane] + cnt_s[3][lane]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            // two levels of arrival counters: a thousand adds to ONE word take longer than the rest of the kernel (they are served one after
            // the other), so the chunks of a future step count on that step's word and only its last chunk goes on to the launch's
            bool z_last = true;
            if (p.nchunks > 1) {
                unsigned* zc = p.counter + SEG_COUNTER_WORDS * (1 + z);
                z_last = __hip_atomic_fetch_add(zc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)p.nchunks - 1;
                if (z_last) __hip_atomic_store(zc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // left zero for the next launch
            }
            last_s = z_last && __hip_atomic_fetch_add(p.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)p.Z - 1;
        }
    }
    __syncthreads();
    if (!last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // wave-cooperative sums, the same order on every run: lane j holds chunk j of a (z, h) pair (nchunks <= 64), a butterfly adds the lanes;
    // SEG_RED_U pairs per pass have their loads in flight together (every pass is one memory round trip)
    const int items = p.Z * p.H;            // <= 2^30: B * Z is limited to SEG_CE_MAX_ROWS
    float local = 0.f;
    for (int i0 = wave * SEG_RED_U; i0 < items; i0 += SEG_WAVES * SEG_RED_U) {
        float f[SEG_RED_U];
        int c[SEG_RED_U][SEG_CE_MAX_KS], n[SEG_RED_U];
#pragma unroll
        for (int u = 0; u < SEG_RED_U; ++u) {           // every load is issued (at a clamped, valid address) and selected afterwards:
            const int i = i0 + u;                       // a load behind a branch would be waited for before the next one goes out
            const bool in = i < items && lane < p.nchunks;
            const int ic = min(i, items - 1);
            const size_t blk = (size_t)(ic / p.H) * p.nchunks + min(lane, p.nchunks - 1);
            const int hh = ic % p.H;
            const float fv = __hip_atomic_load(p.fpart + blk * p.H + hh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            f[u] = in ? fv : 0.f;
#pragma unroll
            for (int k = 0; k < SEG_CE_MAX_KS; ++k) {
                const int cv = __hip_atomic_load(p.ipart + (blk * p.nks + (k < p.nks ? k : 0)) * p.H + hh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                c[u][k] = (in && k < p.nks) ? cv : 0;
            }
            n[u] = __hip_atomic_load(p.n_valid + ic, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int u = 0; u < SEG_RED_U; ++u) {
            const int i = i0 + u;
            const float s = wave_sum(f[u]);
#pragma unroll
            for (int k = 0; k < SEG_CE_MAX_KS; ++k) c[u][k] = wave_sum(c[u][k]);
            if (i >= items) continue;
            const float term = n[u] > 0 ? s / (float)n[u] : 0.f;        // a (z, h) pair without a valid label adds nothing
            local += term;
            if (lane == 0) {
                if (p.loss_terms) p.loss_terms[i] = term;
#pragma unroll
                for (int k = 0; k < SEG_CE_MAX_KS; ++k)
                    if (k < p.nks) p.correct[(size_t)k * items + i] = c[u][k];
            }
        }
    }
    if (lane == 0) red_s[wave] = local;
    __syncthreads();
    if (tid == 0) {
        *p.loss = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        *p.counter = 0u;
    }
}

void batch_chunks(int B, int max_chunks, int waves, int* chunk, int* nchunks) {
    const int c = B / max_chunks + (B % max_chunks ? 1 : 0);
    *chunk = c < waves ? waves : c;
    *nchunks = (B + *chunk - 1) / *chunk;
}

int check_head_windows(const char* who, int ld, int H, const int* col0, const int* C) {
    for (int h = 0; h < H; ++h) {
        EGX_CHECK(C[h] >= 1 && C[h] <= SEG_CE_MAX_CLASSES, "%s: head %d has C=%d classes (needs 1 <= C <= %d)", who, h, C[h], SEG_CE_MAX_CLASSES);
        EGX_CHECK(col0[h] >= 0 && col0[h] <= ld - C[h], "%s: head %d covers columns [%d, %d) of a row of ld=%d", who, h, col0[h], col0[h] + C[h], ld);
        for (int g = 0; g < h; ++g)
            EGX_CHECK(col0[h] >= col0[g] + C[g] || col0[g] >= col0[h] + C[h], "%s: heads %d and %d overlap (columns [%d, %d) and [%d, %d))", who,
                      g, h, col0[g], col0[g] + C[g], col0[h], col0[h] + C[h]);
    }
    return 0;
}

static size_t seg_counter_bytes(int Z) { return (size_t)(1 + Z) * SEG_COUNTER_WORDS * sizeof(unsigned); }

static int seg_ce_check_dims(int B, int Z, int H, int n_ks) {
    EGX_CHECK(B >= 1 && Z >= 1, "segmented_ce: B=%d Z=%d (both need to be >= 1)", B, Z);
    EGX_CHECK((long long)B * Z <= (long long)SEG_CE_MAX_ROWS, "segmented_ce: B * Z = %lld rows (needs B * Z <= %d)", (long long)B * Z, SEG_CE_MAX_ROWS);
    EGX_CHECK(H >= 1 && H <= SEG_CE_MAX_HEADS, "segmented_ce: H=%d (needs 1 <= H <= %d heads)", H, SEG_CE_MAX_HEADS);
    EGX_CHECK(n_ks >= 0 && n_ks <= SEG_CE_MAX_KS, "segmented_ce: n_ks=%d (needs 0 <= n_ks <= %d)", n_ks, SEG_CE_MAX_KS);
    return 0;
}

size_t segmented_ce_scratch_bytes(int B, int Z, int H, int n_ks) {
    if (seg_ce_check_dims(B, Z, H, n_ks)) return 0;
    int chunk, nchunks;
    batch_chunks(B, SEG_MAX_CHUNKS, SEG_WAVES, &chunk, &nchunks);
    // [arrival counters: 64 B each, the launch's and one per future step][nll partials][count partials]
    return seg_counter_bytes(Z) + (size_t)Z * nchunks * H * sizeof(float) + (size_t)Z * nchunks * (n_ks > 0 ? n_ks : 1) * H * sizeof(int);
}

int segmented_ce(const float* logits, int ld, const int64_t* target, int B, int Z, int H, const int* col0, const int* C, const int* ks,
                 int n_ks, float* loss, float* loss_terms, int* n_valid, int* correct, float* dlogits, void* scratch, hipStream_t st) {
    EGX_CHECK(logits && target && col0 && C && loss && n_valid && scratch, "segmented_ce: null pointer argument");
    if (seg_ce_check_dims(B, Z, H, n_ks)) return 1;
    EGX_CHECK(n_ks == 0 || (ks && correct), "segmented_ce: null pointer argument (ks / correct with n_ks=%d)", n_ks);
    EGX_CHECK(ld >= 1, "segmented_ce: ld=%d (needs ld >= 1)", ld);
    if (check_head_windows("segmented_ce", ld, H, col0, C)) return 1;
    int min_c = SEG_CE_MAX_CLASSES, covered = 0;
    for (int h = 0; h < H; ++h) {
        min_c = C[h] < min_c ? C[h] : min_c;
        covered += C[h];
    }
    for (int k = 0; k < n_ks; ++k)
        EGX_CHECK(ks[k] >= 1 && ks[k] <= min_c, "segmented_ce: ks[%d]=%d (needs 1 <= k <= %d, the narrowest head)", k, ks[k], min_c);
    SegCeParams p;
    p.logits = logits; p.target = target; p.B = B; p.Z = Z; p.H = H; p.ld = ld; p.nks = n_ks;
    batch_chunks(B, SEG_MAX_CHUNKS, SEG_WAVES, &p.chunk, &p.nchunks);
    p.gaps = covered != ld;
    for (int h = 0; h < SEG_CE_MAX_HEADS; ++h) { p.col0[h] = h < H ? col0[h] : 0; p.C[h] = h < H ? C[h] : 0; }
    for (int k = 0; k < SEG_CE_MAX_KS; ++k) p.ks[k] = k < n_ks ? ks[k] : 0;
    p.loss = loss; p.loss_terms = loss_terms; p.n_valid = n_valid; p.correct = correct; p.dlogits = dlogits;
    p.counter = (unsigned*)scratch;
    p.fpart = (float*)((char*)scratch + seg_counter_bytes(Z));
    p.ipart = (int*)(p.fpart + (size_t)Z * p.nchunks * H);
    hipLaunchKernelGGL(segmented_ce_kernel, dim3((unsigned)(Z * p.nchunks)), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
