// The test epoch of the action-recognition translators after the model: MultiTaskClassificationTask.test_epoch_end,
// HOI/tasks/lta/long_term_anticipation.py:96-158 (the same code in long_term_anticipation_taskspecfic.py:100-162),
//   per clip i: video_preds[clip_id] += preds[i]  |  = torch.max(video_preds[clip_id], preds[i]), from torch.zeros; video_labels[clip_id] = labels[i]
//   topk_errors(stack(video_preds), stack(video_labels)[:, h], (1, 5)) per head                       (evaluation/lta/lta_metrics.py:38-84)
// as a device-resident accumulator (view_ensemble_update, one launch per batch) and its metric (view_ensemble_topk, one launch per epoch).
//
//   state   : [256 B header: arrival counter of the top-k launch, dropped clips][labels int64 (capacity, H)][views int32 (capacity)]
//             [count partials][rows fp32 (capacity, ld)], ld = sum of C, the heads packed side by side. All zero = empty: the reference's
//             torch.zeros rows, which is also where "max" starts from (a video whose logits are all negative ends as a row of zeros).
//   update  : a workgroup per (clip i, chunk of 256 columns), a column per thread. The workgroup of the FIRST clip of a video in the batch
//             owns the video for this launch: it reads the stored value once, folds clips i, i + 1, ... of that video in row order in a
//             register and writes it back; every other workgroup of the video leaves after the look-back. A wave finds the clips of its video by
//             comparing 64 slots at a time (one ballot). So a video's row is ONE left fold in arrival order - the same bits on every run
//             and however the views are spread over rows and calls -, no two workgroups touch one row, and there are no float atomics.
//             Loads and stores are lane-contiguous along the columns.
//   top-k   : 4 waves, a wave per video, its heads one after the other; C <= 512 in up to 8 registers per lane, beyond that a lane-strided
//             loop. rank by the rule of seg_ce.hip (outranks, common.h) on the key (NaN ranks as the greatest value, as torch.topk has
//             it); counts go through per-workgroup partials that the last workgroup to arrive adds in workgroup order. The arrival
//             counter leaves itself zero.
#include "common.h"
#include "kernels.h"

namespace egx {

constexpr int VE_WAVES = 4;
constexpr int VE_MAX_BLOCKS = 256;                                              // workgroups of the top-k launch (videos are strided over them)
constexpr int VE_HEADER_BYTES = 256;
constexpr int VE_DROPPED_WORD = 16;                                             // 64 bytes past the arrival counter
constexpr int VE_PART_WORDS = 1 + SEG_CE_MAX_HEADS + SEG_CE_MAX_KS * SEG_CE_MAX_HEADS;      // [non-finite][invalid[h]][correct[k][h]]
constexpr int VE_PART_STRIDE = 24;
constexpr int VE_GROUP = 4;                                                     // clips of a video whose loads are in flight together

struct VeLayout { size_t labels, views, parts, rows, bytes; int ld; };

static VeLayout ve_layout(int capacity, int H, const int* C) {
    VeLayout L;
    L.ld = 0;
    for (int h = 0; h < H; ++h) L.ld += C[h];
    L.labels = VE_HEADER_BYTES;
    L.views = L.labels + (size_t)capacity * H * sizeof(int64_t);
    L.parts = align_up(L.views + (size_t)capacity * sizeof(int), 16);
    L.rows = align_up(L.parts + (size_t)VE_MAX_BLOCKS * VE_PART_STRIDE * sizeof(int), 256);
    L.bytes = L.rows + (size_t)capacity * L.ld * sizeof(float);
    return L;
}

struct VeUpdateParams {
    const float* x; const int64_t* labels; const void* slots;
    int slot_i64, slot0, B, H, ld_in, ld, capacity, method;
    int col0[SEG_CE_MAX_HEADS], C[SEG_CE_MAX_HEADS];
    float* rows; int64_t* vlabels; int* views; unsigned* dropped;
};

__device__ __forceinline__ long long ve_slot(const VeUpdateParams& p, int j) {
    return p.slot_i64 ? (long long)((const int64_t*)p.slots)[j] : (long long)((const int*)p.slots)[j];
}

// torch.max(a, b) of two tensors: a NaN in either operand wins; sum: one fp32 add
__device__ __forceinline__ float ve_fold(float v, float x, int method) {
    return method == VIEW_ENS_SUM ? v + x : ((x > v || x != x) ? x : v);
}

__global__ __launch_bounds__(256) void view_ensemble_update_kernel(VeUpdateParams p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x;
    const int c = blockIdx.y * 256 + tid;
    const long long s = p.slots ? ve_slot(p, i) : (long long)p.slot0 + i;
    if (s < 0 || s >= p.capacity) {                                             // dropped, and counted once per clip
        if (blockIdx.y == 0 && tid == 0) atomicAdd(p.dropped, 1u);
        return;
    }
    if (p.slots)                                                                // an earlier clip of the batch owns this video
        for (int j0 = 0; j0 < i; j0 += 64) {
            const int j = j0 + lane;
            if (__ballot(j < i && ve_slot(p, j) == s) != 0ull) return;
        }
    // the column of the input row that holds state column c (the heads may lie anywhere in the input row, they are packed in the state)
    int cin = -1, base = 0;
#pragma unroll
    for (int h = 0; h < SEG_CE_MAX_HEADS; ++h) {
        if (h < p.H && c >= base && c < base + p.C[h]) cin = p.col0[h] + (c - base);
        base += h < p.H ? p.C[h] : 0;
    }
    const bool live = c < p.ld && cin >= 0;
    float* dst = p.rows + (size_t)s * p.ld + (live ? c : 0);
    const float* src = p.x + (live ? cin : 0);
    float v = live ? *dst : 0.f;
    int n = 0, jl = i;
    if (!p.slots) {
        if (live) v = ve_fold(v, src[(size_t)i * p.ld_in], p.method);
        n = 1;
    } else {
        for (int j0 = i; j0 < p.B; j0 += 64) {
            const int j = j0 + lane;
            unsigned long long m = __ballot(j < p.B && ve_slot(p, j) == s);
            n += __popcll(m);
            while (m) {                                                         // VE_GROUP clips per round: their loads go out together, the folds stay in order
                int r[VE_GROUP];
                float xs[VE_GROUP];
#pragma unroll
                for (int u = 0; u < VE_GROUP; ++u) {
                    r[u] = m ? j0 + __ffsll((long long)m) - 1 : -1;
                    m &= m - 1;                                                 // 0 stays 0
                }
#pragma unroll
                for (int u = 0; u < VE_GROUP; ++u) xs[u] = (live && r[u] >= 0) ? src[(size_t)r[u] * p.ld_in] : 0.f;
#pragma unroll
                for (int u = 0; u < VE_GROUP; ++u)
                    if (r[u] >= 0) { v = ve_fold(v, xs[u], p.method); jl = r[u]; }
            }
        }
    }
    if (live) *dst = v;
    if (blockIdx.y == 0 && wave == 0) {
        if (lane < p.H) p.vlabels[(size_t)s * p.H + lane] = p.labels[(size_t)jl * p.H + lane];       // the video's label is its LAST clip's
        if (lane == 0) p.views[s] += n;
    }
}

struct VeTopkParams {
    const float* rows; const int64_t* vlabels;
    int n, H, ld, nks, nblocks;
    int col0[SEG_CE_MAX_HEADS], C[SEG_CE_MAX_HEADS], ks[SEG_CE_MAX_KS];
    int* rank; int* pred; int* result; int* parts; unsigned* counter; const unsigned* dropped;
};

struct VeOut { int rank, pred, nonfinite; };

__device__ __forceinline__ float ve_key(float x) { return x != x ? INFINITY : x; }
__device__ __forceinline__ bool ve_nonfinite(float x) { return !(fabsf(x) <= 3.402823466e+38f); }
__device__ __forceinline__ int wave_min_int(int v) { return -wave_max(-v); }

// C <= 64 * NR: element c = lane + 64 j lives in register j; y < 0: no valid label (rank -1)
template <int NR>
__device__ __forceinline__ VeOut ve_regs(const float* __restrict__ seg, int C, int y, int lane) {
    float v[NR];
    bool nf = false;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const bool in = lane + 64 * j < C;
        const float x = in ? seg[lane + 64 * j] : 0.f;
        nf |= in && ve_nonfinite(x);
        v[j] = in ? ve_key(x) : -INFINITY;
    }
    float m = v[0], zy = -INFINITY;
#pragma unroll
    for (int j = 0; j < NR; ++j) { m = fmaxf(m, v[j]); zy = lane + 64 * j == y ? v[j] : zy; }
    m = wave_max(m);
    zy = __shfl(zy, y & 63, 64);
    int r = 0, best = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int c = lane + 64 * j;
        const bool in = c < C;
        r += (in && y >= 0) ? outranks(v[j], zy, c, y) : 0;
        best = (in && v[j] == m) ? min(best, c) : best;
    }
    VeOut o;
    o.rank = y >= 0 ? wave_sum(r) : -1;
    o.pred = wave_min_int(best);
    o.nonfinite = __ballot(nf) != 0ull ? 1 : 0;
    return o;
}

// C > 512: a lane-strided pass; every lane owns at least one element
__device__ __forceinline__ VeOut ve_loop(const float* __restrict__ seg, int C, int y, int lane) {
    const float zy = y >= 0 ? ve_key(seg[y]) : 0.f;
    float bv = -INFINITY;
    int bi = 0x7fffffff, r = 0;
    bool nf = false;
#pragma unroll 4
    for (int c = lane; c < C; c += 64) {
        const float x = seg[c];
        nf |= ve_nonfinite(x);
        const float k = ve_key(x);
        r += y >= 0 ? outranks(k, zy, c, y) : 0;
        if (k > bv || bi == 0x7fffffff) { bv = k; bi = c; }              // strictly greater: the lane keeps its lowest column of the value
    }
    const float m = wave_max(bv);
    VeOut o;
    o.rank = y >= 0 ? wave_sum(r) : -1;
    o.pred = wave_min_int(bv == m ? bi : 0x7fffffff);
    o.nonfinite = __ballot(nf) != 0ull ? 1 : 0;
    return o;
}

__global__ __launch_bounds__(256) void view_ensemble_topk_kernel(VeTopkParams p) {
    __shared__ int part_s[VE_WAVES][VE_PART_STRIDE];
    __shared__ int col0_s[SEG_CE_MAX_HEADS], C_s[SEG_CE_MAX_HEADS], ks_s[SEG_CE_MAX_KS];
    __shared__ bool last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < SEG_CE_MAX_HEADS) { col0_s[tid] = p.col0[tid]; C_s[tid] = p.C[tid]; }
    if (tid < SEG_CE_MAX_KS) ks_s[tid] = p.ks[tid];
    if (lane < VE_PART_STRIDE) part_s[wave][lane] = 0;
    __syncthreads();
    for (int v = blockIdx.x * VE_WAVES + wave; v < p.n; v += p.nblocks * VE_WAVES) {      // the wave's videos, in this order
        const float* row = p.rows + (size_t)v * p.ld;
        int nf = 0;
#pragma unroll 1
        for (int h = 0; h < p.H; ++h) {
            const int C = C_s[h];
            const int64_t y64 = p.vlabels[(size_t)v * p.H + h];
            const int y = __builtin_amdgcn_readfirstlane((y64 < 0 || y64 >= C) ? -1 : (int)y64);        // the same in every lane
            const float* seg = row + col0_s[h];
            VeOut o;
            if (C <= 64) o = ve_regs<1>(seg, C, y, lane);
            else if (C <= 128) o = ve_regs<2>(seg, C, y, lane);
            else if (C <= 256) o = ve_regs<4>(seg, C, y, lane);
            else if (C <= 512) o = ve_regs<8>(seg, C, y, lane);
            else o = ve_loop(seg, C, y, lane);
            nf |= o.nonfinite;
            if (lane == 0) {
                p.rank[(size_t)v * p.H + h] = o.rank;
                p.pred[(size_t)v * p.H + h] = o.pred;
                if (y < 0) part_s[wave][1 + h] += 1;
                else
                    for (int k = 0; k < p.nks; ++k) part_s[wave][1 + SEG_CE_MAX_HEADS + k * SEG_CE_MAX_HEADS + h] += o.rank < ks_s[k] ? 1 : 0;
            }
        }
        if (lane == 0) part_s[wave][0] += nf;
    }
    __syncthreads();
    // Workgroup partials -> the state's partial area, the last workgroup to arrive adds them (the hand-off of seg_ce.hip: wave 0 stores every
    // handed-off word write-through at agent scope, drains its stores, then ONE relaxed agent-scope add draws the ticket; the reader loads
    // every such word at agent scope)
    if (wave == 0) {
        if (lane < VE_PART_WORDS)
            __hip_atomic_store(p.parts + (size_t)blockIdx.x * VE_PART_STRIDE + lane,
                               (part_s[0][lane] + part_s[1][lane]) + (part_s[2][lane] + part_s[3][lane]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0)
            last_s = __hip_atomic_fetch_add(p.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)p.nblocks - 1;
    }
    __syncthreads();
    if (!last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (tid < VE_PART_WORDS) {
        int sum = 0;
        for (int b = 0; b < p.nblocks; ++b)                                     // workgroup order: the same on every run
            sum += __hip_atomic_load(p.parts + (size_t)b * VE_PART_STRIDE + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // result: n, n_dropped, n_nonfinite, n_invalid[H], correct[nks][H]
        if (tid == 0) p.result[2] = sum;
        else if (tid <= SEG_CE_MAX_HEADS) {
            if (tid - 1 < p.H) p.result[3 + tid - 1] = sum;
        } else {
            const int k = (tid - 1 - SEG_CE_MAX_HEADS) / SEG_CE_MAX_HEADS, h = (tid - 1 - SEG_CE_MAX_HEADS) % SEG_CE_MAX_HEADS;
            if (k < p.nks && h < p.H) p.result[3 + p.H + k * p.H + h] = sum;
        }
    } else if (tid == 64) {
        p.result[0] = p.n;
        p.result[1] = (int)__hip_atomic_load(p.dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // left zero for the next launch
    }
}

static int ve_check_state(const char* who, int capacity, int H, const int* C) {
    EGX_CHECK(C, "%s: null pointer argument", who);
    EGX_CHECK(H >= 1 && H <= SEG_CE_MAX_HEADS, "%s: H=%d (needs 1 <= H <= %d heads)", who, H, SEG_CE_MAX_HEADS);
    EGX_CHECK(capacity >= 1, "%s: capacity=%d (needs capacity >= 1 videos)", who, capacity);
    long long ld = 0;
    for (int h = 0; h < H; ++h) {
        EGX_CHECK(C[h] >= 1 && C[h] <= SEG_CE_MAX_CLASSES, "%s: head %d has C=%d classes (needs 1 <= C <= %d)", who, h, C[h], SEG_CE_MAX_CLASSES);
        ld += C[h];
    }
    EGX_CHECK((long long)capacity * ld <= (1ll << 31), "%s: capacity * sum(C) = %lld state elements (needs <= 2^31)", who, (long long)capacity * ld);
    return 0;
}

size_t view_ensemble_state_bytes(int capacity, int H, const int* C, size_t* offsets) {
    if (ve_check_state("view_ensemble_state", capacity, H, C)) return 0;
    const VeLayout L = ve_layout(capacity, H, C);
    if (offsets) { offsets[0] = L.labels; offsets[1] = L.views; offsets[2] = L.rows; }
    return L.bytes;
}

int view_ensemble_update(const float* preds, int ld, int B, int H, const int* col0, const int* C, const int64_t* labels, const void* slots,
                         int slot_bytes, int slot0, int method, int capacity, void* state, hipStream_t st) {
    EGX_CHECK(preds && labels && col0 && C && state, "view_ensemble_update: null pointer argument");
    if (ve_check_state("view_ensemble_update", capacity, H, C)) return 1;
    EGX_CHECK(B >= 1 && B <= VIEW_ENS_MAX_BATCH, "view_ensemble_update: B=%d (needs 1 <= B <= %d clips)", B, VIEW_ENS_MAX_BATCH);
    EGX_CHECK(ld >= 1, "view_ensemble_update: ld=%d (needs ld >= 1)", ld);
    if (check_head_windows("view_ensemble_update", ld, H, col0, C)) return 1;
    EGX_CHECK(method == VIEW_ENS_SUM || method == VIEW_ENS_MAX, "view_ensemble_update: method=%d (needs 0 = sum or 1 = max)", method);
    if (slots) EGX_CHECK(slot_bytes == 4 || slot_bytes == 8, "view_ensemble_update: slot_bytes=%d (needs 4 = int32 or 8 = int64)", slot_bytes);
    else EGX_CHECK(slot0 >= 0 && (long long)slot0 + B <= capacity, "view_ensemble_update: slot0=%d B=%d (needs 0 <= slot0 and slot0 + B <= capacity = %d)", slot0, B, capacity);
    const VeLayout L = ve_layout(capacity, H, C);
    VeUpdateParams p;
    p.x = preds; p.labels = labels; p.slots = slots; p.slot_i64 = slot_bytes == 8; p.slot0 = slot0;
    p.B = B; p.H = H; p.ld_in = ld; p.ld = L.ld; p.capacity = capacity; p.method = method;
    for (int h = 0; h < SEG_CE_MAX_HEADS; ++h) { p.col0[h] = h < H ? col0[h] : 0; p.C[h] = h < H ? C[h] : 0; }
    char* s = (char*)state;
    p.rows = (float*)(s + L.rows); p.vlabels = (int64_t*)(s + L.labels); p.views = (int*)(s + L.views);
    p.dropped = (unsigned*)s + VE_DROPPED_WORD;
    hipLaunchKernelGGL(view_ensemble_update_kernel, dim3((unsigned)B, (unsigned)cdiv(L.ld, 256)), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

int view_ensemble_topk(int n, int capacity, int H, const int* C, const int* ks, int n_ks, void* state, int* rank, int* pred, int* result,
                       hipStream_t st) {
    EGX_CHECK(C && ks && state && rank && pred && result, "view_ensemble_topk: null pointer argument");
    if (ve_check_state("view_ensemble_topk", capacity, H, C)) return 1;
    EGX_CHECK(n >= 1 && n <= capacity, "view_ensemble_topk: n=%d (needs 1 <= n <= capacity = %d)", n, capacity);
    EGX_CHECK(n_ks >= 1 && n_ks <= SEG_CE_MAX_KS, "view_ensemble_topk: n_ks=%d (needs 1 <= n_ks <= %d)", n_ks, SEG_CE_MAX_KS);
    int min_c = SEG_CE_MAX_CLASSES;
    for (int h = 0; h < H; ++h) min_c = C[h] < min_c ? C[h] : min_c;
    for (int k = 0; k < n_ks; ++k)
        EGX_CHECK(ks[k] >= 1 && ks[k] <= min_c, "view_ensemble_topk: ks[%d]=%d (needs 1 <= k <= %d, the narrowest head)", k, ks[k], min_c);
    const VeLayout L = ve_layout(capacity, H, C);
    VeTopkParams p;
    char* s = (char*)state;
    p.rows = (const float*)(s + L.rows); p.vlabels = (const int64_t*)(s + L.labels);
    p.n = n; p.H = H; p.ld = L.ld; p.nks = n_ks;
    p.nblocks = cdiv(n, VE_WAVES) < VE_MAX_BLOCKS ? cdiv(n, VE_WAVES) : VE_MAX_BLOCKS;
    int base = 0;
    for (int h = 0; h < SEG_CE_MAX_HEADS; ++h) { p.col0[h] = base; p.C[h] = h < H ? C[h] : 0; base += p.C[h]; }
    for (int k = 0; k < SEG_CE_MAX_KS; ++k) p.ks[k] = k < n_ks ? ks[k] : 0;
    p.rank = rank; p.pred = pred; p.result = result;
    p.parts = (int*)(s + L.parts); p.counter = (unsigned*)s; p.dropped = (const unsigned*)s + VE_DROPPED_WORD;
    hipLaunchKernelGGL(view_ensemble_topk_kernel, dim3((unsigned)p.nblocks), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
