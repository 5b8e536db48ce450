// The TTM / LAM validation epoch on the device: merged per-row scores and the VOC-style average precision of both classes.
// PostProcessor.update / _merge_output (HHI/utils/ttm/utils.py:46-114; HHI/utils/lam/utils.py: every input row is its own row) and
// run_evaluation (HHI/utils/ttm/metrics.py:26-71, 138-199, 232-247):
//   score = softmax(mean over the row's windows of logits (n_w, 2))[1], label = the label of the row's first window
//   AP of a class: rows by score descending, tp = cumsum(label), precision tp / k made non-increasing from the right, summed over the
//   rows where recall changes (the positive rows); class 0 on (1 - score, 1 - label), i.e. rows by score ascending; confusion counts
//   at score >= 0.5.
//
//   update  : a thread per window. The first window of a run of equal slots owns the run: it adds the run's logits in window order onto
//             the slot's stored sum, so a row's sum is the same left fold however its windows are split across calls. No float atomics.
//   finish  : a workgroup per tile of SEG_AP_TILE rows: fp32 mean and softmax, the score, the six counts by integer atomics.
//   sort    : a stable LSD radix sort of (key, row | label << 31), 8-bit digits, 4 passes; the key is the order-preserving image of the
//             fp32 score. Per pass: tile histograms (LDS integer atomics), a workgroup per digit scans its row of tile counts in tile
//             order, and the scatter ranks its tile again - inside a wave by ballots, across rounds and waves by per-wave LDS counters.
//             Class 1 sorts by the complemented digit (descending, the lower row first among equal keys), class 0 runs the four passes
//             again on the plain digit (ascending, the lower row first): the tie rule holds in both without a tie-group pass.
//   AP      : tile counts -> their prefix -> tile maxima of the rational precisions (tp_a k_b against tp_b k_a in 64 bits) -> their
//             suffix -> the fp64 terms of the positive rows, per tile, added in tile order by one workgroup. Every cross-tile step is a
//             launch boundary: nothing inside a launch depends on another workgroup.
//   N <= one tile: ONE workgroup runs the eight sort passes and both classes' AP (seg_ap_small_kernel), after the finish launch.
// The launch count depends on N only.
#include "common.h"
#include "kernels.h"

namespace egx {

constexpr int SAP_THREADS = 256, SAP_WAVES = 4, SAP_IPT = 16;      // a tile = 256 threads x 16 items
constexpr int SAP_MAX_TILES = SEG_AP_MAX_ROWS / SEG_AP_TILE;       // 4096: one thread per 16 tiles in the single-workgroup scans
static_assert(SAP_THREADS * SAP_IPT == SEG_AP_TILE && SAP_MAX_TILES == SEG_AP_TILE, "segment_ap: tile geometry");
constexpr int SAP_N_COUNTS = 7;                                    // n, n_pos, TP, FN, FP, TN, n_nonfinite
constexpr uint32_t SAP_ROW_MASK = 0x00ffffffu;                     // row index bits of a sort value; bit 31: the row's label

// ---- scratch: [persistent state | work], carved for `capacity` rows ------------------------------------------------------------------
struct SapBufs {
    float2* sum; int* count; int* label;                           // state: zero = empty
    uint32_t* key[2]; uint32_t* val[2];                            // the sort's ping-pong buffers
    uint32_t* sorted1;                                             // class 1's sorted values (class 0's end in val[1])
    uint32_t* hist; uint32_t* excl; uint32_t* dtot;                // [256][tiles] digit-major, [256]
    int* ap_cnt; int* ap_pre; int2* ap_max; int2* ap_suf; double* ap_part;      // [2][SAP_MAX_TILES]
};

static size_t sap_carve(void* scratch, int capacity, SapBufs* b) {
    size_t off = 0;
    char* base = (char*)scratch;
    auto take = [&](size_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
    const size_t cap = (size_t)capacity, tiles = (size_t)cdiv(capacity, SEG_AP_TILE);
    SapBufs t;
    t.sum = (float2*)take(cap * 8); t.count = (int*)take(cap * 4); t.label = (int*)take(cap * 4);
    for (int i = 0; i < 2; ++i) { t.key[i] = (uint32_t*)take(cap * 4); t.val[i] = (uint32_t*)take(cap * 4); }
    t.sorted1 = (uint32_t*)take(cap * 4);
    t.hist = (uint32_t*)take(256 * tiles * 4); t.excl = (uint32_t*)take(256 * tiles * 4); t.dtot = (uint32_t*)take(256 * 4);
    t.ap_cnt = (int*)take(2 * SAP_MAX_TILES * 4); t.ap_pre = (int*)take(2 * SAP_MAX_TILES * 4);
    t.ap_max = (int2*)take(2 * SAP_MAX_TILES * 8); t.ap_suf = (int2*)take(2 * SAP_MAX_TILES * 8);
    t.ap_part = (double*)take(2 * SAP_MAX_TILES * 8);
    if (b) *b = t;
    return off;
}

static int sap_check_rows(const char* who, const char* what, int n) {
    EGX_CHECK(n >= 1 && n <= SEG_AP_MAX_ROWS, "%s: %s=%d (needs 1 <= %s <= %d rows)", who, what, n, what, SEG_AP_MAX_ROWS);
    return 0;
}

size_t segment_ap_scratch_bytes(int capacity) {
    if (sap_check_rows("segment_ap_scratch", "capacity", capacity)) return 0;
    return sap_carve(nullptr, capacity, nullptr);
}

// ---- update ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SAP_THREADS) void seg_score_update_kernel(const float* logits, int ld, int B, const int64_t* slots, int slot0,
                                                                       const int64_t* labels, int capacity, float2* sum, int* count,
                                                                       int* label) {
    const int i = blockIdx.x * SAP_THREADS + threadIdx.x;
    if (i >= B) return;
    const int64_t s = slots ? slots[i] : (int64_t)slot0 + i;
    if (i > 0 && (slots ? slots[i - 1] : s - 1) == s) return;       // not the first window of its run: the run's owner adds it
    if (s < 0 || s >= capacity) return;                             // a slot outside the accumulator is dropped, never written
    float2 a = sum[s];
    const int c = count[s];
    if (c == 0) label[s] = labels[i] == 1 ? 1 : 0;                  // utils.py:78: the label of the row's first window
    int j = i;
    do {
        const float* row = logits + (size_t)j * ld;
        a.x += row[0];
        a.y += row[1];
        ++j;
    } while (slots && j < B && slots[j] == s);
    sum[s] = a;
    count[s] = c + (j - i);
}

int segment_scores_update(const float* logits, int ld, int B, const int64_t* slots, int slot0, const int64_t* labels, int capacity,
                          void* scratch, hipStream_t st) {
    EGX_CHECK(logits && labels && scratch, "segment_scores_update: null pointer argument (logits, labels and scratch are required)");
    if (sap_check_rows("segment_scores_update", "capacity", capacity)) return 1;
    EGX_CHECK(ld >= 2, "segment_scores_update: ld=%d (needs ld >= 2: a row holds the two class logits)", ld);
    EGX_CHECK(B >= 1 && B <= SEG_AP_MAX_ROWS, "segment_scores_update: B=%d (needs 1 <= B <= %d windows)", B, SEG_AP_MAX_ROWS);
    EGX_CHECK(slots || (slot0 >= 0 && slot0 <= capacity - B),
              "segment_scores_update: rows %d .. %d without slots (needs 0 <= slot0 and slot0 + B <= capacity = %d)", slot0, slot0 + B - 1, capacity);
    SapBufs b;
    sap_carve(scratch, capacity, &b);
    hipLaunchKernelGGL(seg_score_update_kernel, dim3((unsigned)cdiv(B, SAP_THREADS)), dim3(SAP_THREADS), 0, st, logits, ld, B, slots, slot0,
                       labels, capacity, b.sum, b.count, b.label);
    EGX_LAUNCH_CHECK();
    return 0;
}

// ---- finish ------------------------------------------------------------------------------------------------------------------------
// the order-preserving image of an fp32 value: a < b as floats <=> key(a) < key(b) as unsigned; the canonical NaN ranks above +inf
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t u = __float_as_uint(s);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__global__ __launch_bounds__(SAP_THREADS) void seg_score_finish_kernel(int N, const float2* sum, const int* count, const int* label,
                                                                       float* score, unsigned long long* result) {
    __shared__ int cnt_s[SAP_WAVES][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int c[6] = {0, 0, 0, 0, 0, 0};                                  // n_pos, TP, FN, FP, TN, n_nonfinite
    for (int r = 0; r < SAP_IPT; ++r) {
        const int i = blockIdx.x * SEG_AP_TILE + r * SAP_THREADS + tid;
        if (i >= N) break;
        const float2 s = sum[i];
        const float n = (float)count[i];                            // a row without a window: 0 / 0, counted as non-finite
        const float a = s.x / n, b = s.y / n;
        const float m = fmaxf(a, b);
        const float e0 = expf(a - m), e1 = expf(b - m);             // max-subtracted: the larger term is 1
        float sc = e1 / (e0 + e1);
        const bool finite = sc == sc;                               // in [0, 1] or NaN
        if (!finite) sc = __uint_as_float(0x7fc00000u);             // ONE NaN: the sort's order of such a row is defined
        score[i] = sc;
        const int pos = label[i], pred = sc >= 0.5f ? 1 : 0;        // metrics.py:233-236: a score of exactly 0.5 is predicted positive
        c[0] += pos; c[1] += pred & pos; c[2] += (1 - pred) & pos; c[3] += pred & (1 - pos); c[4] += (1 - pred) & (1 - pos);
        c[5] += finite ? 0 : 1;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int w = wave_sum(c[k]);
        if (lane == 0) cnt_s[wave][k] = w;
    }
    __syncthreads();
    if (tid < 6) {
        const int v = (cnt_s[0][tid] + cnt_s[1][tid]) + (cnt_s[2][tid] + cnt_s[3][tid]);
        if (v) atomicAdd(result + 1 + tid, (unsigned long long)v);   // integers: the sum does not depend on the order
    }
}

// ---- workgroup scans (256 threads), fixed order ------------------------------------------------------------------------------------
// exclusive prefix sum of v over the threads; *total = the sum. lds: SAP_WAVES ints.
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    __syncthreads();                                                // lds may still be read from an earlier scan
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SAP_WAVES; ++w) {
        const int t = lds[w];
        if (w < wave) base += t;
        tot += t;
    }
    *total = tot;
    return base + x - v;
}

// A precision tp / k as an exact rational (int2: x = tp, y = k >= 1); {0, 1} is zero. tp, k <= 2^24: the products stay below 2^48.
__device__ __forceinline__ int2 rat_max(int2 a, int2 b) {
    return (long long)a.x * b.y >= (long long)b.x * a.y ? a : b;
}
// maximum of v over the threads AFTER this one ({0, 1} for the last); *total = the maximum over all. lds: SAP_WAVES int2.
__device__ __forceinline__ int2 block_suffix_max(int2 v, int2* lds, int2* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int2 x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int2 y;
        y.x = __shfl_down(x.x, o, 64);
        y.y = __shfl_down(x.y, o, 64);
        if (lane + o < 64) x = rat_max(x, y);
    }
    int2 e;
    e.x = __shfl_down(x.x, 1, 64);
    e.y = __shfl_down(x.y, 1, 64);
    if (lane == 63) e = make_int2(0, 1);
    __syncthreads();
    if (lane == 0) lds[wave] = x;
    __syncthreads();
    int2 tot = make_int2(0, 1);
#pragma unroll
    for (int w = SAP_WAVES - 1; w >= 0; --w) {
        const int2 t = lds[w];
        if (w > wave) e = rat_max(e, t);
        tot = rat_max(tot, t);
    }
    *total = tot;
    return e;
}
// sum of v over the threads by a fixed tree (wave butterflies, then the four waves in order): the same bits in every thread and run
__device__ __forceinline__ double block_sum(double v, double* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double w = wave_sum(v);
    __syncthreads();
    if (lane == 0) lds[wave] = w;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// ---- the radix sort ----------------------------------------------------------------------------------------------------------------
struct SortPass {
    const uint32_t* key_in; const uint32_t* val_in;                 // NULL key_in: pass 0 reads score / label (the value is row | label << 31)
    const float* score; const int* label;
    uint32_t* key_out; uint32_t* val_out; int* order_out;           // NULL key_out: the last pass writes the values and the row order only
    int shift; uint32_t flip;                                       // digit = ((key >> shift) & 255) ^ flip; flip 255 sorts descending
};

// pass `pass` (0 .. 3) of class `cls`: score -> [0] -> [1] -> [0] -> the class's sorted values + order
__host__ __device__ inline SortPass sort_pass(const SapBufs& b, const float* score, int* order1, int* order0, int cls, int pass) {
    SortPass p;
    p.score = score; p.label = b.label;
    p.key_in = pass == 0 ? nullptr : b.key[(pass - 1) & 1];
    p.val_in = pass == 0 ? nullptr : b.val[(pass - 1) & 1];
    p.key_out = pass == 3 ? nullptr : b.key[pass & 1];
    p.val_out = pass == 3 ? (cls == 1 ? b.sorted1 : b.val[1]) : b.val[pass & 1];
    p.order_out = pass == 3 ? (cls == 1 ? order1 : order0) : nullptr;
    p.shift = 8 * pass;
    p.flip = cls == 1 ? 255u : 0u;
    return p;
}

__device__ __forceinline__ uint32_t sort_key_at(const SortPass& p, int i) { return p.key_in ? p.key_in[i] : score_key(p.score[i]); }
__device__ __forceinline__ uint32_t sort_val_at(const SortPass& p, int i) {
    return p.val_in ? p.val_in[i] : ((uint32_t)i | ((uint32_t)p.label[i] << 31));
}

__global__ __launch_bounds__(SAP_THREADS) void seg_sort_hist_kernel(SortPass p, int N, int tiles, uint32_t* hist) {
    __shared__ uint32_t h_s[256];
    const int tid = threadIdx.x;
    h_s[tid] = 0;
    __syncthreads();
    for (int r = 0; r < SAP_IPT; ++r) {
        const int i = blockIdx.x * SEG_AP_TILE + r * SAP_THREADS + tid;
        if (i < N) atomicAdd(&h_s[((sort_key_at(p, i) >> p.shift) & 255u) ^ p.flip], 1u);
    }
    __syncthreads();
    hist[(size_t)tid * tiles + blockIdx.x] = h_s[tid];
}

// workgroup d: the exclusive prefix of digit d's tile counts in tile order, and the digit's total. tiles <= 4096 = 256 threads x 16.
__global__ __launch_bounds__(SAP_THREADS) void seg_sort_scan_kernel(const uint32_t* hist, int tiles, uint32_t* excl, uint32_t* dtot) {
    __shared__ int scan_s[SAP_WAVES];
    const int tid = threadIdx.x;
    const uint32_t* row = hist + (size_t)blockIdx.x * tiles;
    uint32_t* out = excl + (size_t)blockIdx.x * tiles;
    int v[SAP_IPT], s = 0;
#pragma unroll
    for (int j = 0; j < SAP_IPT; ++j) {
        const int t = tid * SAP_IPT + j;
        v[j] = t < tiles ? (int)row[t] : 0;
        s += v[j];
    }
    int total;
    int run = block_excl_scan(s, scan_s, &total);
#pragma unroll
    for (int j = 0; j < SAP_IPT; ++j) {
        const int t = tid * SAP_IPT + j;
        if (t < tiles) out[t] = (uint32_t)run;
        run += v[j];
    }
    if (tid == 0) dtot[blockIdx.x] = (uint32_t)total;
}

// The tile's items: wave w holds positions tile0 + 1024 w + 64 r + lane (r = 0 .. 15), so a wave's rounds and the waves are in position
// order. -> off[r]: the number of items of the same digit before the item in its wave; whist_s[w][d]: the items of digit d in the waves
// before w; tot_s[d]: the tile's count.
__device__ __forceinline__ void rank_tile(const SortPass& p, int tile0, int N, uint32_t (&key)[SAP_IPT], uint32_t (&val)[SAP_IPT],
                                          int (&off)[SAP_IPT], uint32_t (*whist_s)[256], uint32_t* tot_s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int w = 0; w < SAP_WAVES; ++w) whist_s[w][tid] = 0;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < SAP_IPT; ++r) {
        const int i = tile0 + wave * (64 * SAP_IPT) + r * 64 + lane;
        const bool active = i < N;
        key[r] = active ? sort_key_at(p, i) : 0u;
        val[r] = active ? sort_val_at(p, i) : 0u;
        const uint32_t d = ((key[r] >> p.shift) & 255u) ^ p.flip;
        unsigned long long same = __ballot(active);                 // the active lanes with this lane's digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(active && on);
            same &= on ? bal : ~bal;
        }
        if (!active) same = 1ull << lane;                           // keeps the shuffle below defined; adds nothing
        const int rank = __popcll(same & below);
        uint32_t before = 0;
        if (active && rank == 0) before = atomicAdd(&whist_s[wave][d], (uint32_t)__popcll(same));
        before = __shfl(before, __ffsll((long long)same) - 1, 64);   // from the group's first lane
        off[r] = (int)before + rank;
    }
    __syncthreads();
    uint32_t run = 0;
#pragma unroll
    for (int w = 0; w < SAP_WAVES; ++w) {
        const uint32_t c = whist_s[w][tid];
        whist_s[w][tid] = run;
        run += c;
    }
    tot_s[tid] = run;
    __syncthreads();
}

__device__ __forceinline__ void scatter_tile(const SortPass& p, int tile0, int N, const uint32_t (&key)[SAP_IPT], const uint32_t (&val)[SAP_IPT],
                                             const int (&off)[SAP_IPT], const uint32_t (*whist_s)[256], const uint32_t* base_s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < SAP_IPT; ++r) {
        const int i = tile0 + wave * (64 * SAP_IPT) + r * 64 + lane;
        if (i >= N) continue;
        const uint32_t d = ((key[r] >> p.shift) & 255u) ^ p.flip;
        const uint32_t dst = base_s[d] + whist_s[wave][d] + (uint32_t)off[r];     // < N: a permutation of the N active items
        if (p.key_out) p.key_out[dst] = key[r];
        p.val_out[dst] = val[r];
        if (p.order_out) p.order_out[dst] = (int)(val[r] & SAP_ROW_MASK);
    }
}

__global__ __launch_bounds__(SAP_THREADS) void seg_sort_scatter_kernel(SortPass p, int N, int tiles, const uint32_t* excl, const uint32_t* dtot) {
    __shared__ uint32_t whist_s[SAP_WAVES][256];
    __shared__ uint32_t tot_s[256], base_s[256];
    __shared__ int scan_s[SAP_WAVES];
    const int tid = threadIdx.x, tile0 = blockIdx.x * SEG_AP_TILE;
    uint32_t key[SAP_IPT], val[SAP_IPT];
    int off[SAP_IPT];
    rank_tile(p, tile0, N, key, val, off, whist_s, tot_s);
    int total;
    const int dbase = block_excl_scan((int)dtot[tid], scan_s, &total);      // the digits before this one, over all tiles
    base_s[tid] = (uint32_t)dbase + excl[(size_t)tid * tiles + blockIdx.x];
    __syncthreads();
    scatter_tile(p, tile0, N, key, val, off, whist_s, base_s);
}

// ---- the AP pass over a class's sorted values ----------------------------------------------------------------------------------------
struct ApTile { int count; int2 best; double sum; };
// Thread t holds positions tile0 + 16 t + j. pre: the class's positives before the tile; later: the largest precision after the tile;
// P: the class's positives. count needs none of them, best needs pre, sum needs all three.
__device__ __forceinline__ ApTile ap_tile(const uint32_t* sorted, int cls, int tile0, int N, int pre, int2 later, int P, int* scan_s,
                                          int2* max_s, double* sum_s) {
    const int tid = threadIdx.x;
    const int p0 = tile0 + tid * SAP_IPT;
    int lab[SAP_IPT], s = 0;
#pragma unroll
    for (int j = 0; j < SAP_IPT; ++j) {
        const int i = p0 + j;
        lab[j] = i < N ? (int)((sorted[i] >> 31) ^ (uint32_t)(cls == 0)) : 0;       // class 0 scores 1 - label
        s += lab[j];
    }
    ApTile out;
    int tp = pre + block_excl_scan(s, scan_s, &out.count);
    int tps[SAP_IPT];
    int2 mine = make_int2(0, 1);
#pragma unroll
    for (int j = 0; j < SAP_IPT; ++j) {
        tp += lab[j];
        tps[j] = tp;
        if (p0 + j < N) mine = rat_max(mine, make_int2(tp, p0 + j + 1));
    }
    int2 env = rat_max(block_suffix_max(mine, max_s, &out.best), later);           // the largest precision after this thread's positions
    const double dP = (double)P;
    double acc = 0.0;
#pragma unroll
    for (int j = SAP_IPT - 1; j >= 0; --j) {
        if (p0 + j >= N) continue;
        env = rat_max(env, make_int2(tps[j], p0 + j + 1));
        // metrics.py:68-70: (recall_i - recall_{i-1}) * precision_i where recall changes, i.e. at a positive row
        if (lab[j]) acc += ((double)tps[j] / dP - (double)(tps[j] - 1) / dP) * ((double)env.x / (double)env.y);
    }
    out.sum = block_sum(acc, sum_s);
    return out;
}

#define SAP_AP_LDS() \
    __shared__ int scan_s[SAP_WAVES]; \
    __shared__ int2 max_s[SAP_WAVES]; \
    __shared__ double sum_s[SAP_WAVES]

// grid (tiles, 2 classes); stage 0: tile counts, 1: tile maxima, 2: tile terms
__global__ __launch_bounds__(SAP_THREADS) void seg_ap_tile_kernel(SapBufs b, int N, int stage, const long long* result) {
    SAP_AP_LDS();
    const int cls = blockIdx.y, t = blockIdx.x, at = cls * SAP_MAX_TILES + t;
    const uint32_t* sorted = cls == 1 ? b.sorted1 : b.val[1];
    const int n_pos = stage == 2 ? (int)result[1] : 0;
    const int pre = stage >= 1 ? b.ap_pre[at] : 0;
    int2 later = make_int2(0, 1);
    if (stage == 2) later = b.ap_suf[at];
    const ApTile r = ap_tile(sorted, cls, t * SEG_AP_TILE, N, pre, later, cls == 1 ? n_pos : N - n_pos, scan_s, max_s, sum_s);
    if (threadIdx.x != 0) return;
    if (stage == 0) b.ap_cnt[at] = r.count;
    else if (stage == 1) b.ap_max[at] = r.best;
    else b.ap_part[at] = r.sum;
}

// one workgroup per class over the tiles, thread t holding tiles 16 t + j. stage 0: prefix of the counts; 1: suffix of the maxima
__global__ __launch_bounds__(SAP_THREADS) void seg_ap_scan_kernel(SapBufs b, int tiles, int stage) {
    SAP_AP_LDS();
    (void)sum_s;
    const int tid = threadIdx.x, at0 = blockIdx.x * SAP_MAX_TILES + tid * SAP_IPT;
    if (stage == 0) {
        int v[SAP_IPT], s = 0;
#pragma unroll
        for (int j = 0; j < SAP_IPT; ++j) {
            v[j] = tid * SAP_IPT + j < tiles ? b.ap_cnt[at0 + j] : 0;
            s += v[j];
        }
        int total;
        int run = block_excl_scan(s, scan_s, &total);
#pragma unroll
        for (int j = 0; j < SAP_IPT; ++j) {
            if (tid * SAP_IPT + j < tiles) b.ap_pre[at0 + j] = run;
            run += v[j];
        }
    } else {
        int2 v[SAP_IPT], mine = make_int2(0, 1);
#pragma unroll
        for (int j = 0; j < SAP_IPT; ++j) {
            v[j] = tid * SAP_IPT + j < tiles ? b.ap_max[at0 + j] : make_int2(0, 1);
            mine = rat_max(mine, v[j]);
        }
        int2 total;
        int2 run = block_suffix_max(mine, max_s, &total);
#pragma unroll
        for (int j = SAP_IPT - 1; j >= 0; --j) {
            if (tid * SAP_IPT + j < tiles) b.ap_suf[at0 + j] = run;
            run = rat_max(run, v[j]);
        }
    }
}

// result: int64 n, n_pos, TP, FN, FP, TN, n_nonfinite | fp64 AP0, AP1, mAP, acc
__device__ __forceinline__ void write_result(long long* result, int N, double ap0, double ap1) {
    const long long n_pos = result[1], bad = result[6];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (bad > 0 || n_pos == N) ap0 = nan;                           // a class without a positive row (metrics.py:157: 0 / 0)
    if (bad > 0 || n_pos == 0) ap1 = nan;
    double* f = (double*)(result + SAP_N_COUNTS);
    result[0] = N;
    f[0] = ap0; f[1] = ap1; f[2] = (ap0 + ap1) / 2.0;
    f[3] = (double)(result[2] + result[5]) / (double)N;
}

__global__ __launch_bounds__(SAP_THREADS) void seg_ap_final_kernel(SapBufs b, int N, int tiles, long long* result) {
    __shared__ double sum_s[SAP_WAVES];
    const int tid = threadIdx.x;
    double ap[2];
    for (int cls = 0; cls < 2; ++cls) {
        double acc = 0.0;                                           // the tile partials in tile order
        for (int j = 0; j < SAP_IPT; ++j)
            if (tid * SAP_IPT + j < tiles) acc += b.ap_part[cls * SAP_MAX_TILES + tid * SAP_IPT + j];
        ap[cls] = block_sum(acc, sum_s);
    }
    if (tid == 0) write_result(result, N, ap[0], ap[1]);
}

// N <= one tile: the eight sort passes through the global ping-pong buffers (a workgroup barrier orders them) and both classes' AP
__global__ __launch_bounds__(SAP_THREADS) void seg_ap_small_kernel(SapBufs b, int N, const float* score, int* order1, int* order0,
                                                                   long long* result) {
    __shared__ uint32_t whist_s[SAP_WAVES][256];
    __shared__ uint32_t tot_s[256], base_s[256];
    SAP_AP_LDS();
    const int tid = threadIdx.x;
    for (int cls = 1; cls >= 0; --cls)
        for (int pass = 0; pass < 4; ++pass) {
            const SortPass p = sort_pass(b, score, order1, order0, cls, pass);
            uint32_t key[SAP_IPT], val[SAP_IPT];
            int off[SAP_IPT];
            rank_tile(p, 0, N, key, val, off, whist_s, tot_s);
            int total;
            base_s[tid] = (uint32_t)block_excl_scan((int)tot_s[tid], scan_s, &total);
            __syncthreads();
            scatter_tile(p, 0, N, key, val, off, whist_s, base_s);
            __threadfence_block();
            __syncthreads();                                        // the next pass reads what this one wrote
        }
    const int n_pos = (int)result[1];
    double ap[2];
    for (int cls = 0; cls < 2; ++cls)
        ap[cls] = ap_tile(cls == 1 ? b.sorted1 : b.val[1], cls, 0, N, 0, make_int2(0, 1), cls == 1 ? n_pos : N - n_pos, scan_s, max_s, sum_s).sum;
    if (tid == 0) write_result(result, N, ap[0], ap[1]);
}

int segment_ap(int N, int capacity, void* scratch, float* score, int* order1, int* order0, void* result, hipStream_t st) {
    EGX_CHECK(scratch && score && order1 && order0 && result, "segment_ap: null pointer argument (scratch, score, order1, order0 and result are required)");
    if (sap_check_rows("segment_ap", "capacity", capacity)) return 1;
    EGX_CHECK(N >= 1 && N <= capacity, "segment_ap: N=%d (needs 1 <= N <= capacity = %d rows)", N, capacity);
    SapBufs b;
    sap_carve(scratch, capacity, &b);
    const int tiles = cdiv(N, SEG_AP_TILE);
    long long* res = (long long*)result;
    EGX_HIP(hipMemsetAsync(result, 0, SEGMENT_AP_RESULT_BYTES, st));
    hipLaunchKernelGGL(seg_score_finish_kernel, dim3((unsigned)tiles), dim3(SAP_THREADS), 0, st, N, b.sum, b.count, b.label, score,
                       (unsigned long long*)result);
    EGX_LAUNCH_CHECK();
    if (tiles == 1) {
        hipLaunchKernelGGL(seg_ap_small_kernel, dim3(1), dim3(SAP_THREADS), 0, st, b, N, score, order1, order0, res);
        EGX_LAUNCH_CHECK();
        return 0;
    }
    for (int cls = 1; cls >= 0; --cls)
        for (int pass = 0; pass < 4; ++pass) {
            const SortPass p = sort_pass(b, score, order1, order0, cls, pass);
            hipLaunchKernelGGL(seg_sort_hist_kernel, dim3((unsigned)tiles), dim3(SAP_THREADS), 0, st, p, N, tiles, b.hist);
            EGX_LAUNCH_CHECK();
            hipLaunchKernelGGL(seg_sort_scan_kernel, dim3(256), dim3(SAP_THREADS), 0, st, b.hist, tiles, b.excl, b.dtot);
            EGX_LAUNCH_CHECK();
            hipLaunchKernelGGL(seg_sort_scatter_kernel, dim3((unsigned)tiles), dim3(SAP_THREADS), 0, st, p, N, tiles, b.excl, b.dtot);
            EGX_LAUNCH_CHECK();
        }
    for (int stage = 0; stage < 3; ++stage) {
        hipLaunchKernelGGL(seg_ap_tile_kernel, dim3((unsigned)tiles, 2), dim3(SAP_THREADS), 0, st, b, N, stage, res);
        EGX_LAUNCH_CHECK();
        if (stage < 2) {
            hipLaunchKernelGGL(seg_ap_scan_kernel, dim3(2), dim3(SAP_THREADS), 0, st, b, tiles, stage);
            EGX_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(seg_ap_final_kernel, dim3(1), dim3(SAP_THREADS), 0, st, b, N, tiles, res);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
