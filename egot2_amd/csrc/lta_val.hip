// The validation step of the long-term-anticipation task in one launch: HOI/tasks/lta/long_term_anticipation.py:222-248 (and :313-341),
//   preds = model.generate(input, k = K)          K sequences of Z tokens per clip and head: Categorical(logits).sample() K times, argmax at K = 1
//   AUED(pred.permute(0, 2, 1).cpu(), labels)     evaluation/lta/lta_metrics.py:86-114: for every prefix length, the edit distance of the
//                                                 closest of the K sequences, a Python loop of editdistance.eval
// on the (B, Z, ld) stack of the MultiTaskHead's outputs, whose heads are column windows [col0[h], col0[h] + C[h]) of a row.
//
//   grid    : a workgroup of 4 waves per (head h, clip b). Wave w draws the rows of future steps w, w + 4, ... (a row is two dependent trips
//             to memory, so the rows of a clip are spread over waves instead of queued in one); the K x Z tokens stay in LDS; then wave w
//             runs the edit-distance tables of sequences w, w + 4, ...
//   draws   : pass 1 over the window (lane-strided): max, NaN flag, argmax (lowest index among equals). Pass 2 (the lines are in cache):
//             lane L owns the CONTIGUOUS chunk [L * CH, (L + 1) * CH), CH = ceil(C / 64) <= 32, and writes the running sum of
//             exp(x - max) over its chunk to LDS; the 64 chunk totals are added in lane order by every lane alike (64 v_readlane + add, the
//             same bits in every lane), which gives each lane its base. cdf[i] = base[lane(i)] + running[i]: a chain of at most 32 + 64
//             additions instead of 2048, and - unlike a tree scan - EXACTLY non-decreasing and exactly flat across classes of probability 0
//             (the last value of chunk L and base[L + 1] are the same sum). Lane k < K then finds #{i : cdf[i] <= u_k * S} by bisection
//             (S = cdf[C - 1], the product in fp64), clamped to the last class of non-zero probability (u * S can round to S).
//   key     : site_key(seed, LTA_VAL_KEY_LAYER = 0x17A, site = h); u_k of row r = b * Z + z is word k of that row: rand_quad(key, r, k >> 1),
//             .x for even k, .y for odd k; u = (w + 0.5) / 2^32. (tests/lta_val_ref.py restates it.)
//   tables  : all Z prefix distances of one sequence are the diagonal of ONE (Z + 1) x (Z + 1) Levenshtein table. Lane j owns column j + 1 and
//             the table is swept along anti-diagonals (2 Z - 1 steps, one lane shift each); the min over a wave's sequences stays in the
//             lane's register, the min over the waves goes through LDS. Lane z of wave 0 ends up with min_dist[b, z, h].
//   sums    : wave 0 adds its Z values to dist_sum with 64-bit integer vector atomics (zeroed by a memset node in front of the launch).
//             Integers only: the same bits on every run.
#include "common.h"
#include "kernels.h"

namespace egx {

constexpr int LV_WAVES = 4;
constexpr uint32_t LTA_VAL_KEY_LAYER = 0x17A;

struct LtaValParams {
    const float* logits; const int64_t* labels; const int64_t* preds_in; const uint64_t* seed_ptr; uint64_t seed;
    int B, Z, K, H, ld;
    int col0[SEG_CE_MAX_HEADS], C[SEG_CE_MAX_HEADS];
    int64_t* preds; int* min_dist; unsigned long long* dist_sum;
};

// The K tokens of one row (b, z) of head h into tok[k * LTA_VAL_MAX_Z + z] (lanes k < K write them); -1 for a row that cannot be sampled
__device__ __forceinline__ void lv_draw_row(const float* __restrict__ seg, int C, int K, uint64_t key, uint32_t row, float* __restrict__ cdf,
                                            int64_t* __restrict__ tok_z, int64_t* __restrict__ preds_z, int Z, int lane) {
    // pass 1: max and its lowest index, NaN flag
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    bool nan = false;
    for (int c = lane; c < C; c += 64) {
        const float x = seg[c];
        nan |= x != x;
        if (x > bv) { bv = x; bi = c; }        // strict: the lowest index of the lane's elements stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    // a row with a NaN or +inf, or without a finite logit, has no distribution: token -1 for every draw (the reference raises)
    const bool valid = __ballot(nan) == 0ull && bv > -INFINITY && bv < INFINITY;
    int token = -1;
    if (K == 1) {
        token = valid ? bi : -1;
    } else if (valid) {
        const int CH = (C + 63) >> 6;
        const int i0 = lane * CH, i1 = min(C, i0 + CH);
        float run = 0.f;
        int lastpos = -1;
        for (int i = i0; i < i1; ++i) {
            const float e = expf(seg[i] - bv);      // max-subtracted: the largest term is 1, exp(-inf) = 0
            run += e;
            cdf[i] = run;
            lastpos = e > 0.f ? i : lastpos;
        }
        float base = 0.f, acc = 0.f;
#pragma unroll
        for (int l = 0; l < 64; ++l) {              // the chunk totals in lane order, the same chain in every lane
            const float t = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(run), l));
            base = lane == l ? acc : base;
            acc += t;
        }
        lastpos = wave_max(lastpos);
        for (int i = i0; i < i1; ++i) cdf[i] += base;
        __builtin_amdgcn_wave_barrier();
        if (lane < K) {
            const uint2 q = rand_quad(key, row, (uint32_t)lane >> 1);
            const uint32_t w = (lane & 1) ? q.y : q.x;
            const double t = ((double)w + 0.5) * (1.0 / 4294967296.0) * (double)acc;
            int lo = 0, hi = C;
            while (lo < hi) {                       // first i with cdf[i] > t
                const int mid = (lo + hi) >> 1;
                if ((double)cdf[mid] <= t) lo = mid + 1; else hi = mid;
            }
            token = min(lo, lastpos);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < K) {
        tok_z[lane * LTA_VAL_MAX_Z] = token;
        preds_z[(size_t)lane * Z] = token;
    }
}

__global__ __launch_bounds__(256) void lta_validate_kernel(LtaValParams p) {
    __shared__ float cdf_s[LV_WAVES][SEG_CE_MAX_CLASSES];
    __shared__ int64_t tok_s[LTA_VAL_MAX_K * LTA_VAL_MAX_Z];
    __shared__ int dist_s[LV_WAVES][LTA_VAL_MAX_Z];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x / p.B, b = blockIdx.x % p.B;
    const int Z = p.Z, K = p.K;
    const size_t seq0 = (size_t)blockIdx.x * K * Z;             // preds[h, b, 0, 0]
    if (p.preds_in) {
        for (int i = tid; i < K * Z; i += 256) {
            const int64_t t = p.preds_in[seq0 + i];
            tok_s[(i / Z) * LTA_VAL_MAX_Z + i % Z] = t;
            if (p.preds) p.preds[seq0 + i] = t;
        }
    } else {
        int c0 = 0, C = 0;
#pragma unroll
        for (int g = 0; g < SEG_CE_MAX_HEADS; ++g)
            if (g == h) { c0 = p.col0[g]; C = p.C[g]; }
        const uint64_t key = site_key(p.seed_ptr ? *p.seed_ptr : p.seed, LTA_VAL_KEY_LAYER, (uint32_t)h);
        for (int z = wave; z < Z; z += LV_WAVES) {              // wave w: future steps w, w + 4, ...
            const size_t row = (size_t)b * Z + z;
            lv_draw_row(p.logits + row * p.ld + c0, C, K, key, (uint32_t)row, cdf_s[wave], tok_s + z, p.preds + seq0 + z, Z, lane);
        }
    }
    if (!p.labels) return;                      // the same in every thread
    __syncthreads();
    // wave w runs the tables of sequences w, w + 4, ...
    int best = 0x7fffffff;
    const int64_t lab = lane < Z ? p.labels[((size_t)b * Z + lane) * p.H + h] : 0;
    for (int k = wave; k < K; k += LV_WAVES) {
        // cell (i, j) = D[i + 1][j + 1] is computed by lane j at step s = i + j. cur: the lane's cell of the step before, D[i][j + 1]
        // (before its first step D[0][j + 1] = j + 1); l1: the left lane's, D[i + 1][j]; l2: the left lane's of two steps before, D[i][j]
        const int64_t* tk = tok_s + k * LTA_VAL_MAX_Z;
        int cur = lane + 1, l2 = 0;
        for (int s = 0; s < 2 * Z - 1; ++s) {
            int l1 = __shfl_up(cur, 1, 64);
            l1 = lane == 0 ? s + 1 : l1;            // D[i + 1][0] = i + 1
            const int i = s - lane;
            const bool on = i >= 0 && i < Z && lane < Z;
            const int64_t t = tk[on ? i : 0];
            const int cost = (t == lab && t >= 0) ? 0 : 1;      // a negative token (a row that could not be sampled) equals no label
            const int nv = min(min(cur, l1) + 1, l2 + cost);
            l2 = l1;
            if (on) {
                cur = nv;
                best = i == lane ? min(best, nv) : best;
            }
        }
    }
    dist_s[wave][lane] = best;
    __syncthreads();
    if (wave == 0 && lane < Z) {
        const int m = min(min(dist_s[0][lane], dist_s[1][lane]), min(dist_s[2][lane], dist_s[3][lane]));
        if (p.min_dist) p.min_dist[((size_t)b * Z + lane) * p.H + h] = m;
        if (p.dist_sum) atomicAdd(p.dist_sum + (size_t)lane * p.H + h, (unsigned long long)m);
    }
}

int lta_validate(const float* logits, int ld, const int64_t* labels, int B, int Z, int H, const int* col0, const int* C, int K, uint64_t seed,
                 const uint64_t* seed_ptr, const int64_t* preds_in, int64_t* preds, int* min_dist, int64_t* dist_sum, hipStream_t st) {
    EGX_CHECK(logits || preds_in, "lta_validate: null pointer argument (logits and preds_in are both NULL: nothing to sample from, nothing to score)");
    EGX_CHECK(preds || preds_in, "lta_validate: null pointer argument (preds)");
    EGX_CHECK(B >= 1, "lta_validate: B=%d (needs B >= 1)", B);
    EGX_CHECK(Z >= 1 && Z <= LTA_VAL_MAX_Z, "lta_validate: Z=%d (needs 1 <= Z <= %d future steps)", Z, LTA_VAL_MAX_Z);
    EGX_CHECK((long long)B * Z <= (long long)SEG_CE_MAX_ROWS, "lta_validate: B * Z = %lld rows (needs B * Z <= %d)", (long long)B * Z, SEG_CE_MAX_ROWS);
    EGX_CHECK(K >= 1 && K <= LTA_VAL_MAX_K, "lta_validate: K=%d (needs 1 <= K <= %d sequences per clip)", K, LTA_VAL_MAX_K);
    EGX_CHECK(H >= 1 && H <= SEG_CE_MAX_HEADS, "lta_validate: H=%d (needs 1 <= H <= %d heads)", H, SEG_CE_MAX_HEADS);
    EGX_CHECK(labels || (!min_dist && !dist_sum), "lta_validate: null pointer argument (labels, with min_dist or dist_sum asked for)");
    EGX_CHECK(!preds_in || labels, "lta_validate: null pointer argument (labels: preds_in is the metric-only entry)");
    if (!preds_in) {
        EGX_CHECK(col0 && C, "lta_validate: null pointer argument (col0 / C)");
        EGX_CHECK(ld >= 1, "lta_validate: ld=%d (needs ld >= 1)", ld);
        if (check_head_windows("lta_validate", ld, H, col0, C)) return 1;
        // A HOST seed is baked into a captured graph: every replay would draw the SAME sequences (the rule of the dropout seed, encoder.hip)
        if (K > 1 && !seed_ptr) {
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
            EGX_CHECK(cs == hipStreamCaptureStatusNone, "lta_validate: K=%d draws with a host seed cannot be captured in a hipGraph: every replay would "
                      "repeat the same sequences; pass seed_ptr (train.LTAValidation owns one), use K = 1, or launch eagerly", K);
        }
    }
    LtaValParams p;
    p.logits = logits; p.labels = labels; p.preds_in = preds_in; p.seed_ptr = preds_in ? nullptr : seed_ptr; p.seed = seed;
    p.B = B; p.Z = Z; p.K = K; p.H = H; p.ld = ld;
    for (int h = 0; h < SEG_CE_MAX_HEADS; ++h) { p.col0[h] = (h < H && !preds_in) ? col0[h] : 0; p.C[h] = (h < H && !preds_in) ? C[h] : 0; }
    p.preds = preds; p.min_dist = min_dist; p.dist_sum = (unsigned long long*)dist_sum;
    if (dist_sum) EGX_HIP(hipMemsetAsync(dist_sum, 0, (size_t)Z * H * sizeof(int64_t), st));
    hipLaunchKernelGGL(lta_validate_kernel, dim3((unsigned)H * (unsigned)B), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
