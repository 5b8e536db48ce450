// The criterion and the metrics of an EgoT2-g multi-task step in one launch: Unified3TaskTranslation
// (HHI/tasks/multitask/video_tasktranslation.py:39-66, accuracy :101-102) and Unified6TaskTranslation (HOI/tasks/multitask/video_task.py:537-577,
// validation :683-736),
//   loss = sum over tasks t of ratio_t * nn.CrossEntropyLoss()(logits_t (B, |V|, sy), target_t[:, 1:])     (3 or 6 terms, each read with .item())
//   ARMetric / LTAMetric (HOI/evaluation/lta/lta_metrics.py:164-211, 229-292), PNRMetric / OSCCMetric (HOI/evaluation/pnr/metrics.py:139-257):
//   the argmax of a position's logits mapped from its vocabulary word to the task's original label, in Python loops with .item() per clip
// on the decoder's (sy, B, |V|) output, read in place through the (B, |V|, sy) view the models return (the class axis is contiguous).
//
//   grid    : a workgroup per (task, chunk of target rows b); 4 waves, a wave per row b walking its sy positions, so whether a whole row is
//             right (seq_correct) needs no exchange. Every workgroup of task t first counts the valid labels of ITS task over all B * sy
//             positions (the normaliser depends on the labels only), so d loss / d logits of its rows is final in the same pass.
//   row     : the row routine of seg_ce.hip. V <= 512: lane-strided dword loads (rows have no alignment), the row stays in up to 8 registers
//             per lane; wave butterflies for max, exp-sum and the two argmaxes; the gradient is written from the registers, so every logit is
//             read once. V > 512: a per-lane online max / exp-sum pass, then one re-read (from L2) that writes the gradient.
//   metrics : word_label (vocabulary word -> original label, -1: none) is staged in LDS once per workgroup; the free argmax a and the argmax r
//             over the mapped words share the row pass.
//   sums    : per-workgroup partials go to scratch; the last workgroup to arrive sums the chunks of every task in a fixed order, divides by
//             n_valid and adds ratio_t * term_t for t = 0, 1, ...: the same bits on every run, no float atomics. The arrival counters leave
//             themselves zero, and counters and partials are laid out for 8 tasks always, so launches of every T share one scratch buffer.
#include <string.h>
#include "common.h"
#include "kernels.h"

namespace egx {

constexpr int SEQ_WAVES = 4;
constexpr int SEQ_MAX_CHUNKS = 256;         // chunks of rows per task: bounds the label count every workgroup repeats
constexpr int SEQ_COUNTER_WORDS = 16;       // an arrival counter per 64 bytes: [launch][task 0] ... [task 7]
constexpr int SEQ_PART_WORDS = 8;           // a workgroup's partial: nll sum, n_valid, token_correct, seq_correct, scored, invalid, correct, correct_restricted
constexpr int SEQ_NONE = 1 << 30;           // index of "no word": it loses every tie

struct SeqTaskDev {
    const float* logits; const int64_t* target; float* dlogits; const int* word_label; const int64_t* labels; int* pred;
    long long sb, ss, tsb, tss, lsb, lss;
    int B, sy, chunk, nchunks, blk0;
    float ratio;
};

struct SeqCeParams {
    SeqTaskDev task[SEQ_CE_MAX_TASKS];
    int T, V;
    int* result;            // [loss][loss_terms T][n_valid T][token_correct T][seq_correct T][scored T][invalid T][correct T][correct_restricted T]
    unsigned* counter;      // arrival counters, zero before the first launch
    int* part;              // [SEQ_CE_MAX_TASKS][SEQ_MAX_CHUNKS][SEQ_PART_WORDS]
};

struct SeqOut { float nll; int a, r; };

// V <= 64 * NR: word c = lane + 64 j lives in register j. y < 0: the position has no valid label (no nll; zeros for the gradient).
template <int NR>
__device__ __forceinline__ SeqOut seq_regs(const float* __restrict__ row, float* __restrict__ drow, int V, int y, float scale,
                                           const int* __restrict__ wl, int lane) {
    float v[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) v[j] = lane + 64 * j < V ? row[lane + 64 * j] : -INFINITY;
    float m = v[0], zy = -INFINITY, bv = -INFINITY, rv = -INFINITY;
    int bi = SEQ_NONE, ri = SEQ_NONE;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int c = lane + 64 * j;
        const bool in = c < V;
        m = fmaxf(m, v[j]);
        zy = c == y ? v[j] : zy;
        if (in && argmax_better(v[j], c, bv, bi)) { bv = v[j]; bi = c; }
        if (wl && in && wl[c] >= 0 && argmax_better(v[j], c, rv, ri)) { rv = v[j]; ri = c; }
    }
    SeqOut o;
    o.a = wave_argmax(bv, bi).i;
    o.r = wl ? wave_argmax(rv, ri).i : SEQ_NONE;
    o.nll = 0.f;
    if (y >= 0) {
        m = wave_max(m);
        zy = __shfl(zy, y & 63, 64);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            v[j] = lane + 64 * j < V ? expf(v[j] - m) : 0.f;        // max-subtracted: the largest term is 1
            s += v[j];
        }
        s = wave_sum(s);
        o.nll = (m - zy) + logf(s);
        if (drow) {
            const float rs = 1.f / s;
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int c = lane + 64 * j;
                if (c < V) drow[c] = scale != 0.f ? (v[j] * rs - (c == y ? 1.f : 0.f)) * scale : 0.f;
            }
        }
    } else if (drow) {
#pragma unroll
        for (int j = 0; j < NR; ++j)
            if (lane + 64 * j < V) drow[lane + 64 * j] = 0.f;
    }
    return o;
}

// V > 512: per-lane online max / exp-sum over the lane's words, combined across the wave; the gradient pass reads the row again
__device__ __forceinline__ SeqOut seq_loop(const float* __restrict__ row, float* __restrict__ drow, int V, int y, float scale,
                                           const int* __restrict__ wl, int lane) {
    float ml = row[lane], sl = 1.f;             // V > 512: every lane owns a word
    float bv = ml, rv = -INFINITY;
    int bi = lane, ri = SEQ_NONE;
    if (wl && wl[lane] >= 0) { rv = ml; ri = lane; }
#pragma unroll 4
    for (int c = lane + 64; c < V; c += 64) {
        const float x = row[c];
        if (argmax_better(x, c, bv, bi)) { bv = x; bi = c; }
        if (wl && wl[c] >= 0 && argmax_better(x, c, rv, ri)) { rv = x; ri = c; }
        if (x > ml) { sl = sl * expf(ml - x) + 1.f; ml = x; }
        else sl += expf(x - ml);
    }
    SeqOut o;
    o.a = wave_argmax(bv, bi).i;
    o.r = wl ? wave_argmax(rv, ri).i : SEQ_NONE;
    o.nll = 0.f;
    if (y >= 0) {
        const float zy = row[y];
        const float m = wave_max(ml);
        const float s = wave_sum(sl * expf(ml - m));
        o.nll = (m - zy) + logf(s);
        if (drow) {
            const float rs = 1.f / s;
            if (scale != 0.f) {
#pragma unroll 4
                for (int c = lane; c < V; c += 64) drow[c] = (expf(row[c] - m) * rs - (c == y ? 1.f : 0.f)) * scale;
            } else {
                for (int c = lane; c < V; c += 64) drow[c] = 0.f;
            }
        }
    } else if (drow) {
        for (int c = lane; c < V; c += 64) drow[c] = 0.f;
    }
    return o;
}

__global__ __launch_bounds__(256) void sequence_ce_kernel(SeqCeParams p) {
    __shared__ int wl_s[SEQ_CE_MAX_CLASSES];            // word -> original label of this workgroup's task
    __shared__ int cnt_s[SEQ_WAVES];
    __shared__ float nll_s[SEQ_WAVES];
    __shared__ int acc_s[SEQ_WAVES][6];
    __shared__ float term_s[SEQ_CE_MAX_TASKS];
    __shared__ float scale_s;
    __shared__ bool last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t = 0;
#pragma unroll
    for (int u = 1; u < SEQ_CE_MAX_TASKS; ++u) t = (u < p.T && (int)blockIdx.x >= p.task[u].blk0) ? u : t;
    const SeqTaskDev& k = p.task[t];
    const int chunk_id = (int)blockIdx.x - k.blk0;
    const int V = p.V, sy = k.sy;
    const bool has_wl = k.word_label != nullptr;
    if (has_wl)
        for (int c = tid; c < V; c += 256) wl_s[c] = k.word_label[c];

    // n_valid[t] over ALL rows and positions of the task: every workgroup of this task counts it itself
    int cnt = 0;
    const int n_pos = k.B * sy;             // <= 2^22, checked on the host
    for (int i = tid; i < n_pos; i += 256) {
        const int b = i / sy, s = i - b * sy;
        const int64_t y = k.target[b * k.tsb + s * k.tss];
        cnt += (y >= 0 && y < V) ? 1 : 0;
    }
    cnt = wave_sum(cnt);
    if (lane == 0) cnt_s[wave] = cnt;
    __syncthreads();                        // also: wl_s is staged
    if (tid == 0) {
        const int n = (cnt_s[0] + cnt_s[1]) + (cnt_s[2] + cnt_s[3]);
        scale_s = n > 0 ? k.ratio / (float)n : 0.f;
    }
    __syncthreads();
    const float scale = scale_s;
    const int* wl = has_wl ? wl_s : nullptr;

    // the wave's sums: the results of the butterflies are the same in every lane, so every lane carries them; added in row order
    float nll_acc = 0.f;
    int n_tok = 0, n_seq = 0, n_scored = 0, n_invalid = 0, n_correct = 0, n_restricted = 0;
    const int b_end = min(k.B, (chunk_id + 1) * k.chunk);
    for (int b = chunk_id * k.chunk + wave; b < b_end; b += SEQ_WAVES) {      // wave w: rows w, w + 4, ... of the chunk, in this order
        int row_valid = 0, row_right = 0;
#pragma unroll 1
        for (int s = 0; s < sy; ++s) {
            const int64_t y64 = k.target[b * k.tsb + s * k.tss];
            // ignore_index (-100) / out-of-range label: no loss, no count, no gradient. The label is the same in every lane.
            const int y = __builtin_amdgcn_readfirstlane((y64 < 0 || y64 >= V) ? -1 : (int)y64);
            const float* row = k.logits + (b * k.sb + s * k.ss);
            float* drow = k.dlogits ? k.dlogits + (b * k.sb + s * k.ss) : nullptr;
            if (y < 0 && !has_wl) {         // nothing to compute: the gradient row is zero
                if (drow)
                    for (int c = lane; c < V; c += 64) drow[c] = 0.f;
                continue;
            }
            SeqOut o;
            if (V <= 64) o = seq_regs<1>(row, drow, V, y, scale, wl, lane);
            else if (V <= 128) o = seq_regs<2>(row, drow, V, y, scale, wl, lane);
            else if (V <= 256) o = seq_regs<4>(row, drow, V, y, scale, wl, lane);
            else if (V <= 512) o = seq_regs<8>(row, drow, V, y, scale, wl, lane);
            else o = seq_loop(row, drow, V, y, scale, wl, lane);
            if (y >= 0) {
                nll_acc += o.nll;
                row_valid += 1;
                row_right += o.a == y ? 1 : 0;
            }
            if (has_wl) {
                const int la = wl_s[o.a];                           // o.a is a word of the row: V >= 1
                const int lr = o.r != SEQ_NONE ? wl_s[o.r] : -1;    // no mapped word at all: no label
                if (k.pred && lane == 0) {
                    int* pr = k.pred + ((size_t)b * sy + s) * 2;
                    pr[0] = la;
                    pr[1] = lr;
                }
                if (k.labels) {
                    const int64_t lab = k.labels[b * k.lsb + s * k.lss];
                    if (lab >= 0) {         // a label < 0: the position is not scored
                        n_scored += 1;
                        n_invalid += la < 0 ? 1 : 0;
                        n_correct += (int64_t)la == lab ? 1 : 0;
                        n_restricted += (int64_t)lr == lab ? 1 : 0;
                    }
                }
            }
        }
        n_tok += row_right;
        n_seq += (row_valid > 0 && row_right == row_valid) ? 1 : 0;
    }
    if (lane == 0) {
        nll_s[wave] = nll_acc;
        acc_s[wave][0] = n_tok; acc_s[wave][1] = n_seq; acc_s[wave][2] = n_scored;
        acc_s[wave][3] = n_invalid; acc_s[wave][4] = n_correct; acc_s[wave][5] = n_restricted;
    }
    __syncthreads();
    // Workgroup partials -> scratch, the last workgroup to arrive sums them. The hand-off of segmented_ce_kernel (wave 0 stores and signals):
    // every handed-off word is stored write-through at agent scope, the wave drains its stores, then ONE relaxed agent-scope add draws the
    // ticket; the reader loads every such word at agent scope (past its CU's L1). No release fence, so no L2 write-back per workgroup.
    if (wave == 0) {
        int* mine = p.part + ((size_t)t * SEQ_MAX_CHUNKS + chunk_id) * SEQ_PART_WORDS;
        if (lane == 0)
            __hip_atomic_store((float*)mine, (nll_s[0] + nll_s[1]) + (nll_s[2] + nll_s[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 1)
            __hip_atomic_store(mine + 1, (cnt_s[0] + cnt_s[1]) + (cnt_s[2] + cnt_s[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane >= 2 && lane < SEQ_PART_WORDS) {
            const int j = lane - 2;
            __hip_atomic_store(mine + lane, (acc_s[0][j] + acc_s[1][j]) + (acc_s[2][j] + acc_s[3][j]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            // two levels of arrival counters (adds to ONE word are served one after the other): the chunks of a task count on that task's
            // word and only its last chunk goes on to the launch's
            bool t_last = true;
            if (k.nchunks > 1) {
                unsigned* tc = p.counter + SEQ_COUNTER_WORDS * (1 + t);
                t_last = __hip_atomic_fetch_add(tc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)k.nchunks - 1;
                if (t_last) __hip_atomic_store(tc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);        // left zero for the next launch
            }
            last_s = t_last && __hip_atomic_fetch_add(p.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)p.T - 1;
        }
    }
    __syncthreads();
    if (!last_s) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // a wave per task (tasks w, w + 4): lane j adds chunks j, j + 64, ... in this order, a butterfly adds the lanes: the same order on every run
    for (int u = wave; u < p.T; u += SEQ_WAVES) {
        const int nch = p.task[u].nchunks;
        const int* base = p.part + (size_t)u * SEQ_MAX_CHUNKS * SEQ_PART_WORDS;
        float f = 0.f;
        int iv[6] = {0, 0, 0, 0, 0, 0};
        for (int j = lane; j < nch; j += 64) {
            const int* q = base + (size_t)j * SEQ_PART_WORDS;
            f += __hip_atomic_load((const float*)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int w = 0; w < 6; ++w) iv[w] += __hip_atomic_load(q + 2 + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const int n = __hip_atomic_load(base + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // chunk 0's count: every chunk holds the same
        f = wave_sum(f);
#pragma unroll
        for (int w = 0; w < 6; ++w) iv[w] = wave_sum(iv[w]);
        if (lane == 0) {
            const float term = n > 0 ? f / (float)n : 0.f;          // a task without a valid label adds nothing
            term_s[u] = term;
            ((float*)p.result)[1 + u] = term;
            p.result[1 + p.T + u] = n;
#pragma unroll
            for (int w = 0; w < 6; ++w) p.result[1 + (2 + w) * p.T + u] = iv[w];
        }
    }
    __syncthreads();
    if (tid == 0) {
        float loss = 0.f;
        for (int u = 0; u < p.T; ++u) loss += p.task[u].ratio * term_s[u];
        ((float*)p.result)[0] = loss;
        *p.counter = 0u;            // left zero for the next launch
    }
}

size_t sequence_ce_scratch_bytes() {
    // [arrival counters: 64 B each, the launch's and one per task][partials]: the same layout for every T and every shape
    return (size_t)(1 + SEQ_CE_MAX_TASKS) * SEQ_COUNTER_WORDS * sizeof(unsigned) +
           (size_t)SEQ_CE_MAX_TASKS * SEQ_MAX_CHUNKS * SEQ_PART_WORDS * sizeof(int);
}

int sequence_ce(const SeqCeTask* tasks, int T, int V, int* result, void* scratch, hipStream_t st) {
    EGX_CHECK(tasks && result && scratch, "sequence_ce: null pointer argument (tasks, result and scratch are required)");
    EGX_CHECK(T >= 1 && T <= SEQ_CE_MAX_TASKS, "sequence_ce: T=%d (needs 1 <= T <= %d tasks)", T, SEQ_CE_MAX_TASKS);
    EGX_CHECK(V >= 2 && V <= SEQ_CE_MAX_CLASSES, "sequence_ce: V=%d (needs 2 <= V <= %d words)", V, SEQ_CE_MAX_CLASSES);
    SeqCeParams p;
    memset(&p, 0, sizeof(p));
    int blocks = 0;
    for (int t = 0; t < T; ++t) {
        const SeqCeTask& a = tasks[t];
        EGX_CHECK(a.logits && a.target, "sequence_ce: null pointer argument (logits / target of task %d)", t);
        EGX_CHECK(a.B >= 1, "sequence_ce: task %d has B=%d (needs B >= 1)", t, a.B);
        EGX_CHECK(a.sy >= 1 && a.sy <= SEQ_CE_MAX_SY, "sequence_ce: task %d has sy=%d (needs 1 <= sy <= %d positions)", t, a.sy, SEQ_CE_MAX_SY);
        EGX_CHECK((long long)a.B * a.sy <= (long long)SEQ_CE_MAX_ROWS, "sequence_ce: task %d has B * sy = %lld rows (needs B * sy <= %d)", t,
                  (long long)a.B * a.sy, SEQ_CE_MAX_ROWS);
        EGX_CHECK(!a.labels || a.word_label, "sequence_ce: task %d has labels without word_label", t);
        EGX_CHECK(!a.word_label || a.labels, "sequence_ce: task %d has word_label without labels", t);
        EGX_CHECK(!a.pred || a.word_label, "sequence_ce: task %d has pred without word_label", t);
        EGX_CHECK(a.stride_b >= 0 && a.stride_s >= 0 && a.target_stride_b >= 0 && a.target_stride_s >= 0 && a.labels_stride_b >= 0 &&
                      a.labels_stride_s >= 0, "sequence_ce: task %d has a negative stride", t);
        EGX_CHECK(!a.d_logits || ((a.B == 1 || a.stride_b >= V) && (a.sy == 1 || a.stride_s >= V)),
                  "sequence_ce: task %d has d_logits with overlapping rows (strides %lld, %lld need to be >= V = %d)", t, a.stride_b, a.stride_s, V);
        SeqTaskDev& k = p.task[t];
        k.logits = a.logits; k.target = a.target; k.dlogits = a.d_logits; k.word_label = a.word_label; k.labels = a.labels; k.pred = a.pred;
        k.sb = a.stride_b; k.ss = a.stride_s; k.tsb = a.target_stride_b; k.tss = a.target_stride_s;
        k.lsb = a.labels_stride_b; k.lss = a.labels_stride_s;
        k.B = a.B; k.sy = a.sy; k.ratio = a.ratio;
        batch_chunks(a.B, SEQ_MAX_CHUNKS, SEQ_WAVES, &k.chunk, &k.nchunks);
        k.blk0 = blocks;
        blocks += k.nchunks;
    }
    p.T = T; p.V = V; p.result = result;
    p.counter = (unsigned*)scratch;
    p.part = (int*)((char*)scratch + (size_t)(1 + SEQ_CE_MAX_TASKS) * SEQ_COUNTER_WORDS * sizeof(unsigned));
    hipLaunchKernelGGL(sequence_ce_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
