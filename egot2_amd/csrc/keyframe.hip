// The criterion and the metrics of the PNR keyframe task in one launch: KeyframeLocalisation2Loader.training_step,
// HOI/tasks/pnr/video_taskspecific_pnr.py:24-63 (and keyframe_detection.py:23-70),
//   loss = BCELoss(mean)(sigmoid(preds.squeeze(1)), labels.float())          or  mean(state_change_label.T * CE(preds, argmax(labels)))
//   keyframe_distance / keyframe_accuracy (HOI/evaluation/pnr/metrics.py:23-80): two Python loops with four to six .item() reads per clip
// and, on decoder logits, PnrOsccMetric.pnr_distance / oscc_acc (metrics.py:102-134): the argmax restricted to the vocabulary columns `cols`.
//
//   grid    : a workgroup per chunk of clips; 4 waves, a wave per clip row, a lane per frame (T <= 64). The frame's column is cols[t] (a
//             kernel argument) or t. The V-column scan for the unrestricted argmax (cols only) is a lane-strided loop.
//   row     : wave butterflies for argmax (torch.argmax: the first NaN, else the lowest index among equal maxima), max and the sums; the
//             gradient row is written in whole (every column of ld, zeros outside the frames) from the lanes' registers. The fp64 distance
//             of a clip is plain C++ in lane 0.
//   sums    : per-workgroup partials (loss, distance, three counts) go to scratch; the last workgroup to arrive adds the chunks by a fixed
//             butterfly: the same bits on every run, no float atomics. The arrival counter leaves itself zero.
#include "common.h"
#include "kernels.h"

namespace egx {

constexpr int KF_WAVES = 4;
constexpr int KF_MAX_CHUNKS = 64;           // chunks of clips: lane j of the last workgroup holds chunk j
constexpr int KF_COUNTER_BYTES = 64;

struct KeyframeParams {
    const float* logits; const float* target; const int64_t* label; const int64_t* state_change;
    const double* fps; const int64_t* clip_start; const int64_t* clip_end; const int64_t* pnr_frame;
    int B, T, V, ld, kind, has_cols, chunk, nchunks;
    int cols[KEYFRAME_MAX_T];
    float* loss; float* loss_rows; float* dlogits; int* pred; int* label_frame; int* counts; double* dist; double* dist_sum;
    unsigned* counter;      // arrival counter, zero before the first launch
    double* dpart;          // [KF_MAX_CHUNKS]      sum of the chunk's distances
    float* fpart;           // [KF_MAX_CHUNKS]      sum of the chunk's loss rows
    int* ipart;             // [KF_MAX_CHUNKS][3]   n_sc, n_correct, n_outside of the chunk
};

constexpr int KF_NO_FRAME = 1 << 30;        // index of a lane without a frame: it loses every tie

__global__ __launch_bounds__(256) void keyframe_criterion_kernel(KeyframeParams p) {
    __shared__ short frame_of_s[KEYFRAME_MAX_V];       // column -> frame, -1 for a column that is no frame (cols only)
    __shared__ int cols_s[KEYFRAME_MAX_T];             // indexed by a run-time frame below
    __shared__ float loss_s[KF_WAVES];
    __shared__ double dist_s[KF_WAVES];
    __shared__ int cnt_s[KF_WAVES][3];
    __shared__ bool last_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T;
    const bool is_frame = lane < T;
    if (p.has_cols) {
        if (tid == 0) {
#pragma unroll
            for (int t = 0; t < KEYFRAME_MAX_T; ++t) cols_s[t] = p.cols[t];
        }
        for (int c = tid; c < p.V; c += 256) frame_of_s[c] = -1;
        __syncthreads();
        if (tid < T) frame_of_s[cols_s[tid]] = (short)tid;
        __syncthreads();
    }
    const int col = is_frame ? (p.has_cols ? cols_s[lane] : lane) : 0;         // in [0, V): checked on the host

    float loss_acc = 0.f;           // the wave's rows, added in row order (the same value in every lane)
    double dist_acc = 0.0;
    int n_sc = 0, n_correct = 0, n_outside = 0;
    const int b_end = min(p.B, (blockIdx.x + 1) * p.chunk);
    for (int b = blockIdx.x * p.chunk + wave; b < b_end; b += KF_WAVES) {
        const float* row = p.logits + (size_t)b * p.ld;
        const float x = is_frame ? row[col] : -INFINITY;
        const WaveBest best = wave_argmax(x, is_frame ? lane : KF_NO_FRAME);
        const int pred = best.i;

        int lab = -1;               // the label frame; -1: none given
        if (p.label) {
            const int64_t l = p.label[b];
            lab = (l >= 0 && l < T) ? (int)l : -2;          // outside [0, T): equals no prediction, and adds no CE loss or gradient
        } else if (p.target) {
            lab = wave_argmax(is_frame ? p.target[(size_t)b * T + lane] : -INFINITY, is_frame ? lane : KF_NO_FRAME).i;
        }
        const bool sc = p.state_change ? p.state_change[b] == 1 : true;

        if (p.has_cols) {           // the argmax over all V columns: is it one of the frames?
            float gv = -INFINITY;
            int gi = KF_NO_FRAME;
            for (int c = lane; c < p.V; c += 64) {
                const float v = row[c];
                if (argmax_better(v, c, gv, gi)) { gv = v; gi = c; }
            }
            const WaveBest g = wave_argmax(gv, gi);
            n_outside += frame_of_s[g.i] < 0 ? 1 : 0;
        }
        n_sc += sc ? 1 : 0;
        n_correct += (sc && lab >= 0 && pred == lab) ? 1 : 0;

        float row_loss = 0.f, g = 0.f;
        if (p.kind == KEYFRAME_BCE) {
            // logit form: softplus(x) = max(x, 0) + log1p(exp(-|x|)), softplus(-x) likewise; sigmoid(x) from the same exp(-|x|)
            const float y = is_frame ? p.target[(size_t)b * T + lane] : 0.f;
            const float e = expf(-fabsf(x));            // a lane without a frame: exp(-inf) = 0
            const float l1p = log1pf(e);
            const float sp_pos = fmaxf(x, 0.f) + l1p, sp_neg = fmaxf(-x, 0.f) + l1p;
            const float term = is_frame ? fminf(sp_neg, 100.f) * y + fminf(sp_pos, 100.f) * (1.f - y) : 0.f;
            const float inv_t = 1.f / (float)T;
            row_loss = wave_sum(term) * inv_t;
            const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            g = (sig - y) * (inv_t / (float)p.B);
        } else if (p.kind == KEYFRAME_CE) {
            const bool on = sc && lab >= 0;
            const float m = wave_max(x);
            const float ex = is_frame ? expf(x - m) : 0.f;      // max-subtracted: the largest term is 1
            const float s = wave_sum(ex);
            const float xy = __shfl(x, lab >= 0 ? lab : 0, 64);
            row_loss = on ? (m - xy) + logf(s) : 0.f;
            g = on ? (ex / s - (lane == lab ? 1.f : 0.f)) / (float)p.B : 0.f;
        }
        if (p.dlogits) {            // the whole row of ld columns: the frame's gradient at its column, zero everywhere else
            float* drow = p.dlogits + (size_t)b * p.ld;
            for (int c0 = 0; c0 < p.ld; c0 += 64) {
                const int c = c0 + lane;
                int t = -1;
                if (p.has_cols) t = c < p.V ? (int)frame_of_s[c] : -1;
                else t = c < T ? c : -1;
                const float gt = __shfl(g, t >= 0 ? t : 0, 64);
                if (c < p.ld) drow[c] = t >= 0 ? gt : 0.f;
            }
        }
        loss_acc += row_loss;
        if (lane == 0) {
            p.pred[b] = pred;
            if (p.label_frame) p.label_frame[b] = lab >= 0 ? lab : -1;
            if (p.loss_rows) p.loss_rows[b] = row_loss;
            if (p.fps) {
                // metrics.py:57-67 in fp64, in that order: (end - start) / T * pred, minus (pnr - start), abs, over fps
                double d = 0.0;
                if (sc) {
                    const int64_t start = p.clip_start[b];
                    const double mapped = (double)(p.clip_end[b] - start) / (double)T * (double)pred;
                    const double gt = (double)(p.pnr_frame[b] - start);
                    d = fabs(mapped - gt) / p.fps[b];
                }
                if (p.dist) p.dist[b] = d;
                dist_acc += d;
            }
        }
    }
    if (lane == 0) {
        loss_s[wave] = loss_acc; dist_s[wave] = dist_acc;
        cnt_s[wave][0] = n_sc; cnt_s[wave][1] = n_correct; cnt_s[wave][2] = n_outside;
    }
    __syncthreads();
    // Workgroup partials -> scratch, the last workgroup to arrive sums them. The hand-off of segmented_ce_kernel (wave 0 stores and signals):
    // every handed-off word is stored write-through at agent scope, the wave drains its stores, then ONE relaxed agent-scope add draws the
    // ticket; the reader loads every such word at agent scope (past its CU's L1). No release fence, so no L2 write-back per workgroup.
    if (wave == 0) {
        if (lane == 0) {
            __hip_atomic_store(p.fpart + blockIdx.x, (loss_s[0] + loss_s[1]) + (loss_s[2] + loss_s[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(p.dpart + blockIdx.x, (dist_s[0] + dist_s[1]) + (dist_s[2] + dist_s[3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane < 3)
            __hip_atomic_store(p.ipart + blockIdx.x * 3 + lane, (cnt_s[0][lane] + cnt_s[1][lane]) + (cnt_s[2][lane] + cnt_s[3][lane]),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0)
            last_s = __hip_atomic_fetch_add(p.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)p.nchunks - 1;
    }
    __syncthreads();
    if (!last_s || wave != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // lane j holds chunk j (nchunks <= 64); every load is issued at a clamped, valid address and selected afterwards
    const bool in = lane < p.nchunks;
    const int j = min(lane, p.nchunks - 1);
    const float fv = __hip_atomic_load(p.fpart + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double dv = __hip_atomic_load(p.dpart + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int iv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) iv[k] = __hip_atomic_load(p.ipart + j * 3 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float fsum = wave_sum(in ? fv : 0.f);
    const double dsum = wave_sum(in ? dv : 0.0);
#pragma unroll
    for (int k = 0; k < 3; ++k) iv[k] = wave_sum(in ? iv[k] : 0);
    if (lane == 0) {
        if (p.loss) *p.loss = fsum / (float)p.B;
        if (p.dist_sum) *p.dist_sum = dsum;
        p.counts[0] = iv[0]; p.counts[1] = iv[1]; p.counts[2] = iv[2]; p.counts[3] = p.B;
        *p.counter = 0u;            // left zero for the next launch
    }
}

static int kf_check_B(int B) {
    EGX_CHECK(B >= 1 && B <= KEYFRAME_MAX_ROWS, "keyframe_criterion: B=%d (needs 1 <= B <= %d clips)", B, KEYFRAME_MAX_ROWS);
    return 0;
}

size_t keyframe_scratch_bytes(int B) {
    if (kf_check_B(B)) return 0;
    // [arrival counter: 64 B][distance partials][loss partials][count partials]: the same layout for every B
    return KF_COUNTER_BYTES + (size_t)KF_MAX_CHUNKS * (sizeof(double) + sizeof(float) + 3 * sizeof(int));
}

int keyframe_criterion(const float* logits, int ld, int B, int T, const int* cols, int V, int kind, const float* target, const int64_t* label,
                       const int64_t* state_change, const double* fps, const int64_t* clip_start, const int64_t* clip_end,
                       const int64_t* pnr_frame, float* loss, float* loss_rows, float* dlogits, int* pred, int* label_frame, int* counts,
                       double* dist, double* dist_sum, void* scratch, hipStream_t st) {
    EGX_CHECK(logits && counts && pred && scratch, "keyframe_criterion: null pointer argument (logits, pred, counts and scratch are required)");
    if (kf_check_B(B)) return 1;
    EGX_CHECK(T >= 1 && T <= KEYFRAME_MAX_T, "keyframe_criterion: T=%d (needs 1 <= T <= %d frames)", T, KEYFRAME_MAX_T);
    EGX_CHECK(V >= T && V <= KEYFRAME_MAX_V, "keyframe_criterion: V=%d (needs T <= V <= %d columns, T=%d)", V, KEYFRAME_MAX_V, T);
    EGX_CHECK(cols || V == T, "keyframe_criterion: V=%d without cols (needs V == T = %d: frame t is column t)", V, T);
    EGX_CHECK(ld >= V, "keyframe_criterion: ld=%d (needs ld >= V = %d)", ld, V);
    if (cols)
        for (int t = 0; t < T; ++t) {
            EGX_CHECK(cols[t] >= 0 && cols[t] < V, "keyframe_criterion: cols[%d]=%d (needs 0 <= column < V = %d)", t, cols[t], V);
            for (int u = 0; u < t; ++u) EGX_CHECK(cols[u] != cols[t], "keyframe_criterion: cols[%d] and cols[%d] are both %d (duplicate column)", u, t, cols[t]);
        }
    EGX_CHECK(kind == KEYFRAME_BCE || kind == KEYFRAME_CE || kind == KEYFRAME_METRIC, "keyframe_criterion: kind=%d (needs 0 bce, 1 ce or 2 metric)", kind);
    if (kind == KEYFRAME_METRIC) {
        EGX_CHECK(!loss && !loss_rows && !dlogits, "keyframe_criterion: kind metric takes no loss (loss, loss_rows and d_logits must be NULL)");
    } else {
        EGX_CHECK(kind != KEYFRAME_BCE || target, "keyframe_criterion: kind bce needs target");
        EGX_CHECK(kind != KEYFRAME_CE || target || label, "keyframe_criterion: kind ce needs target or label");
        EGX_CHECK(loss, "keyframe_criterion: null pointer argument (loss, with kind bce / ce)");
    }
    const int n_timing = (fps ? 1 : 0) + (clip_start ? 1 : 0) + (clip_end ? 1 : 0) + (pnr_frame ? 1 : 0);
    EGX_CHECK(n_timing == 0 || n_timing == 4, "keyframe_criterion: %d of the 4 timing arrays (fps, clip_start, clip_end, pnr_frame: all four, or none)", n_timing);
    EGX_CHECK(n_timing == 4 || (!dist && !dist_sum), "keyframe_criterion: dist / dist_sum without the timing arrays");
    KeyframeParams p;
    p.logits = logits; p.target = target; p.label = label; p.state_change = state_change;
    p.fps = fps; p.clip_start = clip_start; p.clip_end = clip_end; p.pnr_frame = pnr_frame;
    p.B = B; p.T = T; p.V = V; p.ld = ld; p.kind = kind; p.has_cols = cols ? 1 : 0;
    batch_chunks(B, KF_MAX_CHUNKS, KF_WAVES, &p.chunk, &p.nchunks);
    for (int t = 0; t < KEYFRAME_MAX_T; ++t) p.cols[t] = (cols && t < T) ? cols[t] : 0;
    p.loss = loss; p.loss_rows = loss_rows; p.dlogits = dlogits; p.pred = pred; p.label_frame = label_frame; p.counts = counts;
    p.dist = dist; p.dist_sum = dist_sum;
    p.counter = (unsigned*)scratch;
    p.dpart = (double*)((char*)scratch + KF_COUNTER_BYTES);
    p.fpart = (float*)(p.dpart + KF_MAX_CHUNKS);
    p.ipart = (int*)(p.fpart + KF_MAX_CHUNKS);
    hipLaunchKernelGGL(keyframe_criterion_kernel, dim3((unsigned)p.nchunks), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
