// The batch table of a ragged d = 128 batch built ON THE DEVICE from device lengths (egx_ragged_cap_train_fwd / egx_ragged_cap_bwd, fused.h
// RaggedTableParams): what ragged_plan() (fused_host.hip) builds on the host and ships in launch arguments, so that a captured hipGraph
// serves every batch that fits its capacity. With it the two small launches the capacity path adds: the zeroing of the rows no clip of this
// replay owns (the weight-gradient launches run at capacity sizes and must add exact zeros there) and the loss of a batch without clips.
#include "common.h"
#include "fused.h"

namespace egx {

namespace {
constexpr int RT_THREADS = 1024;
constexpr int RT_SUMS = 2 + FUSED_MAX_SEG;      // tiles, tokens, packed rows of segment 0 .. 3

// One workgroup. Thread t owns the clips [t per, (t + 1) per) (per = ceil(B_cap / 1024)): their sums, an inclusive scan of the 1024 thread sums
// in LDS, then the records from the thread's exclusive prefix on. Integer sums: the table is the same whatever the order.
__global__ __launch_bounds__(RT_THREADS) void ragged_table_kernel(RaggedTableParams p) {
    __shared__ int sc[RT_SUMS][RT_THREADS];
    __shared__ int bad_s;
    const int tid = threadIdx.x, K = p.K;
    const int per = (p.B_cap + RT_THREADS - 1) / RT_THREADS;
    const int b0 = min(tid * per, p.B_cap), b1 = min(b0 + per, p.B_cap);
    if (tid == 0) bad_s = 0;
    // ---- validation (the host cannot see these lengths) and the thread's own sums. A clip that fails adds nothing: no sum can overflow.
    int loc[RT_SUMS], bad = 0;
#pragma unroll
    for (int j = 0; j < RT_SUMS; ++j) loc[j] = 0;
    for (int b = b0; b < b1; ++b) {
        int S = 0, nz = 0, cb = 0, T[FUSED_MAX_SEG] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < FUSED_MAX_SEG; ++k) {
            if (k < K) {
                const int t = p.lengths[(size_t)b * K + k];
                if (t < 0 || t > p.T_pad[k]) cb |= RAGGED_BAD_LENGTH;
                else { T[k] = t; S += t; nz += t > 0; }
            }
        }
        if (!cb && nz != 0 && nz != K) cb |= RAGGED_BAD_PARTIAL;
        if (!cb && S > TILED_MAX_S) cb |= RAGGED_BAD_CLIP;
        bad |= cb;
        if (!cb) {
            loc[0] += (S + FUSED_TOK_PAD - 1) / FUSED_TOK_PAD; loc[1] += S;
#pragma unroll
            for (int k = 0; k < FUSED_MAX_SEG; ++k) loc[2 + k] += T[k];
        }
    }
#pragma unroll
    for (int j = 0; j < RT_SUMS; ++j) sc[j][tid] = loc[j];
    __syncthreads();
    for (int o = 1; o < RT_THREADS; o <<= 1) {
        int v[RT_SUMS];
#pragma unroll
        for (int j = 0; j < RT_SUMS; ++j) v[j] = tid >= o ? sc[j][tid - o] : 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RT_SUMS; ++j) sc[j][tid] += v[j];
        __syncthreads();
    }
    const int tiles_all = sc[0][RT_THREADS - 1], tok_all = sc[1][RT_THREADS - 1];
    if (tok_all > p.tok_cap || tiles_all > p.tile_cap) bad |= RAGGED_BAD_TOKENS;        // (tokens within the capacity imply tiles within it)
    if (bad) atomicOr(&bad_s, bad);
    __syncthreads();
    const int bad_all = bad_s;

    int* rec0 = p.tab;
    int* map = p.tab + (size_t)p.B_cap * RAGGED_REC;
    int* rseg = map + p.tile_cap;
    int* meta = rseg + (size_t)p.B_cap * FUSED_MAX_SEG;
    if (bad_all) {
        // a batch the kernels must not run: the table of an EMPTY batch (every clip empty, every tile surplus), so that no length indexes anything;
        // the call completes with zero logits, zero loss and zero gradients, and the sticky status word says why
        for (int b = b0; b < b1; ++b) {
            for (int j = 0; j < RAGGED_REC; ++j) rec0[(size_t)b * RAGGED_REC + j] = 0;
            for (int k = 0; k < FUSED_MAX_SEG; ++k) rseg[(size_t)b * FUSED_MAX_SEG + k] = 0;
            if (p.eff_target) p.eff_target[b] = -1;
        }
        for (int j = tid; j < p.tile_cap; j += RT_THREADS) map[j] = -1;
        if (tid < RAGGED_META) meta[tid] = tid == RM_STATUS ? bad_all : 0;
        if (tid == 0 && p.status) atomicOr(p.status, (unsigned)bad_all);
        return;
    }
    int run[RT_SUMS];
#pragma unroll
    for (int j = 0; j < RT_SUMS; ++j) run[j] = sc[j][tid] - loc[j];        // exclusive prefix of the thread's first clip
    for (int b = b0; b < b1; ++b) {
        int* rec = rec0 + (size_t)b * RAGGED_REC;
        int S = 0, T[FUSED_MAX_SEG] = {0, 0, 0, 0};
        for (int j = 0; j < RAGGED_REC; ++j) rec[j] = 0;        // an empty clip's record is zero
#pragma unroll
        for (int k = 0; k < FUSED_MAX_SEG; ++k) {
            if (k < K) { T[k] = p.lengths[(size_t)b * K + k]; if (T[k] > 0) { rec[RG_T + k] = T[k]; rec[RG_OFF + k] = S; } S += T[k]; }
            rseg[(size_t)b * FUSED_MAX_SEG + k] = k < K ? run[2 + k] : 0;
        }
        if (p.eff_target) p.eff_target[b] = (S > 0 && p.target) ? p.target[b] : -1;     // an empty clip never reaches the loss (weighted_ce skips labels < 0)
        if (S > 0) {
            const int nt = (S + FUSED_TOK_PAD - 1) / FUSED_TOK_PAD;
            rec[RG_TILE0] = run[0]; rec[RG_S] = S; rec[RG_TOK0] = run[1];
            rec[RG_OUT0] = run[1]; rec[RG_OUTN] = S;        // with a head (the only case here): every token of the clip leaves the last layer
            for (int j = 0; j < nt; ++j) map[run[0] + j] = b;
            run[0] += nt; run[1] += S;
#pragma unroll
            for (int k = 0; k < FUSED_MAX_SEG; ++k) run[2 + k] += T[k];
        }
    }
    for (int j = tiles_all + tid; j < p.tile_cap; j += RT_THREADS) map[j] = -1;       // surplus tiles: their workgroups leave at once
    if (tid == 0) {
        meta[RM_TOKENS] = tok_all; meta[RM_TILES] = tiles_all;
        for (int k = 0; k < FUSED_MAX_SEG; ++k) meta[RM_SEG_ROWS + k] = sc[2 + k][RT_THREADS - 1];
        meta[RM_STATUS] = 0;
        meta[RM_ANY] = tok_all > 0 ? 1 : 0;
    }
}

// rows [first, cap_rows) of every listed array, first from the table's totals; float4 stores, SLACK_BLOCKS workgroups per array
constexpr int SLACK_BLOCKS = 16;
__global__ __launch_bounds__(256) void ragged_slack_zero_kernel(RaggedSlackParams p) {
    const RaggedSlackDesc d = p.d[blockIdx.y];
    int first = p.meta[d.kind == RS_TOKENS ? RM_TOKENS : d.kind == RS_TILES ? RM_TILES : RM_SEG_ROWS + (d.kind - RS_SEG0)];
    first = first < 0 ? 0 : first;
    if (first >= d.cap_rows) return;
    const size_t q0 = (size_t)first * (d.row_bytes / 16), q1 = (size_t)d.cap_rows * (d.row_bytes / 16);
    float4* dst = reinterpret_cast<float4*>(d.base);
    for (size_t i = q0 + (size_t)blockIdx.x * 256 + threadIdx.x; i < q1; i += (size_t)SLACK_BLOCKS * 256) dst[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ void ragged_empty_loss_kernel(const int* meta, float* loss) {
    if (!meta[RM_ANY]) *loss = 0.f;      // no clip: weighted_ce left 0 / 0
}
}  // namespace

int ragged_table_build(const RaggedTableParams& p, hipStream_t st) {
    EGX_CHECK(p.lengths && p.tab && p.K >= 1 && p.K <= FUSED_MAX_SEG && p.B_cap >= 1 && p.tok_cap >= 1 && p.tile_cap >= 1,
              "ragged table: null pointer or empty capacity");
    hipLaunchKernelGGL(ragged_table_kernel, dim3(1), dim3(RT_THREADS), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

int ragged_slack_add(RaggedSlackParams& p, void* base, size_t row_bytes, size_t cap_rows, int kind) {
    if (!base || !cap_rows) return 0;
    EGX_CHECK(p.n < RAGGED_SLACK_MAX, "ragged capacity: more than %d arrays to clear", RAGGED_SLACK_MAX);
    EGX_CHECK(row_bytes % 16 == 0 && (((uintptr_t)base) & 15) == 0 && row_bytes < ((size_t)1 << 31) && cap_rows < ((size_t)1 << 31),
              "ragged capacity: rows of %zu bytes at %p cannot be cleared in 16-byte pieces", row_bytes, base);
    RaggedSlackDesc& d = p.d[p.n++];
    d.base = (char*)base; d.row_bytes = (unsigned)row_bytes; d.cap_rows = (int)cap_rows; d.kind = kind;
    return 0;
}

int ragged_slack_zero(const RaggedSlackParams& p, hipStream_t st) {
    if (!p.n) return 0;
    EGX_CHECK(p.meta, "ragged capacity: the table's totals are missing");
    hipLaunchKernelGGL(ragged_slack_zero_kernel, dim3(SLACK_BLOCKS, p.n), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

int ragged_empty_loss(const int* meta, float* loss, hipStream_t st) {
    hipLaunchKernelGGL(ragged_empty_loss_kernel, dim3(1), dim3(1), 0, st, meta, loss);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
