// Gradient-norm clipping and the non-finite guard of the captured step (ABI v28 additions: egx_grad_norm and the gated / guarded twins of the
// bump and update launches, which live next to the kernels they mirror in train.hip).
//
// The reference trains through Lightning's Trainer (HHI/scripts/run_ttm.py:21, HOI/scripts/lta/run_lta.py:238) with gradient_clip_val and
// track_grad_norm at their defaults, so this is not a parity item: it is what a recipe moved onto train.GraphedStep expects to keep. In a
// replayed graph the host cannot look at the loss or the gradients, so the norm and the decision are device work:
//
//   grad_sqsum_kernel    sum of squares of up to GRAD_NORM_TABLE flat fp32 buffers in ONE grouped launch, in fp64 (every square of an fp32 is
//                        exact there, and no finite fp32 can overflow the sum) and in a fixed order: element -> thread -> wave -> workgroup is
//                        a function of the buffer sizes alone, not of timing and not of a buffer's alignment. One fp64 partial per workgroup,
//                        a plain store to its own slot. Bandwidth-bound: 4 B read per element, a few fp64 FMAs per 16 B.
//   guard_finish_kernel  one workgroup adds the partials in index order and writes norm, coef (torch.nn.utils.clip_grad_norm_'s formula),
//                        apply and the counters. A launch of its own instead of a last-arriver ticket in the first: ~2 us more, and no spin,
//                        no fence protocol, nothing that could hang.
#include <math.h>

#include "../../include/egot2x.h"
#include "common.h"
#include "kernels.h"

namespace egx {

static_assert(sizeof(GuardBlock) == sizeof(egx_guard_block) && sizeof(GuardBlock) == 40, "GuardBlock is egx_guard_block");
static_assert(offsetof(GuardBlock, coef) == offsetof(egx_guard_block, coef) && offsetof(GuardBlock, apply) == offsetof(egx_guard_block, apply) &&
              offsetof(GuardBlock, steps) == offsetof(egx_guard_block, steps) && offsetof(GuardBlock, clipped) == offsetof(egx_guard_block, clipped),
              "GuardBlock is egx_guard_block");
static_assert(GRAD_NORM_TABLE == EGX_GRAD_NORM_TABLE, "one table size");

constexpr int GG_THREADS = 256, GG_WAVES = GG_THREADS / 64;

// The buffers of one grouped launch: workgroups [blk0[i], blk0[i + 1]) serve buffer i (none for an empty one)
struct SqsumTable {
    const float* p[GRAD_NORM_TABLE];
    unsigned long long n[GRAD_NORM_TABLE];
    unsigned blk0[GRAD_NORM_TABLE + 1];
    int count;
};

__device__ __forceinline__ void sq_acc4(double (&acc)[4], const float4 x) {
    acc[0] = fma((double)x.x, (double)x.x, acc[0]);
    acc[1] = fma((double)x.y, (double)x.y, acc[1]);
    acc[2] = fma((double)x.z, (double)x.z, acc[2]);
    acc[3] = fma((double)x.w, (double)x.w, acc[3]);
}

// Thread t of a buffer's nb workgroups owns the 4-element groups t, t + nb * 256, ...; lane e of a group goes to accumulator e. The aligned
// path reads a group as one float4, the other as four floats: the same values into the same accumulators in the same order.
__global__ __launch_bounds__(GG_THREADS) void grad_sqsum_kernel(SqsumTable tab, double* __restrict__ partial) {
    int b = 0;
    while (b + 1 < tab.count && blockIdx.x >= tab.blk0[b + 1]) ++b;
    const float* __restrict__ g = tab.p[b];
    const size_t n = tab.n[b];
    const size_t nb = tab.blk0[b + 1] - tab.blk0[b];
    const size_t stride = nb * GG_THREADS, full = n >> 2;
    size_t v = (size_t)(blockIdx.x - tab.blk0[b]) * GG_THREADS + threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
        for (; v + 3 * stride < full; v += 4 * stride) {        // four loads in flight; accumulated in the order of the plain loop
            const float4 x0 = g4[v], x1 = g4[v + stride], x2 = g4[v + 2 * stride], x3 = g4[v + 3 * stride];
            sq_acc4(acc, x0); sq_acc4(acc, x1); sq_acc4(acc, x2); sq_acc4(acc, x3);
        }
        for (; v < full; v += stride) sq_acc4(acc, g4[v]);
    } else {
        for (; v < full; v += stride) sq_acc4(acc, make_float4(g[4 * v], g[4 * v + 1], g[4 * v + 2], g[4 * v + 3]));
    }
    if (v == full) {                                            // exactly one thread: the n % 4 elements behind the last whole group
        for (size_t j = 4 * full; j < n; ++j) acc[j & 3] = fma((double)g[j], (double)g[j], acc[j & 3]);
    }
    double s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double wave_sum[GG_WAVES];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

struct GuardFinishArgs {
    const double* partial; unsigned long long n_partials;
    double max_norm; int has_max_norm, skip_nonfinite;
    GuardBlock* guard;
};

// Thread t adds its run of ceil(n / 256) consecutive partials in index order, thread 0 the 256 run sums in thread order.
__global__ __launch_bounds__(GG_THREADS) void guard_finish_kernel(GuardFinishArgs a) {
#pragma clang fp contract(off)
    __shared__ double run_sum[GG_THREADS];
    const size_t run = (a.n_partials + GG_THREADS - 1) / GG_THREADS;
    const size_t lo = threadIdx.x * run, hi = lo + run < a.n_partials ? lo + run : a.n_partials;
    double s = 0.0;
    for (size_t i = lo; i < hi; ++i) s += a.partial[i];
    run_sum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sqsum = 0.0;
    for (int t = 0; t < GG_THREADS; ++t) sqsum += run_sum[t];
    const double norm = sqrt(sqsum);
    const bool finite = isfinite(sqsum);
    float coef = 1.0f;
    if (a.has_max_norm) {
        const double c = a.max_norm / (norm + 1e-6);
        if (c < 1.0) coef = (float)c;
    }
    const int apply = (finite || !a.skip_nonfinite) ? 1 : 0;
    GuardBlock* gb = a.guard;
    gb->norm = norm;
    gb->coef = coef;
    gb->apply = apply;
    gb->steps += 1;
    if (!apply) gb->skipped += 1;
    else if (coef < 1.0f) gb->clipped += 1;
}

// Workgroups of every buffer of one grouped launch: one per 1024 elements while GRAD_NORM_MAX_BLOCKS allows; beyond it every non-empty buffer
// keeps one and the rest of the budget is shared in proportion to the sizes. A function of the sizes alone. Returns their sum.
static unsigned plan_blocks(const size_t* ns, int count, unsigned* blocks) {
    unsigned long long want[GRAD_NORM_TABLE], total = 0;
    int nonempty = 0;
    for (int i = 0; i < count; ++i) {
        want[i] = ((unsigned long long)ns[i] + 1023) / 1024;
        total += want[i];
        nonempty += want[i] != 0;
    }
    unsigned sum = 0;
    for (int i = 0; i < count; ++i) {
        unsigned long long nb = want[i];
        if (total > (unsigned long long)GRAD_NORM_MAX_BLOCKS && nb != 0) {
            const unsigned long long budget = GRAD_NORM_MAX_BLOCKS - nonempty;
            const unsigned long long share = 1 + (unsigned long long)((unsigned __int128)budget * (nb - 1) / (total - nonempty));
            if (share < nb) nb = share;
        }
        blocks[i] = (unsigned)nb;
        sum += blocks[i];
    }
    return sum;
}

static bool sizes_ok(const size_t* ns, int n_bufs) { return ns != nullptr && n_bufs >= 1; }

size_t grad_norm_scratch_bytes(const size_t* ns, int n_bufs) {
    if (!sizes_ok(ns, n_bufs)) return 0;
    size_t partials = 0;
    unsigned blocks[GRAD_NORM_TABLE];
    for (int i0 = 0; i0 < n_bufs; i0 += GRAD_NORM_TABLE)
        partials += plan_blocks(ns + i0, n_bufs - i0 < GRAD_NORM_TABLE ? n_bufs - i0 : GRAD_NORM_TABLE, blocks);
    return align_up((partials > 0 ? partials : 1) * sizeof(double), 256);
}

int grad_norm(const float* const* bufs, const size_t* ns, int n_bufs, void* scratch, size_t scratch_bytes, double max_norm, int has_max_norm,
              int skip_nonfinite, GuardBlock* guard, hipStream_t st) {
    const char* who = "egx_grad_norm";
    EGX_CHECK(n_bufs >= 1, "%s: n_bufs = %d (needs n_bufs >= 1)", who, n_bufs);
    EGX_CHECK(bufs && ns && scratch && guard, "%s: null pointer argument (bufs, ns, scratch or guard)", who);
    EGX_CHECK(!has_max_norm || max_norm >= 0.0, "%s: max_norm = %g (needs max_norm >= 0 and not NaN)", who, max_norm);
    for (int i = 0; i < n_bufs; ++i) {
        EGX_CHECK(bufs[i] || ns[i] == 0, "%s: null pointer argument (buffer %d of %zu elements)", who, i, ns[i]);
        EGX_CHECK((reinterpret_cast<uintptr_t>(bufs[i]) & 3) == 0, "%s: buffer %d at %p is not 4-byte aligned", who, i, (const void*)bufs[i]);
    }
    EGX_CHECK((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "%s: scratch at %p is not 8-byte aligned", who, scratch);
    const size_t need = grad_norm_scratch_bytes(ns, n_bufs);
    EGX_CHECK(scratch_bytes >= need, "%s: scratch of %zu bytes, egx_grad_norm_scratch_bytes asks for %zu", who, scratch_bytes, need);
    double* partial = static_cast<double*>(scratch);
    size_t done = 0;
    for (int i0 = 0; i0 < n_bufs; i0 += GRAD_NORM_TABLE) {
        SqsumTable tab;
        unsigned blocks[GRAD_NORM_TABLE];
        tab.count = n_bufs - i0 < GRAD_NORM_TABLE ? n_bufs - i0 : GRAD_NORM_TABLE;
        const unsigned total = plan_blocks(ns + i0, tab.count, blocks);
        tab.blk0[0] = 0;
        for (int i = 0; i < GRAD_NORM_TABLE; ++i) {
            const bool live = i < tab.count;
            tab.p[i] = live ? bufs[i0 + i] : nullptr;
            tab.n[i] = live ? ns[i0 + i] : 0;
            tab.blk0[i + 1] = tab.blk0[i] + (live ? blocks[i] : 0);
        }
        if (total == 0) continue;                   // only empty buffers in this range
        hipLaunchKernelGGL(grad_sqsum_kernel, dim3(total), dim3(GG_THREADS), 0, st, tab, partial + done);
        EGX_LAUNCH_CHECK();
        done += total;
    }
    GuardFinishArgs a;
    a.partial = partial; a.n_partials = done; a.max_norm = has_max_norm ? max_norm : 0.0; a.has_max_norm = has_max_norm ? 1 : 0;
    a.skip_nonfinite = skip_nonfinite ? 1 : 0; a.guard = guard;
    hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(GG_THREADS), 0, st, a);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx

using namespace egx;

extern "C" {

size_t egx_grad_norm_scratch_bytes(const size_t* ns, int n_bufs) { return grad_norm_scratch_bytes(ns, n_bufs); }

int egx_grad_norm(const float* const* bufs, const size_t* ns, int n_bufs, void* scratch, size_t scratch_bytes, const egx_grad_norm_cfg* cfg,
                  egx_guard_block* guard, void* stream) {
    EGX_CHECK(cfg, "egx_grad_norm: null pointer argument (cfg)");
    return grad_norm(bufs, ns, n_bufs, scratch, scratch_bytes, cfg->max_norm, cfg->has_max_norm, cfg->skip_nonfinite,
                     reinterpret_cast<GuardBlock*>(guard), (hipStream_t)stream);
}

int egx_counter_add_gated(int64_t* counter, int64_t inc, const egx_guard_block* guard, void* stream) {
    return counter_add_gated(counter, inc, reinterpret_cast<const GuardBlock*>(guard), (hipStream_t)stream);
}

int egx_lr_update_gated(const egx_lr_schedule* schedule, int64_t* step, const double* base_lr, int n_groups, float* lr_out,
                        const egx_guard_block* guard, void* stream) {
    EGX_CHECK(schedule, "lr_update_gated: null schedule");
    return lr_update_gated(schedule->kind, schedule->warmup_steps, schedule->t_total, schedule->T_max, schedule->cycles, schedule->factors,
                           schedule->n, step, base_lr, n_groups, lr_out, reinterpret_cast<const GuardBlock*>(guard), (hipStream_t)stream);
}

int egx_adam_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const int64_t* step,
                          const float* lr_dev, float lr, float beta1, float beta2, float eps, float weight_decay, int decoupled,
                          const egx_guard_block* guard, void* stream) {
    EGX_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f,
              "adam_step_guarded: invalid hyper-parameters (needs 0 <= beta < 1, eps >= 0)");
    return adam_step_guarded(param, grad, exp_avg, exp_avg_sq, n, step, lr_dev, lr, beta1, beta2, eps, weight_decay, decoupled,
                             reinterpret_cast<const GuardBlock*>(guard), (hipStream_t)stream);
}

int egx_sgd_step_guarded(float* param, const float* grad, float* momentum_buf, size_t n, const int64_t* step, const float* lr_dev, float lr,
                         float momentum, float dampening, float weight_decay, int nesterov, const egx_guard_block* guard, void* stream) {
    return sgd_step_guarded(param, grad, momentum_buf, n, step, lr_dev, lr, momentum, dampening, weight_decay, nesterov,
                            reinterpret_cast<const GuardBlock*>(guard), (hipStream_t)stream);
}

}  // extern "C"
