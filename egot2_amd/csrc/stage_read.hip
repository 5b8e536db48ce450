// Stage read (test hook, ABI v26): copies ONE intermediate of a d = 128 encoder call out of its workspaces into a dense row-major matrix
// in token order. Plain C++, one thread per output element: nothing here is on a product path. The layouts are the producers': the
// offsets come from fused_host.hip, the tile and bit positions from fused_dev.h (hid_tile_index_*, alive_bit_index).
#include "common.h"
#include "fused.h"
#include "fused_dev.h"

namespace egx {

// row of the 48-row clip / tile grid that holds dense token n
__device__ static size_t grid_row(const StageReadParams& p, int n) {
    if (p.rtab) {
        for (int b = 0; b < p.B_clips; ++b) {       // (an empty clip of a capacity batch has a zero record: it owns no token)
            const int* rec = p.rtab + (size_t)b * RAGGED_REC;
            if (n >= rec[RG_TOK0] && n < rec[RG_TOK0] + rec[RG_S]) return (size_t)rec[RG_TILE0] * FUSED_TOK_PAD + (size_t)(n - rec[RG_TOK0]);
        }
        return 0;       // (never: the host sizes `rows` by the batch's tokens)
    }
    const int c = n / p.S_clip, s = n - c * p.S_clip;
    return (size_t)c * p.tpc * FUSED_TOK_PAD + s;
}

__device__ static float bf16_widen(unsigned short h) { return __uint_as_float((uint32_t)h << 16); }

__global__ __launch_bounds__(256) void stage_read_kernel(StageReadParams p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.rows * p.cols) return;
    const int n = (int)(i / p.cols), c = (int)(i - (size_t)n * p.cols);
    float v = 0.f;
    if (p.layout == SR_DENSE) {
        v = reinterpret_cast<const float*>(p.src)[i];
    } else {
        const size_t g = grid_row(p, n);
        if (p.layout == SR_GRID) {
            v = reinterpret_cast<const float*>(p.src)[g * p.cols + c];
        } else if (p.layout == SR_PLANES) {
            const unsigned short* s = reinterpret_cast<const unsigned short*>(p.src) + g * p.cols + c;
            for (int k = 0; k < p.n_planes; ++k) v += bf16_widen(s[(size_t)k * p.plane_stride]);      // high + middle + low part: exact
        } else {
            const size_t tile = g / FUSED_TOK_PAD;                  // the workgroup ("virtual clip") that owns the row
            const int row = (int)(g - tile * FUSED_TOK_PAD), t = row >> 4, r = row & 15;
            if (p.layout == SR_HID) {
                const int nht = p.cols / 16, ht = c >> 4, u = c & 15;
                const size_t base = ((tile * FUSED_TOK_TILES + t) * nht + ht) * (size_t)HTILE_ELEMS;
                v = p.bf16 ? bf16_widen(reinterpret_cast<const unsigned short*>(p.src)[base + hid_tile_index_bf16(r, u)])
                           : reinterpret_cast<const float*>(p.src)[base + hid_tile_index_f32(r, u)];
            } else {        // SR_ALIVE
                const int hb = c >> 5, u = c & 31, lane = r + 16 * ((u & 15) >> 2);
                const uint32_t word = reinterpret_cast<const uint32_t*>(p.src)[(tile * (size_t)(p.cols / 32) + hb) * 64 + lane];
                v = (float)((word >> alive_bit_index(t, u)) & 1u);
            }
        }
    }
    if (p.out_bytes == 1) reinterpret_cast<unsigned char*>(p.out)[i] = v != 0.f ? 1 : 0;
    else reinterpret_cast<float*>(p.out)[i] = v;
}

int stage_read(const StageReadParams& p, hipStream_t st) {
    EGX_CHECK(p.src && p.out && p.rows >= 0 && p.cols > 0, "stage read: null pointer or empty item");
    EGX_CHECK(p.out_bytes == 4 || p.out_bytes == 1, "stage read: out_bytes=%d", p.out_bytes);
    const size_t n = (size_t)p.rows * p.cols;
    if (!n) return 0;
    EGX_CHECK(n < ((size_t)1 << 31) * 256, "stage read: item too large");
    hipLaunchKernelGGL(stage_read_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
    EGX_LAUNCH_CHECK();
    return 0;
}

}  // namespace egx
