// Area resampling, upstream pixelNeRF's F.interpolate(mode="area") of its images (include/pnr.h, pnr_resize_area_u8 /
// pnr_resize_area_f32, fixes the arithmetic): every target sample is the mean of the source samples under its window
//   [floor(i n_in / n_out), ceil((i + 1) n_in / n_out))  along each axis, in integer arithmetic.
//   k_resize_area_u8   interleaved bytes (F, H, W, C) -> (F, Ht, Wt, C): exact integer window sums, the mean rounded half up
//   k_resize_area_f32  fp32 planes (F, H, W) -> (F, Ht, Wt): the window summed in fp64 row-major, ONE rounding to fp32
// In both a thread owns ONE target pixel and the lanes of a wave run along a target row, so what a wave reads of one source
// row is one contiguous segment (neighbouring windows touch or overlap) and what it writes is one contiguous run.  The byte
// input is read byte by byte — C consecutive bytes per lane and column, never a lane per channel — since a pool slot starts at
// any byte.  Both are bound by memory: a source byte is read once (up to the overlap), a target byte written once; nothing is
// kept between launches, no workspace, no atomics, and the bits depend on nothing but the input.  A window is summed by ONE
// thread in the header's order: a target far smaller than its source (a 1 x 1 target of a large image) runs long, not wrong.
#include "pnr_common.h"

namespace pnr {

constexpr int RSZ_THREADS = 256;                          // 4 waves

// The window of target index i (include/pnr.h).  i < n_out < 2^31 and n_in < 2^31: the products need 64 bits.
__device__ __forceinline__ void area_window(int i, int n_in, int n_out, int& lo, int& hi) {
    lo = (int)(((int64_t)i * n_in) / n_out);
    hi = (int)((((int64_t)i + 1) * n_in + n_out - 1) / n_out);
}

// Workgroup b serves frame b / blocks_per_frame and the target pixels [256 c, 256 c + 256) of it, row-major,
// c = b % blocks_per_frame.  The sums are 64-bit: 255 * n < 2^39 for every window the size checks admit (n <= H W < 2^31).
template <int C>
__global__ void __launch_bounds__(RSZ_THREADS) k_resize_area_u8(const uint8_t* __restrict__ in, int64_t in_stride, int H, int W,
                                                                uint8_t* __restrict__ out, int64_t out_stride, int Ht, int Wt,
                                                                int blocks_per_frame) {
    const int64_t f = blockIdx.x / (unsigned)blocks_per_frame;
    const int chunk = (int)(blockIdx.x - (unsigned)f * (unsigned)blocks_per_frame);
    const int64_t p = (int64_t)chunk * RSZ_THREADS + threadIdx.x;              // may pass 2^31 in the last workgroup: 64 bits
    if (p >= (int64_t)Ht * Wt) return;
    const int y = (int)(p / Wt), x = (int)(p - (int64_t)y * Wt);
    int r0, r1, c0, c1;
    area_window(y, H, Ht, r0, r1);
    area_window(x, W, Wt, c0, c1);
    const uint8_t* frame = in + f * in_stride;
    uint64_t S[C];
#pragma unroll
    for (int k = 0; k < C; ++k) S[k] = 0;
    for (int r = r0; r < r1; ++r) {
        const uint8_t* q = frame + ((int64_t)r * W + c0) * C;
        for (int c = c0; c < c1; ++c, q += C) {
#pragma unroll
            for (int k = 0; k < C; ++k) S[k] += q[k];
        }
    }
    const uint64_t n = (uint64_t)(r1 - r0) * (uint64_t)(c1 - c0);
    uint8_t* d = out + f * out_stride + p * C;
#pragma unroll
    for (int k = 0; k < C; ++k) d[k] = (uint8_t)((2 * S[k] + n) / (2 * n));
}

// grid = planes x chunks of a target plane; one thread, one target element
__global__ void __launch_bounds__(RSZ_THREADS) k_resize_area_f32(const float* __restrict__ in, int H, int W, float* __restrict__ out,
                                                                 int Ht, int Wt, int blocks_per_frame) {
    const int64_t f = blockIdx.x / (unsigned)blocks_per_frame;
    const int chunk = (int)(blockIdx.x - (unsigned)f * (unsigned)blocks_per_frame);
    const int64_t p = (int64_t)chunk * RSZ_THREADS + threadIdx.x;
    if (p >= (int64_t)Ht * Wt) return;
    const int y = (int)(p / Wt), x = (int)(p - (int64_t)y * Wt);
    int r0, r1, c0, c1;
    area_window(y, H, Ht, r0, r1);
    area_window(x, W, Wt, c0, c1);
    const float* plane = in + f * ((int64_t)H * W);
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) {
        const float* q = plane + (int64_t)r * W;
        for (int c = c0; c < c1; ++c) acc += (double)q[c];
    }
    const double n = (double)((int64_t)(r1 - r0) * (int64_t)(c1 - c0));        // < 2^31: exact
    out[f * ((int64_t)Ht * Wt) + p] = (float)(acc / n);
}

// The size checks both entry points share: the workgroups of one frame, or 0 for sizes that are refused.
static inline int64_t resize_blocks_per_frame(int32_t F, int32_t H, int32_t W, int32_t Ht, int32_t Wt) {
    const int64_t lim = (int64_t)1 << 31;
    if (F < 1 || H < 1 || W < 1 || Ht < 1 || Wt < 1 || (int64_t)H * W >= lim || (int64_t)Ht * Wt >= lim) return 0;
    const int64_t bpf = ((int64_t)Ht * Wt + RSZ_THREADS - 1) / RSZ_THREADS;    // <= 2^23
    if ((int64_t)F > (lim - 1) / bpf) return 0;                                 // one launch: the grid's x extent
    return bpf;
}

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_resize_area_u8(const uint8_t* in_u8, int64_t in_stride, int32_t F, int32_t H, int32_t W, int32_t C,
                                      uint8_t* out_u8, int64_t out_stride, int32_t Ht, int32_t Wt, void* stream) {
    if (!in_u8 || !out_u8) return PNR_E_NULL;
    const int64_t bpf = resize_blocks_per_frame(F, H, W, Ht, Wt);
    if (bpf == 0 || C < 1 || C > 4) return PNR_E_SHAPE;
    if (in_stride < (int64_t)H * W * C || out_stride < (int64_t)Ht * Wt * C) return PNR_E_SHAPE;
    const dim3 grid((unsigned)(F * bpf)), block(RSZ_THREADS);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: hipLaunchKernelGGL(k_resize_area_u8<1>, grid, block, 0, s, in_u8, in_stride, H, W, out_u8, out_stride, Ht, Wt, (int)bpf); break;
        case 2: hipLaunchKernelGGL(k_resize_area_u8<2>, grid, block, 0, s, in_u8, in_stride, H, W, out_u8, out_stride, Ht, Wt, (int)bpf); break;
        case 3: hipLaunchKernelGGL(k_resize_area_u8<3>, grid, block, 0, s, in_u8, in_stride, H, W, out_u8, out_stride, Ht, Wt, (int)bpf); break;
        default: hipLaunchKernelGGL(k_resize_area_u8<4>, grid, block, 0, s, in_u8, in_stride, H, W, out_u8, out_stride, Ht, Wt, (int)bpf); break;
    }
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_resize_area_f32(const float* in, int32_t F, int32_t H, int32_t W, float* out, int32_t Ht, int32_t Wt,
                                       void* stream) {
    if (!in || !out) return PNR_E_NULL;
    const int64_t bpf = resize_blocks_per_frame(F, H, W, Ht, Wt);
    if (bpf == 0) return PNR_E_SHAPE;
    if ((((uintptr_t)in) & 3) != 0 || (((uintptr_t)out) & 3) != 0) return PNR_E_ALIGN;
    hipLaunchKernelGGL(k_resize_area_f32, dim3((unsigned)(F * bpf)), dim3(RSZ_THREADS), 0, (hipStream_t)stream, in, H, W, out, Ht, Wt,
                       (int)bpf);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
