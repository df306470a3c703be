// Shared by the kernels around a rendered frame and the optimiser step (eval.hip, vis.hip, optim.hip): the workgroup fold
// their bit-exact sums and extrema go through, the byte quantisation and its inverse (video.hip, data.hip), and the 16 x 16
// pixel tiling of a frame.
#pragma once
#include "pnr_common.h"

namespace pnr {

// The LDS tree of an N = 256 thread workgroup: thread t combines its slot with t + 128, then t + 64, .., t + 1 (8 levels), so
// slot 0 holds the result in an order fixed by the launch shape alone: what the bit-exact tests of these kernels rest on.  The
// caller fills its LDS arrays at [tid]; fold(i, j) combines slot j INTO slot i with i, the lower index, on the left (nan_min is
// not symmetric in NaN payloads) and may cover several arrays, which then share the barriers.  Ends on the last level's
// barrier: slot 0 may be read at once, and whoever reuses the arrays syncs first.
template <int N, class Fold> __device__ __forceinline__ void block_fold(int tid, Fold fold) {
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) fold(tid, tid + s);
        __syncthreads();
    }
}

// clamp to [0, 1] that keeps a NaN (fminf / fmaxf would turn it into a bound: the host path's metrics are NaN then)
__device__ __forceinline__ float clamp01(float v) { return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
// (x * 255).astype(uint8) of a clamped value: ONE fp32 product, then truncation ((k / 255) * 255 may land just below k); NaN -> 0
__device__ __forceinline__ uint8_t quant_u8(float x) { return x == x ? (uint8_t)(int)__fmul_rn(x, 255.0f) : (uint8_t)0; }
// T(b, balanced), an image byte as the network's input (include/pnr.h, pnr_image_to_tensor): float(b) / 255.0f, ONE correctly
// rounded division (torchvision's ToTensor); balanced: then (. - 0.5f) / 0.5f, each operation rounded on its own (Normalize(0.5,
// 0.5)).  The only place this arithmetic exists: pnr_image_to_tensor, pnr_views_to_tensor_u8 and pnr_train_batch_u8 call it.
// unit_to_tensor is its second half on its own: the colour-jitter gathers (data_u8.h) put their chain between the two.
__device__ __forceinline__ float unit_to_tensor(float v, int balanced) { return balanced ? __fdiv_rn(__fsub_rn(v, 0.5f), 0.5f) : v; }
__device__ __forceinline__ float u8_to_tensor(uint32_t b, int balanced) {
    return unit_to_tensor(__fdiv_rn((float)b, 255.0f), balanced);
}

// ---------------------------------------------------------------- a frame as 16 x 16 pixel tiles, one workgroup per tile
constexpr int FRAME_TILE = 16;                              // pixels per tile edge; one thread per pixel
constexpr int FRAME_THREADS = FRAME_TILE * FRAME_TILE;      // 256 = 4 waves
constexpr int64_t FRAME_MAX_TILES = (int64_t)1 << 23;       // 2^23 workgroups of 256 threads: a launch stays below 2^32 threads
struct Pixel { int x, y; };
// top-left pixel of workgroup `block`'s tile (tiles in row-major order), and the pixel thread `tid` owns in it
__device__ __forceinline__ Pixel tile_origin(int block, int tiles_x) {
    return {(block % tiles_x) * FRAME_TILE, (block / tiles_x) * FRAME_TILE};
}
__device__ __forceinline__ Pixel tile_pixel(int block, int tiles_x, int tid) {
    return {tile_origin(block, tiles_x).x + (tid & (FRAME_TILE - 1)), tile_origin(block, tiles_x).y + tid / FRAME_TILE};
}
static inline int frame_tiles_x(int32_t W) { return (W + FRAME_TILE - 1) / FRAME_TILE; }
static inline int64_t frame_tiles(int32_t W, int32_t H) { return (int64_t)frame_tiles_x(W) * frame_tiles_x(H); }
// a frame whose pixel index fits an int32; frame_shape_ok: and whose tiles fit one launch
static inline bool frame_pixels_ok(int32_t W, int32_t H) { return W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31); }
static inline bool frame_shape_ok(int32_t W, int32_t H) { return frame_pixels_ok(W, H) && frame_tiles(W, H) <= FRAME_MAX_TILES; }

}  // namespace pnr
