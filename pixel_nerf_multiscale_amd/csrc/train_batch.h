// The ray half of a training batch row, shared by k_train_batch (stage_kernels.hip, fp32 images) and k_train_batch_u8
// (data.hip, 8-bit images): ONE body, so both write the same ray bits for the same poses, intrinsics and indices.
#pragma once
#include "pnr_common.h"

namespace pnr {

struct BatchCams {                                      // what every row of a batch shares
    const float* poses;                                 // (SB, NV, 4, 4) c2w
    const float* focal;                                 // (SB, 2)
    const float* c;                                     // (SB, 2) or NULL = (W/2, H/2)
    int NV, W, H;
    float z_near, z_far;
};

// Row (o, idx): idx = view * H * W + pixel.  In range -> r = [pose[:3, 3], pinhole_ray, z_near, z_far] (the RayCam built here
// from the pose row: bit-identical to k_gen_rays for the same camera and pixel), view / pix set, true.  An index outside
// [0, NV*H*W) reads nothing, leaves r all NaN and returns false.  NV * H * W < 2^31 (checked by the entry points).
__device__ __forceinline__ bool batch_ray(const BatchCams& b, int64_t o, int64_t idx, float* r /* 8 */, int& view, int& pix) {
    const int HW = b.H * b.W;
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = nan;
    if (idx < 0 || idx >= (int64_t)b.NV * HW) return false;
    view = (int)idx / HW;
    pix = (int)idx - view * HW;
    const float* P = b.poses + (o * b.NV + view) * 16;
    RayCam cam;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cam.R[a * 3 + 0] = P[a * 4 + 0]; cam.R[a * 3 + 1] = P[a * 4 + 1]; cam.R[a * 3 + 2] = P[a * 4 + 2];
        cam.o[a] = P[a * 4 + 3];
    }
    cam.fx = b.focal[o * 2]; cam.fy = b.focal[o * 2 + 1];
    cam.cx = b.c ? b.c[o * 2] : (float)b.W * 0.5f;
    cam.cy = b.c ? b.c[o * 2 + 1] : (float)b.H * 0.5f;
    cam.zn = b.z_near; cam.zf = b.z_far; cam.W = b.W; cam.H = b.H;
    r[0] = cam.o[0]; r[1] = cam.o[1]; r[2] = cam.o[2];
    pinhole_ray(cam, pix, r + 3);
    r[6] = cam.zn; r[7] = cam.zf;
    return true;
}

// One 16-byte store.  A vector-typed store stays ONE instruction; a float4 struct assignment is split into four scalar stores
// early, and where a scalar route beside it stores the same values the two get merged into dword stores.
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_f32x4(float* p /* 16-byte aligned */, float a, float b, float c, float d) {
    *(f32x4*)p = f32x4{a, b, c, d};
}

// row i of rays_out (.., 8) and, when asked for, of rgb_out (.., 3)
__device__ __forceinline__ void batch_store(float* __restrict__ rays_out, float* __restrict__ rgb_out, int64_t i, const float* r,
                                            const float* g) {
    float* ro = rays_out + i * 8;
    if ((((uintptr_t)rays_out) & 15) == 0) {            // 32-byte rows: two 16-byte stores
        store_f32x4(ro, r[0], r[1], r[2], r[3]);
        store_f32x4(ro + 4, r[4], r[5], r[6], r[7]);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) ro[k] = r[k];
    }
    if (rgb_out) {
        float* go = rgb_out + i * 3;
        go[0] = g[0]; go[1] = g[1]; go[2] = g[2];
    }
}

// the size conditions pnr_train_batch and pnr_train_batch_u8 share
static inline bool batch_shape_ok(int32_t SB, int32_t NV, int32_t W, int32_t H, int64_t B) {
    if (SB <= 0 || NV <= 0 || W <= 0 || H <= 0 || B < 0 || (int64_t)NV * H * W >= ((int64_t)1 << 31)) return false;
    return B <= (((int64_t)1 << 39) / SB);              // SB * B / 256 workgroups fit the grid
}

}  // namespace pnr
