// The data layer's two gathers from 8-BIT images, each ONE body for the plain entry points (data.hip, JITTER = false) and for
// the colour-jitter ones (jitter.hip, JITTER = true): a training batch gathered from bytes, and the selected source views of
// such a batch converted to the network's input where they lie.  The images of a split stay on the card as the bytes their
// files hold (3 per pixel instead of 12), so a step uploads its index buffer and nothing else.  include/pnr.h fixes the
// arithmetic: T(b, balanced) is u8_to_tensor (frame_common.h), the rays are batch_ray's (train_batch.h), the colour chain is
// jitter_chain (jitter.h), put between the byte's division by 255 and the balanced map.  With JITTER = false the chain and its
// record are compiled out: the kernels are the ones data.hip held.  Both are latency-bound at training shapes (a batch is
// some thousand rays, a view 48 KiB of bytes).
#pragma once
#include "frame_common.h"
#include "train_batch.h"
#include "jitter.h"                                // last: it switches fp contraction off for what follows

namespace pnr {

constexpr int VT_THREADS = 256;
constexpr int VT_PIX = 4;                          // pixels per thread: 4 C bytes in, one float4 per plane out

// The three colour bytes of one pixel at p: one dword when C = 4 and the address allows it, else three byte loads; a fourth
// channel is stepped over.
__device__ __forceinline__ void load_pixel_u8(const uint8_t* __restrict__ p, int C, uint32_t* b /* 3 */) {
    if (C == 4 && (((uintptr_t)p) & 3) == 0) {
        const uint32_t w = *(const uint32_t*)p;
        b[0] = w & 255u; b[1] = (w >> 8) & 255u; b[2] = (w >> 16) & 255u;
    } else {
        b[0] = p[0]; b[1] = p[1]; b[2] = p[2];
    }
}

// The colour bytes of np <= 4 consecutive pixels at p.  whole_dwords (np == 4 and p dword-aligned): C whole dwords, 12 or 16
// consecutive bytes per lane, a wave reads one contiguous run; else byte by byte, and only bytes of the np pixels are touched
// (the rest of b is 0).  The bytes in b do not depend on the route.
__device__ __forceinline__ void load_pixels_u8(const uint8_t* __restrict__ p, int np, int C, bool whole_dwords,
                                               uint32_t (*b)[VT_PIX] /* [3][VT_PIX] */) {
    if (whole_dwords) {
        const uint32_t* w = (const uint32_t*)p;
        if (C == 3) {
            const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];                  // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            b[0][0] = w0 & 255u;         b[1][0] = (w0 >> 8) & 255u;  b[2][0] = (w0 >> 16) & 255u;
            b[0][1] = w0 >> 24;          b[1][1] = w1 & 255u;         b[2][1] = (w1 >> 8) & 255u;
            b[0][2] = (w1 >> 16) & 255u; b[1][2] = w1 >> 24;          b[2][2] = w2 & 255u;
            b[0][3] = (w2 >> 8) & 255u;  b[1][3] = (w2 >> 16) & 255u; b[2][3] = w2 >> 24;
        } else {
#pragma unroll
            for (int q = 0; q < VT_PIX; ++q) {
                const uint32_t wq = w[q];
                b[0][q] = wq & 255u; b[1][q] = (wq >> 8) & 255u; b[2][q] = (wq >> 16) & 255u;
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < VT_PIX; ++q) {
#pragma unroll
            for (int k = 0; k < 3; ++k) b[k][q] = q < np ? (uint32_t)p[q * C + k] : 0u;
        }
    }
}

// ------------------------------------------------------------------ training batch from bytes
// k_train_batch (stage_kernels.hip) with interleaved bytes (SB, NV, H, W, C) in place of the fp32 planes: one thread per
// sampled ray, the same batch_ray, the colour 0.5 T(b) + 0.5 (one fma: 0.5 T is exact, so it is the product and the sum
// rounded on their own).  A gather of C adjacent bytes per ray.  JITTER: the pixel goes through object o's chain first.
template <bool JITTER>
__global__ void __launch_bounds__(256) k_train_batch_u8(const uint8_t* __restrict__ images, BatchCams cams, int C, int balanced,
                                                        const int64_t* __restrict__ pix_inds, int64_t B, int64_t total,
                                                        const float* __restrict__ jitter /* (SB, 8), JITTER only */,
                                                        float* __restrict__ rays_out, float* __restrict__ rgb_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t o = i / B;
    const int64_t idx = pix_inds[i];
    const float nan = __int_as_float(0x7fc00000);
    float r[8], g[3] = {nan, nan, nan};
    int v, pix;
    if (batch_ray(cams, o, idx, r, v, pix) && rgb_out) {
        const uint8_t* p = images + (o * ((int64_t)cams.NV * cams.H * cams.W) + idx) * C;      // idx = v H W + pix
        uint32_t b[3];
        load_pixel_u8(p, C, b);
        if (JITTER) {
            float x[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = u8_to_tensor(b[k], 0);
            jitter_chain<false>(jitter_load(jitter + o * 8), x[0], x[1], x[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = fmaf(unit_to_tensor(x[k], balanced), 0.5f, 0.5f);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = fmaf(u8_to_tensor(b[k], balanced), 0.5f, 0.5f);
        }
    }
    batch_store(rays_out, rgb_out, i, r, g);
}

// ------------------------------------------------------------------ selected views, bytes -> planes
// Workgroup b serves selected view b / blocks_per_view (= (o, j), o-major) and the pixel groups [256 c, 256 c + 256) of it,
// c = b % blocks_per_view; a thread owns pixels [4 q, 4 q + 4).  The view index comes from the device, so the kernel is the
// range check: outside [0, NV) nothing is read and the three planes are filled with NaN.
// Loads: a whole group of a view whose first byte is dword-aligned is C whole dwords; a view that starts inside a dword (any
// view may: a view is H W C bytes, and the buffer may be a slice of a pool) and the up to 3 pixels behind the last whole group
// are read byte by byte.  Either way only bytes of the selected view are touched.  Stores: a float4 per plane (a wave writes
// 1 KiB rows) when the planes are 16-byte aligned, which needs H W % 4 == 0 under an aligned `out`; else scalar.  The bits do
// not depend on the route: both fill the same bytes b[].  JITTER: every pixel goes through object o's chain.
template <bool JITTER>
__global__ void __launch_bounds__(VT_THREADS) k_views_to_tensor_u8(const uint8_t* __restrict__ images,
                                                                   const int64_t* __restrict__ view_ord, int NV, int NS, int HW,
                                                                   int C, int balanced, int blocks_per_view,
                                                                   const float* __restrict__ jitter /* (SB, 8), JITTER only */,
                                                                   float* __restrict__ out) {
    const int64_t sel = blockIdx.x / (unsigned)blocks_per_view;                  // o * NS + j
    const int chunk = (int)(blockIdx.x - (unsigned)sel * (unsigned)blocks_per_view);
    const int64_t p0 = ((int64_t)chunk * VT_THREADS + threadIdx.x) * VT_PIX;     // may pass 2^31 in the last workgroup: 64 bits
    if (p0 >= HW) return;
    const int np = HW - p0 < VT_PIX ? (int)(HW - p0) : VT_PIX;
    const int64_t o = sel / NS;
    const int64_t v = view_ord[sel];
    const bool live = v >= 0 && v < NV;
    float t[3][VT_PIX];
    if (live) {
        const uint8_t* view = images + (o * NV + v) * ((int64_t)HW * C);
        uint32_t b[3][VT_PIX];
        load_pixels_u8(view + p0 * C, np, C, np == VT_PIX && (((uintptr_t)view) & 3) == 0, b);
        if (JITTER) {
            const JitterRec rec = jitter_load(jitter + o * 8);
#pragma unroll
            for (int q = 0; q < VT_PIX; ++q) {
                float x[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) x[k] = u8_to_tensor(b[k][q], 0);
                jitter_chain<false>(rec, x[0], x[1], x[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) t[k][q] = unit_to_tensor(x[k], balanced);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int q = 0; q < VT_PIX; ++q) t[k][q] = u8_to_tensor(b[k][q], balanced);
            }
        }
    } else {
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int q = 0; q < VT_PIX; ++q) t[k][q] = nan;
        }
    }
    float* dst = out + sel * 3 * (int64_t)HW + p0;
    const bool vec = np == VT_PIX && (HW & 3) == 0 && (((uintptr_t)out) & 15) == 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float* d = dst + (int64_t)k * HW;
        if (vec) {
            store_f32x4(d, t[k][0], t[k][1], t[k][2], t[k][3]);
        } else {
#pragma unroll
            for (int q = 0; q < VT_PIX; ++q)
                if (q < np) d[q] = t[k][q];
        }
    }
}

// ------------------------------------------------------------------ the checks and launches both pairs of entry points share
static inline bool bytes_args_ok(int32_t C, int32_t balanced) { return (C == 3 || C == 4) && (balanced == 0 || balanced == 1); }

template <bool JITTER>
static inline int32_t launch_train_batch_u8(const uint8_t* images_u8, const float* poses, const float* focal, const float* c, int32_t SB,
                                            int32_t NV, int32_t W, int32_t H, float z_near, float z_far, const int64_t* pix_inds,
                                            int64_t B, float* rays_out, float* rgb_gt_out, int32_t C, int32_t balanced,
                                            const float* jitter, void* stream) {
    if (!poses || !focal || !pix_inds || !rays_out || (rgb_gt_out && !images_u8) || (JITTER && !jitter)) return PNR_E_NULL;
    if (!bytes_args_ok(C, balanced) || !batch_shape_ok(SB, NV, W, H, B)) return PNR_E_SHAPE;
    if (B == 0) return PNR_OK;
    const int64_t total = (int64_t)SB * B;
    const BatchCams cams{poses, focal, c, NV, W, H, z_near, z_far};
    hipLaunchKernelGGL(k_train_batch_u8<JITTER>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images_u8,
                       cams, C, balanced, pix_inds, B, total, jitter, rays_out, rgb_gt_out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

template <bool JITTER>
static inline int32_t launch_views_to_tensor_u8(const uint8_t* images_u8, const int64_t* view_ord, int32_t SB, int32_t NV, int32_t NS,
                                                int32_t W, int32_t H, int32_t C, int32_t balanced, const float* jitter, float* out,
                                                void* stream) {
    if (!images_u8 || !view_ord || !out || (JITTER && !jitter)) return PNR_E_NULL;
    if (SB < 1 || NV < 1 || NS < 1 || W < 1 || H < 1 || (int64_t)NV * H * W >= ((int64_t)1 << 31) || !bytes_args_ok(C, balanced))
        return PNR_E_SHAPE;
    if (((uintptr_t)out & 3) != 0) return PNR_E_ALIGN;
    const int HW = W * H;
    const int64_t bpv = ((int64_t)HW + VT_THREADS * VT_PIX - 1) / (VT_THREADS * VT_PIX);       // <= 2^21
    if ((int64_t)SB * NS > (((int64_t)1 << 31) - 1) / bpv) return PNR_E_SHAPE;                 // one launch: the grid's x extent
    hipLaunchKernelGGL(k_views_to_tensor_u8<JITTER>, dim3((unsigned)((int64_t)SB * NS * bpv)), dim3(VT_THREADS), 0,
                       (hipStream_t)stream, images_u8, view_ord, NV, NS, HW, C, balanced, (int)bpv, jitter, out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

}  // namespace pnr
