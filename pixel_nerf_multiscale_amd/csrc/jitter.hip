// Colour-jitter augmentation where the bytes lie (include/pnr.h, "colour jitter"): pnr_color_jitter_plan draws one record per
// object from the step's key — four factors and the order of the four operations — and, where contrast takes part, reduces the
// object's grey mean over ALL its views, so that every view of an object goes through one colour map.  The two gathers of the
// data layer then apply the record to what a step uses only: the sampled pixels and the chosen source views (data_u8.h, the
// kernels of pnr_train_batch_u8 / pnr_views_to_tensor_u8 with the chain of jitter.h switched on).
// The reduction reads every byte of the batch once (bandwidth-bound: 3 bytes per pixel); the sum is fp64 in an order the launch
// shape fixes — a thread's pixels in ascending order, the workgroup's LDS tree, the partials of an object the same way — with no
// atomics, so the same bytes give the same bits.
#include "data_u8.h"

namespace pnr {

enum { DRAW_JITTER = 10 };                              // 0..3 the render samplers', 8 and 9 the training draws' (train_draw.hip)
constexpr int JB_THREADS = 256;
constexpr int JB_ITERS = PNR_JITTER_BLOCK / (JB_THREADS * VT_PIX);
static_assert(JB_ITERS * JB_THREADS * VT_PIX == PNR_JITTER_BLOCK, "a workgroup covers PNR_JITTER_BLOCK pixels in whole rounds");

struct JitterRanges { float v[4]; };                    // brightness, contrast, saturation, hue

// lo + (hi - lo) u with lo, hi = centre -+ range, every operation rounded on its own
__device__ __forceinline__ float jitter_factor(float centre, float range, uint32_t word) {
    const float lo = jsub(centre, range), hi = jadd(centre, range);
    return jadd(lo, jmul(jsub(hi, lo), u01(word)));
}

// Object o's draw: block 0 holds the four factors' words, word 0 of block 1 the order.  mean is left 0.
__device__ __forceinline__ JitterRec jitter_draw(uint64_t seed, int64_t o, const JitterRanges& rg, uint32_t& code) {
    const u32x4 a = philox4x32(seed, (uint32_t)o, (uint32_t)((uint64_t)o >> 32), DRAW_JITTER, 0u);
    const u32x4 b = philox4x32(seed, (uint32_t)o, (uint32_t)((uint64_t)o >> 32), DRAW_JITTER, 1u);
    code = __umulhi(b.x, 24u);
    return {jitter_factor(1.0f, rg.v[0], a.x), jitter_factor(1.0f, rg.v[1], a.y), jitter_factor(1.0f, rg.v[2], a.z),
            jitter_factor(0.0f, rg.v[3], a.w), 0.0f, jitter_order(code)};
}

// Workgroup b: object b / nblk, pixels [PNR_JITTER_BLOCK c, PNR_JITTER_BLOCK (c + 1)) of its NV H W, c = b % nblk.  Round `it`
// gives thread t the pixels [4 g, 4 g + 4), g = 256 it + t; the loads are load_pixels_u8's (whole dwords when the object's first
// byte is dword-aligned and the group is whole, else byte by byte: only bytes of this object are touched).  An object whose
// contrast factor is exactly 1 needs no mean: its workgroups leave at once and their partials are never read.  obj_base: the
// call's object o draws with the counter of object obj_base + o of the step; bytes, partials and records stay the call's rows.
__global__ void __launch_bounds__(JB_THREADS) k_jitter_partials(const uint8_t* __restrict__ images, int64_t npix, int C, int nblk,
                                                                JitterRanges rg, uint64_t seed, int64_t obj_base,
                                                                double* __restrict__ partials) {
    __shared__ double s[JB_THREADS];
    const int64_t o = blockIdx.x / (unsigned)nblk;
    const int64_t first = (int64_t)(blockIdx.x - (unsigned)o * (unsigned)nblk) * PNR_JITTER_BLOCK;
    uint32_t code;
    const JitterRec rec = jitter_draw(seed, obj_base + o, rg, code);
    if (rec.contrast == 1.0f) return;                   // the whole workgroup: the draw depends on o alone
    const uint8_t* obj = images + o * npix * C;
    const bool aligned = (((uintptr_t)obj) & 3) == 0;
    double acc = 0.0;
    for (int it = 0; it < JB_ITERS; ++it) {
        const int64_t p0 = first + ((int64_t)it * JB_THREADS + threadIdx.x) * VT_PIX;
        if (p0 >= npix) break;
        const int np = npix - p0 < VT_PIX ? (int)(npix - p0) : VT_PIX;
        uint32_t b[3][VT_PIX];
        load_pixels_u8(obj + p0 * C, np, C, aligned && np == VT_PIX, b);
#pragma unroll
        for (int q = 0; q < VT_PIX; ++q) {
            if (q < np) {
                float x[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) x[k] = u8_to_tensor(b[k][q], 0);
                jitter_chain<true>(rec, x[0], x[1], x[2]);
                acc += (double)jitter_gray(x[0], x[1], x[2]);
            }
        }
    }
    s[threadIdx.x] = acc;
    block_fold<JB_THREADS>(threadIdx.x, [&](int i, int j) { s[i] += s[j]; });
    if (threadIdx.x == 0) partials[blockIdx.x] = s[0];
}

// Workgroup o writes object o's record; with partials it folds the object's nblk of them first (thread t adds partials t,
// t + 256, .. in that order, then the LDS tree), divides by the pixel count in fp64 and rounds ONCE to fp32.
__global__ void __launch_bounds__(JB_THREADS) k_jitter_record(JitterRanges rg, uint64_t seed, int64_t obj_base,
                                                              const double* __restrict__ partials, int nblk, int64_t npix,
                                                              float* __restrict__ record_out) {
    __shared__ double s[JB_THREADS];
    const int64_t o = blockIdx.x;
    uint32_t code;
    JitterRec rec = jitter_draw(seed, obj_base + o, rg, code);
    if (partials && rec.contrast != 1.0f) {             // the whole workgroup
        double acc = 0.0;
        for (int k = threadIdx.x; k < nblk; k += JB_THREADS) acc += partials[o * nblk + k];
        s[threadIdx.x] = acc;
        block_fold<JB_THREADS>(threadIdx.x, [&](int i, int j) { s[i] += s[j]; });
        rec.mean = (float)(s[0] / (double)npix);
    }
    if (threadIdx.x == 0) {
        float* row = record_out + o * 8;
        row[0] = rec.brightness; row[1] = rec.contrast; row[2] = rec.saturation; row[3] = rec.hue;
        row[4] = rec.mean; row[5] = (float)code; row[6] = 0.0f; row[7] = 0.0f;
    }
}

static inline int64_t jitter_blocks(int32_t NV, int32_t W, int32_t H) {
    return ((int64_t)NV * H * W + PNR_JITTER_BLOCK - 1) / PNR_JITTER_BLOCK;
}
// the plan's workspace: one fp64 partial per (object, block of PNR_JITTER_BLOCK pixels)
static inline double* jitter_carve(Bump& ws, int32_t SB, int32_t NV, int32_t W, int32_t H) {
    return ws.take<double>((uint64_t)SB * (uint64_t)jitter_blocks(NV, W, H), 8);
}

}  // namespace pnr

using namespace pnr;

extern "C" uint64_t pnr_color_jitter_workspace_bytes(int32_t SB, int32_t NV, int32_t W, int32_t H) {
    if (!batch_shape_ok(SB, NV, W, H, 0)) return 0;
    return bytes_of([&](Bump& b) { jitter_carve(b, SB, NV, W, H); });
}

extern "C" int32_t pnr_color_jitter_plan_at(const uint8_t* images_u8, int32_t SB, int32_t NV, int32_t W, int32_t H, int32_t C,
                                            const float* ranges, uint64_t seed, int64_t obj_base, float* record_out, void* workspace,
                                            uint64_t ws_bytes, void* stream) {
    if (!ranges || !record_out) return PNR_E_NULL;
    JitterRanges rg;
    for (int k = 0; k < 4; ++k) {
        rg.v[k] = ranges[k];
        if (!(rg.v[k] >= 0.0f && rg.v[k] <= (k == 3 ? 0.5f : 1.0f))) return PNR_E_SHAPE;      // NaN fails too
    }
    if ((C != 3 && C != 4) || !batch_shape_ok(SB, NV, W, H, 0)) return PNR_E_SHAPE;
    if (obj_base < 0 || obj_base > 0x7fffffffffffffffLL - SB) return PNR_E_SHAPE;           // the last counter stays inside int64
    const bool reduce = rg.v[1] != 0.0f;                // a contrast range of 0: every factor is exactly 1, no mean is needed
    const int64_t nblk = jitter_blocks(NV, W, H), npix = (int64_t)NV * H * W;
    double* partials = nullptr;
    if (reduce) {
        if (!images_u8 || !workspace) return PNR_E_NULL;
        if (((uintptr_t)workspace & 7) != 0) return PNR_E_ALIGN;
        if (ws_bytes < pnr_color_jitter_workspace_bytes(SB, NV, W, H)) return PNR_E_WORKSPACE;
        if ((int64_t)SB > (((int64_t)1 << 31) - 1) / nblk) return PNR_E_SHAPE;                 // one launch: the grid's x extent
        Bump ws(workspace);
        partials = jitter_carve(ws, SB, NV, W, H);
        hipLaunchKernelGGL(k_jitter_partials, dim3((unsigned)(SB * nblk)), dim3(JB_THREADS), 0, (hipStream_t)stream, images_u8, npix, C,
                           (int)nblk, rg, seed, obj_base, partials);
        PNR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_jitter_record, dim3((unsigned)SB), dim3(JB_THREADS), 0, (hipStream_t)stream, rg, seed, obj_base,
                       (const double*)partials, (int)nblk, npix, record_out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_color_jitter_plan(const uint8_t* images_u8, int32_t SB, int32_t NV, int32_t W, int32_t H, int32_t C,
                                         const float* ranges, uint64_t seed, float* record_out, void* workspace, uint64_t ws_bytes,
                                         void* stream) {
    return pnr_color_jitter_plan_at(images_u8, SB, NV, W, H, C, ranges, seed, 0, record_out, workspace, ws_bytes, stream);
}

extern "C" int32_t pnr_train_batch_u8_jitter(const uint8_t* images_u8, const float* poses, const float* focal, const float* c,
                                             int32_t SB, int32_t NV, int32_t W, int32_t H, float z_near, float z_far,
                                             const int64_t* pix_inds, int64_t B, float* rays_out, float* rgb_gt_out, int32_t C,
                                             int32_t balanced, const float* jitter, void* stream) {
    return launch_train_batch_u8<true>(images_u8, poses, focal, c, SB, NV, W, H, z_near, z_far, pix_inds, B, rays_out, rgb_gt_out, C,
                                       balanced, jitter, stream);
}

extern "C" int32_t pnr_views_to_tensor_u8_jitter(const uint8_t* images_u8, const int64_t* view_ord, int32_t SB, int32_t NV,
                                                 int32_t NS, int32_t W, int32_t H, int32_t C, int32_t balanced, float* out,
                                                 const float* jitter, void* stream) {
    return launch_views_to_tensor_u8<true>(images_u8, view_ord, SB, NV, NS, W, H, C, balanced, jitter, out, stream);
}
