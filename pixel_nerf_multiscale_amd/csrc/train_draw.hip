// The training step's draws on the device: which pixels a step trains on and which views it encodes, keyed by (seed) — the
// caller's per-step key — instead of drawn on the host from two global generators and uploaded.  include/pnr.h fixes the
// arithmetic (all integer, so a host model pins it bit for bit); the outputs are the index buffers pnr_train_batch /
// pnr_train_batch_u8 / pnr_views_to_tensor_u8 already take.  One launch, latency-bound: a step draws some thousand pixels.
#include "train_draw.h"

namespace pnr {

// A box coordinate: the float truncated towards zero.  NaN, inf and anything at or past +-2^31 cannot be a coordinate
// (W, H < 2^31) and would not survive the conversion: they come back as -1, which the range check below refuses.
__device__ __forceinline__ int box_coord(float f) {
    return (f > -2147483648.0f && f < 2147483648.0f) ? (int)f : -1;
}

// Work items [0, n_pix): pixel (o, j) = i / B, i % B.  Work items [n_pix, n_pix + SB): the NS source views of object i - n_pix
// (when NS > 0; draw_views, train_draw.h).  obj_base: the call's object o is object obj_base + o of the step — it enters the two
// counters and nothing else (boxes and outputs are the call's own rows), so a call over a slice of a batch writes that slice's rows.
__global__ void __launch_bounds__(256) k_train_draw(const float* __restrict__ bbox, int SB, int NV, int W, int H, int64_t B, int NS,
                                                    uint64_t seed, int64_t obj_base, int64_t n_pix, int64_t* __restrict__ pix_out,
                                                    int64_t* __restrict__ view_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pix) {
        const uint64_t ctr = (uint64_t)(obj_base * B + i);
        const u32x4 r = philox4x32(seed, (uint32_t)ctr, (uint32_t)(ctr >> 32), DRAW_PIX, 0u);
        const int64_t o = i / B;
        const int view = (int)mulhi(r.x, (uint32_t)NV);
        int cmin = 0, rmin = 0, cmax = W - 1, rmax = H - 1;
        if (bbox) {
            const float* b = bbox + (o * NV + view) * 4;
            cmin = box_coord(b[0]); rmin = box_coord(b[1]); cmax = box_coord(b[2]); rmax = box_coord(b[3]);
        }
        int64_t idx = -1;
        if (0 <= cmin && cmin <= cmax && cmax < W && 0 <= rmin && rmin <= rmax && rmax < H) {
            const int col = cmin + (int)mulhi(r.y, (uint32_t)(cmax + 1 - cmin));
            const int row = rmin + (int)mulhi(r.z, (uint32_t)(rmax + 1 - rmin));
            idx = (int64_t)view * H * W + (int64_t)row * W + col;
        }
        pix_out[i] = idx;
        return;
    }
    const int64_t o = i - n_pix;
    if (NS <= 0 || o >= SB) return;
    draw_views(seed, (uint64_t)(obj_base + o), NV, NS, view_out + o * NS);
}

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_train_draw_at(const float* bbox, int32_t SB, int32_t NV, int32_t W, int32_t H, int64_t B, int32_t NS,
                                     uint64_t seed, int64_t obj_base, int64_t* pix_inds_out, int64_t* view_ord_out, void* stream) {
    const int32_t rc = draw_args_check(SB, NV, W, H, B, NS, obj_base, pix_inds_out, view_ord_out);
    if (rc != PNR_OK) return rc;
    if (B == 0 && NS == 0) return PNR_OK;
    const int64_t n_pix = (int64_t)SB * B;
    const int64_t total = n_pix + SB;
    hipLaunchKernelGGL(k_train_draw, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bbox, SB, NV, W, H, B, NS,
                       seed, obj_base, n_pix, pix_inds_out, view_ord_out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_train_draw(const float* bbox, int32_t SB, int32_t NV, int32_t W, int32_t H, int64_t B, int32_t NS, uint64_t seed,
                                  int64_t* pix_inds_out, int64_t* view_ord_out, void* stream) {
    return pnr_train_draw_at(bbox, SB, NV, W, H, B, NS, seed, 0, pix_inds_out, view_ord_out, stream);
}
