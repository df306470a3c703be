// What the training draws share (train_draw.hip: pixels inside boxes; mask_draw.hip: pixels by mask population): the draw ids,
// mulhi, and the source-view walk — ONE body, so both entry points write the same views for the same (seed, object).
#pragma once
#include "train_batch.h"

namespace pnr {

enum { DRAW_PIX = 8, DRAW_VIEWS = 9, DRAW_MASK_PIX = 11 };    // 0..3 are the render samplers' (pnr_common.h), 10 the jitter's
constexpr int DRAW_MAX_NS = 64;

__device__ __forceinline__ uint32_t mulhi(uint32_t x, uint32_t n) { return __umulhi(x, n); }    // (uint64(x) * n) >> 32: in [0, n)

// The NS source views of the step's object `obj` (include/pnr.h, pnr_train_draw) -> view_out[0 .. NS).  The walk keeps its
// chosen views ascending in a 64-entry private array (insertion, NS^2 / 4 moves): NS is a handful in training.
__device__ __forceinline__ void draw_views(uint64_t seed, uint64_t obj, int NV, int NS, int64_t* __restrict__ view_out) {
    int chosen[DRAW_MAX_NS];                             // ascending
    u32x4 r = {0u, 0u, 0u, 0u};
    for (int s = 0; s < NS; ++s) {
        if ((s & 3) == 0) r = philox4x32(seed, (uint32_t)obj, (uint32_t)(obj >> 32), DRAW_VIEWS, (uint32_t)(s >> 2));
        const int w = s & 3;
        const uint32_t word = w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w;
        int t = (int)mulhi(word, (uint32_t)(NV - s));    // the t-th view not chosen yet
        int k = 0;
        while (k < s && t >= chosen[k]) { ++t; ++k; }    // every chosen c <= t (after the steps before it) pushes t by one
        for (int m = s; m > k; --m) chosen[m] = chosen[m - 1];
        chosen[k] = t;
        view_out[s] = t;
    }
}

// the checks pnr_train_draw_at and pnr_train_draw_masked_at share; PNR_OK when a launch may follow
static inline int32_t draw_args_check(int32_t SB, int32_t NV, int32_t W, int32_t H, int64_t B, int32_t NS, int64_t obj_base,
                                      const int64_t* pix_inds_out, const int64_t* view_ord_out) {
    if (NS < 0 || NS > DRAW_MAX_NS || !batch_shape_ok(SB, NV, W, H, B) || NS > NV) return PNR_E_SHAPE;
    if ((B > 0 && !pix_inds_out) || (NS > 0 && !view_ord_out)) return PNR_E_NULL;
    // the last pixel counter, (obj_base + SB) * B - 1, and the last view counter stay inside int64
    constexpr int64_t I64_MAX = 0x7fffffffffffffffLL;
    if (obj_base < 0 || obj_base > I64_MAX - SB || (B > 0 && obj_base + SB > I64_MAX / B)) return PNR_E_SHAPE;
    if (((int64_t)SB * B + SB + 255) / 256 > (((int64_t)1 << 31) - 1)) return PNR_E_SHAPE;      // one launch: the grid's x extent
    return PNR_OK;
}

}  // namespace pnr
