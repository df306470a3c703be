// Mask-weighted training draws on the device (the reference's util.masked_sample, util.py:210-222): a bit table of an object's
// foreground with one row prefix, built once per pool, and the step's pixels drawn from it by population — the first B_inside
// slots of an object from its inside pixels, the rest from its outside pixels, all views pooled.  include/pnr.h fixes the
// arithmetic; everything is integer, there are no atomics, nothing is allocated or read back.
#include "train_draw.h"

namespace pnr {

constexpr int MASK_SCAN = 256;                          // rows per chunk of the prefix scan = its workgroup

// One wave per (row, 64-column segment): the ballot of "byte >= thresh" is the segment's two words, LSB first; a lane past W
// votes 0, so the tail bits are zero.  Grid-stride over the segments, whole waves at a time (the ballot's lanes stay together).
__global__ void __launch_bounds__(256) k_mask_pack(const uint8_t* __restrict__ masks, int64_t n_rows, int W, int Wd, int segs,
                                                   int64_t pix_stride, int thresh, uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t total = n_rows * segs;
    for (int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g < total; g += n_waves) {
        const int64_t row = g / segs;                   // n * R + r: the mask rows of all objects are one run of W pixels each
        const int s = (int)(g - row * segs);
        const int col = s * 64 + lane;
        bool in = false;
        if (col < W) in = (int)masks[(row * W + col) * pix_stride] >= thresh;
        const uint64_t v = __ballot(in);
        if (lane == 0) {
            uint32_t* out = bits + row * Wd + 2 * s;
            out[0] = (uint32_t)v;
            if (2 * s + 1 < Wd) out[1] = (uint32_t)(v >> 32);
        }
    }
}

// One workgroup per object: rows[0] = 0, rows[r + 1] = rows[r] + popcount(row r), R walked in chunks of MASK_SCAN rows — a
// thread counts one row's Wd words, an inclusive scan in LDS orders the chunk, the chunk's total carries into the next.
__global__ void __launch_bounds__(MASK_SCAN) k_mask_rows(const uint32_t* __restrict__ bits, int R, int Wd, uint32_t* __restrict__ rows) {
    __shared__ uint32_t sh[MASK_SCAN];
    const int t = threadIdx.x;
    const uint32_t* b = bits + (int64_t)blockIdx.x * R * Wd;
    uint32_t* out = rows + (int64_t)blockIdx.x * ((int64_t)R + 1);
    uint32_t carry = 0;
    if (t == 0) out[0] = 0;
    for (int r0 = 0; r0 < R; r0 += MASK_SCAN) {
        const int r = r0 + t;
        uint32_t n = 0;
        if (r < R) {
            const uint32_t* w = b + (int64_t)r * Wd;
            for (int k = 0; k < Wd; ++k) n += (uint32_t)__popc(w[k]);
        }
        sh[t] = n;
        __syncthreads();
        for (int d = 1; d < MASK_SCAN; d <<= 1) {
            const uint32_t add = t >= d ? sh[t - d] : 0u;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        if (r < R) out[r + 1] = carry + sh[t];
        carry += sh[MASK_SCAN - 1];
        __syncthreads();                                // sh is rewritten by the next chunk
    }
}

// Work items as in k_train_draw: [0, n_pix) the pixels, [n_pix, n_pix + SB) the views of object i - n_pix.  A pixel reads
// rows[o, 0 .. R] and the Wd words of ONE row r < R of bits[o]; whatever those hold, it reads nothing else: the search keeps
// 0 <= lo < hi <= R, the walk runs over w < Wd.
__global__ void __launch_bounds__(256) k_train_draw_masked(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ rows,
                                                           int SB, int NV, int W, int R, int Wd, int64_t B, int64_t B_inside, int NS,
                                                           uint64_t seed, int64_t obj_base, int64_t n_pix,
                                                           int64_t* __restrict__ pix_out, int64_t* __restrict__ view_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pix) {
        const uint64_t ctr = (uint64_t)(obj_base * B + i);
        const uint32_t x = philox4x32(seed, (uint32_t)ctr, (uint32_t)(ctr >> 32), DRAW_MASK_PIX, 0u).x;
        const int64_t o = i / B;
        const int64_t j = i - o * B;
        const uint32_t* cum = rows + o * ((int64_t)R + 1);
        const uint32_t all = (uint32_t)R * (uint32_t)W;              // NV * H * W < 2^31
        const uint32_t n_in = cum[R];
        int64_t idx = -1;
        if (n_in <= all) {
            const uint32_t n_out = all - n_in;
            bool inside = j < B_inside;
            if (inside ? n_in == 0 : n_out == 0) inside = !inside;  // an empty population: the other one, same x
            const uint32_t k = mulhi(x, inside ? n_in : n_out);
            // the last row with cum[r] <= k: an upper bound over the R + 1 prefix entries (cum[0] = 0 <= k < cum[R])
            int lo = 0, hi = R;
            while (hi - lo > 1) {
                const int mid = lo + ((hi - lo) >> 1);
                const uint32_t c = inside ? cum[mid] : (uint32_t)mid * (uint32_t)W - cum[mid];
                if (c <= k) lo = mid; else hi = mid;
            }
            uint32_t rem = k - (inside ? cum[lo] : (uint32_t)lo * (uint32_t)W - cum[lo]);
            const uint32_t* w = bits + (o * R + lo) * Wd;
            for (int q = 0; q < Wd; ++q) {
                uint32_t word = inside ? w[q] : ~w[q];
                if (q == Wd - 1 && (W & 31)) word &= (1u << (W & 31)) - 1u;      // the tail is no pixel of either population
                const uint32_t c = (uint32_t)__popc(word);
                if (rem < c) {
                    for (uint32_t z = 0; z < rem; ++z) word &= word - 1u;        // drop the rem lowest set bits (rem < 32)
                    idx = (int64_t)lo * W + q * 32 + (__ffs((int)word) - 1);
                    break;
                }
                rem -= c;
            }
        }
        pix_out[i] = idx;
        return;
    }
    const int64_t o = i - n_pix;
    if (NS <= 0 || o >= SB) return;
    draw_views(seed, (uint64_t)(obj_base + o), NV, NS, view_out + o * NS);
}

// One thread per gathered pixel (o, j): the bit of pixel pix_inds[o, j] in bits[o], as 1.0f / 0.0f.  The indices live on the device, so
// the kernel is the range check: an index outside [0, R * W) reads nothing and writes NaN.  row < R and col >> 5 < Wd: the one
// word read lies inside bits[o].
__global__ void __launch_bounds__(256) k_mask_gather(const uint32_t* __restrict__ bits, int W, int R, int Wd, const int64_t* __restrict__ pix_inds,
                                                     int64_t B, int64_t total, float* __restrict__ mask_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int64_t p = pix_inds[i];
    float v = __builtin_nanf("");
    if (p >= 0 && p < (int64_t)R * W) {
        const int64_t o = i / B;
        const int row = (int)(p / W), col = (int)(p - (int64_t)row * W);
        v = (bits[(o * R + row) * Wd + (col >> 5)] >> (col & 31)) & 1u ? 1.0f : 0.0f;
    }
    mask_out[i] = v;
}

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_mask_table_build(const uint8_t* masks_u8, int32_t N, int32_t NV, int32_t H, int32_t W, int64_t pix_stride,
                                        int32_t thresh, uint32_t* bits_out, uint32_t* rows_out, void* stream) {
    if (!masks_u8 || !bits_out || !rows_out) return PNR_E_NULL;
    if (N < 1 || NV < 1 || H < 1 || W < 1 || (int64_t)NV * H * W >= ((int64_t)1 << 31) || pix_stride < 1 || thresh < 1 || thresh > 255)
        return PNR_E_SHAPE;
    if ((((uintptr_t)bits_out) | ((uintptr_t)rows_out)) & 3) return PNR_E_ALIGN;
    const int R = NV * H, Wd = (W + 31) / 32, segs = (W + 63) / 64;
    const int64_t n_rows = (int64_t)N * R;
    const int64_t blocks = (n_rows * segs + 3) / 4;     // 4 waves per workgroup; past the cap the waves stride
    hipLaunchKernelGGL(k_mask_pack, dim3((unsigned)(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, (hipStream_t)stream,
                       masks_u8, n_rows, W, Wd, segs, pix_stride, thresh, bits_out);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mask_rows, dim3((unsigned)N), dim3(MASK_SCAN), 0, (hipStream_t)stream, bits_out, R, Wd, rows_out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_train_draw_masked_at(const uint32_t* bits, const uint32_t* rows, int32_t SB, int32_t NV, int32_t W, int32_t H,
                                            int64_t B, int64_t B_inside, int32_t NS, uint64_t seed, int64_t obj_base,
                                            int64_t* pix_inds_out, int64_t* view_ord_out, void* stream) {
    const int32_t rc = draw_args_check(SB, NV, W, H, B, NS, obj_base, pix_inds_out, view_ord_out);
    if (rc != PNR_OK) return rc;
    if (B_inside < 0 || B_inside > B) return PNR_E_SHAPE;
    if (B > 0 && (!bits || !rows)) return PNR_E_NULL;
    if (B == 0 && NS == 0) return PNR_OK;
    const int64_t n_pix = (int64_t)SB * B;
    const int64_t total = n_pix + SB;
    hipLaunchKernelGGL(k_train_draw_masked, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, rows, SB, NV,
                       W, NV * H, (W + 31) / 32, B, B_inside, NS, seed, obj_base, n_pix, pix_inds_out, view_ord_out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_train_draw_masked(const uint32_t* bits, const uint32_t* rows, int32_t SB, int32_t NV, int32_t W, int32_t H,
                                         int64_t B, int64_t B_inside, int32_t NS, uint64_t seed, int64_t* pix_inds_out,
                                         int64_t* view_ord_out, void* stream) {
    return pnr_train_draw_masked_at(bits, rows, SB, NV, W, H, B, B_inside, NS, seed, 0, pix_inds_out, view_ord_out, stream);
}

extern "C" int32_t pnr_mask_gather(const uint32_t* bits, int32_t SB, int32_t NV, int32_t H, int32_t W, const int64_t* pix_inds, int64_t B,
                                   float* mask_out, void* stream) {
    if (!batch_shape_ok(SB, NV, W, H, B)) return PNR_E_SHAPE;
    if (B > 0 && (!bits || !pix_inds || !mask_out)) return PNR_E_NULL;
    if ((((uintptr_t)bits) | ((uintptr_t)mask_out)) & 3 || (((uintptr_t)pix_inds) & 7)) return PNR_E_ALIGN;
    if (B == 0) return PNR_OK;
    const int64_t total = (int64_t)SB * B;
    hipLaunchKernelGGL(k_mask_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, W, NV * H,
                       (W + 31) / 32, pix_inds, B, total, mask_out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
