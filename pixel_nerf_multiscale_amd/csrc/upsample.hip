// The tail of upstream pixelNeRF's SpatialEncoder.forward: every encoder level resized to level 0's size (bilinear,
// align_corners=True) and concatenated along the channels into ONE map, and the adjoint of that (include/pnr.h,
// pnr_upsample_concat / pnr_upsample_concat_bwd, fixes the arithmetic):
//   k_upsample_nchw   out   (N, sumC, H0, W0) fp32: a workgroup owns 1024 consecutive pixels of one plane; stores run along W
//   k_upsample_nhwc16 out16 (N, H0, W0, sumC) bf16 / fp16: a workgroup owns 64 pixels x 64 channels; it samples with the lanes
//                     along the pixels (the reads run along W), turns the tile round in LDS and stores 128-byte channel runs
//   k_upsample_bwd    one level's gradient in gather form: a thread owns ONE texel, walks the fine nodes whose taps land on it
//                     in a fixed order and adds the products in fp64 — no floating-point atomics, the same inputs give the
//                     same bits
// All three are bound by memory and by integer address arithmetic; none keeps an intermediate in memory.
#include "pnr_common.h"

// include/pnr.h fixes every operation as a separately rounded fp32 operation: nothing in this file is fused (as in optim.hip).
// The products and sums are written with the plain operators, which this pragma governs; the __fmul_rn / __fadd_rn of the HIP
// headers are plain operators compiled under the default -ffp-contract=fast, and inlined here they fuse into an fma.
#pragma clang fp contract(off)

namespace pnr {

constexpr int UPS_THREADS = 256;                          // 4 waves
constexpr int UPS_PER_THREAD = 4;                         // pixels of one thread of k_upsample_nchw
constexpr int UPS_CHUNK = UPS_THREADS * UPS_PER_THREAD;   // pixels of one workgroup of k_upsample_nchw
constexpr int UPS_TILE = 64;                              // k_upsample_nhwc16: pixels and channels of one workgroup
constexpr int UPS_TILE_LD = UPS_TILE + 2;                 // 16-bit elements of an LDS row: 33 dwords, so a column walk changes bank
constexpr int UPS_MAX_HW = 32768;                         // D * (n_in - 1) stays inside int32

struct UpsLevels {
    const float* map[PNR_MAX_LEVELS];
    int c0[PNR_MAX_LEVELS + 1];                           // first channel of a level in the concatenation; c0[n] = sumC
    int h[PNR_MAX_LEVELS], w[PNR_MAX_LEVELS];
    int n;
};

// Where fine index D of an axis with n_out samples lies among the n_in coarse ones: taps i0, i1 with weights mu, lam.  The
// position is the exact rational D (n_in - 1) / (n_out - 1); only lam's division and mu's subtraction round.
struct AxisPos { int i0, i1; float lam, mu; };

__device__ __forceinline__ AxisPos axis_pos(int D, int n_in, int n_out) {
    AxisPos p;
    p.i0 = 0;
    p.lam = 0.0f;
    if (n_in > 1 && n_out > 1) {
        const int num = D * (n_in - 1), den = n_out - 1;
        p.i0 = num / den;
        p.lam = __fdiv_rn((float)(num - p.i0 * den), (float)den);
    }
    p.i1 = min(p.i0 + 1, n_in - 1);
    p.mu = 1.0f - p.lam;
    return p;
}

__device__ __forceinline__ float lerp2(float mu, float a, float lam, float b) {
    return mu * a + lam * b;
}

// One output value from one plane (h x w) of a level; a level of the output's own size is copied.
__device__ __forceinline__ float upsample_at(const float* __restrict__ plane, int h, int w, int H0, int W0, int y, int x) {
    if (h == H0 && w == W0) return plane[y * w + x];
    const AxisPos py = axis_pos(y, h, H0), px = axis_pos(x, w, W0);
    const float* r0 = plane + py.i0 * w;
    const float* r1 = plane + py.i1 * w;
    const float top = lerp2(px.mu, r0[px.i0], px.lam, r0[px.i1]);
    const float bot = lerp2(px.mu, r1[px.i0], px.lam, r1[px.i1]);
    return lerp2(py.mu, top, py.lam, bot);
}

__device__ __forceinline__ int level_of(const UpsLevels& L, int c) {
    int l = 0;
    while (l + 1 < L.n && c >= L.c0[l + 1]) ++l;
    return l;
}

// grid = planes (N sumC) x chunks of the plane; everything about the level is uniform over the workgroup
__global__ void __launch_bounds__(UPS_THREADS) k_upsample_nchw(UpsLevels L, int chunks, float* __restrict__ out) {
    const int H0 = L.h[0], W0 = L.w[0], HW = H0 * W0, sumC = L.c0[L.n];
    const int plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
    const int n = plane / sumC, c = plane - n * sumC;
    const int l = level_of(L, c);
    const int h = L.h[l], w = L.w[l];
    const float* src = L.map[l] + ((size_t)n * (L.c0[l + 1] - L.c0[l]) + (c - L.c0[l])) * ((size_t)h * w);
    float* dst = out + (size_t)plane * HW;
#pragma unroll
    for (int j = 0; j < UPS_PER_THREAD; ++j) {
        const int pix = chunk * UPS_CHUNK + j * UPS_THREADS + threadIdx.x;
        if (pix < HW) {
            const int y = pix / W0;
            dst[pix] = upsample_at(src, h, w, H0, W0, y, pix - y * W0);
        }
    }
}

// round to nearest even; a NaN stays a (quiet) NaN
__device__ __forceinline__ uint16_t to_bf16_rne(float v) {
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ uint16_t to_f16_rne(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }

// grid = maps (N) x pixel tiles x channel tiles (sumC % 8 == 0, so a tile's last channel group is whole or absent)
template <bool BF16>
__global__ void __launch_bounds__(UPS_THREADS) k_upsample_nhwc16(UpsLevels L, int pix_tiles, int ch_tiles,
                                                                 uint16_t* __restrict__ out16) {
    __shared__ uint16_t tile[UPS_TILE][UPS_TILE_LD];      // [channel][pixel]
    const int H0 = L.h[0], W0 = L.w[0], HW = H0 * W0, sumC = L.c0[L.n];
    const int ct = blockIdx.x % ch_tiles, pt = (blockIdx.x / ch_tiles) % pix_tiles, n = blockIdx.x / (ch_tiles * pix_tiles);
    const int tid = threadIdx.x;
    {   // sample: lane = pixel, a wave takes 16 channels one after the other (the level is uniform over the wave)
        const int p = tid & (UPS_TILE - 1), pix = pt * UPS_TILE + p;
        const int y = pix / W0, x = pix - y * W0;
        for (int i = 0; i < UPS_TILE / 4; ++i) {
            const int cl = (tid >> 6) * (UPS_TILE / 4) + i, c = ct * UPS_TILE + cl;
            float v = 0.0f;
            if (pix < HW && c < sumC) {
                const int l = level_of(L, c);
                const int h = L.h[l], w = L.w[l];
                const float* src = L.map[l] + ((size_t)n * (L.c0[l + 1] - L.c0[l]) + (c - L.c0[l])) * ((size_t)h * w);
                v = upsample_at(src, h, w, H0, W0, y, x);
            }
            tile[cl][p] = BF16 ? to_bf16_rne(v) : to_f16_rne(v);
        }
    }
    __syncthreads();
    // store: 8 consecutive threads write the 128 bytes of one pixel's 64 channels, 16 bytes each
    const int g = tid & 7;
#pragma unroll
    for (int j = 0; j < UPS_TILE / 32; ++j) {
        const int p = j * 32 + (tid >> 3), pix = pt * UPS_TILE + p;
        const int c = ct * UPS_TILE + g * 8;
        if (pix < HW && c < sumC) {
            uint32_t q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = (uint32_t)tile[g * 8 + 2 * k][p] | ((uint32_t)tile[g * 8 + 2 * k + 1][p] << 16);
            *reinterpret_cast<uint4*>(out16 + ((size_t)n * HW + pix) * sumC + c) = make_uint4(q[0], q[1], q[2], q[3]);
        }
    }
}

// Fine indices D whose taps can land on coarse index i: those with i0 in {i - 1, i}.  A superset is enough — the walk below
// recomputes every node's taps with axis_pos and keeps what lands on i.
__device__ __forceinline__ void support(int i, int n_in, int n_out, int& lo, int& hi) {
    lo = 0;
    hi = n_out - 1;
    if (n_in > 1 && n_out > 1) {
        const int a = n_in - 1, b = n_out - 1;            // i0(D) = floor(D a / b) >= i - 1  <=>  D >= ceil((i - 1) b / a)
        lo = i > 0 ? ((i - 1) * b + a - 1) / a : 0;       // (i - 1) b < 2^30
        hi = min(b, ((i + 1) * b + a - 1) / a);           // i0(D) <= i  <=>  D a < (i + 1) b
    }
}

// d_level (N, C, h, w) = the adjoint of the resize applied to channels [c_first, c_first + C) of d_out (N, sumC, H0, W0).
// A thread owns one texel: fine rows ascending, fine columns ascending inside a row, taps (y0 x0, y0 x1, y1 x0, y1 x1) inside
// a node; w = fl(wy wx) in fp32, the product with the gradient and the sum in fp64 (the product is exact), ONE rounding at
// the end.  Where i0 == i1 both taps land on the same texel and both count.
__global__ void __launch_bounds__(UPS_THREADS) k_upsample_bwd(const float* __restrict__ d_out, int sumC, int H0, int W0,
                                                              int c_first, int C, int h, int w, int total,
                                                              float* __restrict__ d_level) {
    const int e = blockIdx.x * UPS_THREADS + threadIdx.x;
    if (e >= total) return;
    const int x = e % w, y = (e / w) % h, c = (e / (w * h)) % C, n = e / (w * h * C);
    const float* g = d_out + ((size_t)n * sumC + c_first + c) * ((size_t)H0 * W0);
    if (h == H0 && w == W0) {                             // a slice copy (uniform over the launch)
        d_level[e] = g[y * W0 + x];
        return;
    }
    int ylo, yhi, xlo, xhi;
    support(y, h, H0, ylo, yhi);
    support(x, w, W0, xlo, xhi);
    double acc = 0.0;
    for (int Y = ylo; Y <= yhi; ++Y) {
        const AxisPos py = axis_pos(Y, h, H0);
        const bool y0 = py.i0 == y, y1 = py.i1 == y;
        if (!y0 && !y1) continue;
        const float* grow = g + (size_t)Y * W0;
        for (int X = xlo; X <= xhi; ++X) {
            const AxisPos px = axis_pos(X, w, W0);
            const bool x0 = px.i0 == x, x1 = px.i1 == x;
            if (!x0 && !x1) continue;
            const double gv = (double)grow[X];
            if (y0 && x0) acc += (double)(py.mu * px.mu) * gv;
            if (y0 && x1) acc += (double)(py.mu * px.lam) * gv;
            if (y1 && x0) acc += (double)(py.lam * px.mu) * gv;
            if (y1 && x1) acc += (double)(py.lam * px.lam) * gv;
        }
    }
    d_level[e] = (float)acc;
}

// The checks the two entry points share; fills the level table but for the pointers.
static int32_t ups_shapes(const int32_t* lat_c, const int32_t* lat_h, const int32_t* lat_w, int32_t n_levels, int32_t n_maps,
                          UpsLevels& L) {
    if (!lat_c || !lat_h || !lat_w) return PNR_E_NULL;
    if (n_levels < 1 || n_levels > PNR_MAX_LEVELS || n_maps < 0) return PNR_E_SHAPE;
    const int64_t lim = (int64_t)1 << 31;
    int64_t sumC = 0;
    L.n = n_levels;
    for (int l = 0; l < n_levels; ++l) {
        if (lat_c[l] < 1 || lat_h[l] < 1 || lat_w[l] < 1 || lat_h[l] > UPS_MAX_HW || lat_w[l] > UPS_MAX_HW) return PNR_E_SHAPE;
        if ((int64_t)lat_c[l] >= lim) return PNR_E_SHAPE;
        if ((int64_t)n_maps * lat_c[l] >= lim || (int64_t)n_maps * lat_c[l] * lat_h[l] * lat_w[l] >= lim) return PNR_E_SHAPE;
        L.c0[l] = (int)sumC;
        L.h[l] = lat_h[l];
        L.w[l] = lat_w[l];
        sumC += lat_c[l];
        if (sumC >= lim) return PNR_E_SHAPE;
    }
    L.c0[n_levels] = (int)sumC;
    if ((int64_t)n_maps * sumC >= lim || (int64_t)n_maps * sumC * lat_h[0] * lat_w[0] >= lim) return PNR_E_SHAPE;
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_upsample_concat(const float* const* levels, const int32_t* lat_c, const int32_t* lat_h,
                                       const int32_t* lat_w, int32_t n_levels, int32_t n_maps, float* out, void* out16,
                                       int32_t out16_dtype, void* stream) {
    if (!levels) return PNR_E_NULL;
    UpsLevels L;
    PNR_TRY(ups_shapes(lat_c, lat_h, lat_w, n_levels, n_maps, L));
    for (int l = 0; l < n_levels; ++l) {
        if (!levels[l]) return PNR_E_NULL;
        L.map[l] = levels[l];
    }
    if (!out && !out16) return PNR_E_NULL;
    const int sumC = L.c0[n_levels];
    if (out16) {
        if (sumC % 8 != 0) return PNR_E_SHAPE;
        if (out16_dtype != PNR_BF16 && out16_dtype != PNR_F16) return PNR_E_UNSUPPORTED;
        if (((uintptr_t)out16 & 15) != 0) return PNR_E_ALIGN;
    }
    if (n_maps == 0) return PNR_OK;

    hipStream_t s = (hipStream_t)stream;
    const int64_t HW = (int64_t)L.h[0] * L.w[0];
    if (out) {      // planes x chunks <= elements < 2^31
        const int chunks = (int)((HW + UPS_CHUNK - 1) / UPS_CHUNK);
        const int64_t grid = (int64_t)n_maps * sumC * chunks;
        hipLaunchKernelGGL(k_upsample_nchw, dim3((unsigned)grid), dim3(UPS_THREADS), 0, s, L, chunks, out);
        PNR_LAUNCH_CHECK();
    }
    if (out16) {
        const int pix_tiles = (int)((HW + UPS_TILE - 1) / UPS_TILE), ch_tiles = (sumC + UPS_TILE - 1) / UPS_TILE;
        const int64_t grid = (int64_t)n_maps * pix_tiles * ch_tiles;
        if (out16_dtype == PNR_BF16)
            hipLaunchKernelGGL(k_upsample_nhwc16<true>, dim3((unsigned)grid), dim3(UPS_THREADS), 0, s, L, pix_tiles, ch_tiles,
                               (uint16_t*)out16);
        else
            hipLaunchKernelGGL(k_upsample_nhwc16<false>, dim3((unsigned)grid), dim3(UPS_THREADS), 0, s, L, pix_tiles, ch_tiles,
                               (uint16_t*)out16);
        PNR_LAUNCH_CHECK();
    }
    return PNR_OK;
}

extern "C" int32_t pnr_upsample_concat_bwd(const float* d_out, const int32_t* lat_c, const int32_t* lat_h, const int32_t* lat_w,
                                           int32_t n_levels, int32_t n_maps, float* const* d_levels, void* stream) {
    if (!d_out || !d_levels) return PNR_E_NULL;
    UpsLevels L;
    PNR_TRY(ups_shapes(lat_c, lat_h, lat_w, n_levels, n_maps, L));
    if (n_maps == 0) return PNR_OK;
    hipStream_t s = (hipStream_t)stream;
    for (int l = 0; l < n_levels; ++l) {
        if (!d_levels[l]) continue;
        const int C = L.c0[l + 1] - L.c0[l];
        const int total = (int)((int64_t)n_maps * C * L.h[l] * L.w[l]);
        hipLaunchKernelGGL(k_upsample_bwd, dim3((unsigned)((total + UPS_THREADS - 1) / UPS_THREADS)), dim3(UPS_THREADS), 0, s,
                           d_out, L.c0[n_levels], L.h[0], L.w[0], L.c0[l], C, L.h[l], L.w[l], total, d_levels[l]);
        PNR_LAUNCH_CHECK();
    }
    return PNR_OK;
}
