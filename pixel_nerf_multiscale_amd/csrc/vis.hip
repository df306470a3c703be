// The picture a pixelNeRF run is judged by (reference train/train.py:423-537, vis_step) and the colour map behind it
// (src/util/util.py:13-30, image_float_to_uint8 + a 256-entry table), where the render left its outputs: per pass one row
// [source views | ground truth | cmap(depth) | rgb | cmap(opacity)], plus the mean squared error behind the view's PSNR.
// A whole-frame minimum has to exist before any byte can, so each entry point is three launches on the caller's stream:
// per-tile partials, ONE workgroup that folds them in tile order, the writer.  include/pnr.h fixes the arithmetic.
// Latency-bound: a 128 x 128 view is 64 workgroups; the point is that nothing is copied to the host and nothing waits.
#include "frame_common.h"

namespace pnr {

constexpr uint64_t VS_RECORD_BYTES = 64;           // the fold's record at the head of the workspace (up to 8 floats)

// min / max as np.min / np.max: a NaN on either side is the answer
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

// image_float_to_uint8 for one element: (x - vmin) / (vmax - vmin), one product with 255, truncation; not finite -> 0
__device__ __forceinline__ uint8_t quant_map(float x, float vmin, float den) {
    const float p = __fmul_rn(__fdiv_rn(__fsub_rn(x, vmin), den), 255.0f);
    return __builtin_isfinite(p) ? (uint8_t)(int)p : (uint8_t)0;
}
// `if vmax - vmin < 1e-10: vmax += 1e-10`: the difference in fp32, the comparison and the sum in fp64, one rounding back
__device__ __forceinline__ float widen_vmax(float vmin, float vmax) {
    return (double)__fsub_rn(vmax, vmin) < 1e-10 ? (float)((double)vmax + 1e-10) : vmax;
}

// (min, max) over the workgroup into red[0][0], red[1][0]; the caller syncs before it reuses `red`
__device__ __forceinline__ void block_minmax(float lo, float hi, float (*red)[FRAME_THREADS], int tid) {
    red[0][tid] = lo;
    red[1][tid] = hi;
    block_fold<FRAME_THREADS>(tid, [red](int i, int j) {
        red[0][i] = nan_min(red[0][i], red[0][j]); red[1][i] = nan_max(red[1][i], red[1][j]);
    });
}
// sum over the workgroup (block_fold); the caller syncs before it reuses `red`
__device__ __forceinline__ double block_sum(double a, double* red, int tid) {
    red[tid] = a;
    block_fold<FRAME_THREADS>(tid, [red](int i, int j) { red[i] += red[j]; });
    return red[0];
}

// ------------------------------------------------------------------------------------------------------------ pnr_cmap
// per tile: (min, max) of the map -> part[2 tile], part[2 tile + 1]
__global__ void __launch_bounds__(FRAME_THREADS) k_cmap_reduce(const float* __restrict__ map, int stride, int W, int H, int tiles_x,
                                                               float* __restrict__ part) {
    __shared__ float red[2][FRAME_THREADS];
    const int tid = threadIdx.x;
    const auto [gx, gy] = tile_pixel((int)blockIdx.x, tiles_x, tid);
    float lo = INFINITY, hi = -INFINITY;
    if (gx < W && gy < H) lo = hi = map[((int64_t)gy * W + gx) * stride];
    block_minmax(lo, hi, red, tid);
    if (tid == 0) { part[2 * (int64_t)blockIdx.x] = red[0][0]; part[2 * (int64_t)blockIdx.x + 1] = red[1][0]; }
}

// ONE workgroup: thread t folds the tiles t, t + 256, .. in ascending order.  record = (vmin, widened vmax)
__global__ void __launch_bounds__(FRAME_THREADS) k_cmap_fold(const float* __restrict__ part, int tiles, float* __restrict__ record,
                                                             float* __restrict__ minmax) {
    __shared__ float red[2][FRAME_THREADS];
    const int tid = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    for (int t = tid; t < tiles; t += FRAME_THREADS) { lo = nan_min(lo, part[2 * (int64_t)t]); hi = nan_max(hi, part[2 * (int64_t)t + 1]); }
    block_minmax(lo, hi, red, tid);
    if (tid == 0) {
        lo = red[0][0];
        hi = red[1][0];
        if (minmax) { minmax[0] = lo; minmax[1] = hi; }
        record[0] = lo;
        record[1] = widen_vmax(lo, hi);
    }
}

__global__ void __launch_bounds__(FRAME_THREADS) k_cmap_write(const float* __restrict__ map, int stride, int W, int H, int tiles_x,
                                                              const uint8_t* __restrict__ lut, const float* __restrict__ record,
                                                              uint8_t* __restrict__ out) {
    const int tid = threadIdx.x;
    const auto [gx, gy] = tile_pixel((int)blockIdx.x, tiles_x, tid);
    if (gx >= W || gy >= H) return;
    const float vmin = record[0], den = __fsub_rn(record[1], vmin);
    const int64_t pix = (int64_t)gy * W + gx;
    const int b = quant_map(map[pix * stride], vmin, den);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[pix * 3 + c] = lut[b * 3 + c];
}

// ------------------------------------------------------------------------------------------------------- pnr_vis_panel
struct VisPass {
    const float* rgb; const float* depth; const float* weights;
    int rgb_stride, depth_stride, weights_stride, K;
};
struct VisArgs {
    const float* images;
    VisPass pass[2];
    int src[PNR_VIS_MAX_SRC];
    int NS, gt_view, n_pass, W, H, tiles_x, tiles;
    const uint8_t* lut;
    float* panel_f32; uint8_t* panel_u8; float* alpha_out; float* stats; double* mse;
    float* record;        // workspace: n_pass x (alpha vmin, alpha widened vmax, depth vmin, depth widened vmax)
    double* se_part;      // (tiles): squared-error sum of the tile
    float* mm_part;       // (n_pass, tiles, 6): rgb min max, alpha min max, depth min max of the tile
    float* alpha_ws;      // (n_pass, H*W)
};

// Launch one, a workgroup per 16 x 16 pixel tile: the opacity of every pass (fp64 sum in ascending k, one rounding), the tile's
// partial extrema and, from the last pass's colours against the ground-truth tile, its squared-error sum.
__global__ void __launch_bounds__(FRAME_THREADS) k_vis_reduce(VisArgs a) {
    __shared__ float red[2][FRAME_THREADS];
    __shared__ double dred[FRAME_THREADS];
    const int tid = threadIdx.x;
    const auto [gx, gy] = tile_pixel((int)blockIdx.x, a.tiles_x, tid);
    const bool inside = gx < a.W && gy < a.H;
    const int64_t HW = (int64_t)a.W * a.H, pix = (int64_t)gy * a.W + gx;

    for (int p = 0; p < a.n_pass; ++p) {
        const VisPass& ps = a.pass[p];
        float v[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
        if (inside) {
            const float* c = ps.rgb + pix * ps.rgb_stride;
            v[0] = nan_min(nan_min(c[0], c[1]), c[2]);
            v[1] = nan_max(nan_max(c[0], c[1]), c[2]);
            const float* w = ps.weights + pix * ps.weights_stride;
            double s = 0.0;
            for (int k = 0; k < ps.K; ++k) s += (double)w[k];
            const float al = (float)s;
            a.alpha_ws[p * HW + pix] = al;
            if (a.alpha_out) a.alpha_out[p * HW + pix] = al;
            v[2] = v[3] = al;
            v[4] = v[5] = ps.depth[pix * ps.depth_stride];
        }
        float* out = a.mm_part + ((int64_t)p * a.tiles + blockIdx.x) * 6;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            block_minmax(v[2 * q], v[2 * q + 1], red, tid);
            if (tid == 0) { out[2 * q] = red[0][0]; out[2 * q + 1] = red[1][0]; }
            __syncthreads();
        }
    }
    if (!a.mse) return;                                                    // uniform over the launch
    double se = 0.0;
    if (inside) {
        const VisPass& ps = a.pass[a.n_pass - 1];
        const float* c = ps.rgb + pix * ps.rgb_stride;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float g = fmaf(a.images[((int64_t)a.gt_view * 3 + ch) * HW + pix], 0.5f, 0.5f);
            const double d = (double)c[ch] - (double)g;
            se = __dadd_rn(se, __dmul_rn(d, d));                          // the square rounded on its own, as the header states it
        }
    }
    se = block_sum(se, dred, tid);
    if (tid == 0) a.se_part[blockIdx.x] = se;
}

// Launch two, ONE workgroup: thread t folds the tiles t, t + 256, .. in ascending order, then the tree — no atomics, the same
// inputs give the same bits.
__global__ void __launch_bounds__(FRAME_THREADS) k_vis_fold(VisArgs a) {
    __shared__ float red[2][FRAME_THREADS];
    __shared__ double dred[FRAME_THREADS];
    const int tid = threadIdx.x;
    for (int p = 0; p < a.n_pass; ++p) {
        const float* part = a.mm_part + (int64_t)p * a.tiles * 6;
        float m[6];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float lo = INFINITY, hi = -INFINITY;
            for (int t = tid; t < a.tiles; t += FRAME_THREADS) {
                lo = nan_min(lo, part[(int64_t)t * 6 + 2 * q]);
                hi = nan_max(hi, part[(int64_t)t * 6 + 2 * q + 1]);
            }
            block_minmax(lo, hi, red, tid);
            m[2 * q] = red[0][0];
            m[2 * q + 1] = red[1][0];
            __syncthreads();
        }
        if (tid == 0) {
            if (a.stats) {
#pragma unroll
                for (int q = 0; q < 6; ++q) a.stats[p * 6 + q] = m[q];
            }
            a.record[p * 4 + 0] = m[2];
            a.record[p * 4 + 1] = widen_vmax(m[2], m[3]);
            a.record[p * 4 + 2] = m[4];
            a.record[p * 4 + 3] = widen_vmax(m[4], m[5]);
        }
    }
    if (!a.mse) return;
    double se = 0.0;
    for (int t = tid; t < a.tiles; t += FRAME_THREADS) se += a.se_part[t];
    se = block_sum(se, dred, tid);
    if (tid == 0) *a.mse = se / (3.0 * (double)a.W * (double)a.H);
}

// Launch three, a workgroup per (pixel tile, panel column, pass): every thread writes the three channels of one panel pixel.
__global__ void __launch_bounds__(FRAME_THREADS) k_vis_write(VisArgs a) {
    const int tid = threadIdx.x;
    const auto [gx, gy] = tile_pixel((int)blockIdx.x, a.tiles_x, tid);
    if (gx >= a.W || gy >= a.H) return;
    const int col = blockIdx.y, p = blockIdx.z, NS = a.NS;
    const int64_t HW = (int64_t)a.W * a.H, pix = (int64_t)gy * a.W + gx;
    const VisPass& ps = a.pass[p];
    float v[3];
    if (col <= NS) {                                                       // a source view, or the ground truth at col == NS
        const int view = col < NS ? a.src[col] : a.gt_view;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = fmaf(a.images[((int64_t)view * 3 + c) * HW + pix], 0.5f, 0.5f);
    } else if (col == NS + 2) {
        const float* c = ps.rgb + pix * ps.rgb_stride;
        v[0] = c[0]; v[1] = c[1]; v[2] = c[2];
    } else {
        const bool is_depth = col == NS + 1;
        const float* rec = a.record + p * 4 + (is_depth ? 2 : 0);
        const float x = is_depth ? ps.depth[pix * ps.depth_stride] : a.alpha_ws[p * HW + pix];
        const int b = quant_map(x, rec[0], __fsub_rn(rec[1], rec[0]));
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn((float)a.lut[b * 3 + c], 255.0f);
    }
    const int64_t at = ((((int64_t)p * a.H + gy) * (NS + 4) + col) * a.W + gx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.panel_f32) a.panel_f32[at + c] = v[c];
        if (a.panel_u8) a.panel_u8[at + c] = quant_u8(clamp01(v[c]));
    }
}

}  // namespace pnr

using namespace pnr;

// pnr_cmap's workspace: the fold's record | (min, max) partials of every tile
struct CmapWs { float* record; float* part; };
static CmapWs carve_cmap(Bump& b, int W, int H) {
    CmapWs w;
    w.record = b.take<float>(VS_RECORD_BYTES / sizeof(float));
    w.part = b.take<float>((uint64_t)frame_tiles(W, H) * 2);
    return w;
}
extern "C" uint64_t pnr_cmap_workspace_bytes(int32_t W, int32_t H) {
    if (!frame_shape_ok(W, H)) return 0;
    return bytes_of([&](Bump& b) { carve_cmap(b, W, H); });
}

extern "C" int32_t pnr_cmap(const float* map, int32_t stride, int32_t W, int32_t H, const uint8_t* lut, uint8_t* out_u8,
                            float* minmax, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!map || !out_u8 || !lut || !workspace) return PNR_E_NULL;
    if (((uintptr_t)workspace & 3) != 0) return PNR_E_ALIGN;
    if (!frame_shape_ok(W, H)) return PNR_E_SHAPE;
    if (stride == 0) stride = 1;
    if (stride < 1) return PNR_E_SHAPE;
    Bump bump(workspace);
    const CmapWs ws = carve_cmap(bump, W, H);
    if (workspace_bytes < bump.off) return PNR_E_WORKSPACE;
    const int tiles = (int)frame_tiles(W, H), tiles_x = frame_tiles_x(W);
    float *record = ws.record, *part = ws.part;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_cmap_reduce, dim3((unsigned)tiles), dim3(FRAME_THREADS), 0, s, map, stride, W, H, tiles_x, part);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cmap_fold, dim3(1), dim3(FRAME_THREADS), 0, s, (const float*)part, tiles, record, minmax);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cmap_write, dim3((unsigned)tiles), dim3(FRAME_THREADS), 0, s, map, stride, W, H, tiles_x, lut,
                       (const float*)record, out_u8);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

// workspace: record (64 bytes) | squared-error partials (tiles doubles) | extrema partials (n_pass, tiles, 6) | alpha (n_pass, H W)
struct VisWs { float* record; double* se_part; float* mm_part; float* alpha; };
static VisWs carve_vis(Bump& b, int W, int H, int n_pass) {
    const uint64_t tiles = (uint64_t)frame_tiles(W, H);
    VisWs w;
    w.record = b.take<float>(VS_RECORD_BYTES / sizeof(float));
    w.se_part = b.take<double>(tiles);
    w.mm_part = b.take<float>((uint64_t)n_pass * tiles * 6);
    w.alpha = b.take<float>((uint64_t)n_pass * (uint64_t)W * (uint64_t)H);
    return w;
}
extern "C" uint64_t pnr_vis_panel_workspace_bytes(int32_t W, int32_t H, int32_t n_pass) {
    if (!frame_shape_ok(W, H) || n_pass < 1 || n_pass > 2) return 0;
    return bytes_of([&](Bump& b) { carve_vis(b, W, H, n_pass); });
}

extern "C" int32_t pnr_vis_panel(const float* images, int32_t NV, const int32_t* src_views, int32_t NS, int32_t gt_view,
                                 const pnr_vis_pass* passes, int32_t n_pass, int32_t W, int32_t H, const uint8_t* lut,
                                 float* panel_f32, uint8_t* panel_u8, float* alpha, float* stats, double* mse, void* workspace,
                                 uint64_t workspace_bytes, void* stream) {
    if (!images || !src_views || !passes || !lut) return PNR_E_NULL;
    if (n_pass < 1 || n_pass > 2) return PNR_E_SHAPE;
    for (int p = 0; p < n_pass; ++p)
        if (!passes[p].rgb || !passes[p].depth || !passes[p].weights) return PNR_E_NULL;
    const bool any = panel_f32 || panel_u8 || alpha || stats || mse;
    if (any && !workspace) return PNR_E_NULL;
    if (((uintptr_t)workspace & 7) != 0) return PNR_E_ALIGN;
    if (!frame_shape_ok(W, H)) return PNR_E_SHAPE;
    if (NS < 1 || NS > PNR_VIS_MAX_SRC || NV < 1 || gt_view < 0 || gt_view >= NV) return PNR_E_SHAPE;
    for (int i = 0; i < NS; ++i)
        if (src_views[i] < 0 || src_views[i] >= NV) return PNR_E_SHAPE;
    VisArgs a;
    for (int p = 0; p < n_pass; ++p) {
        const pnr_vis_pass& in = passes[p];
        VisPass& ps = a.pass[p];
        if (in.K < 1) return PNR_E_SHAPE;
        ps.rgb = in.rgb; ps.depth = in.depth; ps.weights = in.weights; ps.K = in.K;
        ps.rgb_stride = in.rgb_stride ? in.rgb_stride : 3;
        ps.depth_stride = in.depth_stride ? in.depth_stride : 1;
        ps.weights_stride = in.weights_stride ? in.weights_stride : in.K;
        if (ps.rgb_stride < 3 || ps.depth_stride < 1 || ps.weights_stride < in.K) return PNR_E_SHAPE;
    }
    if (n_pass == 1) a.pass[1] = a.pass[0];
    if (!any) return PNR_OK;
    Bump bump(workspace);
    const VisWs ws = carve_vis(bump, W, H, n_pass);
    if (workspace_bytes < bump.off) return PNR_E_WORKSPACE;
    const int64_t tiles = frame_tiles(W, H);
    a.images = images;
    for (int i = 0; i < PNR_VIS_MAX_SRC; ++i) a.src[i] = i < NS ? src_views[i] : 0;
    a.NS = NS; a.gt_view = gt_view; a.n_pass = n_pass; a.W = W; a.H = H;
    a.tiles_x = frame_tiles_x(W); a.tiles = (int)tiles;
    a.lut = lut; a.panel_f32 = panel_f32; a.panel_u8 = panel_u8; a.alpha_out = alpha; a.stats = stats; a.mse = mse;
    a.record = ws.record; a.se_part = ws.se_part; a.mm_part = ws.mm_part; a.alpha_ws = ws.alpha;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vis_reduce, dim3((unsigned)tiles), dim3(FRAME_THREADS), 0, s, a);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vis_fold, dim3(1), dim3(FRAME_THREADS), 0, s, a);
    PNR_LAUNCH_CHECK();
    if (panel_f32 || panel_u8) {
        hipLaunchKernelGGL(k_vis_write, dim3((unsigned)tiles, (unsigned)(NS + 4), (unsigned)n_pass), dim3(FRAME_THREADS), 0, s, a);
        PNR_LAUNCH_CHECK();
    }
    return PNR_OK;
}
