// The back end of the evaluation loop (reference eval/eval.py:286-347) for ONE rendered frame, where it lies on the device:
// clamp, the truncating uint8 quantisation of the PNGs (:301), the render | ground-truth strip (write_compare), the
// normalised depth (:288-289), and the two numbers finish.txt is made of — the mean squared error behind PSNR and the mean
// SSIM (:324-332, as evalio.ssim restates skimage: uniform 7x7 window, sample covariance, whole windows only, per channel).
// Latency-bound: a 128 x 128 frame is 64 workgroups; the point is that nothing waits on the host.
// And the two numbers alone for F frames in one call, clamped or not: the tail of eval/eval_approx.py:136-148 (pnr_eval_frames),
// and for F pairs of 8-bit interleaved frames as a PNG decoder returns them: eval/calc_metrics.py:218-234 (pnr_eval_frames_u8).
#include "frame_common.h"

namespace pnr {

constexpr int EV_HALO = 3;                         // (7 - 1) / 2
constexpr int EV_LDS = FRAME_TILE + 2 * EV_HALO;   // 22
constexpr int EV_WIN = 2 * EV_HALO + 1;            // 7

struct EvalArgs {
    const float* rgb; const float* depth; const float* gt;
    int rgb_stride, depth_stride, W, H, tiles_x;
    float z_near, z_range;
    uint8_t* rgb_u8; uint8_t* compare_u8; float* depth_norm;
    double* part;                                  // (tiles, 2): squared-error sum, SSIM sum of the tile; NULL = no metrics
};

// Sum of (a, b) over the workgroup (block_fold), the same bits in every thread.
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[FRAME_THREADS], int tid) {
    red[0][tid] = a;
    red[1][tid] = b;
    block_fold<FRAME_THREADS>(tid, [red](int i, int j) { red[0][i] += red[0][j]; red[1][i] += red[1][j]; });
    a = red[0][0];
    b = red[1][0];
}

// The tile body k_eval_frame and k_eval_frames share.  Load: the tile at (x0, y0) and a 3-pixel halo of the render x — clamped
// to [0, 1] when `clamp`, as it is otherwise — and of the ground truth g = 0.5 gt + 0.5 go to LDS (all three channels, 11.6 KB).
// gt NULL (k_eval_frame without metrics or compare strip): g = 0.
using EvalTile = float[3][EV_LDS][EV_LDS];
__device__ __forceinline__ void eval_tile_load(const float* rgb, int rgb_stride, const float* gt, int W, int H, int x0, int y0,
                                               bool clamp, EvalTile& sx, EvalTile& sg, int tid) {
    const int64_t HW = (int64_t)W * H;
    for (int i = tid; i < EV_LDS * EV_LDS; i += FRAME_THREADS) {
        const int ly = i / EV_LDS, lx = i % EV_LDS;
        const int gy = y0 - EV_HALO + ly, gx = x0 - EV_HALO + lx;
        float v[3] = {0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};       // outside the image: never part of a whole window
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int64_t pix = (int64_t)gy * W + gx;
            const float* p = rgb + pix * rgb_stride;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = clamp ? clamp01(p[c]) : p[c];
                if (gt) g[c] = fmaf(gt[c * HW + pix], 0.5f, 0.5f);         // the bits of torch's images * 0.5 + 0.5
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { sx[c][ly][lx] = v[c]; sg[c][ly][lx] = g[c]; }
    }
    __syncthreads();
}

// Sums: every thread owns the pixel (x0 + tx, y0 + ty): its squared error and — when the pixel is the centre of a whole window
// — its SSIM term from the 49 taps around it; then the workgroup's (squared-error sum, SSIM sum) in every thread.  The window
// arithmetic is fp64: mean first, then CENTRED second moments (sum (x - mx)(y - my)), so a white background with variances
// around 1e-7 keeps them; the MI355X runs fp64 FMAs at half the fp32 rate, and 2 x 49 taps x 3 channels per pixel are nothing
// next to the render.
__device__ __forceinline__ void eval_tile_sums(const EvalTile& sx, const EvalTile& sg, int W, int H, int x0, int y0,
                                               double (*red)[FRAME_THREADS], int tid, double& se, double& ss) {
    const int tx = tid & (FRAME_TILE - 1), ty = tid / FRAME_TILE;
    const int gy = y0 + ty, gx = x0 + tx;
    const int cy = ty + EV_HALO, cx = tx + EV_HALO;
    se = 0.0;
    ss = 0.0;
    if (gy < H && gx < W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = (double)sx[c][cy][cx] - (double)sg[c][cy][cx];
            se += d * d;
        }
        if (gy >= EV_HALO && gy < H - EV_HALO && gx >= EV_HALO && gx < W - EV_HALO) {
            constexpr double NP = EV_WIN * EV_WIN, C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
            for (int c = 0; c < 3; ++c) {
                double mx = 0.0, my = 0.0;
                for (int dy = 0; dy < EV_WIN; ++dy)
#pragma unroll
                    for (int dx = 0; dx < EV_WIN; ++dx) { mx += (double)sx[c][ty + dy][tx + dx]; my += (double)sg[c][ty + dy][tx + dx]; }
                mx /= NP;
                my /= NP;
                double vx = 0.0, vy = 0.0, vxy = 0.0;
                for (int dy = 0; dy < EV_WIN; ++dy)
#pragma unroll
                    for (int dx = 0; dx < EV_WIN; ++dx) {
                        const double ex = (double)sx[c][ty + dy][tx + dx] - mx, ey = (double)sg[c][ty + dy][tx + dx] - my;
                        vx += ex * ex; vy += ey * ey; vxy += ex * ey;
                    }
                vx /= NP - 1.0; vy /= NP - 1.0; vxy /= NP - 1.0;
                ss += ((2.0 * mx * my + C1) * (2.0 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2));
            }
        }
    }
    block_sum2(se, ss, red, tid);
}

// One workgroup per 16 x 16 tile of ONE frame: the tile body on the clamped render, then every thread writes its pixel's bytes
// and depth, and thread 0 the tile's partial pair.
__global__ void __launch_bounds__(FRAME_THREADS) k_eval_frame(EvalArgs a) {
    __shared__ EvalTile sx, sg;
    __shared__ double red[2][FRAME_THREADS];
    const int tid = threadIdx.x, tx = tid & (FRAME_TILE - 1), ty = tid / FRAME_TILE;
    const auto [x0, y0] = tile_origin((int)blockIdx.x, a.tiles_x);
    const int W = a.W, H = a.H;
    eval_tile_load(a.rgb, a.rgb_stride, a.gt, W, H, x0, y0, true, sx, sg, tid);

    const int gy = y0 + ty, gx = x0 + tx;
    const int cy = ty + EV_HALO, cx = tx + EV_HALO;
    if (gy < H && gx < W) {
        const int64_t pix = (int64_t)gy * W + gx;
        if (a.rgb_u8) {
#pragma unroll
            for (int c = 0; c < 3; ++c) a.rgb_u8[pix * 3 + c] = quant_u8(sx[c][cy][cx]);
        }
        if (a.compare_u8) {                                                // np.hstack((render, ground truth)): rows of 2 W pixels
            uint8_t* row = a.compare_u8 + (int64_t)gy * W * 6;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                row[(int64_t)gx * 3 + c] = quant_u8(sx[c][cy][cx]);
                row[((int64_t)W + gx) * 3 + c] = quant_u8(clamp01(sg[c][cy][cx]));
            }
        }
        if (a.depth_norm) a.depth_norm[pix] = __fdiv_rn(__fsub_rn(a.depth[pix * a.depth_stride], a.z_near), a.z_range);
    }
    if (!a.part) return;                                                   // uniform over the launch

    double se, ss;
    eval_tile_sums(sx, sg, W, H, x0, y0, red, tid, se, ss);
    if (tid == 0) { a.part[2 * (int64_t)blockIdx.x] = se; a.part[2 * (int64_t)blockIdx.x + 1] = ss; }
}

// F frames in one launch (the approximate evaluation, eval/eval_approx.py:136-148: SB objects' target views, NOT clamped there):
// workgroup b works on tile b % tiles of frame b / tiles with the same tile body and leaves its pair at part[b] — frame f's
// pairs are part[f tiles .. (f + 1) tiles), what k_eval_finish's workgroup f folds.
struct EvalFramesArgs {
    const float* rgb; const float* gt;
    int64_t frame_stride;                          // floats between two frames of rgb
    int rgb_stride, W, H, tiles_x, tiles, clamp;
    double* part;                                  // (F, tiles, 2)
};

__global__ void __launch_bounds__(FRAME_THREADS) k_eval_frames(EvalFramesArgs a) {
    __shared__ EvalTile sx, sg;
    __shared__ double red[2][FRAME_THREADS];
    const int tid = threadIdx.x;
    const int f = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x % a.tiles;
    const auto [x0, y0] = tile_origin(tile, a.tiles_x);
    const int W = a.W, H = a.H;
    eval_tile_load(a.rgb + f * a.frame_stride, a.rgb_stride, a.gt + (int64_t)f * 3 * W * H, W, H, x0, y0, a.clamp != 0, sx, sg, tid);
    double se, ss;
    eval_tile_sums(sx, sg, W, H, x0, y0, red, tid, se, ss);
    if (tid == 0) { a.part[2 * (int64_t)blockIdx.x] = se; a.part[2 * (int64_t)blockIdx.x + 1] = ss; }
}

// F pairs of 8-bit interleaved frames in one launch (eval/calc_metrics.py:218-234: the saved PNGs against the dataset's images).
// Another load in front of the same sums: x = p / 255.0f, one correctly rounded fp32 division — the bits of
// imread(..).astype(np.float32) / 255.0 — for the render and for the ground truth; a fourth channel is stepped over ([..., :3]).
// Byte loads: a frame may start at any address.  The thread that owns a pixel also writes x * 2 - 1 of both images to the
// planar (F, 3, H, W) outputs, the LPIPS inputs of :232-233, when they are asked for.
struct EvalFramesU8Args {
    const uint8_t* pred; const uint8_t* gt;
    int pred_ch, gt_ch, W, H, tiles_x, tiles;
    float* pred_planar; float* gt_planar;          // (F, 3, H, W) each, or NULL
    double* part;                                  // (F, tiles, 2)
};

__device__ __forceinline__ void eval_tile_load_u8(const uint8_t* pred, int pred_ch, const uint8_t* gt, int gt_ch, int W, int H,
                                                  int x0, int y0, EvalTile& sx, EvalTile& sg, int tid) {
    for (int i = tid; i < EV_LDS * EV_LDS; i += FRAME_THREADS) {
        const int ly = i / EV_LDS, lx = i % EV_LDS;
        const int gy = y0 - EV_HALO + ly, gx = x0 - EV_HALO + lx;
        float v[3] = {0.0f, 0.0f, 0.0f}, g[3] = {0.0f, 0.0f, 0.0f};       // outside the image: never part of a whole window
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int64_t pix = (int64_t)gy * W + gx;
            const uint8_t* p = pred + pix * pred_ch;
            const uint8_t* q = gt + pix * gt_ch;
#pragma unroll
            for (int c = 0; c < 3; ++c) { v[c] = __fdiv_rn((float)p[c], 255.0f); g[c] = __fdiv_rn((float)q[c], 255.0f); }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) { sx[c][ly][lx] = v[c]; sg[c][ly][lx] = g[c]; }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(FRAME_THREADS) k_eval_frames_u8(EvalFramesU8Args a) {
    __shared__ EvalTile sx, sg;
    __shared__ double red[2][FRAME_THREADS];
    const int tid = threadIdx.x, tx = tid & (FRAME_TILE - 1), ty = tid / FRAME_TILE;
    const int f = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x % a.tiles;
    const auto [x0, y0] = tile_origin(tile, a.tiles_x);
    const int W = a.W, H = a.H;
    const int64_t HW = (int64_t)W * H;
    eval_tile_load_u8(a.pred + f * HW * a.pred_ch, a.pred_ch, a.gt + f * HW * a.gt_ch, a.gt_ch, W, H, x0, y0, sx, sg, tid);

    const int gy = y0 + ty, gx = x0 + tx;
    const int cy = ty + EV_HALO, cx = tx + EV_HALO;
    if (gy < H && gx < W) {
        const int64_t at = (int64_t)f * 3 * HW + (int64_t)gy * W + gx;
#pragma unroll
        for (int c = 0; c < 3; ++c) {                                      // x * 2.0 - 1.0: two fp32 operations, the product exact
            if (a.pred_planar) a.pred_planar[at + c * HW] = __fsub_rn(__fmul_rn(sx[c][cy][cx], 2.0f), 1.0f);
            if (a.gt_planar) a.gt_planar[at + c * HW] = __fsub_rn(__fmul_rn(sg[c][cy][cx], 2.0f), 1.0f);
        }
    }
    double se, ss;
    eval_tile_sums(sx, sg, W, H, x0, y0, red, tid, se, ss);
    if (tid == 0) { a.part[2 * (int64_t)blockIdx.x] = se; a.part[2 * (int64_t)blockIdx.x + 1] = ss; }
}

// One workgroup per FRAME (one for k_eval_frame): thread t adds the frame's tiles t, t + 256, .. in ascending order, then
// block_sum2 — no atomics, the same inputs give the same bits, and a frame's pair is made of that frame's partial pairs alone.
// metrics[2 f] = mean squared error over 3 H W elements, metrics[2 f + 1] = mean SSIM over 3 (H - 6)(W - 6) windows.
__global__ void __launch_bounds__(FRAME_THREADS) k_eval_finish(const double* __restrict__ part, int tiles, int W, int H,
                                                               double* __restrict__ metrics) {
    __shared__ double red[2][FRAME_THREADS];
    const int tid = threadIdx.x;
    part += 2 * (int64_t)blockIdx.x * tiles;
    metrics += 2 * (int64_t)blockIdx.x;
    double se = 0.0, ss = 0.0;
    for (int t = tid; t < tiles; t += FRAME_THREADS) { se += part[2 * (int64_t)t]; ss += part[2 * (int64_t)t + 1]; }
    block_sum2(se, ss, red, tid);
    if (tid == 0) {
        metrics[0] = se / (3.0 * (double)W * (double)H);
        metrics[1] = ss / (3.0 * (double)(W - 2 * EV_HALO) * (double)(H - 2 * EV_HALO));
    }
}

}  // namespace pnr

using namespace pnr;

// The metrics' workspace: one (squared error, SSIM) pair of partial sums per frame and tile.
static double* carve_eval(Bump& b, int64_t frames, int W, int H) { return b.take<double>((uint64_t)frames * (uint64_t)frame_tiles(W, H) * 2); }
static uint64_t eval_ws_bytes(int64_t frames, int W, int H) { return bytes_of([&](Bump& b) { carve_eval(b, frames, W, H); }); }

extern "C" uint64_t pnr_eval_frame_workspace_bytes(int32_t W, int32_t H) {
    if (!frame_pixels_ok(W, H)) return 0;                  // not the tile limit: pnr_eval_frame refuses such a frame itself
    return eval_ws_bytes(1, W, H);
}

extern "C" int32_t pnr_eval_frame(const float* rgb, int32_t rgb_stride, const float* depth, int32_t depth_stride, const float* gt,
                                  int32_t W, int32_t H, float z_near, float z_far, uint8_t* rgb_u8, uint8_t* compare_u8,
                                  float* depth_norm, double* metrics, void* workspace, uint64_t workspace_bytes, void* stream) {
    if (!rgb) return PNR_E_NULL;
    if ((compare_u8 || metrics) && !gt) return PNR_E_NULL;
    if (depth_norm && !depth) return PNR_E_NULL;
    if (metrics && !workspace) return PNR_E_NULL;
    if (!frame_pixels_ok(W, H)) return PNR_E_SHAPE;
    if (rgb_stride == 0) rgb_stride = 3;
    if (depth_stride == 0) depth_stride = 1;
    if (rgb_stride < 3 || depth_stride < 1) return PNR_E_SHAPE;
    if (metrics && (W < EV_WIN || H < EV_WIN)) return PNR_E_SHAPE;
    if (depth_norm && z_far == z_near) return PNR_E_SHAPE;
    const int64_t tiles = frame_tiles(W, H);
    if (tiles > FRAME_MAX_TILES) return PNR_E_SHAPE;
    if (metrics && workspace_bytes < pnr_eval_frame_workspace_bytes(W, H)) return PNR_E_WORKSPACE;
    if (!rgb_u8 && !compare_u8 && !depth_norm && !metrics) return PNR_OK;
    EvalArgs a;
    a.rgb = rgb; a.depth = depth; a.gt = gt;
    a.rgb_stride = rgb_stride; a.depth_stride = depth_stride; a.W = W; a.H = H; a.tiles_x = frame_tiles_x(W);
    a.z_near = z_near; a.z_range = z_far - z_near;
    a.rgb_u8 = rgb_u8; a.compare_u8 = compare_u8; a.depth_norm = depth_norm;
    Bump bump(workspace);
    a.part = metrics ? carve_eval(bump, 1, W, H) : nullptr;
    hipLaunchKernelGGL(k_eval_frame, dim3((unsigned)tiles), dim3(FRAME_THREADS), 0, (hipStream_t)stream, a);
    PNR_LAUNCH_CHECK();
    if (metrics) {
        hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(FRAME_THREADS), 0, (hipStream_t)stream, (const double*)a.part, (int)tiles, W,
                           H, metrics);
        PNR_LAUNCH_CHECK();
    }
    return PNR_OK;
}

// F x tiles pairs; 0 for a shape pnr_eval_frames refuses
extern "C" uint64_t pnr_eval_frames_workspace_bytes(int32_t F, int32_t W, int32_t H) {
    if (F < 1 || !frame_pixels_ok(W, H) || W < EV_WIN || H < EV_WIN) return 0;
    const int64_t tiles = frame_tiles(W, H);
    if (tiles > FRAME_MAX_TILES / F) return 0;
    return eval_ws_bytes(F, W, H);
}

extern "C" int32_t pnr_eval_frames(const float* rgb, int32_t rgb_stride, int64_t frame_stride, const float* gt, int32_t F, int32_t W,
                                   int32_t H, int32_t clamp, double* metrics, void* workspace, uint64_t workspace_bytes,
                                   void* stream) {
    if (!rgb || !gt || !metrics || !workspace) return PNR_E_NULL;
    if (F < 1 || !frame_pixels_ok(W, H) || W < EV_WIN || H < EV_WIN) return PNR_E_SHAPE;
    const int64_t tiles = frame_tiles(W, H);
    if (tiles > FRAME_MAX_TILES / F) return PNR_E_SHAPE;                  // F x tiles workgroups in one launch
    if (rgb_stride == 0) rgb_stride = 3;
    if (rgb_stride < 3) return PNR_E_SHAPE;
    const int64_t frame_floats = (int64_t)W * H * rgb_stride;
    if (frame_stride == 0) frame_stride = frame_floats;
    if (frame_stride < frame_floats) return PNR_E_SHAPE;
    if (workspace_bytes < pnr_eval_frames_workspace_bytes(F, W, H)) return PNR_E_WORKSPACE;
    EvalFramesArgs a;
    a.rgb = rgb; a.gt = gt; a.frame_stride = frame_stride;
    a.rgb_stride = rgb_stride; a.W = W; a.H = H; a.tiles_x = frame_tiles_x(W); a.tiles = (int)tiles; a.clamp = clamp;
    Bump bump(workspace);
    a.part = carve_eval(bump, F, W, H);
    hipLaunchKernelGGL(k_eval_frames, dim3((unsigned)(F * tiles)), dim3(FRAME_THREADS), 0, (hipStream_t)stream, a);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_eval_finish, dim3((unsigned)F), dim3(FRAME_THREADS), 0, (hipStream_t)stream, (const double*)a.part,
                       (int)tiles, W, H, metrics);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

// the pairs of pnr_eval_frames: the same F x tiles partial pairs
extern "C" uint64_t pnr_eval_frames_u8_workspace_bytes(int32_t F, int32_t W, int32_t H) {
    return pnr_eval_frames_workspace_bytes(F, W, H);
}

extern "C" int32_t pnr_eval_frames_u8(const uint8_t* pred, int32_t pred_channels, const uint8_t* gt, int32_t gt_channels, int32_t F,
                                      int32_t W, int32_t H, float* pred_planar, float* gt_planar, double* metrics, void* workspace,
                                      uint64_t workspace_bytes, void* stream) {
    if (!pred || !gt || !metrics || !workspace) return PNR_E_NULL;
    if (F < 1 || !frame_pixels_ok(W, H) || W < EV_WIN || H < EV_WIN) return PNR_E_SHAPE;
    if ((pred_channels != 3 && pred_channels != 4) || (gt_channels != 3 && gt_channels != 4)) return PNR_E_SHAPE;
    const int64_t tiles = frame_tiles(W, H);
    if (tiles > FRAME_MAX_TILES / F) return PNR_E_SHAPE;                  // F x tiles workgroups in one launch
    if (workspace_bytes < pnr_eval_frames_u8_workspace_bytes(F, W, H)) return PNR_E_WORKSPACE;
    EvalFramesU8Args a;
    a.pred = pred; a.gt = gt; a.pred_ch = pred_channels; a.gt_ch = gt_channels;
    a.W = W; a.H = H; a.tiles_x = frame_tiles_x(W); a.tiles = (int)tiles;
    a.pred_planar = pred_planar; a.gt_planar = gt_planar;
    Bump bump(workspace);
    a.part = carve_eval(bump, F, W, H);
    hipLaunchKernelGGL(k_eval_frames_u8, dim3((unsigned)(F * tiles)), dim3(FRAME_THREADS), 0, (hipStream_t)stream, a);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_eval_finish, dim3((unsigned)F), dim3(FRAME_THREADS), 0, (hipStream_t)stream, (const double*)a.part,
                       (int)tiles, W, H, metrics);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
