// Camera gradients of the training backward: d(out) -> d(view directions), d(rays), d(stored pose, focal, c).
// (include/pnr.h: pnr_point_mlp_bwd_cam)  Runs after point_bwd's k_features_bwd on the same dzx rows and leaves
// that kernel, its launch and every gradient it writes as they are.
//
//   k_cam_grad      one wave per point, four points per block (the shape of k_features_bwd), views in sequence:
//                   per (point, view) the 16-float record [dR | dt | dfx dfy dcx dcy]; per point dp and d_dir
//   k_cam_partial   per (object, view) and chunk of CAMG_CHUNK points: the records summed in fp64, fixed order
//   k_cam_fold      per (view, component): the chunk partials folded in chunk order in fp64, rounded once to fp32
//   k_ray_fold      per ray: d_o = sum_k dp_k, d_d = sum_k (z_k dp_k + d_dir_k) in sample order in fp64; columns 6:8 = 0
// No atomics: every sum has one owner and one order, so every output is bit-reproducible.
#include "cam_grad.h"

namespace pnr {

__device__ __forceinline__ float pick3(int i, float a, float b, float c) { return i == 0 ? a : i == 1 ? b : c; }

static __global__ void __launch_bounds__(256) k_cam_grad(
    pnr_views vw, PointSrc src, int64_t P, int64_t pts_per_obj, int L, int use_code_viewdirs, int num_freqs,
    float freq_factor, const float* __restrict__ dzx, int ldz, float* __restrict__ d_dirs /* (P,3) or null */,
    float* __restrict__ pt /* (P,6): dp, d_dir; or null */, float4* __restrict__ rec /* (n_views*P, 4) or null */) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= P) return;
    const bool want_p = (pt != nullptr) || (rec != nullptr);
    float p[3], d[3];
    fetch_point(src, g, p, d);
    const int obj = (int)(g / pts_per_obj);
    float dp[3] = {0.f, 0.f, 0.f}, ddir[3] = {0.f, 0.f, 0.f};
    const int dd = use_code_viewdirs ? 6 : 3;
    const int dcode = dd + 2 * num_freqs * dd;            // entries produced by the code
    for (int v = 0; v < vw.n_views; ++v) {
        const int view = obj * vw.n_views + v;
        const Cam cam = load_cam(vw, view);
        float xr[3], dr[3];
        rot3(cam.R, p, xr);
        rot3(cam.R, d, dr);
        const float* drow = dzx + ((size_t)v * P + g) * ldz;
        float du = 0.f, dv = 0.f;
        if (want_p) {                                     // the lookup's slope, as k_features_bwd forms it
            float u, w;
            project(cam, xr, u, w);
            int c0 = 0;
            for (int lvl = 0; lvl < vw.n_levels; ++lvl) {
                const int W = vw.lat_w[lvl], H = vw.lat_h[lvl], C = vw.lat_c[lvl];
                const float usx = uv_sx(vw, lvl), usy = uv_sy(vw, lvl);
                const Taps t = bilinear_taps(u * usx, w * usy, W, H);
                const TapsGrad tg = bilinear_taps_grad(u * usx, w * usy, W, H);
                for (int ch = lane; ch < C; ch += 64) {
                    const float gz = drow[c0 + ch];
                    const float* lb = vw.latent[lvl] + ((size_t)view * C + ch) * (size_t)(H * W);
                    float sx = 0.f, sy = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float val = lb[t.off[i]];
                        sx += val * tg.dx[i];
                        sy += val * tg.dy[i];
                    }
                    du += gz * (sx * usx);
                    dv += gz * (sy * usy);
                }
                c0 += C;
            }
        }
        // positional code: lanes over the code entries; entries 0..2 of a group belong to x_rot, 3..5 (coded view directions) to dr
        float dxr[3] = {0.f, 0.f, 0.f}, ddr[3] = {0.f, 0.f, 0.f};
        for (int j = lane; j < dcode; j += 64) {
            const float gc = drow[L + j];
            int i;
            float slope;
            if (j < dd) { i = j; slope = 1.0f; }
            else {
                const int q = (j - dd) / dd;
                i = (j - dd) % dd;
                const float f = freq_factor * (float)(1 << (q >> 1));
                const float ph = (q & 1) ? 1.57079637050628662109375f : 0.0f;
                const float x = i < 3 ? pick3(i, xr[0], xr[1], xr[2]) : pick3(i - 3, dr[0], dr[1], dr[2]);
                slope = f * cosf(fmaf(x, f, ph));
            }
            const float val = gc * slope;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dxr[k] += (i == k) ? val : 0.f;
                ddr[k] += (i == k + 3) ? val : 0.f;
            }
        }
        du = wave_sum(du); dv = wave_sum(dv);
#pragma unroll
        for (int k = 0; k < 3; ++k) { dxr[k] = wave_sum(dxr[k]); ddr[k] = wave_sum(ddr[k]); }
        if (!use_code_viewdirs) {                         // the three raw columns behind the code
#pragma unroll
            for (int k = 0; k < 3; ++k) ddr[k] = drow[L + dcode + k];
        }
        const float xc = xr[0] + cam.t[0], yc = xr[1] + cam.t[1], zc = xr[2] + cam.t[2];
        // the projection's share of d(x_rot): it is d(t) as well (the code reads x_rot without t)
        const float dt[3] = {du * (-cam.fx / zc), dv * (-cam.fy / zc),
                             du * (xc * cam.fx / (zc * zc)) + dv * (yc * cam.fy / (zc * zc))};
#pragma unroll
        for (int k = 0; k < 3; ++k) dxr[k] += dt[k];
        // p = R^T x_rot, d = R^T dr
        dp[0] += cam.R[0] * dxr[0] + cam.R[3] * dxr[1] + cam.R[6] * dxr[2];
        dp[1] += cam.R[1] * dxr[0] + cam.R[4] * dxr[1] + cam.R[7] * dxr[2];
        dp[2] += cam.R[2] * dxr[0] + cam.R[5] * dxr[1] + cam.R[8] * dxr[2];
        ddir[0] += cam.R[0] * ddr[0] + cam.R[3] * ddr[1] + cam.R[6] * ddr[2];
        ddir[1] += cam.R[1] * ddr[0] + cam.R[4] * ddr[1] + cam.R[7] * ddr[2];
        ddir[2] += cam.R[2] * ddr[0] + cam.R[5] * ddr[1] + cam.R[8] * ddr[2];
        if (rec && lane == 0) {
            float4* r = rec + ((size_t)v * P + g) * 4;
            float m[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) m[i * 3 + j] = fmaf(ddr[i], d[j], dxr[i] * p[j]);
            r[0] = make_float4(m[0], m[1], m[2], m[3]);
            r[1] = make_float4(m[4], m[5], m[6], m[7]);
            r[2] = make_float4(m[8], dt[0], dt[1], dt[2]);
            r[3] = make_float4(du * (-xc / zc), dv * (-yc / zc), du, dv);
        }
    }
    if (lane == 0) {
        if (d_dirs) { d_dirs[g * 3 + 0] = ddir[0]; d_dirs[g * 3 + 1] = ddir[1]; d_dirs[g * 3 + 2] = ddir[2]; }
        if (pt) {
            float* q = pt + g * 6;
            q[0] = dp[0]; q[1] = dp[1]; q[2] = dp[2]; q[3] = ddir[0]; q[4] = ddir[1]; q[5] = ddir[2];
        }
    }
}

// grid (chunks, views).  Thread t: component t & 15 of the records chunk_first + (t >> 4), + 16, ..; then the 16 sub-sums in order.
static __global__ void __launch_bounds__(256) k_cam_partial(const float* __restrict__ rec, int64_t P, int64_t pts_per_obj,
                                                            int n_views, double* __restrict__ part) {
    __shared__ double sh[16][16];
    const int view = blockIdx.y, obj = view / n_views, v = view % n_views;
    const int comp = threadIdx.x & 15, sub = threadIdx.x >> 4;
    const int64_t first = (int64_t)blockIdx.x * CAMG_CHUNK;
    const int64_t left = pts_per_obj - first;
    const int n = (int)(left < CAMG_CHUNK ? left : CAMG_CHUNK);
    const float* r = rec + ((size_t)v * P + (size_t)obj * pts_per_obj + first) * 16 + comp;
    double acc = 0.0;
    for (int j = sub; j < n; j += 16) acc += (double)r[(size_t)j * 16];
    sh[sub][comp] = acc;
    __syncthreads();
    if (threadIdx.x < 16) {
        double sum = sh[0][comp];
#pragma unroll
        for (int k = 1; k < 16; ++k) sum += sh[k][comp];
        part[((size_t)view * gridDim.x + blockIdx.x) * 16 + comp] = sum;
    }
}

static __global__ void k_cam_fold(const double* __restrict__ part, int n_chunks, int n, float* __restrict__ d_cam) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;          // (view, component)
    if (e >= n) return;
    const int view = e >> 4, comp = e & 15;
    double sum = 0.0;
    for (int k = 0; k < n_chunks; ++k) sum += part[((size_t)view * n_chunks + k) * 16 + comp];
    d_cam[e] = (float)sum;
}

static __global__ void k_ray_fold(const float* __restrict__ pt, const float* __restrict__ z, int64_t n_rays, int K,
                                  float* __restrict__ d_rays) {
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= n_rays) return;
    double o[3] = {0.0, 0.0, 0.0}, dd[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k) {
        const float* q = pt + (ray * K + k) * 6;
        const double zk = (double)z[ray * K + k];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            o[i] += (double)q[i];
            dd[i] += zk * (double)q[i] + (double)q[3 + i];
        }
    }
    float* r = d_rays + ray * 8;
    r[0] = (float)o[0]; r[1] = (float)o[1]; r[2] = (float)o[2];
    r[3] = (float)dd[0]; r[4] = (float)dd[1]; r[5] = (float)dd[2];
    r[6] = 0.f; r[7] = 0.f;                                       // near, far: no gradient (out of scope)
}

static inline uint64_t n_chunks_of(const pnr_views* vw, int64_t P) {
    const int64_t ppo = vw->n_objs > 0 ? P / vw->n_objs : 0;
    return (uint64_t)((ppo + CAMG_CHUNK - 1) / CAMG_CHUNK);
}
// Workspace (256-byte pieces behind a base rounded up to 256, + that slack): 6 floats per point for the ray or direction
// gradients, and for the camera gradients 16 floats per (view, point) and 16 doubles per (object, view, chunk).
struct CamGradWs { float* pt; float* rec; double* part; };
static CamGradWs carve_cam_grad(Bump& b, const pnr_views* vw, int64_t P, bool want_point, bool want_cam) {
    CamGradWs w{};
    if (!want_point && !want_cam) return w;
    if (want_point) w.pt = b.take<float>((uint64_t)P * 6, 256);
    if (want_cam) {
        w.rec = b.take<float>((uint64_t)vw->n_views * P * 16, 256);
        w.part = b.take<double>((uint64_t)vw->n_objs * vw->n_views * n_chunks_of(vw, P) * 16, 256);
    }
    b.take<uint8_t>(256, 256);
    return w;
}
uint64_t cam_grad_workspace_bytes(const pnr_views* vw, int64_t P, bool want_point, bool want_cam) {
    return bytes_of([&](Bump& b) { carve_cam_grad(b, vw, P, want_point, want_cam); });
}

int32_t cam_grad_launch(const pnr_params* prm, const pnr_views* vw, PointSrc src, int64_t P, int64_t pts_per_obj, int L,
                        const float* dzx, int ldz, const CamGradOut& out, hipStream_t s) {
    const bool want_cam = out.d_cam != nullptr, want_rays = out.d_rays != nullptr;
    if (!want_cam && !want_rays && !out.d_dirs) return PNR_OK;
    Bump bump(round_up_256(out.ws));
    const CamGradWs w = carve_cam_grad(bump, vw, P, want_rays || out.d_dirs, want_cam);
    if (out.ws_bytes < bump.off) return PNR_E_WORKSPACE;
    float* pt = want_rays ? w.pt : nullptr;         // the per-point records feed the ray fold alone; d_dirs is written directly
    float* rec = w.rec;
    double* part = w.part;
    hipLaunchKernelGGL(k_cam_grad, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, *vw, src, P, pts_per_obj, L,
                       prm->use_code_viewdirs, prm->num_freqs, prm->freq_factor, dzx, ldz, out.d_dirs, pt, (float4*)rec);
    PNR_LAUNCH_CHECK();
    if (want_cam) {
        const int views = vw->n_objs * vw->n_views, nch = (int)n_chunks_of(vw, P);
        hipLaunchKernelGGL(k_cam_partial, dim3((unsigned)nch, (unsigned)views), dim3(256), 0, s, rec, P, pts_per_obj, vw->n_views, part);
        PNR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_cam_fold, dim3((unsigned)((views * 16 + 255) / 256)), dim3(256), 0, s, part, nch, views * 16, out.d_cam);
        PNR_LAUNCH_CHECK();
    }
    if (want_rays) {
        const int64_t n_rays = P / src.K;
        hipLaunchKernelGGL(k_ray_fold, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, s, pt, src.z, n_rays, src.K, out.d_rays);
        PNR_LAUNCH_CHECK();
    }
    return PNR_OK;
}

}  // namespace pnr
