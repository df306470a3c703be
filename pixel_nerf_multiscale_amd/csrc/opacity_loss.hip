// Opacity losses on the (n_rays, K) compositing weights: the reference's AlphaLossNV2 (model/loss.py:24-37, both of its modes) and
// a binary cross entropy against a foreground mask, value and gradient, with the numbers a trainer logs left in one device
// buffer.  include/pnr.h fixes the arithmetic: fp64 from the weights' sum to the loss, one rounding to fp32 at the end.
// Latency-bound: 512 .. ~50 k rays of 64 .. 128 weights, at most ~50 MB read once; the fold is one workgroup over 16 bytes a ray.
#include "pnr_common.h"

namespace pnr {

constexpr int FOLD_THREADS = 1024;                 // one workgroup = 16 waves
constexpr int FOLD_WAVES = FOLD_THREADS / 64;

struct AlphaCfg {
    int mode;
    double lo, hi, clamp_alpha;
};

// the 64 lanes' sum in every lane: xor butterfly 32, 16, .., 1 — every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// torch.clamp: both bounds pass at equality, a NaN stays a NaN (fmin / fmax would drop it)
__device__ __forceinline__ double clamp_keep_nan(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

__device__ __forceinline__ double alpha_term(const AlphaCfg& c, double alpha, double m) {
    const double a = clamp_keep_nan(alpha, c.lo, c.hi);
    if (c.mode == PNR_ALPHA_OPAQUE) return -log(a);
    if (c.mode == PNR_ALPHA_MASK) return -(m * log(a) + (1.0 - m) * log(1.0 - a));
    const double t = log(a) + log(1.0 - a);
    return t < -c.clamp_alpha ? -c.clamp_alpha : t;     // clamp_min; a NaN stays
}

// d term / d alpha: zero outside [lo, hi] (torch's clamp backward), for NV2 also where clamp_min cut the term
__device__ __forceinline__ double alpha_term_grad(const AlphaCfg& c, double alpha, double m) {
    if (alpha < c.lo || alpha > c.hi) return 0.0;
    const double a = alpha;                             // inside the bounds (or NaN): the clamp is the identity
    if (c.mode == PNR_ALPHA_OPAQUE) return -1.0 / a;
    if (c.mode == PNR_ALPHA_MASK) return -(m / a - (1.0 - m) / (1.0 - a));
    if (log(a) + log(1.0 - a) < -c.clamp_alpha) return 0.0;
    return 1.0 / a - 1.0 / (1.0 - a);
}

// One wave per ray: lane l adds w[r, l], w[r, l + 64], .. in ascending k, then wave_sum_f64.  A lane without a weight holds +0.
__device__ __forceinline__ double ray_alpha(const float* __restrict__ w, int K, int lane) {
    double s = 0.0;
    for (int k = lane; k < K; k += 64) s += (double)w[k];
    return wave_sum_f64(s);
}

__global__ void __launch_bounds__(256) k_alpha_sum(const float* __restrict__ coarse_w, int Kc, const float* __restrict__ fine_w, int Kf,
                                                   int64_t n_rays, double* __restrict__ alpha_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n_rays) return;                            // whole waves leave together
    if (coarse_w) {
        const double a = ray_alpha(coarse_w + r * Kc, Kc, lane);
        if (lane == 0) alpha_out[r] = a;
    }
    if (fine_w) {
        const double a = ray_alpha(fine_w + r * Kf, Kf, lane);
        if (lane == 0) alpha_out[n_rays + r] = a;
    }
}

// ONE workgroup.  The per-ray term is evaluated here, where it is summed: the entry point has no workspace, and 16 bytes a ray
// is all this reads.  Summation order, fixed by n_rays alone: ray r goes to thread r % 1024, a thread adds its rays in ascending
// r; wave sum = wave_sum_f64; block sum = wave 0 + wave 1 + .. + wave 15.
__global__ void __launch_bounds__(FOLD_THREADS) k_alpha_fold(const double* __restrict__ alpha, const float* __restrict__ mask, int64_t n_rays,
                                                             int has_c, int has_f, AlphaCfg cfg, double lambda_c, double lambda_f,
                                                             float* __restrict__ losses) {
    __shared__ double part[2][FOLD_WAVES];
    const int tid = threadIdx.x;
    double sc = 0.0, sf = 0.0;
    for (int64_t r = tid; r < n_rays; r += FOLD_THREADS) {
        const double m = cfg.mode == PNR_ALPHA_MASK ? (double)mask[r] : 0.0;
        if (has_c) sc += alpha_term(cfg, alpha[r], m);
        if (has_f) sf += alpha_term(cfg, alpha[n_rays + r], m);
    }
    sc = wave_sum_f64(sc);
    sf = wave_sum_f64(sf);
    if ((tid & 63) == 0) { part[0][tid >> 6] = sc; part[1][tid >> 6] = sf; }
    __syncthreads();
    if (tid == 0) {
        double tc = part[0][0], tf = part[1][0];
        for (int w = 1; w < FOLD_WAVES; ++w) { tc += part[0][w]; tf += part[1][w]; }
        const double n = (double)n_rays;
        const float lc = (has_c && n_rays > 0) ? (float)(lambda_c * (tc / n)) : 0.0f;      // n == 0: three zeros, not 0 / 0
        const float lf = (has_f && n_rays > 0) ? (float)(lambda_f * (tf / n)) : 0.0f;
        losses[0] = lc;
        losses[1] = lf;
        losses[2] = __fadd_rn(lc, lf);
    }
}

// One wave per ray: every lane evaluates the ray's one gradient value (the same bits in all of them) and writes it to its columns.
__global__ void __launch_bounds__(256) k_alpha_loss_bwd(const double* __restrict__ alpha, const float* __restrict__ mask, int64_t n_rays,
                                                        int Kc, int Kf, AlphaCfg cfg, double lambda_c, double lambda_f,
                                                        const float* __restrict__ d_total, float* __restrict__ d_coarse_w,
                                                        float* __restrict__ d_fine_w) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n_rays) return;
    const double d = d_total ? (double)*d_total : 1.0;
    const double m = cfg.mode == PNR_ALPHA_MASK ? (double)mask[r] : 0.0;
    const double n = (double)n_rays;
    if (d_coarse_w) {
        // d * (lambda / n * t'): a power-of-two d_total scales the fp64 value, and so its fp32 rounding, exactly
        const float g = (float)(d * (lambda_c / n * alpha_term_grad(cfg, alpha[r], m)));
        float* out = d_coarse_w + r * Kc;
        for (int k = lane; k < Kc; k += 64) out[k] = g;
    }
    if (d_fine_w) {
        const float g = (float)(d * (lambda_f / n * alpha_term_grad(cfg, alpha[n_rays + r], m)));
        float* out = d_fine_w + r * Kf;
        for (int k = lane; k < Kf; k += 64) out[k] = g;
    }
}

// the checks both entry points share; PNR_OK when a launch may follow
static inline int32_t alpha_args_check(bool has_c, int32_t Kc, bool has_f, int32_t Kf, const float* mask, int64_t n_rays, int32_t mode,
                                       float clamp_lo, float clamp_hi, const void* alpha) {
    if ((!has_c && !has_f) || (mode == PNR_ALPHA_MASK && !mask) || !alpha) return PNR_E_NULL;
    if ((has_c && Kc < 1) || (has_f && Kf < 1) || n_rays < 0 || n_rays > ((int64_t)1 << 32)) return PNR_E_SHAPE;   // n / 4 workgroups fit the grid
    if (mode != PNR_ALPHA_NV2 && mode != PNR_ALPHA_OPAQUE && mode != PNR_ALPHA_MASK) return PNR_E_SHAPE;
    if (!(clamp_lo > 0.0f && clamp_lo < clamp_hi && clamp_hi < 1.0f)) return PNR_E_SHAPE;        // a NaN bound fails too
    if (((uintptr_t)alpha) & 7) return PNR_E_ALIGN;
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_alpha_loss(const float* coarse_w, int32_t Kc, const float* fine_w, int32_t Kf, const float* mask, int64_t n_rays,
                                  int32_t mode, float lambda_coarse, float lambda_fine, float clamp_lo, float clamp_hi, float clamp_alpha,
                                  double* alpha_out, float* losses, void* stream) {
    if (!losses) return PNR_E_NULL;
    PNR_TRY(alpha_args_check(coarse_w != nullptr, Kc, fine_w != nullptr, Kf, mask, n_rays, mode, clamp_lo, clamp_hi, alpha_out));
    const AlphaCfg cfg{mode, (double)clamp_lo, (double)clamp_hi, (double)clamp_alpha};
    if (n_rays > 0) {
        hipLaunchKernelGGL(k_alpha_sum, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream, coarse_w, Kc, fine_w, Kf,
                           n_rays, alpha_out);
        PNR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_alpha_fold, dim3(1), dim3(FOLD_THREADS), 0, (hipStream_t)stream, (const double*)alpha_out, mask, n_rays,
                       coarse_w ? 1 : 0, fine_w ? 1 : 0, cfg, (double)lambda_coarse, (double)lambda_fine, losses);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_alpha_loss_bwd(const double* alpha, const float* mask, int64_t n_rays, int32_t Kc, int32_t Kf, int32_t mode,
                                      float lambda_coarse, float lambda_fine, float clamp_lo, float clamp_hi, float clamp_alpha,
                                      const float* d_total, float* d_coarse_w, float* d_fine_w, void* stream) {
    PNR_TRY(alpha_args_check(d_coarse_w != nullptr, Kc, d_fine_w != nullptr, Kf, mask, n_rays, mode, clamp_lo, clamp_hi, alpha));
    if (n_rays == 0) return PNR_OK;
    const AlphaCfg cfg{mode, (double)clamp_lo, (double)clamp_hi, (double)clamp_alpha};
    hipLaunchKernelGGL(k_alpha_loss_bwd, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream, alpha, mask, n_rays, Kc, Kf,
                       cfg, (double)lambda_coarse, (double)lambda_fine, d_total, d_coarse_w, d_fine_w);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
