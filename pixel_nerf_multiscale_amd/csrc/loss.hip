// The trainer's RGB loss (reference model/loss.py:99-103 as train/train.py:338-346 combines it): torch.nn.MSELoss /
// L1Loss(reduction="mean") of the coarse and the fine pass against the ground-truth colours, value and gradient, with the
// three numbers the reference reads back (loss_dict rc / rf / t) left in one device buffer.  Latency-bound: 512 .. ~50 k rays,
// at most 1.8 MB read.
#include "pnr_common.h"

namespace pnr {

constexpr int LOSS_THREADS = 1024;                 // one workgroup = 16 waves
constexpr int LOSS_WAVES = LOSS_THREADS / 64;

template <bool L1> __device__ __forceinline__ float loss_term(float x, float g) {
    const float d = x - g;
    return L1 ? fabsf(d) : d * d;
}

// ONE workgroup.  Summation order, fixed by the launch shape alone (bit-reproducible):
//   element e goes to thread e % 1024, chain (e / 1024) % 4 of that thread, chains run in ascending e;
//   thread sum = (c0 + c1) + (c2 + c3); wave sum = wave_sum of pnr_common.h (xor butterfly 32, 16, .., 1; every lane ends with the same bits); block sum = wave 0 + wave 1 + .. + wave 15.
// A term's path has n / 4096 + 2 + 6 + 15 additions: 27 at 5000 rays, 60 at 50 k.
template <bool L1>
__global__ void __launch_bounds__(LOSS_THREADS) k_rgb_loss(const float* __restrict__ coarse, const float* __restrict__ fine,
                                                           const float* __restrict__ gt, int64_t n /* 3 * n_rays */,
                                                           float lambda_c, float lambda_f, float* __restrict__ losses) {
    __shared__ float part[2][LOSS_WAVES];
    const int tid = threadIdx.x;
    float ac[4] = {0.f, 0.f, 0.f, 0.f}, af[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t e = tid;
    for (; e + 3 * LOSS_THREADS < n; e += 4 * LOSS_THREADS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = gt[e + j * LOSS_THREADS];
            ac[j] += loss_term<L1>(coarse[e + j * LOSS_THREADS], g);
            if (fine) af[j] += loss_term<L1>(fine[e + j * LOSS_THREADS], g);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j, e += LOSS_THREADS) {
        if (e < n) {
            const float g = gt[e];
            ac[j] += loss_term<L1>(coarse[e], g);
            if (fine) af[j] += loss_term<L1>(fine[e], g);
        }
    }
    const float sc = wave_sum((ac[0] + ac[1]) + (ac[2] + ac[3]));
    const float sf = wave_sum((af[0] + af[1]) + (af[2] + af[3]));
    if ((tid & 63) == 0) { part[0][tid >> 6] = sc; part[1][tid >> 6] = sf; }
    __syncthreads();
    if (tid == 0) {
        float tc = part[0][0], tf = part[1][0];
        for (int w = 1; w < LOSS_WAVES; ++w) { tc += part[0][w]; tf += part[1][w]; }
        const float Lc = n > 0 ? tc / (float)n : 0.0f, Lf = n > 0 ? tf / (float)n : 0.0f;   // n == 0: three zeros, not 0 / 0
        const float rc = lambda_c * Lc;
        const float rf = fine ? lambda_f * Lf : 0.0f;
        losses[0] = rc;
        losses[1] = rf;
        losses[2] = fine ? __fadd_rn(rc, rf) : Lc;         // train.py:338-345: no lambda_coarse without a fine pass
    }
}

// d_x = d_total * w * 2 (x - gt) / n   (MSE)   |   d_total * w * sign(x - gt) / n, sign(0) = 0   (L1)
// s = d_total * (w * (2 / n)) first, so a power-of-two d_total (a GradScaler scale) scales every element exactly.
template <bool L1>
__global__ void __launch_bounds__(256) k_rgb_loss_bwd(const float* __restrict__ coarse, const float* __restrict__ fine,
                                                      const float* __restrict__ gt, int64_t n, float w_c, float w_f,
                                                      const float* __restrict__ d_total, float* __restrict__ d_coarse,
                                                      float* __restrict__ d_fine) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const float d = d_total ? *d_total : 1.0f;
    const float per = (L1 ? 1.0f : 2.0f) / (float)n;
    const float g = gt[e];
    if (d_coarse) {
        const float s = d * (w_c * per), r = coarse[e] - g;
        d_coarse[e] = L1 ? (r > 0.f ? s : r < 0.f ? -s : r != r ? r : 0.0f) : s * r;
    }
    if (d_fine) {
        const float s = d * (w_f * per), r = fine[e] - g;
        d_fine[e] = L1 ? (r > 0.f ? s : r < 0.f ? -s : r != r ? r : 0.0f) : s * r;
    }
}

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_rgb_loss(const float* coarse_rgb, const float* fine_rgb, const float* rgb_gt, int64_t n_rays,
                                int32_t use_l1, float lambda_coarse, float lambda_fine, float* losses, void* stream) {
    if (!coarse_rgb || !rgb_gt || !losses) return PNR_E_NULL;
    if (n_rays < 0 || n_rays > ((int64_t)1 << 37)) return PNR_E_SHAPE;
    const int64_t n = 3 * n_rays;
    if (use_l1)
        hipLaunchKernelGGL(k_rgb_loss<true>, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, coarse_rgb, fine_rgb, rgb_gt, n,
                           lambda_coarse, lambda_fine, losses);
    else
        hipLaunchKernelGGL(k_rgb_loss<false>, dim3(1), dim3(LOSS_THREADS), 0, (hipStream_t)stream, coarse_rgb, fine_rgb, rgb_gt, n,
                           lambda_coarse, lambda_fine, losses);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_rgb_loss_bwd(const float* coarse_rgb, const float* fine_rgb, const float* rgb_gt, int64_t n_rays,
                                    int32_t use_l1, float lambda_coarse, float lambda_fine, const float* d_total,
                                    float* d_coarse_rgb, float* d_fine_rgb, void* stream) {
    if (!coarse_rgb || !rgb_gt || (d_fine_rgb && !fine_rgb)) return PNR_E_NULL;
    if (n_rays < 0 || n_rays > ((int64_t)1 << 37)) return PNR_E_SHAPE;      // 3 n / 256 workgroups fit the grid
    if (n_rays == 0 || (!d_coarse_rgb && !d_fine_rgb)) return PNR_OK;
    const int64_t n = 3 * n_rays;
    const float w_c = fine_rgb ? lambda_coarse : 1.0f;       // the weight each pass has in `total`
    const dim3 grid((unsigned)((n + 255) / 256));
    if (use_l1)
        hipLaunchKernelGGL(k_rgb_loss_bwd<true>, grid, dim3(256), 0, (hipStream_t)stream, coarse_rgb, fine_rgb, rgb_gt, n, w_c,
                           lambda_fine, d_total, d_coarse_rgb, d_fine_rgb);
    else
        hipLaunchKernelGGL(k_rgb_loss_bwd<false>, grid, dim3(256), 0, (hipStream_t)stream, coarse_rgb, fine_rgb, rgb_gt, n, w_c,
                           lambda_fine, d_total, d_coarse_rgb, d_fine_rgb);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
