// The back end of the training step (reference train/train.py:375-412 with trainlib/trainer.py:169): what follows
// loss.backward() — GradScaler.unscale_, clip_grad_norm_, the found-inf skip, Adam, GradScaler.update — as three launches
// over every trainable tensor at once, with nothing read back:
//   k_grad_sumsq     per chunk: the fp64 sum of (grad * inv_scale)^2 and a non-finite flag, into the workspace
//   k_optim_reduce   ONE workgroup: the norm, clip_coef, found_inf, the scaler, t (or `skipped`), the step's two scalars
//   k_adam_apply     per chunk: m, v, p; returns at once on a skipped step
// The first and the last are streaming passes (g once; g, m, v, p in and m, v, p out: 28 bytes per parameter) and are bound by
// HBM; the one in the middle is bound by its launch.  No floating-point atomics: every sum has an order fixed by the chunk
// table alone, so the same inputs give the same bits.
#include <math.h>

#include "frame_common.h"

// include/pnr.h fixes the arithmetic as separately rounded fp32 operations (what torch's kernels round, in another order):
// hipcc's default -ffp-contract=fast would fuse the products into the sums.  As in mesh.hip, nothing in this file is fused.
#pragma clang fp contract(off)

namespace pnr {

constexpr int OPT_THREADS = 256;                          // 4 waves
constexpr int OPT_VEC = 4;                                // floats of one 16-byte access
constexpr int OPT_PER_THREAD = 4;                         // 16-byte accesses of one thread in one chunk
constexpr int OPT_CHUNK = OPT_THREADS * OPT_VEC * OPT_PER_THREAD;   // 4096 elements: 16 KiB of each array
constexpr int OPT_MAX_GRID = 2048;                        // 8 workgroups for each of 256 CUs; the chunks beyond are grid-strided, evenly

// What a chunk table entry resolves to; n == 0 for an entry that does not fit its tables (nothing is read or written then).
struct ChunkView { float* p; int64_t flat; int n; };

__device__ __forceinline__ ChunkView chunk_view(const pnr_optim_segment* __restrict__ segs, int n_segs,
                                                const pnr_optim_chunk* __restrict__ chunks, int64_t c, int64_t n_flat) {
    ChunkView cv;
    cv.p = nullptr; cv.flat = 0; cv.n = 0;
    const pnr_optim_chunk ch = chunks[c];
    if (ch.segment < 0 || ch.segment >= n_segs || ch.first < 0) return cv;
    const pnr_optim_segment sg = segs[ch.segment];
    if (!sg.param || sg.offset < 0 || ch.first >= sg.n || sg.offset > n_flat || sg.n > n_flat - sg.offset) return cv;
    const int64_t left = sg.n - ch.first;
    cv.p = sg.param + ch.first;
    cv.flat = sg.offset + ch.first;
    cv.n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    return cv;
}

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for Inf and NaN

// Sum of `a` over the workgroup and OR of `bad` (block_fold).
__device__ __forceinline__ void block_sum_or(double& a, int& bad, double* red, int* redb, int tid) {
    red[tid] = a;
    redb[tid] = bad;
    block_fold<OPT_THREADS>(tid, [red, redb](int i, int j) { red[i] += red[j]; redb[i] |= redb[j]; });
    a = red[0];
    bad = redb[0];
    __syncthreads();                                      // the next chunk of a grid-strided workgroup reuses red
}

// The inverse scale the gradients carry: (float)(1 / (double)scale), or 1 without a scaler.
__device__ __forceinline__ float inv_scale_of(const pnr_optim_state* st, int use_scaler) {
    return use_scaler ? (float)(1.0 / (double)st->scale) : 1.0f;
}

// Element e of a chunk belongs to thread (e / 4) % 256, which visits its elements in ascending order: 16 fp64 additions per
// thread, then the 8 levels of block_sum_or.  The order depends on the element's place in its chunk alone — the 16-byte and
// the scalar loads feed the same additions.  DIV (pnr_adam_step_div with grad_div > 1): the gradient is a SUM over grad_div ranks
// and every use of it is ((grad * inv_scale) * inv_div); without DIV the multiply is not compiled in.
template <bool DIV>
__global__ void __launch_bounds__(OPT_THREADS) k_grad_sumsq(const pnr_optim_segment* __restrict__ segs, int n_segs,
                                                            const pnr_optim_chunk* __restrict__ chunks, int64_t n_chunks,
                                                            const float* __restrict__ grad, int64_t n_flat,
                                                            const pnr_optim_state* __restrict__ st, int use_scaler, float inv_div,
                                                            double* __restrict__ part, int32_t* __restrict__ flag) {
    __shared__ double red[OPT_THREADS];
    __shared__ int redb[OPT_THREADS];
    const int tid = threadIdx.x;
    const float inv = inv_scale_of(st, use_scaler);
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ChunkView cv = chunk_view(segs, n_segs, chunks, c, n_flat);
        const float* g = grad + cv.flat;
        const bool vec = (cv.flat & (OPT_VEC - 1)) == 0;  // the flat buffer itself is 16-byte aligned (checked on the host)
        double acc = 0.0;
        int bad = 0;
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = (j * OPT_THREADS + tid) * OPT_VEC;
            float x[OPT_VEC] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (vec && e + OPT_VEC <= cv.n) {
                const float4 q = *reinterpret_cast<const float4*>(g + e);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < OPT_VEC; ++k)
                    if (e + k < cv.n) x[k] = g[e + k];
            }
#pragma unroll
            for (int k = 0; k < OPT_VEC; ++k) {
                float u = x[k] * inv;                     // rounded to fp32, as unscale_ leaves it
                if (DIV) u = u * inv_div;
                bad |= finite_f(u) ? 0 : 1;
                const double d = (double)u;
                acc += d * d;                             // the square of an fp32 value is exact in fp64
            }
        }
        block_sum_or(acc, bad, red, redb, tid);
        if (tid == 0) { part[c] = acc; flag[c] = bad; }
    }
}

struct ReduceArgs {
    double lr, beta1, beta2, max_norm;
    float growth, backoff;
    int growth_interval, use_scaler;
};

// ONE workgroup.  Thread t adds the partials of chunks t, t + 256, .. in ascending order, then block_sum_or: the longest
// addition path of grad_norm is 16 + 8 (k_grad_sumsq) + ceil(n_chunks / 256) + 8 additions.
__global__ void __launch_bounds__(OPT_THREADS) k_optim_reduce(const double* __restrict__ part, const int32_t* __restrict__ flag,
                                                              int64_t n_chunks, ReduceArgs a, pnr_optim_state* __restrict__ st) {
    __shared__ double red[OPT_THREADS];
    __shared__ int redb[OPT_THREADS];
    const int tid = threadIdx.x;
    double s = 0.0;
    int bad = 0;
    for (int64_t c = tid; c < n_chunks; c += OPT_THREADS) { s += part[c]; bad |= flag[c]; }
    block_sum_or(s, bad, red, redb, tid);
    if (tid != 0) return;

    const double total = sqrt(s);
    const int found = (bad != 0 || !(total <= 1.79769313486231570e+308)) ? 1 : 0;
    st->grad_norm = total;
    st->found_inf = found;
    st->inv_scale = inv_scale_of(st, a.use_scaler);       // of the scale these gradients carry: k_adam_apply reads it
    if (found) {
        st->clip_coef = 0.0f;                             // nothing is applied
        st->skipped += 1;
    } else {
        double coef = 1.0;
        if (a.max_norm > 0.0) {
            coef = a.max_norm / (total + 1e-6);
            if (!(coef < 1.0)) coef = 1.0;
        }
        st->clip_coef = (float)coef;
        const int64_t t = st->step + 1;
        st->step = t;
        st->step_size = (float)(a.lr / (1.0 - pow(a.beta1, (double)t)));
        st->rsqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow(a.beta2, (double)t)));
    }
    if (a.use_scaler) {                                   // GradScaler.update
        if (found) {
            st->scale = st->scale * a.backoff;
            st->growth_tracker = 0;
        } else {
            const int tr = st->growth_tracker + 1;
            if (tr >= a.growth_interval) {
                const float grown = st->scale * a.growth;
                if (finite_f(grown)) st->scale = grown;   // torch keeps the scale where growing it would overflow
                st->growth_tracker = 0;
            } else {
                st->growth_tracker = tr;
            }
        }
    }
}

struct AdamConsts { float beta1, one_minus_beta1, beta2, one_minus_beta2, eps, inv_scale, clip_coef, step_size, rsqrt_bc2, inv_div; };

template <bool DIV>
__device__ __forceinline__ void adam_elem(float grad, float& m, float& v, float& p, const AdamConsts& k) {
    float g = grad * k.inv_scale;
    if (DIV) g = g * k.inv_div;
    g = g * k.clip_coef;
    m = k.beta1 * m + k.one_minus_beta1 * g;
    v = k.beta2 * v + (k.one_minus_beta2 * g) * g;
    const float denom = __fsqrt_rn(v) * k.rsqrt_bc2 + k.eps;
    p = p - k.step_size * __fdiv_rn(m, denom);
}

// 28 bytes per parameter.  A chunk takes 16-byte loads and stores when its parameter pointer and its flat offset are both
// 16-byte aligned (every chunk of a tensor torch allocated); a view that starts inside its storage takes the scalar body, and
// so does the last, partial quad of a segment.  Plain stores: m, v and p are read again next step and nothing else is
// between, so there is no reason to steer them past the L2.
template <bool DIV>
__global__ void __launch_bounds__(OPT_THREADS) k_adam_apply(const pnr_optim_segment* __restrict__ segs, int n_segs,
                                                            const pnr_optim_chunk* __restrict__ chunks, int64_t n_chunks,
                                                            const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                            float* __restrict__ exp_avg_sq, int64_t n_flat,
                                                            const pnr_optim_state* __restrict__ st, AdamConsts k) {
    if (st->found_inf) return;                            // uniform over the launch: p, m, v keep their bits
    k.inv_scale = st->inv_scale;
    k.clip_coef = st->clip_coef;
    k.step_size = st->step_size;
    k.rsqrt_bc2 = st->rsqrt_bc2;
    const int tid = threadIdx.x;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ChunkView cv = chunk_view(segs, n_segs, chunks, c, n_flat);
        const float* g = grad + cv.flat;
        float* m = exp_avg + cv.flat;
        float* v = exp_avg_sq + cv.flat;
        float* p = cv.p;
        const bool vec = (cv.flat & (OPT_VEC - 1)) == 0 && ((uintptr_t)p & 15) == 0;
#pragma unroll
        for (int j = 0; j < OPT_PER_THREAD; ++j) {
            const int e = (j * OPT_THREADS + tid) * OPT_VEC;
            if (vec && e + OPT_VEC <= cv.n) {
                const float4 gq = *reinterpret_cast<const float4*>(g + e);
                float4 mq = *reinterpret_cast<const float4*>(m + e);
                float4 vq = *reinterpret_cast<const float4*>(v + e);
                float4 pq = *reinterpret_cast<const float4*>(p + e);
                adam_elem<DIV>(gq.x, mq.x, vq.x, pq.x, k);
                adam_elem<DIV>(gq.y, mq.y, vq.y, pq.y, k);
                adam_elem<DIV>(gq.z, mq.z, vq.z, pq.z, k);
                adam_elem<DIV>(gq.w, mq.w, vq.w, pq.w, k);
                *reinterpret_cast<float4*>(m + e) = mq;
                *reinterpret_cast<float4*>(v + e) = vq;
                *reinterpret_cast<float4*>(p + e) = pq;
            } else {
#pragma unroll
                for (int q = 0; q < OPT_VEC; ++q)
                    if (e + q < cv.n) {
                        float mm = m[e + q], vv = v[e + q], pp = p[e + q];
                        adam_elem<DIV>(g[e + q], mm, vv, pp, k);
                        m[e + q] = mm; v[e + q] = vv; p[e + q] = pp;
                    }
            }
        }
    }
}

// pnr_adam_step's workspace, 16-byte pieces: every chunk's fp64 sum of squares | every chunk's non-finite flag
struct OptimWs { double* part; int32_t* flag; };
static OptimWs carve_optim(Bump& b, int64_t n_chunks) {
    OptimWs w;
    w.part = b.take<double>((uint64_t)n_chunks, 16);
    w.flag = b.take<int32_t>((uint64_t)n_chunks, 16);
    b.pad(16);
    return w;
}
constexpr int64_t OPT_MAX_CHUNKS = (int64_t)1 << 31;      // 2^43 parameters

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int64_t pnr_optim_plan(const int64_t* seg_n, int32_t n_segments, pnr_optim_chunk* chunks_out, int64_t max_chunks) {
    if (n_segments < 0 || max_chunks < 0) return PNR_E_SHAPE;
    if (n_segments > 0 && !seg_n) return PNR_E_NULL;
    int64_t count = 0;
    for (int32_t s = 0; s < n_segments; ++s) {
        if (seg_n[s] < 0) return PNR_E_SHAPE;
        for (int64_t first = 0; first < seg_n[s]; first += OPT_CHUNK) {
            if (chunks_out && count < max_chunks) {
                chunks_out[count].segment = s;
                chunks_out[count].reserved = 0;
                chunks_out[count].first = first;
            }
            ++count;
        }
    }
    return count;
}

extern "C" uint64_t pnr_optim_workspace_bytes(int64_t n_chunks) {
    if (n_chunks < 0 || n_chunks >= OPT_MAX_CHUNKS) return 0;
    return bytes_of([&](Bump& b) { carve_optim(b, n_chunks); });
}

extern "C" int32_t pnr_adam_step_div(const pnr_optim_segment* segments, int32_t n_segments, const pnr_optim_chunk* chunks,
                                     int64_t n_chunks, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat,
                                     double lr, double beta1, double beta2, double eps, double max_norm,
                                     const pnr_optim_scaler* scaler, int32_t grad_div, pnr_optim_state* state, void* workspace,
                                     uint64_t workspace_bytes, void* stream) {
    if (grad_div < 1) return PNR_E_SHAPE;
    if (n_segments < 0 || n_chunks < 0 || n_flat < 0 || n_chunks >= OPT_MAX_CHUNKS) return PNR_E_SHAPE;
    if (!state) return PNR_E_NULL;
    if (n_chunks > 0 && (!segments || !chunks || !grad || !exp_avg || !exp_avg_sq || !workspace)) return PNR_E_NULL;
    if (n_chunks > 0 && (n_segments < 1 || n_flat < 1)) return PNR_E_SHAPE;
    if (scaler && scaler->growth_interval < 1) return PNR_E_SHAPE;
    if (n_chunks > 0 && workspace_bytes < pnr_optim_workspace_bytes(n_chunks)) return PNR_E_WORKSPACE;
    if ((((uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)workspace) & 15) != 0) return PNR_E_ALIGN;
    if ((((uintptr_t)state | (uintptr_t)segments | (uintptr_t)chunks) & 7) != 0) return PNR_E_ALIGN;
    if (n_chunks == 0) return PNR_OK;                     // no gradient anywhere: torch's Adam does nothing either

    Bump bump(workspace);
    const OptimWs ws = carve_optim(bump, n_chunks);
    double* part = ws.part;
    int32_t* flag = ws.flag;
    const int use_scaler = scaler ? 1 : 0;
    // at most OPT_MAX_GRID workgroups, every one with the same number of chunks (give or take one in the last round): 3500 chunks
    // run as 1750 workgroups of two, not as 2048 of which 1452 take a second one while the rest idle
    const int64_t rounds = (n_chunks + OPT_MAX_GRID - 1) / OPT_MAX_GRID;
    const unsigned grid = (unsigned)((n_chunks + rounds - 1) / rounds);
    hipStream_t s = (hipStream_t)stream;
    const bool div = grad_div > 1;
    const float inv_div = 1.0f / (float)grad_div;         // rounded once, here

    hipLaunchKernelGGL((div ? k_grad_sumsq<true> : k_grad_sumsq<false>), dim3(grid), dim3(OPT_THREADS), 0, s, segments, (int)n_segments,
                       chunks, n_chunks, grad, n_flat, (const pnr_optim_state*)state, use_scaler, inv_div, part, flag);
    PNR_LAUNCH_CHECK();

    ReduceArgs ra;
    ra.lr = lr; ra.beta1 = beta1; ra.beta2 = beta2; ra.max_norm = max_norm;
    ra.growth = scaler ? scaler->growth_factor : 1.0f;
    ra.backoff = scaler ? scaler->backoff_factor : 1.0f;
    ra.growth_interval = scaler ? scaler->growth_interval : 1;
    ra.use_scaler = use_scaler;
    hipLaunchKernelGGL(k_optim_reduce, dim3(1), dim3(OPT_THREADS), 0, s, (const double*)part, (const int32_t*)flag, n_chunks, ra, state);
    PNR_LAUNCH_CHECK();

    AdamConsts k;
    k.beta1 = (float)beta1; k.one_minus_beta1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2; k.one_minus_beta2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.inv_scale = 1.0f; k.clip_coef = 1.0f; k.step_size = 0.0f; k.rsqrt_bc2 = 1.0f;      // read from `state` on the device
    k.inv_div = inv_div;
    hipLaunchKernelGGL((div ? k_adam_apply<true> : k_adam_apply<false>), dim3(grid), dim3(OPT_THREADS), 0, s, segments, (int)n_segments,
                       chunks, n_chunks, grad, exp_avg, exp_avg_sq, n_flat, (const pnr_optim_state*)state, k);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_adam_step(const pnr_optim_segment* segments, int32_t n_segments, const pnr_optim_chunk* chunks,
                                 int64_t n_chunks, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat,
                                 double lr, double beta1, double beta2, double eps, double max_norm,
                                 const pnr_optim_scaler* scaler, pnr_optim_state* state, void* workspace,
                                 uint64_t workspace_bytes, void* stream) {
    return pnr_adam_step_div(segments, n_segments, chunks, n_chunks, grad, exp_avg, exp_avg_sq, n_flat, lr, beta1, beta2, eps, max_norm,
                             scaler, 1, state, workspace, workspace_bytes, stream);
}
