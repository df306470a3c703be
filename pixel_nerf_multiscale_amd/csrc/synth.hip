// Procedural datasets (include/pnr.h, "procedural datasets"): objects made of a few ellipsoids and boxes, ray-cast exactly into
// the bytes an SRN folder would hold — white background, mask = "no channel is 255" — with the ground-truth depth, F frames in
// ONE launch.
//   pnr_synth_render   k_synth_render   per workgroup a run of 256 pixels of one frame: the scene's records once into LDS;
//                                       per thread four neighbouring pixels, ss x ss sub-samples each, 12 colour bytes as 3 dwords
// No atomics, no workspace.  The bound is the stores (3 to 8 bytes per pixel against at most 16 x 8 ray / primitive tests of a
// few dozen flops); the point is that a data set starts on a seed, not on files.
#include "pnr_common.h"

// The header states every fp32 operation of the ray cast and its order; a fused multiply-add would be another rounding.
#pragma clang fp contract(off)

namespace pnr {

constexpr int SY_THREADS = 64;                        // one wave
constexpr int SY_PIX = 4;                             // pixels per thread: 12 colour bytes = 3 dwords
constexpr int SY_RUN = SY_THREADS * SY_PIX;           // pixels per workgroup
constexpr int SY_REC = PNR_SYNTH_REC;
constexpr int SY_LDS_REC = SY_REC + 4;                // the record, then ol (3) and one pad

struct SynthArgs {
    const float* scenes; int n_scenes, P;
    const int32_t* scene_ids; const float* poses;
    int W; int64_t HW; int64_t runs;                  // workgroups per frame
    float fx, fy, cx, cy;
    int ss; float inv_n, ambient, one_minus, l[3];
    uint8_t* rgb; int64_t rgb_stride;
    uint8_t* mask; float* depth;
};

// IEEE square root: sqrtf is correctly rounded under hipcc's default; the header's __fsqrt_rn is the native approximation (1 ulp)
// unless OCML_BASIC_ROUNDED_OPERATIONS is defined
__device__ __forceinline__ float sqrt_rn(float x) { return __builtin_sqrtf(x); }

__device__ __forceinline__ float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

// The nearest hit of the ray (o, d) over the staged primitives: t, or +inf; then its colour.  rec: LDS, [p][SY_LDS_REC].
__device__ __forceinline__ bool synth_sample(const float* rec, int P, const float d[3], const float l[3], float ambient,
                                             float one_minus, float& t_out, float col[3]) {
    float best = __builtin_inff();
    int win = -1, win_face = 0;
    float win_tp = 0.0f;
    for (int p = 0; p < P; ++p) {
        const float* r = rec + p * SY_LDS_REC;
        const float kind = r[0];
        if (kind != 1.0f && kind != 2.0f) continue;
        float dl[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) dl[i] = dot3(r[4 + 3 * i], r[5 + 3 * i], r[6 + 3 * i], d[0], d[1], d[2]);
        const float* ol = r + SY_REC;
        const float* h = r + 13;
        if (kind == 1.0f) {
            const float tc = -dot3(ol[0], ol[1], ol[2], dl[0], dl[1], dl[2]);
            float oe[3], de[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) { oe[i] = __fdiv_rn(ol[i] + tc * dl[i], h[i]); de[i] = __fdiv_rn(dl[i], h[i]); }
            const float A = dot3(de[0], de[1], de[2], de[0], de[1], de[2]);
            const float B = dot3(oe[0], oe[1], oe[2], de[0], de[1], de[2]);
            const float Cq = dot3(oe[0], oe[1], oe[2], oe[0], oe[1], oe[2]) - 1.0f;
            const float disc = B * B - A * Cq;
            if (!(disc > 0.0f)) continue;
            const float tp = __fdiv_rn(-B - sqrt_rn(disc), A);
            const float t = tc + tp;
            if (!(t > 0.0f)) continue;
            if (t < best) { best = t; win = p; win_tp = tp; }
        } else {
            float tn = -__builtin_inff(), tf = __builtin_inff();
            int face = 0;
            bool miss = false;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (dl[a] == 0.0f) {
                    if (fabsf(ol[a]) > h[a]) miss = true;
                } else {
                    const float t1 = __fdiv_rn(-h[a] - ol[a], dl[a]), t2 = __fdiv_rn(h[a] - ol[a], dl[a]);
                    const float lo = t2 < t1 ? t2 : t1, hi = t2 > t1 ? t2 : t1;
                    if (lo > tn) { tn = lo; face = a; }
                    if (hi < tf) tf = hi;
                }
            }
            if (miss || !(tn < tf) || !(tn > 0.0f)) continue;
            if (tn < best) { best = tn; win = p; win_face = face; }
        }
    }
    t_out = best;
    if (win < 0) {
        col[0] = col[1] = col[2] = 1.0f;
        return false;
    }
    const float* r = rec + win * SY_LDS_REC;
    float n[3];
    if (r[0] == 1.0f) {
        const float* ol = r + SY_REC;
        const float* h = r + 13;
        float dl[3], g[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) dl[i] = dot3(r[4 + 3 * i], r[5 + 3 * i], r[6 + 3 * i], d[0], d[1], d[2]);
        const float tc = -dot3(ol[0], ol[1], ol[2], dl[0], dl[1], dl[2]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float oe = __fdiv_rn(ol[i] + tc * dl[i], h[i]), de = __fdiv_rn(dl[i], h[i]);
            g[i] = __fdiv_rn(oe + win_tp * de, h[i]);
        }
        float m[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) m[j] = (r[4 + j] * g[0] + r[7 + j] * g[1]) + r[10 + j] * g[2];
        const float len = sqrt_rn(dot3(m[0], m[1], m[2], m[0], m[1], m[2]));
#pragma unroll
        for (int j = 0; j < 3; ++j) n[j] = __fdiv_rn(m[j], len);
    } else {
        const float* row = r + 4 + 3 * win_face;
        const float dlf = dot3(row[0], row[1], row[2], d[0], d[1], d[2]);
        const float s = dlf > 0.0f ? -1.0f : 1.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) n[j] = row[j] * s;
    }
    float k = dot3(n[0], n[1], n[2], l[0], l[1], l[2]);
    k = k > 0.0f ? k : 0.0f;
    const float shade = ambient + one_minus * k;
#pragma unroll
    for (int c = 0; c < 3; ++c) col[c] = r[16 + c] * shade;
    return true;
}

__device__ __forceinline__ uint32_t synth_byte(float mean, bool any_hit) {
    const float w = mean * 255.0f + 0.5f;
    uint32_t b = !(w > 0.0f) ? 0u : w >= 255.0f ? 255u : (uint32_t)(int)floorf(w);
    if (any_hit && b > 254u) b = 254u;
    return b;
}

__global__ void __launch_bounds__(SY_THREADS) k_synth_render(SynthArgs a) {
    __shared__ float rec[PNR_SYNTH_MAX_PRIMS * SY_LDS_REC];
    __shared__ float cam[12];                                              // C row major (9), o (3)
    const int tid = threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x / a.runs, run = (int64_t)blockIdx.x - f * a.runs;
    const float* pose = a.poses + f * 16;
    const int sid = a.scene_ids[f];
    const int P = (sid >= 0 && sid < a.n_scenes) ? a.P : 0;               // uniform over the workgroup
    if (tid < 12) cam[tid] = tid < 9 ? pose[(tid / 3) * 4 + tid % 3] : pose[(tid - 9) * 4 + 3];
    if (tid < P) {
        const float* src = a.scenes + ((int64_t)sid * a.P + tid) * SY_REC;
        float* dst = rec + tid * SY_LDS_REC;
#pragma unroll
        for (int i = 0; i < SY_REC; ++i) dst[i] = src[i];
        const float q0 = pose[3] - src[1], q1 = pose[7] - src[2], q2 = pose[11] - src[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) dst[SY_REC + i] = dot3(src[4 + 3 * i], src[5 + 3 * i], src[6 + 3 * i], q0, q1, q2);
        dst[SY_REC + 3] = 0.0f;
    }
    __syncthreads();

    const int64_t i0 = run * SY_RUN + (int64_t)tid * SY_PIX;              // first pixel of this thread, inside the frame or past it
    if (i0 >= a.HW) return;
    const int npix = a.HW - i0 < SY_PIX ? (int)(a.HW - i0) : SY_PIX;
    uint32_t bytes[3 * SY_PIX];
    uint32_t mk[SY_PIX];
    float dep[SY_PIX];
    const float half = 0.5f;
#pragma unroll
    for (int k = 0; k < SY_PIX; ++k) {
        mk[k] = 0; dep[k] = 0.0f;
        bytes[3 * k] = bytes[3 * k + 1] = bytes[3 * k + 2] = 0;
        if (k >= npix) continue;
        const int64_t i = i0 + k;
        const int row = (int)(i / a.W), colx = (int)(i - (int64_t)row * a.W);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        bool any_hit = false;
        for (int b = 0; b < a.ss; ++b) {
            const float y = (float)row + (__fdiv_rn((float)b + half, (float)a.ss) - half);
            const float v = -__fdiv_rn(y - a.cy, a.fy);
            for (int s = 0; s < a.ss; ++s) {
                const float x = (float)colx + (__fdiv_rn((float)s + half, (float)a.ss) - half);
                const float u = __fdiv_rn(x - a.cx, a.fx);
                const float len = sqrt_rn((u * u + v * v) + 1.0f);
                const float dc0 = __fdiv_rn(u, len), dc1 = __fdiv_rn(v, len), dc2 = __fdiv_rn(-1.0f, len);
                float d[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) d[j] = dot3(cam[3 * j], cam[3 * j + 1], cam[3 * j + 2], dc0, dc1, dc2);
                float t, col[3];
                const bool hit = synth_sample(rec, P, d, a.l, a.ambient, a.one_minus, t, col);
                any_hit = any_hit || hit;
                if (b == 0 && s == 0) dep[k] = t;                          // +inf on a miss
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + col[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) bytes[3 * k + c] = synth_byte(acc[c] * a.inv_n, any_hit);
        mk[k] = any_hit ? 255u : 0u;
    }

    uint8_t* dst = a.rgb + f * a.rgb_stride + 3 * i0;                      // bytes [3 i0, 3 (i0 + npix)) of the frame's 3 HW
    if (npix == SY_PIX && ((uintptr_t)dst & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            ((uint32_t*)dst)[q] = bytes[4 * q] | bytes[4 * q + 1] << 8 | bytes[4 * q + 2] << 16 | bytes[4 * q + 3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < 3 * SY_PIX; ++j)
            if (j < 3 * npix) dst[j] = (uint8_t)bytes[j];
    }
    if (a.mask) {
        uint8_t* m = a.mask + f * a.HW + i0;
        if (npix == SY_PIX && ((uintptr_t)m & 3) == 0) *(uint32_t*)m = mk[0] | mk[1] << 8 | mk[2] << 16 | mk[3] << 24;
        else {
#pragma unroll
            for (int k = 0; k < SY_PIX; ++k)
                if (k < npix) m[k] = (uint8_t)mk[k];
        }
    }
    if (a.depth) {
        float* z = a.depth + f * a.HW + i0;
#pragma unroll
        for (int k = 0; k < SY_PIX; ++k)
            if (k < npix) z[k] = dep[k];
    }
}

static inline bool finite_h(float v) { return v - v == 0.0f; }               // false for NaN and Inf

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_synth_render(const float* scenes, int32_t n_scenes, int32_t P, const int32_t* scene_ids, const float* poses,
                                    int32_t F, int32_t W, int32_t H, float fx, float fy, float cx, float cy, int32_t ss, float ambient,
                                    float light_x, float light_y, float light_z, uint8_t* rgb_out, int64_t rgb_frame_stride,
                                    uint8_t* mask_out, float* depth_out, void* stream) {
    if (!scenes || !scene_ids || !poses || !rgb_out) return PNR_E_NULL;
    if (n_scenes < 0 || P < 1 || P > PNR_SYNTH_MAX_PRIMS || F < 1 || W < 1 || H < 1) return PNR_E_SHAPE;
    const int64_t HW = (int64_t)W * H;
    if (HW >= ((int64_t)1 << 31) || (int64_t)F * HW >= ((int64_t)1 << 31) || rgb_frame_stride < 3 * HW) return PNR_E_SHAPE;
    if (ss != 1 && ss != 2 && ss != 4) return PNR_E_SHAPE;
    if (!finite_h(fx) || !finite_h(fy) || fx == 0.0f || fy == 0.0f || !finite_h(cx) || !finite_h(cy)) return PNR_E_SHAPE;
    if (!(ambient >= 0.0f && ambient <= 1.0f)) return PNR_E_SHAPE;
    const double lx = light_x, ly = light_y, lz = light_z, norm = sqrt(lx * lx + ly * ly + lz * lz);
    if (!(norm > 0.0) || !(norm < 1e300)) return PNR_E_SHAPE;               // zero, NaN or Inf
    if ((((uintptr_t)scenes | (uintptr_t)scene_ids | (uintptr_t)poses | (uintptr_t)depth_out) & 3) != 0) return PNR_E_ALIGN;
    SynthArgs a;
    a.scenes = scenes; a.n_scenes = n_scenes; a.P = P; a.scene_ids = scene_ids; a.poses = poses;
    a.W = W; a.HW = HW; a.runs = (HW + SY_RUN - 1) / SY_RUN;
    a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    a.ss = ss; a.inv_n = 1.0f / (float)(ss * ss); a.ambient = ambient; a.one_minus = 1.0f - ambient;
    a.l[0] = (float)(lx / norm); a.l[1] = (float)(ly / norm); a.l[2] = (float)(lz / norm);
    a.rgb = rgb_out; a.rgb_stride = rgb_frame_stride; a.mask = mask_out; a.depth = depth_out;
    const int64_t blocks = a.runs * F;                                        // <= F HW < 2^31
    if (blocks * SY_THREADS >= ((int64_t)1 << 32)) return PNR_E_SHAPE;        // more threads than one launch takes
    hipLaunchKernelGGL(k_synth_render, dim3((unsigned)blocks), dim3(SY_THREADS), 0, (hipStream_t)stream, a);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
