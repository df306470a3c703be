// The colour chain of the jitter augmentation (include/pnr.h, "colour jitter"): one record per object — four factors, the
// object's grey mean, the order of the four operations — applied to one pixel in [0, 1].  Shared by the plan's reduction
// (jitter.hip: the operations in front of contrast) and by the two jitter gathers (data_u8.h: the whole chain), so the mean is
// taken over exactly the values the gathers would see.  No operation indexes memory, so any record, NaN included, is safe to
// apply.
#pragma once
#include "frame_common.h"

// Every fp32 operation of the chain is rounded on its own.  hipcc's default -ffp-contract=fast turns a product and a sum into
// one fma — also when they are spelled __fmul_rn and __fadd_rn, which the HIP headers define as plain operators compiled under
// that default (measured here: contrast and saturation came out one ulp off the separately rounded model).  So the chain uses
// the three below, compiled with contraction off, and nothing from here to the end of a file that includes this header is
// fused (as in mesh.hip, optim.hip and upsample.hip).  Include it after the headers whose device functions are meant to fuse.
#pragma clang fp contract(off)

namespace pnr {

__device__ __forceinline__ float jadd(float a, float b) { return a + b; }
__device__ __forceinline__ float jsub(float a, float b) { return a - b; }
__device__ __forceinline__ float jmul(float a, float b) { return a * b; }

enum { JIT_BRIGHTNESS = 0, JIT_CONTRAST = 1, JIT_SATURATION = 2, JIT_HUE = 3 };

struct JitterRec {
    float brightness, contrast, saturation, hue, mean;
    uint32_t order;                                     // operation k of the chain in bits [4 k, 4 k + 4)
};

// The Lehmer code q in [0, 24) over [brightness, contrast, saturation, hue]: q / 6, then (q % 6) / 2, then q % 2, each picking
// from what is left (kept as nibbles, lowest first).
__device__ __forceinline__ uint32_t jitter_order(uint32_t q) {
    const uint32_t pick[3] = {q / 6u, (q % 6u) / 2u, q % 2u};
    uint32_t left = 0x3210u, out = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t sh = 4u * pick[k];
        out |= ((left >> sh) & 15u) << (4 * k);
        left = ((left >> (sh + 4u)) << sh) | (left & ((1u << sh) - 1u));
    }
    return out | ((left & 15u) << 12);
}

// row: the 8 floats of a record.  An order code outside [0, 24) (or NaN) counts as 0.
__device__ __forceinline__ JitterRec jitter_load(const float* __restrict__ row) {
    const float q = row[5];
    return {row[0], row[1], row[2], row[3], row[4], jitter_order(q >= 0.0f && q < 24.0f ? (uint32_t)q : 0u)};
}

__device__ __forceinline__ float jitter_gray(float r, float g, float b) {
    return jadd(jadd(jmul(0.2989f, r), jmul(0.587f, g)), jmul(0.114f, b));
}

// clamp(f x + w y): the blend brightness (w = 0 is left out by its caller), contrast and saturation share
__device__ __forceinline__ float jitter_blend(float f, float x, float wy) { return clamp01(jadd(jmul(f, x), wy)); }

__device__ __forceinline__ void jitter_hue(float h, float& r, float& g, float& b) {
    const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
    const bool eq = maxc == minc;
    const float cr = jsub(maxc, minc);
    const float s = __fdiv_rn(cr, eq ? 1.0f : maxc);
    const float d = eq ? 1.0f : cr;
    const float rc = __fdiv_rn(jsub(maxc, r), d), gc = __fdiv_rn(jsub(maxc, g), d), bc = __fdiv_rn(jsub(maxc, b), d);
    const bool is_r = maxc == r, is_g = maxc == g && !is_r, is_b = !(maxc == g) && !is_r;
    const float hr = is_r ? jsub(bc, gc) : 0.0f;
    const float hg = is_g ? jsub(jadd(2.0f, rc), bc) : 0.0f;
    const float hb = is_b ? jsub(jadd(4.0f, gc), rc) : 0.0f;
    float H = jadd(__fdiv_rn(jadd(jadd(hr, hg), hb), 6.0f), 1.0f);      // in [5/6, 11/6]
    H = H >= 1.0f ? jsub(H, 1.0f) : H;             // fmod(H, 1) on that interval; the difference is exact
    const float t = jadd(H, h);
    H = jsub(t, floorf(t));
    if (H == 1.0f) H = 0.0f;                            // t just below 0: t + 1 rounds to 1
    const float h6 = jmul(H, 6.0f);
    const float fi = floorf(h6);
    const float f = jsub(h6, fi);
    const int i = (fi >= 0.0f && fi < 7.0f ? (int)fi : 0) % 6;
    const float v = maxc;
    const float p = clamp01(jmul(v, jsub(1.0f, s)));
    const float q = clamp01(jmul(v, jsub(1.0f, jmul(s, f))));
    const float u = clamp01(jmul(v, jsub(1.0f, jmul(s, jsub(1.0f, f)))));
    r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? u : v;
    g = i == 0 ? u : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
    b = i == 0 ? p : i == 1 ? p : i == 2 ? u : i == 3 ? v : i == 4 ? v : q;
}

// The record's operations in its order on one pixel in [0, 1]; an operation whose factor is exactly its identity is skipped, so
// an identity record leaves the pixel's bits alone.  UNTIL_CONTRAST: stop in front of contrast (what the mean is taken over).
template <bool UNTIL_CONTRAST> __device__ __forceinline__ void jitter_chain(const JitterRec& j, float& r, float& g, float& b) {
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const uint32_t op = (j.order >> (4 * k)) & 15u;
        if (op == JIT_BRIGHTNESS) {
            if (j.brightness != 1.0f) {
                r = clamp01(jmul(j.brightness, r)); g = clamp01(jmul(j.brightness, g)); b = clamp01(jmul(j.brightness, b));
            }
        } else if (op == JIT_CONTRAST) {
            if (UNTIL_CONTRAST) return;
            if (j.contrast != 1.0f) {
                const float wm = jmul(jsub(1.0f, j.contrast), j.mean);
                r = jitter_blend(j.contrast, r, wm); g = jitter_blend(j.contrast, g, wm); b = jitter_blend(j.contrast, b, wm);
            }
        } else if (op == JIT_SATURATION) {
            if (j.saturation != 1.0f) {
                const float wg = jmul(jsub(1.0f, j.saturation), jitter_gray(r, g, b));
                r = jitter_blend(j.saturation, r, wg); g = jitter_blend(j.saturation, g, wg); b = jitter_blend(j.saturation, b, wg);
            }
        } else {
            if (j.hue != 0.0f) jitter_hue(j.hue, r, g, b);
        }
    }
}

}  // namespace pnr
