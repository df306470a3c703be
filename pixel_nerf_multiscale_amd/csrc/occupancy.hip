// Empty-space culling in front of the render launch (include/pnr.h, "empty-space culling"): a bit grid of occupied cells from
// sigma samples, the rays of a batch of frames turned into each frame's ordered list of rays that hit an occupied cell, with
// their [near, far] tightened to the occupied stretch, and the gather that puts the rendered hits back into whole frames.
//   pnr_occ_build        k_occ_build   per word of the bit grid: 32 cells along z, dilation included; no atomics
//   pnr_ray_bounds       k_rb_trace    per ray: clip, walk the cells (Amanatides & Woo), bounds; per workgroup the hit count
//                        k_rb_scan     ONE workgroup per frame: exclusive scan of its workgroups' counts, and the frame's count
//                        k_rb_emit     per ray: its slot, and its row of the frame's compact list
//   pnr_frame_from_hits  k_frame_from_hits  per pixel: background, or its record
// Integer scans in a fixed order, no atomics, no workgroup waits on another: the lists are the ones a sequential walk gives.
#include "pnr_common.h"

// The header states every fp32 operation of the traversal and its order; a fused multiply-add would be another rounding.
#pragma clang fp contract(off)

namespace pnr {

constexpr int OCC_THREADS = 256;                      // 4 waves
constexpr int OCC_MAX_DILATE = 4;
constexpr int OCC_MAX_CELLS = 1 << 20;                // per axis: cx + cy + cz + 3 steps stay far inside int32
constexpr int64_t OCC_MAX_WORDS = (int64_t)1 << 31;   // words of one grid
constexpr int64_t RB_MAX_BLOCKS = ((int64_t)1 << 31) - 1;

static inline int occ_wz(int cz) { return (cz + 31) >> 5; }

// ---------------------------------------------------------------- the bit grid
struct OccField {
    const float* field; int64_t stride;
    int nx, ny, nz;
    double thresh;
};
// a sample is hot iff (double)f >= thresh or f is NaN: everything that is not certainly below the threshold
__device__ __forceinline__ bool occ_hot(const OccField& g, int64_t p) { return !((double)g.field[p * g.stride] < g.thresh); }

// Cell c is occupied iff a raw-occupied cell c' with |c' - c| <= dilate (every axis) exists, and c' is raw-occupied iff one of
// its corner samples c' .. c' + 1 is hot: together, iff a hot sample lies in [c - dilate, c + dilate + 1] on every axis
// (clipped to the lattice: the corners of the cells that exist are exactly the samples that exist).  A thread ORs the hot
// samples of that box's (i, j) columns into one 64-bit column mask along z, then a bit of its word is 2 * dilate + 2
// neighbouring bits of the mask.
__global__ void __launch_bounds__(OCC_THREADS) k_occ_build(OccField g, int dilate, int accumulate, int wz, int64_t n_words,
                                                           uint32_t* bits) {
    const int64_t w = (int64_t)blockIdx.x * OCC_THREADS + threadIdx.x;
    if (w >= n_words) return;
    const int cy = g.ny - 1, cz = g.nz - 1;
    const int kw = (int)(w % wz), j = (int)((w / wz) % cy), i = (int)(w / ((int64_t)wz * cy));
    const int i0 = max(i - dilate, 0), i1 = min(i + dilate + 1, g.nx - 1);
    const int j0 = max(j - dilate, 0), j1 = min(j + dilate + 1, g.ny - 1);
    const int zb = kw * 32 - dilate;                                  // the sample of the mask's bit 0
    const int z0 = max(zb, 0), z1 = min(kw * 32 + 32 + dilate, g.nz - 1);   // at most 33 + 2 * dilate <= 41 bits
    uint64_t m = 0;
    for (int ii = i0; ii <= i1; ++ii) {
        for (int jj = j0; jj <= j1; ++jj) {
            const int64_t base = ((int64_t)ii * g.ny + jj) * g.nz;
            for (int z = z0; z <= z1; ++z)
                if (occ_hot(g, base + z)) m |= (uint64_t)1 << (z - zb);
        }
    }
    uint64_t any = 0;
    for (int s = 0; s <= 2 * dilate + 1; ++s) any |= m >> s;          // cell k of the word: samples zb + k .. zb + k + 2 dilate + 1
    uint32_t word = (uint32_t)any;
    const int valid = cz - kw * 32;                                   // cells of this word that exist (>= 1)
    if (valid < 32) word &= ((uint32_t)1 << valid) - 1u;
    if (accumulate) word |= bits[w];
    bits[w] = word;
}

// ---------------------------------------------------------------- the traversal
struct RbGrid {
    float lo[3], hi[3], h[3], inv_h[3];
    int n[3];                                         // cells per axis
    int wz;
    const uint32_t* bits;
    float pad;
};

// min / max by ONE comparison each (fminf / fmaxf leave the sign of a zero open): b where it is strictly smaller / larger
__device__ __forceinline__ float min_s(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float max_s(float a, float b) { return b > a ? b : a; }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and Inf

__device__ __forceinline__ bool rb_occupied(const RbGrid& g, int ci, int cj, int ck) {
    const uint32_t word = g.bits[((int64_t)ci * g.n[1] + cj) * g.wz + (ck >> 5)];
    return (word >> (ck & 31)) & 1u;
}
// coordinate of cell boundary b (0 .. n) of an axis: the last one is hi itself
__device__ __forceinline__ float rb_boundary(float lo, float hi, float h, int n, int b) {
    return b == n ? hi : lo + (float)b * h;
}

// -> hit; nf = the tightened (near, far).  pnr.h states this function step by step.
__device__ __forceinline__ bool rb_trace(const RbGrid& g, const float4 ra, const float4 rb, float2& nf) {
    const float o[3] = {ra.x, ra.y, ra.z}, d[3] = {ra.w, rb.x, rb.y};
    const float near = rb.z, far = rb.w;
    bool ok = finite_f(near) && finite_f(far);
#pragma unroll
    for (int a = 0; a < 3; ++a) ok = ok && finite_f(o[a]) && finite_f(d[a]);
    if (!ok) return false;
    if (d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f) return false;
    if (near > far) return false;
    float t0 = near, t1 = far;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (d[a] == 0.0f) {
            if (o[a] < g.lo[a] || o[a] > g.hi[a]) return false;
        } else {
            const float ta = __fdiv_rn(g.lo[a] - o[a], d[a]), tb = __fdiv_rn(g.hi[a] - o[a], d[a]);
            t0 = max_s(t0, min_s(ta, tb));
            t1 = min_s(t1, max_s(ta, tb));
        }
    }
    if (t0 > t1) return false;
    int c[3], step[3];
    float tmax[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = o[a] + t0 * d[a];
        float f = floorf((p - g.lo[a]) * g.inv_h[a]);
        f = min_s((float)(g.n[a] - 1), max_s(0.0f, f));               // f where 0 < f < n - 1, else the bound
        c[a] = min(max((int)f, 0), g.n[a] - 1);                       // (the integer clamp changes nothing: f is in range)
        step[a] = d[a] > 0.0f ? 1 : d[a] < 0.0f ? -1 : 0;
        tmax[a] = step[a] == 0 ? __builtin_inff()
                               : __fdiv_rn(rb_boundary(g.lo[a], g.hi[a], g.h[a], g.n[a], c[a] + (step[a] > 0 ? 1 : 0)) - o[a], d[a]);
    }
    bool hit = false;
    float t_in = 0.0f, t_out = 0.0f, t_cur = t0;
    const int max_steps = g.n[0] + g.n[1] + g.n[2] + 3;               // a walk changes one index by one per step: it cannot be longer
    for (int s = 0; s < max_steps; ++s) {
        const float tm = min_s(min_s(tmax[0], tmax[1]), tmax[2]);
        const float te = max_s(min_s(tm, t1), t_cur);                 // where the segment leaves this cell
        if (rb_occupied(g, c[0], c[1], c[2])) {
            if (!hit) { t_in = t_cur; hit = true; }
            t_out = te;
        }
        if (!(tm < t1)) break;                                        // the segment ends inside this cell
        const int axis = (tmax[0] <= tmax[1] && tmax[0] <= tmax[2]) ? 0 : (tmax[1] <= tmax[2] ? 1 : 2);
        bool left = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (a != axis) continue;
            c[a] += step[a];
            if (step[a] == 0 || c[a] < 0 || c[a] >= g.n[a]) { left = true; continue; }
            tmax[a] = __fdiv_rn(rb_boundary(g.lo[a], g.hi[a], g.h[a], g.n[a], c[a] + (step[a] > 0 ? 1 : 0)) - o[a], d[a]);
        }
        if (left) break;
        t_cur = te;
    }
    if (!hit) return false;
    nf.x = max_s(near, t_in - g.pad);
    nf.y = min_s(far, t_out + g.pad);
    return true;
}

// Workspace of n rays in F frames of bpf = ceil(R / OCC_THREADS) workgroups each: bounds float2 (n) | workgroup counts uint32 (F bpf)
struct RbWs { float2* bounds; uint32_t* blk; };
static inline int64_t rb_bpf(int64_t R) { return (R + OCC_THREADS - 1) / OCC_THREADS; }
static inline RbWs rb_carve(Bump& b, int64_t n, int64_t R) {
    RbWs w;
    w.bounds = b.take<float2>((uint64_t)n, 16);
    w.blk = b.take<uint32_t>((uint64_t)((n / R) * rb_bpf(R)), 16);
    b.pad(16);
    return w;
}
static inline uint64_t rb_ws_bytes(int64_t n, int64_t R) { return bytes_of([&](Bump& b) { rb_carve(b, n, R); }); }

// Exclusive scan of one uint32 per thread over the workgroup; `total` the same in every thread.
__device__ __forceinline__ uint32_t block_scan_excl_u32(uint32_t v, uint32_t* wave_tot, int tid, uint32_t& total) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < OCC_THREADS / 64; ++w) {
        const uint32_t t = wave_tot[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();                                  // wave_tot may be written again by the caller's next scan
    total = all;
    return before + inc - v;
}

// workgroup blockIdx.x = f * bpf + b owns rays f R + b OCC_THREADS + tid of frame f
__global__ void __launch_bounds__(OCC_THREADS) k_rb_trace(RbGrid g, const float4* rays, int64_t R, int64_t bpf, RbWs w, int32_t* slot) {
    __shared__ uint32_t wave_tot[OCC_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t f = blockIdx.x / bpf, j = (blockIdx.x % bpf) * OCC_THREADS + tid;
    const bool live = j < R;
    const int64_t i = f * R + j;
    bool hit = false;
    if (live) {
        float2 nf = make_float2(0.0f, 0.0f);
        hit = rb_trace(g, rays[i * 2], rays[i * 2 + 1], nf);
        w.bounds[i] = nf;
    }
    uint32_t total;
    const uint32_t excl = block_scan_excl_u32(hit ? 1u : 0u, wave_tot, tid, total);
    if (live) slot[i] = hit ? (int32_t)excl : -1;                     // within the workgroup; k_rb_emit adds what lies in front
    if (tid == 0) w.blk[blockIdx.x] = total;
}

// ONE workgroup per frame walks the frame's bpf counts OCC_THREADS at a time with a running carry.
__global__ void __launch_bounds__(OCC_THREADS) k_rb_scan(uint32_t* blk, int64_t bpf, int64_t* counts) {
    __shared__ uint32_t wave_tot[OCC_THREADS / 64];
    const int tid = threadIdx.x;
    uint32_t* mine = blk + (int64_t)blockIdx.x * bpf;
    uint32_t carry = 0;
    for (int64_t base = 0; base < bpf; base += OCC_THREADS) {
        const int64_t b = base + tid;
        const uint32_t v = b < bpf ? mine[b] : 0u;
        uint32_t total;
        const uint32_t off = carry + block_scan_excl_u32(v, wave_tot, tid, total);
        if (b < bpf) mine[b] = off;
        carry += total;
    }
    if (tid == 0) counts[blockIdx.x] = (int64_t)carry;
}

__global__ void __launch_bounds__(OCC_THREADS) k_rb_emit(const float4* rays, int64_t R, int64_t bpf, RbWs w, int32_t* slot, float4* rays_out) {
    const int64_t f = blockIdx.x / bpf, j = (blockIdx.x % bpf) * OCC_THREADS + threadIdx.x;
    if (j >= R) return;
    const int64_t i = f * R + j;
    const int32_t local = slot[i];
    if (local < 0) return;
    const int64_t s = (int64_t)w.blk[blockIdx.x] + local;             // < R: a count of this frame's rays in front of ray j
    if (s >= R) return;                                               // only a workspace k_rb_scan did not fill says otherwise
    slot[i] = (int32_t)s;
    const float2 nf = w.bounds[i];
    const float4 rb = rays[i * 2 + 1];
    rays_out[(f * R + s) * 2] = rays[i * 2];
    rays_out[(f * R + s) * 2 + 1] = make_float4(rb.x, rb.y, nf.x, nf.y);
}

// ---------------------------------------------------------------- the gather
__global__ void __launch_bounds__(OCC_THREADS) k_frame_from_hits(const float* rec, int64_t rec_stride, const int32_t* slot, int64_t n,
                                                                 int64_t R, float bg, float* out, int64_t out_stride) {
    const int64_t i = (int64_t)blockIdx.x * OCC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t s = slot[i];
    float4 v = make_float4(bg, bg, bg, 0.0f);
    if (s >= 0 && s < R) {                                            // a slot past the frame can only come from a foreign buffer
        const float* r = rec + ((i / R) * R + s) * rec_stride;
        v = make_float4(r[0], r[1], r[2], r[3]);
    }
    float* o = out + i * out_stride;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

static inline bool finite_d(double v) { return v - v == 0.0; }

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_occ_build(const float* field, int32_t stride, int32_t nx, int32_t ny, int32_t nz, double thresh,
                                 int32_t dilate, int32_t accumulate, uint32_t* bits, void* stream) {
    if (!field || !bits) return PNR_E_NULL;
    if (nx < 2 || ny < 2 || nz < 2 || stride < 1 || dilate < 0 || dilate > OCC_MAX_DILATE) return PNR_E_SHAPE;
    if (nx - 1 > OCC_MAX_CELLS || ny - 1 > OCC_MAX_CELLS || nz - 1 > OCC_MAX_CELLS) return PNR_E_SHAPE;
    const int wz = occ_wz(nz - 1);
    if ((int64_t)(nx - 1) * (ny - 1) >= OCC_MAX_WORDS || (int64_t)(nx - 1) * (ny - 1) * wz >= OCC_MAX_WORDS) return PNR_E_SHAPE;
    if ((int64_t)nx * ny >= OCC_MAX_WORDS || (int64_t)nx * ny * nz >= OCC_MAX_WORDS) return PNR_E_SHAPE;
    if (((uintptr_t)field & 3) || ((uintptr_t)bits & 3)) return PNR_E_ALIGN;
    const int64_t n_words = (int64_t)(nx - 1) * (ny - 1) * wz;
    OccField g;
    g.field = field; g.stride = stride; g.nx = nx; g.ny = ny; g.nz = nz; g.thresh = thresh;
    hipLaunchKernelGGL(k_occ_build, dim3((unsigned)((n_words + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0,
                       (hipStream_t)stream, g, (int)dilate, (int)accumulate, wz, n_words, bits);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

static inline int32_t rb_sizes_ok(int64_t n, int64_t R) {
    if (n < 0 || R < 1 || n >= ((int64_t)1 << 31) || R >= ((int64_t)1 << 31) || n % R != 0) return 0;
    return (n / R) * rb_bpf(R) <= RB_MAX_BLOCKS;
}

extern "C" uint64_t pnr_ray_bounds_workspace_bytes(int64_t n, int64_t rays_per_frame) {
    if (!rb_sizes_ok(n, rays_per_frame)) return 0;
    return rb_ws_bytes(n, rays_per_frame);
}

extern "C" int32_t pnr_ray_bounds(const float* rays, int64_t n, int64_t rays_per_frame, const double* c1, const double* c2,
                                  const int32_t* cells, const uint32_t* bits, double pad, void* workspace, uint64_t workspace_bytes,
                                  float* rays_out, int32_t* slot_out, int64_t* counts_out, void* stream) {
    if (!rays || !c1 || !c2 || !cells || !bits || !workspace || !rays_out || !slot_out || !counts_out) return PNR_E_NULL;
    if (!rb_sizes_ok(n, rays_per_frame)) return PNR_E_SHAPE;
    RbGrid g;
    for (int a = 0; a < 3; ++a) {
        if (cells[a] < 1 || cells[a] > OCC_MAX_CELLS) return PNR_E_SHAPE;
        if (!finite_d(c1[a]) || !finite_d(c2[a])) return PNR_E_SHAPE;
        g.lo[a] = (float)c1[a]; g.hi[a] = (float)c2[a];
        g.h[a] = (float)((c2[a] - c1[a]) / (double)cells[a]);
        g.inv_h[a] = (float)((double)cells[a] / (c2[a] - c1[a]));
        g.n[a] = cells[a];
        // the box and its cells must survive the rounding to fp32
        if (!(g.hi[a] > g.lo[a]) || !(g.h[a] > 0.0f) || !(fabsf(g.hi[a]) <= 3.402823466e+38f) || !(fabsf(g.lo[a]) <= 3.402823466e+38f) ||
            !(g.inv_h[a] > 0.0f) || !(g.inv_h[a] <= 3.402823466e+38f))
            return PNR_E_SHAPE;
    }
    g.wz = occ_wz(cells[2]);
    if ((int64_t)cells[0] * cells[1] >= OCC_MAX_WORDS || (int64_t)cells[0] * cells[1] * g.wz >= OCC_MAX_WORDS) return PNR_E_SHAPE;
    if (!(pad >= 0.0) || !finite_d(pad)) return PNR_E_SHAPE;
    g.pad = (float)pad;
    g.bits = bits;
    if (workspace_bytes < rb_ws_bytes(n, rays_per_frame)) return PNR_E_WORKSPACE;
    if (((uintptr_t)rays & 15) || ((uintptr_t)rays_out & 15) || ((uintptr_t)workspace & 15) || ((uintptr_t)bits & 3) ||
        ((uintptr_t)slot_out & 3) || ((uintptr_t)counts_out & 7))
        return PNR_E_ALIGN;
    if (n == 0) return PNR_OK;
    const int64_t R = rays_per_frame, F = n / R, bpf = rb_bpf(R);
    Bump b(workspace);
    const RbWs w = rb_carve(b, n, R);
    hipLaunchKernelGGL(k_rb_trace, dim3((unsigned)(F * bpf)), dim3(OCC_THREADS), 0, (hipStream_t)stream, g, (const float4*)rays, R, bpf,
                       w, slot_out);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rb_scan, dim3((unsigned)F), dim3(OCC_THREADS), 0, (hipStream_t)stream, w.blk, bpf, counts_out);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rb_emit, dim3((unsigned)(F * bpf)), dim3(OCC_THREADS), 0, (hipStream_t)stream, (const float4*)rays, R, bpf, w,
                       slot_out, (float4*)rays_out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_frame_from_hits(const float* rec, int32_t rec_stride, const int32_t* slot, int64_t n, int64_t rays_per_frame,
                                       float bg, float* out, int32_t out_stride, void* stream) {
    if (!rec || !slot || !out) return PNR_E_NULL;
    if (!rb_sizes_ok(n, rays_per_frame) || rec_stride < 4 || out_stride < 4) return PNR_E_SHAPE;
    if (((uintptr_t)rec & 3) || ((uintptr_t)slot & 3) || ((uintptr_t)out & 3)) return PNR_E_ALIGN;
    if (n == 0) return PNR_OK;
    hipLaunchKernelGGL(k_frame_from_hits, dim3((unsigned)((n + OCC_THREADS - 1) / OCC_THREADS)), dim3(OCC_THREADS), 0,
                       (hipStream_t)stream, rec, (int64_t)rec_stride, slot, n, rays_per_frame, bg, out, (int64_t)out_stride);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
