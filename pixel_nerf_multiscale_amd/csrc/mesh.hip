// Mesh extraction where the density lies (reference util/recon.py: marching_cubes with util.gen_grid, and PyMCubes behind it):
// the grid points the network is asked at, and marching cubes over the sigma column of its answer, from the field to the
// indexed triangle list.  Output sizes depend on the data, so the work is two calls with ONE host read between them:
//   pnr_mc_count   k_mc_classify  per grid point: the case of its cell and its three owned-edge flags; per workgroup the totals
//                  k_mc_scan_totals  ONE workgroup: exclusive scan of the workgroup totals, in place, and the two counts
//                  k_mc_apply     per grid point: its vertex and triangle offsets
//   pnr_mc_emit    k_mc_emit      per grid point: its own vertices and its cell's triangles
// Integer scans in a fixed order, no atomics, no workgroup waits on another: the result is the one a sequential walk gives.
#include "pnr_common.h"

#define PNR_MC_TABLE_DECL __device__ __attribute__((aligned(16))) const
#include "mc_tables.h"

// Nothing in this file may be fused: the grid and the vertices reproduce numpy's separately rounded fp64 operations, and
// hipcc's default -ffp-contract=fast turns a product and a sum into one fma — also when they are spelled __dmul_rn and
// __dadd_rn, which the HIP headers define as plain operators compiled under that default: 3 * (2 / 6) - 1 is 0 in numpy
// and -5.6e-17 fused.  So the fp64 arithmetic below uses these four, compiled with contraction off.
#pragma clang fp contract(off)

namespace pnr {

__device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__device__ __forceinline__ double dsub(double a, double b) { return a - b; }
__device__ __forceinline__ double dmul(double a, double b) { return a * b; }
__device__ __forceinline__ double ddiv(double a, double b) { return a / b; }

constexpr int MC_THREADS = 256;                       // 4 waves
constexpr int MC_PER_THREAD = 4;                      // consecutive grid points of one thread
constexpr int MC_BLOCK = MC_THREADS * MC_PER_THREAD;  // grid points (and, in k_mc_scan_totals, workgroup totals) per scan step
constexpr int64_t MC_MAX_POINTS = (int64_t)1 << 28;   // 5 triangles per cell and 3 vertices per point stay inside int32

struct McGrid {
    const float* field; int64_t stride;
    int nx, ny, nz;
    int64_t n;                                        // nx * ny * nz
    double iso;
};

// Workspace of n grid points, B = ceil(n / MC_BLOCK) workgroups (every array padded to whole workgroups, so the 4-wide stores
// of a thread never need a tail): code uint16 | voff uint32 | toff uint32 | block totals uint2 (padded to MC_BLOCK entries).
struct McWs { uint16_t* code; uint32_t* voff; uint32_t* toff; uint2* blk; };
static inline int64_t mc_blocks(int64_t n) { return (n + MC_BLOCK - 1) / MC_BLOCK; }
static inline McWs mc_carve(Bump& b, int64_t n) {
    const int64_t B = mc_blocks(n), npad = B * MC_BLOCK, bpad = (B + MC_BLOCK - 1) / MC_BLOCK * MC_BLOCK;
    McWs w;
    w.code = b.take<uint16_t>(npad);
    w.voff = b.take<uint32_t>(npad);
    w.toff = b.take<uint32_t>(npad);
    w.blk = b.take<uint2>(bpad);
    return w;
}
static inline McWs mc_carve(const void* ws, int64_t n) { Bump b(const_cast<void*>(ws)); return mc_carve(b, n); }
static inline uint64_t mc_ws_bytes(int64_t n) { return bytes_of([&](Bump& b) { mc_carve(b, n); }); }

// code: bits 0-7 the cell's case (0 for a point that is no cell origin), bits 8-10 the owned-edge flags (axis 0, 1, 2)
__device__ __forceinline__ int code_flags(uint32_t code) { return (int)(code >> 8) & 7; }
__device__ __forceinline__ int code_case(uint32_t code) { return (int)code & 255; }

// One row of the table per thread into LDS; the caller synchronises.
__device__ __forceinline__ void load_table(uint4* tab, int tid) { tab[tid] = ((const uint4*)PNR_MC_TABLE)[tid]; }
__device__ __forceinline__ int table_ntri(const uint4* tab, int cs) { return (int)(tab[cs].w >> 24); }
__device__ __forceinline__ int table_edge(const uint4& row, int b) {
    const uint32_t w = b < 4 ? row.x : b < 8 ? row.y : b < 12 ? row.z : row.w;
    return (int)(w >> ((b & 3) * 8)) & 255;
}

// Exclusive scan over the workgroup of a packed pair (vertices in the low word, triangles in the high word: neither total
// of one launch reaches 2^31).  Returns the exclusive prefix; `total` is the workgroup's sum, the same in every thread.
__device__ __forceinline__ uint64_t block_scan_excl(uint64_t v, uint64_t* wave_tot, int tid, uint64_t& total) {
    const int lane = tid & 63, wave = tid >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MC_THREADS / 64; ++w) {
        const uint64_t t = wave_tot[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();                                  // wave_tot may be written again by the caller's next scan
    total = all;
    return before + inc - v;
}

__device__ __forceinline__ bool mc_inside(const McGrid& g, int64_t p) { return (double)g.field[p * g.stride] >= g.iso; }

__global__ void __launch_bounds__(MC_THREADS) k_mc_classify(McGrid g, McWs w) {
    __shared__ uint4 tab[256];
    __shared__ uint64_t wave_tot[MC_THREADS / 64];
    const int tid = threadIdx.x;
    load_table(tab, tid);
    __syncthreads();
    const int64_t p0 = ((int64_t)blockIdx.x * MC_THREADS + tid) * MC_PER_THREAD;
    const int64_t sj = g.nz, si = (int64_t)g.ny * g.nz;
    uint32_t codes[MC_PER_THREAD];
    uint64_t mine = 0;
#pragma unroll
    for (int r = 0; r < MC_PER_THREAD; ++r) {
        const int64_t p = p0 + r;
        uint32_t code = 0;
        if (p < g.n) {
            const int k = (int)(p % g.nz), j = (int)((p / g.nz) % g.ny), i = (int)(p / si);
            const bool hi = i + 1 < g.nx, hj = j + 1 < g.ny, hk = k + 1 < g.nz;
            const bool c0 = mc_inside(g, p);
            const bool c1 = hi && mc_inside(g, p + si), c2 = hj && mc_inside(g, p + sj), c4 = hk && mc_inside(g, p + 1);
            const int flags = (hi && c1 != c0 ? 1 : 0) | (hj && c2 != c0 ? 2 : 0) | (hk && c4 != c0 ? 4 : 0);
            int cs = 0;
            if (hi && hj && hk) {
                const bool c3 = mc_inside(g, p + si + sj), c5 = mc_inside(g, p + si + 1), c6 = mc_inside(g, p + sj + 1);
                const bool c7 = mc_inside(g, p + si + sj + 1);
                cs = (int)c0 | (int)c1 << 1 | (int)c2 << 2 | (int)c3 << 3 | (int)c4 << 4 | (int)c5 << 5 | (int)c6 << 6 | (int)c7 << 7;
            }
            code = (uint32_t)cs | (uint32_t)flags << 8;
            mine += (uint64_t)__popc(flags) | (uint64_t)table_ntri(tab, cs) << 32;
        }
        codes[r] = code;
    }
    *(uint2*)(w.code + p0) = make_uint2(codes[0] | codes[1] << 16, codes[2] | codes[3] << 16);     // padded: always in bounds
    uint64_t total;
    block_scan_excl(mine, wave_tot, tid, total);
    if (tid == 0) w.blk[blockIdx.x] = make_uint2((uint32_t)total, (uint32_t)(total >> 32));
}

// ONE workgroup walks the totals MC_BLOCK at a time with a running carry: 2^28 points are 2^18 totals, 256 steps.
__global__ void __launch_bounds__(MC_THREADS) k_mc_scan_totals(uint2* blk, int64_t n_blocks, int64_t* counts) {
    __shared__ uint64_t wave_tot[MC_THREADS / 64];
    const int tid = threadIdx.x;
    uint64_t carry = 0;
    for (int64_t base = 0; base < n_blocks; base += MC_BLOCK) {
        const int64_t b0 = base + (int64_t)tid * MC_PER_THREAD;
        uint64_t v[MC_PER_THREAD], mine = 0;
#pragma unroll
        for (int r = 0; r < MC_PER_THREAD; ++r) {
            uint2 t = make_uint2(0u, 0u);
            if (b0 + r < n_blocks) t = blk[b0 + r];
            v[r] = (uint64_t)t.x | (uint64_t)t.y << 32;
            mine += v[r];
        }
        uint64_t total;
        uint64_t off = carry + block_scan_excl(mine, wave_tot, tid, total);
#pragma unroll
        for (int r = 0; r < MC_PER_THREAD; ++r) {
            if (b0 + r < n_blocks) blk[b0 + r] = make_uint2((uint32_t)off, (uint32_t)(off >> 32));
            off += v[r];
        }
        carry += total;
    }
    if (tid == 0) { counts[0] = (int64_t)(uint32_t)carry; counts[1] = (int64_t)(carry >> 32); }
}

__global__ void __launch_bounds__(MC_THREADS) k_mc_apply(McWs w) {
    __shared__ uint4 tab[256];
    __shared__ uint64_t wave_tot[MC_THREADS / 64];
    const int tid = threadIdx.x;
    load_table(tab, tid);
    __syncthreads();
    const int64_t p0 = ((int64_t)blockIdx.x * MC_THREADS + tid) * MC_PER_THREAD;
    const uint2 packed = *(const uint2*)(w.code + p0);
    const uint32_t codes[MC_PER_THREAD] = {packed.x & 0xffffu, packed.x >> 16, packed.y & 0xffffu, packed.y >> 16};
    uint64_t v[MC_PER_THREAD], mine = 0;
#pragma unroll
    for (int r = 0; r < MC_PER_THREAD; ++r) {
        v[r] = (uint64_t)__popc(code_flags(codes[r])) | (uint64_t)table_ntri(tab, code_case(codes[r])) << 32;
        mine += v[r];
    }
    uint64_t total;
    const uint2 b = w.blk[blockIdx.x];
    uint64_t off = ((uint64_t)b.x | (uint64_t)b.y << 32) + block_scan_excl(mine, wave_tot, tid, total);
    uint32_t vo[MC_PER_THREAD], to[MC_PER_THREAD];
#pragma unroll
    for (int r = 0; r < MC_PER_THREAD; ++r) {
        vo[r] = (uint32_t)off; to[r] = (uint32_t)(off >> 32);
        off += v[r];
    }
    *(uint4*)(w.voff + p0) = make_uint4(vo[0], vo[1], vo[2], vo[3]);
    *(uint4*)(w.toff + p0) = make_uint4(to[0], to[1], to[2], to[3]);
}

struct McEmit {
    double origin[3], scale[3];
    int64_t n_vertices, n_triangles;
    double* vertices; int32_t* triangles;
};

__global__ void __launch_bounds__(MC_THREADS) k_mc_emit(McGrid g, McWs w, McEmit o) {
    __shared__ uint4 tab[256];
    const int tid = threadIdx.x;
    load_table(tab, tid);
    __syncthreads();
    const int64_t p0 = ((int64_t)blockIdx.x * MC_THREADS + tid) * MC_PER_THREAD;
    const int64_t sj = g.nz, si = (int64_t)g.ny * g.nz;
    const uint2 packed = *(const uint2*)(w.code + p0);
    if ((packed.x | packed.y) == 0u) return;                       // no crossing at any of the four points (padding included)
    const uint32_t codes[MC_PER_THREAD] = {packed.x & 0xffffu, packed.x >> 16, packed.y & 0xffffu, packed.y >> 16};
#pragma unroll
    for (int r = 0; r < MC_PER_THREAD; ++r) {
        const uint32_t code = codes[r];
        if (code == 0u) continue;
        const int64_t p = p0 + r;
        if (p >= g.n) continue;                                    // only a workspace pnr_mc_count did not fill says otherwise
        const int idx[3] = {(int)(p / si), (int)((p / g.nz) % g.ny), (int)(p % g.nz)};
        const bool hi = idx[0] + 1 < g.nx, hj = idx[1] + 1 < g.ny, hk = idx[2] + 1 < g.nz;
        const int flags = code_flags(code) & ((hi ? 1 : 0) | (hj ? 2 : 0) | (hk ? 4 : 0));
        const int cs = hi && hj && hk ? code_case(code) : 0;
        if (flags) {
            const int64_t step[3] = {si, sj, 1};
            const double fa = (double)g.field[p * g.stride];
            int64_t vid = w.voff[p];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(flags >> a & 1)) continue;
                const double fb = (double)g.field[(p + step[a]) * g.stride];
                const double t = ddiv(dsub(g.iso, fa), dsub(fb, fa));
                if (vid < o.n_vertices) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double x = c == a ? dadd((double)idx[c], t) : (double)idx[c];
                        o.vertices[vid * 3 + c] = dadd(dmul(x, o.scale[c]), o.origin[c]);
                    }
                }
                ++vid;
            }
        }
        const uint4 row = tab[cs];
        const int nt = (int)(row.w >> 24);
        const int64_t t0 = w.toff[p];
        for (int t = 0; t < nt; ++t) {
            if (t0 + t >= o.n_triangles) break;
            int32_t vi[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int e = table_edge(row, t * 3 + m), axis = e >> 2, slot = e & 3;
                // the edge's lower corner: the slot-th corner whose `axis` bit is clear
                const int c = axis == 0 ? slot << 1 : axis == 1 ? (slot & 1) | (slot >> 1) << 2 : slot;
                const int64_t q = p + (c & 1) * si + (c >> 1 & 1) * sj + (c >> 2 & 1);
                const int qf = code_flags(w.code[q]);
                vi[m] = (int32_t)(w.voff[q] + (uint32_t)__popc(qf & ((1 << axis) - 1)));
            }
            int32_t* dst = o.triangles + (t0 + t) * 3;
            dst[0] = vi[0]; dst[1] = vi[1]; dst[2] = vi[2];
        }
    }
}

// ---------------------------------------------------------------- the grid (util.gen_grid, ij indexing) and the fake view directions
struct GridArgs {
    double lo[3], hi[3], step[3];
    int n[3];
    int64_t first, count;
    float* xyz; float* dirs;
};

// np.linspace(lo, hi, n, dtype=float32)[i]: i * step + lo in fp64, unfused, the last sample hi itself, then ONE rounding
__device__ __forceinline__ float linspace_f32(const GridArgs& a, int c, int i) {
    double v = dadd(dmul((double)i, a.step[c]), a.lo[c]);
    if (a.n[c] > 1 && i == a.n[c] - 1) v = a.hi[c];
    return (float)v;
}

__global__ void __launch_bounds__(MC_THREADS) k_grid_points(GridArgs a) {
    const int64_t t = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= a.count) return;
    const int64_t p = a.first + t;
    const int k = (int)(p % a.n[2]), j = (int)((p / a.n[2]) % a.n[1]), i = (int)(p / ((int64_t)a.n[1] * a.n[2]));
    const float x = linspace_f32(a, 0, i), y = linspace_f32(a, 1, j), z = linspace_f32(a, 2, k);
    a.xyz[t * 3 + 0] = x; a.xyz[t * 3 + 1] = y; a.xyz[t * 3 + 2] = z;
    if (a.dirs) {
        // -p / |p| (recon.py:54); the origin itself gets (0, 0, 0) where the reference's 0 / 0 is NaN
        const float nrm = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
        const bool ok = nrm > 0.0f;
        a.dirs[t * 3 + 0] = ok ? __fdiv_rn(-x, nrm) : 0.0f;
        a.dirs[t * 3 + 1] = ok ? __fdiv_rn(-y, nrm) : 0.0f;
        a.dirs[t * 3 + 2] = ok ? __fdiv_rn(-z, nrm) : 0.0f;
    }
}

static inline int32_t mc_check(const float* field, int32_t stride, int32_t nx, int32_t ny, int32_t nz, const void* ws,
                               uint64_t ws_bytes) {
    if (!field || !ws) return PNR_E_NULL;
    if (nx < 2 || ny < 2 || nz < 2 || stride < 1) return PNR_E_SHAPE;
    if ((int64_t)nx * ny > MC_MAX_POINTS || (int64_t)nx * ny * nz > MC_MAX_POINTS) return PNR_E_SHAPE;
    if (ws_bytes < mc_ws_bytes((int64_t)nx * ny * nz)) return PNR_E_WORKSPACE;
    if ((uintptr_t)ws & 15) return PNR_E_ALIGN;
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

static_assert(sizeof(PNR_MC_TABLE) == 256 * sizeof(uint4), "one 16-byte row per case");

extern "C" uint64_t pnr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    if ((int64_t)nx * ny > MC_MAX_POINTS || (int64_t)nx * ny * nz > MC_MAX_POINTS) return 0;
    return mc_ws_bytes((int64_t)nx * ny * nz);
}

extern "C" int32_t pnr_mc_count(const float* field, int32_t stride, int32_t nx, int32_t ny, int32_t nz, double iso, void* workspace,
                                uint64_t workspace_bytes, int64_t* counts, void* stream) {
    if (!counts) return PNR_E_NULL;
    PNR_TRY(mc_check(field, stride, nx, ny, nz, workspace, workspace_bytes));
    McGrid g;
    g.field = field; g.stride = stride; g.nx = nx; g.ny = ny; g.nz = nz; g.n = (int64_t)nx * ny * nz; g.iso = iso;
    const McWs w = mc_carve(workspace, g.n);
    const int64_t B = mc_blocks(g.n);
    hipLaunchKernelGGL(k_mc_classify, dim3((unsigned)B), dim3(MC_THREADS), 0, (hipStream_t)stream, g, w);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mc_scan_totals, dim3(1), dim3(MC_THREADS), 0, (hipStream_t)stream, w.blk, B, counts);
    PNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mc_apply, dim3((unsigned)B), dim3(MC_THREADS), 0, (hipStream_t)stream, w);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_mc_emit(const float* field, int32_t stride, int32_t nx, int32_t ny, int32_t nz, double iso,
                               const double* origin, const double* scale, const void* workspace, uint64_t workspace_bytes,
                               int64_t n_vertices, int64_t n_triangles, double* vertices, int32_t* triangles, void* stream) {
    if (!origin || !scale) return PNR_E_NULL;
    PNR_TRY(mc_check(field, stride, nx, ny, nz, workspace, workspace_bytes));
    if (n_vertices < 0 || n_triangles < 0 || n_vertices > 3 * MC_MAX_POINTS || n_triangles > 5 * MC_MAX_POINTS) return PNR_E_SHAPE;
    if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles)) return PNR_E_NULL;
    if (n_vertices == 0 && n_triangles == 0) return PNR_OK;
    McGrid g;
    g.field = field; g.stride = stride; g.nx = nx; g.ny = ny; g.nz = nz; g.n = (int64_t)nx * ny * nz; g.iso = iso;
    McEmit o;
    for (int c = 0; c < 3; ++c) { o.origin[c] = origin[c]; o.scale[c] = scale[c]; }
    o.n_vertices = n_vertices; o.n_triangles = n_triangles; o.vertices = vertices; o.triangles = triangles;
    hipLaunchKernelGGL(k_mc_emit, dim3((unsigned)mc_blocks(g.n)), dim3(MC_THREADS), 0, (hipStream_t)stream, g,
                       mc_carve(workspace, g.n), o);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_grid_points(const double* c1, const double* c2, const int32_t* reso, int64_t first, int64_t count,
                                   int32_t fake_viewdirs, float* xyz_out, float* viewdirs_out, void* stream) {
    if (!c1 || !c2 || !reso || !xyz_out || (fake_viewdirs && !viewdirs_out)) return PNR_E_NULL;
    if (reso[0] < 1 || reso[1] < 1 || reso[2] < 1) return PNR_E_SHAPE;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)reso[0] * reso[1] >= lim || (int64_t)reso[0] * reso[1] * reso[2] >= lim) return PNR_E_SHAPE;
    const int64_t n = (int64_t)reso[0] * reso[1] * reso[2];
    if (first < 0 || count < 0 || first > n || count > n - first) return PNR_E_SHAPE;
    if (count == 0) return PNR_OK;
    GridArgs a;
    for (int c = 0; c < 3; ++c) {
        a.lo[c] = c1[c]; a.hi[c] = c2[c]; a.n[c] = reso[c];
        a.step[c] = reso[c] > 1 ? (c2[c] - c1[c]) / (double)(reso[c] - 1) : 0.0;
    }
    a.first = first; a.count = count; a.xyz = xyz_out; a.dirs = fake_viewdirs ? viewdirs_out : nullptr;
    hipLaunchKernelGGL(k_grid_points, dim3((unsigned)((count + MC_THREADS - 1) / MC_THREADS)), dim3(MC_THREADS), 0,
                       (hipStream_t)stream, a);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
