// Training path: PixelNeRFNet.forward with a tape + its backward, and the backward of
// the per-ray stages, in fp32.  The reference trains through autograd (train/train.py:324-346,382-410:
// calc_losses -> renderer(net) with want_weights, loss.backward()); here the same gradients are explicit
// kernels behind three C entry points that the Python autograd Functions call:
//   pnr_point_mlp_train_fwd / pnr_point_mlp_bwd   d(out) -> d(MLP weights), d(latent maps), d(z_samp|xyz)
//   pnr_composite_bwd                             d(weights,rgb,depth) -> d(rgb,sigma), d(z_samp)
//   pnr_sample_fine_bwd                           d(z_sorted) -> d(coarse depth)   (nerf.py:287-289: the
//                                                 depth-guided samples are not detached)
// Layer math (resnetfc.py:53-62,173-236):  x = lin_in(code); per block b: [combine views at
// b == combine_layer]; xin = x + lin_z_b(z); h = fc_0(relu(xin)); x = xin + fc_1(relu(h));
// out = lin_out(relu(x)); rgb = sigmoid, sigma = relu.
#include <type_traits>

#include "cam_grad.h"
#include "f32_kernels.h"

namespace pnr {

// Y[M,N] = R + mask( act(X[M,K]) op(W) + b ),  op(W)[n][k] = TRANS_W ? W[k*ldw+n] : W[n*ldw+k]
// mask: keep where Mk[m,n] > 0 (the ReLU derivative of a saved pre-activation).  R, Mk, b may be NULL; R may alias Y.
template <bool RELU_X, bool TRANS_W>
static __global__ void __launch_bounds__(256) k_gemm_f32(
    const float* __restrict__ X, int ldx, const float* __restrict__ W, int ldw, const float* __restrict__ b,
    const float* R, int ldr, const float* __restrict__ Mk, int ldm, float* Y, int ldy, int M, int N, int K) {
    __shared__ float Xs[16][64 + 4];
    __shared__ float Ws[16][64 + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int li = tid + i * 256;
            {
                int r = li >> 4, kk = li & 15;
                int m = m0 + r, k = k0 + kk;
                float xv = (m < M && k < K) ? X[(size_t)m * ldx + k] : 0.f;
                if (RELU_X) xv = fmaxf(xv, 0.f);
                Xs[kk][r] = xv;
            }
            if (TRANS_W) {
                int r = li & 63, kk = li >> 6;
                int n = n0 + r, k = k0 + kk;
                Ws[kk][r] = (n < N && k < K) ? W[(size_t)k * ldw + n] : 0.f;
            } else {
                int r = li >> 4, kk = li & 15;
                int n = n0 + r, k = k0 + kk;
                Ws[kk][r] = (n < N && k < K) ? W[(size_t)n * ldw + k] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            float xa[4], wb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { xa[i] = Xs[kk][ty * 4 + i]; wb[i] = Ws[kk][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(xa[i], wb[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int m = m0 + ty * 4 + i;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int n = n0 + tx * 4 + j;
            if (n >= N) continue;
            float v = acc[i][j];
            if (b) v += b[n];
            if (Mk && !(Mk[(size_t)m * ldm + n] > 0.f)) v = 0.f;
            if (R) v += R[(size_t)m * ldr + n];
            Y[(size_t)m * ldy + n] = v;
        }
    }
}

// dW[N,K] += sum_m dY[m,n] act(X[m,k]) over this block's row range; db[n] += sum_m dY[m,n] (k-tile 0 only).
// 64x64 output tile, 16 rows per step; every row split (grid z) stores its partial sums to its own slice (see grad_w).
template <bool RELU_X>
static __global__ void __launch_bounds__(256) k_grad_w_f32(
    const float* __restrict__ dY, int ldy, const float* __restrict__ X, int ldx, float* __restrict__ dW, int ldw,
    float* __restrict__ db, int M, int N, int K, int rows_per_split, size_t zs_w, size_t zs_b) {
    __shared__ float Ys[16][64 + 4];
    __shared__ float Xs[16][64 + 4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int n0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int mb = blockIdx.z * rows_per_split;
    const int me = min(M, mb + rows_per_split);
    float acc[4][4];
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int m0 = mb; m0 < me; m0 += 16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int li = tid + i * 256;
            int mm = li >> 6, c = li & 63;
            int m = m0 + mm;
            bool ok = m < me;
            Ys[mm][c] = (ok && n0 + c < N) ? dY[(size_t)m * ldy + n0 + c] : 0.f;
            float xv = (ok && k0 + c < K) ? X[(size_t)m * ldx + k0 + c] : 0.f;
            if (RELU_X) xv = fmaxf(xv, 0.f);
            Xs[mm][c] = xv;
        }
        __syncthreads();
#pragma unroll
        for (int mm = 0; mm < 16; ++mm) {
            float ya[4], xb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { ya[i] = Ys[mm][ty * 4 + i]; xb[i] = Xs[mm][tx * 4 + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bsum[i] += ya[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(ya[i], xb[j], acc[i][j]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int n = n0 + ty * 4 + i;
        if (n >= N) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int k = k0 + tx * 4 + j;
            if (k < K) dW[blockIdx.z * zs_w + (size_t)n * ldw + k] = acc[i][j];
        }
        if (db && blockIdx.y == 0 && tx == 0) db[blockIdx.z * zs_b + n] = bsum[i];
    }
}

// ------------------------------------------------------------------ fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32)
// C[M,N] = R + mask( sum_r act(A(m,r)) B(r,n) + bias[n] )   or   C += ... (atomics, SPLIT over r)
//   A_RC: A stored (M, R) r-contiguous (lda) — else stored (R, M) m-contiguous
//   B_RC: B stored (N, R) r-contiguous (ldb) — else stored (R, N) n-contiguous
// forward  y = x W^T   : A_RC, B_RC          dX = dY W : A_RC, !B_RC          dW = dY^T x : !A_RC, !B_RC (SPLIT)
// 128x128 tile per 256-thread block, 4 waves x (2x2) 32x32 accumulators, r-step 16 through LDS (A and B
// tiles stored r-major so a fragment read is 64 consecutive floats), register-staged global prefetch of
// the next r-tile behind the MFMAs.  One float per lane per operand: a = A[row = l%32][r = l/32],
// b = B[r = l/32][col = l%32]; acc[j] = C[8*(j/4) + 4*(l/32) + j%4][l%32].
// (the vector types of all the tile GEMMs of this section)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// Loads are unconditional (indices clamped into the operand, the value zeroed afterwards): a predicated
// load would put a branch and a full vmcnt(0) wait in front of every element.
template <bool RC>
__device__ __forceinline__ void mg_fetch(const float* __restrict__ S, int ld, int x0, int X, int r0, int r1, bool relu,
                                         float (&v)[8]) {
    const int t = threadIdx.x;
    if (RC) {           // stored (X, R): thread -> (row = t/4 + 64 i, 4 r's at 4*(t%4))
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int x = x0 + (t >> 2) + 64 * i, r = r0 + 4 * (t & 3);
            const float* p = S + (size_t)min(x, X - 1) * ld;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float val = p[min(r + e, r1 - 1)];
                val = (x < X && r + e < r1) ? val : 0.f;
                v[i * 4 + e] = relu ? fmaxf(val, 0.f) : val;
            }
        }
    } else {            // stored (R, X): thread -> (r = t/32 + 8 i, 4 x's at 4*(t%32))
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = r0 + (t >> 5) + 8 * i, x = x0 + 4 * (t & 31);
            const float* p = S + (size_t)min(r, r1 - 1) * ld;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float val = p[min(x + e, X - 1)];
                val = (r < r1 && x + e < X) ? val : 0.f;
                v[i * 4 + e] = relu ? fmaxf(val, 0.f) : val;
            }
        }
    }
}

// Interior tiles of 16-byte-aligned operands: plain float4 loads, no bounds logic.
template <bool RC>
__device__ __forceinline__ void mg_fetch_fast(const float* __restrict__ S, int ld, int x0, int r0, bool relu, float (&v)[8]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float4* p = RC ? (const float4*)(S + (size_t)(x0 + (t >> 2) + 64 * i) * ld + r0 + 4 * (t & 3))
                             : (const float4*)(S + (size_t)(r0 + (t >> 5) + 8 * i) * ld + x0 + 4 * (t & 31));
        float4 q = *p;
        v[i * 4 + 0] = relu ? fmaxf(q.x, 0.f) : q.x;
        v[i * 4 + 1] = relu ? fmaxf(q.y, 0.f) : q.y;
        v[i * 4 + 2] = relu ? fmaxf(q.z, 0.f) : q.z;
        v[i * 4 + 3] = relu ? fmaxf(q.w, 0.f) : q.w;
    }
}

template <bool RC, bool RELU>
__device__ __forceinline__ void mg_stage(float (*T)[132], float (&v)[8]) {
    const int t = threadIdx.x;
    if (RELU) {          // applied here, not at the fetch: a use right behind the load would stall on it
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
    }
    if (RC) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) T[4 * (t & 3) + e][(t >> 2) + 64 * i] = v[i * 4 + e];
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)      // rows are 528 B apart: one 16-byte store per thread, conflict-free
            *(float4*)&T[(t >> 5) + 8 * i][4 * (t & 31)] = make_float4(v[i * 4], v[i * 4 + 1], v[i * 4 + 2], v[i * 4 + 3]);
    }
}

// The output head: Y[M,4] = act(X[M,K]) W[4,K]^T + b — 4 output columns make a tile GEMM mostly padding (the 64 x 64 FMA kernel
// ran it at 0.65 TB/s of X).  One wave per row: lanes read the row as float4 (coalesced), keep their slice of W in registers,
// and the four dot products are summed over the wave; 4 rows in flight per wave.  HBM-bound: 4 K bytes per row.
template <bool RELU_X, int KQ /* K / 256 */>
static __global__ void __launch_bounds__(256) k_linear_head(const float* __restrict__ X, int ldx, const float* __restrict__ W, int ldw,
                                                            const float* __restrict__ b, float* __restrict__ Y, int ldy, int M) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
    float4 w[4][KQ];
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int q = 0; q < KQ; ++q) w[n][q] = *(const float4*)(W + (size_t)n * ldw + 256 * q + 4 * lane);
    const float b0 = b ? b[0] : 0.f, b1 = b ? b[1] : 0.f, b2 = b ? b[2] : 0.f, b3 = b ? b[3] : 0.f;
    for (int m0 = wave * 4; m0 < M; m0 += n_waves * 4) {
        float4 x[4][KQ];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + r < M ? m0 + r : M - 1;
#pragma unroll
            for (int q = 0; q < KQ; ++q) x[r][q] = *(const float4*)(X + (size_t)m * ldx + 256 * q + 4 * lane);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < KQ; ++q) {
                float4 v = x[r][q];
                if (RELU_X) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[n] = fmaf(v.w, w[n][q].w, fmaf(v.z, w[n][q].z, fmaf(v.y, w[n][q].y, fmaf(v.x, w[n][q].x, acc[n]))));
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = wave_sum_dpp(acc[n]);
            if (lane == 0 && m0 + r < M) *(float4*)(Y + (size_t)(m0 + r) * ldy) = make_float4(acc[0] + b0, acc[1] + b1, acc[2] + b2, acc[3] + b3);
        }
    }
}

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {
    f32x2v f = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2v));
}

// ------------------------------------------------------------------ shared by the seven 128 x 128 MFMA tile GEMMs below
// (k_mgemm_f32, k_mgemm_bf16, k_mgemm_bf16x3: register-staged; k_hgemm_dma, k_sgemm_dma, k_sgemm_dma_kt, k_hgemm_dma_kt: LDS-DMA.)
// The tile order, the accumulators and their 2 x 2 products, the LDS-DMA issue and wait and the epilogues are stated here, once.
// 1-D grid with an XCD-aware tile order.  Workgroup ids go round the 8 XCDs, each with its own L2: the tiles that share an
// operand — the N tiles of one 128-row block of the activations, or all (m, n) tiles of one reduction split — get
// consecutive slots on ONE XCD, so the operand is fetched from HBM once instead of once per tile (measured before:
// activations re-read 1.8-2.7x, after: 1.0x; profiles/r03_pmc_train_mem.txt).  n_groups rounded up to the 8 XCDs.
static inline dim3 mgemm_grid(int64_t n_groups, int group) { return dim3((unsigned)(((n_groups + 7) / 8) * 8 * group)); }

template <bool SPLIT>
__host__ __device__ __forceinline__ bool mgemm_tile_of(int block, int M, int N, int Rn, int r_per_split, int& bx, int& by, int& bz) {
    const int gx = (M + 127) / 128, gy = (N + 127) / 128;
    const int xcd = block & 7, slot = block >> 3;
    const int G = SPLIT ? gx * gy : gy;
    const int NG = SPLIT ? (Rn + r_per_split - 1) / r_per_split : gx;
    const int grp = (slot / G) * 8 + xcd, tg = slot % G;
    bx = by = bz = 0;
    if (grp >= NG) return false;        // padding block of the rounded-up grid
    if (SPLIT) { bz = grp; bx = tg % gx; by = tg / gx; }
    else { bx = grp; by = tg; }
    return true;
}
template <bool SPLIT>
__device__ __forceinline__ bool mgemm_tile(int M, int N, int Rn, int r_per_split, int& bx, int& by, int& bz) {
    return mgemm_tile_of<SPLIT>((int)blockIdx.x, M, N, Rn, r_per_split, bx, by, bz);
}

__device__ __forceinline__ void tile_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// One reduction step of a wave's 2 x 2 fragments (a0, a1: rows wm, wm + 32; b0, b1: columns wn, wn + 32), one helper per operand
// form.  The operands are SWAPPED (mfma(b, a)): the 32 x 32 tiles come out transposed, as mgemm_epilogue below takes them.
__device__ __forceinline__ void tile_mfma_f32(f32x16 (&acc)[2][2], float a0, float a1, float b0, float b1) {
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a0, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, a1, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, a1, acc[1][1], 0, 0, 0);
}
__device__ __forceinline__ void tile_mfma_bf16(f32x16 (&acc)[2][2], bf16x8 a0, bf16x8 a1, bf16x8 b0, bf16x8 b1) {
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b0, a0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b1, a0, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b0, a1, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b1, a1, acc[1][1], 0, 0, 0);
}
// bf16x3, one accumulator: both fragments as their hi and lo images; hi*lo + lo*hi + hi*hi, the small terms first
__device__ __forceinline__ void mfma_bf16x3(f32x16& acc, bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, al, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl, ah, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, ah, acc, 0, 0, 0);
}
// relu on packed bf16 values (sign bit set -> 0): what staging relu(fp32) and rounding gives
__device__ __forceinline__ bf16x8 relu_bf16x8(bf16x8 v) {
    const s16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return __builtin_bit_cast(bf16x8, __builtin_elementwise_max(__builtin_bit_cast(s16x8, v), z));
}

// A wave's share of one k-step by LDS-DMA: PIECES (4 or 8) lane-linear 1-KiB pieces — lane l's 16 bytes from src + voff[j] to LDS
// byte dst + 0x400 j + 16 l.  M0 (the destination base) is the compiler's: saved, written and restored in the ONE statement that
// reads it.  hipcc does not count these loads: dma_step_wait does.
template <int PIECES>
__device__ __forceinline__ void dma_issue(const uint32_t (&voff)[PIECES], const char* src, uint32_t dst) {
    static_assert(PIECES == 4 || PIECES == 8, "a wave issues 4 or 8 pieces per k-step");
    uint32_t keep;
    if constexpr (PIECES == 8)
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %10\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %9\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %9\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %9\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %9\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %9\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %6, %9\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %7, %9\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %8, %9\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "v"(voff[4]), "v"(voff[5]), "v"(voff[6]), "v"(voff[7]),
                       "s"(src), "s"(dst)
                     : "memory", "scc");
    else
        asm volatile("s_mov_b32 %0, m0\n\t"
                     "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5\n\t"
                     "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %5\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "s"(src), "s"(dst) : "memory", "scc");
}
// The head of k-step ks of a DMA k-loop with DEPTH k-steps in flight: wait for this wave's pieces of k-step ks — DEPTH 1: the
// only ones outstanding; DEPTH 3 (4-piece k-steps): all but those of the `younger` (= nk - 1 - ks) k-steps issued behind it —
// and for the wave's own LDS reads, then the barrier: every wave's pieces of k-step ks are in, and the slot the caller issues
// into next has no reader left.
template <int DEPTH>
__device__ __forceinline__ void dma_step_wait(int younger = 0) {
    static_assert(DEPTH == 1 || DEPTH == 3, "one or three k-steps in flight");
    if (DEPTH == 3 && younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (DEPTH == 3 && younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Epilogue of a 128 x 128 workgroup tile whose MFMAs ran with the operands SWAPPED (mfma(b, a)): the 32 x 32 tiles come out
// transposed — lane lc holds row m, its registers 4 consecutive n per group of four (n = 8 (e >> 2) + 4 lr + (e & 3)) — so
// C, the residual R, the relu mask and the bf16 copy move as 16-byte (8-byte) rows instead of single elements: 16 instead of
// 64 memory instructions per thread and tensor (the element-wise form was 30-45 % of the forward / dX launch).  Same
// products, same sums.  16-byte accesses need every leading dimension % 4 == 0 and aligned bases; otherwise by element.
// (host and device: pnr_debug_linear reports the epilogue form a launch takes)
__host__ __device__ __forceinline__ bool mgemm_vec_ok(const float* bias, const float* R, int ldr, const void* Mk, int ldm, bool m16,
                                                      const float* C, int ldc, const uint16_t* C16, int ldc16, size_t zs_c) {
    return ((ldc | ldr | ldm | ldc16) & 3) == 0 && (((uintptr_t)C | (uintptr_t)R | (uintptr_t)bias) & 15) == 0 &&
           ((uintptr_t)Mk & (m16 ? 7 : 15)) == 0 && ((uintptr_t)C16 & 7) == 0 && (zs_c & 3) == 0;
}
template <bool SPLIT, bool M16>
__device__ __forceinline__ void mgemm_epilogue(const f32x16 (&acc)[2][2], int m0, int n0, int wm, int wn, int lc, int lr, int bz,
                                               const float* __restrict__ bias, const float* R, int ldr, const void* __restrict__ Mk,
                                               int ldm, float* C, int ldc, uint16_t* __restrict__ C16, int ldc16, int M, int N,
                                               size_t zs_c) {
    const bool vec_ok = mgemm_vec_ok(bias, R, ldr, Mk, ldm, M16, C, ldc, C16, ldc16, zs_c);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm + 32 * i + lc;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = n0 + wn + 32 * j + 8 * q + 4 * lr;          // n .. n + 3
                if (n >= N) continue;
                const bool vec = vec_ok && n + 3 < N;
                const int nu = N - n < 4 ? N - n : 4;                       // elements of the group inside the matrix
                float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                if (bias) {
                    if (vec) { const float4 b4 = *(const float4*)(bias + n); v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w; }
                    else { for (int u = 0; u < nu; ++u) v[u] += bias[n + u]; }
                }
                if (SPLIT) {
                    float* dst = C + bz * zs_c + (size_t)m * ldc + n;       // this split's own slice (grad_w)
                    if (vec) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                    else { for (int u = 0; u < nu; ++u) dst[u] = v[u]; }
                    continue;
                }
                if (Mk) {
                    // The two mask forms differ on NaN only: the fp32 mask (m > 0) drops a NaN pre-activation, the bf16 one (sign
                    // clear and not zero) keeps a positive-sign NaN (tests/test_gpu_train_gemm.py pins both).
                    if (M16) {               // bf16 tape value > 0: sign clear and not zero
                        const uint16_t* mp = (const uint16_t*)Mk + (size_t)m * ldm + n;
                        uint16_t b16[4] = {0, 0, 0, 0};
                        if (vec) { const uint2 w = *(const uint2*)mp; b16[0] = w.x & 0xffffu; b16[1] = w.x >> 16; b16[2] = w.y & 0xffffu; b16[3] = w.y >> 16; }
                        else { for (int u = 0; u < nu; ++u) b16[u] = mp[u]; }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (!((b16[u] & 0x8000u) == 0 && (b16[u] & 0x7fffu) != 0)) v[u] = 0.f;
                    } else {
                        const float* mp = (const float*)Mk + (size_t)m * ldm + n;
                        float mk[4] = {0.f, 0.f, 0.f, 0.f};
                        if (vec) { const float4 w = *(const float4*)mp; mk[0] = w.x; mk[1] = w.y; mk[2] = w.z; mk[3] = w.w; }
                        else { for (int u = 0; u < nu; ++u) mk[u] = mp[u]; }
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (!(mk[u] > 0.f)) v[u] = 0.f;
                    }
                }
                if (R) {
                    const float* rp = R + (size_t)m * ldr + n;
                    if (vec) { const float4 w = *(const float4*)rp; v[0] += w.x; v[1] += w.y; v[2] += w.z; v[3] += w.w; }
                    else { for (int u = 0; u < nu; ++u) v[u] += rp[u]; }
                }
                if (C) {
                    float* dst = C + (size_t)m * ldc + n;
                    if (vec) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                    else { for (int u = 0; u < nu; ++u) dst[u] = v[u]; }
                }
                if (C16) {
                    uint16_t* dst = C16 + (size_t)m * ldc16 + n;
                    const uint2 w = {pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3])};
                    if (vec) *(uint2*)dst = w;
                    else {
                        const uint16_t h[4] = {(uint16_t)(w.x & 0xffffu), (uint16_t)(w.x >> 16), (uint16_t)(w.y & 0xffffu), (uint16_t)(w.y >> 16)};
                        for (int u = 0; u < nu; ++u) dst[u] = h[u];
                    }
                }
            }
    }
}

// The same epilogue through LDS, for the kernels whose 64-KiB ring is free once the k-loop is done (k_hgemm_dma, k_sgemm_dma).
// mgemm_epilogue's accesses follow the accumulator layout — a lane owns a ROW, so one memory instruction touches 32 rows with
// 16-32 bytes each — and that was more than half of those launches (forward 69 -> 32 us, dX 86 -> 26 us with the epilogue
// compiled out: profiles/r04_hgemm_epilogue.txt).  Here the accumulators go to LDS as a [128][128] fp32 tile (16-byte chunk c of
// row r at 16 (c ^ (r & 31)): the transposed writes and the row-wise reads are both conflict-free), and a half-wave then owns
// one 512-byte ROW SEGMENT: the mask, the residual, C and the bf16 copy move as whole 128-byte lines.  Same values, same
// operations in the same order per element (acc + bias, mask, + residual, round) — bit-identical to mgemm_epilogue.
// Requires the vector conditions of mgemm_epilogue and N % 4 == 0 (tile_epilogue_ok); every thread of the block calls it.
__host__ __device__ __forceinline__ bool tile_epilogue_ok(const float* bias, const float* R, int ldr, const void* Mk, int ldm,
                                                          bool m16, const float* C, int ldc, const uint16_t* C16, int ldc16, int N) {
    return (N & 3) == 0 && mgemm_vec_ok(bias, R, ldr, Mk, ldm, m16, C, ldc, C16, ldc16, 0);
}
// tile_epilogue_lds's form for a result that only leaves as its bf16 copy (eight columns per lane)
__host__ __device__ __forceinline__ bool tile_epilogue_c16_only(bool m16, const float* R, const void* Mk, int ldm, const float* C,
                                                                const uint16_t* C16, int ldc16, int N) {
    return (m16 || !Mk) && !C && !R && C16 && (N & 7) == 0 && (((uintptr_t)C16 | (uintptr_t)Mk) & 15) == 0 && ((ldc16 | ldm) & 7) == 0;
}
template <bool M16>
__device__ __forceinline__ void tile_epilogue_lds(const f32x16 (&acc)[2][2], char* tile, int t, int m0, int n0, int wm, int wn, int lc,
                                                  int lr, const float* __restrict__ bias, const float* R, int ldr,
                                                  const void* __restrict__ Mk, int ldm, float* C, int ldc,
                                                  uint16_t* __restrict__ C16, int ldc16, int M, int N) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                  // no wave reads a ring slot any more (the last k-step's DMA was waited for)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = wm + 32 * i + lc, ch = (wn + 32 * j + 8 * q + 4 * lr) >> 2;
                *(float4*)(tile + row * 512 + 16 * (ch ^ (row & 31))) =
                    make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
            }
    __syncthreads();
    if (tile_epilogue_c16_only(M16, R, Mk, ldm, C, C16, ldc16, N)) {
        // only the bf16 copy leaves (fc_0-type forward, dh of the backward): a lane takes EIGHT columns, so the copy and the
        // mask move as 16-byte pieces (8-byte accesses run at 0.54-0.70x the 16-byte rate: MI355X_MICROARCH.md), a quarter-wave
        // per 256-byte row segment.  Same operations per element.
        const int c8 = t & 15, n8 = n0 + 8 * c8, rq = t >> 4;
        if (n8 >= N) return;
        float bb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (bias) {
            const float4 u0 = *(const float4*)(bias + n8), u1 = *(const float4*)(bias + n8 + 4);
            bb[0] = u0.x; bb[1] = u0.y; bb[2] = u0.z; bb[3] = u0.w; bb[4] = u1.x; bb[5] = u1.y; bb[6] = u1.z; bb[7] = u1.w;
        }
#pragma unroll
        for (int it0 = 0; it0 < 8; it0 += 4) {
            uint4 mk[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int m = m0 + rq + 16 * (it0 + u);
                mk[u] = make_uint4(0u, 0u, 0u, 0u);
                if (Mk && m < M) mk[u] = *(const uint4*)((const uint16_t*)Mk + (size_t)m * ldm + n8);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int r = rq + 16 * (it0 + u), m = m0 + r;
                if (m >= M) continue;
                const float4 a0 = *(const float4*)(tile + r * 512 + 16 * ((2 * c8) ^ (r & 31)));
                const float4 a1 = *(const float4*)(tile + r * 512 + 16 * ((2 * c8 + 1) ^ (r & 31)));
                float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                if (bias) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += bb[e];
                }
                if (Mk) {
                    const uint32_t w[4] = {mk[u].x, mk[u].y, mk[u].z, mk[u].w};
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const uint32_t b16 = (e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu);
                        if (!((b16 & 0x8000u) == 0 && (b16 & 0x7fffu) != 0)) v[e] = 0.f;
                    }
                }
                *(uint4*)(C16 + (size_t)m * ldc16 + n8) =
                    make_uint4(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
            }
        }
        return;
    }
    const int c = t & 31, n = n0 + 4 * c, r0 = t >> 5;
    if (n >= N) return;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) b4 = *(const float4*)(bias + n);
#pragma unroll
    for (int it0 = 0; it0 < 16; it0 += 4) {
        float4 rv[4];
        uint2 mk16[4];
        float4 mk32[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {                // the batch's global loads first: four rows in flight per thread
            const int m = m0 + r0 + 8 * (it0 + u);
            rv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            mk16[u] = make_uint2(0u, 0u);
            mk32[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < M) {
                if (R) rv[u] = *(const float4*)(R + (size_t)m * ldr + n);
                if (Mk) {
                    if (M16) mk16[u] = *(const uint2*)((const uint16_t*)Mk + (size_t)m * ldm + n);
                    else mk32[u] = *(const float4*)((const float*)Mk + (size_t)m * ldm + n);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + 8 * (it0 + u), m = m0 + r;
            if (m >= M) continue;
            const float4 a4 = *(const float4*)(tile + r * 512 + 16 * (c ^ (r & 31)));
            float v[4] = {a4.x, a4.y, a4.z, a4.w};
            if (bias) { v[0] += b4.x; v[1] += b4.y; v[2] += b4.z; v[3] += b4.w; }
            if (Mk) {
                if (M16) {
                    const uint16_t b16[4] = {(uint16_t)(mk16[u].x & 0xffffu), (uint16_t)(mk16[u].x >> 16), (uint16_t)(mk16[u].y & 0xffffu),
                                             (uint16_t)(mk16[u].y >> 16)};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (!((b16[e] & 0x8000u) == 0 && (b16[e] & 0x7fffu) != 0)) v[e] = 0.f;
                } else {
                    const float mk[4] = {mk32[u].x, mk32[u].y, mk32[u].z, mk32[u].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (!(mk[e] > 0.f)) v[e] = 0.f;
                }
            }
            if (R) { v[0] += rv[u].x; v[1] += rv[u].y; v[2] += rv[u].z; v[3] += rv[u].w; }
            if (C) *(float4*)(C + (size_t)m * ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
            if (C16) *(uint2*)(C16 + (size_t)m * ldc16 + n) = make_uint2(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]));
        }
    }
}

template <bool A_RC, bool B_RC, bool RELU_A, bool RELU_B, bool SPLIT>
static __global__ void __launch_bounds__(256) k_mgemm_f32(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, const float* __restrict__ bias,
    const float* R, int ldr, const float* __restrict__ Mk, int ldm, float* C, int ldc, float* __restrict__ rowsum,
    int M, int N, int Rn, int r_per_split, int vec_ok, size_t zs_c = 0, size_t zs_r = 0) {
    __shared__ float As[2][16][132];
    __shared__ float Bs[2][16][132];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int bx, by, bz;
    if (!mgemm_tile<SPLIT>(M, N, Rn, r_per_split, bx, by, bz)) return;
    const int m0 = bx * 128, n0 = by * 128;
    const int rb = SPLIT ? bz * r_per_split : 0;
    const int re = SPLIT ? min(Rn, rb + r_per_split) : Rn;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    f32x16 acc[2][2];
    tile_zero(acc);
    float va[8], vb[8];
    float rs = 0.f;
    const bool fast_a = (vec_ok & 1) && m0 + 128 <= M, fast_b = (vec_ok & 2) && n0 + 128 <= N;   // block-uniform
    auto fetch = [&](int r) {
        const bool full = r + 16 <= re;
        if (fast_a && full) mg_fetch_fast<A_RC>(A, lda, m0, r, false, va);
        else mg_fetch<A_RC>(A, lda, m0, M, r, re, false, va);
        if (fast_b && full) mg_fetch_fast<B_RC>(B, ldb, n0, r, false, vb);
        else mg_fetch<B_RC>(B, ldb, n0, N, r, re, false, vb);
    };
    // Software pipeline: tile i's MFMAs run with tile i+1 already in LDS (staged before them, from registers
    // fetched one iteration earlier) and tile i+2 in flight from global memory.
    fetch(rb);
    mg_stage<A_RC, RELU_A>(As[0], va);
    mg_stage<B_RC, RELU_B>(Bs[0], vb);
    if (rb + 16 < re) fetch(rb + 16);
    __syncthreads();
    int buf = 0;
    for (int r0 = rb; r0 < re; r0 += 16) {
        if (r0 + 16 < re) {
            mg_stage<A_RC, RELU_A>(As[buf ^ 1], va);
            mg_stage<B_RC, RELU_B>(Bs[buf ^ 1], vb);
            if (r0 + 32 < re) fetch(r0 + 32);
        }
        const int lr = lane >> 5, lc = lane & 31;
        // 4 groups of 2 r-steps; group g+1's fragments are read while group g's 8 MFMAs (512 cycles) run
        float fa[2][4], fb[2][4];
        auto frag = [&](int g, float (&a)[4], float (&b)[4]) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int r = 2 * (2 * g + q) + lr;
                a[2 * q] = As[buf][r][wm + lc]; a[2 * q + 1] = As[buf][r][wm + 32 + lc];
                b[2 * q] = Bs[buf][r][wn + lc]; b[2 * q + 1] = Bs[buf][r][wn + 32 + lc];
            }
        };
        frag(0, fa[0], fb[0]);
        __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g < 3) frag(g + 1, fa[(g + 1) & 1], fb[(g + 1) & 1]);
            float(&a)[4] = fa[g & 1];
            float(&b)[4] = fb[g & 1];
#pragma unroll
            for (int q = 0; q < 2; ++q) tile_mfma_f32(acc, a[2 * q], a[2 * q + 1], b[2 * q], b[2 * q + 1]);
            if (g < 3) {        // keep the next group's reads ahead of this group's MFMAs in the schedule
                __builtin_amdgcn_sched_group_barrier(0x100, 8, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
        }
        if (rowsum && by == 0 && t < 128) {
#pragma unroll
            for (int r = 0; r < 16; ++r) rs += As[buf][r][t];
        }
        __syncthreads();
        buf ^= 1;
    }
    const int lr = lane >> 5, lc = lane & 31;
    mgemm_epilogue<SPLIT, false>(acc, m0, n0, wm, wn, lc, lr, bz, bias, R, ldr, Mk, ldm, C, ldc, nullptr, 0, M, N, zs_c);
    if (rowsum && by == 0 && t < 128 && m0 + t < M) {
        if (SPLIT) rowsum[bz * zs_r + m0 + t] = rs;
        else atomicAdd(rowsum + m0 + t, rs);
    }
}

// ------------------------------------------------------------------ bf16 MFMA GEMM on the fp32 tape (opt-in, AMP-like)
// Same contract and operand forms as k_mgemm_f32, but the products run on v_mfma_f32_32x32x16_bf16: operands are
// converted fp32 -> bf16 while they are staged into LDS (the tape, the weights and every result stay fp32 in
// memory, accumulation is fp32).  The reference's counterpart is its AMP switch (train/train.py:385-398).
// 128x128 tile, 32-deep reduction tiles, LDS image [row][32 k] bf16 with 80-byte rows (conflict-free
// ds_read_b128 fragment reads: lane = (row l%32, k-half l/32) takes 8 consecutive k).  Operands stored
// reduction-major are transposed in registers: a thread owns a 4(r) x 4(x) block and writes 4 x 8 bytes.
// Requirements (else the caller uses k_mgemm_f32): 16-byte aligned operands, leading dimensions % 4 == 0,
// the reduction extent % 32 == 0 unless SPLIT (whose row tail is zero-filled), x extents % 4 == 0.


__device__ __forceinline__ float bf16_lo(uint32_t p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

// H16: the operand is stored as bf16 (the 16-bit tape of train_precision="bf16"): half the bytes, expanded to the fp32 values
// mh_stage packs straight back — the staged LDS image is bit-identical to the one an fp32 copy of the same tensor gives,
// because that copy would be rounded by the same v_cvt_pk_bf16_f32 here.
template <bool RC, bool H16 = false>
__device__ __forceinline__ void mh_fetch(const void* __restrict__ Sv, int ld, int x0, int X, int r0, int r1, float4 (&v)[4]) {
    const int t = threadIdx.x;
    if (H16) {
        const uint16_t* S = (const uint16_t*)Sv;
        if (RC) {        // a row's 32-r slice is 64 B: 4 lanes x 16 B, 64 rows per instruction (v[2i], v[2i+1]: row t/4 + 64 i)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int x = min(x0 + (t >> 2) + 64 * i, X - 1);
                const uint4 a = *(const uint4*)(S + (size_t)x * ld + r0 + 8 * (t & 3));
                v[2 * i] = make_float4(bf16_lo(a.x), bf16_hi(a.x), bf16_lo(a.y), bf16_hi(a.y));
                v[2 * i + 1] = make_float4(bf16_lo(a.z), bf16_hi(a.z), bf16_lo(a.w), bf16_hi(a.w));
            }
        } else {
            const int x = min(x0 + 4 * (t >> 3), X - 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = min(r0 + 4 * (t & 7) + i, r1 - 1);
                const uint2 a = *(const uint2*)(S + (size_t)r * ld + x);
                v[i] = make_float4(bf16_lo(a.x), bf16_hi(a.x), bf16_lo(a.y), bf16_hi(a.y));
            }
        }
        return;
    }
    const float* S = (const float*)Sv;
    if (RC) {            // stored (X, R): a row's 32-r slice is 128 B = 8 lanes x 16 B, 32 rows per instruction (v[i]: row t/8 + 32 i).
        // (One thread reading its own 64 contiguous bytes — 2 lanes per row — issued 4x the L1 requests of this mapping: the
        // forward / dX GEMMs were bound by the request rate, 1.7-1.9 TB/s: profiles/r03_pmc_train_mem.txt.)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = min(x0 + (t >> 3) + 32 * i, X - 1);
            v[i] = *(const float4*)(S + (size_t)x * ld + r0 + 4 * (t & 7));
        }
    } else {             // stored (R, X): thread -> 4 r's at 4*(t&7), 4 x's at 4*(t>>3)
        const int x = min(x0 + 4 * (t >> 3), X - 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = min(r0 + 4 * (t & 7) + i, r1 - 1);
            v[i] = *(const float4*)(S + (size_t)r * ld + x);
        }
    }
}

// residual of a bf16 pair: (f0 - bf16(f0), f1 - bf16(f1)) packed as bf16 — the "lo" part of the bf16x3 split
__device__ __forceinline__ uint32_t pk_bf16_lo(float f0, float f1, uint32_t hi) {
    return pk_bf16(f0 - __builtin_bit_cast(float, hi << 16), f1 - __builtin_bit_cast(float, hi & 0xffff0000u));
}

template <bool RC, bool RELU, bool ZERO_TAIL, bool H16 = false>
__device__ __forceinline__ void mh_stage(uint16_t (*T)[40], float4 (&v)[4], int r0, int r1, uint16_t (*TL)[40] = nullptr) {
    const int t = threadIdx.x;
    // the loads above are unconditional and complete HERE (not earlier: hipcc would otherwise sink them into the
    // tail predicate and wait on each one)
    asm volatile("" : "+v"(v[0].x), "+v"(v[0].y), "+v"(v[0].z), "+v"(v[0].w), "+v"(v[1].x), "+v"(v[1].y), "+v"(v[1].z), "+v"(v[1].w),
                      "+v"(v[2].x), "+v"(v[2].y), "+v"(v[2].z), "+v"(v[2].w), "+v"(v[3].x), "+v"(v[3].y), "+v"(v[3].z), "+v"(v[3].w));
    float f[16] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w,
                   v[2].x, v[2].y, v[2].z, v[2].w, v[3].x, v[3].y, v[3].z, v[3].w};
    if (RELU) {
#pragma unroll
        for (int e = 0; e < 16; ++e) f[e] = fmaxf(f[e], 0.f);
    }
    if (RC && H16) {     // f[8 i + j]: row t/4 + 64 i, r = 8 (t&3) + j   (mh_fetch<true, true>)
        if (ZERO_TAIL) {
#pragma unroll
            for (int e = 0; e < 16; ++e) f[e] = (r0 + 8 * (t & 3) + (e & 7) < r1) ? f[e] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint4 w = {pk_bf16(f[8 * i], f[8 * i + 1]), pk_bf16(f[8 * i + 2], f[8 * i + 3]), pk_bf16(f[8 * i + 4], f[8 * i + 5]),
                             pk_bf16(f[8 * i + 6], f[8 * i + 7])};
            *(uint4*)&T[(t >> 2) + 64 * i][8 * (t & 3)] = w;
        }
    } else if (RC) {     // f[4 i + j]: row t/8 + 32 i, r = 4 (t&7) + j       (mh_fetch<true, false>)
        if (ZERO_TAIL) {
#pragma unroll
            for (int e = 0; e < 16; ++e) f[e] = (r0 + 4 * (t & 7) + (e & 3) < r1) ? f[e] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint2 w = {pk_bf16(f[4 * i], f[4 * i + 1]), pk_bf16(f[4 * i + 2], f[4 * i + 3])};
            *(uint2*)&T[(t >> 3) + 32 * i][4 * (t & 7)] = w;
            if (TL) {       // residual image (bf16x3)
                const uint2 wl = {pk_bf16_lo(f[4 * i], f[4 * i + 1], w.x), pk_bf16_lo(f[4 * i + 2], f[4 * i + 3], w.y)};
                *(uint2*)&TL[(t >> 3) + 32 * i][4 * (t & 7)] = wl;
            }
        }
    } else {
        if (ZERO_TAIL) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) f[4 * i + e] = (r0 + 4 * (t & 7) + i < r1) ? f[4 * i + e] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {        // element (r = 4*(t&7)+i, x = 4*(t>>3)+e) is f[4 i + e]
            uint2 w = {pk_bf16(f[e], f[4 + e]), pk_bf16(f[8 + e], f[12 + e])};
            *(uint2*)&T[4 * (t >> 3) + e][4 * (t & 7)] = w;
            if (TL) {
                uint2 wl = {pk_bf16_lo(f[e], f[4 + e], w.x), pk_bf16_lo(f[8 + e], f[12 + e], w.y)};
                *(uint2*)&TL[4 * (t >> 3) + e][4 * (t & 7)] = wl;
            }
        }
    }
}

// A16 / B16 / M16: that operand / the mask is a bf16 tensor of the 16-bit tape; C16 (may be NULL): a bf16 copy of the result for
// the tape, C may then be NULL (a result that only the tape keeps: fc_0's output).
template <bool A_RC, bool B_RC, bool RELU_A, bool RELU_B, bool SPLIT, bool A16 = false, bool B16 = false, bool M16 = false>
static __global__ void __launch_bounds__(256) k_mgemm_bf16(
    const void* __restrict__ A, int lda, const void* __restrict__ B, int ldb, const float* __restrict__ bias,
    const float* R, int ldr, const void* __restrict__ Mk, int ldm, float* C, int ldc, float* __restrict__ rowsum,
    int M, int N, int Rn, int r_per_split, size_t zs_c = 0, size_t zs_r = 0, uint16_t* __restrict__ C16 = nullptr, int ldc16 = 0) {
    __shared__ __attribute__((aligned(16))) uint16_t As[2][128][40];
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][128][40];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int bx, by, bz;
    if (!mgemm_tile<SPLIT>(M, N, Rn, r_per_split, bx, by, bz)) return;
    const int m0 = bx * 128, n0 = by * 128;
    const int rb = SPLIT ? bz * r_per_split : 0;
    const int re = SPLIT ? min(Rn, rb + r_per_split) : Rn;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int lr = lane >> 5, lc = lane & 31;
    f32x16 acc[2][2];
    tile_zero(acc);
    float4 va[4], vb[4];
    float rs = 0.f;
    mh_fetch<A_RC, A16>(A, lda, m0, M, rb, re, va);
    mh_fetch<B_RC, B16>(B, ldb, n0, N, rb, re, vb);
    mh_stage<A_RC, RELU_A, SPLIT, A16>(As[0], va, rb, re);
    mh_stage<B_RC, RELU_B, false, B16>(Bs[0], vb, rb, re);
    if (rb + 32 < re) {
        mh_fetch<A_RC, A16>(A, lda, m0, M, rb + 32, re, va);
        mh_fetch<B_RC, B16>(B, ldb, n0, N, rb + 32, re, vb);
    }
    __syncthreads();
    int buf = 0;
    for (int r0 = rb; r0 < re; r0 += 32) {
        if (r0 + 32 < re) {
            mh_stage<A_RC, RELU_A, SPLIT, A16>(As[buf ^ 1], va, r0 + 32, re);
            mh_stage<B_RC, RELU_B, false, B16>(Bs[buf ^ 1], vb, r0 + 32, re);
            if (r0 + 64 < re) {
                mh_fetch<A_RC, A16>(A, lda, m0, M, r0 + 64, re, va);
                mh_fetch<B_RC, B16>(B, ldb, n0, N, r0 + 64, re, vb);
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int ko = 16 * s + 8 * lr;
            tile_mfma_bf16(acc, *(const bf16x8*)&As[buf][wm + lc][ko], *(const bf16x8*)&As[buf][wm + 32 + lc][ko],
                           *(const bf16x8*)&Bs[buf][wn + lc][ko], *(const bf16x8*)&Bs[buf][wn + 32 + lc][ko]);
        }
        if (rowsum && by == 0 && t < 128) {       // bias gradient = row sums of the (bf16-rounded) A tile
#pragma unroll
            for (int r = 0; r < 32; r += 2) {
                uint32_t p = *(const uint32_t*)&As[buf][t][r];
                rs += __builtin_bit_cast(float, p << 16) + __builtin_bit_cast(float, p & 0xffff0000u);
            }
        }
        __syncthreads();
        buf ^= 1;
    }
    mgemm_epilogue<SPLIT, M16>(acc, m0, n0, wm, wn, lc, lr, bz, bias, R, ldr, Mk, ldm, C, ldc, C16, ldc16, M, N, zs_c);
    if (rowsum && by == 0 && t < 128 && m0 + t < M) {
        if (SPLIT) rowsum[bz * zs_r + m0 + t] = rs;
        else atomicAdd(rowsum + m0 + t, rs);
    }
}

// ------------------------------------------------------------------ bf16 GEMM with an LDS-DMA k-loop (round 4)
// C (M, N) = act(A (M, K)) . B (N, K)^T, both operands bf16 and ROW-CONTIGUOUS in the reduction index (the 16-bit tape's
// activations / the bf16 gradient stream against bf16 copies of the weights, k_w_to_bf16): the forward and dX GEMMs of the
// bf16 mode.  Same 128 x 128 tile, same MFMA (32x32x16 bf16, operands swapped), same k order and the same epilogue as
// k_mgemm_bf16 — bit-identical results — but the tiles go global -> LDS by LDS-DMA (global_load_lds_dwordx4), no register
// pass, no conversion, into two 32-KiB slots (k-steps of 64: the next one lands while this one is multiplied).
// k_mgemm_bf16's loop issues tile i + 2 only after staging tile i + 1 through registers, and the activation rows (a slice of every
// 1-KiB row per k-step, ~100 MB working set over the chip) come from beyond the L2, so every iteration paid a loaded memory
// latency (profiles/r03_pmc_train_mem.txt, profiles/r04_pmc_train_mem.txt).
// A k-step takes a whole 128-byte LINE of every row: with 64-byte chunks (k-steps of 32, four 16-KiB slots, three in flight —
// this kernel's first form) the k-loop ran at the L2's REQUEST rate, 15 TB/s for half lines against 22 TB/s for whole lines at
// fewer bytes in flight (tools/dev/ubench/dma_piece_ubench.hip, profiles/r04_dma_piece_ubench.txt).
// LDS image of a tile: [128 rows][8 chunks of 16 B], chunk c of row r at r*128 + 16*(c ^ ((r >> 1) & 7)): with ds_read_b128's
// lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...: MI355X_MICROARCH.md, LDS) the 16 rows of a group — eight even, eight
// odd, their r >> 1 distinct mod 8 — then fall on 16 different bank quads.  An LDS-DMA piece is lane-linear (lane l -> base + 16 l =
// row l >> 3, physical chunk l & 7), so the swizzle is on the SOURCE address.  A wave issues 8 pieces per k-step (waves 0, 1: the
// A tile, waves 2, 3: the B tile).  Requires K % 64 == 0 (else the register-staged kernel).
template <bool RELU_A, bool M16>
static __global__ void __launch_bounds__(256, 2) k_hgemm_dma(
    const uint16_t* __restrict__ A, int lda, const uint16_t* __restrict__ B, int ldb, const float* __restrict__ bias,
    const float* R, int ldr, const void* __restrict__ Mk, int ldm, float* C, int ldc, uint16_t* __restrict__ C16, int ldc16,
    int M, int N, int K) {
    __shared__ __attribute__((aligned(1024))) char ring[2 * 32768];
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    int bx, by, bz;
    if (!mgemm_tile<false>(M, N, K, 0, bx, by, bz)) return;
    const int m0 = bx * 128, n0 = by * 128;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int lr = lane >> 5, lc = lane & 31;
    // ---- loader: this wave's eight pieces of a k-step (8 rows x 128 B each) of its operand
    const bool loads_b = wv >= 2;
    const uint16_t* src = loads_b ? B : A;
    const int ld = loads_b ? ldb : lda, x0 = loads_b ? n0 : m0, X = loads_b ? N : M;
    uint32_t voff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = 8 * (8 * (wv & 1) + j) + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        const int xr = x0 + row < X ? row : X - 1 - x0;            // rows past the edge re-read the last one (never stored)
        voff[j] = (uint32_t)xr * (uint32_t)ld * 2u + 16u * c;      // relative to the tile's first row: fits 32 bits for any M
    }
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)ring;
    const uint32_t dst0 = __builtin_amdgcn_readfirstlane(ring_lds + (loads_b ? 16384 : 0) + 8192 * (wv & 1));
    const char* src_tile = (const char*)src + (size_t)x0 * ld * 2;
    auto issue = [&](int ks) __attribute__((always_inline)) {        // 64 k = 128 B further along every row
        dma_issue<8>(voff, src_tile + (size_t)ks * 128, dst0 + (uint32_t)(ks & 1) * 32768u);
    };
    f32x16 acc[2][2];
    tile_zero(acc);
    const int nk = K >> 6;
    issue(0);
    // fragment addresses within a slot (fixed over the loop): row r, logical chunk 2 s + lr of the row's eight
    uint32_t fa[2][4], fb[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int sp = 0; sp < 4; ++sp) {
            const int ra = wm + 32 * i + lc, rb = wn + 32 * i + lc;
            fa[i][sp] = (uint32_t)ra * 128u + 16u * ((2 * sp + lr) ^ ((ra >> 1) & 7));
            fb[i][sp] = 16384u + (uint32_t)rb * 128u + 16u * ((2 * sp + lr) ^ ((rb >> 1) & 7));
        }
    for (int ks = 0; ks < nk; ++ks) {
        dma_step_wait<1>();
        if (ks + 1 < nk) issue(ks + 1);
        const char* slot = ring + (ks & 1) * 32768;
#pragma unroll
        for (int sp = 0; sp < 4; ++sp) {
            bf16x8 a0 = *(const bf16x8*)(slot + fa[0][sp]);
            bf16x8 a1 = *(const bf16x8*)(slot + fa[1][sp]);
            const bf16x8 b0 = *(const bf16x8*)(slot + fb[0][sp]);
            const bf16x8 b1 = *(const bf16x8*)(slot + fb[1][sp]);
            if (RELU_A) { a0 = relu_bf16x8(a0); a1 = relu_bf16x8(a1); }
            tile_mfma_bf16(acc, a0, a1, b0, b1);
        }
    }
    if (tile_epilogue_ok(bias, R, ldr, Mk, ldm, M16, C, ldc, C16, ldc16, N))
        tile_epilogue_lds<M16>(acc, ring, t, m0, n0, wm, wn, lc, lr, bias, R, ldr, Mk, ldm, C, ldc, C16, ldc16, M, N);
    else
        mgemm_epilogue<false, M16>(acc, m0, n0, wm, wn, lc, lr, 0, bias, R, ldr, Mk, ldm, C, ldc, C16, ldc16, M, N, 0);
}

// ------------------------------------------------------------------ fp32 GEMM with an LDS-DMA k-loop (round 4)
// C (M, N) = act(A (M, K)) . B (N, K)^T on v_mfma_f32_32x32x2_f32, both operands fp32 and row-contiguous in the reduction index
// — every layer of the fp32 inference path (activations x nn.Linear weights as stored) and the taped fp32 forward.  The
// structure of k_hgemm_dma: 128 x 128 tile, 16-deep k-steps (a 64-byte row chunk per tile row), global -> LDS by LDS-DMA
// into four 16-KiB slots, three k-steps in flight, source-side swizzle.  What changes against k_mgemm_f32 besides the
// pipeline is the fragment traffic: that kernel reads one float per lane and MFMA (32 ds_read_b32 per k-step); here a lane
// reads a 16-byte chunk of its row — lanes of k-half 0 the even chunk, of k-half 1 the odd chunk of a chunk pair — and MFMA e
// of the pair multiplies reduction indices (4 c + e, 4 c + 4 + e): 8 ds_read_b128 per k-step, every product still summed
// exactly once (the grouping of the sum differs from k_mgemm_f32's: fp32 rounding-level differences, inside the 1e-4 / 5e-4
// tolerances of the parity and gradient tests).
template <bool RELU_A>
static __global__ void __launch_bounds__(256, 2) k_sgemm_dma(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, const float* __restrict__ bias,
    const float* R, int ldr, const float* __restrict__ Mk, int ldm, float* C, int ldc, int M, int N, int K) {
    __shared__ __attribute__((aligned(1024))) char ring[4 * 16384];
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    int bx, by, bz;
    if (!mgemm_tile<false>(M, N, K, 0, bx, by, bz)) return;
    const int m0 = bx * 128, n0 = by * 128;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int lr = lane >> 5, lc = lane & 31;
    const bool loads_b = wv >= 2;
    const float* src = loads_b ? B : A;
    const int ld = loads_b ? ldb : lda, x0 = loads_b ? n0 : m0, X = loads_b ? N : M;
    uint32_t voff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 16 * (4 * (wv & 1) + j) + (lane >> 2);
        const int c = (lane & 3) ^ ((row >> 3) & 3);
        const int xr = x0 + row < X ? row : X - 1 - x0;
        voff[j] = (uint32_t)xr * (uint32_t)ld * 4u + 16u * c;      // relative to the tile's first row
    }
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)ring;
    const uint32_t dst0 = __builtin_amdgcn_readfirstlane(ring_lds + (loads_b ? 8192 : 0) + 4096 * (wv & 1));
    const char* src_tile = (const char*)src + (size_t)x0 * ld * 4;
    auto issue = [&](int ks) __attribute__((always_inline)) {        // 16 floats further along every row
        dma_issue<4>(voff, src_tile + (size_t)ks * 64, dst0 + (uint32_t)(ks & 3) * 16384u);
    };
    f32x16 acc[2][2];
    tile_zero(acc);
    const int nk = K >> 4;
    for (int ks = 0; ks < 3 && ks < nk; ++ks) issue(ks);
    // fragment addresses within a slot: row r, chunk 2 cp + lr of chunk pair cp
    uint32_t fa[2][2], fb[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
            const int ra = wm + 32 * i + lc, rb = wn + 32 * i + lc;
            fa[i][cp] = (uint32_t)ra * 64u + 16u * ((2 * cp + lr) ^ ((ra >> 3) & 3));
            fb[i][cp] = 8192u + (uint32_t)rb * 64u + 16u * ((2 * cp + lr) ^ ((rb >> 3) & 3));
        }
    for (int ks = 0; ks < nk; ++ks) {
        dma_step_wait<3>(nk - 1 - ks);
        if (ks + 3 < nk) issue(ks + 3);
        const char* slot = ring + (ks & 3) * 16384;
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
            float4 a0 = *(const float4*)(slot + fa[0][cp]);
            float4 a1 = *(const float4*)(slot + fa[1][cp]);
            const float4 b0 = *(const float4*)(slot + fb[0][cp]);
            const float4 b1 = *(const float4*)(slot + fb[1][cp]);
            if (RELU_A) {
                a0.x = fmaxf(a0.x, 0.f); a0.y = fmaxf(a0.y, 0.f); a0.z = fmaxf(a0.z, 0.f); a0.w = fmaxf(a0.w, 0.f);
                a1.x = fmaxf(a1.x, 0.f); a1.y = fmaxf(a1.y, 0.f); a1.z = fmaxf(a1.z, 0.f); a1.w = fmaxf(a1.w, 0.f);
            }
            const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
            const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) tile_mfma_f32(acc, av0[e], av1[e], bv0[e], bv1[e]);
        }
    }
    if (tile_epilogue_ok(bias, R, ldr, (const void*)Mk, ldm, false, C, ldc, nullptr, 0, N))
        tile_epilogue_lds<false>(acc, ring, t, m0, n0, wm, wn, lc, lr, bias, R, ldr, (const void*)Mk, ldm, C, ldc, nullptr, 0, M, N);
    else
        mgemm_epilogue<false, false>(acc, m0, n0, wm, wn, lc, lr, 0, bias, R, ldr, (const void*)Mk, ldm, C, ldc, nullptr, 0, M, N, 0);
}

// The weight-gradient form of k_sgemm_dma: dW (N, K) partial of one row slice = dY (m, N)^T . act(X (m, K)), fp32 operands stored
// reduction-major.  Tiles of 16 points x 128 columns (512-byte rows) by LDS-DMA, three k-steps in flight; the fragments are
// k_mgemm_f32's — one float per lane and MFMA, lanes of one k across consecutive columns (conflict-free without a swizzle) —
// and so is the order of the sums: partials are that kernel's bits.  Slice bounds multiples of 16.
template <bool RELU_B>
static __global__ void __launch_bounds__(256, 2) k_sgemm_dma_kt(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
    float* __restrict__ rowsum, int M, int N, int Rn, int r_per_split, size_t zs_c, size_t zs_r) {
    __shared__ __attribute__((aligned(1024))) char ring[4 * 16384];
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    int bx, by, bz;
    if (!mgemm_tile<true>(M, N, Rn, r_per_split, bx, by, bz)) return;
    const int m0 = bx * 128, n0 = by * 128;
    const int rb = bz * r_per_split, re = min(Rn, rb + r_per_split);
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int lr = lane >> 5, lc = lane & 31;
    const bool loads_b = wv >= 2;
    const float* src = loads_b ? B : A;
    const int ld = loads_b ? ldb : lda, x0 = loads_b ? n0 : m0;
    uint32_t voff[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 2 * (4 * (wv & 1) + j) + (lane >> 5);           // row of the 16-row tile (a piece = 2 rows x 512 B)
        voff[j] = (uint32_t)row * (uint32_t)ld * 4u + (uint32_t)x0 * 4u + 16u * (lane & 31);
    }
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)ring;
    const uint32_t dst0 = __builtin_amdgcn_readfirstlane(ring_lds + (loads_b ? 8192 : 0) + 4096 * (wv & 1));
    const char* src_rb = (const char*)src + (size_t)rb * ld * 4;
    auto issue = [&](int ks) __attribute__((always_inline)) {        // 16 reduction rows further
        dma_issue<4>(voff, src_rb + (size_t)ks * 16 * ld * 4, dst0 + (uint32_t)(ks & 3) * 16384u);
    };
    f32x16 acc[2][2];
    tile_zero(acc);
    const int nk = (re - rb) >> 4;
    for (int ks = 0; ks < 3 && ks < nk; ++ks) issue(ks);
    float rs = 0.f;
    for (int ks = 0; ks < nk; ++ks) {
        dma_step_wait<3>(nk - 1 - ks);
        if (ks + 3 < nk) issue(ks + 3);
        const float* As = (const float*)(ring + (ks & 3) * 16384);          // [16 rows][128]
        const float* Bs = As + 2048;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int r = 2 * e + lr;
            const float a0 = As[r * 128 + wm + lc], a1 = As[r * 128 + wm + 32 + lc];
            float b0 = Bs[r * 128 + wn + lc], b1 = Bs[r * 128 + wn + 32 + lc];
            if (RELU_B) { b0 = fmaxf(b0, 0.f); b1 = fmaxf(b1, 0.f); }
            tile_mfma_f32(acc, a0, a1, b0, b1);
        }
        if (rowsum && by == 0 && t < 128) {
#pragma unroll
            for (int r = 0; r < 16; ++r) rs += As[r * 128 + t];
        }
    }
    mgemm_epilogue<true, false>(acc, m0, n0, wm, wn, lc, lr, bz, nullptr, nullptr, 0, nullptr, 0, C, ldc, nullptr, 0, M, N, zs_c);
    if (rowsum && by == 0 && t < 128 && m0 + t < M) rowsum[bz * zs_r + m0 + t] = rs;
}

// The weight-gradient form of k_hgemm_dma: dW (N, K) partial of one row slice = dY (m, N)^T . act(X (m, K)), both operands bf16
// and stored REDUCTION-major (a row = one point, the output index contiguous).  Tiles of 32 points x 128 columns go
// global -> LDS by LDS-DMA as they are (256-byte rows, full-line reads) and the MFMA fragments — 8 consecutive points of one
// column per lane — come out of the K-major image with gfx950's transposing LDS read (ds_read_b64_tr_b16: 4 rows x 16
// columns per 16-lane group, delivered column-major).  A k-step is 64 points (two 32-KiB slots, the next one lands while this
// one is multiplied): with 32-point k-steps in four 16-KiB slots the DMA stream with its waits and barriers alone took 38 of
// the launch's 46 us (profiles/r04_hgemm_epilogue.txt) — half as many barriers and waits per byte now.  Element j of a lane's fragment is reduction index 16 s + 8 lr + j,
// exactly as in k_mgemm_bf16, so partials (and with them every weight gradient) are bit-identical to that kernel's.
// LDS image: [64 rows][16 chunks of 16 B], chunk ch of row r at 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))) — the
// swizzle that keeps both the transposed reads and row reads conflict-free on 256-byte rows (cdna_hip_programming.md T10);
// applied on the DMA's source address.  Needs the slice bounds and M to be multiples of 64 (no zero-filled tail rows).
template <bool RELU_B>
static __global__ void __launch_bounds__(256, 2) k_hgemm_dma_kt(
    const uint16_t* __restrict__ A, int lda, const uint16_t* __restrict__ B, int ldb, float* __restrict__ C, int ldc,
    float* __restrict__ rowsum, int M /* output rows (A's columns) */, int N /* output columns (B's columns) */, int Rn,
    int r_per_split, size_t zs_c, size_t zs_r) {
    __shared__ __attribute__((aligned(1024))) char ring[2 * 32768];
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    int bx, by, bz;
    if (!mgemm_tile<true>(M, N, Rn, r_per_split, bx, by, bz)) return;
    const int m0 = bx * 128, n0 = by * 128;
    const int rb = bz * r_per_split, re = min(Rn, rb + r_per_split);
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int lr = lane >> 5, lc = lane & 31;
    auto swz = [](int row) { return ((row & 3) << 2) | ((row >> 2) & 3); };
    const bool loads_b = wv >= 2;
    const uint16_t* src = loads_b ? B : A;
    const int ld = loads_b ? ldb : lda, x0 = loads_b ? n0 : m0;
    uint32_t voff[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int row = 4 * (8 * (wv & 1) + j) + (lane >> 4);           // row of the 64-row tile this lane's piece slot holds
        const int ch = (lane & 15) ^ swz(row);
        voff[j] = (uint32_t)row * (uint32_t)ld * 2u + (uint32_t)x0 * 2u + 16u * ch;
    }
    const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)ring;
    const uint32_t dst0 = __builtin_amdgcn_readfirstlane(ring_lds + (loads_b ? 16384 : 0) + 8192 * (wv & 1));
    const char* src_rb = (const char*)src + (size_t)rb * ld * 2;
    auto issue = [&](int ks) __attribute__((always_inline)) {        // 64 reduction rows further
        dma_issue<8>(voff, src_rb + (size_t)ks * 64 * ld * 2, dst0 + (uint32_t)(ks & 1) * 32768u);
    };
    f32x16 acc[2][2];
    tile_zero(acc);
    const int nk = (re - rb) >> 6;
    if (nk > 0) issue(0);
    // transposed-read addresses within a slot: fragment (i, s, h) = rows 16 s + 8 lr + 4 h .. + 3 of the 16-column block that
    // holds this lane's column; lane 4 q + p of a 16-lane group supplies row q, chunk (p >> 1), 8-byte half (p & 1)
    const int q = (lane & 15) >> 2, pp = lane & 3;
    auto tr_addr = [&](int col0 /* first column of the 32-column fragment */, int sp, int h) -> uint32_t {
        const int row = 16 * sp + 8 * lr + 4 * h + q;
        const int ch = ((col0 + 16 * ((lane >> 4) & 1)) >> 3) + (pp >> 1);
        return 256u * row + 16u * (ch ^ swz(row)) + 8u * (pp & 1);
    };
    uint32_t fa[2][4][2], fb[2][4][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int sp = 0; sp < 4; ++sp)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                fa[i][sp][h] = tr_addr(wm + 32 * i, sp, h);
                fb[i][sp][h] = 16384u + tr_addr(wn + 32 * i, sp, h);
            }
    float rs = 0.f;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    auto frag = [&](uint32_t slot_lds, const uint32_t (&ad)[2]) __attribute__((always_inline)) -> bf16x8 {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(slot_lds + ad[0]));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(uintptr_t)(slot_lds + ad[1]));
        const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    };
    for (int ks = 0; ks < nk; ++ks) {
        dma_step_wait<1>();
        if (ks + 1 < nk) issue(ks + 1);
        const uint32_t slot_lds = ring_lds + (uint32_t)(ks & 1) * 32768u;
#pragma unroll
        for (int sp = 0; sp < 4; ++sp) {
            const bf16x8 a0 = frag(slot_lds, fa[0][sp]);
            const bf16x8 a1 = frag(slot_lds, fa[1][sp]);
            bf16x8 b0 = frag(slot_lds, fb[0][sp]);
            bf16x8 b1 = frag(slot_lds, fb[1][sp]);
            if (RELU_B) { b0 = relu_bf16x8(b0); b1 = relu_bf16x8(b1); }
            tile_mfma_bf16(acc, a0, a1, b0, b1);
        }
        if (rowsum && by == 0 && t < 128) {       // bias gradient = sums over the points of A's column t, pairwise like k_mgemm_bf16
            const char* slot = ring + (ks & 1) * 32768;
#pragma unroll
            for (int r = 0; r < 64; r += 2) {
                const uint16_t u0 = *(const uint16_t*)(slot + 256 * r + 16 * ((t >> 3) ^ swz(r)) + 2 * (t & 7));
                const uint16_t u1 = *(const uint16_t*)(slot + 256 * (r + 1) + 16 * ((t >> 3) ^ swz(r + 1)) + 2 * (t & 7));
                rs += __builtin_bit_cast(float, (uint32_t)u0 << 16) + __builtin_bit_cast(float, (uint32_t)u1 << 16);
            }
        }
    }
    mgemm_epilogue<true, false>(acc, m0, n0, wm, wn, lc, lr, bz, nullptr, nullptr, 0, nullptr, 0, C, ldc, nullptr, 0, M, N, zs_c);
    if (rowsum && by == 0 && t < 128 && m0 + t < M) rowsum[bz * zs_r + m0 + t] = rs;
}

// bf16 copies of the hidden layers' weights for k_hgemm_dma: Wb = W (N, K) as stored, Wt = W^T (K, N) for the dX products
// (entry i: a (rows, cols) matrix; wt may be NULL)
static constexpr int W16_MAX = 3 * PNR_MAX_BLOCKS;
struct W16Table { const float* w[W16_MAX]; uint16_t* wb[W16_MAX]; uint16_t* wt[W16_MAX]; int rows[W16_MAX]; int cols[W16_MAX]; int n; };
static __global__ void k_w_to_bf16(W16Table tb) {
    const int i = blockIdx.y;
    const int R = tb.rows[i], Cn = tb.cols[i];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)R * Cn) return;
    const int r = (int)(e / Cn), c = (int)(e - (int64_t)r * Cn);
    const uint16_t v = (uint16_t)(pk_bf16(tb.w[i][e], 0.f) & 0xffffu);
    tb.wb[i][e] = v;
    if (tb.wt[i]) tb.wt[i][(size_t)c * R + r] = v;
}
// fp32 transposes of a table of (rows, cols) matrices: wt (cols, rows)
struct W32Table { const float* w[W16_MAX]; float* wt[W16_MAX]; int rows[W16_MAX]; int cols[W16_MAX]; int n; };
static __global__ void k_w_transpose_f32(W32Table tb) {
    const int i = blockIdx.y;
    const int R = tb.rows[i], Cn = tb.cols[i];
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)R * Cn) return;
    const int r = (int)(e / Cn), c = (int)(e - (int64_t)r * Cn);
    tb.wt[i][(size_t)c * R + r] = tb.w[i][e];
}
// bf16 copy of the first L columns of zx (the latent part: the operand of the lin_z products)
static __global__ void k_cols_to_bf16(const float* __restrict__ x, int64_t rows, int ld, int L, uint16_t* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // one thread per pair of columns
    const int half = L >> 1;
    if (i >= rows * half) return;
    const int64_t r = i / half;
    const int c = (int)(i - r * half) * 2;
    const float2 v = *(const float2*)(x + r * ld + c);
    *(uint32_t*)(y + r * L + c) = pk_bf16(v.x, v.y);
}

// bf16x3: fp32-class products on the bf16 MFMA.  Every operand is split x = hi + lo (two bf16 images in LDS) and a
// product is hi*hi + hi*lo + lo*hi (the lo*lo term is below 2^-16 relative): 3 MFMAs at 16x the fp32-MFMA rate, error
// ~1e-5 instead of bf16's 4e-3.  Same contract and requirements as k_mgemm_bf16; single LDS buffer per image (40 KB),
// the next tile's global loads fly during the MFMAs.
template <bool A_RC, bool B_RC, bool RELU_A, bool RELU_B, bool SPLIT>
static __global__ void __launch_bounds__(256) k_mgemm_bf16x3(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, const float* __restrict__ bias,
    const float* R, int ldr, const float* __restrict__ Mk, int ldm, float* C, int ldc, float* __restrict__ rowsum,
    int M, int N, int Rn, int r_per_split, size_t zs_c = 0, size_t zs_r = 0) {
    __shared__ __attribute__((aligned(16))) uint16_t As[2][128][40];      // [hi, lo]
    __shared__ __attribute__((aligned(16))) uint16_t Bs[2][128][40];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    int bx, by, bz;
    if (!mgemm_tile<SPLIT>(M, N, Rn, r_per_split, bx, by, bz)) return;
    const int m0 = bx * 128, n0 = by * 128;
    const int rb = SPLIT ? bz * r_per_split : 0;
    const int re = SPLIT ? min(Rn, rb + r_per_split) : Rn;
    const int wm = (wv >> 1) * 64, wn = (wv & 1) * 64;
    const int lr = lane >> 5, lc = lane & 31;
    f32x16 acc[2][2];
    tile_zero(acc);
    float4 va[4], vb[4];
    float rs = 0.f;
    mh_fetch<A_RC>(A, lda, m0, M, rb, re, va);
    mh_fetch<B_RC>(B, ldb, n0, N, rb, re, vb);
    for (int r0 = rb; r0 < re; r0 += 32) {
        mh_stage<A_RC, RELU_A, SPLIT>(As[0], va, r0, re, As[1]);
        mh_stage<B_RC, RELU_B, false>(Bs[0], vb, r0, re, Bs[1]);
        __syncthreads();
        if (r0 + 32 < re) {
            mh_fetch<A_RC>(A, lda, m0, M, r0 + 32, re, va);
            mh_fetch<B_RC>(B, ldb, n0, N, r0 + 32, re, vb);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int ko = 16 * s + 8 * lr;
            bf16x8 a0h = *(const bf16x8*)&As[0][wm + lc][ko], a0l = *(const bf16x8*)&As[1][wm + lc][ko];
            bf16x8 a1h = *(const bf16x8*)&As[0][wm + 32 + lc][ko], a1l = *(const bf16x8*)&As[1][wm + 32 + lc][ko];
            bf16x8 b0h = *(const bf16x8*)&Bs[0][wn + lc][ko], b0l = *(const bf16x8*)&Bs[1][wn + lc][ko];
            bf16x8 b1h = *(const bf16x8*)&Bs[0][wn + 32 + lc][ko], b1l = *(const bf16x8*)&Bs[1][wn + 32 + lc][ko];
            mfma_bf16x3(acc[0][0], a0h, a0l, b0h, b0l);
            mfma_bf16x3(acc[0][1], a0h, a0l, b1h, b1l);
            mfma_bf16x3(acc[1][0], a1h, a1l, b0h, b0l);
            mfma_bf16x3(acc[1][1], a1h, a1l, b1h, b1l);
        }
        if (rowsum && by == 0 && t < 128) {
#pragma unroll
            for (int r = 0; r < 32; r += 2) {
                uint32_t ph = *(const uint32_t*)&As[0][t][r], pl = *(const uint32_t*)&As[1][t][r];
                rs += (__builtin_bit_cast(float, ph << 16) + __builtin_bit_cast(float, pl << 16)) +
                      (__builtin_bit_cast(float, ph & 0xffff0000u) + __builtin_bit_cast(float, pl & 0xffff0000u));
            }
        }
        __syncthreads();
    }
    mgemm_epilogue<SPLIT, false>(acc, m0, n0, wm, wn, lc, lr, bz, bias, R, ldr, Mk, ldm, C, ldc, nullptr, 0, M, N, zs_c);
    if (rowsum && by == 0 && t < 128 && m0 + t < M) {
        if (SPLIT) rowsum[bz * zs_r + m0 + t] = rs;
        else atomicAdd(rowsum + m0 + t, rs);
    }
}

// dW (N, K) += dY (M, N)^T X (M, K) for a SKINNY X (K <= 96: lin_in's 42 / 78 inputs), db (N) += column sums of dY.  fp32.
// A block owns a row slice and 256 output rows n: thread n keeps the K accumulators of its row in registers and walks the
// slice; the X rows (the same for every thread) are staged 32 at a time through LDS and read back as broadcasts, dY is
// read coalesced.  HBM-bound on dY (4 N bytes per point).  Round 3 ran this product on the 128 x 128 fp32 MFMA tile kernel
// with 42 live columns of 128 (174 us per 49152 x 512 call, 0.6 TB/s).
template <int KMAX>
static __global__ void __launch_bounds__(256) k_grad_w_skinny(const float* __restrict__ dY, int ldy, const float* __restrict__ X,
                                                              int ldx, float* __restrict__ dW, int ldw, float* __restrict__ db,
                                                              int M, int N, int K, int rows_per_split, size_t zs_w, size_t zs_b) {
    __shared__ __attribute__((aligned(16))) float Xs[32][KMAX];      // (16-byte aligned: the broadcast reads below are ds_read_b128)
    const int t = threadIdx.x;
    const int n = blockIdx.x * 256 + t;
    dW += blockIdx.y * zs_w;
    if (db) db += blockIdx.y * zs_b;
    const int mb = blockIdx.y * rows_per_split, me = min(M, mb + rows_per_split);
    float acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
    float bs = 0.f;
    const bool live = n < N;
    for (int m0 = mb; m0 < me; m0 += 32) {
        const int nr = min(32, me - m0);
        __syncthreads();
        for (int e = t; e < 32 * KMAX; e += 256) {
            const int r = e / KMAX, k = e - r * KMAX;
            Xs[r][k] = (r < nr && k < K) ? X[(size_t)(m0 + r) * ldx + k] : 0.f;
        }
        __syncthreads();
        float g[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) g[r] = (live && r < nr) ? dY[(size_t)(m0 + r) * ldy + n] : 0.f;     // 32 loads in flight
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            bs += g[r];
#pragma unroll
            for (int k4 = 0; k4 < KMAX / 4; ++k4) {
                const float4 x4 = *(const float4*)&Xs[r][4 * k4];
                acc[4 * k4 + 0] = fmaf(g[r], x4.x, acc[4 * k4 + 0]);
                acc[4 * k4 + 1] = fmaf(g[r], x4.y, acc[4 * k4 + 1]);
                acc[4 * k4 + 2] = fmaf(g[r], x4.z, acc[4 * k4 + 2]);
                acc[4 * k4 + 3] = fmaf(g[r], x4.w, acc[4 * k4 + 3]);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)           // (compile-time indices: a run-time index would put acc[] into scratch)
            if (k < K) dW[(size_t)n * ldw + k] = acc[k];
        if (db) db[n] = bs;
    }
}

// dW (4, K) += dY(M,4)^T act(X(M,K)),  db (4) += column sums of dY — the output head (d_out = 4).  HBM-bound: 4 K bytes per
// row.  A block owns one row slice x 128 columns: thread (cq = t & 31, rl = t >> 5) takes the float4 of columns 4 cq .. + 3 of
// rows rl, rl + 8, .. of the slice (a wave reads two 512-B row segments per instruction), eight loads in flight; the eight
// row lanes are summed through LDS in a fixed order (bit-reproducible).  Round 3's form — one thread per column walking the
// whole slice, 2 x 64 blocks — was latency-bound at 0.35 TB/s (248 us per 49152 x 512 call).
template <bool RELU_X>
static __global__ void __launch_bounds__(256) k_grad_w_head(const float4* __restrict__ dY, const float* __restrict__ X,
                                                            int ldx, float* __restrict__ dW, int ldw,
                                                            float* __restrict__ db, int M, int K, int rows_per_split,
                                                            size_t zs_w, size_t zs_b) {
    __shared__ float red[8][4][132];                       // [row lane][output row][column] (+4 pad)
    __shared__ float redb[8][4];
    const int t = threadIdx.x, cq = t & 31, rl = t >> 5;
    const int k = blockIdx.x * 128 + 4 * cq;
    dW += blockIdx.y * zs_w;
    if (db) db += blockIdx.y * zs_b;
    const int mb = blockIdx.y * rows_per_split, me = min(M, mb + rows_per_split);
    float a[4][4];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) a[o][c] = 0.f;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    const bool vec = k + 3 < K && (ldx & 3) == 0 && (((uintptr_t)X) & 15) == 0;
    auto row = [&](int m, float4& x, float4& g) {
        g = dY[m];
        if (vec) x = *(const float4*)(X + (size_t)m * ldx + k);
        else {
            const float* xr = X + (size_t)m * ldx;
            x = make_float4(k < K ? xr[k] : 0.f, k + 1 < K ? xr[k + 1] : 0.f, k + 2 < K ? xr[k + 2] : 0.f, k + 3 < K ? xr[k + 3] : 0.f);
        }
    };
    auto acc = [&](float4 x, const float4& g) {
        if (RELU_X) { x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f); }
        const float gv[4] = {g.x, g.y, g.z, g.w}, xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int c = 0; c < 4; ++c) a[o][c] = fmaf(gv[o], xv[c], a[o][c]);
        b0 += g.x; b1 += g.y; b2 += g.z; b3 += g.w;
    };
    int m = mb + rl;
    for (; m + 56 < me; m += 64) {                          // eight rows of this row lane in flight
        float4 x[8], g[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) row(m + 8 * u, x[u], g[u]);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc(x[u], g[u]);
    }
    for (; m < me; m += 8) {
        float4 x, g;
        row(m, x, g);
        acc(x, g);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) red[rl][o][4 * cq + c] = a[o][c];
    if (cq == 0) { redb[rl][0] = b0; redb[rl][1] = b1; redb[rl][2] = b2; redb[rl][3] = b3; }
    __syncthreads();
    for (int e = t; e < 4 * 128; e += 256) {                 // (output row o, column c): the eight row lanes in order
        const int o = e >> 7, c = e & 127;
        float sum = red[0][o][c];
#pragma unroll
        for (int r = 1; r < 8; ++r) sum += red[r][o][c];
        if (blockIdx.x * 128 + c < K) dW[(size_t)o * ldw + blockIdx.x * 128 + c] = sum;
    }
    if (db && blockIdx.x == 0 && t < 4) {
        float sum = redb[0][t];
#pragma unroll
        for (int r = 1; r < 8; ++r) sum += redb[r][t];
        db[t] = sum;
    }
}

// d(pre-activation) of the output head: rgb = sigmoid(o) -> y(1-y); sigma = relu(o) -> [y > 0]
static __global__ void k_out_act_bwd(const float4* __restrict__ out, const float4* __restrict__ d_out, int64_t n,
                                     float4* __restrict__ d_o4) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 y = out[i], g = d_out[i];
    g.x *= y.x * (1.0f - y.x);
    g.y *= y.y * (1.0f - y.y);
    g.z *= y.z * (1.0f - y.z);
    g.w = (y.w > 0.f) ? g.w : 0.f;
    d_o4[i] = g;
}

// backward of util.combine_interleaved (util.py:466-476): mean -> g/NS to every view; max -> g to the
// (first) arg-max view.  xpre (NS, per_view) is the saved per-view input of the reduction.
static __global__ void k_combine_bwd(const float* __restrict__ g, const float* __restrict__ xpre, int NS,
                                     int64_t per_view, int combine_type, float* __restrict__ gv) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per_view) return;
    float gi = g[i];
    if (combine_type == PNR_COMBINE_MAX) {
        int best = 0;
        float bv = xpre[i];
        for (int v = 1; v < NS; ++v) {
            float a = xpre[i + v * per_view];
            if (a > bv) { bv = a; best = v; }
        }
        for (int v = 0; v < NS; ++v) gv[i + v * per_view] = (v == best) ? gi : 0.f;
    } else {
        float s = gi / (float)NS;
        for (int v = 0; v < NS; ++v) gv[i + v * per_view] = s;
    }
}

// backward of the feature build (k_features_f32): one wave per point, views in sequence.
//   d_latent[level][view][c][tap] += dzx[row][c] * w_tap                       (encoder.py:182,198 grid_sample)
//   d(point) through the projection (backup2:215-221) and the positional code (code.py:30-46)
// dzx rows are view-major (row = v*P + g).  d_lat entries may be NULL (encoder frozen); d_xyz / d_z may be NULL.
// p: the caller's d_latent maps (fp32, NCHW).  q (round 4; maps beyond the LDS path): per level a 64-bit FIXED-POINT copy of
// the same map in the backward workspace that the taps are summed into with integer atomics — integer addition commutes, so
// the sum does not depend on the order the contributions arrive in: the latent gradient of DTU-sized and multi-scale maps is
// bit-reproducible from run to run like every other gradient.  scale_bits: the map's common binary exponent (k_latq_scale).
struct LatGrad { float* p[PNR_MAX_LEVELS]; long long* q[PNR_MAX_LEVELS]; const int* scale_bits; };

// max |dzx[:, :L]| as float bits (atomicMax on the bits of a non-negative float is an order-independent integer maximum)
static __global__ void __launch_bounds__(256) k_abs_max_cols(const float* __restrict__ x, int64_t rows, int ld, int L, unsigned* __restrict__ out) {
    float m = 0.f;
    unsigned bad = 0u;
    const int64_t n = rows * L;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / L;
        const float v = fabsf(x[r * ld + (i - r * L)]);
        if (v <= __FLT_MAX__) m = fmaxf(m, v);                // every finite value sets the scale (up to 3.40282347e38)
        else bad = 1u;                                        // NaN / inf: remembered in out[1], k_latq_finalize propagates it
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(out, __float_as_uint(m));
    if (bad) atomicOr(out + 1, 1u);
}
// The fixed-point scale 2^s of the maps: every contribution is |g w| <= max|g| < 2^ex and a map entry sums at most n_terms of
// them, so with s = 61 - ex - ceil(log2(n_terms)) no partial sum can leave the int64 range, and the resolution 2^-s is
// ~2^-40 of the largest gradient element (fp32 atomics resolve 2^-24 of the running sum).
static __global__ void k_latq_scale(const unsigned* __restrict__ max_bits, long long n_terms, int* __restrict__ scale_bits) {
    const float mx = __uint_as_float(*max_bits);
    int ex = 0;
    if (mx > 0.f) (void)frexpf(mx, &ex);                      // mx < 2^ex
    int lg = 0;
    while ((1ll << lg) < n_terms && lg < 62) ++lg;
    int sb = 61 - ex - lg;
    sb = sb > 1000 ? 1000 : sb < -1000 ? -1000 : sb;
    *scale_bits = sb;
}
// d_latent += fixed-point map * 2^-s
static __global__ void k_latq_finalize(const long long* __restrict__ q, int64_t n, const int* __restrict__ scale_bits,
                                       const unsigned* __restrict__ nonfinite, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // a non-finite incoming gradient has no fixed-point image: the whole map says so, as the reference's float sum would in
    // the entries it reaches
    out[i] += *nonfinite ? __builtin_nanf("") : (float)ldexp((double)q[i], -*scale_bits);
}

static __global__ void __launch_bounds__(256) k_features_bwd(
    pnr_views vw, PointSrc src, int64_t P, int64_t pts_per_obj, int L, int d_in, int use_code_viewdirs,
    int num_freqs, float freq_factor, const float* __restrict__ dzx, int ldz, LatGrad dl, float* __restrict__ d_xyz,
    float* __restrict__ d_z) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (g >= P) return;
    const bool want_p = (d_xyz != nullptr) || (d_z != nullptr);
    float p[3], d[3];
    fetch_point(src, g, p, d);
    const int obj = (int)(g / pts_per_obj);
    float dp[3] = {0.f, 0.f, 0.f};
    for (int v = 0; v < vw.n_views; ++v) {
        const int view = obj * vw.n_views + v;
        Cam cam = load_cam(vw, view);
        float xr[3];
        rot3(cam.R, p, xr);
        float u, w;
        project(cam, xr, u, w);
        const float* drow = dzx + ((size_t)v * P + g) * ldz;
        float du = 0.f, dv = 0.f;
        int c0 = 0;
        for (int lvl = 0; lvl < vw.n_levels; ++lvl) {
            const int W = vw.lat_w[lvl], H = vw.lat_h[lvl], C = vw.lat_c[lvl];
            const float usx = uv_sx(vw, lvl), usy = uv_sy(vw, lvl);      // d(texel coordinate) / d(uv)
            Taps t = bilinear_taps(u * usx, w * usy, W, H);
            TapsGrad tg = bilinear_taps_grad(u * usx, w * usy, W, H);
            for (int ch = lane; ch < C; ch += 64) {
                float gz = drow[c0 + ch];
                size_t base = ((size_t)view * C + ch) * (size_t)(H * W);
                if (dl.p[lvl]) {
                    if (dl.q[lvl]) {          // order-independent: 64-bit fixed-point integer atomics (see LatGrad)
                        const double sc = ldexp(1.0, *dl.scale_bits);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (t.w[i] != 0.f)
                                atomicAdd((unsigned long long*)(dl.q[lvl] + base + t.off[i]),
                                          (unsigned long long)__double2ll_rn((double)(gz * t.w[i]) * sc));
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (t.w[i] != 0.f) atomicAdd(dl.p[lvl] + base + t.off[i], gz * t.w[i]);
                    }
                }
                if (want_p) {
                    const float* lb = vw.latent[lvl] + base;
                    float sx = 0.f, sy = 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float val = lb[t.off[i]];
                        sx += val * tg.dx[i];
                        sy += val * tg.dy[i];
                    }
                    du += gz * (sx * usx);
                    dv += gz * (sy * usy);
                }
            }
            c0 += C;
        }
        if (!want_p) continue;
        // positional code: lanes over the code entries, partial d(x_rot) per lane
        float dxr[3] = {0.f, 0.f, 0.f};
        const int dd = use_code_viewdirs ? 6 : 3;
        const int dcode = dd + 2 * num_freqs * dd;        // entries produced by the code
        for (int j = lane; j < dcode; j += 64) {
            float gc = drow[L + j];
            int i;
            float dv_dx;
            if (j < dd) { i = j; dv_dx = 1.0f; }
            else {
                int q = (j - dd) / dd;
                i = (j - dd) % dd;
                float f = freq_factor * (float)(1 << (q >> 1));
                float ph = (q & 1) ? 1.57079637050628662109375f : 0.0f;
                dv_dx = (i < 3) ? f * cosf(fmaf(xr[i], f, ph)) : 0.f;
            }
            if (i < 3) dxr[i] += gc * dv_dx;
        }
        du = wave_sum(du); dv = wave_sum(dv);
        dxr[0] = wave_sum(dxr[0]); dxr[1] = wave_sum(dxr[1]); dxr[2] = wave_sum(dxr[2]);
        float xc = xr[0] + cam.t[0], yc = xr[1] + cam.t[1], zc = xr[2] + cam.t[2];
        dxr[0] += du * (-cam.fx / zc);
        dxr[1] += dv * (-cam.fy / zc);
        dxr[2] += du * (xc * cam.fx / (zc * zc)) + dv * (yc * cam.fy / (zc * zc));
        // p = R^T x_rot
        dp[0] += cam.R[0] * dxr[0] + cam.R[3] * dxr[1] + cam.R[6] * dxr[2];
        dp[1] += cam.R[1] * dxr[0] + cam.R[4] * dxr[1] + cam.R[7] * dxr[2];
        dp[2] += cam.R[2] * dxr[0] + cam.R[5] * dxr[1] + cam.R[8] * dxr[2];
    }
    if (lane == 0) {
        if (d_xyz) { d_xyz[g * 3 + 0] = dp[0]; d_xyz[g * 3 + 1] = dp[1]; d_xyz[g * 3 + 2] = dp[2]; }
        if (d_z) d_z[g] = dp[0] * d[0] + dp[1] * d[1] + dp[2] * d[2];
    }
}

// Latent gradient for ONE small map (C*T floats fit in LDS), bit-reproducible: a block owns a run of points of one
// (object, view); thread t owns channels t, t + 256, .. and walks the run's points IN ORDER, adding their four tap
// contributions into its own entries of an LDS map ([texel][channel]) — no entry is ever touched by two threads, so there
// is no atomic and no race inside the block.  The block's partial map goes to its own slice of the backward workspace and
// k_latent_reduce sums the slices in block order into d_latent (+=).  Replaces round 2's LDS float atomics + global
// atomics (sum order = arrival order).  dzx rows are view-major (row = v*P + g).
static constexpr int LATG_PPB = 256;                      // points per block (the tap table: 8 KiB of LDS)
static __global__ void __launch_bounds__(256) k_latent_grad_lds(
    pnr_views vw, PointSrc src, int64_t P, int64_t pts_per_obj, int L, const float* __restrict__ dzx, int ldz,
    float* __restrict__ part /* (blocks_x, views, T*C) */) {
    extern __shared__ float acc[];                         // [T][C], then the tap table
    const int C = vw.lat_c[0], W = vw.lat_w[0], H = vw.lat_h[0], T = W * H;
    int* tap_off = (int*)(acc + (size_t)T * C);            // [LATG_PPB][4]
    float* tap_w = (float*)(tap_off + LATG_PPB * 4);       // [LATG_PPB][4]
    const int view = blockIdx.y, obj = view / vw.n_views, v = view % vw.n_views;
    const int64_t g0 = (int64_t)obj * pts_per_obj + (int64_t)blockIdx.x * LATG_PPB;
    const int64_t g1 = min((int64_t)(obj + 1) * pts_per_obj, g0 + LATG_PPB);
    const int n = (int)(g1 - g0);
    for (int i = threadIdx.x; i < T * C; i += 256) acc[i] = 0.f;
    if ((int)threadIdx.x < n) {                            // one thread per point: its four taps
        float p[3], d[3], xr[3], u, w;
        const Cam cam = load_cam(vw, view);
        fetch_point(src, g0 + threadIdx.x, p, d);
        rot3(cam.R, p, xr);
        project(cam, xr, u, w);
        const Taps t = bilinear_taps(u * uv_sx(vw, 0), w * uv_sy(vw, 0), W, H);
#pragma unroll
        for (int i = 0; i < 4; ++i) { tap_off[threadIdx.x * 4 + i] = t.off[i]; tap_w[threadIdx.x * 4 + i] = t.w[i]; }
    }
    __syncthreads();
    for (int ch = threadIdx.x; ch < C; ch += 256) {        // the owner of channel ch, points in order
        const float* dcol = dzx + ((size_t)v * P + g0) * ldz + ch;
        // sixteen points' gradients in flight (the walk itself stays in point order: one global round trip per point made
        // this loop latency-bound, 133 us per 49152-point call)
        for (int q0 = 0; q0 < n; q0 += 16) {
            float gz[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) gz[j] = (q0 + j < n) ? dcol[(size_t)(q0 + j) * ldz] : 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int q = q0 + j;
                if (q < n) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float wgt = tap_w[q * 4 + i];
                        if (wgt != 0.f) acc[tap_off[q * 4 + i] * C + ch] += gz[j] * wgt;
                    }
                }
            }
        }
    }
    __syncthreads();
    float* out = part + ((size_t)blockIdx.x * gridDim.y + view) * (size_t)T * C;
    for (int i = threadIdx.x; i < T * C; i += 256) out[i] = acc[i];
}

// d_lat (view, C, H, W) += sum over the blocks' partial maps ([texel][channel]) in block order
static __global__ void k_latent_reduce(const float* __restrict__ part, int nbx, int views, int C, int T, float* __restrict__ d_lat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;        // over (view, texel, channel)
    if (i >= (int64_t)views * T * C) return;
    const int view = (int)(i / ((int64_t)T * C)), r = (int)(i % ((int64_t)T * C));
    float a = 0.f;
    for (int b = 0; b < nbx; ++b) a += part[((size_t)b * views + view) * (size_t)T * C + r];
    d_lat[(size_t)view * C * T + (size_t)(r % C) * T + r / C] += a;
}

// ------------------------------------------------------------------ composite backward (nerf.py:178-182,223-249)
// One wave per ray, samples walked from the far end so the suffix sum S_k = sum_{j>k} G_j w_j is a running
// carry:  G_k = dL/dw_k = gw_k + g_rgb.c_k + g_depth z_k - [white] sum(g_rgb);
//         dL/dalpha_k = G_k T_k - S_k / (1 - alpha_k + 1e-10);   alpha = 1 - exp(-delta relu(sigma)).
static __global__ void __launch_bounds__(256) k_composite_bwd(
    const float* __restrict__ rays, const float* __restrict__ z, const float4* __restrict__ rgbs, int64_t n_rays,
    int K, int white_bkgd, const float* __restrict__ g_w, const float* __restrict__ g_rgb,
    const float* __restrict__ g_depth, float4* __restrict__ d_rgbs, float* __restrict__ d_z) {
    extern __shared__ float smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
    if (ray >= n_rays) return;
    float* Tk = smem + (size_t)wv * 3 * K;       // exclusive transmittance
    float* dD = Tk + K;                           // d(delta_k)
    float* dZ = dD + K;                           // direct term of depth = sum w z
    const float far = rays[ray * 8 + 7];
    const float* zr = z + ray * K;
    const float4* cr = rgbs + ray * K;
    // forward transmittance, as k_composite
    float carry = 1.0f;
    for (int k0 = 0; k0 < K; k0 += 64) {
        int k = k0 + lane;
        bool act = k < K;
        float zk = act ? zr[k] : 0.f;
        float zn = (k + 1 < K) ? zr[k + 1] : far;
        float sg = act ? fmaxf(cr[k].w, 0.0f) : 0.f;
        float alpha = act ? 1.0f - expf(-(zn - zk) * sg) : 0.0f;
        float tr = act ? (1.0f - alpha) + 1e-10f : 1.0f;
        float incl = wave_scan_mul(tr, lane);
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 1.0f;
        if (act) Tk[k] = carry * excl;
        carry *= __shfl(incl, 63, 64);
    }
    const float gr = g_rgb ? g_rgb[ray * 3 + 0] : 0.f, gg = g_rgb ? g_rgb[ray * 3 + 1] : 0.f,
                gb = g_rgb ? g_rgb[ray * 3 + 2] : 0.f, gd = g_depth ? g_depth[ray] : 0.f;
    const float gbg = white_bkgd ? (gr + gg + gb) : 0.f;
    float suffix = 0.f;                           // S for the highest k of the current segment
    const int nseg = (K + 63) / 64;
    for (int sgm = nseg - 1; sgm >= 0; --sgm) {
        int k = sgm * 64 + (63 - lane);           // lane 0 holds the farthest sample of the segment
        bool act = k < K;
        float zk = act ? zr[k] : 0.f;
        float zn = (k + 1 < K) ? zr[k + 1] : far;
        float4 c = act ? cr[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        float delta = zn - zk;
        float sg = fmaxf(c.w, 0.0f);
        float e = expf(-delta * sg);
        float alpha = act ? 1.0f - e : 0.f;
        float T = act ? Tk[k] : 0.f;
        float w = alpha * T;
        float G = (g_w ? (act ? g_w[ray * K + k] : 0.f) : 0.f) + gr * c.x + gg * c.y + gb * c.z + gd * zk - gbg;
        float gwk = act ? G * w : 0.f;
        float incl = wave_scan_add(gwk, lane);    // inclusive over farther-or-equal samples of this segment
        float S = suffix + incl - gwk;            // strictly farther samples
        suffix += __shfl(incl, 63, 64);
        float dalpha = G * T - S / ((1.0f - alpha) + 1e-10f);
        float dsig = (c.w > 0.f) ? dalpha * delta * e : 0.f;
        float ddel = dalpha * sg * e;
        if (act) {
            d_rgbs[ray * K + k] = make_float4(w * gr, w * gg, w * gb, dsig);
            dD[k] = ddel;
            dZ[k] = w * gd;
        }
    }
    if (d_z) {
        __builtin_amdgcn_wave_barrier();
        // delta_k = z_{k+1} - z_k (k < K-1), delta_{K-1} = far - z_{K-1}
        for (int k = lane; k < K; k += 64)
            d_z[ray * K + k] = dZ[k] - dD[k] + ((k > 0) ? dD[k - 1] : 0.f);
    }
}

// ------------------------------------------------------------------ depth-guided samples backward (nerf.py:150-161,287-295)
// z_d = clamp(depth + g*std, near, far) is differentiable in depth; after cat + sort the sample sits at the
// slot holding its value.  d(depth) = sum over unclamped depth samples of d(z_sorted) at that slot.
static __global__ void __launch_bounds__(256) k_sample_fine_bwd(
    const float* __restrict__ rays, const float* __restrict__ depth, int64_t n_rays, int Kt, int n_dep,
    float depth_std, const float* __restrict__ gn, uint64_t seed, int64_t ray_base,
    const float* __restrict__ z_sorted, const float* __restrict__ d_z_sorted, float* __restrict__ d_depth) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const float near = rays[ray * 8 + 6], far = rays[ray * 8 + 7];
    const float dpt = depth[ray];
    const float* zs = z_sorted + ray * Kt;
    const float* gz = d_z_sorted + ray * Kt;
    float acc = 0.f;
    for (int j = lane; j < n_dep; j += 64) {
        float g = gn ? gn[ray * n_dep + j] : rng_normal(seed, ray_base + ray, DRAW_G, j);
        float zz = dpt + g * depth_std;
        if (!(zz < far) || !(zz > near)) continue;        // clamped: torch.min / torch.max route the gradient to the bound
        // first slot holding zz (ascending row): lower bound
        int lo = 0, hi = Kt;
        while (lo < hi) {
            int mid = (lo + hi) >> 1;
            if (zs[mid] < zz) lo = mid + 1; else hi = mid;
        }
        // equal values among the depth samples of one ray occupy consecutive slots: rank among equal earlier samples
        int rank = 0;
        for (int jj = 0; jj < j; ++jj) {
            float g2 = gn ? gn[ray * n_dep + jj] : rng_normal(seed, ray_base + ray, DRAW_G, jj);
            float z2 = dpt + g2 * depth_std;
            rank += (z2 == zz) ? 1 : 0;
        }
        int slot = lo + rank;
        if (slot < Kt && zs[slot] == zz) acc += gz[slot];
    }
    acc = wave_sum(acc);
    if (lane == 0) d_depth[ray] = acc;
}


// ------------------------------------------------------------------ host side
// Operands of the dispatchers below.  Mat: a row-major matrix named once — its fp32 form, its bf16 twin (either may be NULL; both
// NULL: no such operand) and the leading dimension the two share.  Activations, the relu mask, the residual and the result are
// all Mats; only the bf16-product kernels read or write a b16 form (the 16-bit tape's).
struct Mat { const float* f32; const uint16_t* b16; int ld; };
static constexpr Mat NO_MAT{nullptr, nullptr, 0};
static inline Mat f32_mat(const float* p, int ld) { return Mat{p, nullptr, ld}; }
static inline Mat f32_only(const Mat& m) { return f32_mat(m.f32, m.ld); }
// Weight: W as nn.Linear stores it + this step's copies laid out (N, K) for THE product it is passed to (W itself for
// y = x W^T, W^T for dX = dY W): nk16 as bf16 — with a bf16 activations operand the GEMM then runs on k_hgemm_dma — and nk32 as
// fp32, the row-contiguous operand k_sgemm_dma wants for a dX product.  NULL when the shapes do not suit those kernels.
struct Weight { const float* f32; int ld; const uint16_t* nk16; const float* nk32; };
static inline Weight plain_weight(const float* w, int ld) { return Weight{w, ld, nullptr, nullptr}; }

struct Tape {
    int H, L, E;                     // d_hidden, d_latent, row stride of zx
    float* zx;                       // (NS*P, E)
    float* A[PNR_MAX_BLOCKS + 1];    // block inputs after lin_z; A[n_blocks] = input of lin_out
    float* h[PNR_MAX_BLOCKS];        // fc_0 outputs (pre-activation)
    float* xpre;                     // (NS*P, H) per-view stream entering the view reduction (NS > 1)
    float* o4;                       // (P, 4) head pre-activations
    int64_t rows[PNR_MAX_BLOCKS + 1];
    uint64_t total;
    // 16-bit tape (train_precision = "bf16"): the block inputs and fc_0 outputs are kept as bf16 — exactly the values the
    // bf16-product GEMMs stage anyway, so gradients are bit-identical to the fp32 tape's — and the fp32 residual stream the
    // forward keeps adding to lives in two ping-pong buffers (stream()).
    bool h16;
    uint16_t* A16[PNR_MAX_BLOCKS + 1];
    uint16_t* h16p[PNR_MAX_BLOCKS];
    float* xw[2];
    // bf16 copies of fc_0 / fc_1 of every block, as stored (forward) and transposed (dX), written by the forward: the
    // operands of k_hgemm_dma (index 2 b: fc_0, 2 b + 1: fc_1); NULL when d_hidden does not suit that kernel
    uint16_t* Wb[2 * PNR_MAX_BLOCKS];
    uint16_t* Wt[2 * PNR_MAX_BLOCKS];
    // the same for the lin_z products (forward and weight gradient): bf16 copy of zx's latent columns (rows x L) and of lin_z's
    // weights; NULL when d_latent does not suit the kernels
    uint16_t* z16;
    uint16_t* Wz[PNR_MAX_BLOCKS];
    uint16_t* Wzt[PNR_MAX_BLOCKS];       // lin_z^T (L, H): the operand of d(out)/d(latent columns) = dx . W_z
    // fp32 tape, fp32 products: W^T of every hidden weight (2 b: fc_0, 2 b + 1: fc_1) and of lin_z, written by the forward — the
    // row-contiguous operand k_sgemm_dma wants for the dX products
    float* Wt32[2 * PNR_MAX_BLOCKS];
    float* Wzt32[PNR_MAX_BLOCKS];
    LatCL lat_cl;                        // channels-last fp32 copies of the latent maps for the feature build (latent_cl_build)

    // the fp32 residual stream entering block b (b = n_blocks: entering lin_out, read by non-MFMA kernels): its tape slot, or
    // on the 16-bit tape the ping-pong buffer of that block — every block writes the other one
    float* stream(int b) const { return h16 ? xw[b & 1] : A[b]; }
    // what the tape keeps of a block, in whichever form it keeps it: the block's input and fc_0's output (GEMM operands in
    // the forward, operands and relu masks in the backward), and the latent columns of zx (lin_z's operand)
    Mat block_in(int b) const { return Mat{A[b], A16[b], H}; }
    Mat hidden(int b) const { return Mat{h[b], h16p[b], H}; }
    Mat z() const { return z16 ? Mat{nullptr, z16, L} : f32_mat(zx, E); }
    // a hidden weight (i = 2 b: fc_0, 2 b + 1: fc_1) / lin_z of block b with the step's copies for y = x W^T and for dX = dY W
    Weight hidden_w(const float* w, int i) const { return Weight{w, H, Wb[i], nullptr}; }
    Weight hidden_w_dx(const float* w, int i) const { return Weight{w, H, Wt[i], Wt32[i]}; }
    Weight lin_z_w(const float* w, int b) const { return Weight{w, L, Wz[b], nullptr}; }
    Weight lin_z_w_dx(const float* w, int b) const { return Weight{w, L, Wzt[b], Wzt32[b]}; }
};
static inline bool dma_gemm_ok(const pnr_mlp* mlp) { return mlp->d_hidden % 128 == 0; }
static inline bool dma_lin_z_ok(const pnr_mlp* mlp) { return dma_gemm_ok(mlp) && mlp->d_latent > 0 && mlp->d_latent % 128 == 0; }

// the bf16-product mode keeps a 16-bit tape when every hidden GEMM takes the bf16 MFMA kernel (d_hidden a multiple of 32)
static bool tape_is_16bit(const pnr_params* prm, const pnr_mlp* mlp) {
    return prm && prm->precision == PNR_BF16 && prm->train_tape_fp32 == 0 && mlp->d_hidden >= 32 && mlp->d_hidden % 32 == 0;
}

static Tape carve_tape(const pnr_mlp* mlp, const pnr_views* vw, int64_t P, void* base, bool h16 = false) {
    Tape t{};
    t.h16 = h16;
    t.H = mlp->d_hidden; t.L = mlp->d_latent; t.E = feature_stride(mlp);
    const int NS = vw->n_views, H = t.H, L = t.L, nz = n_lin_z(mlp);
    Bump bump(round_up_256(base));      // 256-byte pieces, + 256 for the rounding
    auto take = [&](uint64_t floats) { return bump.take<float>(floats, 256); };
    auto take16 = [&](uint64_t halves) { return bump.take<uint16_t>(halves, 256); };
    t.zx = take((uint64_t)NS * P * t.E);
    if (h16) {
        t.xw[0] = take((uint64_t)NS * P * H);
        t.xw[1] = take((uint64_t)NS * P * H);
    }
    for (int b = 0; b <= mlp->n_blocks; ++b) {
        t.rows[b] = (NS > 1 && b >= mlp->combine_layer) ? P : (int64_t)NS * P;
        if (h16) {
            t.A16[b] = take16((uint64_t)t.rows[b] * H);
            if (b < mlp->n_blocks) t.h16p[b] = take16((uint64_t)t.rows[b] * H);
        } else {
            t.A[b] = take((uint64_t)t.rows[b] * H);
            if (b < mlp->n_blocks) t.h[b] = take((uint64_t)t.rows[b] * H);
        }
    }
    t.xpre = NS > 1 ? take((uint64_t)NS * P * H) : nullptr;
    t.o4 = take((uint64_t)P * 4);
    if (h16 && dma_gemm_ok(mlp))
        for (int i = 0; i < 2 * mlp->n_blocks; ++i) { t.Wb[i] = take16((uint64_t)H * H); t.Wt[i] = take16((uint64_t)H * H); }
    if (L > 0) { bump.pad(256); t.lat_cl = latent_cl_carve(bump, *vw); }
    if (!h16 && H % 16 == 0) {
        for (int i = 0; i < 2 * mlp->n_blocks; ++i) t.Wt32[i] = take((uint64_t)H * H);
        if (L > 0 && L % 4 == 0)
            for (int b = 0; b < nz; ++b) t.Wzt32[b] = take((uint64_t)H * L);
    }
    if (h16 && dma_lin_z_ok(mlp)) {
        t.z16 = take16((uint64_t)NS * P * L);
        for (int b = 0; b < nz; ++b) { t.Wz[b] = take16((uint64_t)H * L); t.Wzt[b] = take16((uint64_t)H * L); }
    }
    bump.take<uint8_t>(256, 256);
    t.total = bump.off;
    return t;
}

uint64_t train_tape_bytes(const pnr_mlp* mlp, const pnr_views* vw, int64_t P) {
    return carve_tape(mlp, vw, P, nullptr).total;
}
uint64_t train_tape_bytes_p(const pnr_params* prm, const pnr_mlp* mlp, const pnr_views* vw, int64_t P) {
    return carve_tape(mlp, vw, P, nullptr, tape_is_16bit(prm, mlp)).total;
}

// Scratch for the weight gradients (carved from the backward workspace): every row split of a dW GEMM writes its own
// (N, K) slice, the slices are then summed in a fixed order — no fp32 atomics race, so gradients are reproducible.
struct DetWs { float* part; uint64_t floats; };
static constexpr int DET_MAX_SPLITS = 64;
static uint64_t det_ws_floats(const pnr_mlp* mlp) {
    const uint64_t H = mlp->d_hidden, L = mlp->d_latent, D = mlp->d_in;
    uint64_t wmax = H * H;
    if (H * L > wmax) wmax = H * L;
    if (H * D > wmax) wmax = H * D;
    return (uint64_t)DET_MAX_SPLITS * (wmax + H);
}

// one small single-level map: the latent gradient runs on per-block partial maps (k_latent_grad_lds); bytes of the slices
// dynamic LDS k_latent_grad_lds needs for this map: the [T][C] accumulator + the tap table of a block's points
static size_t latent_grad_lds_bytes(const pnr_views* vw) {
    return (size_t)vw->lat_c[0] * vw->lat_h[0] * vw->lat_w[0] * 4 + (size_t)LATG_PPB * 4 * 8;
}
// LDS a block may ask for on this device (gfx950: 160 KiB)
static size_t lds_per_block_limit() {
    static PerDevice cache;
    return (size_t)device_attr(cache, hipDeviceAttributeMaxSharedMemoryPerBlock, 64 * 1024);
}
static bool latent_grad_in_lds(const pnr_views* vw) {
    // the real requirement (map + tap table) against what the device grants; maps up to 64 KiB as before
    return vw->n_levels == 1 && (size_t)vw->lat_c[0] * vw->lat_h[0] * vw->lat_w[0] * 4 <= 64 * 1024 &&
           latent_grad_lds_bytes(vw) <= lds_per_block_limit();
}
static uint64_t latent_part_bytes(const pnr_views* vw, int64_t P) {
    if (!latent_grad_in_lds(vw) || vw->n_objs < 1) return 0;
    const uint64_t nbx = ((uint64_t)(P / vw->n_objs) + LATG_PPB - 1) / LATG_PPB;
    return nbx * vw->n_objs * vw->n_views * (uint64_t)vw->lat_c[0] * vw->lat_h[0] * vw->lat_w[0] * 4;
}

// maps that take the fixed-point route (everything the LDS path does not serve): 8 bytes per map element + the scale words
static uint64_t latent_q_bytes(const pnr_views* vw) {
    if (latent_grad_in_lds(vw)) return 0;
    uint64_t n = 0;
    for (int l = 0; l < vw->n_levels; ++l)
        n += (uint64_t)vw->n_objs * vw->n_views * vw->lat_c[l] * vw->lat_h[l] * vw->lat_w[l];
    return n * 8 + 256;
}
// The backward's workspace (256-byte pieces behind a base rounded up to 256, + that slack): the gradient stream and its second
// buffer, dh (16-bit tape: the two bf16 streams overlay it, see point_bwd), the gradient at the assembled rows, at the head's
// output, the weight-gradient slices, and the latent gradient's partial maps or fixed-point maps.
struct TrainBwdWs {
    float *dx, *dx2, *dh, *dzx, *do4;
    DetWs dws;
    float* lat_part;
    uint8_t* lat_q;        // [scale words (256 B)][fixed-point maps], latent_q_bytes
};
static TrainBwdWs carve_train_bwd(Bump& b, const pnr_mlp* mlp, const pnr_views* vw, int64_t P) {
    const uint64_t MV = (uint64_t)vw->n_views * P, H = mlp->d_hidden, E = feature_stride(mlp);
    TrainBwdWs w;
    w.dx = b.take<float>(MV * H, 256);
    w.dx2 = b.take<float>(MV * H, 256);
    w.dh = b.take<float>(MV * H, 256);
    w.dzx = b.take<float>(MV * E, 256);
    w.do4 = b.take<float>((uint64_t)P * 4, 256);
    w.dws = DetWs{b.take<float>(det_ws_floats(mlp), 256), det_ws_floats(mlp)};
    w.lat_part = (float*)b.take<uint8_t>(latent_part_bytes(vw, P), 256);
    w.lat_q = b.take<uint8_t>(latent_q_bytes(vw), 256);
    b.take<uint8_t>(256, 256);
    return w;
}
uint64_t train_bwd_workspace_bytes(const pnr_mlp* mlp, const pnr_views* vw, int64_t P) {
    return bytes_of([&](Bump& b) { carve_train_bwd(b, mlp, vw, P); });
}

static inline int vec_flags(const float* A, int lda, const float* B, int ldb) {
    return ((((uintptr_t)A & 15) == 0 && lda % 4 == 0) ? 1 : 0) | ((((uintptr_t)B & 15) == 0 && ldb % 4 == 0) ? 2 : 0);
}

static inline bool al16(const void* p, int ld) { return ((uintptr_t)p & 15) == 0 && ld % 4 == 0; }

// What a dispatcher below launched (gemm / head_dx / grad_w), for pnr_debug_linear only: production calls pass no record, so the
// dispatch costs one pointer test per launch.  id: PNR_DBG_K_* of the launch site; epi: PNR_DBG_EPI_* of a tile kernel's
// epilogue (evaluated with the kernel's own arguments); splits / rows / reduce: the row slicing of a weight gradient.
struct DbgSite { int id, epi, splits, rows, reduce; };
// a tile kernel's epilogue arguments, and which epilogue it has: mgemm_epilogue (registers), or tile_epilogue_lds where it qualifies
struct EpiArgs {
    const float* bias; const float* R; int ldr; const void* Mk; int ldm; bool m16; const float* C; int ldc; const uint16_t* C16; int ldc16; int N;
};
enum EpiKind { EPI_NOT_TILE, EPI_REG, EPI_LDS };
static int epilogue_form(bool lds_kernel, const EpiArgs& e) {
    if (lds_kernel && tile_epilogue_ok(e.bias, e.R, e.ldr, e.Mk, e.ldm, e.m16, e.C, e.ldc, e.C16, e.ldc16, e.N))
        return tile_epilogue_c16_only(e.m16, e.R, e.Mk, e.ldm, e.C, e.C16, e.ldc16, e.N) ? PNR_DBG_EPI_LDS_C16 : PNR_DBG_EPI_LDS;
    return mgemm_vec_ok(e.bias, e.R, e.ldr, e.Mk, e.ldm, e.m16, e.C, e.ldc, e.C16, e.ldc16, 0) ? PNR_DBG_EPI_REG_VEC : PNR_DBG_EPI_REG_ELEM;
}

// The tail every candidate of a dispatcher shares: the debug record, the launch, the launch check.
template <class Launch>
static int32_t launch_site(DbgSite* dbg, int id, EpiKind kind, const EpiArgs* e, Launch&& launch) {
    if (dbg) {
        dbg->id = id;
        if (kind != EPI_NOT_TILE) dbg->epi = epilogue_form(kind == EPI_LDS, *e);
    }
    launch();
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

// Runtime booleans -> template flags: f(std::bool_constant<flag>{}...), so a launch picks its kernel instantiation with flag()
template <class F> static inline void with_flags(F&& f) { f(); }
template <class F, class... Rest> static inline void with_flags(F&& f, bool flag, Rest... rest) {
    if (flag) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
    else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// Y (M, N) = res + mask( act(x) op(W) + b ): the forward (TRANS_W = false: y = x W^T) and dX (TRANS_W = true: dX = dY W) products
// of the taped step; the first candidate whose predicate holds is launched.  b, res, mask may be absent; res may alias y.
// mode: 0 = fp32 MFMA, 1 = bf16 MFMA, 3 = bf16x3 split (fp32-class) products on fp32 operands, or PNR_DBG_MODE_TAPE16: the
// 16-bit-tape forms of a bf16 product (pnr.h: gemm16) — x.b16 (the activations as bf16, instead of x.f32), mask.b16 (the relu
// mask as bf16, instead of mask.f32), y.b16 (a bf16 copy of the result; y.f32 may then be NULL) and w.nk16.  Only that mode
// reads or writes a b16 form; only the fp32-product dX reads w.nk32.
template <bool RELU_X, bool TRANS_W>
static int32_t gemm(const Mat& x, const Weight& w, const float* b, const Mat& res, const Mat& mask, const Mat& y, int64_t M, int N, int K,
                    int mode, hipStream_t s, DbgSite* dbg = nullptr) {
    if (M == 0) return PNR_OK;
    const float* X = x.f32; const float* W = w.f32; const float* R = res.f32; const float* Mk = mask.f32;
    float* Y = const_cast<float*>(y.f32);
    const int ldx = x.ld, ldw = w.ld, ldr = res.ld, ldm = mask.ld, ldy = y.ld;
    const dim3 tiles = mgemm_grid((M + 127) / 128, (N + 127) / 128), blk(256);       // of the 128 x 128 tile kernels
    if (mode == PNR_DBG_MODE_TAPE16) {
        const uint16_t* X16 = x.b16; const uint16_t* Mk16 = mask.b16; const uint16_t* W16 = w.nk16;
        uint16_t* Y16 = const_cast<uint16_t*>(y.b16);
        if (!(N >= 32 && K >= 32 && K % 32 == 0 && N % 4 == 0 && al16(W, ldw))) return PNR_E_UNSUPPORTED;
        const void* Xp = X16 ? (const void*)X16 : (const void*)X;
        const void* Mp = Mk16 ? (const void*)Mk16 : (const void*)Mk;
        const EpiArgs e{b, R, ldr, Mp, ldm, Mk16 != nullptr, Y, ldy, Y16, ldy, N};
        // both operands bf16 and row-contiguous in the reduction index: the LDS-DMA k-loop (W16 is (N, K), leading dimension K)
        if (X16 && W16 && K % 64 == 0 && ldx % 8 == 0 && ((uintptr_t)X16 & 15) == 0 && ((uintptr_t)W16 & 15) == 0 && !(Mk && !Mk16))
            return launch_site(dbg, Mk16 ? PNR_DBG_K_HGEMM_DMA_M16 : PNR_DBG_K_HGEMM_DMA, EPI_LDS, &e, [&] {
                with_flags([&](auto m16) {
                    hipLaunchKernelGGL((k_hgemm_dma<RELU_X, m16()>), tiles, blk, 0, s, X16, ldx, W16, K, b, R, ldr, Mp, ldm, Y, ldy, Y16, ldy,
                                       (int)M, N, K);
                }, Mk16 != nullptr);
            });
        return launch_site(dbg, X16 ? (Mk16 ? PNR_DBG_K_MGEMM_BF16_A16_M16 : PNR_DBG_K_MGEMM_BF16_A16)
                                    : (Mk16 ? PNR_DBG_K_MGEMM_BF16_M16 : PNR_DBG_K_MGEMM_BF16_G16), EPI_REG, &e, [&] {
            with_flags([&](auto a16, auto m16) {
                hipLaunchKernelGGL((k_mgemm_bf16<true, !TRANS_W, RELU_X, false, false, a16(), false, m16()>), tiles, blk, 0, s, Xp, ldx,
                                   (const void*)W, ldw, b, R, ldr, Mp, ldm, Y, ldy, (float*)nullptr, (int)M, N, K, 0, (size_t)0, (size_t)0,
                                   Y16, ldy);
            }, X16 != nullptr, Mk16 != nullptr);
        });
    }
    const int half = mode;
    const EpiArgs e{b, R, ldr, Mk, ldm, false, Y, ldy, nullptr, 0, N};
    // fp32 dX with W^T as an (N, K) row-major copy: both operands row-contiguous in the reduction index -> LDS-DMA k-loop
    if (TRANS_W && w.nk32 && !half && N >= 32 && K >= 64 && K % 16 == 0 && al16(X, ldx) && ((uintptr_t)w.nk32 & 15) == 0)
        return launch_site(dbg, PNR_DBG_K_SGEMM_DMA_WT, EPI_LDS, &e, [&] {
            hipLaunchKernelGGL((k_sgemm_dma<RELU_X>), tiles, blk, 0, s, X, ldx, w.nk32, K, b, R, ldr, Mk, ldm, Y, ldy, (int)M, N, K);
        });
    if (half && N >= 32 && K >= 32 && K % 32 == 0 && N % 4 == 0 && al16(X, ldx) && al16(W, ldw))
        return launch_site(dbg, half == 3 ? PNR_DBG_K_MGEMM_BF16X3 : PNR_DBG_K_MGEMM_BF16, EPI_REG, &e, [&] {
            if (half == 3)
                hipLaunchKernelGGL((k_mgemm_bf16x3<true, !TRANS_W, RELU_X, false, false>), tiles, blk, 0, s, X, ldx, W, ldw, b, R, ldr, Mk,
                                   ldm, Y, ldy, (float*)nullptr, (int)M, N, K, 0);
            else
                hipLaunchKernelGGL((k_mgemm_bf16<true, !TRANS_W, RELU_X, false, false>), tiles, blk, 0, s, X, ldx, W, ldw, b, R, ldr, Mk,
                                   ldm, Y, ldy, (float*)nullptr, (int)M, N, K, 0);
        });
    // fp32 products, activations x weights as stored: both operands row-contiguous in the reduction index -> LDS-DMA k-loop
    if (!TRANS_W && !half && N >= 32 && K >= 64 && K % 16 == 0 && al16(X, ldx) && al16(W, ldw))
        return launch_site(dbg, PNR_DBG_K_SGEMM_DMA, EPI_LDS, &e, [&] {
            hipLaunchKernelGGL((k_sgemm_dma<RELU_X>), tiles, blk, 0, s, X, ldx, W, ldw, b, R, ldr, Mk, ldm, Y, ldy, (int)M, N, K);
        });
    if (N >= 32 && K >= 16)         // MFMA tile kernel; the skinny heads (N = 4, K = 4) stay on the FMA kernel
        return launch_site(dbg, PNR_DBG_K_MGEMM_F32, EPI_REG, &e, [&] {
            hipLaunchKernelGGL((k_mgemm_f32<true, !TRANS_W, RELU_X, false, false>), tiles, blk, 0, s, X, ldx, W, ldw, b, R, ldr, Mk, ldm, Y,
                               ldy, (float*)nullptr, (int)M, N, K, 0, vec_flags(X, ldx, W, ldw));
        });
    // the output head (lin_out, d_out = 4)
    if (!TRANS_W && N == 4 && !R && !Mk && (K == 256 || K == 512) && al16(X, ldx) && al16(W, ldw) && al16(Y, ldy))
        return launch_site(dbg, K == 512 ? PNR_DBG_K_LINEAR_HEAD_512 : PNR_DBG_K_LINEAR_HEAD_256, EPI_NOT_TILE, nullptr, [&] {
            int64_t blocks = (M + 15) / 16;
            if (blocks > 2048) blocks = 2048;
            if (K == 512)
                hipLaunchKernelGGL((k_linear_head<RELU_X, 2>), dim3((unsigned)blocks), blk, 0, s, X, ldx, W, ldw, b, Y, ldy, (int)M);
            else
                hipLaunchKernelGGL((k_linear_head<RELU_X, 1>), dim3((unsigned)blocks), blk, 0, s, X, ldx, W, ldw, b, Y, ldy, (int)M);
        });
    return launch_site(dbg, PNR_DBG_K_GEMM_F32, EPI_NOT_TILE, nullptr, [&] {
        hipLaunchKernelGGL((k_gemm_f32<RELU_X, TRANS_W>), dim3((unsigned)((M + 63) / 64), (N + 63) / 64), blk, 0, s, X, ldx, W, ldw, b, R,
                           ldr, Mk, ldm, Y, ldy, (int)M, N, K);
    });
}

// dX of the output head: Y (P, N) = mask(Mk > 0) (.) (X (P, 4) . W (4, N)) — four products per element, i.e. a stream: one
// thread per four columns with its W columns in registers, a half-wave per 512-byte row segment (k_gemm_f32's 64 x 64 tile
// stored it as 4-byte pieces at 16-byte stride: 55 us for 200 MB).  The sum is k_gemm_f32's chain (k ascending from 0), so the
// values are that kernel's; Y16 (optional) = the bf16 copy the 16-bit-tape backward otherwise makes with k_to_bf16.
// Needs N / 4 a power of two <= 256 (the grid stride keeps a thread on its columns) and 16-byte-aligned rows.
static __global__ void __launch_bounds__(256) k_head_dx(const float4* __restrict__ X, const float* __restrict__ W, int ldw,
                                                        const float* __restrict__ Mk, int ldm, float* __restrict__ Y, int ldy,
                                                        uint16_t* __restrict__ Y16, int ldy16, int64_t P, int N) {
    const int per_row = N >> 2;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(i0 & (per_row - 1)), n = 4 * c;
    const int64_t row_stride = ((int64_t)gridDim.x * 256) / per_row;
    const float4 w0 = *(const float4*)(W + n), w1 = *(const float4*)(W + (size_t)ldw + n), w2 = *(const float4*)(W + 2 * (size_t)ldw + n),
                 w3 = *(const float4*)(W + 3 * (size_t)ldw + n);
    const float wk[4][4] = {{w0.x, w0.y, w0.z, w0.w}, {w1.x, w1.y, w1.z, w1.w}, {w2.x, w2.y, w2.z, w2.w}, {w3.x, w3.y, w3.z, w3.w}};
    for (int64_t m = i0 / per_row; m < P; m += row_stride) {
        const float4 d = X[m];
        const float4 mk = Mk ? *(const float4*)(Mk + (size_t)m * ldm + n) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float xs[4] = {d.x, d.y, d.z, d.w}, mv[4] = {mk.x, mk.y, mk.z, mk.w};
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) a = fmaf(xs[k], wk[k][j], a);
            v[j] = (mv[j] > 0.f) ? a : 0.f;
        }
        *(float4*)(Y + (size_t)m * ldy + n) = make_float4(v[0], v[1], v[2], v[3]);
        if (Y16) *(uint2*)(Y16 + (size_t)m * ldy16 + n) = make_uint2(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]));
    }
}
static bool head_dx_ok(const float* X, const float* W, int ldw, const float* Mk, int ldm, const float* Y, int ldy, int N, int K) {
    const int per_row = N >> 2;
    return K == 4 && N % 4 == 0 && per_row >= 1 && per_row <= 256 && (per_row & (per_row - 1)) == 0 && al16(X, 4) && al16(W, ldw) &&
           al16(Y, ldy) && (!Mk || al16(Mk, ldm));
}
static int32_t head_dx(const float* X, const float* W, int ldw, const float* Mk, int ldm, float* Y, int ldy, uint16_t* Y16, int64_t P,
                       int N, hipStream_t s, DbgSite* dbg = nullptr) {
    if (P == 0) return PNR_OK;
    const int per_row = N >> 2;
    int64_t blocks = (P * per_row + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (dbg) dbg->id = PNR_DBG_K_HEAD_DX;
    hipLaunchKernelGGL(k_head_dx, dim3((unsigned)blocks), dim3(256), 0, s, (const float4*)X, W, ldw, Mk, ldm, Y, ldy, Y16, ldy, P, N);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

// db (N) += column sums of dY alone: a frozen weight with a trainable bias (needs_input_grad False / True)
__global__ void k_col_sums(const float* __restrict__ dY, int ldy, float* __restrict__ db, int M, int N, int rows, size_t zs_b) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    db += blockIdx.y * zs_b;
    const int m0 = blockIdx.y * rows, m1 = min(M, m0 + rows);
    float acc = 0.f;
    for (int m = m0; m < m1; ++m) acc += dY[(size_t)m * ldy + n];
    db[n] = acc;
}

// the same over the gradient stream's bf16 copy (what the GEMM path's row sums of the staged tile add up)
__global__ void k_col_sums16(const uint16_t* __restrict__ dY, int ldy, float* __restrict__ db, int M, int N, int rows, size_t zs_b) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    db += blockIdx.y * zs_b;
    const int m0 = blockIdx.y * rows, m1 = min(M, m0 + rows);
    float acc = 0.f;
    for (int m = m0; m < m1; ++m) acc += __builtin_bit_cast(float, (uint32_t)dY[(size_t)m * ldy + n] << 16);
    db[n] = acc;
}

// y (+)= act(x) W^T + b on the fp32 MFMA tile kernel, for the fp32 inference path (point_f32.hip): the same GEMM the taped
// training forward uses.  W (N, K) row-major as nn.Linear stores it; accum adds to what Y holds.
int32_t linear_f32_mfma(const float* X, int ldx, const float* W, int ldw, const float* b, bool relu_in, bool accum, float* Y,
                        int ldy, int64_t M, int N, int K, hipStream_t s) {
    const Mat x = f32_mat(X, ldx), y = f32_mat(Y, ldy), res = f32_mat(accum ? Y : nullptr, ldy);
    const Weight w = plain_weight(W, ldw);
    if (relu_in) return gemm<true, false>(x, w, b, res, NO_MAT, y, M, N, K, 0, s);
    return gemm<false, false>(x, w, b, res, NO_MAT, y, M, N, K, 0, s);
}

// Ordered sum of the per-split partials: out[i] += part[0][i] + part[1][i] + ... (fixed order -> run-to-run identical bits)
__global__ void k_reduce_parts(const float* __restrict__ part, int nz, size_t zs, float* __restrict__ out, int ld, int rows, int cols) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i % cols);
    float acc = 0.f;
    for (int z = 0; z < nz; ++z) acc += part[(size_t)z * zs + i];
    out[(size_t)r * ld + c] += acc;
}

// the weight's and the bias's partials in one launch (same fixed order per element)
__global__ void k_reduce_parts2(const float* __restrict__ pw, const float* __restrict__ pb, int nz, size_t zs_w, size_t zs_b,
                                float* __restrict__ dW, int ldw, int K, float* __restrict__ db) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)zs_w) {
        float acc = 0.f;
        for (int z = 0; z < nz; ++z) acc += pw[(size_t)z * zs_w + i];
        const int r = (int)(i / K), c = (int)(i % K);
        dW[(size_t)r * ldw + c] += acc;
    } else if (i < (int64_t)(zs_w + zs_b)) {
        const int64_t j = i - (int64_t)zs_w;
        float acc = 0.f;
        for (int z = 0; z < nz; ++z) acc += pb[(size_t)z * zs_b + j];
        db[j] += acc;
    }
}

// dW (N, K) += dY^T act(X),  db (N) += column sums of dY;  rows split over the grid, one partial slice per split,
// ordered reduction at the end.  Either output may be NULL (a frozen parameter): the GEMM kernels need dW, so a bias-only
// request takes k_col_sums.  x.b16 (the 16-bit tape's form of the operand, instead of x.f32) goes to the bf16 MFMA kernels only;
// dy.b16 (the gradient stream's bf16 copy, read instead of dy.f32) needs x.b16.  half: as gemm's mode (0, 1, 3).
template <bool RELU_X>
static int32_t grad_w(const Mat& dy, const Mat& x, float* dW, int ldw, float* db, int64_t M, int N, int K, int half, const DetWs& ws,
                      hipStream_t s, DbgSite* dbg = nullptr) {
    if ((!dW && !db) || M == 0) return PNR_OK;
    const float* dY = dy.f32; const uint16_t* dY16 = dy.b16; const float* X = x.f32; const uint16_t* X16 = x.b16;
    const int ldy = dy.ld, ldx = x.ld;
    const size_t zs_w = (size_t)N * K, zs_b = (size_t)N;
    // rows per split: the kernel's natural slice, enlarged until the splits fit the scratch
    auto splits_for = [&](int rows, int* rows_out) -> int {
        int64_t nz = (M + rows - 1) / rows;
        int64_t cap = (int64_t)(ws.floats / (zs_w + zs_b));
        if (cap > DET_MAX_SPLITS) cap = DET_MAX_SPLITS;
        if (cap < 1) cap = 1;
        if (nz > cap) {
            int64_t r = (M + cap - 1) / cap;
            r = (r + rows - 1) / rows * rows;          // keep the kernel's row granularity
            rows = (int)r;
            nz = (M + rows - 1) / rows;
        }
        *rows_out = rows;
        return (int)nz;
    };
    float* pw = ws.part;                 // (nz, N, K)
    int rows = 0, nz = 0;
    const dim3 blk(256);
    // the tail every candidate shares: its launch into the partial slices, then their ordered sums
    auto run = [&](int id, auto&& launch) -> int32_t {
        PNR_TRY(launch_site(dbg, id, EPI_NOT_TILE, nullptr, launch));
        float* pb = pw + (size_t)nz * zs_w;
        if (dbg) { dbg->splits = nz; dbg->rows = rows; dbg->reduce = dW && db ? 2 : 1; }
        if (dW && db)            // one launch for the weight and its bias (60 -> 40 launches per training step)
            hipLaunchKernelGGL(k_reduce_parts2, dim3((unsigned)((zs_w + zs_b + 255) / 256)), blk, 0, s, pw, pb, nz, zs_w, zs_b, dW, ldw, K, db);
        else if (dW)
            hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)((zs_w + 255) / 256)), blk, 0, s, pw, nz, zs_w, dW, ldw, N, K);
        else
            hipLaunchKernelGGL(k_reduce_parts, dim3((unsigned)((zs_b + 255) / 256)), blk, 0, s, pb, nz, zs_b, db, N, 1, N);
        PNR_LAUNCH_CHECK();
        return PNR_OK;
    };
    if (!ws.part || ws.floats < zs_w + zs_b) return PNR_E_WORKSPACE;
    if (!dW) {
        nz = splits_for(2048, &rows);
        float* pb = pw + (size_t)nz * zs_w;
        const dim3 grid((N + 255) / 256, (unsigned)nz);
        return run(dY16 ? PNR_DBG_K_COL_SUMS16 : PNR_DBG_K_COL_SUMS, [&] {
            if (dY16) hipLaunchKernelGGL(k_col_sums16, grid, blk, 0, s, dY16, ldy, pb, (int)M, N, rows, zs_b);
            else hipLaunchKernelGGL(k_col_sums, grid, blk, 0, s, dY, ldy, pb, (int)M, N, rows, zs_b);
        });
    }
    const bool mfma_shape = N >= 32 && K >= 32;
    const bool use_half = half && mfma_shape && N % 4 == 0 && K % 4 == 0 && (dY16 ? ldy % 8 == 0 : al16(dY, ldy)) && (X16 ? true : al16(X, ldx));
    if (X16 && !(use_half && half == 1)) return PNR_E_UNSUPPORTED;      // the 16-bit tape is read by the bf16 MFMA kernel only
    if (dY16 && !X16) return PNR_E_UNSUPPORTED;
    const bool head = !mfma_shape && N == 4 && ldy == 4 && ((uintptr_t)dY & 15) == 0;
    // lin_in: few input columns against d_hidden output rows — its own kernel, fp32 operands in every mode
    if (!RELU_X && !X16 && !dY16 && K <= 96 && N >= 64 && dY && X) {
        // partial slices are small (N K floats): many of them, so that the chip is filled
        int64_t want = (M + 191) / 192;
        int64_t cap = (int64_t)(ws.floats / (zs_w + zs_b));
        if (cap > 1024) cap = 1024;
        if (want > cap) want = cap;
        if (want < 1) want = 1;
        rows = (int)((M + want - 1) / want);
        nz = (int)((M + rows - 1) / rows);
        float* pbs = db ? pw + (size_t)nz * zs_w : nullptr;
        const dim3 grid((N + 255) / 256, (unsigned)nz);
        return run(K <= 48 ? PNR_DBG_K_GRAD_W_SKINNY48 : PNR_DBG_K_GRAD_W_SKINNY96, [&] {
            if (K <= 48) hipLaunchKernelGGL((k_grad_w_skinny<48>), grid, blk, 0, s, dY, ldy, X, ldx, pw, K, pbs, (int)M, N, K, rows, zs_w, zs_b);
            else hipLaunchKernelGGL((k_grad_w_skinny<96>), grid, blk, 0, s, dY, ldy, X, ldx, pw, K, pbs, (int)M, N, K, rows, zs_w, zs_b);
        });
    }
    // the LDS-DMA kernel runs two workgroups per CU: 32 slices x 16 tiles of a 512 x 512 weight = one full round of the chip's
    // 512 slots (48 slices of 1024 rows were 1.5 rounds), and a third less partial-sum traffic for k_reduce_parts
    const bool dma_kt = use_half && X16 && dY16 && M % 64 == 0 && N % 128 == 0 && K % 128 == 0 && ldy % 8 == 0 && ldx % 8 == 0 &&
                        (((uintptr_t)dY16 | (uintptr_t)X16) & 15) == 0;
    static constexpr int DW_SLICES = 32;
    int rows_dma = (int)(((M + DW_SLICES - 1) / DW_SLICES + 63) / 64 * 64);
    if (rows_dma < 256) rows_dma = 256;
    // (the same slices for every bf16-product weight gradient, whichever kernel and tape format: the two tape formats stay
    // bit-identical)
    const bool dma32 = !use_half && !half && mfma_shape && M % 32 == 0 && N % 128 == 0 && K % 128 == 0 && al16(dY, ldy) && al16(X, ldx);
    const bool slices32 = (use_half && half == 1 && M % 32 == 0) || dma32;        // (fp32 products on k_sgemm_dma_kt: the same grid)
    nz = splits_for(slices32 ? rows_dma : mfma_shape ? 1024 : head ? 256 : 2048, &rows);
    float* pbk = db ? pw + (size_t)nz * zs_w : nullptr;
    if (head)
        return run(PNR_DBG_K_GRAD_W_HEAD, [&] {
            hipLaunchKernelGGL((k_grad_w_head<RELU_X>), dim3((K + 127) / 128, (unsigned)nz), blk, 0, s, (const float4*)dY, X, ldx, pw, K, pbk,
                               (int)M, K, rows, zs_w, zs_b);
        });
    if (!mfma_shape)
        return run(PNR_DBG_K_GRAD_W_F32, [&] {
            hipLaunchKernelGGL((k_grad_w_f32<RELU_X>), dim3((N + 63) / 64, (K + 63) / 64, (unsigned)nz), blk, 0, s, dY, ldy, X, ldx, pw, K, pbk,
                               (int)M, N, K, rows, zs_w, zs_b);
        });
    // dW = A B with A(n, r = m) = dY[m][n] and B(r = m, k) = act(X[m][k]): both stored reduction-major
    const dim3 grid = mgemm_grid(nz, ((N + 127) / 128) * ((K + 127) / 128));
    if (use_half && half == 3)
        return run(PNR_DBG_K_MGEMM_BF16X3_DW, [&] {
            hipLaunchKernelGGL((k_mgemm_bf16x3<false, false, false, RELU_X, true>), grid, blk, 0, s, dY, ldy, X, ldx, (const float*)nullptr,
                               (const float*)nullptr, 0, (const float*)nullptr, 0, pw, K, pbk, N, K, (int)M, rows, zs_w, zs_b);
        });
    if (dma_kt && rows % 64 == 0)
        return run(PNR_DBG_K_HGEMM_DMA_KT, [&] {
            hipLaunchKernelGGL((k_hgemm_dma_kt<RELU_X>), grid, blk, 0, s, dY16, ldy, X16, ldx, pw, K, pbk, N, K, (int)M, rows, zs_w, zs_b);
        });
    if (use_half && X16)        // the tape's operand as bf16, the gradient stream in whichever form it came
        return run(dY16 ? PNR_DBG_K_MGEMM_BF16_DW_A16B16 : PNR_DBG_K_MGEMM_BF16_DW_B16, [&] {
            with_flags([&](auto a16) {
                hipLaunchKernelGGL((k_mgemm_bf16<false, false, false, RELU_X, true, a16(), true, false>), grid, blk, 0, s,
                                   dY16 ? (const void*)dY16 : (const void*)dY, ldy, (const void*)X16, ldx, (const float*)nullptr,
                                   (const float*)nullptr, 0, (const void*)nullptr, 0, pw, K, pbk, N, K, (int)M, rows, zs_w, zs_b);
            }, dY16 != nullptr);
        });
    if (use_half)
        return run(PNR_DBG_K_MGEMM_BF16_DW, [&] {
            hipLaunchKernelGGL((k_mgemm_bf16<false, false, false, RELU_X, true>), grid, blk, 0, s, dY, ldy, X, ldx, (const float*)nullptr,
                               (const float*)nullptr, 0, (const float*)nullptr, 0, pw, K, pbk, N, K, (int)M, rows, zs_w, zs_b);
        });
    if (dma32 && rows % 16 == 0)
        return run(PNR_DBG_K_SGEMM_DMA_KT, [&] {
            hipLaunchKernelGGL((k_sgemm_dma_kt<RELU_X>), grid, blk, 0, s, dY, ldy, X, ldx, pw, K, pbk, N, K, (int)M, rows, zs_w, zs_b);
        });
    return run(PNR_DBG_K_MGEMM_F32_DW, [&] {
        hipLaunchKernelGGL((k_mgemm_f32<false, false, false, RELU_X, true>), grid, blk, 0, s, dY, ldy, X, ldx, (const float*)nullptr,
                           (const float*)nullptr, 0, (const float*)nullptr, 0, pw, K, pbk, N, K, (int)M, rows, vec_flags(dY, ldy, X, ldx),
                           zs_w, zs_b);
    });
}

// bf16 copy of a fp32 tensor (the residual stream behind a view reduction, or lin_in's output when no lin_z follows)
static __global__ void k_to_bf16(const float* __restrict__ x, int64_t n, uint16_t* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (uint16_t)(pk_bf16(x[i], 0.f) & 0xffffu);
}

static int32_t to_bf16(const float* x, int64_t n, uint16_t* y, hipStream_t s) {
    hipLaunchKernelGGL(k_to_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, y);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

// The step's weight copies in one launch: a table entry per hidden weight (2 b: fc_0, 2 b + 1: fc_1) and, for the first n_z
// blocks, per lin_z; copies(tb, entry, i, is_lin_z) sets the entry's destination(s) for hidden weight i / lin_z of block i.
template <class Table, class Copies>
static int32_t weight_copies(void (*kernel)(Table), const pnr_mlp* mlp, int n_z, Copies copies, hipStream_t s) {
    const int H = mlp->d_hidden, L = mlp->d_latent;
    Table tb{};
    for (int i = 0; i < 2 * mlp->n_blocks; ++i) {
        tb.w[i] = (i & 1) ? mlp->fc1_w[i >> 1] : mlp->fc0_w[i >> 1];
        tb.rows[i] = tb.cols[i] = H;
        copies(tb, i, i, false);
    }
    tb.n = 2 * mlp->n_blocks;
    for (int b = 0; b < n_z; ++b, ++tb.n) {
        tb.w[tb.n] = mlp->lin_z_w[b]; tb.rows[tb.n] = H; tb.cols[tb.n] = L;
        copies(tb, tb.n, b, true);
    }
    const int64_t biggest = (int64_t)H * (H > L ? H : L);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((biggest + 255) / 256), (unsigned)tb.n), dim3(256), 0, s, tb);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

// The taped forward.  fp32 tape: every block input and fc_0 output is a tape slot.  16-bit tape (train_precision = "bf16", see
// Tape): same GEMMs, same operands after rounding; the fp32 residual stream ping-pongs between two buffers, and every GEMM
// that produces a block input or an fc_0 output also (or only) writes the bf16 copy the tape keeps.
int32_t point_train_fwd(const pnr_params* prm, const pnr_mlp* mlp, const pnr_views* vw, PointSrc src, int64_t P,
                        int64_t pts_per_obj, float* out, void* tape, uint64_t tape_bytes, hipStream_t s) {
    if (tape_bytes < train_tape_bytes_p(prm, mlp, vw, P)) return PNR_E_WORKSPACE;
    const int NS = vw->n_views, L = mlp->d_latent, Din = mlp->d_in, H = mlp->d_hidden, E = feature_stride(mlp);
    const int nb = mlp->n_blocks, cl = mlp->combine_layer, nz = n_lin_z(mlp);
    if (NS > 1 && cl >= nb) return PNR_E_UNSUPPORTED;
    const Tape t = carve_tape(mlp, vw, P, tape, tape_is_16bit(prm, mlp));
    const int64_t MV = (int64_t)NS * P;
    if (MV > 0x7fffffff) return PNR_E_SHAPE;
    // GEMM products: 0 = fp32 MFMA, 1 = bf16 MFMA, 3 = bf16x3 split (fp32-class); the products on the 16-bit tape's operands
    // take its bf16 forms
    const int half = prm->precision == PNR_BF16 ? 1 : prm->precision == PNR_BF16X3 ? 3 : 0;
    const int tape_mode = t.h16 ? (int)PNR_DBG_MODE_TAPE16 : half;
    PNR_TRY(features_launch(*vw, src, 0, (int)P, pts_per_obj, L, Din, prm->use_code_viewdirs, prm->num_freqs, prm->freq_factor, t.zx, E, s,
                            (t.lat_cl.p[0] && P >= 4096) ? latent_cl_build(*vw, t.lat_cl, s) : LatCL{}));
    PNR_LAUNCH_CHECK();
    if (t.Wb[0]) {      // bf16 copies of the hidden weights (as stored + transposed) for the LDS-DMA GEMMs of forward and backward
        PNR_TRY(weight_copies<W16Table>(k_w_to_bf16, mlp, t.z16 ? nz : 0, [&](W16Table& tb, int e, int i, bool lin_z) {
            tb.wb[e] = lin_z ? t.Wz[i] : t.Wb[i];
            tb.wt[e] = lin_z ? t.Wzt[i] : t.Wt[i];
        }, s));
        if (t.z16 && nz > 0) {
            const int64_t n2 = MV * (L / 2);
            hipLaunchKernelGGL(k_cols_to_bf16, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, t.zx, MV, E, L, t.z16);
            PNR_LAUNCH_CHECK();
        }
    } else if (t.Wt32[0] && !half) {      // W^T of the hidden weights (and lin_z) for the backward's dX products on k_sgemm_dma
        PNR_TRY(weight_copies<W32Table>(k_w_transpose_f32, mlp, t.Wzt32[0] ? nz : 0, [&](W32Table& tb, int e, int i, bool lin_z) {
            tb.wt[e] = lin_z ? t.Wzt32[i] : t.Wt32[i];
        }, s));
    }
    auto combine = [&](float* dst) -> int32_t {
        int64_t per_view = P * H;
        hipLaunchKernelGGL(k_combine_f32, dim3((unsigned)((per_view + 255) / 256)), dim3(256), 0, s, t.xpre, NS,
                           per_view, mlp->combine_type, dst);
        PNR_LAUNCH_CHECK();
        return PNR_OK;
    };
    // does lin_z rewrite the input of block b?  (otherwise what lin_in / fc_1 / the view reduction left is final already)
    auto lin_z_at = [&](int b) { return L > 0 && b < nz; };
    // lin_in (Din is not a multiple of 32: the fp32 kernels, fp32 operand zx)
    const bool comb0 = NS > 1 && cl == 0;
    const Mat code = f32_mat(t.zx + L, E), x0 = f32_mat(comb0 ? t.xpre : t.stream(0), H);
    PNR_TRY((gemm<false, false>(code, plain_weight(mlp->lin_in_w, Din), mlp->lin_in_b, NO_MAT, NO_MAT, x0, MV, H, Din, half, s)));
    if (comb0) PNR_TRY(combine(t.stream(0)));
    if (t.h16 && !lin_z_at(0)) PNR_TRY(to_bf16(t.stream(0), t.rows[0] * H, t.A16[0], s));
    for (int b = 0; b < nb; ++b) {
        const int64_t M = t.rows[b];
        const Mat x = f32_mat(t.stream(b), H);
        if (lin_z_at(b)) {
            // x += lin_z[b](z), in place; 16-bit tape: + its bf16 copy = the block input, from the same launch when z suits a
            // bf16-product kernel (as bf16 copies of both operands: the LDS-DMA kernel, same rounding, same sums)
            const bool z_mfma = t.h16 && (t.z16 || (L % 32 == 0 && al16(t.zx, E)));
            const Mat xin{x.f32, z_mfma ? t.A16[b] : nullptr, H};
            PNR_TRY((gemm<false, false>(t.z(), t.lin_z_w(mlp->lin_z_w[b], b), mlp->lin_z_b[b], x, NO_MAT, xin, M, H, L,
                                        z_mfma ? tape_mode : half, s)));
            if (t.h16 && !z_mfma) PNR_TRY(to_bf16(x.f32, M * H, t.A16[b], s));
        }
        // h = fc_0(relu(x)); 16-bit tape: operand and result live on the tape only
        PNR_TRY((gemm<true, false>(t.block_in(b), t.hidden_w(mlp->fc0_w[b], 2 * b), mlp->fc0_b[b], NO_MAT, NO_MAT, t.hidden(b), M, H, H,
                                   tape_mode, s)));
        // x' = x + fc_1(relu(h)): fp32 for the chain, into the view reduction's input where that follows; 16-bit tape: its bf16
        // copy = the next block's input (unless lin_z / the reduction rewrite it)
        const bool comb = NS > 1 && b + 1 == cl;
        const Mat x_next{comb ? t.xpre : t.stream(b + 1), !comb && !lin_z_at(b + 1) ? t.A16[b + 1] : nullptr, H};
        PNR_TRY((gemm<true, false>(t.hidden(b), t.hidden_w(mlp->fc1_w[b], 2 * b + 1), mlp->fc1_b[b], x, NO_MAT, x_next, M, H, H, tape_mode, s)));
        if (comb) {
            PNR_TRY(combine(t.stream(b + 1)));
            if (t.h16 && !lin_z_at(b + 1)) PNR_TRY(to_bf16(t.stream(b + 1), t.rows[b + 1] * H, t.A16[b + 1], s));
        }
    }
    const Mat x_out = f32_mat(t.stream(nb), H), o4 = f32_mat(t.o4, 4);
    PNR_TRY((gemm<true, false>(x_out, plain_weight(mlp->lin_out_w, H), mlp->lin_out_b, NO_MAT, NO_MAT, o4, P, 4, H, half, s)));
    hipLaunchKernelGGL(k_out_act, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, t.o4, P, out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

int32_t point_bwd(const pnr_params* prm, const pnr_mlp* mlp, const pnr_views* vw, PointSrc src, int64_t P,
                  int64_t pts_per_obj, const float* out, const float* d_out, void* tape, uint64_t tape_bytes,
                  const pnr_mlp_grads* gr, float* const* d_latent, float* d_xyz, float* d_z, void* workspace,
                  uint64_t ws_bytes, hipStream_t s, const CamGradOut* cam /* camera gradients (cam_grad.hip), or null */) {
    if (tape_bytes < train_tape_bytes_p(prm, mlp, vw, P)) return PNR_E_WORKSPACE;
    Bump bump(round_up_256(workspace));
    const TrainBwdWs w = carve_train_bwd(bump, mlp, vw, P);
    if (ws_bytes < bump.off) return PNR_E_WORKSPACE;
    const int NS = vw->n_views, L = mlp->d_latent, Din = mlp->d_in, H = mlp->d_hidden, E = feature_stride(mlp);
    const int nb = mlp->n_blocks, cl = mlp->combine_layer, nz = n_lin_z(mlp);
    if (NS > 1 && cl >= nb) return PNR_E_UNSUPPORTED;
    const Tape t = carve_tape(mlp, vw, P, tape, tape_is_16bit(prm, mlp));
    const int64_t MV = (int64_t)NS * P;
    const int half = prm->precision == PNR_BF16 ? 1 : prm->precision == PNR_BF16X3 ? 3 : 0;
    const int tape_mode = t.h16 ? (int)PNR_DBG_MODE_TAPE16 : half;
    float *dx = w.dx, *dx2 = w.dx2, *dh = w.dh, *dzx = w.dzx, *do4 = w.do4, *lat_part = w.lat_part;
    const DetWs dws = w.dws;
    uint8_t* lat_q = w.lat_q;
    const bool want_p = d_xyz || d_z;
    const bool want_code = want_p || cam;      // the gradient at the code columns of dzx
    bool want_lat = false;
    LatGrad lg{};
    for (int l = 0; l < vw->n_levels; ++l) { lg.p[l] = d_latent ? d_latent[l] : nullptr; want_lat |= lg.p[l] != nullptr; }
    const bool want_dz = L > 0 && (want_lat || want_code);

    hipLaunchKernelGGL(k_out_act_bwd, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const float4*)out,
                       (const float4*)d_out, P, (float4*)do4);
    PNR_LAUNCH_CHECK();
    const Mat g4 = f32_mat(do4, 4), x_out = f32_mat(t.stream(nb), H);
    PNR_TRY((grad_w<true>(g4, x_out, gr->lin_out_w, H, gr->lin_out_b, P, 4, H, half, dws, s)));
    bool dz_started = false;
    // 16-bit tape: the fp32 dh buffer holds the two bf16 streams instead (dh, and the copy of dx)
    uint16_t* dh16 = (uint16_t*)dh;
    uint16_t* dx16 = dh16 + (size_t)MV * H;
    // the gradient stream: fp32 for the residual sums, with its bf16 copy (b16) while one is valid
    Mat g = f32_mat(dx, H);
    if (head_dx_ok(do4, mlp->lin_out_w, H, x_out.f32, H, dx, H, H, 4)) {
        // the head's dX as a stream, with the gradient stream's first bf16 copy from the same pass (the head is behind the
        // view reduction: P rows, the row count of the last block)
        const bool copy16 = t.h16 && nb > 0 && t.rows[nb - 1] == P;
        PNR_TRY(head_dx(do4, mlp->lin_out_w, H, x_out.f32, H, dx, H, copy16 ? dx16 : nullptr, P, H, s));
        if (copy16) g.b16 = dx16;
    } else {
        PNR_TRY((gemm<false, true>(g4, plain_weight(mlp->lin_out_w, H), nullptr, NO_MAT, x_out, g, P, H, 4, half, s)));
    }
    for (int b = nb - 1; b >= 0; --b) {
        const int64_t M = t.rows[b];
        // The four products of a block.  16-bit tape: every operand is read as the bf16 the fp32-tape form would round it to —
        // the tape operands / masks, and the gradient stream: dh exists as bf16 only (its two readers stage it as bf16 anyway), dx
        // keeps its fp32 form for the residual sum and gets a bf16 copy from the epilogue that produces it.  Same roundings
        // of the same values: gradients stay bit-identical to the fp32-tape form; 0.76x the bytes of a block's backward.
        if (t.h16 && !g.b16) { PNR_TRY(to_bf16(dx, M * H, dx16, s)); g.b16 = dx16; }
        const Mat x_in = t.block_in(b), hid = t.hidden(b);
        const Mat gh = t.h16 ? Mat{nullptr, dh16, H} : f32_mat(dh, H);
        PNR_TRY((grad_w<true>(g, hid, gr->fc1_w[b], H, gr->fc1_b[b], M, H, H, half, dws, s)));
        PNR_TRY((gemm<false, true>(g, t.hidden_w_dx(mlp->fc1_w[b], 2 * b + 1), nullptr, NO_MAT, hid, gh, M, H, H, tape_mode, s)));
        PNR_TRY((grad_w<true>(gh, x_in, gr->fc0_w[b], H, gr->fc0_b[b], M, H, H, half, dws, s)));
        PNR_TRY((gemm<false, true>(gh, t.hidden_w_dx(mlp->fc0_w[b], 2 * b), nullptr, f32_only(g), x_in, g, M, H, H, tape_mode, s)));
        if (L > 0 && b < nz) {
            // lin_z: with the bf16 copy of the latent columns both products read the bf16 forms, else fp32 operands only
            const Mat z = t.z(), gz = z.b16 ? g : f32_only(g);
            PNR_TRY((grad_w<false>(gz, z, gr->lin_z_w[b], L, gr->lin_z_b[b], M, H, L, half, dws, s)));
            if (want_dz) {
                const Mat dz = f32_mat(dzx, E), dz_so_far = f32_mat(dz_started ? dzx : nullptr, E);
                PNR_TRY((gemm<false, true>(gz, t.lin_z_w_dx(mlp->lin_z_w[b], b), nullptr, dz_so_far, NO_MAT, dz, M, L, H,
                                           z.b16 ? tape_mode : half, s)));
                dz_started = true;
            }
        }
        if (NS > 1 && b == cl) {
            int64_t per_view = P * H;
            hipLaunchKernelGGL(k_combine_bwd, dim3((unsigned)((per_view + 255) / 256)), dim3(256), 0, s, dx, t.xpre, NS,
                               per_view, mlp->combine_type, dx2);
            PNR_LAUNCH_CHECK();
            float* tmp = dx; dx = dx2; dx2 = tmp;
            g = f32_mat(dx, H);         // (P rows became NS P rows of another buffer: no bf16 copy of those)
        }
    }
    const Mat gx = f32_only(g), code = f32_mat(t.zx + L, E);
    PNR_TRY((grad_w<false>(gx, code, gr->lin_in_w, Din, gr->lin_in_b, MV, H, Din, half, dws, s)));
    if ((want_code || want_lat) && L > 0 && !dz_started) PNR_HIP_CHECK(hipMemsetAsync(dzx, 0, (size_t)MV * E * 4, s));
    if (want_code)
        PNR_TRY((gemm<false, true>(gx, plain_weight(mlp->lin_in_w, Din), nullptr, NO_MAT, NO_MAT, f32_mat(dzx + L, E), MV, Din, H,
                                   half, s)));
    // small single-level map: latent gradient on per-block partial maps + an ordered reduction (bit-reproducible)
    if (want_lat && L > 0 && latent_grad_in_lds(vw)) {
        const int T = vw->lat_h[0] * vw->lat_w[0], C = vw->lat_c[0], views = vw->n_objs * vw->n_views;
        const size_t lds = latent_grad_lds_bytes(vw);
        const int nbx = (int)((pts_per_obj + LATG_PPB - 1) / LATG_PPB);
        if (lds > 48 * 1024) {          // only above the default limit, and once per device (the attribute sticks to the function)
            static PerDevice raised;
            int* done = raised.slot();
            if (!done || !*done) {
                PNR_HIP_CHECK(hipFuncSetAttribute((const void*)k_latent_grad_lds, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  (int)lds_per_block_limit()));
                if (done) *done = 1;
            }
        }
        hipLaunchKernelGGL(k_latent_grad_lds, dim3(nbx, views), dim3(256), lds, s, *vw, src, P, pts_per_obj, L, dzx, E, lat_part);
        PNR_LAUNCH_CHECK();
        const int64_t tot = (int64_t)views * T * C;
        hipLaunchKernelGGL(k_latent_reduce, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, lat_part, nbx, views, C, T, lg.p[0]);
        PNR_LAUNCH_CHECK();
        lg.p[0] = nullptr;
        want_lat = false;
    }
    const bool fixed_point = want_lat && L > 0 && latent_q_bytes(vw) > 0;
    if (fixed_point) {
        // larger / multi-level maps: the taps are summed with 64-bit fixed-point integer atomics (order-independent, so
        // bit-reproducible) into workspace copies of the maps, scaled by the gradient's own magnitude, and added to d_latent
        // by k_latq_finalize.  (Round 3 summed fp32 atomics in arrival order.)
        unsigned* max_bits = (unsigned*)lat_q;
        int* scale_bits = (int*)(lat_q + 64);
        long long* q = (long long*)(lat_q + 256);
        PNR_HIP_CHECK(hipMemsetAsync(lat_q, 0, latent_q_bytes(vw), s));
        hipLaunchKernelGGL(k_abs_max_cols, dim3(1024), dim3(256), 0, s, dzx, MV, E, L, max_bits);
        PNR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_latq_scale, dim3(1), dim3(1), 0, s, max_bits, (long long)(4 * MV), scale_bits);
        PNR_LAUNCH_CHECK();
        lg.scale_bits = scale_bits;
        for (int l = 0; l < vw->n_levels; ++l) {
            const uint64_t n = (uint64_t)vw->n_objs * vw->n_views * vw->lat_c[l] * vw->lat_h[l] * vw->lat_w[l];
            lg.q[l] = lg.p[l] ? q : nullptr;
            q += n;
        }
    }
    if (want_p || (want_lat && L > 0)) {
        hipLaunchKernelGGL(k_features_bwd, dim3((unsigned)((P + 3) / 4)), dim3(256), 0, s, *vw, src, P, pts_per_obj, L, Din,
                           prm->use_code_viewdirs, prm->num_freqs, prm->freq_factor, dzx, E, lg, d_xyz, d_z);
        PNR_LAUNCH_CHECK();
    }
    if (cam) PNR_TRY(cam_grad_launch(prm, vw, src, P, pts_per_obj, L, dzx, E, *cam, s));
    if (fixed_point) {
        for (int l = 0; l < vw->n_levels; ++l) {
            if (!lg.q[l]) continue;
            const int64_t n = (int64_t)vw->n_objs * vw->n_views * vw->lat_c[l] * vw->lat_h[l] * vw->lat_w[l];
            hipLaunchKernelGGL(k_latq_finalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lg.q[l], n, lg.scale_bits,
                               (const unsigned*)lat_q + 1, lg.p[l]);
            PNR_LAUNCH_CHECK();
        }
    }
    return PNR_OK;
}

}  // namespace pnr

using namespace pnr;

// Host-side view of the tile GEMMs' grid (tests: every tile exactly once, the tiles that share an operand on one XCD).
extern "C" int64_t pnr_debug_gemm_grid(int32_t M, int32_t N, int32_t Rn, int32_t rows_per_split, int32_t split) {
    const int64_t gx = (M + 127) / 128, gy = (N + 127) / 128;
    if (split) return mgemm_grid(((int64_t)Rn + rows_per_split - 1) / rows_per_split, (int)(gx * gy)).x;
    return mgemm_grid(gx, (int)gy).x;
}
extern "C" int32_t pnr_debug_gemm_tile(int32_t block, int32_t M, int32_t N, int32_t Rn, int32_t rows_per_split, int32_t split,
                                       int32_t* out3) {
    int bx, by, bz;
    const bool ok = split ? mgemm_tile_of<true>(block, M, N, Rn, rows_per_split, bx, by, bz)
                          : mgemm_tile_of<false>(block, M, N, Rn, rows_per_split, bx, by, bz);
    out3[0] = bx; out3[1] = by; out3[2] = bz;
    return ok ? 1 : 0;
}

// One product through the production dispatchers (include/pnr.h: pnr_debug_linear_args); tests/test_gpu_train_gemm.py.
template <bool RELU>
static int32_t debug_linear(pnr_debug_linear_args* a, hipStream_t s, DbgSite* d) {
    const int64_t M = a->m;
    const int N = a->n, K = a->k;
    const Mat x{(const float*)a->x, (const uint16_t*)a->x16, a->ldx}, res{a->r, nullptr, a->ldr};
    const Mat mask{(const float*)a->mk, (const uint16_t*)a->mk16, a->ldm}, y{(const float*)a->y, (const uint16_t*)a->y16, a->ldy};
    // w16: the (n, k) copy in the form the mode reads (bf16 for PNR_DBG_MODE_TAPE16, fp32 W^T for a mode-0 dX)
    const Weight w{(const float*)a->w, a->ldw, (const uint16_t*)a->w16, (const float*)a->w16};
    const bool mode_ok = a->mode == 0 || a->mode == 1 || a->mode == 3 || a->mode == PNR_DBG_MODE_TAPE16;
    switch (a->op) {
    case PNR_DBG_OP_FWD:
        return mode_ok ? gemm<RELU, false>(x, w, a->b, res, mask, y, M, N, K, a->mode, s, d) : PNR_E_UNSUPPORTED;
    case PNR_DBG_OP_DX:
        return mode_ok ? gemm<RELU, true>(x, w, a->b, res, mask, y, M, N, K, a->mode, s, d) : PNR_E_UNSUPPORTED;
    case PNR_DBG_OP_HEAD_DX:
        if (!head_dx_ok(x.f32, w.f32, a->ldw, mask.f32, a->ldm, y.f32, a->ldy, N, K)) return PNR_E_UNSUPPORTED;
        return head_dx(x.f32, w.f32, a->ldw, mask.f32, a->ldm, (float*)a->y, a->ldy, (uint16_t*)a->y16, M, N, s, d);
    case PNR_DBG_OP_DW:
        return grad_w<RELU>(Mat{a->g, (const uint16_t*)a->g16, a->ldg}, x, (float*)a->y, a->ldy, a->db, M, N, K, a->mode,
                            DetWs{a->ws, a->ws_floats}, s, d);
    }
    return PNR_E_UNSUPPORTED;
}

// Which latent-gradient route pnr_point_mlp_bwd takes for these maps (include/pnr.h); tests/test_gpu_train_fp64.py.
extern "C" int32_t pnr_debug_latent_grad_route(const pnr_views* vw, int64_t n_points) {
    if (!vw || vw->n_levels < 1 || n_points <= 0) return PNR_DBG_LATG_NONE;
    if (latent_grad_in_lds(vw)) return PNR_DBG_LATG_LDS;
    return latent_q_bytes(vw) > 0 ? PNR_DBG_LATG_FIXED_POINT : PNR_DBG_LATG_NONE;
}

extern "C" int32_t pnr_debug_linear(pnr_debug_linear_args* a, void* stream) {
    if (!a) return PNR_E_NULL;
    a->kernel = PNR_DBG_K_NONE;
    a->epilogue = PNR_DBG_EPI_NONE;
    a->splits = a->rows_per_split = a->reduce = 0;
    if (a->m < 0 || a->m > 0x7fffffff || a->n < 0 || a->k < 0) return PNR_E_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t M = a->m;
    switch (a->op) {
    case PNR_DBG_OP_TO_BF16:
        if (!a->x || !a->y16) return PNR_E_NULL;
        if (M > 0) hipLaunchKernelGGL(k_to_bf16, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, (const float*)a->x, M, (uint16_t*)a->y16);
        PNR_LAUNCH_CHECK();
        return PNR_OK;
    case PNR_DBG_OP_COLS_TO_BF16: {
        if (!a->x || !a->y16) return PNR_E_NULL;
        if (a->k % 2 || a->ldx % 2 || a->k > a->ldx || ((uintptr_t)a->x & 7) || ((uintptr_t)a->y16 & 3)) return PNR_E_ALIGN;
        const int64_t n2 = M * (a->k / 2);
        if (n2 > 0) hipLaunchKernelGGL(k_cols_to_bf16, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, (const float*)a->x, M, a->ldx, a->k,
                                       (uint16_t*)a->y16);
        PNR_LAUNCH_CHECK();
        return PNR_OK;
    }
    case PNR_DBG_OP_W_TO_BF16: {
        if (!a->x || !a->y16) return PNR_E_NULL;
        W16Table tb{};
        tb.w[0] = (const float*)a->x; tb.wb[0] = (uint16_t*)a->y16; tb.wt[0] = (uint16_t*)a->y16t;
        tb.rows[0] = (int)M; tb.cols[0] = a->k; tb.n = 1;
        if (M * a->k > 0) hipLaunchKernelGGL(k_w_to_bf16, dim3((unsigned)((M * a->k + 255) / 256), 1u), dim3(256), 0, s, tb);
        PNR_LAUNCH_CHECK();
        return PNR_OK;
    }
    }
    DbgSite d{};
    const int32_t rc = a->relu ? debug_linear<true>(a, s, &d) : debug_linear<false>(a, s, &d);
    a->kernel = d.id;
    a->epilogue = d.epi;
    a->splits = d.splits;
    a->rows_per_split = d.rows;
    a->reduce = d.reduce;
    return rc;
}

extern "C" int32_t pnr_composite_bwd(const float* rays, const float* z, const float* rgbsigma, int64_t n_rays,
                                     int32_t K, int32_t white_bkgd, const float* d_weights, const float* d_rgb,
                                     const float* d_depth, float* d_rgbsigma, float* d_z, void* stream) {
    if (!rays || !z || !rgbsigma || !d_rgbsigma) return PNR_E_NULL;
    if (n_rays < 0 || K <= 0) return PNR_E_SHAPE;
    if ((((uintptr_t)rgbsigma | (uintptr_t)d_rgbsigma) & 15) != 0) return PNR_E_ALIGN;
    if (n_rays == 0) return PNR_OK;
    size_t lds = (size_t)4 * 3 * K * sizeof(float);
    if (lds > 64 * 1024) return PNR_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_composite_bwd, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), lds, (hipStream_t)stream, rays, z,
                       (const float4*)rgbsigma, n_rays, K, white_bkgd, d_weights, d_rgb, d_depth, (float4*)d_rgbsigma, d_z);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_sample_fine_bwd(const float* rays, const float* depth, int64_t n_rays, int32_t n_coarse,
                                       int32_t n_fine, int32_t n_fine_depth, float depth_std, const float* g,
                                       uint64_t seed, int64_t ray_index_base, const float* z_sorted,
                                       const float* d_z_sorted, float* d_depth, void* stream) {
    if (!rays || !depth || !z_sorted || !d_z_sorted || !d_depth) return PNR_E_NULL;
    if (n_rays < 0 || n_coarse <= 0 || n_fine < 0 || n_fine_depth < 0 || n_fine_depth > n_fine) return PNR_E_SHAPE;
    if (n_rays == 0) return PNR_OK;
    hipLaunchKernelGGL(k_sample_fine_bwd, dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rays,
                       depth, n_rays, n_coarse + n_fine, n_fine_depth, depth_std, g, seed, ray_index_base, z_sorted,
                       d_z_sorted, d_depth);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
