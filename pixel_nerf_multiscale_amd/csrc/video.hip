// The two ends of the video drivers (reference eval/gen_video.py, eval/eval_real.py) where they lie on the device: a stack of
// F rendered frames to bytes in ONE launch (gen_video.py:236, eval_real.py:151: (frames.cpu().numpy() * 255).astype(uint8)),
// the source-view strip (gen_video.py:239-241), and an 8-bit image to the network's input tensor (util.py:68-79).
// include/pnr.h fixes the arithmetic.  Bandwidth-trivial (40 frames of 128 x 128 are 7.5 MB read, 1.9 MB written); the point
// is that 3 bytes per pixel leave the card instead of 12 and that nothing waits on the host.
#include "frame_common.h"

namespace pnr {

constexpr int VF_THREADS = FRAME_THREADS;          // 256 = 4 waves
constexpr int VF_DWORDS = 3;                       // output dwords per body thread: 12 bytes = 4 pixels

// The byte of a product p = x * 255.0f: truncation toward zero where numpy's cast is defined (-1 < p < 256; a small negative
// product and -0.0 give 0), else saturation (0 for p <= -1 and for NaN, 255 for p >= 256) and one count.
__device__ __forceinline__ uint32_t sat_u8(float p, int& n_out) {
    if (p > -1.0f && p < 256.0f) return (uint32_t)(int)p;
    ++n_out;
    return p >= 256.0f ? 255u : 0u;
}

struct VideoArgs {
    const float* rgb; int stride;                  // floats per pixel
    uint8_t* out;
    int64_t n_bytes;                               // 3 F H W
    int head;                                      // bytes in front of the first whole dword of `out`
    int n_edge;                                    // head + tail bytes, at most 6
    int64_t body_dwords;                           // whole dwords from out + head on
    int64_t n_body;                                // threads that own VF_DWORDS of them each
    unsigned long long* count;                     // NULL = not counted
};

// Flat over the byte stream out[j], j = 3 pixel + channel: thread g < n_body owns the dwords [3 g, 3 g + 3) behind the head
// (the last one may own fewer), the n_edge threads after them one head or tail byte each.  VEC: the stream is dense and both
// ends are aligned, so dword d is exactly the float4 d of `rgb`.  Otherwise the thread walks its bytes' (pixel, channel) pairs
// with scalar loads — a stride-4 record, an `out` that starts inside a dword, an unaligned base.  The counts of a workgroup are
// folded in LDS and leave as ONE integer atomic, and only when they are not zero: exact, and the same in any order.
template <bool VEC> __global__ void __launch_bounds__(VF_THREADS) k_video_frames(VideoArgs a) {
    __shared__ int red[VF_THREADS];
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * VF_THREADS + tid;
    int n_out = 0;
    if (g < a.n_body) {
        const int64_t d0 = g * VF_DWORDS;
        const int nd = a.body_dwords - d0 < VF_DWORDS ? (int)(a.body_dwords - d0) : VF_DWORDS;
        uint32_t* dst = (uint32_t*)(a.out + a.head) + d0;
        if (VEC) {
            const float4* src = (const float4*)a.rgb + d0;
#pragma unroll
            for (int q = 0; q < VF_DWORDS; ++q) {
                if (q < nd) {
                    const float4 v = src[q];
                    dst[q] = sat_u8(__fmul_rn(v.x, 255.0f), n_out) | sat_u8(__fmul_rn(v.y, 255.0f), n_out) << 8 |
                             sat_u8(__fmul_rn(v.z, 255.0f), n_out) << 16 | sat_u8(__fmul_rn(v.w, 255.0f), n_out) << 24;
                }
            }
        } else {
            const int64_t j = a.head + 4 * d0;
            const int64_t pix = j / 3;
            int c = (int)(j - 3 * pix);
            const float* p = a.rgb + pix * a.stride;
            for (int q = 0; q < nd; ++q) {
                uint32_t w = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    w |= sat_u8(__fmul_rn(p[c], 255.0f), n_out) << (8 * b);
                    if (++c == 3) { c = 0; p += a.stride; }
                }
                dst[q] = w;
            }
        }
    } else if (g < a.n_body + a.n_edge) {
        const int e = (int)(g - a.n_body);
        const int64_t j = e < a.head ? e : a.head + 4 * a.body_dwords + (e - a.head);
        const int64_t pix = j / 3;
        a.out[j] = (uint8_t)sat_u8(__fmul_rn(a.rgb[pix * a.stride + (j - 3 * pix)], 255.0f), n_out);
    }
    if (!a.count) return;                                                  // uniform over the launch
    red[tid] = n_out;
    block_fold<VF_THREADS>(tid, [&](int i, int j) { red[i] += red[j]; });
    if (tid == 0 && red[0] != 0) atomicAdd(a.count, (unsigned long long)red[0]);
}

// np.hstack over the views of ((x * scale + lo) * 255).astype(uint8): a thread per output pixel
__global__ void __launch_bounds__(VF_THREADS) k_view_strip(const float* __restrict__ images, int NS, int W, int H, float scale,
                                                           float lo, uint8_t* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * VF_THREADS + threadIdx.x, row = (int64_t)NS * W;
    if (idx >= row * H) return;
    const int y = (int)(idx / row), r = (int)(idx - y * row), v = r / W, x = r - v * W;
    const int64_t HW = (int64_t)H * W;
    int unused = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = images[((int64_t)v * 3 + c) * HW + (int64_t)y * W + x];
        out[idx * 3 + c] = (uint8_t)sat_u8(__fmul_rn(__fadd_rn(__fmul_rn(t, scale), lo), 255.0f), unused);
    }
}

// torchvision's ToTensor (balanced: followed by Normalize(0.5, 0.5)) for an (H, W, 3) byte image: a thread per pixel
__global__ void __launch_bounds__(VF_THREADS) k_image_to_tensor(const uint8_t* __restrict__ img, int64_t HW, int balanced,
                                                                float* __restrict__ out) {
    const int64_t pix = (int64_t)blockIdx.x * VF_THREADS + threadIdx.x;
    if (pix >= HW) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * HW + pix] = u8_to_tensor(img[pix * 3 + c], balanced);
}

static inline unsigned blocks_for(int64_t threads) { return (unsigned)((threads + VF_THREADS - 1) / VF_THREADS); }

}  // namespace pnr

using namespace pnr;

extern "C" int32_t pnr_video_frames(const float* rgb, int32_t rgb_stride, int32_t F, int32_t W, int32_t H, uint8_t* out_u8,
                                    int64_t* n_out_of_range, void* stream) {
    if (!rgb || !out_u8) return PNR_E_NULL;
    if (F < 1 || !frame_pixels_ok(W, H) || (int64_t)F * W * H >= ((int64_t)1 << 31)) return PNR_E_SHAPE;      // W H < 2^31: no overflow
    if (rgb_stride == 0) rgb_stride = 3;
    if (rgb_stride < 3) return PNR_E_SHAPE;
    if (((uintptr_t)rgb & 3) != 0 || ((uintptr_t)n_out_of_range & 7) != 0) return PNR_E_ALIGN;
    VideoArgs a;
    a.rgb = rgb; a.stride = rgb_stride; a.out = out_u8;
    a.n_bytes = 3 * (int64_t)F * W * H;
    const int lead = (int)((4 - ((uintptr_t)out_u8 & 3)) & 3);
    a.head = lead < a.n_bytes ? lead : (int)a.n_bytes;
    a.body_dwords = (a.n_bytes - a.head) / 4;
    a.n_edge = (int)(a.n_bytes - 4 * a.body_dwords);
    a.n_body = (a.body_dwords + VF_DWORDS - 1) / VF_DWORDS;
    a.count = (unsigned long long*)n_out_of_range;
    hipStream_t s = (hipStream_t)stream;
    if (n_out_of_range) PNR_HIP_CHECK(hipMemsetAsync(n_out_of_range, 0, sizeof(int64_t), s));
    const bool vec = rgb_stride == 3 && ((uintptr_t)rgb & 15) == 0 && a.head == 0;
    const unsigned blocks = blocks_for(a.n_body + a.n_edge);              // at most 2^29 + 6 threads
    if (vec) hipLaunchKernelGGL(k_video_frames<true>, dim3(blocks), dim3(VF_THREADS), 0, s, a);
    else hipLaunchKernelGGL(k_video_frames<false>, dim3(blocks), dim3(VF_THREADS), 0, s, a);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_view_strip(const float* images, int32_t NS, int32_t W, int32_t H, float scale, float lo, uint8_t* out_u8,
                                  void* stream) {
    if (!images || !out_u8) return PNR_E_NULL;
    if (NS < 1 || !frame_pixels_ok(W, H) || (int64_t)NS * W * H >= ((int64_t)1 << 31)) return PNR_E_SHAPE;
    if (((uintptr_t)images & 3) != 0) return PNR_E_ALIGN;
    hipLaunchKernelGGL(k_view_strip, dim3(blocks_for((int64_t)NS * W * H)), dim3(VF_THREADS), 0, (hipStream_t)stream, images, NS, W,
                       H, scale, lo, out_u8);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}

extern "C" int32_t pnr_image_to_tensor(const uint8_t* img_u8, int32_t W, int32_t H, int32_t balanced, float* out, void* stream) {
    if (!img_u8 || !out) return PNR_E_NULL;
    if (!frame_pixels_ok(W, H) || (balanced != 0 && balanced != 1)) return PNR_E_SHAPE;
    if (((uintptr_t)out & 3) != 0) return PNR_E_ALIGN;
    hipLaunchKernelGGL(k_image_to_tensor, dim3(blocks_for((int64_t)W * H)), dim3(VF_THREADS), 0, (hipStream_t)stream, img_u8,
                       (int64_t)W * H, balanced, out);
    PNR_LAUNCH_CHECK();
    return PNR_OK;
}
