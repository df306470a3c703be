// The data layer's two entry points: a training batch gathered from 8-BIT images, and the selected source views of such a
// batch converted to the network's input where they lie.  The kernels, their checks and their launches are data_u8.h's, shared
// with the colour-jitter pair (jitter.hip); here they run without a chain.
#include "data_u8.h"

using namespace pnr;

extern "C" int32_t pnr_train_batch_u8(const uint8_t* images_u8, const float* poses, const float* focal, const float* c, int32_t SB,
                                      int32_t NV, int32_t W, int32_t H, float z_near, float z_far, const int64_t* pix_inds,
                                      int64_t B, float* rays_out, float* rgb_gt_out, int32_t C, int32_t balanced, void* stream) {
    return launch_train_batch_u8<false>(images_u8, poses, focal, c, SB, NV, W, H, z_near, z_far, pix_inds, B, rays_out, rgb_gt_out, C,
                                        balanced, nullptr, stream);
}

extern "C" int32_t pnr_views_to_tensor_u8(const uint8_t* images_u8, const int64_t* view_ord, int32_t SB, int32_t NV, int32_t NS,
                                          int32_t W, int32_t H, int32_t C, int32_t balanced, float* out, void* stream) {
    return launch_views_to_tensor_u8<false>(images_u8, view_ord, SB, NV, NS, W, H, C, balanced, nullptr, out, stream);
}
