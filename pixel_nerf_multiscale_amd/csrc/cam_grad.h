// Camera gradients of the training backward (cam_grad.hip; include/pnr.h: pnr_point_mlp_bwd_cam).
#pragma once
#include "pnr_common.h"

namespace pnr {

// What pnr_point_mlp_bwd_cam asks for on top of pnr_point_mlp_bwd; every output may be NULL.
struct CamGradOut {
    float* d_dirs;      // (P, 3), explicit points
    float* d_rays;      // (n_rays, 8), rays mode
    float* d_cam;       // (n_objs * n_views, 16): [dR 9 | dt 3 | dfx dfy dcx dcy]
    void* ws;           // cam_grad_workspace_bytes
    uint64_t ws_bytes;
};

static constexpr int CAMG_CHUNK = 1024;      // points of one (object, view) that one block of k_cam_partial folds

uint64_t cam_grad_workspace_bytes(const pnr_views* vw, int64_t P, bool want_point, bool want_cam);
// dzx (n_views * P rows of stride ldz, view-major): the gradient at the assembled [latent | code] rows, as point_bwd leaves it
int32_t cam_grad_launch(const pnr_params* prm, const pnr_views* vw, PointSrc src, int64_t P, int64_t pts_per_obj, int L,
                        const float* dzx, int ldz, const CamGradOut& out, hipStream_t s);

}  // namespace pnr
