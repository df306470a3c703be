/*
 * pnr.h — C ABI of libpnr_hip.so, the MI355X (gfx950) native pixelNeRF render hot path.
 *
 * The reference (Zxhh123/pixel-nerf-multiscale) is pure Python and has NO native interface; this header
 * is the boundary a maintainer would bind with ctypes.  Each entry point names
 * the reference code it replaces (paths relative to the reference's src/).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors' data_ptr()), fp32,
 *    contiguous, row-major, unless stated otherwise; the library never allocates or frees device
 *    memory and keeps no mutable global state.
 *  - `stream` is a hipStream_t (0 = default stream).  Every call is asynchronous on it and
 *    never synchronises the host.
 *  - return: 0 ok; <0 PNR_E_* (bad argument / unsupported configuration); >0 a hipError_t.
 */
#ifndef PNR_H
#define PNR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PNR_VERSION 102          /* 0.1.2: pnr_views.uv_scale_{x,y} (opt-in upstream texel mapping); 101: output strides, per-object ray index stride.
                                  * Added since, backward compatible (no bump): the training front end, pnr_train_batch / pnr_rgb_loss / pnr_rgb_loss_bwd;
                                  * the evaluation back end, pnr_eval_frame / pnr_eval_frame_workspace_bytes; mesh extraction,
                                  * pnr_grid_points / pnr_mc_workspace_bytes / pnr_mc_count / pnr_mc_emit; the training back end, pnr_optim_chunk_elems /
                                  * pnr_optim_plan / pnr_optim_workspace_bytes / pnr_adam_step; the visualisation panel and the colour map, pnr_cmap_workspace_bytes /
                                  * pnr_cmap / pnr_vis_panel_workspace_bytes / pnr_vis_panel; the video drivers' ends, pnr_video_frames /
                                  * pnr_view_strip / pnr_image_to_tensor; the approximate evaluation's batched metrics, pnr_eval_frames /
                                  * pnr_eval_frames_workspace_bytes; the metrics of saved 8-bit images, pnr_eval_frames_u8 /
                                  * pnr_eval_frames_u8_workspace_bytes; the camera gradients, pnr_point_mlp_bwd_cam /
                                  * pnr_train_bwd_cam_workspace_bytes; the data layer's 8-bit batches, pnr_train_batch_u8 /
                                  * pnr_views_to_tensor_u8; the training draws, pnr_train_draw; the fused launch's work split as a
                                  * host diagnostic, pnr_debug_point_split; the colour-jitter augmentation of 8-bit batches,
                                  * pnr_color_jitter_workspace_bytes / pnr_color_jitter_plan / pnr_train_batch_u8_jitter /
                                  * pnr_views_to_tensor_u8_jitter; the data-parallel training step — an object base in the keyed
                                  * draws and a divisor folded into the optimiser, pnr_train_draw_at / pnr_color_jitter_plan_at /
                                  * pnr_adam_step_div; area resampling of images, pnr_resize_area_u8 / pnr_resize_area_f32; empty-space
                                  * culling, pnr_occ_build / pnr_ray_bounds_workspace_bytes / pnr_ray_bounds / pnr_frame_from_hits;
                                  * mask-weighted training draws, pnr_mask_table_build / pnr_train_draw_masked /
                                  * pnr_train_draw_masked_at; the opacity losses, pnr_mask_gather / pnr_alpha_loss / pnr_alpha_loss_bwd;
                                  * procedural datasets, pnr_synth_render */
#define PNR_MAX_LEVELS 5         /* encoder levels of a multi-scale latent (encoder.py:62-73) */
#define PNR_MAX_BLOCKS 8         /* ResnetFC blocks (resnetfc.py:147) */

enum {
    PNR_OK = 0,
    PNR_E_NULL = -1,             /* required pointer is NULL */
    PNR_E_SHAPE = -2,            /* inconsistent / out-of-range sizes */
    PNR_E_UNSUPPORTED = -3,      /* configuration the kernels do not implement */
    PNR_E_WORKSPACE = -4,        /* workspace too small */
    PNR_E_ALIGN = -5,            /* pointer not 16-byte aligned where required */
    PNR_E_PACKED = -6            /* packed weights / latents missing or of the wrong kind */
};

enum { PNR_F32 = 0, PNR_BF16 = 1, PNR_F16 = 2,          /* arithmetic type of the fc layers */
       PNR_BF16X3 = 3 };                                 /* training entry points only: bf16 MFMA with every operand split
                                                          * hi + lo, 3 products per term — fp32-class results */
enum { PNR_COMBINE_AVERAGE = 0, PNR_COMBINE_MAX = 1 }; /* util.combine_interleaved (util.py:466-476) */

/* ResnetFC parameters (resnetfc.py:128-158), PyTorch nn.Linear layout: weight (out,in), y = x W^T + b.
 * State-dict keys: lin_in, lin_z.{b}, blocks.{b}.fc_0 / fc_1, lin_out.  use_spade / softplus (beta>0)
 * are not supported (no shipped config uses them). */
typedef struct pnr_mlp {
    int32_t d_in;                /* 42 = 39 pos-enc + 3 viewdirs, or 78 with use_code_viewdirs */
    int32_t d_latent;            /* 256 single-scale, 512 multi-scale; sum of level channels */
    int32_t d_hidden;            /* 512 in every shipped config; MFMA path requires 512 */
    int32_t d_out;               /* 4 */
    int32_t n_blocks;            /* 5 */
    int32_t combine_layer;       /* 3: views are reduced before this block; lin_z exists for b < min(combine_layer, n_blocks) */
    int32_t combine_type;        /* PNR_COMBINE_* */
    int32_t packed_objs;         /* projected streams only: number of objects `packed` holds a stream for (0 = 1) */
    const float* lin_in_w;  const float* lin_in_b;
    const float* lin_z_w[PNR_MAX_BLOCKS];  const float* lin_z_b[PNR_MAX_BLOCKS];
    const float* fc0_w[PNR_MAX_BLOCKS];    const float* fc0_b[PNR_MAX_BLOCKS];
    const float* fc1_w[PNR_MAX_BLOCKS];    const float* fc1_b[PNR_MAX_BLOCKS];
    const float* lin_out_w; const float* lin_out_b;
    /* produced once by pnr_pack_mlp(); required when precision != PNR_F32 */
    const void* packed;
    uint64_t packed_bytes;
    int32_t packed_dtype;        /* PNR_BF16 / PNR_F16 */
    int32_t packed_texels;       /* 0: plain stream (pnr_pack_mlp).  T > 0: stream from pnr_pack_mlp_projected; T = Hl*Wl of
                                  * the last latent level (lin_z pre-multiplied with that level's maps) */
} pnr_mlp;

/* What PixelNeRFNet.encode() leaves on the module (models.py.backup2:108-150) + the encoder's latent
 * map(s) (encoder.py:106-136).  View index = obj * n_views + v (repeat_interleave order, util.py:58-65). */
typedef struct pnr_views {
    int32_t n_objs;              /* SB */
    int32_t n_views;             /* NS per object */
    const float* w2c;            /* (SB*NS, 3, 4) [R^T | -R^T t] */
    const float* focal;          /* (n_focal, 2): fx, fy with fy ALREADY negated (backup2:139) */
    const float* c;              /* (n_c, 2) principal point */
    int32_t n_focal;             /* 1 (broadcast) or SB*NS */
    int32_t n_c;                 /* 1 (broadcast) or SB*NS */
    int32_t n_levels;            /* 1 = single-scale */
    int32_t reserved0;
    const float* latent[PNR_MAX_LEVELS];   /* (SB*NS, C_i, H_i, W_i) NCHW fp32, reference layout */
    int32_t lat_c[PNR_MAX_LEVELS];
    int32_t lat_h[PNR_MAX_LEVELS];
    int32_t lat_w[PNR_MAX_LEVELS];
    /* required when precision != PNR_F32: per level (SB*NS, H_i, W_i, C_i) channels-last, 16-bit (packed_dtype),
     * 16-byte aligned.  Either carved from the blob pnr_pack_latents() writes (level i at the offset it reports), or
     * the encoder's own output when it already runs channels-last in half precision (zero copy).
     * With these present the fp32 NCHW pointers above may be NULL. */
    const void* latent_packed[PNR_MAX_LEVELS];
    int32_t packed_dtype;
    int32_t reserved1;
    /* Texel coordinate of an image point on level i = uv * uv_scale_{x,y}[i].  0 (the default of a zeroed struct) = 1.0 =
     * the reference fork's mapping: encoder.py:152-164 normalises uv by the LATENT size and ignores image_size, so the
     * texel coordinate equals the image-pixel coordinate — the parity target.  Opt-in: upstream pixelNeRF's
     * mapping (uv * latent_scaling / image_size, align_corners) = W_i / W_image, H_i / H_image per level — what a
     * checkpoint trained with upstream semantics expects (SpatialEncoder.uv_scale = "image"; parity unpinned: the
     * reference holds no fixture for it).  The gradient of the lookup w.r.t. uv carries the same factor. */
    float uv_scale_x[PNR_MAX_LEVELS];
    float uv_scale_y[PNR_MAX_LEVELS];
} pnr_views;

/* NeRFRenderer attributes (render/nerf.py:62-96) + the PixelNeRFNet switches the kernels need. */
typedef struct pnr_params {
    int32_t n_coarse;            /* Kc */
    int32_t n_fine;              /* Kf (0 = coarse pass only) */
    int32_t n_fine_depth;        /* Kfd <= Kf */
    int32_t white_bkgd;
    int32_t lindisp;
    int32_t use_code_viewdirs;   /* positional-encode [xyz, viewdirs] together (backup2:207-209) */
    int32_t num_freqs;           /* 6 (code.py:11) */
    int32_t precision;           /* PNR_F32 | PNR_BF16 | PNR_F16 */
    float depth_std;
    float freq_factor;           /* 1.5 (conf/default.conf:18) */
    int32_t train_tape_fp32;     /* training with precision = PNR_BF16: 0 = 16-bit tape (block inputs and fc_0 outputs kept as
                                  * bf16 — the values the bf16-product GEMMs stage anyway: gradients are bit-identical to the
                                  * fp32 tape's), 1 = fp32 tape */
    int32_t park_fp32;           /* fused kernel, several source views: 0 = the per-view residual streams wait for the view
                                  * reduction (util.combine_interleaved, util.py:466-476) in the kernel's 16-bit format — half
                                  * the bytes, the rounding every layer input takes anyway; 1 = as fp32, the reference's
                                  * reduction of fp32 activations (symmetric in the view order), ~3 % slower on 3-view shapes */
    int32_t reserved[4];
} pnr_params;

/* Explicit random draws, reference order (render/nerf.py:111,135,141,158).  A NULL member (or a NULL
 * struct) selects the in-kernel counter-based generator keyed by (seed, global ray index). */
typedef struct pnr_noise {
    const float* noise_c;        /* (N, Kc)      U[0,1) */
    const float* u;              /* (N, Kf-Kfd)  U[0,1) */
    const float* r;              /* (N, Kf-Kfd)  U[0,1) */
    const float* g;              /* (N, Kfd)     N(0,1) */
    /* Key of the in-kernel generator for a call that holds a RANGE of every object's rays (one rank's shard of an
     * (SB, B, 8) batch cut along B, as nn.DataParallel(dim=1) cuts it, render/nerf.py:367-371): ray i of object o counts as
     * global ray  ray_index_base + o * ray_index_obj_stride + i.  0 = objects follow each other (stride = rays_per_obj),
     * which is what an unsharded call means; a shard passes base = first ray of its range, stride = B. */
    int64_t ray_index_obj_stride;
} pnr_noise;

/* Outputs of NeRFRenderer.forward (render/nerf.py:278-303); any member may be NULL. */
typedef struct pnr_outputs {
    float* coarse_rgb;           /* (N,3) */
    float* coarse_depth;         /* (N)   */
    float* coarse_weights;       /* (N,Kc) */
    float* fine_rgb;             /* (N,3) */
    float* fine_depth;           /* (N)   */
    float* fine_weights;         /* (N,Kc+Kf) */
    float* z_coarse;             /* (N,Kc)    sampled depths (debug / tests) */
    float* z_fine;               /* (N,Kc+Kf) sorted */
    /* optional hipEvent_t handles recorded on `stream` immediately before / after the COARSE pass's point-network
     * launch (the dominant kernel), so a caller can time that kernel inside a whole-path call; NULL = off */
    void* ev_point_begin;
    void* ev_point_end;
    /* Row strides in floats of the rgb / depth / weights outputs; 0 = dense (3, 1, Kc, Kc+Kf).  With strides the members
     * above may point INTO one packed per-ray record — e.g. rgb at +0, depth at +3 of a (N, 4) buffer that is this rank's
     * slice of an all_gather buffer — so a sharded frame is written where the collective reads it (no copies). */
    int32_t rgb_stride;
    int32_t depth_stride;
    int32_t coarse_weights_stride;
    int32_t fine_weights_stride;
} pnr_outputs;

int32_t pnr_version(void);
const char* pnr_error_string(int32_t code);

/* ---- one-time packing ------------------------------------------------------------------------ */
/* Repack an MLP's fp32 weights into the fragment stream the MFMA kernel consumes in order
 * (bf16 or fp16; biases folded in).  `out` must hold pnr_packed_mlp_bytes() bytes, 16-B aligned. */
uint64_t pnr_packed_mlp_bytes(const pnr_mlp* mlp);
int32_t pnr_pack_mlp(const pnr_mlp* mlp, int32_t dtype, void* out, uint64_t out_bytes, void* stream);
/* Projected stream: for 1..16 objects (1..8 source views each) whose LAST latent level has 256 channels on
 * 4 <= Hl*Wl <= 256 texels (single-scale SRN / NMR maps; the coarsest level of the multi-scale encoder — the levels
 * before it, whole 256-channel groups, are still gathered) bilinear lookup and lin_z are both linear, so
 * lin_z_b(index(uv)) = (W_z,b . Lat) . w(uv) with w the point's 4 tap weights spread over the Hl*Wl texels.  The
 * stream then carries W_z,b . Lat (512 x Hl*Wl; the block's bias added to every column, the tap weights summing to 1) in
 * place of W_z,b (512 x d_latent) and the kernel needs no latent
 * gather; with several views the per-view part of the stream is laid out once per view, each copy with its own
 * view's product; with several objects the blob holds one such stream per object and the kernels assign their workgroups
 * per object.  Re-pack whenever the weights OR the latent maps change; pnr_packed_mlp_projected_bytes() returns 0 when
 * the shapes do not qualify.  Set pnr_mlp.packed_texels = Hl*Wl and pnr_mlp.packed_objs = views->n_objs on the struct that
 * carries this stream; it is refused (PNR_E_PACKED) for any other object count or map size. */
uint64_t pnr_packed_mlp_projected_bytes(const pnr_mlp* mlp, const pnr_views* views);
int32_t pnr_pack_mlp_projected(const pnr_mlp* mlp, const pnr_views* views, int32_t dtype, void* out,
                               uint64_t out_bytes, void* stream);
/* Channels-last low-precision copy of the latent maps for the MFMA kernel's gather. */
uint64_t pnr_packed_latent_bytes(const pnr_views* views);
/* level_offsets (host array of PNR_MAX_LEVELS, may be NULL) receives the byte offset of every level inside `out` */
int32_t pnr_pack_latents(const pnr_views* views, int32_t dtype, void* out, uint64_t out_bytes,
                         uint64_t* level_offsets, void* stream);

/* ---- stage entry points (also what the tests call) ------------------------------------------- */
/* NeRFRenderer.sample_coarse (render/nerf.py:98-118).  rays (N,8) -> z (N,Kc). */
int32_t pnr_sample_coarse(const float* rays, int64_t n_rays, int32_t n_coarse, int32_t lindisp,
                          const float* noise_c, uint64_t seed, int64_t ray_index_base,
                          float* z_out, void* stream);

/* NeRFRenderer.composite, compositing half (render/nerf.py:178-182,223-249).
 * rgbsigma (N,K,4) model output -> weights (N,K) [nullable], rgb (N,3), depth (N). */
int32_t pnr_composite(const float* rays, const float* z, const float* rgbsigma, int64_t n_rays, int32_t K,
                      int32_t white_bkgd, float* weights_out, float* rgb_out, float* depth_out, void* stream);

/* sample_fine + sample_fine_depth + cat + sort (render/nerf.py:120-161,285-295).
 * -> z_out (N, Kc + n_fine) ascending. */
int32_t pnr_sample_fine(const float* rays, const float* z_coarse, const float* weights, const float* depth,
                        int64_t n_rays, int32_t n_coarse, int32_t n_fine, int32_t n_fine_depth,
                        float depth_std, int32_t lindisp, const float* u, const float* r, const float* g,
                        uint64_t seed, int64_t ray_index_base, float* z_out, void* stream);

/* PixelNeRFNet.forward (models.py.backup2:155-282): world points -> (r,g,b,sigma).
 * Two ways to name the points:
 *   rays != NULL: point (ray i, sample k) = o_i + z[i,k] d_i, viewdir d_i  (render/nerf.py:185,204);
 *                 n_points = n_rays*K, out (n_rays, K, 4)
 *   rays == NULL: explicit xyz / viewdirs (SB, P, 3); n_points = SB*P, out (SB, P, 4)
 * points_per_obj = points per object (n_points / views->n_objs). */
int32_t pnr_point_mlp(const pnr_params* params, const pnr_mlp* mlp, const pnr_views* views,
                      const float* rays, const float* z, int32_t K,
                      const float* xyz, const float* viewdirs,
                      int64_t n_points, int64_t points_per_obj,
                      float* out, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- the whole path: NeRFRenderer.forward with a PixelNeRFNet model (render/nerf.py:251-303) --- */
/* rays (N,8), N = SB*B, rays_per_obj = B.  fine may be NULL (mlp_fine=None -> coarse MLP, backup2:258).
 * PNR_BF16 / PNR_F16: each pass is ONE kernel launch — coarse positions (sample_coarse) are generated in the kernel, every
 * workgroup composites the rays it evaluated; the resampling (sample_fine .. sort) runs at the head of the fine launch for
 * batches of up to 2048 rays and as one launch between the passes above that; the results are bit-identical to calling the
 * stage entry points above in sequence.  PNR_F32: the stages in sequence. */
uint64_t pnr_workspace_bytes(const pnr_params* params, const pnr_mlp* mlp, const pnr_views* views,
                             int64_t n_rays);
int32_t pnr_render(const pnr_params* params, const pnr_mlp* coarse, const pnr_mlp* fine,
                   const pnr_views* views, const float* rays, int64_t n_rays, int64_t rays_per_obj,
                   const pnr_noise* noise, uint64_t seed, int64_t ray_index_base,
                   const pnr_outputs* outputs, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- training: the same path under autograd, train/train.py:324-346,382-410 ---------- */
/* Gradient buffers, shaped like the pnr_mlp weights; every non-NULL member is ACCUMULATED into (+=: per-split partial
 * products summed by an ordered reduction, no floating-point atomics — bit-reproducible), so the caller zeroes
 * them (or passes .grad tensors).  NULL members are skipped. */
typedef struct pnr_mlp_grads {
    float* lin_in_w;  float* lin_in_b;
    float* lin_z_w[PNR_MAX_BLOCKS];  float* lin_z_b[PNR_MAX_BLOCKS];
    float* fc0_w[PNR_MAX_BLOCKS];    float* fc0_b[PNR_MAX_BLOCKS];
    float* fc1_w[PNR_MAX_BLOCKS];    float* fc1_b[PNR_MAX_BLOCKS];
    float* lin_out_w; float* lin_out_b;
} pnr_mlp_grads;

/* Saved activations of one pnr_point_mlp_train_fwd call (what autograd would keep for ResnetFC.forward,
 * resnetfc.py:173-236) and the scratch its backward needs.  fp32 arithmetic, fp32 latent maps required. */
uint64_t pnr_train_tape_bytes(const pnr_mlp* mlp, const pnr_views* views, int64_t n_points);   /* fp32 tape: the upper bound */
/* the tape of a call with these params (precision = PNR_BF16 keeps a 16-bit tape: ~0.6 x the bytes) */
uint64_t pnr_train_tape_bytes_for(const pnr_params* params, const pnr_mlp* mlp, const pnr_views* views, int64_t n_points);
uint64_t pnr_train_bwd_workspace_bytes(const pnr_mlp* mlp, const pnr_views* views, int64_t n_points);

/* PixelNeRFNet.forward as pnr_point_mlp (same point naming), keeping the tape. */
int32_t pnr_point_mlp_train_fwd(const pnr_params* params, const pnr_mlp* mlp, const pnr_views* views,
                                const float* rays, const float* z, int32_t K,
                                const float* xyz, const float* viewdirs,
                                int64_t n_points, int64_t points_per_obj,
                                float* out, void* tape, uint64_t tape_bytes, void* stream);

/* Backward of the call above: d_out (n_points,4) w.r.t. the activated outputs `out`.
 *   grads      MLP weight/bias gradients (+=)
 *   d_latent   per level, same shape as views->latent[level] (+=), or NULL entries / NULL array (encoder frozen,
 *              PixelNeRFNet.stop_encoder_grad, models.py.backup2:228-229)
 *   d_xyz      (n_points,3) explicit mode, or d_z (n_rays,K) rays mode: gradient w.r.t. the sample
 *              positions (needed because nerf.py:287-289 does not detach the depth-guided samples); NULL = skip */
int32_t pnr_point_mlp_bwd(const pnr_params* params, const pnr_mlp* mlp, const pnr_views* views,
                          const float* rays, const float* z, int32_t K,
                          const float* xyz, const float* viewdirs,
                          int64_t n_points, int64_t points_per_obj,
                          const float* out, const float* d_out, void* tape, uint64_t tape_bytes,
                          const pnr_mlp_grads* grads, float* const* d_latent, float* d_xyz, float* d_z,
                          void* workspace, uint64_t workspace_bytes, void* stream);

/* pnr_point_mlp_bwd plus the camera gradients the reference's autograd gives (xyz = o + z d, the view directions, and
 * self.poses / self.focal / self.c, models.py.backup2:108-150,166-221).  Three more outputs, each may be NULL:
 *   d_dirs   (n_points, 3)  explicit mode only: gradient at viewdirs
 *   d_rays   (n_rays, 8)    rays mode only: columns 0:3 d(origin), 3:6 d(direction); columns 6:8 (near, far) are written
 *                           as exact zeros (the reference's are not: a documented deviation)
 *   d_cam    (n_objs*n_views, 16), 16-byte aligned: per stored view [dR 9, row-major | dt 3 | dfx dfy dcx dcy], the gradient
 *            at views->w2c and at the (fx, fy, cx, cy) that view reads (fy in its stored, negated form).  A caller whose
 *            focal / c hold fewer rows than views sums the records of the views that share a row.
 * Every output is written (=), not accumulated.  With all three NULL the call is pnr_point_mlp_bwd: same launches, same
 * workspace.  A mode / output mismatch (d_rays with explicit points, d_dirs with rays) returns PNR_E_SHAPE before any launch.
 * workspace: pnr_train_bwd_cam_workspace_bytes(mlp, views, n_points, want_point = d_dirs or d_rays wanted, want_cam);
 * with both flags 0 it equals pnr_train_bwd_workspace_bytes.
 *
 * Arithmetic, for point g and view v (R, t the stored w2c rows, p and d the world point and direction, xr = R p,
 * xc = xr + t, dr = R d; du, dv the gradient at the pixel coordinate with the level's uv scale applied):
 *   ddr   = gradient at dr: the identity and sine entries of the 6-wide code (use_code_viewdirs), else the three raw columns
 *   dt    = (du (-fx/zc), dv (-fy/zc), du xc fx/zc^2 + dv yc fy/zc^2)       the projection's share only: the positional code
 *                                                                          reads xr without t
 *   dxr   = dt + gradient of the positional code at xr
 *   dR[i][j] = dxr[i] p[j] + ddr[i] d[j];  dfx = du (-xc/zc), dfy = dv (-yc/zc), dcx = du, dcy = dv
 *   d_dir = sum_v R^T ddr,  dp = sum_v R^T dxr;  per ray d_o = sum_k dp_k, d_d = sum_k (z_k dp_k + d_dir_k)
 * Summation order (no floating-point atomics; every output is bit-reproducible): the (point, view) records are fp32; the
 * points of an (object, view) are cut into chunks of 1024; inside a chunk sub-sum s = 0..15 adds records s, s+16, .. in that
 * order in fp64 and the 16 sub-sums are added in order s = 0..15; the chunk sums are folded in chunk order in fp64 and
 * rounded once to fp32.  The per-ray sums run over k = 0..K-1 in fp64 and are rounded once. */
uint64_t pnr_train_bwd_cam_workspace_bytes(const pnr_mlp* mlp, const pnr_views* views, int64_t n_points,
                                           int32_t want_point, int32_t want_cam);
int32_t pnr_point_mlp_bwd_cam(const pnr_params* params, const pnr_mlp* mlp, const pnr_views* views,
                              const float* rays, const float* z, int32_t K,
                              const float* xyz, const float* viewdirs,
                              int64_t n_points, int64_t points_per_obj,
                              const float* out, const float* d_out, void* tape, uint64_t tape_bytes,
                              const pnr_mlp_grads* grads, float* const* d_latent, float* d_xyz, float* d_z,
                              float* d_dirs, float* d_rays, float* d_cam,
                              void* workspace, uint64_t workspace_bytes, void* stream);

/* Backward of pnr_composite (render/nerf.py:178-182,223-249).  d_weights / d_rgb / d_depth may be NULL (zero);
 * writes d_rgbsigma (N,K,4) and, when non-NULL, d_z (N,K) (deltas and depth depend on z). */
int32_t pnr_composite_bwd(const float* rays, const float* z, const float* rgbsigma, int64_t n_rays, int32_t K,
                          int32_t white_bkgd, const float* d_weights, const float* d_rgb, const float* d_depth,
                          float* d_rgbsigma, float* d_z, void* stream);

/* Backward of pnr_sample_fine w.r.t. the coarse depth (only the n_fine_depth samples are differentiable):
 * g / seed / ray_index_base as given to the forward call; z_sorted is its output. */
int32_t pnr_sample_fine_bwd(const float* rays, const float* depth, int64_t n_rays, int32_t n_coarse,
                            int32_t n_fine, int32_t n_fine_depth, float depth_std, const float* g,
                            uint64_t seed, int64_t ray_index_base, const float* z_sorted,
                            const float* d_z_sorted, float* d_depth, void* stream);

/* ResnetFC.forward (model/resnetfc.py:173-236) on rows the caller assembled: zx (n_outer, n_inner_views, n_inner_points,
 * d_latent + d_in) fp32 with the latent part FIRST; the n_inner_views row blocks are reduced (mean / max, util.py:466-476)
 * in front of block combine_layer, i.e. combine_inner_dims = (n_inner_views, n_inner_points).  out (n_outer,
 * n_inner_points, d_out), no activation.  fp32 arithmetic (the 1e-4 parity path); any d_hidden / d_out. */
uint64_t pnr_resnetfc_workspace_bytes(const pnr_mlp* mlp, int32_t n_inner_views);
int32_t pnr_resnetfc_forward(const pnr_mlp* mlp, const float* zx, int64_t n_outer, int32_t n_inner_views,
                             int64_t n_inner_points, float* out, void* workspace, uint64_t workspace_bytes,
                             void* stream);

/* SpatialEncoder.index (model/encoder.py:138-205): uv (uv_views, n_points, 2) image points -> out (n_objs*n_views, L,
 * n_points) fp32; bilinear, border padding, align_corners, every level normalised by ITS latent size and concatenated
 * along the channels.  uv_views = 1 broadcasts one set of points to every view (encoder.py:148-149), else n_objs*n_views.
 * Reads views->latent[] (fp32 NCHW) and lat_c/h/w only. */
int32_t pnr_index_latent(const pnr_views* views, const float* uv, int64_t n_points, int32_t uv_views, float* out,
                         void* stream);

/* pnr_render for the rays of ONE camera, generated inside the render launch (util.gen_rays, util/util.py:118-148,243-281, then
 * NeRFRenderer.forward): ray i is pixel pix0 + i (row-major) of the W x H pinhole image of camera-to-world matrix c2w.
 * What the reference's eval drivers do per frame (eval/eval.py:250-293: gen_rays on the host, H2D, split, render_par per
 * chunk) as one call with no ray tensor.  views->n_objs must be 1.  Results are bit-identical to pnr_gen_rays + pnr_render.
 * ray_index_base counts rays for the in-kernel noise exactly as in pnr_render (pass pix0 when sharding one frame). */
int32_t pnr_render_camera(const pnr_params* params, const pnr_mlp* coarse, const pnr_mlp* fine,
                          const pnr_views* views, const float* c2w /* host, 16 floats */, int32_t W, int32_t H,
                          float fx, float fy, float cx, float cy, float z_near, float z_far, int64_t pix0,
                          int64_t n_rays, const pnr_noise* noise, uint64_t seed, int64_t ray_index_base,
                          const pnr_outputs* outputs, void* workspace, uint64_t workspace_bytes, void* stream);

/* util.gen_rays for one camera (util/util.py:118-148,243-281): pixels [pix0, pix0+n) of a W x H pinhole image. */
int32_t pnr_gen_rays(const float* c2w /* host, 16 floats */, int32_t W, int32_t H, float fx, float fy,
                     float cx, float cy, float z_near, float z_far, int64_t pix0, int64_t n,
                     float* rays_out, void* stream);

/* ---- training front end: the batch and the loss of Trainer.calc_losses (train/train.py:237-373) ---------------------- */
/* Rays and ground-truth colours of sampled pixels (train.py:280-311, which builds gen_rays of ALL NV views and keeps B rows):
 * one thread per sampled ray.  pix_inds[o, i] = view * H * W + row * W + col (train.py:298) names a pixel of object o;
 * rays_out[o, i] = [pose[:3, 3], R . unproj(col, row), z_near, z_far], bit-identical to what pnr_gen_rays writes for that
 * camera and pixel; rgb_gt_out[o, i] = 0.5 * images[o, view, :, row, col] + 0.5 (bit-identical to torch's images * 0.5 + 0.5).
 * The indices live on the device, so the kernel is the range check: an index outside [0, NV*H*W) reads nothing and its row of
 * both outputs is written as NaN.  NV*H*W must be below 2^31. */
int32_t pnr_train_batch(const float* images,   /* (SB, NV, 3, H, W), in [-1, 1] as the data loader gives them; may be NULL with rgb_gt_out NULL */
                        const float* poses,    /* (SB, NV, 4, 4) camera-to-world */
                        const float* focal,    /* (SB, 2): fx, fy */
                        const float* c,        /* (SB, 2), or NULL = (W/2, H/2) */
                        int32_t SB, int32_t NV, int32_t W, int32_t H, float z_near, float z_far,
                        const int64_t* pix_inds, /* (SB, B) */
                        int64_t B, float* rays_out /* (SB, B, 8) */, float* rgb_gt_out /* (SB, B, 3) or NULL */,
                        void* stream);

/* torch.nn.MSELoss / L1Loss(reduction="mean") (model/loss.py:99-103) of the coarse and the fine colours, dense (n_rays, 3),
 * as train.py:338-346 combines them: L = mean over 3*n_rays elements of (x - gt)^2 or |x - gt|;
 *   losses[0] = lambda_coarse * Lc, losses[1] = lambda_fine * Lf (0 without a fine pass)    — loss_dict "rc", "rf"
 *   losses[2] = total = losses[0] + losses[1], or Lc (no lambda) when fine_rgb is NULL        — loss_dict "t"
 * One launch of one workgroup, fixed summation order (csrc/loss.hip), no atomics: the same inputs give the same bits.
 * n_rays == 0 writes three zeros. */
int32_t pnr_rgb_loss(const float* coarse_rgb, const float* fine_rgb /* NULL: no fine pass */, const float* rgb_gt,
                     int64_t n_rays, int32_t use_l1, float lambda_coarse, float lambda_fine,
                     float* losses /* 3 floats */, void* stream);
/* Gradient of `total`: d_x = d_total * w * 2 (x - gt) / (3 n_rays), or d_total * w * sign(x - gt) / (3 n_rays) with
 * sign(0) = 0 for L1; w = the weight the pass has in total (lambda, or 1 for the coarse pass when fine_rgb is NULL).  d_total is
 * read on the device (a GradScaler scale arrives without a host round trip); a power of two scales every element exactly. */
int32_t pnr_rgb_loss_bwd(const float* coarse_rgb, const float* fine_rgb, const float* rgb_gt, int64_t n_rays,
                         int32_t use_l1, float lambda_coarse, float lambda_fine,
                         const float* d_total /* 1 float; NULL = 1 */,
                         float* d_coarse_rgb, float* d_fine_rgb /* (n_rays, 3); either may be NULL */, void* stream);

/* ---- opacity losses on the compositing weights, csrc/opacity_loss.hip ------------------------------------------------------------
 * The reference's AlphaLossNV2 (model/loss.py:24-37) in both of its modes and a binary cross entropy against a foreground mask, for
 * the coarse and / or the fine pass's weights (n_rays, K) as the renderer leaves them under want_weights.  Everything from the
 * weights' sum to the loss is fp64; each output is rounded to fp32 once.  No atomics: the same inputs give the same bits.
 *
 * Per pass alpha_r = sum_k (double) w[r, k], one wave per ray, in an order the shape alone fixes: lane l (0..63) adds w[r, l],
 * w[r, l + 64], .. in ascending k starting from +0, then the 64 lane sums are folded by an xor butterfly over lane distances
 * 32, 16, 8, 4, 2, 1 (v = v + v[lane ^ d]).  alpha_out[0, r] is the coarse pass's, alpha_out[1, r] the fine pass's; the row of a
 * NULL pass is not written.  a = alpha < lo ? lo : (alpha > hi ? hi : alpha) with lo = (double) clamp_lo, hi = (double) clamp_hi:
 * torch.clamp, a NaN stays a NaN.  The per-ray term t_r:
 *   PNR_ALPHA_NV2     t = log a + log(1 - a), then t < -clamp_alpha ? -clamp_alpha : t        (loss.py:32-33)
 *   PNR_ALPHA_OPAQUE  t = -log a                                                              (BCELoss(a, 1), loss.py:28-30)
 *   PNR_ALPHA_MASK    t = -(m log a + (1 - m) log(1 - a)), m = (double) mask[r], any m in [0, 1]
 * L = (sum_r t_r) / n_rays: ray r goes to thread r % 1024 of ONE workgroup, a thread adds its rays in ascending r, a wave folds by
 * the butterfly above, and the 16 wave sums are added in ascending wave order.  (The term is evaluated by the workgroup that sums
 * it: the call has no workspace, and alpha_out is what the backward needs.)
 *   losses[0] = (float)((double) lambda_coarse * Lc), 0 for a NULL pass;  losses[1] = (float)((double) lambda_fine * Lf), likewise
 *   losses[2] = losses[0] + losses[1] in fp32.  The lambdas ALWAYS apply — unlike pnr_rgb_loss, whose total drops lambda_coarse
 *   when there is no fine pass.  n_rays == 0 writes three zeros.
 * Two launches: a grid over the rays for alpha, one workgroup for the terms and their sum.
 *
 * pnr_alpha_loss_bwd, one launch, one wave per ray: with g = t'(a) —
 *   NV2  1 / a - 1 / (1 - a), and 0 where log a + log(1 - a) < -clamp_alpha;   OPAQUE  -1 / a;   MASK  -(m / a - (1 - m) / (1 - a))
 * — and g = 0 where alpha < lo or alpha > hi (both bounds pass at equality: torch's clamp backward; a NaN alpha passes and stays a
 * NaN), d_w[r, k] = (float)((double) d_total * ((double) lambda / n_rays * g)) for every k.  d_total is read on the device; a
 * power of two scales every element exactly.  alpha is what the forward wrote; Kc, Kf, mode and the clamps must be the forward's.
 *   PNR_E_NULL   both passes NULL (forward: coarse_w and fine_w; backward: d_coarse_w and d_fine_w), PNR_ALPHA_MASK without mask,
 *                alpha_out / alpha or losses NULL
 *   PNR_E_SHAPE  K < 1 for a pass that is not NULL, n_rays < 0 or > 2^32, a mode outside the three, clamp_lo / clamp_hi not
 *                satisfying 0 < clamp_lo < clamp_hi < 1
 *   PNR_E_ALIGN  alpha_out / alpha not 8-byte aligned
 * Nothing is allocated or read back; every check runs before any launch. */
enum { PNR_ALPHA_NV2 = 0, PNR_ALPHA_OPAQUE = 1, PNR_ALPHA_MASK = 2 };
int32_t pnr_alpha_loss(const float* coarse_w /* (n_rays, Kc) or NULL */, int32_t Kc, const float* fine_w /* (n_rays, Kf) or NULL */,
                       int32_t Kf, const float* mask /* (n_rays); PNR_ALPHA_MASK only */, int64_t n_rays, int32_t mode,
                       float lambda_coarse, float lambda_fine, float clamp_lo, float clamp_hi, float clamp_alpha,
                       double* alpha_out /* (2, n_rays) */, float* losses /* 3 floats */, void* stream);
int32_t pnr_alpha_loss_bwd(const double* alpha /* (2, n_rays), what the forward wrote */, const float* mask, int64_t n_rays, int32_t Kc,
                           int32_t Kf, int32_t mode, float lambda_coarse, float lambda_fine, float clamp_lo, float clamp_hi,
                           float clamp_alpha, const float* d_total /* 1 float on the device; NULL = 1 */,
                           float* d_coarse_w /* (n_rays, Kc) or NULL */, float* d_fine_w /* (n_rays, Kf) or NULL */, void* stream);

/* ---- evaluation back end: what eval/eval.py:286-347 does with a rendered frame, on the device ---------------------------- */
/* One frame, where the render left it: x = clamp(rgb, 0, 1) (eval.py:291-293; a NaN stays a NaN), g = 0.5 * gt + 0.5
 * (eval.py:318, the bits of torch's images * 0.5 + 0.5), both fp32.
 *   rgb_u8      (uint8) trunc(x * 255.0f): one fp32 product, then truncation — (all_rgb * 255).astype(np.uint8), eval.py:301;
 *               the byte of a NaN is 0
 *   compare_u8  the same quantisation of np.hstack((x, g)) (the reference's write_compare strip)
 *   depth_norm  (depth - z_near) / (z_far - z_near), eval.py:288-289
 *   metrics[0]  mean over 3 H W elements of (x - g)^2; PSNR (eval.py:324-328, data_range 1) is 10 log10(1 / metrics[0])
 *   metrics[1]  mean SSIM (eval.py:329-332: skimage compare_ssim, multichannel, data_range 1, restated from the published
 *               definition): per channel, on the window centres 3 <= row < H - 3, 3 <= col < W - 3 (whole windows only),
 *               mu = the 7 x 7 mean, v = the sample (co)variance of the window (divisor 48), C1 = 1e-4, C2 = 9e-4,
 *               S = ((2 mu_x mu_y + C1)(2 v_xy + C2)) / ((mu_x^2 + mu_y^2 + C1)(v_x + v_y + C2)), averaged over centres and
 *               channels.  The moments are CENTRED sums, sum (x - mu_x)(y - mu_y), in fp64: a white background keeps
 *               variances around 1e-7.  A NaN in the render makes both metrics NaN.
 * Strides in floats per pixel (0 = dense: 3, 1): with 4 / 4 and depth = rgb + 3 the frame is read from the packed (N, 4)
 * per-ray record of pnr_outputs.rgb_stride, where a sharded frame is gathered.  One launch over 16 x 16 tiles that leaves one
 * partial pair per tile in `workspace`, then one workgroup that adds them in a fixed order (csrc/eval.hip): no atomics, the
 * same inputs give the same bits.  Every check below is made before any launch:
 *   PNR_E_NULL       rgb NULL; compare_u8 or metrics without gt; depth_norm without depth; metrics without workspace
 *   PNR_E_SHAPE      W < 1, H < 1, W * H >= 2^31 or more than 2^23 tiles; a stride below the record's own width;
 *                    metrics with min(W, H) < 7; depth_norm with z_far == z_near
 *   PNR_E_WORKSPACE  metrics with fewer workspace bytes than the size function asks for (16 bytes per tile; 0 for a bad shape) */
uint64_t pnr_eval_frame_workspace_bytes(int32_t W, int32_t H);
int32_t pnr_eval_frame(const float* rgb, int32_t rgb_stride,       /* rendered (H*W) pixels x 3, UNclamped */
                       const float* depth, int32_t depth_stride,   /* (H*W), or NULL */
                       const float* gt,                            /* (3, H, W) planar in [-1, 1] as the data loader gives it, or NULL */
                       int32_t W, int32_t H, float z_near, float z_far,
                       uint8_t* rgb_u8,                            /* (H, W, 3), or NULL */
                       uint8_t* compare_u8,                        /* (H, 2W, 3), or NULL */
                       float* depth_norm,                          /* (H, W), or NULL */
                       double* metrics,                            /* 2 doubles, or NULL */
                       void* workspace, uint64_t workspace_bytes, void* stream);

/* F frames in one call: the tail of eval/eval_approx.py:136-148, which renders one target view of each of SB objects in one
 * call and compares them UNCLAMPED.  rgb: F frames of (H*W) pixels x 3, `rgb_stride` floats per pixel (0 = 3), `frame_stride`
 * floats from one frame to the next (0 = W * H * rgb_stride: a gap between frames is never read); gt (F, 3, H, W).  Per frame
 * the arithmetic of pnr_eval_frame's metrics, word for word — g = fmaf(gt, 0.5, 0.5), centred fp64 window moments, one partial
 * pair per 16 x 16 tile, a fixed-order fold without atomics — on x = clamp(rgb, 0, 1) when clamp != 0 (metrics[2 f], [2 f + 1]
 * are then bit for bit what pnr_eval_frame writes for frame f alone) and on x = rgb as it is when clamp == 0 (a NaN stays a
 * NaN either way and makes that frame's pair NaN).  One launch over F x tiles workgroups, one with a workgroup per frame that
 * folds that frame's pairs: frame f's pair depends on frame f's pixels only.  Every check is made before any launch:
 *   PNR_E_NULL       rgb, gt, metrics or workspace NULL
 *   PNR_E_SHAPE      F < 1; min(W, H) < 7; W * H >= 2^31; F x tiles > 2^23; rgb_stride 1 or 2 (or negative); a non-zero
 *                    frame_stride below W * H * rgb_stride
 *   PNR_E_WORKSPACE  fewer workspace bytes than the size function asks for (16 bytes per frame and tile; 0 for a bad shape) */
uint64_t pnr_eval_frames_workspace_bytes(int32_t F, int32_t W, int32_t H);
int32_t pnr_eval_frames(const float* rgb, int32_t rgb_stride   /* floats per pixel, 0 = 3 */,
                        int64_t frame_stride                   /* floats between frames, 0 = W*H*rgb_stride */,
                        const float* gt                        /* (F, 3, H, W) planar, in [-1, 1] */,
                        int32_t F, int32_t W, int32_t H, int32_t clamp,
                        double* metrics                        /* (F, 2): mse, mean SSIM */,
                        void* workspace, uint64_t workspace_bytes, void* stream);

/* F pairs of saved 8-bit images in one call: the arithmetic of eval/calc_metrics.py:218-234, which reads the PNGs eval.py
 * wrote and the dataset's images back and recomputes PSNR and SSIM on them.  pred (F, H, W, pred_channels) and gt
 * (F, H, W, gt_channels), uint8, dense and interleaved as a PNG decoder returns them, 3 or 4 channels each: frame f starts at
 * byte f * H * W * channels, NO alignment is assumed (a 7 x 7 RGB frame is 147 bytes), and a fourth channel is never part of
 * any result (the reference's [..., :3]).  x = float(p) / 255.0f, ONE correctly rounded fp32 division — the bits of
 * imageio.imread(..).astype(np.float32) / 255.0, :226-227 — and g the same of the ground truth; on (x, g) the arithmetic of
 * pnr_eval_frames, word for word: centred fp64 window moments, whole 7 x 7 windows only, divisor 48, C1 = 1e-4, C2 = 9e-4, one
 * partial pair per 16 x 16 tile, the same fixed-order fold without atomics.  (The exact integer window sums 8-bit inputs
 * would allow are deliberately not used: the reference's inputs are the rounded quotients, and the two entry points share one
 * arithmetic.)  metrics[2 f] = mean squared error, metrics[2 f + 1] = mean SSIM of pair f, which depend on pair f's bytes only.
 * pred_planar / gt_planar, when not NULL: x * 2.0f - 1.0f (two fp32 operations) as (F, 3, H, W), the LPIPS inputs of :232-233.
 * One launch over F x tiles workgroups, then the fold with a workgroup per frame.  Every check is made before any launch:
 *   PNR_E_NULL       pred, gt, metrics or workspace NULL
 *   PNR_E_SHAPE      F < 1; min(W, H) < 7; a channel count other than 3 or 4; W * H >= 2^31; F x tiles > 2^23
 *   PNR_E_WORKSPACE  fewer workspace bytes than the size function asks for (that of pnr_eval_frames; 0 for a bad shape) */
uint64_t pnr_eval_frames_u8_workspace_bytes(int32_t F, int32_t W, int32_t H);
int32_t pnr_eval_frames_u8(const uint8_t* pred, int32_t pred_channels   /* (F, H, W, pred_channels), 3 or 4 */,
                           const uint8_t* gt, int32_t gt_channels       /* (F, H, W, gt_channels), 3 or 4 */,
                           int32_t F, int32_t W, int32_t H,
                           float* pred_planar, float* gt_planar         /* (F, 3, H, W) each, or NULL */,
                           double* metrics                              /* (F, 2): mse, mean SSIM */,
                           void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- visualisation: the colour map of src/util/util.py:13-30 and the panel of train/train.py:423-537 (vis_step), csrc/vis.hip -- */
/* quantize(map), the reference's image_float_to_uint8 for a float32 map:
 *   vmin, vmax  the map's fp32 minimum and maximum; a NaN anywhere makes both NaN (np.min)
 *   widening    if vmax - vmin (one fp32 subtraction) < 1e-10, compared in fp64: vmax = fp32(double(vmax) + 1e-10)
 *   q           (x - vmin) / (vmax - vmin): one fp32 subtraction, one correctly rounded fp32 division
 *   byte        trunc(q * 255.0f), ONE fp32 product contracted with nothing; a product that is not finite gives 0 (numpy's cast
 *               is undefined there; 0 is what it yields where this was developed)
 * So a constant non-zero map (0 / 0) and a map with a NaN are byte 0 everywhere, the all-zero map too (0 / 1e-10), and the
 * largest element of any other map is byte 255.
 * cmap(map, lut) = lut[quantize(map)], lut a (256, 3) uint8 table on the device, owned by the caller.  The package's default
 * table (util.hot_lut) is PARITY UNPINNED: it restates the "hot" ramp (r = min(1, x / 0.375), g = clamp((x - 0.375) / 0.375),
 * b = clamp((x - 0.75) / 0.25), x = i / 255 in fp64, byte floor(255 v + 0.5), RGB order); OpenCV's own COLORMAP_HOT table may
 * differ and comes out as BGR, which the reference shows unswapped.  Whoever has cv2 passes its table.
 *
 * pnr_cmap: out_u8 (H, W, 3) = cmap(map); minmax (2 floats, or NULL) = vmin, vmax before the widening.  `stride` in floats per
 * pixel (0 = 1) lets `map` look into a per-pixel record.  Three launches: per-tile (min, max) into the workspace, one workgroup
 * that folds them in tile order, the writer.  No atomics, nothing allocated, nothing read back, the same inputs give the same
 * bits.  Checks, all before any launch:
 *   PNR_E_NULL       map, out_u8, lut or workspace NULL
 *   PNR_E_SHAPE      W < 1, H < 1, W * H >= 2^31 or more than 2^23 tiles; stride < 1
 *   PNR_E_WORKSPACE  fewer bytes than pnr_cmap_workspace_bytes (64 + 8 per 16 x 16 tile; 0 for a bad shape)
 *   PNR_E_ALIGN      workspace not 4-byte aligned */
#define PNR_VIS_MAX_SRC 8
uint64_t pnr_cmap_workspace_bytes(int32_t W, int32_t H);
int32_t  pnr_cmap(const float* map, int32_t stride /* floats per pixel, 0 = 1 */, int32_t W, int32_t H,
                  const uint8_t* lut /* device, 256 x 3 */, uint8_t* out_u8 /* (H, W, 3) */,
                  float* minmax /* 2 floats, or NULL */, void* workspace, uint64_t workspace_bytes, void* stream);

/* pnr_vis_panel: the panel of vis_step for ONE target view.  n_pass rows of height H (coarse, then fine if there is one), each
 * [src_0 .. src_{NS-1}, gt, cmap(depth), rgb, cmap(alpha)] in tiles W wide: (n_pass H, (NS + 4) W, 3).
 *   image tiles  0.5 * image + 0.5 with the bits of torch's images * 0.5 + 0.5 (as pnr_eval_frame's g)
 *   alpha[p]     sum_k weights[p, k] (train.py:480,485), accumulated in fp64 in ascending k, rounded once to fp32.  NOT PINNED
 *                to torch's fp32 .sum(-1), whose order is unspecified: all terms are non-negative, so the two are within
 *                K * 2^-24 * alpha[p] of each other
 *   panel_f32    the image tiles as above, the rendered rgb as it is (unclamped), the colour-map bytes as fp32(byte) / 255.0f
 *                (for all 256 bytes the reference's float64 byte / 255 rounded to fp32)
 *   panel_u8     trunc(clamp(x, 0, 1) * 255.0f) of the same values; for the colour-map tiles the LUT byte itself
 *   alpha        (n_pass, H, W), the opacity maps
 *   stats        n_pass x 6 fp32: rgb min, max, alpha min, max, depth min, max (the reference prints the first four)
 *   mse          mean over 3 H W elements of (double(x) - double(g))^2, x the LAST pass's unclamped rgb, g the ground-truth tile;
 *                fp64 sums in a fixed order.  PSNR = -10 log10(mse) (util.psnr)
 * Strides in floats per pixel (0 = dense: 3, 1, K) let the pass pointers look into the packed per-ray record of
 * NeRFRenderer.forward_packed.  src_views and passes are HOST arrays, read before the call returns.  Three launches on the
 * caller's stream: pixel tiles (alpha, per-tile extrema and squared-error sums into the workspace), one workgroup that folds
 * them in tile order into stats, mse and a record in the workspace, the writer over output tiles (only when a panel is asked
 * for).  No floating-point atomics, nothing allocated, nothing read back, the same inputs give the same bits.  Checks, all
 * before any launch:
 *   PNR_E_NULL       images, src_views, passes or lut NULL; a pass without rgb, depth or weights; an output (mse among them)
 *                    without a workspace
 *   PNR_E_SHAPE      W < 1, H < 1, W * H >= 2^31 or more than 2^23 tiles; n_pass not 1 or 2; NS < 1 or NS > PNR_VIS_MAX_SRC;
 *                    NV < 1; a view index outside [0, NV); K < 1; a stride below the record's own width
 *   PNR_E_WORKSPACE  fewer bytes than pnr_vis_panel_workspace_bytes (64 + (8 + 24 n_pass) per tile + 4 n_pass W H; 0 for a
 *                    bad shape)
 *   PNR_E_ALIGN      workspace not 8-byte aligned
 * With every output NULL the call returns 0 and launches nothing. */
typedef struct pnr_vis_pass {      /* one row of the panel: what the renderer left for this pass */
    const float* rgb; const float* depth; const float* weights;      /* (H*W) x 3, (H*W), (H*W) x K */
    int32_t rgb_stride, depth_stride, weights_stride;                /* floats per pixel; 0 = dense (3, 1, K) */
    int32_t K;
} pnr_vis_pass;
uint64_t pnr_vis_panel_workspace_bytes(int32_t W, int32_t H, int32_t n_pass);
int32_t  pnr_vis_panel(const float* images /* device, (NV, 3, H, W) in [-1, 1] */, int32_t NV,
                       const int32_t* src_views /* HOST, NS entries */, int32_t NS, int32_t gt_view,
                       const pnr_vis_pass* passes /* HOST */, int32_t n_pass /* 1 or 2 */, int32_t W, int32_t H,
                       const uint8_t* lut, float* panel_f32, uint8_t* panel_u8 /* either may be NULL */,
                       float* alpha /* (n_pass, H, W) or NULL */, float* stats /* n_pass x 6 or NULL */,
                       double* mse /* 1 double or NULL */, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- novel-view video: the two ends of eval/gen_video.py and eval/eval_real.py on the device, csrc/video.hip ------------------
 * byte(p), the quantisation of a product p shared by pnr_video_frames and pnr_view_strip:
 *   in range      -1 < p < 256: truncation toward zero, numpy's astype(np.uint8) wherever numpy's cast is defined; a small
 *                 negative product and -0.0 give 0
 *   out of range  everything else, NaN included, where numpy's cast is undefined and the drivers do not clamp: the byte
 *                 saturates, 0 for p <= -1 and for NaN, 255 for p >= 256
 *
 * pnr_video_frames: F rendered frames to bytes in ONE launch — (frames.cpu().numpy() * 255).astype(np.uint8), gen_video.py:236,
 * eval_real.py:151.  out_u8 (F, H, W, 3) = byte(x * 255.0f): ONE fp32 product contracted with nothing, then byte().  rgb holds
 * F H W pixels, `rgb_stride` floats apart (0 = dense: 3; 4 = the packed per-ray record of pnr_outputs.rgb_stride, where a
 * camera path is rendered frame after frame).  out_u8 may start at ANY byte: the kernel is flat over the byte stream, a thread
 * owns three whole dwords (four pixels), and the up to three bytes in front of the first whole dword and behind the last are
 * written one by one, so nothing outside the 3 F H W bytes is touched.  float4 loads are used only for a dense rgb whose base is
 * 16-byte aligned under a dword-aligned out_u8; the bytes do not depend on the route.
 *   n_out_of_range  optional device int64, SET by the call (zeroed on the stream, then integer atomic adds, at most one per
 *                   workgroup): the number of out-of-range components over all frames.  Exact, whatever the order.
 * Checks, all before any launch:
 *   PNR_E_NULL   rgb or out_u8 NULL
 *   PNR_E_SHAPE  F, W or H < 1, W * H >= 2^31 or F * W * H >= 2^31; a stride below 3
 *   PNR_E_ALIGN  rgb not 4-byte aligned, n_out_of_range not 8-byte aligned
 *
 * pnr_view_strip: the picture of the source views, gen_video.py:239-241.  images (NS, 3, H, W) fp32 -> out_u8 (H, NS W, 3), laid
 * out as np.hstack over the views, = byte(((x * scale) + lo) * 255.0f): three separately rounded fp32 operations in that order.
 * scale = lo = 0.5 is the reference's images * 0.5 + 0.5 for a [-1, 1] input; scale = 1, lo = 0 serves a [0, 1] input.
 *   PNR_E_NULL   images or out_u8 NULL
 *   PNR_E_SHAPE  NS, W or H < 1, W * H >= 2^31 or NS * W * H >= 2^31
 *   PNR_E_ALIGN  images not 4-byte aligned
 *
 * pnr_image_to_tensor: an 8-bit image (H, W, 3) on the device -> the network's input (3, H, W) fp32.
 *   balanced = 0  float(b) / 255.0f, one correctly rounded fp32 division: torchvision's ToTensor, which is all that the
 *                 reference fork's get_image_to_tensor_balanced does (src/util/util.py:68-79)
 *   balanced = 1  (float(b) / 255.0f - 0.5f) / 0.5f, each operation rounded on its own: ToTensor + Normalize(0.5, 0.5), upstream
 *                 pixelNeRF's version, range [-1, 1]
 * Pinned to torch's own arithmetic, t.float().div(255)[.sub(0.5).div(0.5)] on the CPU; PARITY UNPINNED against torchvision
 * itself, which is not importable where this library is developed.
 *   PNR_E_NULL   img_u8 or out NULL
 *   PNR_E_SHAPE  W or H < 1, W * H >= 2^31; balanced not 0 or 1
 *   PNR_E_ALIGN  out not 4-byte aligned
 * None of the three reads anything back or allocates. */
int32_t pnr_video_frames(const float* rgb, int32_t rgb_stride /* floats per pixel, 0 = 3 */, int32_t F, int32_t W, int32_t H,
                         uint8_t* out_u8 /* (F, H, W, 3), any byte alignment */,
                         int64_t* n_out_of_range /* device, 1 int64, or NULL */, void* stream);
int32_t pnr_view_strip(const float* images /* (NS, 3, H, W) */, int32_t NS, int32_t W, int32_t H, float scale, float lo,
                       uint8_t* out_u8 /* (H, NS W, 3) */, void* stream);
int32_t pnr_image_to_tensor(const uint8_t* img_u8 /* (H, W, 3) */, int32_t W, int32_t H, int32_t balanced,
                            float* out /* (3, H, W) */, void* stream);

/* ---- data layer: batches whose images stay 8-bit on the device, csrc/data.hip ---------------------------------------------------
 * The images of a batch are the bytes their files hold, interleaved: images_u8 (SB, NV, H, W, C), C = 3 or 4 (a fourth channel
 * is stepped over).  T(b, balanced) below is exactly the fp32 value pnr_image_to_tensor writes for byte b (one device function
 * serves all three entry points).  images_u8 may start at ANY byte (a slice of a pool does); whole-dword loads are used only
 * where the addresses allow them, byte loads otherwise, and the output bits do not depend on the route.  No floating-point
 * atomics; nothing is allocated or read back; all checks run before any launch.
 *
 * pnr_train_batch_u8: pnr_train_batch with images_u8 in place of the fp32 images.
 *   rays_out            bit-identical to what pnr_train_batch writes for the same poses, intrinsics and indices (one device
 *                       function builds the ray in both kernels)
 *   rgb_gt_out[o, i, k] 0.5f * T(b, balanced) + 0.5f for the byte b of channel k at the pixel: bit-identical to pnr_train_batch
 *                       on the fp32 image T would have produced
 *   an index outside [0, NV*H*W) reads nothing and leaves a NaN row in both outputs, as in pnr_train_batch
 *   PNR_E_NULL   as for pnr_train_batch (images_u8 may be NULL with rgb_gt_out NULL)
 *   PNR_E_SHAPE  C not 3 or 4, balanced not 0 or 1, or pnr_train_batch's size conditions
 *   B == 0 returns 0 and launches nothing
 *
 * pnr_views_to_tensor_u8: the selected source views of a batch, converted where they lie.
 *   out[o, j, k, row, col] = T(images_u8[o, view_ord[o, j], row, col, k], balanced): per view what pnr_image_to_tensor gives on
 *   that view, bit for bit.  view_ord is never read on the host, so the kernel is the range check: a view index outside
 *   [0, NV) reads nothing and fills that view's three planes with NaN; a view may be named more than once.  No byte outside the
 *   selected views is read and nothing outside `out` is written.
 *   PNR_E_NULL   images_u8, view_ord or out NULL
 *   PNR_E_SHAPE  SB, NV, NS, W or H < 1, NV * H * W >= 2^31, C not 3 or 4, balanced not 0 or 1; SB * NS views of
 *                ceil(H W / 1024) workgroups each that do not fit one launch (2^31 - 1 workgroups)
 *   PNR_E_ALIGN  out not 4-byte aligned */
int32_t pnr_train_batch_u8(const uint8_t* images_u8 /* (SB, NV, H, W, C), any byte alignment; may be NULL with rgb_gt_out NULL */,
                           const float* poses /* (SB, NV, 4, 4) */, const float* focal /* (SB, 2) */,
                           const float* c /* (SB, 2) or NULL */, int32_t SB, int32_t NV, int32_t W, int32_t H, float z_near,
                           float z_far, const int64_t* pix_inds /* (SB, B) */, int64_t B, float* rays_out /* (SB, B, 8) */,
                           float* rgb_gt_out /* (SB, B, 3) or NULL */, int32_t C, int32_t balanced, void* stream);
int32_t pnr_views_to_tensor_u8(const uint8_t* images_u8 /* (SB, NV, H, W, C), any byte alignment */,
                               const int64_t* view_ord /* (SB, NS), device */, int32_t SB, int32_t NV, int32_t NS, int32_t W,
                               int32_t H, int32_t C, int32_t balanced, float* out /* (SB, NS, 3, H, W) */, void* stream);

/* ---- colour jitter of 8-bit batches, csrc/jitter.hip ----------------------------------------------------------------------------
 * Upstream pixelNeRF trains DTU under ColorJitterDataset: ONE brightness / contrast / saturation / hue draw per object, applied
 * on the host to every float view.  Here the draw is a record on the device and the two gathers above apply it to what a step
 * uses only — the sampled pixels and the chosen source views.  PARITY UNPINNED: the chain is torchvision's tensor arithmetic for
 * float images in [0, 1] as remembered; torchvision is not importable where this library is developed, so this text is the
 * specification.
 *
 * pnr_color_jitter_plan writes record_out[o] = [brightness, contrast, saturation, hue, mean, order code as a float 0..23, 0, 0].
 *   Draws: philox4x32 in the samplers' counter layout (key = seed, counter = (lo32(o), hi32(o), draw id 10, block)); ids 0..3, 8
 *   and 9 are taken, 4..7 are left free for the render path.  Block 0 gives one word each for brightness, contrast, saturation
 *   and hue, word 0 of block 1 the order code.  u = float(word >> 8) * 2^-24;  factor = lo + (hi - lo) * u with lo, hi =
 *   1 -+ range (hue: -+ range) in fp32, the difference, the product and the sum each rounded on their own.  Order: q =
 *   mulhi(word, 24), a Lehmer code over [brightness, contrast, saturation, hue]: q / 6, then (q % 6) / 2, then q % 2, each picking
 *   from what is left; the last operation is the one left over.
 *   mean: computed iff the object's contrast factor is not exactly 1 (else 0).  m = the mean over ALL NV * H * W pixels of the
 *   object of gray(T<(x)), x = float(b) / 255.0f per channel, T< the chain of the operations that precede contrast in the
 *   record's order.  One value per object, not per view: an object's views share ONE colour map, so source and target views stay
 *   photo-consistent.  The fp32 greys are summed in fp64 in a fixed order — per workgroup the partial of a block of
 *   PNR_JITTER_BLOCK consecutive pixels, then one fold per object — divided by the count in fp64 and rounded once to fp32.  No
 *   atomics: the same bytes give the same bits; one object's bytes do not enter another's record.  With ranges[1] == 0 no
 *   reduction is launched and neither images_u8 nor workspace is looked at.
 *   ranges: HOST array of 4 (brightness, contrast, saturation, hue).  workspace: pnr_color_jitter_workspace_bytes(SB, NV, W, H)
 *   bytes, 8-byte aligned (0 bytes for sizes the plan refuses).
 *   PNR_E_NULL       ranges or record_out NULL; images_u8 or workspace NULL with ranges[1] != 0
 *   PNR_E_SHAPE      a brightness, contrast or saturation range outside [0, 1], a hue range outside [0, 0.5], C not 3 or 4, or
 *                    the size conditions of pnr_train_batch_u8 (SB, NV, W, H < 1, NV * H * W >= 2^31); more blocks than one launch
 *   PNR_E_ALIGN      workspace not 8-byte aligned;  PNR_E_WORKSPACE  ws_bytes too small
 *
 * The chain, y = chain(x) on one pixel x = (r, g, b) in [0, 1].  Every fp32 operation is rounded on its own; clamp is to [0, 1];
 * the operations run in the record's order; an operation whose factor is exactly its identity (1, 1, 1, hue 0) is skipped, so an
 * identity record gives the bits of the entry points without a record.
 *   gray(x)        (0.2989f r + 0.587f g) + 0.114f b
 *   brightness f   clamp(f x)
 *   contrast f     clamp(f x + (1 - f) m), m the record's mean, 1 - f rounded once
 *   saturation f   clamp(f x + (1 - f) gray(x))
 *   hue h          RGB -> HSV: maxc, minc, eq = (maxc == minc); s = (maxc - minc) / (eq ? 1 : maxc); d = eq ? 1 : maxc - minc;
 *                  rc = (maxc - r) / d, gc and bc alike; H = [maxc == r] (bc - gc) + [maxc == g and maxc != r] ((2 + rc) - bc) +
 *                  [maxc != g and maxc != r] ((4 + gc) - rc); H = fmod(H / 6 + 1, 1); v = maxc.
 *                  shift: t = H + h; H' = t - floor(t); a result of 1.0f becomes 0.0f.
 *                  HSV -> RGB: i = floor(6 H'), f = 6 H' - i, i mod 6; p = clamp(v (1 - s)), q = clamp(v (1 - s f)),
 *                  t = clamp(v (1 - s (1 - f))); (r, g, b) = (v,t,p), (q,v,p), (p,v,t), (p,q,v), (t,p,v), (v,p,q) for i = 0..5.
 *
 * pnr_train_batch_u8_jitter / pnr_views_to_tensor_u8_jitter: pnr_train_batch_u8 / pnr_views_to_tensor_u8 with the record
 * `jitter` (SB, 8) (one kernel body each, the chain compiled in).  Per selected pixel x = float(b) / 255.0f, y = chain(x) under
 * the pixel's object's record, then the existing map on y: balanced (y - 0.5f) / 0.5f, and 0.5f T + 0.5f for rgb_gt.  Rays, NaN
 * rows and planes for bad indices, checks and return codes are those of the entry points without a record; PNR_E_NULL also for
 * jitter NULL.  The record is device data and is never read on the host: the chain indexes no memory, so any record is safe. */
#define PNR_JITTER_BLOCK 4096    /* pixels per partial sum of pnr_color_jitter_plan's mean */
uint64_t pnr_color_jitter_workspace_bytes(int32_t SB, int32_t NV, int32_t W, int32_t H);
int32_t pnr_color_jitter_plan(const uint8_t* images_u8 /* (SB, NV, H, W, C), any byte alignment */, int32_t SB, int32_t NV, int32_t W,
                              int32_t H, int32_t C, const float* ranges /* HOST, 4 */, uint64_t seed,
                              float* record_out /* (SB, 8) */, void* workspace, uint64_t ws_bytes, void* stream);
int32_t pnr_train_batch_u8_jitter(const uint8_t* images_u8, const float* poses, const float* focal, const float* c, int32_t SB,
                                  int32_t NV, int32_t W, int32_t H, float z_near, float z_far, const int64_t* pix_inds, int64_t B,
                                  float* rays_out, float* rgb_gt_out, int32_t C, int32_t balanced,
                                  const float* jitter /* (SB, 8) */, void* stream);
int32_t pnr_views_to_tensor_u8_jitter(const uint8_t* images_u8, const int64_t* view_ord, int32_t SB, int32_t NV, int32_t NS,
                                      int32_t W, int32_t H, int32_t C, int32_t balanced, float* out,
                                      const float* jitter /* (SB, 8) */, void* stream);
/* pnr_color_jitter_plan_at: the plan of a SLICE of a step's batch.  The call's object o is object obj_base + o of the step: its
 * record is drawn with the counter (lo32(obj_base + o), hi32(obj_base + o), 10, block), everything else — the bytes read, the
 * grey mean (which depends on the object's bytes and its record alone), the row written — is the call's own object o.  The
 * records of objects [k, k + m) under obj_base = k are therefore rows k .. k + m - 1 of the whole batch's plan, bit for bit.
 * pnr_color_jitter_plan is this call with obj_base 0.  Checks and codes as above, and
 *   PNR_E_SHAPE  obj_base < 0 or obj_base + SB past int64 */
int32_t pnr_color_jitter_plan_at(const uint8_t* images_u8, int32_t SB, int32_t NV, int32_t W, int32_t H, int32_t C,
                                 const float* ranges /* HOST, 4 */, uint64_t seed, int64_t obj_base, float* record_out /* (SB, 8) */,
                                 void* workspace, uint64_t ws_bytes, void* stream);

/* ---- training draws on the device, csrc/train_draw.hip ---------------------------------------------------------------------------
 * pnr_train_draw: the pixels a training step samples and the source views it encodes (train/train.py:268-300: per object
 * np.random.choice for the views, util.bbox_sample or a uniform randint for the pixels), drawn by one launch of SB * B + SB work
 * items from philox4x32 keyed by `seed` — the caller's per-step key — so a step's batch depends on (seed) alone and a resumed run
 * sees the batches the uninterrupted run would have.  The outputs are the index buffers pnr_train_batch, pnr_train_batch_u8 and
 * pnr_views_to_tensor_u8 take.  All arithmetic is integer; mulhi(x, n) = (uint64(x) * n) >> 32, a value in [0, n).  Draw ids
 * 8 (pixels) and 9 (views) — 0..3 are the render samplers' — in the counter layout of the samplers: key = (seed lo32, seed hi32),
 * counter = (index lo32, index hi32, draw id, block).
 *
 * Pixel (o, j), r = o * B + j:  (x, y, z, _) = philox4x32(seed, lo32(r), hi32(r), 8, 0);  view = mulhi(x, NV).
 *   without boxes (bbox NULL)   col = mulhi(y, W), row = mulhi(z, H)
 *   with boxes                  (cmin, rmin, cmax, rmax) = the four floats of bbox[o, view] truncated towards zero; the box is
 *                               valid iff all four are finite and 0 <= cmin <= cmax < W and 0 <= rmin <= rmax < H;
 *                               col = cmin + mulhi(y, cmax + 1 - cmin), row = rmin + mulhi(z, rmax + 1 - rmin)
 *   pix_inds_out[o, j] = view * H * W + row * W + col; -1 for an invalid box, which pnr_train_batch turns into a NaN row.  The
 *   boxes are never read on the host, so this kernel is their range check; it reads nothing else.
 * Views of object o (NS <= NV, NS <= 64), s = 0 .. NS - 1 in order: word_s = word s & 3 of philox4x32(seed, lo32(o), hi32(o), 9,
 *   s >> 2); t = mulhi(word_s, NV - s); walk the views chosen so far in ascending order and increment t for each chosen c with
 *   t >= c; view_ord_out[o, s] = t.  A uniformly random ordered subset, with no NV-sized array.
 *
 * Deliberately not the reference's stream, only its distribution (a uniform view, then a uniform cell of its box): without boxes
 * view, row and column are drawn separately instead of one randint(NV * H * W), and the reference's float form
 * rand * (cmax + 1 - cmin) + cmin can round up to cmax + 1 where the integer form cannot.
 *   PNR_E_SHAPE  NS < 0, NS > 64, NS > NV, or pnr_train_batch's size conditions (SB, NV, W, H < 1, B < 0, NV * H * W >= 2^31,
 *                more work items than one launch holds)
 *   PNR_E_NULL   pix_inds_out NULL with B > 0, view_ord_out NULL with NS > 0
 *   B == 0 and NS == 0 returns 0 and launches nothing */
int32_t pnr_train_draw(const float* bbox /* (SB, NV, 4) cmin rmin cmax rmax, or NULL */, int32_t SB, int32_t NV, int32_t W,
                       int32_t H, int64_t B, int32_t NS, uint64_t seed, int64_t* pix_inds_out /* (SB, B) */,
                       int64_t* view_ord_out /* (SB, NS), NULL iff NS == 0 */, void* stream);
/* pnr_train_draw_at: the draws of a SLICE of a step's batch, for a step whose objects are split over several callers (the ranks
 * of a data-parallel run).  The call's object o is object obj_base + o of the step and only the counters see it:
 *   pixel (o, j)        r = (obj_base + o) * B + j, an int64, in place of o * B + j
 *   views of object o   counter index obj_base + o in place of o
 * bbox, pix_inds_out and view_ord_out are the call's own SB rows.  The outputs of objects [k, k + m) under obj_base = k are rows
 * k .. k + m - 1 of the whole batch's call, bit for bit; pnr_train_draw is this call with obj_base 0.  Checks and codes as above, and
 *   PNR_E_SHAPE  obj_base < 0, or obj_base + SB or (obj_base + SB) * B past int64 */
int32_t pnr_train_draw_at(const float* bbox, int32_t SB, int32_t NV, int32_t W, int32_t H, int64_t B, int32_t NS, uint64_t seed,
                          int64_t obj_base, int64_t* pix_inds_out, int64_t* view_ord_out, void* stream);

/* ---- mask-weighted training draws on the device, csrc/mask_draw.hip ----------------------------------------------------------------
 * The reference's other pixel sampler, util.masked_sample(masks, num_pix, prop_inside, thresh) (util/util.py:210-222): a fixed
 * share of an object's rays falls on its foreground, the rest on its background, each uniform over ALL views' pixels of that
 * kind.  Here: a bit table per object, built once (pnr_mask_table_build), and the step's draws from it keyed like
 * pnr_train_draw's (pnr_train_draw_masked).  All arithmetic is integer; no atomics; nothing is allocated or read back; every
 * check runs before any launch.
 *
 * pnr_mask_table_build.  Pixel p = (view * H + row) * W + col of object n has its mask byte at
 * masks_u8[(n * NV * H * W + p) * pix_stride] — pix_stride 1 reads a mask plane, pix_stride 4 with the pointer advanced by 3 an
 * alpha channel where it lies; any byte alignment.  A pixel is INSIDE iff byte >= thresh, thresh in 1..255 (128: b / 255 >= 0.5,
 * the reference's thresh = 0.5 on a float mask).  With Wd = ceil(W / 32) and R = NV * H:
 *   bits_out (N, R, Wd) uint32   bit (col & 31) of word (col >> 5) of row (view * H + row) is set iff the pixel is inside — LSB
 *                                first; the bits at col >= W are ZERO
 *   rows_out (N, R + 1) uint32   rows[0] = 0, rows[r + 1] = rows[r] + popcount(row r): rows[R] is the object's inside count, and
 *                                the outside count before row r is r * W - rows[r], so one prefix serves both populations
 *   PNR_E_NULL   masks_u8, bits_out or rows_out NULL
 *   PNR_E_SHAPE  N, NV, H or W < 1, NV * H * W >= 2^31, pix_stride < 1, thresh outside 1..255
 *   PNR_E_ALIGN  bits_out or rows_out not 4-byte aligned
 *
 * pnr_train_draw_masked_at.  The VIEWS are pnr_train_draw_at's own (draw id 9, the same device function): view_ord_out equals
 * it bit for bit for the same seed, NV, NS and obj_base.  The PIXELS use draw id 11 (0..3 the render samplers', 8 and 9
 * pnr_train_draw's, 10 the colour jitter's; 4..7 stay free for the render path):
 *   pixel (o, j), r = (obj_base + o) * B + j:  (x, _, _, _) = philox4x32(seed, lo32(r), hi32(r), 11, 0)
 *   n_in = rows[o, R], n_out = R * W - n_in.  Slot j < B_inside draws from the inside population, slot j >= B_inside from the
 *   outside population; a slot whose population is EMPTY draws from the other one with the same x (both cannot be empty).  The
 *   reference's randint(0, 0) raises there; the device cannot, and a -1 row would make the optimiser skip the object's every step.
 *   k = mulhi(x, n), n the population's size; the pixel is the k-th of the population in ascending linear index p, all NV views
 *   pooled: np.flatnonzero(inside.ravel())[k], or np.flatnonzero(~inside.ravel())[k].
 *   Selection: with cum[r] = rows[o, r] (inside) or r * W - rows[o, r] (outside), both non-decreasing, the row is the LAST r in
 *   [0, R) with cum[r] <= k — an upper-bound binary search over the R + 1 prefix entries; then the row's Wd words are walked with
 *   popcounts for the (k - cum[r])-th set bit.  Outside, each word is complemented; the last word is masked to its W & 31 valid
 *   bits (when W & 31 != 0), so a tail bit is a pixel of neither population.
 *   pix_inds_out[o, j] = r * W + col.  Whatever the table holds, nothing outside bits[o] / rows[o] is read (the search stays in
 *   [0, R], the walk in [0, Wd)); a bit that is not found — an inconsistent table — writes -1, a NaN row downstream.
 * B_inside is the caller's int(B * prop_inside + 0.5) (util.py:214).  pnr_train_draw_masked is the call with obj_base 0.
 *   Checks and codes of pnr_train_draw_at, and
 *   PNR_E_SHAPE  B_inside < 0 or B_inside > B
 *   PNR_E_NULL   bits or rows NULL with B > 0 */
int32_t pnr_mask_table_build(const uint8_t* masks_u8, int32_t N, int32_t NV, int32_t H, int32_t W, int64_t pix_stride, int32_t thresh,
                             uint32_t* bits_out /* (N, NV * H, ceil(W / 32)) */, uint32_t* rows_out /* (N, NV * H + 1) */,
                             void* stream);
int32_t pnr_train_draw_masked(const uint32_t* bits, const uint32_t* rows, int32_t SB, int32_t NV, int32_t W, int32_t H, int64_t B,
                              int64_t B_inside, int32_t NS, uint64_t seed, int64_t* pix_inds_out /* (SB, B) */,
                              int64_t* view_ord_out /* (SB, NS), NULL iff NS == 0 */, void* stream);
int32_t pnr_train_draw_masked_at(const uint32_t* bits, const uint32_t* rows, int32_t SB, int32_t NV, int32_t W, int32_t H, int64_t B,
                                 int64_t B_inside, int32_t NS, uint64_t seed, int64_t obj_base, int64_t* pix_inds_out,
                                 int64_t* view_ord_out, void* stream);

/* pnr_mask_gather: the ground truth of a mask loss at the step's pixels, read from the table the draws use.
 * mask_out[o, j] = 1.0f if bit (col & 31) of word (col >> 5) of row p / W of bits[o] is set, p = pix_inds[o, j], col = p % W —
 * pnr_mask_table_build's layout — else 0.0f.  An index outside [0, NV * H * W) reads nothing and writes NaN, as a row of
 * pnr_train_batch does.  Nothing outside bits[o] is read.  One launch, one thread per pixel.
 *   PNR_E_SHAPE  pnr_train_batch's size conditions (SB, NV, W, H < 1, B < 0, NV * H * W >= 2^31, SB * B past one launch)
 *   PNR_E_NULL   bits, pix_inds or mask_out NULL with B > 0
 *   PNR_E_ALIGN  bits or mask_out not 4-byte aligned, pix_inds not 8-byte aligned */
int32_t pnr_mask_gather(const uint32_t* bits /* (SB, NV * H, ceil(W / 32)) */, int32_t SB, int32_t NV, int32_t H, int32_t W,
                        const int64_t* pix_inds /* (SB, B) */, int64_t B, float* mask_out /* (SB, B) */, void* stream);

/* Mesh extraction (util/recon.py: marching_cubes, with util.gen_grid util.py:98-115 and PyMCubes behind it), csrc/mesh.hip.
 *
 * pnr_grid_points writes points [first, first + count) of the ij-indexed grid gen_grid(*zip(c1, c2, reso), ij_indexing=True):
 * linear index (i ny + j) nz + k, coordinate = np.linspace(lo, hi, n, dtype=float32)[index] bit for bit (step = (hi - lo) /
 * (n - 1) in fp64, index * step + lo in fp64 unfused, the last sample hi itself, ONE rounding to fp32).  With fake_viewdirs it
 * also writes -p / |p| in fp32 (recon.py:54); a point of length 0 gets (0, 0, 0) where the reference's 0 / 0 is NaN.  c1, c2,
 * reso are HOST arrays of 3 (like c2w of pnr_gen_rays); xyz_out / viewdirs_out (count, 3) on the device.
 *   PNR_E_NULL   c1, c2, reso or xyz_out NULL; fake_viewdirs without viewdirs_out
 *   PNR_E_SHAPE  an axis < 1, 2^31 points or more, first / count negative or past the grid's end */
int32_t pnr_grid_points(const double* c1, const double* c2, const int32_t* reso, int64_t first, int64_t count,
                        int32_t fake_viewdirs, float* xyz_out, float* viewdirs_out, void* stream);

/* Marching cubes over an (nx, ny, nz) fp32 field, element p = (i ny + j) nz + k read at field[p * stride]: stride 4 and
 * field = out + 3 consume the sigma column of pnr_point_mlp's (N, 4) output where it lies.  Output sizes depend on the data,
 * so there are two calls and ONE host read between them: pnr_mc_count leaves the number of vertices and of triangles in
 * counts[0], counts[1] (device int64) and the offsets in `workspace`; the caller reads the counts, allocates, and calls
 * pnr_mc_emit with the SAME field, iso and workspace.  pnr_mc_emit guards every store against the n_vertices / n_triangles it
 * is given.
 *   inside      a grid point is inside iff (double)f >= iso; a NaN is outside
 *   vertices    one per grid edge whose two ends differ, owned by the edge's lower grid point; numbered in linear grid-point
 *               order, then by axis 0, 1, 2.  Index coordinate along the edge's axis a + t, t = (iso - fa) / (fb - fa) in fp64
 *               from the widened fp32 values; output = v * scale + origin per axis, two separately rounded fp64 operations
 *               (numpy's `vertices *= s; vertices + c1`).  origin, scale: HOST arrays of 3 doubles.
 *   triangles   per cell by the case table csrc/mc_tables.h (derived by tools/gen_mc_tables.py), ordered by linear cell index,
 *               then in table order; normals point from inside to outside, so a closed surface around an f >= iso region
 *               has positive signed volume.  (V, 3) fp64 vertices, (T, 3) int32 triangles, both on the device.
 * Integer scans in a fixed order, no atomics: the result equals a sequential walk index for index.  Every check is made
 * before any launch:
 *   PNR_E_NULL       field, workspace, counts, origin or scale NULL; vertices / triangles NULL with a count above 0
 *   PNR_E_SHAPE      an axis < 2, nx ny nz > 2^28 (5 triangles per cell stay inside int32), stride < 1, a negative count
 *   PNR_E_WORKSPACE  fewer workspace bytes than pnr_mc_workspace_bytes (about 10 per grid point; 0 for a bad shape)
 *   PNR_E_ALIGN      workspace not 16-byte aligned */
uint64_t pnr_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int32_t pnr_mc_count(const float* field, int32_t stride, int32_t nx, int32_t ny, int32_t nz, double iso,
                     void* workspace, uint64_t workspace_bytes, int64_t* counts, void* stream);
int32_t pnr_mc_emit(const float* field, int32_t stride, int32_t nx, int32_t ny, int32_t nz, double iso,
                    const double* origin, const double* scale, const void* workspace, uint64_t workspace_bytes,
                    int64_t n_vertices, int64_t n_triangles, double* vertices, int32_t* triangles, void* stream);

/* ---- training back end: what follows loss.backward() in train/train.py:375-412 (GradScaler.unscale_, clip_grad_norm_,
 * scaler.step, scaler.update) with Adam over every trainable tensor (trainlib/trainer.py:169), csrc/optim.hip ------------------
 *
 * Layout.  Gradients, exp_avg (m) and exp_avg_sq (v) each live in ONE flat fp32 buffer of n_flat floats; the parameters stay
 * where the caller's framework put them.  A device table of segments names each tensor: its parameter pointer, its offset in
 * the flat buffers (a multiple of 4, so an aligned tensor keeps 16-byte accesses) and its length.  A device table of chunks
 * cuts the segments into pieces of at most pnr_optim_chunk_elems() = 4096 elements, none straddling a segment;
 * pnr_optim_plan builds it on the host.  A segment of length 0 has no chunk: its p, m, v are not touched (a tensor without a
 * gradient this step, which torch's Adam skips too).
 *
 * Arithmetic of one element, every operation a separately rounded fp32 operation (nothing fused), IEEE square root and division:
 *     g  = (grad * inv_scale) * clip_coef
 *     m' = b1 * m + omb1 * g                       b1 = (float)beta1, omb1 = (float)(1.0 - beta1)
 *     v' = b2 * v + (omb2 * g) * g                 b2 = (float)beta2, omb2 = (float)(1.0 - beta2)
 *     p' = p - step_size * (m' / (sqrt(v') * rsqrt_bc2 + (float)eps))
 * with step_size = (float)(lr / (1 - beta1^t)) and rsqrt_bc2 = (float)(1 / sqrt(1 - beta2^t)) computed in fp64 on the device
 * from the device-resident step count t AFTER its increment: torch.optim.Adam with weight_decay = 0, amsgrad = False, in
 * another order of roundings (torch: lerp, addcmul, addcdiv).  lr, beta1, beta2, eps, max_norm are host doubles read at every
 * call, so a learning-rate schedule is a different argument.
 * Norm and clip (torch.nn.utils.clip_grad_norm_): total = sqrt(sum (grad * inv_scale)^2), the product rounded to fp32, its
 * square and the sum in fp64; clip_coef = (float)min(1, max_norm / (total + 1e-6)) in fp64; max_norm <= 0 gives 1.
 * Scaler (torch.amp.GradScaler.update), optional: `scaler` NULL means inv_scale = 1 and scale / growth_tracker are left alone.
 * Otherwise inv_scale = (float)(1.0 / (double)scale) of the scale the gradients carry, the caller having initialised
 * state->scale; then, non-finite gradients: scale *= backoff_factor, growth_tracker = 0; finite: growth_tracker + 1, and when
 * that reaches growth_interval: scale *= growth_factor (kept where the product is not finite), growth_tracker = 0.
 * Deviation from torch: a non-finite gradient (any grad * inv_scale that is Inf or NaN) skips the step WITH OR WITHOUT a
 * scaler — p, m, v and step keep their bits, skipped += 1, clip_coef = 0 — where torch without a scaler writes NaN into every
 * parameter.  grad is never written: after the call it still holds the scaled, unclipped values.
 *
 * Three launches on `stream`, no floating-point atomics, no host read (csrc/optim.hip): per chunk an fp64 partial and a
 * non-finite flag into `workspace`; ONE workgroup that adds the partials (thread i of 256 the chunks i, i + 256, .. ascending,
 * then a fixed tree) and fills the state record; the update, which returns at once when found_inf is set.  The summation
 * order depends on the chunk table alone: the same inputs give the same bits.  The longest addition path of grad_norm is
 * 16 + 8 + ceil(n_chunks / 256) + 8 fp64 additions.  The update takes 16-byte loads and stores in every chunk whose parameter
 * pointer and flat offset are both 16-byte aligned and a scalar body otherwise.  The device tables are the caller's: an
 * entry that does not fit (segment index or range outside the tables / n_flat) is skipped, nothing else is verified.
 * Every check is made before any launch:
 *   PNR_E_SHAPE      n_segments, n_chunks or n_flat negative, n_chunks >= 2^31; chunks without segments or flat floats;
 *                    scaler->growth_interval < 1
 *   PNR_E_NULL       state NULL; with n_chunks > 0: segments, chunks, grad, exp_avg, exp_avg_sq or workspace NULL
 *   PNR_E_WORKSPACE  fewer workspace bytes than pnr_optim_workspace_bytes (12 per chunk, each part rounded up to 16; 0 for a
 *                    count that is negative or too large)
 *   PNR_E_ALIGN      grad, exp_avg, exp_avg_sq or workspace not 16-byte aligned; state, segments or chunks not 8-byte aligned
 * n_chunks == 0 (no tensor has a gradient) returns PNR_OK without a launch: nothing moves, as in torch. */
typedef struct pnr_optim_state {     /* device record, 56 bytes; the caller zeroes it once (and sets `scale` with a scaler) */
    double grad_norm;                /* total of the last call, Inf / NaN included */
    float clip_coef;                 /* applied by the last call; 0 on a skipped step */
    float scale;                     /* GradScaler's scale, AFTER the last call's update */
    float inv_scale;                 /* what the last call multiplied the gradients by */
    int32_t found_inf;               /* 1: the last call skipped */
    int32_t growth_tracker;
    int32_t reserved0;
    int64_t step;                    /* t: applied steps */
    int64_t skipped;                 /* skipped steps */
    float step_size;                 /* of the last applied step */
    float rsqrt_bc2;
} pnr_optim_state;
typedef struct pnr_optim_segment { float* param; int64_t offset; int64_t n; } pnr_optim_segment;          /* device table */
typedef struct pnr_optim_chunk { int32_t segment; int32_t reserved; int64_t first; } pnr_optim_chunk;     /* device table: elements
                                                                                                           * [first, first + 4096) of the segment, cut at its end */
typedef struct pnr_optim_scaler { float growth_factor; float backoff_factor; int32_t growth_interval; int32_t reserved; } pnr_optim_scaler;   /* host */

int32_t pnr_optim_chunk_elems(void);
/* Host only.  Writes the chunk table of segments of seg_n[0 .. n_segments) elements, in ascending (segment, first) order, into
 * chunks_out (a HOST array of max_chunks entries, or NULL to count) and returns the number of chunks the table needs — entries
 * past max_chunks are counted, not written.  PNR_E_SHAPE for a negative count or length, PNR_E_NULL for seg_n NULL. */
int64_t pnr_optim_plan(const int64_t* seg_n, int32_t n_segments, pnr_optim_chunk* chunks_out, int64_t max_chunks);
uint64_t pnr_optim_workspace_bytes(int64_t n_chunks);
int32_t pnr_adam_step(const pnr_optim_segment* segments, int32_t n_segments, const pnr_optim_chunk* chunks, int64_t n_chunks,
                      const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat,
                      double lr, double beta1, double beta2, double eps, double max_norm,
                      const pnr_optim_scaler* scaler /* host, or NULL */, pnr_optim_state* state,
                      void* workspace, uint64_t workspace_bytes, void* stream);
/* pnr_adam_step_div: the step of a gradient buffer that holds the SUM over grad_div ranks (one all-reduce over the flat buffer)
 * where the mean is meant.  With inv_div = 1.0f / (float)grad_div, rounded once on the host, the gradient enters everything as
 *     u = (grad * inv_scale) * inv_div            two separately rounded fp32 products
 * the norm is sqrt(sum u^2), found_inf is set by a non-finite u, and g = u * clip_coef in the element's arithmetic above: the
 * norm, the clip, the skip and the scaler see the divided gradient, and no pass over the buffer is added.  A power-of-two
 * grad_div is exact (short of underflow): the step on 2 g with grad_div 2 is the step on g, bit for bit.  grad_div == 1 runs the
 * kernels WITHOUT the second product — pnr_adam_step is this call with grad_div 1 and keeps its bits.  Checks and codes as
 * above, and
 *   PNR_E_SHAPE  grad_div < 1 */
int32_t pnr_adam_step_div(const pnr_optim_segment* segments, int32_t n_segments, const pnr_optim_chunk* chunks, int64_t n_chunks,
                          const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n_flat,
                          double lr, double beta1, double beta2, double eps, double max_norm,
                          const pnr_optim_scaler* scaler /* host, or NULL */, int32_t grad_div, pnr_optim_state* state,
                          void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- upstream pixelNeRF's latent map: the tail of its SpatialEncoder.forward, csrc/upsample.hip -------------------------------
 *
 * Every encoder level is resized to level 0's size (bilinear, align_corners=True) and the levels are concatenated along the
 * channels into ONE map of sumC = sum lat_c channels — what F.interpolate + torch.cat give, with the arithmetic written down.
 * levels / d_levels, lat_c, lat_h, lat_w are HOST arrays of n_levels entries; the level maps and the outputs live on the device.
 *
 * Position of fine index D on an axis with n_in coarse and n_out fine samples (exact integers, no rounded scale factor):
 *     n_in == 1 or n_out == 1:  i0 = 0, lam = 0
 *     otherwise:                num = D (n_in - 1);  i0 = num / (n_out - 1) (integer division);
 *                               lam = (float)(num % (n_out - 1)) / (float)(n_out - 1) (IEEE division)
 *     i1 = min(i0 + 1, n_in - 1);  mu = 1.0f - lam
 * Value, every operation a separately rounded fp32 operation (nothing fused), a, b the taps of row y0 at columns x0, x1 and
 * c, d those of row y1:
 *     top = mux a + lamx b;  bot = mux c + lamx d;  out = muy top + lamy bot
 * A level of level 0's own size comes out as a copy; a level may be larger than level 0 (the same formula).  out16 is the
 * round-to-nearest-even conversion of the fp32 value `out` holds or would hold; out, out16 or both may be asked for (one
 * launch each).  `out` is stored along W, out16 along the channels, both in whole row segments.
 *
 * Adjoint.  d_levels[l][n, c, y, x] = the sum of w g over every tap of every fine node that lands on (y, x), g the node's
 * d_out value, w = fl(wy wx) with wy in {muy, lamy} and wx in {mux, lamx} as above; where i0 == i1 both taps land on the same
 * texel and both count.  Gather form: a thread owns one texel and walks the fine nodes of its support (rows ascending,
 * columns ascending inside a row, taps y0x0, y0x1, y1x0, y1x1 inside a node), adds the products (double)w (double)g in fp64 and
 * rounds ONCE to fp32.  No floating-point atomics: the same inputs give the same bits.  Level 0 and every level of its size
 * are a slice copy.  d_levels[l] is WRITTEN (=), not accumulated; a NULL entry is skipped.  One launch per level.
 *
 * Every check is made before any launch:
 *   PNR_E_NULL         levels / d_levels, lat_c, lat_h, lat_w or d_out NULL; a levels[i] NULL; out and out16 both NULL
 *   PNR_E_SHAPE        n_levels outside 1..PNR_MAX_LEVELS; a size < 1, H or W above 32768; n_maps < 0; a level, out or d_out
 *                      of 2^31 elements or more; out16 with sumC % 8 != 0
 *   PNR_E_UNSUPPORTED  out16 with a dtype other than PNR_BF16 / PNR_F16
 *   PNR_E_ALIGN        out16 not 16-byte aligned
 * n_maps == 0 returns PNR_OK without a launch. */
int32_t pnr_upsample_concat(const float* const* levels,       /* device, (N, C_i, H_i, W_i) fp32 NCHW contiguous */
                            const int32_t* lat_c, const int32_t* lat_h, const int32_t* lat_w,
                            int32_t n_levels, int32_t n_maps  /* N */,
                            float* out,                       /* (N, sumC, H_0, W_0) fp32 NCHW, or NULL */
                            void* out16, int32_t out16_dtype, /* (N, H_0, W_0, sumC) channels-last PNR_BF16 / PNR_F16, or NULL */
                            void* stream);
int32_t pnr_upsample_concat_bwd(const float* d_out,           /* (N, sumC, H_0, W_0) */
                                const int32_t* lat_c, const int32_t* lat_h, const int32_t* lat_w,
                                int32_t n_levels, int32_t n_maps,
                                float* const* d_levels,       /* WRITTEN (=), not accumulated; a NULL entry is skipped */
                                void* stream);

/* ---- area resampling of images, csrc/resize.hip ---------------------------------------------------------------------------------
 *
 * Upstream pixelNeRF brings its float images to another image_size with F.interpolate(mode="area"), which is
 * adaptive_avg_pool2d: a target sample is the mean of the source samples under its window.  This text is the specification.
 *
 * Window of target index i on an axis with n_in source and n_out target samples, ALL in integer arithmetic (64-bit products):
 *     lo(i) = floor(i n_in / n_out),   hi(i) = ceil((i + 1) n_in / n_out),   source indices lo(i) .. hi(i) - 1
 * A window is never empty and never leaves the axis.  Windows overlap when n_in / n_out is not an integer; n_out > n_in
 * (upsampling: windows of one or two samples) and n_out == n_in (every window is its own sample: a copy) are ordinary cases,
 * not special paths.  The window of a pixel is rows lo(y) .. hi(y) - 1 (H, Ht) by columns lo(x) .. hi(x) - 1 (W, Wt), n pixels.
 *
 * pnr_resize_area_u8: interleaved bytes (F, H, W, C) -> (F, Ht, Wt, C), C = 1..4, every channel kept and treated alike.
 *     S = the exact integer sum of the window's n bytes of that channel;  out = (2 S + n) / (2 n), integer division:
 *     the exact mean rounded to the nearest byte, a tie (fraction exactly .5) rounded UP.  An all-255 window gives 255.
 *   Accumulator: 64 unsigned bits.  S <= 255 n < 2^39 and 2 S + n < 2^41 for every window the size checks admit (n <= H W <
 *   2^31), so no admitted shape can overflow it.
 *   Frame f of the input starts at in_u8 + f in_stride, of the output at out_u8 + f out_stride (BYTES; a dense stack has the
 *   strides H W C and Ht Wt C), so a view is written straight into its slot of a pool; inside a frame both are dense.  Both
 *   may start at ANY byte; loads and stores are byte-wide.  The bytes between two output frames are not touched.  Input and
 *   output must not overlap.
 *     PNR_E_NULL   in_u8 or out_u8 NULL
 *     PNR_E_SHAPE  F, H, W, Ht or Wt < 1; H W >= 2^31 or Ht Wt >= 2^31; C outside 1..4; in_stride < H W C or out_stride <
 *                  Ht Wt C; F frames of ceil(Ht Wt / 256) workgroups each that do not fit one launch (2^31 - 1 workgroups)
 *
 * pnr_resize_area_f32: fp32 planes (F, H, W) -> (F, Ht, Wt), both dense; F counts PLANES (the caller folds views x channels).
 *     acc = 0.0 (fp64);  for every row of the window, top to bottom, for every column, left to right:  acc = acc + (double)v;
 *     out = (float)(acc / (double)n): one IEEE fp64 division, then ONE rounding to fp32 (to nearest even).
 *   A NaN or an Inf poisons exactly the windows that contain it (Inf and -Inf in one window give NaN), no other.
 *     PNR_E_NULL   in or out NULL
 *     PNR_E_SHAPE  F, H, W, Ht or Wt < 1; H W >= 2^31 or Ht Wt >= 2^31; planes x workgroups past one launch, as above
 *     PNR_E_ALIGN  in or out not 4-byte aligned
 *
 * Both are asynchronous on `stream`, make every check before the launch (one launch each), need no workspace, use no atomics
 * and read nothing back; a thread owns one target pixel and sums its window in the order above, so the same input gives the
 * same bits.  Checked on the CPU against torch's fp64 F.interpolate(mode="area") (tests/test_resize_cpu.py).  NOT pinned:
 * upstream's own loader end to end (its box and focal scaling differ on purpose: util.resize_bbox / util.resize_intrinsics). */
int32_t pnr_resize_area_u8(const uint8_t* in_u8 /* (F, H, W, C), any byte alignment */, int64_t in_stride /* bytes per frame */,
                           int32_t F, int32_t H, int32_t W, int32_t C, uint8_t* out_u8 /* (F, Ht, Wt, C), any byte alignment */,
                           int64_t out_stride /* bytes per frame */, int32_t Ht, int32_t Wt, void* stream);
int32_t pnr_resize_area_f32(const float* in /* (F, H, W) */, int32_t F, int32_t H, int32_t W, float* out /* (F, Ht, Wt) */,
                            int32_t Ht, int32_t Wt, void* stream);

/* ---- empty-space culling in front of the render launch, csrc/occupancy.hip ------------------------------------------------------
 *
 * The render launch evaluates every sample of every ray it is given.  These three calls give it fewer: a bit grid of the cells
 * of a box that hold density, each frame's rays reduced to the ORDERED list of those that pass through such a cell, with
 * [near, far] (ray columns 6:8) tightened to the occupied stretch, and the gather that puts the rendered list back into a
 * frame.  The reference has no counterpart.  This text is the specification; tests/occupancy_util.py restates it in numpy.
 *
 * The grid.  Samples on the lattice of pnr_grid_points, (nx, ny, nz), every axis >= 2; cells (cx, cy, cz) = (nx - 1, ny - 1,
 * nz - 1), cell (i, j, k) between samples i .. i + 1, j .. j + 1, k .. k + 1.  Bit k & 31 of the uint32 word
 * (i cy + j) wz + (k >> 5), wz = ceil(cz / 32), says cell (i, j, k) is occupied; the padding bits k >= cz of a last word are 0.
 *
 * pnr_occ_build: element p = (i ny + j) nz + k of the field is read at field[p * stride], as pnr_mc_count reads it.
 *     hot sample     !((double)f < thresh): f >= thresh, or f is NaN.  Conservative, the opposite of marching cubes' inside.
 *                    (thresh = -inf makes every sample hot, thresh = NaN too.)
 *     raw-occupied   a cell with at least one hot corner sample among its 8
 *     occupied       a cell with a raw-occupied cell within `dilate` cells of it in Chebyshev distance (max over the axes),
 *                    dilate = 0 .. 4; cells outside the grid do not exist
 *     accumulate     != 0: the new words are ORed into those `bits` holds (several view-direction sets, or two MLPs, as one
 *                    grid); 0: `bits` is overwritten, padding included
 *   One thread owns one word, no atomics, one launch, no workspace.
 *     PNR_E_NULL   field or bits NULL
 *     PNR_E_SHAPE  an axis < 2 or with more than 2^20 cells, stride < 1, dilate outside 0..4, 2^31 samples or words or more
 *     PNR_E_ALIGN  field or bits not 4-byte aligned
 *
 * pnr_ray_bounds: rays (n, 8) = [origin, direction, near, far], frame f = rows f R .. f R + R - 1, R = rays_per_frame, n a
 * multiple of R.  c1, c2 (the box's corners, doubles) and cells (cx, cy, cz) are HOST arrays of 3.  Host side, per axis a:
 *     lo = (float)c1, hi = (float)c2, h = (float)((c2 - c1) / cells), inv_h = (float)(cells / (c2 - c1)), the quotients in
 *     fp64; pad32 = (float)pad.
 * Per ray, ALL in fp32, every operation rounded on its own (no fused multiply-add), division IEEE; min(a, b) is "b if b < a
 * else a" and max(a, b) is "b if b > a else a" (so the sign of a zero is settled too):
 *   1. miss if any of the 8 values is NaN or Inf, if the direction is (0, 0, 0), or if near > far.
 *   2. t0 = near, t1 = far.  For a = 0, 1, 2 in this order: if d_a == 0 then miss if o_a < lo_a or o_a > hi_a; else
 *      ta = (lo_a - o_a) / d_a, tb = (hi_a - o_a) / d_a, t0 = max(t0, min(ta, tb)), t1 = min(t1, max(ta, tb)).
 *      Miss if t0 > t1 (t0 == t1, a ray that touches the box, goes on).
 *   3. Start cell, per axis: p = o_a + t0 * d_a;  f = floor((p - lo_a) * inv_h_a);  f = min(cells_a - 1, max(0, f));  c_a = (int)f.
 *      step_a = +1 / -1 / 0 by the sign of d_a.  Boundary b (0 .. cells_a) of an axis lies at B(b) = hi_a for b == cells_a,
 *      else lo_a + (float)b * h_a.  tmax_a = +inf for step_a == 0, else (B(c_a + (step_a > 0 ? 1 : 0)) - o_a) / d_a —
 *      recomputed from the boundary index at every step, never accumulated.
 *   4. hit = false, t_cur = t0.  At most cx + cy + cz + 3 times (a walk changes one index by one per step and cannot be longer;
 *      the bound holds whatever the floating-point values are):
 *        tm = min(min(tmax_0, tmax_1), tmax_2);  te = max(min(tm, t1), t_cur)
 *        if cell c is occupied: on the first such cell t_in = t_cur and hit = true; t_out = te
 *        stop unless tm < t1
 *        axis = 0 if tmax_0 <= tmax_1 and tmax_0 <= tmax_2, else 1 if tmax_1 <= tmax_2, else 2
 *        c_axis += step_axis; stop if it left 0 .. cells_axis - 1; tmax_axis from the new boundary; t_cur = te
 *   5. miss unless hit.  near' = max(near, t_in - pad32), far' = min(far, t_out + pad32).
 * So a ray hits iff its clipped segment passes through an occupied cell; t_in is the entry parameter of the first and t_out
 * the exit parameter of the last one.  Outputs, per frame f with count_f hits:
 *     rays_out (n, 8)   rows f R .. f R + count_f - 1: the hit rays in ASCENDING ray order, columns 0:6 copied, 6:8 =
 *                       (near', far'); the rows past the count are not written.  Must not overlap `rays`.
 *     slot_out (n)      int32: ray i's position in its frame's list, or -1
 *     counts_out (F)    int64, F = n / R
 * The order comes from integer scans in a fixed order, as in mesh.hip, no atomics: the result equals a sequential walk over the
 * rays.  Three launches, nothing read back.  n == 0 returns PNR_OK without a launch.  Every check is made before any launch:
 *     PNR_E_NULL       any pointer NULL
 *     PNR_E_SHAPE      n < 0 or >= 2^31, R < 1, n not a multiple of R, too many workgroups for one launch; a cell count < 1 or
 *                      > 2^20, 2^31 words or more; c1 / c2 not finite, or a box or cell that does not survive the rounding
 *                      to fp32 (hi <= lo, h <= 0, inv_h not finite); pad negative, NaN or Inf
 *     PNR_E_WORKSPACE  fewer workspace bytes than pnr_ray_bounds_workspace_bytes(n, R) (about 8 per ray; 0 for bad sizes)
 *     PNR_E_ALIGN      rays, rays_out or workspace not 16-byte aligned; bits, slot_out not 4-byte, counts_out not 8-byte aligned
 *
 * pnr_frame_from_hits: rec holds one record of rec_stride >= 4 floats per row, [r, g, b, depth, ...], frame f's list from row
 * f R on (what the render launch wrote for rays_out's rows f R .. f R + count_f - 1).  Pixel i of out (n rows of out_stride >=
 * 4 floats, 4 written): [bg, bg, bg, 0] where slot[i] < 0 (or >= R, which pnr_ray_bounds never writes), else the first four
 * floats of record (i / R) R + slot[i].  One thread per pixel, one launch.
 *     PNR_E_NULL   rec, slot or out NULL
 *     PNR_E_SHAPE  n, R as above; a stride < 4
 *     PNR_E_ALIGN  a pointer not 4-byte aligned */
int32_t pnr_occ_build(const float* field, int32_t stride, int32_t nx, int32_t ny, int32_t nz, double thresh, int32_t dilate,
                      int32_t accumulate, uint32_t* bits, void* stream);
uint64_t pnr_ray_bounds_workspace_bytes(int64_t n, int64_t rays_per_frame);
int32_t pnr_ray_bounds(const float* rays, int64_t n, int64_t rays_per_frame, const double* c1, const double* c2,
                       const int32_t* cells, const uint32_t* bits, double pad, void* workspace, uint64_t workspace_bytes,
                       float* rays_out, int32_t* slot_out, int64_t* counts_out, void* stream);
int32_t pnr_frame_from_hits(const float* rec, int32_t rec_stride, const int32_t* slot, int64_t n, int64_t rays_per_frame, float bg,
                            float* out, int32_t out_stride, void* stream);

/* ---- procedural datasets: analytic shapes ray-cast into SRN-form frames, csrc/synth.hip ------------------------------------------
 *
 * A data source that needs no files: objects made of a few ellipsoids and boxes, ray-cast exactly into the bytes an SRN folder
 * would hold (white background, mask = "no channel is 255"), with the ground-truth depth.  The reference's counterpart is
 * scripts/render_shapenet.py (Blender over ShapeNet); nothing of it is restated here.  This text is the specification;
 * tests/synth_util.py restates it in numpy.
 *
 * Scenes.  scenes (n_scenes, P, PNR_SYNTH_REC) floats, P <= PNR_SYNTH_MAX_PRIMS.  One record per primitive:
 *     [0]      kind: 0 = none, 1 = ellipsoid, 2 = box (compared as floats; any other value is none)
 *     [1:4]    centre c
 *     [4:13]   R, world -> local rotation, row major: local = R (world - c)
 *     [13:16]  half-extents h (semi-axes of the ellipsoid, half edge lengths of the box), > 0
 *     [16:19]  albedo
 *     [19]     padding
 * Frames.  Frame f shows scene scene_ids[f] (int32; an index outside [0, n_scenes) gives a background frame: the kernel is the
 * range check) from poses[f], a row-major 4 x 4 camera-to-world matrix in the convention of pnr_gen_rays (x right, y up, the
 * camera looks down -z): C = its upper-left 3 x 3, o = its last column.
 *
 * ALL in fp32, every product, sum, quotient and square root rounded on its own (no fused multiply-add), division and square
 * root IEEE.  dot(a, b) = (a0 b0 + a1 b1) + a2 b2.  Sub-sample (a, b), a, b = 0 .. ss - 1, of pixel (row, col):
 *   1. x = (float)col + off_a, y = (float)row + off_b, off_k = (k + 0.5) / ss - 0.5 (exact).  u = (x - cx) / fx,
 *      v = -((y - cy) / fy), len = sqrt((u u + v v) + 1), dc = (u / len, v / len, -1 / len), d_i = dot(C_i, dc) (C_i = row i).
 *      With ss = 1 this is pnr_gen_rays' pixel, without a half-pixel shift.
 *   2. Per primitive p = 0 .. P - 1 that is not none: q = o - c, ol_i = dot(R_i, q), dl_i = dot(R_i, d).
 *      ellipsoid:  tc = -dot(ol, dl), os_i = ol_i + tc dl_i: the origin moved along the ray to the primitive's side, so that B
 *                  below is small and the discriminant does not cancel.  oe_i = os_i / h_i, de_i = dl_i / h_i (the unit sphere);
 *                  A = dot(de, de), B = dot(oe, de), Cq = dot(oe, oe) - 1; disc = B B - A Cq; a hit needs disc > 0;
 *                  tp = (-B - sqrt(disc)) / A (the smaller root), t = tc + tp; a hit needs t > 0.
 *      box:        tn = -inf, tf = +inf, face = 0.  For a = 0, 1, 2 in this order: if dl_a == 0 the axis contributes no bound
 *                  and the primitive is missed iff |ol_a| > h_a; else t1 = (-h_a - ol_a) / dl_a, t2 = (h_a - ol_a) / dl_a,
 *                  lo = t2 if t2 < t1 else t1, hi = t2 if t2 > t1 else t1; if lo > tn then tn = lo and face = a; if hi < tf
 *                  then tf = hi.  A hit needs tn < tf and tn > 0; t = tn.
 *      The hit with the smallest t wins; best starts at +inf and is replaced only by t < best, so a tie goes to the lower index
 *      and a NaN or Inf never wins.
 *   3. Normal of the winner.  ellipsoid: g_i = (oe_i + tp de_i) / h_i, m_j = (R_0j g_0 + R_1j g_1) + R_2j g_2,
 *      n = m / sqrt(dot(m, m)).  box: s = -1 if dl_face > 0 else 1, n_j = R_face,j s.
 *   4. k = dot(n, l); k = k if k > 0 else 0; shade = ambient + one_minus k; colour_c = albedo_c shade.  A miss has colour 1.
 *      Host side: l = (float)(light / |light|) with the norm and the quotient in fp64, one_minus = 1.0f - ambient in fp32.
 * Per pixel: acc_c = 0, then acc_c = acc_c + colour_c over the sub-samples in the order b = 0 .. ss - 1 (outer), a = 0 .. ss - 1
 * (inner); mean_c = acc_c inv, inv = 1 / ss^2 (a power of two); w = mean_c 255 + 0.5; byte = 0 unless w > 0, 255 for w >= 255,
 * else (int)floor(w).  If any sub-sample hit: mask = 255 and every channel byte = min(byte, 254).  If none hit the bytes are
 * 255, 255, 255 and the mask is 0.  So SRNDataset's rule mask = (img != 255).all(-1) reads the mask back from the bytes.
 * depth = t of the FIRST sub-sample (a = b = 0; the pixel centre for ss = 1) when that one hit, else +inf; t is the parameter
 * along d, which has unit length to fp32 rounding.
 *
 * Outputs.  rgb_out: frame f at rgb_out + f rgb_frame_stride bytes, (H, W, 3) bytes interleaved; rgb_frame_stride >= 3 H W (a
 * pool slot, or a margin between frames); nothing outside the frames' 3 H W bytes is written.  mask_out (F, H, W) bytes and
 * depth_out (F, H, W) floats are dense and optional (NULL).  One workgroup covers a run of 256 pixels of one frame and loads
 * the scene's records (and ol) once; a thread owns four neighbouring pixels and writes their 12 colour bytes as three dwords
 * where the address is 4-byte aligned and the four pixels exist, else byte by byte.  One launch, no atomics, no workspace.
 *     PNR_E_NULL   scenes, scene_ids, poses or rgb_out NULL
 *     PNR_E_SHAPE  n_scenes < 0, P < 1 or P > PNR_SYNTH_MAX_PRIMS, F, W or H < 1, F H W >= 2^31, F ceil(H W / 256) >= 2^26 (the
 *                  threads of one launch), rgb_frame_stride < 3 H W,
 *                  ss not 1, 2 or 4, fx or fy zero or not finite, cx or cy not finite, ambient outside [0, 1] (NaN included),
 *                  a light vector that is zero or not finite
 *     PNR_E_ALIGN  scenes, scene_ids, poses or depth_out not 4-byte aligned */
#define PNR_SYNTH_MAX_PRIMS 8
#define PNR_SYNTH_REC 20
int32_t pnr_synth_render(const float* scenes, int32_t n_scenes, int32_t P, const int32_t* scene_ids, const float* poses, int32_t F,
                         int32_t W, int32_t H, float fx, float fy, float cx, float cy, int32_t ss, float ambient, float light_x,
                         float light_y, float light_z, uint8_t* rgb_out, int64_t rgb_frame_stride, uint8_t* mask_out,
                         float* depth_out, void* stream);

/* Timing hook for bench.py: microseconds between the first and last point-MLP launch of the most recent
 * pnr_render on this thread is NOT kept (no global state); instead the caller brackets calls with
 * hipEvents on `stream`.  These two helpers expose hipEvent timing on an arbitrary hipStream_t to
 * ctypes callers (torch.cuda.Event only sees torch's current stream). */
int32_t pnr_event_create(void** ev);
int32_t pnr_event_record(void* ev, void* stream);
int32_t pnr_event_elapsed_ms(void* start, void* stop, float* ms);   /* synchronises on `stop` */
int32_t pnr_event_destroy(void* ev);

/* Diagnostics of the tile GEMMs behind the fp32 path and the training path (host functions, no device work): size of their
 * 1-D launch grid, and the tile a workgroup id maps to — (m tile, n tile, reduction split) in out3, return 1, or 0 for a
 * padding workgroup of the rounded-up grid.  The order is XCD-aware: workgroup ids go round the 8 XCDs, and the tiles that
 * share an operand take consecutive slots of ONE XCD (tests/test_host_cpu.py checks the bijection and that property). */
int64_t pnr_debug_gemm_grid(int32_t M, int32_t N, int32_t Rn, int32_t rows_per_split, int32_t split);
int32_t pnr_debug_gemm_tile(int32_t block, int32_t M, int32_t N, int32_t Rn, int32_t rows_per_split, int32_t split,
                            int32_t* out3);

/* Diagnostic of the fused point kernel's launch (csrc/point_mfma.hip point_split; a host function, no device work): how a call's
 * work is split over workgroups.  max_wgs: the workgroup cap (the device's CUs, at most 512); n_stream_objs: objects with a
 * projected weight stream of their own (<= 1: none — workgroups then share the whole call); K: 0 for a plain point launch,
 * whose workgroups own runs of 128-point tiles, or the samples per ray of a fused render launch, whose workgroups own whole
 * rays; count: the call's points (K = 0) or rays; per_obj: one object's points or rays (read with n_stream_objs > 1 only).
 * out4 = (grid, tiles_per_wg, rays_per_wg, wgs_per_obj); returns PNR_OK, or the code the launch returns for such sizes. */
int32_t pnr_debug_point_split(int32_t max_wgs, int32_t n_stream_objs, int32_t K, int64_t count, int64_t per_obj, int32_t* out4);

/* Test entry into the training path's linear-layer dispatch (csrc/train_f32.hip: gemm, gemm16, grad_w, head_dx) and its bf16
 * copy kernels: ONE product on caller-owned device buffers, chosen by the production dispatchers from the same shape,
 * alignment and operand-form predicates, asynchronous on `stream`.  The outputs say what ran: `kernel` the launch site
 * (PNR_DBG_K_*), `epilogue` the epilogue form of a forward / dX tile kernel (PNR_DBG_EPI_*), and for a weight gradient
 * `splits` / `rows_per_split` (its row slices) and `reduce` (1: k_reduce_parts, 2: k_reduce_parts2).  Operands by op:
 *   FWD      y (m, n) = mask(act(x) (m, k) . w (n, k)^T + b) + r;  act = relu if `relu`; mask keeps mk > 0 (fp32) or a bf16 mk16
 *            with the sign clear and not zero.  mode 0 / 1 / 3: gemm's fp32 / bf16 / bf16x3 products (x, mk fp32);
 *            mode PNR_DBG_MODE_TAPE16: gemm16 with any of x16, mk16, y16 (the bf16 copy of y; y may then be NULL) and
 *            w16 (w as bf16 (n, k), leading dimension k).  y16 shares ldy, x16 ldx, mk16 ldm.
 *   DX       y (m, n) = mask(x (m, k) . w (k, n));  mode 0: w16 = the fp32 (n, k) copy of w^T (gemm's Wt) or NULL;
 *            mode PNR_DBG_MODE_TAPE16: gemm16 with w16 = bf16 (n, k) copy of w^T, x16, mk16, y16 as for FWD.
 *   HEAD_DX  y (m, n) = mask(x (m, 4) . w (4, n)), y16 optional: the output head's dX kernel (its own shape limits).
 *   DW       y (n, k) += g (m, n)^T . act(x) (m, k) (ldy), db (n) += column sums of g; y and/or db may be NULL.  mode = grad_w's
 *            `half` (0, 1, 3); x16 / g16: the bf16 tape forms.  ws (ws_floats floats): the per-split partials.
 *   TO_BF16 (y16 (m) = RNE(x)), COLS_TO_BF16 (y16 (m, k) = RNE of the first k columns of x (m, ldx)),
 *   W_TO_BF16 (y16 (m, k) = RNE(x), and y16t (k, m) = its transpose unless NULL). */
enum { PNR_DBG_OP_FWD = 0, PNR_DBG_OP_DX = 1, PNR_DBG_OP_HEAD_DX = 2, PNR_DBG_OP_DW = 3, PNR_DBG_OP_TO_BF16 = 4,
       PNR_DBG_OP_COLS_TO_BF16 = 5, PNR_DBG_OP_W_TO_BF16 = 6 };
enum { PNR_DBG_MODE_TAPE16 = 16 };
enum {      /* launch sites of the dispatchers */
    PNR_DBG_K_NONE = 0,
    /* gemm */
    PNR_DBG_K_SGEMM_DMA_WT = 1, PNR_DBG_K_MGEMM_BF16X3 = 2, PNR_DBG_K_MGEMM_BF16 = 3, PNR_DBG_K_SGEMM_DMA = 4,
    PNR_DBG_K_MGEMM_F32 = 5, PNR_DBG_K_LINEAR_HEAD_512 = 6, PNR_DBG_K_LINEAR_HEAD_256 = 7, PNR_DBG_K_GEMM_F32 = 8,
    /* gemm16 */
    PNR_DBG_K_HGEMM_DMA_M16 = 9, PNR_DBG_K_HGEMM_DMA = 10, PNR_DBG_K_MGEMM_BF16_A16_M16 = 11, PNR_DBG_K_MGEMM_BF16_A16 = 12,
    PNR_DBG_K_MGEMM_BF16_M16 = 13, PNR_DBG_K_MGEMM_BF16_G16 = 14,
    /* head_dx */
    PNR_DBG_K_HEAD_DX = 15,
    /* grad_w */
    PNR_DBG_K_COL_SUMS16 = 16, PNR_DBG_K_COL_SUMS = 17, PNR_DBG_K_GRAD_W_SKINNY48 = 18, PNR_DBG_K_GRAD_W_SKINNY96 = 19,
    PNR_DBG_K_MGEMM_BF16X3_DW = 20, PNR_DBG_K_HGEMM_DMA_KT = 21, PNR_DBG_K_MGEMM_BF16_DW_A16B16 = 22,
    PNR_DBG_K_MGEMM_BF16_DW_B16 = 23, PNR_DBG_K_MGEMM_BF16_DW = 24, PNR_DBG_K_SGEMM_DMA_KT = 25, PNR_DBG_K_MGEMM_F32_DW = 26,
    PNR_DBG_K_GRAD_W_HEAD = 27, PNR_DBG_K_GRAD_W_F32 = 28,
    PNR_DBG_K_COUNT = 29
};
enum { PNR_DBG_EPI_NONE = 0, PNR_DBG_EPI_LDS = 1, PNR_DBG_EPI_LDS_C16 = 2, PNR_DBG_EPI_REG_VEC = 3, PNR_DBG_EPI_REG_ELEM = 4 };
typedef struct {
    int32_t op, mode, relu, n, k, reserved0;
    int64_t m;
    const void* x; const void* x16; const void* w; const void* w16; const float* b; const float* r; const void* mk;
    const void* mk16; void* y; void* y16; void* y16t; const float* g; const void* g16; float* db; float* ws;
    uint64_t ws_floats;
    int32_t ldx, ldw, ldr, ldm, ldy, ldg;
    int32_t kernel, epilogue, splits, rows_per_split, reduce, reserved1;      /* out */
} pnr_debug_linear_args;
int32_t pnr_debug_linear(pnr_debug_linear_args* args, void* stream);

/* The route pnr_point_mlp_bwd takes for the latent-map gradient of these maps and n_points points (host only, no launch):
 * PNR_DBG_LATG_LDS per-block partial maps in LDS + an ordered reduction (one level of at most 64 KiB that fits the device's
 * LDS), PNR_DBG_LATG_FIXED_POINT 64-bit fixed-point integer atomics (every other map), PNR_DBG_LATG_NONE nothing to do. */
enum { PNR_DBG_LATG_NONE = 0, PNR_DBG_LATG_LDS = 1, PNR_DBG_LATG_FIXED_POINT = 2 };
int32_t pnr_debug_latent_grad_route(const pnr_views* views, int64_t n_points);

#ifdef __cplusplus
}
#endif
#endif /* PNR_H */
