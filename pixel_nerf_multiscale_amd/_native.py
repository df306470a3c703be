"""
ctypes binding of libpnr_hip.so (include/pnr.h).  The library is REQUIRED: importing this module
raises if it has not been built (python -m pixel_nerf_multiscale_amd.build_native) — there is no
CPU or PyTorch fallback for the render path.
"""
import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PNR_LIB") or os.path.join(HERE, "lib", "libpnr_hip.so")   # PNR_LIB: diagnostic builds (tools/dev)

PNR_MAX_LEVELS = 5
PNR_MAX_BLOCKS = 8
PNR_VIS_MAX_SRC = 8
PNR_JITTER_BLOCK = 4096
PNR_SYNTH_MAX_PRIMS = 8
PNR_SYNTH_REC = 20
PNR_F32, PNR_BF16, PNR_F16 = 0, 1, 2
PNR_BF16X3 = 3     # training entry points only
PRECISIONS = {"fp32": PNR_F32, "f32": PNR_F32, "bf16": PNR_BF16, "fp16": PNR_F16, "f16": PNR_F16, "bf16x3": PNR_BF16X3}
COMBINE = {"average": 0, "max": 1}
PNR_ALPHA_NV2, PNR_ALPHA_OPAQUE, PNR_ALPHA_MASK = 0, 1, 2

_fp = C.c_void_p  # device pointers travel as integers


class pnr_mlp(C.Structure):
    _fields_ = [
        ("d_in", C.c_int32), ("d_latent", C.c_int32), ("d_hidden", C.c_int32), ("d_out", C.c_int32),
        ("n_blocks", C.c_int32), ("combine_layer", C.c_int32), ("combine_type", C.c_int32), ("packed_objs", C.c_int32),
        ("lin_in_w", _fp), ("lin_in_b", _fp),
        ("lin_z_w", _fp * PNR_MAX_BLOCKS), ("lin_z_b", _fp * PNR_MAX_BLOCKS),
        ("fc0_w", _fp * PNR_MAX_BLOCKS), ("fc0_b", _fp * PNR_MAX_BLOCKS),
        ("fc1_w", _fp * PNR_MAX_BLOCKS), ("fc1_b", _fp * PNR_MAX_BLOCKS),
        ("lin_out_w", _fp), ("lin_out_b", _fp),
        ("packed", _fp), ("packed_bytes", C.c_uint64), ("packed_dtype", C.c_int32), ("packed_texels", C.c_int32),
    ]


class pnr_views(C.Structure):
    _fields_ = [
        ("n_objs", C.c_int32), ("n_views", C.c_int32),
        ("w2c", _fp), ("focal", _fp), ("c", _fp),
        ("n_focal", C.c_int32), ("n_c", C.c_int32), ("n_levels", C.c_int32), ("reserved0", C.c_int32),
        ("latent", _fp * PNR_MAX_LEVELS),
        ("lat_c", C.c_int32 * PNR_MAX_LEVELS), ("lat_h", C.c_int32 * PNR_MAX_LEVELS), ("lat_w", C.c_int32 * PNR_MAX_LEVELS),
        ("latent_packed", _fp * PNR_MAX_LEVELS), ("packed_dtype", C.c_int32), ("reserved1", C.c_int32),
        ("uv_scale_x", C.c_float * PNR_MAX_LEVELS), ("uv_scale_y", C.c_float * PNR_MAX_LEVELS),
    ]


class pnr_params(C.Structure):
    _fields_ = [
        ("n_coarse", C.c_int32), ("n_fine", C.c_int32), ("n_fine_depth", C.c_int32), ("white_bkgd", C.c_int32),
        ("lindisp", C.c_int32), ("use_code_viewdirs", C.c_int32), ("num_freqs", C.c_int32), ("precision", C.c_int32),
        ("depth_std", C.c_float), ("freq_factor", C.c_float), ("train_tape_fp32", C.c_int32), ("park_fp32", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class pnr_mlp_grads(C.Structure):
    _fields_ = [
        ("lin_in_w", _fp), ("lin_in_b", _fp),
        ("lin_z_w", _fp * PNR_MAX_BLOCKS), ("lin_z_b", _fp * PNR_MAX_BLOCKS),
        ("fc0_w", _fp * PNR_MAX_BLOCKS), ("fc0_b", _fp * PNR_MAX_BLOCKS),
        ("fc1_w", _fp * PNR_MAX_BLOCKS), ("fc1_b", _fp * PNR_MAX_BLOCKS),
        ("lin_out_w", _fp), ("lin_out_b", _fp),
    ]


class pnr_noise(C.Structure):
    _fields_ = [("noise_c", _fp), ("u", _fp), ("r", _fp), ("g", _fp), ("ray_index_obj_stride", C.c_int64)]


class pnr_outputs(C.Structure):
    _fields_ = [("coarse_rgb", _fp), ("coarse_depth", _fp), ("coarse_weights", _fp), ("fine_rgb", _fp),
                ("fine_depth", _fp), ("fine_weights", _fp), ("z_coarse", _fp), ("z_fine", _fp),
                ("ev_point_begin", _fp), ("ev_point_end", _fp), ("rgb_stride", C.c_int32), ("depth_stride", C.c_int32),
                ("coarse_weights_stride", C.c_int32), ("fine_weights_stride", C.c_int32)]


class pnr_vis_pass(C.Structure):
    _fields_ = [("rgb", _fp), ("depth", _fp), ("weights", _fp), ("rgb_stride", C.c_int32), ("depth_stride", C.c_int32),
                ("weights_stride", C.c_int32), ("K", C.c_int32)]


class pnr_debug_linear_args(C.Structure):
    _fields_ = [
        ("op", C.c_int32), ("mode", C.c_int32), ("relu", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("reserved0", C.c_int32),
        ("m", C.c_int64),
        ("x", _fp), ("x16", _fp), ("w", _fp), ("w16", _fp), ("b", _fp), ("r", _fp), ("mk", _fp), ("mk16", _fp), ("y", _fp),
        ("y16", _fp), ("y16t", _fp), ("g", _fp), ("g16", _fp), ("db", _fp), ("ws", _fp), ("ws_floats", C.c_uint64),
        ("ldx", C.c_int32), ("ldw", C.c_int32), ("ldr", C.c_int32), ("ldm", C.c_int32), ("ldy", C.c_int32), ("ldg", C.c_int32),
        ("kernel", C.c_int32), ("epilogue", C.c_int32), ("splits", C.c_int32), ("rows_per_split", C.c_int32),
        ("reduce", C.c_int32), ("reserved1", C.c_int32),
    ]


class pnr_optim_state(C.Structure):
    """The optimizer's device record (56 bytes); optim.DeviceAdam views its fields as 0-dim tensors at these offsets."""
    _fields_ = [("grad_norm", C.c_double), ("clip_coef", C.c_float), ("scale", C.c_float), ("inv_scale", C.c_float),
                ("found_inf", C.c_int32), ("growth_tracker", C.c_int32), ("reserved0", C.c_int32), ("step", C.c_int64),
                ("skipped", C.c_int64), ("step_size", C.c_float), ("rsqrt_bc2", C.c_float)]


class pnr_optim_segment(C.Structure):
    _fields_ = [("param", _fp), ("offset", C.c_int64), ("n", C.c_int64)]


class pnr_optim_chunk(C.Structure):
    _fields_ = [("segment", C.c_int32), ("reserved", C.c_int32), ("first", C.c_int64)]


class pnr_optim_scaler(C.Structure):
    _fields_ = [("growth_factor", C.c_float), ("backoff_factor", C.c_float), ("growth_interval", C.c_int32),
                ("reserved", C.c_int32)]


# every symbol include/pnr.h declares: name -> (restype, argtypes)
_i32, _i64, _u64, _f = C.c_int32, C.c_int64, C.c_uint64, C.c_float
PROTOTYPES = {
    "pnr_version": (_i32, []),
    "pnr_error_string": (C.c_char_p, [_i32]),
    "pnr_packed_mlp_bytes": (_u64, [C.POINTER(pnr_mlp)]),
    "pnr_pack_mlp": (_i32, [C.POINTER(pnr_mlp), _i32, _fp, _u64, _fp]),
    "pnr_packed_mlp_projected_bytes": (_u64, [C.POINTER(pnr_mlp), C.POINTER(pnr_views)]),
    "pnr_pack_mlp_projected": (_i32, [C.POINTER(pnr_mlp), C.POINTER(pnr_views), _i32, _fp, _u64, _fp]),
    "pnr_packed_latent_bytes": (_u64, [C.POINTER(pnr_views)]),
    "pnr_pack_latents": (_i32, [C.POINTER(pnr_views), _i32, _fp, _u64, C.POINTER(C.c_uint64), _fp]),
    "pnr_sample_coarse": (_i32, [_fp, _i64, _i32, _i32, _fp, _u64, _i64, _fp, _fp]),
    "pnr_composite": (_i32, [_fp, _fp, _fp, _i64, _i32, _i32, _fp, _fp, _fp, _fp]),
    "pnr_sample_fine": (_i32, [_fp, _fp, _fp, _fp, _i64, _i32, _i32, _i32, _f, _i32, _fp, _fp, _fp, _u64, _i64, _fp, _fp]),
    "pnr_point_mlp": (_i32, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_views), _fp, _fp, _i32, _fp, _fp,
                             _i64, _i64, _fp, _fp, _u64, _fp]),
    "pnr_workspace_bytes": (_u64, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_views), _i64]),
    "pnr_render": (_i32, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_mlp), C.POINTER(pnr_views), _fp, _i64,
                          _i64, C.POINTER(pnr_noise), _u64, _i64, C.POINTER(pnr_outputs), _fp, _u64, _fp]),
    "pnr_resnetfc_workspace_bytes": (_u64, [C.POINTER(pnr_mlp), _i32]),
    "pnr_resnetfc_forward": (_i32, [C.POINTER(pnr_mlp), _fp, _i64, _i32, _i64, _fp, _fp, _u64, _fp]),
    "pnr_index_latent": (_i32, [C.POINTER(pnr_views), _fp, _i64, _i32, _fp, _fp]),
    "pnr_render_camera": (_i32, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_mlp), C.POINTER(pnr_views),
                                 C.POINTER(C.c_float), _i32, _i32, _f, _f, _f, _f, _f, _f, _i64, _i64, C.POINTER(pnr_noise), _u64,
                                 _i64, C.POINTER(pnr_outputs), _fp, _u64, _fp]),
    "pnr_train_tape_bytes": (_u64, [C.POINTER(pnr_mlp), C.POINTER(pnr_views), _i64]),
    "pnr_train_tape_bytes_for": (_u64, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_views), _i64]),
    "pnr_train_bwd_workspace_bytes": (_u64, [C.POINTER(pnr_mlp), C.POINTER(pnr_views), _i64]),
    "pnr_point_mlp_train_fwd": (_i32, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_views), _fp, _fp, _i32,
                                       _fp, _fp, _i64, _i64, _fp, _fp, _u64, _fp]),
    "pnr_point_mlp_bwd": (_i32, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_views), _fp, _fp, _i32, _fp, _fp,
                                 _i64, _i64, _fp, _fp, _fp, _u64, C.POINTER(pnr_mlp_grads), C.POINTER(C.c_void_p), _fp, _fp,
                                 _fp, _u64, _fp]),
    "pnr_train_bwd_cam_workspace_bytes": (_u64, [C.POINTER(pnr_mlp), C.POINTER(pnr_views), _i64, _i32, _i32]),
    "pnr_point_mlp_bwd_cam": (_i32, [C.POINTER(pnr_params), C.POINTER(pnr_mlp), C.POINTER(pnr_views), _fp, _fp, _i32, _fp, _fp,
                                     _i64, _i64, _fp, _fp, _fp, _u64, C.POINTER(pnr_mlp_grads), C.POINTER(C.c_void_p), _fp, _fp,
                                     _fp, _fp, _fp, _fp, _u64, _fp]),
    "pnr_composite_bwd": (_i32, [_fp, _fp, _fp, _i64, _i32, _i32, _fp, _fp, _fp, _fp, _fp, _fp]),
    "pnr_sample_fine_bwd": (_i32, [_fp, _fp, _i64, _i32, _i32, _i32, _f, _fp, _u64, _i64, _fp, _fp, _fp, _fp]),
    "pnr_gen_rays": (_i32, [C.POINTER(C.c_float), _i32, _i32, _f, _f, _f, _f, _f, _f, _i64, _i64, _fp, _fp]),
    "pnr_train_batch": (_i32, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _f, _f, _fp, _i64, _fp, _fp, _fp]),
    "pnr_rgb_loss": (_i32, [_fp, _fp, _fp, _i64, _i32, _f, _f, _fp, _fp]),
    "pnr_rgb_loss_bwd": (_i32, [_fp, _fp, _fp, _i64, _i32, _f, _f, _fp, _fp, _fp, _fp]),
    "pnr_eval_frame_workspace_bytes": (_u64, [_i32, _i32]),
    "pnr_eval_frame": (_i32, [_fp, _i32, _fp, _i32, _fp, _i32, _i32, _f, _f, _fp, _fp, _fp, _fp, _fp, _u64, _fp]),
    "pnr_eval_frames_workspace_bytes": (_u64, [_i32, _i32, _i32]),
    "pnr_eval_frames": (_i32, [_fp, _i32, _i64, _fp, _i32, _i32, _i32, _i32, _fp, _fp, _u64, _fp]),
    "pnr_eval_frames_u8_workspace_bytes": (_u64, [_i32, _i32, _i32]),
    "pnr_eval_frames_u8": (_i32, [_fp, _i32, _fp, _i32, _i32, _i32, _i32, _fp, _fp, _fp, _fp, _u64, _fp]),
    "pnr_cmap_workspace_bytes": (_u64, [_i32, _i32]),
    "pnr_cmap": (_i32, [_fp, _i32, _i32, _i32, _fp, _fp, _fp, _fp, _u64, _fp]),
    "pnr_vis_panel_workspace_bytes": (_u64, [_i32, _i32, _i32]),
    "pnr_vis_panel": (_i32, [_fp, _i32, C.POINTER(_i32), _i32, _i32, C.POINTER(pnr_vis_pass), _i32, _i32, _i32, _fp, _fp, _fp,
                             _fp, _fp, _fp, _fp, _u64, _fp]),         # src_views and passes: HOST addresses
    "pnr_video_frames": (_i32, [_fp, _i32, _i32, _i32, _i32, _fp, _fp, _fp]),
    "pnr_view_strip": (_i32, [_fp, _i32, _i32, _i32, _f, _f, _fp, _fp]),
    "pnr_image_to_tensor": (_i32, [_fp, _i32, _i32, _i32, _fp, _fp]),
    "pnr_train_batch_u8": (_i32, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _f, _f, _fp, _i64, _fp, _fp, _i32, _i32, _fp]),
    "pnr_views_to_tensor_u8": (_i32, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _fp, _fp]),
    "pnr_color_jitter_workspace_bytes": (_u64, [_i32, _i32, _i32, _i32]),
    "pnr_color_jitter_plan": (_i32, [_fp, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_float), _u64, _fp, _fp, _u64, _fp]),  # ranges: HOST
    "pnr_color_jitter_plan_at": (_i32, [_fp, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_float), _u64, _i64, _fp, _fp, _u64, _fp]),
    "pnr_train_batch_u8_jitter": (_i32, [_fp, _fp, _fp, _fp, _i32, _i32, _i32, _i32, _f, _f, _fp, _i64, _fp, _fp, _i32, _i32, _fp,
                                         _fp]),
    "pnr_views_to_tensor_u8_jitter": (_i32, [_fp, _fp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _fp, _fp, _fp]),
    "pnr_train_draw": (_i32, [_fp, _i32, _i32, _i32, _i32, _i64, _i32, _u64, _fp, _fp, _fp]),
    "pnr_train_draw_at": (_i32, [_fp, _i32, _i32, _i32, _i32, _i64, _i32, _u64, _i64, _fp, _fp, _fp]),
    "pnr_mask_table_build": (_i32, [_fp, _i32, _i32, _i32, _i32, _i64, _i32, _fp, _fp, _fp]),
    "pnr_train_draw_masked": (_i32, [_fp, _fp, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _u64, _fp, _fp, _fp]),
    "pnr_train_draw_masked_at": (_i32, [_fp, _fp, _i32, _i32, _i32, _i32, _i64, _i64, _i32, _u64, _i64, _fp, _fp, _fp]),
    "pnr_mask_gather": (_i32, [_fp, _i32, _i32, _i32, _i32, _fp, _i64, _fp, _fp]),
    "pnr_alpha_loss": (_i32, [_fp, _i32, _fp, _i32, _fp, _i64, _i32, _f, _f, _f, _f, _f, _fp, _fp, _fp]),
    "pnr_alpha_loss_bwd": (_i32, [_fp, _fp, _i64, _i32, _i32, _i32, _f, _f, _f, _f, _f, _fp, _fp, _fp, _fp]),
    "pnr_grid_points": (_i32, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), _i64, _i64, _i32, _fp, _fp, _fp]),
    "pnr_mc_workspace_bytes": (_u64, [_i32, _i32, _i32]),
    "pnr_mc_count": (_i32, [_fp, _i32, _i32, _i32, _i32, C.c_double, _fp, _u64, _fp, _fp]),
    "pnr_mc_emit": (_i32, [_fp, _i32, _i32, _i32, _i32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), _fp, _u64,
                           _i64, _i64, _fp, _fp, _fp]),
    "pnr_optim_chunk_elems": (_i32, []),
    "pnr_optim_plan": (_i64, [C.POINTER(C.c_int64), _i32, _fp, _i64]),        # chunks_out: a HOST address
    "pnr_optim_workspace_bytes": (_u64, [_i64]),
    "pnr_adam_step": (_i32, [_fp, _i32, _fp, _i64, _fp, _fp, _fp, _i64, C.c_double, C.c_double, C.c_double, C.c_double,
                             C.c_double, C.POINTER(pnr_optim_scaler), _fp, _fp, _u64, _fp]),
    "pnr_adam_step_div": (_i32, [_fp, _i32, _fp, _i64, _fp, _fp, _fp, _i64, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_double, C.POINTER(pnr_optim_scaler), _i32, _fp, _fp, _u64, _fp]),
    "pnr_upsample_concat": (_i32, [C.POINTER(C.c_void_p), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32, _fp,
                                   _fp, _i32, _fp]),                       # levels and the size arrays: HOST addresses
    "pnr_upsample_concat_bwd": (_i32, [_fp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32, _i32,
                                       C.POINTER(C.c_void_p), _fp]),
    "pnr_resize_area_u8": (_i32, [_fp, _i64, _i32, _i32, _i32, _i32, _fp, _i64, _i32, _i32, _fp]),
    "pnr_resize_area_f32": (_i32, [_fp, _i32, _i32, _i32, _fp, _i32, _i32, _fp]),
    "pnr_occ_build": (_i32, [_fp, _i32, _i32, _i32, _i32, C.c_double, _i32, _i32, _fp, _fp]),
    "pnr_ray_bounds_workspace_bytes": (_u64, [_i64, _i64]),
    "pnr_ray_bounds": (_i32, [_fp, _i64, _i64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), _fp, C.c_double,
                              _fp, _u64, _fp, _fp, _fp, _fp]),                 # c1, c2, cells: HOST arrays
    "pnr_frame_from_hits": (_i32, [_fp, _i32, _fp, _i64, _i64, _f, _fp, _i32, _fp]),
    "pnr_synth_render": (_i32, [_fp, _i32, _i32, _fp, _fp, _i32, _i32, _i32, _f, _f, _f, _f, _i32, _f, _f, _f, _f, _fp, _i64, _fp,
                                _fp, _fp]),
    "pnr_event_create": (_i32, [C.POINTER(C.c_void_p)]),
    "pnr_event_record": (_i32, [_fp, _fp]),
    "pnr_event_elapsed_ms": (_i32, [_fp, _fp, C.POINTER(C.c_float)]),
    "pnr_event_destroy": (_i32, [_fp]),
    "pnr_debug_gemm_grid": (C.c_int64, [_i32, _i32, _i32, _i32, _i32]),
    "pnr_debug_gemm_tile": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_int32)]),
    "pnr_debug_point_split": (_i32, [_i32, _i32, _i32, _i64, _i64, C.POINTER(C.c_int32)]),
    "pnr_debug_linear": (_i32, [C.POINTER(pnr_debug_linear_args), _fp]),
    "pnr_debug_latent_grad_route": (_i32, [C.POINTER(pnr_views), _i64]),
}


class Stream:
    """HIP stream handle + the ordinal of the device it belongs to.  Travels through the C ABI as the plain handle
    (`_as_parameter_`); the ordinal is what the launch guard below needs — handle 0 (the default stream) does not say
    which device it means."""
    __slots__ = ("_as_parameter_", "device")

    def __init__(self, handle, device):
        self._as_parameter_ = handle
        self.device = device


def _guarded(fn):
    """The library launches on the calling thread's CURRENT HIP device (it never calls hipSetDevice: include/pnr.h
    'Threading').  The reference picks its GPU with util.get_cuda(gpu_id) and no set_device (eval/eval.py:94), so a
    tensor may live on cuda:N while the current device is 0: every entry point that takes a stream runs under the
    stream's device."""
    def call(*args):
        s = args[-1] if args else None
        if isinstance(s, Stream) and s.device != torch.cuda.current_device():
            with torch.cuda.device(s.device):
                return fn(*args)
        return fn(*args)
    call.__name__ = getattr(fn, "__name__", "pnr_fn")
    return call


class _Lib:
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m pixel_nerf_multiscale_amd.build_native` "
            "(hipcc --offload-arch=gfx950).  The render path has no CPU/PyTorch fallback.")
    cdll = C.CDLL(LIB_PATH)
    lib = _Lib()
    lib._cdll = cdll
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(cdll, name)   # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
        takes_stream = bool(args) and args[-1] is _fp and name not in ("pnr_event_destroy",)
        setattr(lib, name, _guarded(fn) if takes_stream else fn)
    return lib


lib = _load()


class PnrError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        msg = lib.pnr_error_string(rc).decode()
        if -6 <= rc < 0:
            raise ValueError(f"{what}: {msg} (code {rc})")
        raise PnrError(f"{what}: {msg} (code {rc})")


def dptr(t):
    """Device address of a tensor of any dtype for the C ABI (None -> NULL); dtype and layout are the caller's to check."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libpnr_hip needs tensors on a HIP device (cuda:N); got a CPU tensor")
    return t.data_ptr()


def ptr(t):
    """dptr of a contiguous float32 (or uint8) tensor; written out flat, it is called several times per render."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libpnr_hip needs tensors on a HIP device (cuda:N); got a CPU tensor")
    if t.dtype != torch.float32 and t.dtype != torch.uint8:
        raise TypeError(f"expected float32 tensor, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def scratch(nbytes, device):
    """The scratch of one native call that keeps none: max(nbytes, 16) bytes.  torch's allocations are at least 256-byte
    aligned, which covers the 4- and 8-byte alignment the entry points ask for."""
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _want(dtype, shape):
    """'float32 (..., 3|4, ?, 8)': what arg and out say they wanted."""
    dims = []
    for w in shape:
        if w is ...:
            dims.append("...")
        elif w is None:
            dims.append("?")
        elif isinstance(w, tuple):
            dims.append("|".join(str(s) for s in w))
        else:
            dims.append(str(w))
    kind = "a tensor" if dtype is None else str(dtype).replace("torch.", "")
    return f"{kind} ({', '.join(dims)})"


def arg(t, name, dtype, shape, *, contiguous=False):
    """The one check of a tensor argument: dtype (None: any) and shape, a tuple whose entries are an int (exactly), None (any
    size) or a tuple of allowed sizes, behind an optional leading ... for any number of leading dimensions.  Anything else —
    no tensor at all included — is a ValueError that names the argument, what it must be and what it is.  -> t, made
    contiguous when contiguous=True.  The device is same_device's to judge, so host tensors pass."""
    # written out flat, the good case first: wrappers on the per-step path call this several times
    if isinstance(t, torch.Tensor) and (dtype is None or t.dtype == dtype):
        got = t.shape
        fits = got == shape
        if not fits:
            has_lead = len(shape) > 0 and shape[0] is ...
            dims = shape[1:] if has_lead else shape
            if has_lead and len(got) > len(dims):
                got = got[len(got) - len(dims):]
            if len(got) == len(dims):
                for s, w in zip(got, dims):
                    if w is not None and s != w and not (isinstance(w, tuple) and s in w):
                        break
                else:
                    fits = True
        if fits:
            return t.contiguous() if contiguous else t
    got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
    raise ValueError(f"{name} must be {_want(dtype, shape)}, got {got}")


def out(out, name, dtype, shape, dev):
    """The one rule of an optional output tensor (shape: a tuple): None -> a new one of this dtype and shape on dev; a given
    one must have exactly that dtype and shape and be contiguous (at any offset of a larger buffer: a pool's slot), else
    ValueError, and is returned as it is, never copied."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not isinstance(out, torch.Tensor) or out.dtype != dtype or out.shape != shape or not out.is_contiguous():
        got = f"{out.dtype} {tuple(out.shape)} strides {out.stride()}" if isinstance(out, torch.Tensor) else type(out).__name__
        raise ValueError(f"{name} must be a contiguous {_want(dtype, shape)}, got {got}")
    return out


def key64(v, name, limit=1 << 64):
    """A key or an index of the keyed kernels as a host int: 0 <= v < limit (an unsigned 64-bit seed; 1 << 63 for what
    travels as int64)."""
    v = int(v)
    if not 0 <= v < limit:
        raise ValueError(f"{name} must lie in [0, 2^{limit.bit_length() - 1}), got {v}")
    return v


def f32c(t, device=None):
    """float32 + contiguous (+ device) view/copy of t."""
    if device is not None and t.device != device:
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def current_stream(device):
    """torch's current stream on `device` for the C ABI (see Stream)."""
    device = torch.device(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    return Stream(torch.cuda.current_stream(idx).cuda_stream, idx)


def same_device(*tensors):
    """The one device all the given tensors live on; raises when they differ (the library takes raw pointers and
    cannot tell)."""
    devs = {t.device for t in tensors if t is not None}
    if len(devs) != 1:
        raise ValueError(f"tensors of one native call must share a device, got {sorted(str(d) for d in devs)}")
    dev = devs.pop()
    if dev.type != "cuda":
        raise RuntimeError("libpnr_hip needs tensors on a HIP device (cuda:N); got a CPU tensor")
    return dev
