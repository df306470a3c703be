"""The argument helpers of the Python call path (N.arg, N.out, N.key64, util._field_stride) on host tensors, and the contract
every wrapper over them keeps: what is wrong with an argument by itself is a ValueError, a well-formed host tensor is then a
RuntimeError."""
import functools

import pytest
import torch


# ------------------------------------------------------------------------------------------------------------ the helpers
def test_arg_accepts():
    from pixel_nerf_multiscale_amd import _native as N
    t = torch.zeros(2, 3, 4)
    assert N.arg(t, "t", torch.float32, (2, 3, 4)) is t                                   # an exact shape
    assert N.arg(t, "t", torch.float32, (None, 3, None)) is t                             # wildcards
    for last in (3, 4):                                                                   # a tuple of allowed sizes
        u = torch.zeros(5, last, dtype=torch.uint8)
        assert N.arg(u, "u", torch.uint8, (None, (3, 4))) is u
    for lead in ((), (7,), (7, 2)):                                                       # 0, 1 and 2 leading dimensions
        u = torch.zeros(*lead, 5, 6)
        assert N.arg(u, "u", torch.float32, (..., 5, None)) is u
    v = torch.arange(24.0).reshape(4, 6)[:, ::2]
    assert not v.is_contiguous()
    assert N.arg(v, "v", torch.float32, (4, 3)) is v                                      # untouched by default
    c = N.arg(v, "v", torch.float32, (4, 3), contiguous=True)
    assert c.is_contiguous() and torch.equal(c, v)
    assert N.arg(t, "t", torch.float32, (2, 3, 4), contiguous=True) is t                  # nothing to copy


def test_arg_refuses():
    from pixel_nerf_multiscale_amd import _native as N
    t = torch.zeros(2, 3, 4)
    bad = ((t.double(), (2, 3, 4)),                                                       # dtype
           (t, (2, 3)), (t, (2, 3, 4, 1)), (torch.zeros(4), (..., 3, 4)),                 # rank
           (t, (2, 3, 5)), (t, (..., 2, 4)),                                              # size
           (torch.zeros(2, 5), (None, (3, 4))),                                           # outside the allowed sizes
           ([[0.0]], (1, 1)), (None, (1,)))                                               # no tensor at all
    for x, shape in bad:
        with pytest.raises(ValueError, match="the_name"):
            N.arg(x, "the_name", torch.float32, shape)
    with pytest.raises(ValueError, match=r"float32 \(\.\.\., 3\|4, \?, 7\).*got torch.int64 \(2, 2\)"):    # the one wording
        N.arg(torch.zeros(2, 2, dtype=torch.long), "x", torch.float32, (..., (3, 4), None, 7))


def test_out():
    from pixel_nerf_multiscale_amd import _native as N
    o = N.out(None, "o", torch.int32, (2, 3), "cpu")
    assert o.dtype == torch.int32 and tuple(o.shape) == (2, 3) and o.device.type == "cpu"
    given = torch.empty(2, 3, dtype=torch.int32)
    assert N.out(given, "o", torch.int32, (2, 3), "cpu") is given
    slot = torch.empty(4, 2, 3, dtype=torch.int32)[2]                                     # a pool's slot: a storage offset
    assert slot.storage_offset() == 12 and N.out(slot, "o", torch.int32, (2, 3), "cpu") is slot
    for bad in (given.long(), torch.empty(3, 2, dtype=torch.int32), torch.empty(2, 6, dtype=torch.int32)[:, ::2], [[0] * 3] * 2):
        with pytest.raises(ValueError, match="the_name"):
            N.out(bad, "the_name", torch.int32, (2, 3), "cpu")
    assert not torch.empty(4, 6)[:, ::2].is_contiguous()
    with pytest.raises(ValueError):
        N.out(torch.empty(4, 6)[:, ::2], "o", torch.float32, (4, 3), "cpu")


def test_key64():
    from pixel_nerf_multiscale_amd import _native as N
    assert N.key64(0, "seed") == 0 and N.key64((1 << 64) - 1, "seed") == (1 << 64) - 1
    assert N.key64((1 << 63) - 1, "obj_base", 1 << 63) == (1 << 63) - 1
    assert N.key64(torch.tensor(5), "seed") == 5 and type(N.key64(torch.tensor(5), "seed")) is int
    for v, limit in ((-1, 1 << 64), (1 << 64, 1 << 64), (1 << 63, 1 << 63), (-1, 1 << 63)):
        with pytest.raises(ValueError, match="the_name"):
            N.key64(v, "the_name", limit)


def test_field_stride():
    from pixel_nerf_multiscale_amd import util
    assert util._field_stride(torch.zeros(2, 3, 4), "f") == 1
    rec = torch.zeros(24, 4)
    assert util._field_stride(rec[:, 3].view(2, 3, 4), "f") == 4                          # a column of a per-point record
    gap = torch.zeros(2, 4, 4)[:, :3]                                                     # a gap between the rows
    for bad in (torch.zeros(4, 3, 2).permute(2, 1, 0), torch.zeros(2, 4, 3).transpose(1, 2), gap, torch.zeros(3, 4),
                torch.zeros(2, 3, 4, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="the_name"):
            util._field_stride(bad, "the_name")


# ------------------------------------------------------------------------------------------- the wrappers' contract, as a table
# One row per wrapper of util, recon and render.occupancy that hands tensors to the library: a well-formed call from host
# tensors of the smallest legal shapes (SB = 1, NV = 2, H = W = 4, B = 8, NS = 1, C = 3) and what to swap in for a wrong dtype, a
# wrong shape and — where the wrapper takes one — a non-contiguous output.
# util.image_to_tensor has no row: it uploads a host image itself, so a well-formed host call is no refusal.
#
# The table was written against the tree before the helpers existed and passed there except for the cases marked below, each of
# which ended in another exception there and none of which succeeded:
#   [order]  that tree looked at the device before the dtype or the shape, so a malformed host tensor got a RuntimeError where it
#            now gets a ValueError: a change of its own, made so that every wrapper follows the one order DESIGN.md states
#   [out]    that tree judged a given output after the device, or (frame_from_hits) together with it
SB, NV, H, W, B, NS = 1, 2, 4, 4, 8, 1


@functools.lru_cache(maxsize=None)
def _rows():
    from pixel_nerf_multiscale_amd import recon, util
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    f32, u8, i32, i64, f64 = torch.float32, torch.uint8, torch.int32, torch.int64, torch.float64
    z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype)
    strided = lambda *shape, dtype=f32: torch.zeros(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]     # right shape, not contiguous
    img_u8, poses, pix, ords = z(SB, NV, H, W, 3, dtype=u8), z(SB, NV, 4, 4), z(SB, B, dtype=i64), z(SB, NS, dtype=i64)
    bits, rows = z(SB, NV * H, 1, dtype=i32), z(SB, NV * H + 1, dtype=i32)
    rgba = z(SB, NV, H, W, 4, dtype=u8)
    grid = occ.OccupancyGrid.from_cells(torch.ones(1, 1, 1, dtype=torch.bool), (-1, -1, -1), (1, 1, 1))
    box = ((-1, -1, -1), (1, 1, 1))
    # name: (function, good keywords, wrong dtype, wrong shape, non-contiguous output or None)
    return {
        "train_batch": (util.train_batch, dict(images=z(SB, NV, 3, H, W), poses=poses, focal=10.0, c=None, pix_inds=pix, z_near=0.5, z_far=2.0),
                        dict(pix_inds=pix.int()),                                                     # [order]
                        dict(poses=z(SB, NV + 1, 4, 4)), None),                                       # [order]
        "color_jitter_plan": (util.color_jitter_plan, dict(images_u8=img_u8, ranges=(0.4, 0.4, 0.4, 0.1), seed=7),
                              dict(images_u8=img_u8.float()), dict(images_u8=z(SB, NV, H, W, 5, dtype=u8)),
                              dict(out=strided(SB, 8))),                                              # [out]
        "train_batch_u8": (util.train_batch_u8, dict(images_u8=img_u8, poses=poses, focal=10.0, c=None, pix_inds=pix, z_near=0.5, z_far=2.0),
                           dict(images_u8=img_u8.float()), dict(images_u8=z(SB, NV, H, W, 2, dtype=u8)), None),
        "views_to_tensor_u8": (util.views_to_tensor_u8, dict(images_u8=img_u8, view_ord=ords),
                               dict(images_u8=img_u8.float()), dict(images_u8=z(NV, H, W, 3, dtype=u8)), None),
        "train_draw": (util.train_draw, dict(bbox=z(SB, NV, 4), SB=SB, NV=NV, W=W, H=H, B=B, NS=NS, seed=7),
                       dict(bbox=z(SB, NV, 4, dtype=f64)), dict(bbox=z(SB, NV + 1, 4)), dict(out_pix=strided(SB, B, dtype=i64))),
        "mask_table": (util.mask_table, dict(masks=rgba[..., 3:], pix_stride=4),
                       dict(masks=rgba.float()[..., 3:]), dict(masks=rgba[0, 0, :, :, 3:]),
                       dict(out=(strided(SB, NV * H, 1, dtype=i32), rows))),                          # [out]
        "train_draw_masked": (util.train_draw_masked, dict(bits=bits, rows=rows, SB=SB, NV=NV, W=W, H=H, B=B, NS=NS, seed=7, prop_inside=0.5),
                              dict(bits=bits.long()), dict(rows=rows[:, :-1]), dict(out_pix=strided(SB, B, dtype=i64))),
        "mask_gather": (util.mask_gather, dict(bits=bits, pix_inds=pix, NV=NV, H=H, W=W),
                        dict(pix_inds=pix.int()), dict(bits=bits[:, :-1]), dict(out=strided(SB, B))),
        "eval_frame": (util.eval_frame, dict(rgb=z(H, W, 3), gt=z(3, H, W)),
                       dict(rgb=z(H, W, 3, dtype=f64)),                                               # [order]
                       dict(rgb=z(H, W, 4)), dict(metrics_out=strided(2, dtype=f64))),                # [out]
        "eval_frames": (util.eval_frames, dict(rgb=z(1, H, W, 3), gt=z(1, 3, H, W)),
                        dict(gt=z(1, 3, H, W, dtype=f64)), dict(gt=z(1, 4, H, W)), dict(metrics_out=strided(1, 2, dtype=f64))),   # [out]
        "eval_frames_u8": (util.eval_frames_u8, dict(pred_u8=z(1, H, W, 3, dtype=u8), gt_u8=z(1, H, W, 4, dtype=u8)),
                           dict(pred_u8=z(1, H, W, 3)), dict(gt_u8=z(1, H, W, 5, dtype=u8)),
                           dict(metrics_out=strided(1, 2, dtype=f64))),                               # [out]
        "upsample_concat": (util.upsample_concat, dict(levels=[z(1, 8, H, W), z(1, 8, 2, 2)]),
                            dict(levels=[z(1, 8, H, W, dtype=f64)]), dict(levels=[z(8, H, W)]), None),
        "cmap_device": (util.cmap_device, dict(map=z(H, W)), dict(map=z(H, W, dtype=f64)), dict(map=z(H * W)), None),
        "vis_panel": (util.vis_panel, dict(images=z(NV, 3, H, W), src_views=[0], gt_view=1, passes=[(z(H * W, 3), z(H * W), z(H * W, 2))]),
                      dict(images=z(NV, 3, H, W, dtype=f64)), dict(images=z(NV, 4, H, W)), None),
        "video_frames": (util.video_frames, dict(rgb=z(H * W, 3), F=1, H=H, W=W),
                         dict(rgb=z(H * W, 3, dtype=f64)), dict(rgb=z(H * W + 1, 3)), dict(out=strided(H * W * 3, dtype=u8))),    # [out]
        "view_strip": (util.view_strip, dict(images=z(NS, 3, H, W)),
                       dict(images=z(NS, 3, H, W, dtype=f64)), dict(images=z(NS, 4, H, W)), dict(out=strided(H, NS * W, 3, dtype=u8))),  # [out]
        "resize_area_u8": (util.resize_area_u8, dict(images_u8=z(NV, H, W, 3, dtype=u8), size=2),
                           dict(images_u8=z(NV, H, W, 3)), dict(images_u8=z(NV, H, W, 5, dtype=u8)),
                           dict(out=strided(NV, 2, 2, 3, dtype=u8))),                                 # [out]
        "resize_area": (util.resize_area, dict(images=z(NV, 3, H, W), size=2),
                        dict(images=z(NV, 3, H, W, dtype=f64)), dict(images=z(W)), dict(out=strided(NV, 3, 2, 2))),               # [out]
        "extract_mesh": (recon.extract_mesh, dict(field=z(2, 3, 4), iso=0.5),
                         dict(field=z(2, 3, 4, dtype=f64)), dict(field=z(3, 4)), None),
        "from_sigma": (occ.OccupancyGrid.from_sigma, dict(sigma=z(2, 3, 4), c1=box[0], c2=box[1], thresh=1.0),
                       dict(sigma=z(2, 3, 4, dtype=f64)), dict(sigma=z(3, 4)), None),
        "ray_bounds": (occ.ray_bounds, dict(grid=grid, rays=z(4, 8)), dict(rays=z(4, 8, dtype=f64)), dict(rays=z(4, 7)), None),
        "frame_from_hits": (occ.frame_from_hits, dict(rec=z(4, 4), slot=z(4, dtype=i32), rays_per_frame=4, bg=1.0),
                            dict(slot=z(4, dtype=i64)), dict(rec=z(3, 4)), dict(out=strided(4, 4))),  # [out]
    }


WRAPPERS = ("train_batch", "color_jitter_plan", "train_batch_u8", "views_to_tensor_u8", "train_draw", "mask_table", "train_draw_masked",
            "mask_gather", "eval_frame", "eval_frames", "eval_frames_u8", "upsample_concat", "cmap_device", "vis_panel", "video_frames",
            "view_strip", "resize_area_u8", "resize_area", "extract_mesh", "from_sigma", "ray_bounds", "frame_from_hits")


def test_the_table_names_every_row():
    assert tuple(_rows()) == WRAPPERS


@pytest.mark.parametrize("name", WRAPPERS)
def test_wrapper_contract(name):
    fn, good, wrong_dtype, wrong_shape, wrong_out = _rows()[name]
    with pytest.raises(RuntimeError):                     # host tensors pass every check of their own and are refused as such
        fn(**good)
    with pytest.raises(ValueError):
        fn(**{**good, **wrong_dtype})
    with pytest.raises(ValueError):
        fn(**{**good, **wrong_shape})
    if wrong_out is not None:
        (key, value), = wrong_out.items()
        assert not (value[0] if isinstance(value, tuple) else value).is_contiguous()
        with pytest.raises(ValueError):
            fn(**{**good, **wrong_out})


def test_mask_table_takes_both_outputs_or_none():
    from pixel_nerf_multiscale_amd import util
    masks = torch.zeros(SB, NV, H, W, dtype=torch.uint8)
    bits, rows = torch.zeros(SB, NV * H, 1, dtype=torch.int32), torch.zeros(SB, NV * H + 1, dtype=torch.int32)
    for half in ((bits, None), (None, rows), (None, None)):
        with pytest.raises(ValueError, match="out"):
            util.mask_table(masks, out=half)
