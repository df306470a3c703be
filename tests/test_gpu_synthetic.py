"""Procedural datasets on the device: pnr_synth_render against the float32 model of include/pnr.h (tests/synth_util.py) with
torch.equal on bytes, mask and depth; data.SyntheticShapes against SRNDataset's item form, through write_srn_tree and
ResidentSplit; and the smallest end-to-end run — two Trainer epochs lower a fixed validation loss, evaluate writes finish.txt."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
import synth_util as su  # noqa: E402
from hip_util import model_conf  # noqa: E402

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _check(scenes, ids, poses, W, H, focal, c=None, ss=2, want_mask=True, want_depth=True, **kw):
    """One launch against the model: bytes, mask and depth bit for bit.  -> (rgb, mask, depth) of the model."""
    from pixel_nerf_multiscale_amd import util
    fx, fy, cx, cy = util.intrinsics(focal, c, W, H)
    rgb, mask, depth = util.synth_render(_dev(scenes), _dev(ids, torch.int32), _dev(poses), W, H, focal, c, ss=ss,
                                         mask_out=True if want_mask else None, depth_out=True if want_depth else None, **kw)
    want = su.model_render(scenes, ids, poses, W, H, fx, fy, cx, cy, ss=ss, **kw)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (len(ids), H, W, 3)
    assert torch.equal(rgb.cpu(), torch.from_numpy(want[0])), f"{int((rgb.cpu() != torch.from_numpy(want[0])).sum())} bytes differ"
    if want_mask:
        assert mask.dtype == torch.uint8 and torch.equal(mask.cpu(), torch.from_numpy(want[1]))
    else:
        assert mask is None
    if want_depth:
        assert depth.dtype == torch.float32 and torch.equal(depth.cpu(), torch.from_numpy(want[2]))      # +inf == +inf
    else:
        assert depth is None
    return want


@pytest.mark.parametrize("ss", [1, 2, 4])
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (32, 32), (257, 2)])
def test_kernel_equals_model(size, ss):
    """W x H: one pixel; a frame shorter than one thread's four pixels per row; whole dwords; 257 x 2, rows whose length is no
    multiple of 4 and that pass one workgroup's 256 pixels.  The three named scenes in a non-monotonic order."""
    W, H = size
    rgb, mask, depth = _check(su.named_scenes(), [2, 0, 1], su.issue_poses(), W, H, 1.25 * max(W, H), ss=ss)
    if min(W, H) >= 32:
        assert mask.any(axis=(1, 2)).all() and not mask.all() and np.isfinite(depth).any()


def test_empty_scene_p8_and_scene_ids_out_of_range():
    from pixel_nerf_multiscale_amd.data import synthetic
    poses = np.concatenate([su.issue_poses(), su.issue_poses()[:2]])
    rgb, mask, depth = _check(np.zeros((2, 3, su.REC), np.float32), [1, 0, 1], su.issue_poses(), 12, 10, 15.0)
    assert (rgb == 255).all() and (mask == 0).all() and np.isposinf(depth).all()                         # nothing but `none`
    scenes = synthetic.random_scenes(6, 1, max_prims=8)
    assert scenes.shape[1] == 8 and ((scenes[..., 0] != 0).sum(1) >= 6).any()
    rgb, mask, depth = _check(scenes, [5, 0, 6, 3, -1], poses, 24, 20, 26.0)                             # 6 and -1: no such scene
    assert (rgb[[2, 4]] == 255).all() and (mask[[2, 4]] == 0).all() and mask[[0, 1, 3]].any(axis=(1, 2)).all()


def test_intrinsics_and_an_axis_aligned_camera():
    _check(su.named_scenes(), [1, 2], su.issue_poses()[:2], 30, 26, (40.0, 33.0), (13.5, 18.25), ss=2)
    # the camera on the z axis with the identity as its rotation, integer cx, cy: the pixels of column cx have a world direction
    # whose x is exactly 0 and those of row cy one whose y is; the boxes are axis-aligned, one under the axis and one beside it
    pose = np.eye(4, dtype=np.float32)
    pose[2, 3] = 1.3
    boxes = su.table([su.record(2, half=(0.2, 0.1, 0.15), albedo=(0.2, 0.5, 0.8)),
                      su.record(2, centre=(0.35, -0.3, 0.0), half=(0.1, 0.1, 0.1), albedo=(0.7, 0.6, 0.1)),
                      su.record(1, centre=(-0.3, 0.3, 0.0), half=(0.1, 0.15, 0.1))])
    for ss in (1, 2):
        rgb, mask, depth = _check(boxes, [0], pose[None], 9, 9, 8.0, (4.0, 4.0), ss=ss, ambient=0.0, light=(0.0, 0.0, 2.0))
    assert mask[0, 4, 4] == 255 and mask[0, :, 4].any() and not mask[0, :, 4].all()


def test_outputs_absent_and_a_slot_inside_a_larger_buffer():
    from pixel_nerf_multiscale_amd import _native as N, util
    scenes, ids, poses = su.named_scenes(), [0, 2], su.issue_poses()[:2]
    W, H, focal = 13, 7, 16.0
    want = _check(scenes, ids, poses, W, H, focal, want_mask=False, want_depth=False)
    _check(scenes, ids, poses, W, H, focal, want_mask=True, want_depth=False)
    _check(scenes, ids, poses, W, H, focal, want_mask=False, want_depth=True)
    n = 2 * H * W * 3
    d_scenes, d_ids, d_poses = _dev(scenes), _dev(ids, torch.int32), _dev(poses)
    for lead in (5, 8):                                       # a slot that starts inside a dword, and an aligned one
        buf = torch.full((lead + n + 11,), 0x5A, dtype=torch.uint8, device="cuda")
        mbuf = torch.full((3 + 2 * H * W + 6,), 0x5A, dtype=torch.uint8, device="cuda")
        out = buf[lead:lead + n].view(2, H, W, 3)
        got = util.synth_render(d_scenes, d_ids, d_poses, W, H, focal, out=out, mask_out=mbuf[3:3 + 2 * H * W].view(2, H, W))
        assert got[0] is out and got[0].data_ptr() == buf.data_ptr() + lead
        assert torch.equal(out.cpu(), torch.from_numpy(want[0]))
        assert (buf[:lead] == 0x5A).all() and (buf[lead + n:] == 0x5A).all()
        assert (mbuf[:3] == 0x5A).all() and (mbuf[3 + 2 * H * W:] == 0x5A).all()
    # the frame stride of the entry point itself: a margin of 9 bytes behind every frame
    stride = H * W * 3 + 9
    buf = torch.full((2 * stride,), 0x5A, dtype=torch.uint8, device="cuda")
    fx, fy, cx, cy = util.intrinsics(focal, None, W, H)
    N.check(N.lib.pnr_synth_render(d_scenes.data_ptr(), 3, 2, d_ids.data_ptr(), d_poses.data_ptr(), 2, W, H, fx, fy, cx, cy, 2, 0.3,
                                   0.3, 0.5, 0.8, buf.data_ptr(), stride, None, None, N.current_stream(buf.device)), "pnr_synth_render")
    frames = buf.view(2, stride).cpu()
    assert torch.equal(frames[:, :H * W * 3].reshape(2, H, W, 3), torch.from_numpy(want[0])) and (frames[:, H * W * 3:] == 0x5A).all()


def test_refusals_on_device_tensors():
    from pixel_nerf_multiscale_amd import util
    scenes, ids, poses = _dev(su.named_scenes()), _dev([0], torch.int32), _dev(su.issue_poses()[:1])
    for kw in (dict(ss=3), dict(ss=0), dict(ambient=1.5), dict(ambient=-0.1), dict(ambient=float("nan")), dict(light=(0.0, 0.0, 0.0)),
               dict(light=(float("inf"), 0.0, 1.0))):
        with pytest.raises(ValueError):
            util.synth_render(scenes, ids, poses, 8, 8, 10.0, **kw)
    with pytest.raises(ValueError):
        util.synth_render(torch.zeros(1, 9, su.REC, device="cuda"), ids, poses, 8, 8, 10.0)              # P > 8
    with pytest.raises(ValueError):
        util.synth_render(scenes, ids, poses, 8, 8, 0.0)
    with pytest.raises(ValueError, match="share a device"):
        util.synth_render(scenes, ids.cpu(), poses, 8, 8, 10.0)


# ------------------------------------------------------------------------------------------------------------ the dataset
NV, S = 6, 16


def _sets(as_bytes, **kw):
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    return get_split_dataset("synthetic", None, n_objects=4, n_val=2, n_test=1, n_views=NV, image_size=S, seed=3, as_bytes=as_bytes,
                             **kw)


def test_items_have_srn_form_and_equal_the_model():
    from pixel_nerf_multiscale_amd.data import _items, synthetic
    train_b, _, test_b = _sets(True, want_depth=True)
    train_f = _sets(False)[0]
    assert len(train_b) == 4 and len(test_b) == 1 and (train_b.z_near, train_b.z_far, train_b.lindisp) == (0.8, 1.8, False)
    for ds, i in ((train_b, 0), (train_b, 3), (test_b, 0)):
        item = ds[i]
        assert sorted(item) == ["bbox", "c", "depth", "focal", "images", "img_id", "masks", "path", "poses"]
        assert item["path"] == f"synthetic/{ds.stage}/{i:06d}" and item["img_id"] == i
        assert isinstance(item["focal"], float) and item["focal"] == 131.25 * S / 128
        assert item["c"].dtype == torch.float32 and item["c"].tolist() == [S / 2, S / 2]
        for key, dtype, shape in (("images", torch.uint8, (NV, S, S, 3)), ("masks", torch.uint8, (NV, S, S)),
                                  ("bbox", torch.float32, (NV, 4)), ("poses", torch.float32, (NV, 4, 4)),
                                  ("depth", torch.float32, (NV, S, S))):
            assert item[key].dtype == dtype and tuple(item[key].shape) == shape and not item[key].is_cuda, key
        poses = synthetic.view_poses(NV, 3, ds.stage, i)
        want = su.model_render(ds.scenes.numpy(), [i] * NV, poses, S, S, item["focal"], item["focal"], S / 2, S / 2, ss=2)
        assert torch.equal(item["poses"], torch.from_numpy(poses))
        assert torch.equal(item["images"], torch.from_numpy(want[0])) and torch.equal(item["masks"], torch.from_numpy(want[1]))
        assert torch.equal(item["depth"], torch.from_numpy(want[2]))
        m = want[1] != 0
        assert torch.equal(item["masks"] != 0, (item["images"] != 255).all(-1))                         # SRNDataset's rule
        for v in range(NV):
            rows, cols = np.flatnonzero(m[v].any(1)), np.flatnonzero(m[v].any(0))
            assert item["bbox"][v].tolist() == [cols[0], rows[0], cols[-1], rows[-1]]
            assert 0 < cols[0] and cols[-1] < S - 1 and 0 < rows[0] and rows[-1] < S - 1                 # the ball lies inside the frame
    fb, ff = train_b[1], train_f[1]
    assert sorted(ff) == ["bbox", "c", "focal", "images", "img_id", "masks", "path", "poses"]
    assert ff["images"].dtype == torch.float32 and tuple(ff["images"].shape) == (NV, 3, S, S)
    assert torch.equal(ff["images"], _items.images_to_float(fb["images"], True))
    assert ff["masks"].dtype == torch.float32 and torch.equal(ff["masks"], (fb["masks"] != 0)[:, None].float())
    assert torch.equal(ff["bbox"], fb["bbox"]) and torch.equal(ff["poses"], fb["poses"])
    again = _sets(True, want_depth=True)[0][1]                                                          # two constructions are equal
    assert all(torch.equal(again[k], fb[k]) for k in ("images", "masks", "bbox", "poses", "depth"))
    with pytest.raises(IndexError):
        train_b[4]


def test_tree_written_from_kernel_output_reads_back_exactly(tmp_path):
    from pixel_nerf_multiscale_amd.data import SRNDataset, synthetic
    train_b = _sets(True)[0]
    synthetic.write_srn_tree(train_b, str(tmp_path / "shapes"), "train")
    back = SRNDataset(str(tmp_path / "shapes"), stage="train", as_bytes=True)
    assert len(back) == 4
    for i in range(4):
        a, b = train_b[i], back[i]
        assert os.path.basename(b["path"]) == f"{i:06d}" and b["focal"] == a["focal"] and torch.equal(b["c"], a["c"])
        assert all(torch.equal(a[k], b[k]) for k in ("images", "masks", "bbox", "poses"))


def test_resident_split_and_device_draws():
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    train_b = _sets(True)[0]
    split = ResidentSplit(train_b, "cuda", device_boxes=True, device_masks=True)
    assert len(split) == 4 and tuple(split.images.shape) == (4, NV, S, S, 3) and (split.z_near, split.z_far) == (0.8, 1.8)
    assert torch.equal(split.images[2].cpu(), train_b[2]["images"]) and torch.equal(split.bbox[2], train_b[2]["bbox"])
    data = split.batch([3, 1])
    assert {"bbox_dev", "mask_bits", "mask_rows"} <= set(data)
    out = train.make_batch(data, torch.device("cuda"), ray_batch_size=32, nviews=[1, 2], z_near=0.8, z_far=1.8, draws="device",
                           seed=11, prop_inside=0.75, want_mask=True)
    rays, rgb, src_images, src_poses, focal, c, mask_gt = out
    assert tuple(rays.shape) == (2, 32, 8) and tuple(rgb.shape) == (2, 32, 3) and tuple(mask_gt.shape) == (2, 32)
    assert int(mask_gt.sum()) == 2 * 24 and torch.isfinite(rays).all() and float(rgb.min()) >= -1.0 and float(rgb.max()) <= 1.0


# ------------------------------------------------------------------------------------------------------------ end to end
def test_two_epochs_lower_the_validation_loss_and_evaluate_runs(tmp_path):
    """4 objects x 6 views of 16 x 16.  The condition is the issue's: train.validate on a fixed held-out loader, under one key,
    is lower after two Trainer epochs than before.  Then evaluate on the test stage writes finish.txt."""
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio, train
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    train_b, val_b, _ = _sets(True)
    test_f = _sets(False)[2]
    torch.manual_seed(0)
    conf = model_conf(dict(gu.CASES["tiny_ns2_codeview"]), "fp32")
    conf["encoder"]["num_layers"] = 3                       # 16 x 16 images: the third level is 2 x 2, the smallest map the kernels take
    net = PixelNeRFNet(conf).cuda()
    rend = NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, white_bkgd=True).cuda()
    pool = ResidentSplit(train_b, "cuda", device_boxes=True, device_masks=True)
    held_out = list(ResidentSplit(val_b, "cuda", device_boxes=True).batches(2, shuffle=False, drop_last=False))
    t = train.Trainer(net, rend, pool, None, name="run", checkpoints_path=str(tmp_path / "ckpt"), logs_path=str(tmp_path / "logs"),
                      batch_size=2, ray_batch_size=128, nviews=[1], loss=RenderLoss(1.0, 1.0), num_epochs=2, lr=1e-3,
                      print_interval=1, seed=5)

    def held_out_loss():
        key = 987654321
        with rend.keyed(key):
            return train.validate(net, rend, t.render_par, held_out, ray_batch_size=128, nviews=[1], z_near=0.8, z_far=1.8,
                                  loss=RenderLoss(1.0, 1.0), balanced=True, draws="device", seed=key)

    before = held_out_loss()
    assert before == held_out_loss()                        # one key: the same pixels, the same noise, the same number
    t.start()
    after = held_out_loss()
    print(f"held-out loss before {before:.6f}, after two epochs ({t.global_step} steps) {after:.6f}")
    assert t.global_step == 4 and np.isfinite(before) and np.isfinite(after)
    assert after < before
    net.eval()
    out = str(tmp_path / "eval")
    psnr, ssim, count = evalio.evaluate(net, rend, test_f, out, source="0", verbose=False, seed=7, metrics="device")
    rows = [x.split() for x in open(os.path.join(out, "finish.txt")).read().split("\n") if x]
    assert count == 1 and len(rows) == 1 and rows[0][0] == "000000" and np.isfinite(psnr) and np.isfinite(ssim)
    assert sorted(os.listdir(os.path.join(out, "000000"))) == [f"{v:06d}.png" for v in range(1, NV)]
