"""Area resampling on the device (image_size): pnr_resize_area_u8 / pnr_resize_area_f32 against the numpy restatement of
include/pnr.h (tests/resize_util.py; torch.equal — both contracts are bit-exact), ResidentSplit(image_size=...) and
ResizedDataset against the same model on the datasets' own bytes, and the resized data through make_batch, evaluate and one
Trainer epoch."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import data_trees as dt
import golden_util as gu
import resize_util as R
from hip_util import model_conf

pytestmark = pytest.mark.gpu

FILL_IN, FILL_OUT = 0x5A, 0xC3
SIZE, SMALL = 16, (8, 8)
SSIM_TOL, PSNR_TOL = 1e-6, 2e-5                              # tests/test_gpu_eval_back.py's bounds between the two back ends


# ---------------------------------------------------------------------------------------------------- the byte kernel
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("name", sorted(R.GPU_SHAPES))
def test_resize_area_u8_equals_the_model(name, C):
    """F = 1 and 3 frames, the frames of both sides further apart than a frame (odd gaps: frames start at every byte phase),
    the input at byte offsets 0..3 of a larger allocation, the output inside sentinel margins: every target byte is the
    model's, and no byte between or around the output frames is touched."""
    from pixel_nerf_multiscale_amd import _native as N, util
    (H, W), (Ht, Wt) = R.GPU_SHAPES[name]
    for F in (1, 3):
        a = R.bytes_case(F, H, W, C, Ht, Wt)
        want = torch.from_numpy(R.model_u8(a, Ht, Wt))
        if name == "identity_is_a_copy":
            assert torch.equal(want, torch.from_numpy(a))
        if name == "row_past_a_workgroup":
            # a target row past one workgroup's 256 pixels; a source row past what the 64 windows of one wave cover
            assert len(set(a.reshape(-1).tolist())) == 256 and Wt > 256 and W > 64 * -(-W // Wt)
        n_in, n_out = H * W * C, Ht * Wt * C
        in_stride, out_stride = n_in + 5, n_out + 3
        frames = torch.from_numpy(a).reshape(F, n_in).cuda()
        for off in range(4):
            src = torch.full((off + F * in_stride + 8,), FILL_IN, dtype=torch.uint8, device="cuda")
            src[off:off + F * in_stride].view(F, in_stride)[:, :n_in] = frames
            lead = 5 + off
            dst = torch.full((lead + F * out_stride + 8,), FILL_OUT, dtype=torch.uint8, device="cuda")
            rc = N.lib.pnr_resize_area_u8(src.data_ptr() + off, in_stride, F, H, W, C, dst.data_ptr() + lead, out_stride, Ht, Wt,
                                          N.current_stream(dst.device))
            assert rc == 0
            dst = dst.cpu()
            body = dst[lead:lead + F * out_stride].view(F, out_stride)
            assert torch.equal(body[:, :n_out].reshape(F, Ht, Wt, C), want), (F, off)
            assert bool((body[:, n_out:] == FILL_OUT).all()) and bool((dst[:lead] == FILL_OUT).all())
            assert bool((dst[lead + F * out_stride:] == FILL_OUT).all())
        # the wrapper: dense, any leading dimensions, and out= a slot of a pool
        dev = torch.from_numpy(a).cuda()
        assert torch.equal(util.resize_area_u8(dev, (Ht, Wt)).cpu(), want)
        assert torch.equal(util.resize_area_u8(dev[0], (Ht, Wt)).cpu(), want[0])
        assert torch.equal(util.resize_area_u8(dev.view(1, F, H, W, C), (Ht, Wt)).cpu(), want[None])
        pool = torch.full((2, F, Ht, Wt, C), FILL_OUT, dtype=torch.uint8, device="cuda")
        assert util.resize_area_u8(dev, (Ht, Wt), out=pool[1]).data_ptr() == pool[1].data_ptr()
        assert torch.equal(pool[1].cpu(), want) and bool((pool[0] == FILL_OUT).all())
    if Ht == Wt:
        assert torch.equal(util.resize_area_u8(dev, Ht).cpu(), want)            # an int is a square target


def test_resize_area_u8_wrapper_refuses_a_wrong_out():
    from pixel_nerf_multiscale_amd import util
    a = torch.zeros(2, 8, 8, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        util.resize_area_u8(a, 4, out=torch.zeros(2, 4, 4, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        util.resize_area_u8(a, 4, out=torch.zeros(2, 4, 8, 3, dtype=torch.uint8, device="cuda")[:, :, ::2])
    with pytest.raises(ValueError):
        util.resize_area_u8(a, 4, out=torch.zeros(2, 4, 4, 3, dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------------- the float kernel
def _same_floats(got, want):
    """Bit for bit where the model holds a number, NaN where it holds a NaN (a NaN's payload is not part of the contract)."""
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


@pytest.mark.parametrize("name", sorted(R.GPU_SHAPES))
def test_resize_area_f32_equals_the_model(name):
    """b / 255 quotients and balanced values: the kernel's bits are the model's (the fp64 sum in the header's order), and within
    one fp32 ulp of torch's own fp64 F.interpolate(mode="area") cast to fp32 (the bound tests/test_resize_cpu.py derives).  Then
    one NaN and one Inf: exactly the windows that contain them are poisoned.  The raw call writes inside sentinel margins."""
    from pixel_nerf_multiscale_amd import _native as N, util
    (H, W), (Ht, Wt) = R.GPU_SHAPES[name]
    F = 3
    differing = 0
    for kind in ("quotients", "balanced"):
        a = R.floats_case(F, H, W, kind)
        want = torch.from_numpy(R.model_f32(a, Ht, Wt))
        dev = torch.from_numpy(a).cuda()
        got = util.resize_area(dev, (Ht, Wt)).cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == (F, Ht, Wt)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        d = R.ulp_distance(got.numpy(), R.torch_area64(a, Ht, Wt).astype(np.float32))
        assert int(d.max()) <= 1
        differing += int((d > 0).sum())
        assert torch.equal(util.resize_area(dev.view(F, 1, H, W), (Ht, Wt)).cpu(), want[:, None])
        if name == "identity_is_a_copy":
            assert torch.equal(got, torch.from_numpy(a))
    print(f"{name}: {differing} of {2 * F * Ht * Wt} elements differ from torch's fp64 result cast to fp32 (by one ulp)")

    ry, rx, iy, ix = H // 2, W // 2, H - 1, 0
    a[1, ry, rx], a[2, iy, ix] = np.nan, -np.inf
    want = torch.from_numpy(R.model_f32(a, Ht, Wt))
    lead, numel = 3, F * Ht * Wt
    buf = torch.full((numel + 2 * lead,), -777.25, device="cuda")
    src = torch.from_numpy(a).cuda()
    rc = N.lib.pnr_resize_area_f32(src.data_ptr(), F, H, W, buf.data_ptr() + 4 * lead, Ht, Wt, N.current_stream(buf.device))
    assert rc == 0
    buf = buf.cpu()
    got = buf[lead:lead + numel].view(F, Ht, Wt)
    assert bool((buf[:lead] == -777.25).all()) and bool((buf[lead + numel:] == -777.25).all())
    assert _same_floats(got, want)
    rows, cols = R.windows(H, Ht), R.windows(W, Wt)
    holds = lambda r, c: torch.tensor([[r0 <= r < r1 and c0 <= c < c1 for (c0, c1) in cols] for (r0, r1) in rows])
    assert torch.equal(torch.isnan(got[1]), holds(ry, rx)) and torch.equal(got[2] == -np.inf, holds(iy, ix))
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1][~holds(ry, rx)]).all())
    assert bool(torch.isfinite(got[2][~holds(iy, ix)]).all())


# ---------------------------------------------------------------------------------------------------- the trees
NV = 3
SRN_FOCAL, SRN_CX, SRN_CY = 16.5, 8.5, 7.25
SRN_BOXES = [[(2 + v, 3, 12, 13 - v - o % 2) for v in range(NV)] for o in range(4)]       # corners at every phase of a window
ALIGNED_BOXES = [(2, 4, 11, 13), (4, 2, 13, 9), (0, 0, 15, 15)]       # every 2 x 2 window is all foreground or all background
CAT = "02691156"


def _srn_poses(o):
    poses = np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(NV)]).astype(np.float32)
    poses[:, :, 1:3] *= -1.0                                 # stored in the OpenCV convention; the dataset flips it back
    return poses


STEMS = ["000000", "000001", "000002"]


@pytest.fixture(scope="module")
def srn_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("srn16")
    for stage, n_obj in (("train", 4), ("val", 2)):
        for o in range(n_obj):
            images = dt.boxed_views(NV, SIZE, SIZE, SRN_BOXES[o], seed=10 * o + (stage == "val"))
            dt.write_srn_object(str(root / f"cars_{stage}" / f"obj{o}"), images, _srn_poses(o), SRN_FOCAL, SRN_CX, SRN_CY, STEMS)
    return str(root / "cars")


@pytest.fixture(scope="module")
def dvr_tree(tmp_path_factory):
    """Two objects of two views; the masks are L-shaped, so a box is not the mask."""
    root = tmp_path_factory.mktemp("nmr16")
    rng = np.random.default_rng(4)
    for o, name in enumerate(("a", "b")):
        images = rng.integers(0, 256, (2, SIZE, SIZE, 3), dtype=np.uint8)
        masks = np.zeros((2, SIZE, SIZE), np.uint8)
        for v in range(2):
            masks[v, 3 + o:12, 5 - v:7] = 255
            masks[v, 10:12 + v, 5 - v:14 - o] = 255
        cams = {}
        for v in range(2):
            m = np.eye(4)
            m[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            m[:3, 3] = rng.normal(size=3)
            cams[f"world_mat_{v}"], cams[f"camera_mat_{v}"] = m, np.diag([2.1875, 2.1875, 1.0, 1.0])
        dt.write_dvr_object(str(root / CAT / name), images, masks, cams)
    with open(str(root / CAT / "softras_train.lst"), "w") as f:
        f.write("a\nb\n")
    return str(root)


def _dataset(kind, srn_tree, dvr_tree, as_bytes, stage="train"):
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    if kind == "srn":
        return get_split_dataset("srn", srn_tree, want_split=stage, as_bytes=as_bytes)
    return get_split_dataset("dvr", dvr_tree, want_split="train", as_bytes=as_bytes)


def _mask_boxes(item, size):
    """The brute force on the item's own masks: the box of "any source pixel under the window is foreground"."""
    masks = item["masks"].numpy() > 0
    return np.stack([R.mask_box(R.target_mask(m.reshape(m.shape[-2:]), *size)) for m in masks])


# ---------------------------------------------------------------------------------------------------- ResidentSplit
@pytest.mark.parametrize("kind", ["srn", "dvr"])
def test_resident_split_at_an_image_size(kind, srn_tree, dvr_tree):
    from pixel_nerf_multiscale_amd import util
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    dset = _dataset(kind, srn_tree, dvr_tree, True)
    items = [dset[i] for i in range(len(dset))]
    N, nv = len(items), int(items[0]["images"].shape[0])
    split = ResidentSplit(dset, "cuda", image_size=SMALL, device_boxes=True)
    assert tuple(split.images.shape) == (N, nv, 8, 8, 3) and split.nbytes == N * nv * 8 * 8 * 3 and split.image_size == SMALL
    want = torch.from_numpy(np.stack([R.model_u8(it["images"].numpy(), 8, 8) for it in items]))
    assert torch.equal(split.images.cpu(), want)
    boxes = torch.from_numpy(np.stack([_mask_boxes(it, SMALL) for it in items]))
    assert split.bbox.dtype == torch.float32 and torch.equal(split.bbox, boxes)
    assert torch.equal(split.bbox, torch.stack([util.resize_bbox(it["bbox"], (SIZE, SIZE), SMALL) for it in items]))
    assert split.bbox_dev.dtype == torch.float32 and torch.equal(split.bbox_dev.cpu(), boxes)
    assert torch.equal(split.poses.cpu(), torch.stack([it["poses"] for it in items]))
    assert split.focal.dtype == torch.float32 and tuple(split.focal.shape) == (N,)
    assert torch.equal(split.focal, torch.stack([torch.as_tensor(it["focal"], dtype=torch.float32) for it in items]) * 0.5)
    if kind == "srn":
        assert torch.equal(split.c, torch.tensor([[SRN_CX / 2, SRN_CY / 2]] * N)) and split.focal.tolist() == [SRN_FOCAL / 2] * N
    else:
        assert split.c is None
    batch = split.batch([1, 0])
    assert tuple(batch["images"].shape) == (2, nv, 8, 8, 3) and torch.equal(batch["images"].cpu(), want[[1, 0]])
    assert torch.equal(batch["bbox"], boxes[[1, 0]]) and torch.equal(batch["bbox_dev"].cpu(), boxes[[1, 0]])

    # the items' own size, as a pair or as None: the pool and the dicts of a split built without the keyword
    plain = ResidentSplit(dset, "cuda", device_boxes=True)
    assert torch.equal(plain.images.cpu(), torch.stack([it["images"] for it in items]))
    assert torch.equal(plain.bbox, torch.stack([it["bbox"] for it in items]))
    for same in (ResidentSplit(dset, "cuda", device_boxes=True, image_size=(SIZE, SIZE)),
                 ResidentSplit(dset, "cuda", device_boxes=True, image_size=SIZE),
                 ResidentSplit(dset, "cuda", device_boxes=True, image_size=None)):
        a, b = plain.batch([0, 1]), same.batch([0, 1])
        assert sorted(a) == sorted(b) and a["path"] == b["path"]
        for k in a:
            if k != "path":
                assert a[k].dtype == b[k].dtype and a[k].device == b[k].device and torch.equal(a[k], b[k]), k
        assert torch.equal(plain.images, same.images) and torch.equal(plain.poses, same.poses)

    # max_bytes is judged on the resized pool, before anything is allocated
    small, full = N * nv * 8 * 8 * 3, N * nv * SIZE * SIZE * 3
    assert ResidentSplit(dset, "cuda", max_bytes=small, image_size=SMALL).nbytes == small
    with pytest.raises(ValueError, match="max_bytes"):
        ResidentSplit(dset, "cuda", max_bytes=small - 1, image_size=SMALL)
    with pytest.raises(ValueError, match="max_bytes"):
        ResidentSplit(dset, "cuda", max_bytes=full - 1)
    with pytest.raises(ValueError):
        ResidentSplit(dset, "cuda", image_size=(8, 0))

    # two scales: focal becomes (fx sx, fy sy)
    wide = ResidentSplit(dset, "cuda", image_size=(8, 4), device_boxes=True)
    assert torch.equal(wide.images.cpu(), torch.from_numpy(np.stack([R.model_u8(it["images"].numpy(), 8, 4) for it in items])))
    f0 = torch.stack([torch.as_tensor(it["focal"], dtype=torch.float32) for it in items])
    assert torch.equal(wide.focal, torch.stack((f0 * 0.25, f0 * 0.5), dim=-1))
    assert torch.equal(wide.bbox, torch.from_numpy(np.stack([_mask_boxes(it, (8, 4)) for it in items])))


def test_a_tree_written_at_the_small_size_gives_the_same_split(tmp_path):
    """A 16 x 16 SRN tree resampled to 8 x 8, against a tree WRITTEN at 8 x 8 from the model's bytes with the scaled
    intrinsics: the same pool and boxes bit for bit, intrinsics within 1e-6.  The boxes are aligned with the 2 x 2 windows, so
    a window holds foreground alone or background alone and the small files' own masks (no channel is 255) are the resampled
    masks — with a box edge inside a window, a mean of 255s and one 253 would round to 255 and the file would call it
    background."""
    from pixel_nerf_multiscale_amd.data import ResidentSplit, get_split_dataset
    for o in range(2):
        images = dt.boxed_views(NV, SIZE, SIZE, ALIGNED_BOXES, seed=3 + o)
        dt.write_srn_object(str(tmp_path / "big" / "cars_train" / f"obj{o}"), images, _srn_poses(o), SRN_FOCAL, SRN_CX, SRN_CY, STEMS)
        dt.write_srn_object(str(tmp_path / "small" / "cars_train" / f"obj{o}"), R.model_u8(images, 8, 8), _srn_poses(o),
                            SRN_FOCAL / 2, SRN_CX / 2, SRN_CY / 2, STEMS)
    big = ResidentSplit(get_split_dataset("srn", str(tmp_path / "big" / "cars"), want_split="train", as_bytes=True), "cuda",
                        image_size=SMALL, device_boxes=True)
    small = ResidentSplit(get_split_dataset("srn", str(tmp_path / "small" / "cars"), want_split="train", as_bytes=True), "cuda",
                          device_boxes=True)
    assert torch.equal(big.images, small.images) and torch.equal(big.poses, small.poses)
    assert torch.equal(big.bbox, small.bbox) and torch.equal(big.bbox_dev, small.bbox_dev)
    assert big.bbox[0].tolist() == [[1.0, 2.0, 5.0, 6.0], [2.0, 1.0, 6.0, 4.0], [0.0, 0.0, 7.0, 7.0]]
    assert float((big.focal - small.focal).abs().max()) <= 1e-6 and float((big.c - small.c).abs().max()) <= 1e-6


@pytest.mark.parametrize("kind", ["srn", "dvr"])
def test_make_batch_on_a_resized_split(kind, srn_tree, dvr_tree):
    """Device draws on a batch of the resized split: the pixels lie inside the NEW boxes, and rays and colours are
    pnr_train_batch_u8's on the model's bytes with the scaled intrinsics.  With a jitter it runs."""
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.data import ColorJitter, ResidentSplit
    dset = _dataset(kind, srn_tree, dvr_tree, True)
    split = ResidentSplit(dset, "cuda", image_size=SMALL, device_boxes=True)
    ids, seed, B, nviews = [1, 0], 12345, 64, [1, 2]
    data = split.batch(ids)
    nv = int(data["images"].shape[1])
    kw = dict(ray_batch_size=B, nviews=nviews, z_near=dset.z_near, z_far=dset.z_far, balanced=split.balanced, draws="device", seed=seed)
    rays, rgb, src_images, src_poses, focal, c = train.make_batch(data, torch.device("cuda"), **kw)
    NS = train.curr_nviews_for(nviews, seed)
    assert tuple(rays.shape) == (2, B, 8) and tuple(rgb.shape) == (2, B, 3) and tuple(src_images.shape) == (2, NS, 3, 8, 8)
    pix, views = util.train_draw(data["bbox_dev"], 2, nv, 8, 8, B, NS, seed)
    pix = pix.cpu()
    v, row, col = pix // 64, (pix % 64) // 8, pix % 8
    assert int(pix.min()) >= 0 and int(pix.max()) < nv * 64
    box = torch.stack([data["bbox"][o][v[o]] for o in range(2)])                # (2, B, 4)
    assert bool(((col >= box[..., 0]) & (col <= box[..., 2]) & (row >= box[..., 1]) & (row <= box[..., 3])).all())
    model = torch.from_numpy(np.stack([R.model_u8(dset[i]["images"].numpy(), 8, 8) for i in ids])).cuda()
    want_rays, want_rgb = util.train_batch_u8(model, data["poses"], split.focal[ids], None if split.c is None else split.c[ids],
                                              pix.cuda(), dset.z_near, dset.z_far, balanced=split.balanced)
    assert torch.equal(rays, want_rays) and torch.equal(rgb, want_rgb)
    assert not bool(torch.isnan(rays).any()) and not bool(torch.isnan(rgb).any())
    assert torch.equal(src_images, util.views_to_tensor_u8(model, views, balanced=split.balanced))
    assert torch.equal(focal.cpu(), split.focal[ids].reshape(-1, 1).expand(2, 2))
    out = train.make_batch(data, torch.device("cuda"), jitter=ColorJitter(0.4, 0.4, 0.4, 0.1), **kw)
    assert tuple(out[1].shape) == (2, B, 3) and bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(out[2]).all())
    assert torch.equal(out[0], rays)                                            # the jitter changes colours, not rays


# ---------------------------------------------------------------------------------------------------- ResizedDataset
@pytest.mark.parametrize("as_bytes", [True, False])
@pytest.mark.parametrize("kind", ["srn", "dvr"])
def test_resized_dataset_items(kind, as_bytes, srn_tree, dvr_tree):
    from pixel_nerf_multiscale_amd import util
    from pixel_nerf_multiscale_amd.data import ResizedDataset
    dset = _dataset(kind, srn_tree, dvr_tree, as_bytes)
    small = ResizedDataset(dset, SMALL)
    assert len(small) == len(dset) and small.as_bytes is as_bytes and small.balanced == dset.balanced
    assert (small.z_near, small.z_far, small.lindisp) == (dset.z_near, dset.z_far, dset.lindisp)
    for i in range(len(dset)):
        item, got = dset[i], small[i]
        assert sorted(got) == sorted(item)
        for k in item:
            assert type(got[k]) is type(item[k]), k
            if torch.is_tensor(item[k]):
                assert got[k].dtype == item[k].dtype and got[k].device == item[k].device and got[k].dim() == item[k].dim(), k
        nv = int(item["images"].shape[0])
        if as_bytes:
            assert tuple(got["images"].shape) == (nv, 8, 8, 3) and tuple(got["masks"].shape) == (nv, 8, 8)
            assert torch.equal(got["images"], torch.from_numpy(R.model_u8(item["images"].numpy(), 8, 8)))
            assert torch.equal(got["masks"], torch.from_numpy(R.model_u8(item["masks"].numpy()[..., None], 8, 8)[..., 0]))
        else:
            assert tuple(got["images"].shape) == (nv, 3, 8, 8) and tuple(got["masks"].shape) == (nv, 1, 8, 8)
            assert torch.equal(got["images"], torch.from_numpy(R.model_f32(item["images"].numpy(), 8, 8)))
            assert torch.equal(got["masks"], torch.from_numpy(R.model_f32(item["masks"].numpy(), 8, 8)))
            frac = got["masks"][(got["masks"] > 0) & (got["masks"] < 1)]
            assert frac.numel() > 0                         # a float mask becomes fractional along the outline
        assert torch.equal(got["bbox"], torch.from_numpy(_mask_boxes(item, SMALL)))
        assert torch.equal(got["bbox"], util.resize_bbox(item["bbox"], (SIZE, SIZE), SMALL))
        want_focal, want_c = util.resize_intrinsics(item["focal"], item.get("c"), (SIZE, SIZE), SMALL)
        assert float(got["focal"]) == float(want_focal) == float(item["focal"]) / 2
        if kind == "srn":
            assert torch.equal(got["c"], want_c) and got["c"].tolist() == [SRN_CX / 2, SRN_CY / 2]
        assert torch.equal(got["poses"], item["poses"]) and got["path"] == item["path"] and got["img_id"] == item["img_id"]
    same = ResizedDataset(dset, SIZE)[0]                    # the items' own size: passed through
    assert torch.equal(same["images"], dset[0]["images"]) and torch.equal(same["bbox"], dset[0]["bbox"])


# ---------------------------------------------------------------------------------------------------- evaluate and Trainer
def _model():
    """tests/test_gpu_trainer.py's smallest configuration, for 8 x 8 images: without the first pool the third level of an
    8 x 8 image is the 2 x 2 map of 128 channels that a 16 x 16 image leaves there."""
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet
    torch.manual_seed(0)
    conf = model_conf(dict(gu.CASES["tiny_ns2_codeview"]), "fp32")
    conf["encoder"]["num_layers"] = 3
    conf["encoder"]["use_first_pool"] = False
    net = PixelNeRFNet(conf).cuda()
    rend = NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, white_bkgd=True).cuda()
    return net, rend


@pytest.fixture()
def deterministic_convolutions():
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def test_evaluate_on_a_resized_dataset(srn_tree, dvr_tree, tmp_path, deterministic_convolutions):
    """evaluate() over ResizedDataset renders 8 x 8 frames (8 >= 7, the SSIM window) with finite metrics on the device back
    end, and the host back end agrees within the bounds tests/test_gpu_eval_back.py holds the two to."""
    from PIL import Image
    from pixel_nerf_multiscale_amd import evalio
    from pixel_nerf_multiscale_amd.data import ResizedDataset
    net, rend = _model()
    net.eval(); rend.eval()
    small = ResizedDataset(_dataset("srn", srn_tree, dvr_tree, False, stage="val"), SMALL)
    rows = {}
    for back_end in ("device", "host"):
        out = str(tmp_path / back_end)
        m = evalio.evaluate(net, rend, small, out, source="0", verbose=False, seed=5, metrics=back_end)
        rows[back_end] = [x.split() for x in open(os.path.join(out, "finish.txt")).read().split("\n") if x]
        assert m[2] == 2 and np.isfinite(m[0]) and np.isfinite(m[1])
        assert sorted(os.listdir(os.path.join(out, "obj0"))) == ["000001.png", "000002.png"]
        assert np.asarray(Image.open(os.path.join(out, "obj0", "000001.png"))).shape == (8, 8, 3)
    for d, h in zip(rows["device"], rows["host"]):
        assert d[0] == h[0] and np.isfinite(float(d[1])) and np.isfinite(float(d[2]))
        print(f"{d[0]}: |dPSNR| = {abs(float(d[1]) - float(h[1])):.3e} dB  |dSSIM| = {abs(float(d[2]) - float(h[2])):.3e}")
        assert abs(float(d[1]) - float(h[1])) <= PSNR_TOL and abs(float(d[2]) - float(h[2])) <= SSIM_TOL


def test_one_trainer_epoch_on_a_resized_split(srn_tree, dvr_tree, tmp_path, deterministic_convolutions):
    """Two steps on ResidentSplit(image_size=(8, 8)) and a DataLoader-fed validation pass over ResizedDataset: finite losses,
    a checkpoint."""
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.data import ResidentSplit, ResizedDataset
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend = _model()
    split = ResidentSplit(_dataset("srn", srn_tree, dvr_tree, True), "cuda", image_size=SMALL, device_boxes=True)
    val = ResizedDataset(_dataset("srn", srn_tree, dvr_tree, False, stage="val"), SMALL)
    scalars = []

    class Writer:
        def add_scalar(self, tag, value, step):
            scalars.append((tag, float(value), int(step)))

        def add_image(self, *a, **k):
            pass

    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        t = train.Trainer(net, rend, split, val, name="run", checkpoints_path=str(tmp_path / "ckpt"), logs_path=str(tmp_path / "logs"),
                          batch_size=2, ray_batch_size=32, nviews=[1, 2], loss=RenderLoss(1.0, 1.0), num_epochs=1, print_interval=1,
                          seed=5, eval_interval=1, vis_interval=1000, writer=Writer())
        assert t.train_loader is None and t.val_loader is not None and t.batches_per_epoch == 2
        t.start()
    losses = [s[1] for s in scalars if s[0] == "train/t"]
    val_losses = [s[1] for s in scalars if s[0] == "val/loss"]
    assert len(losses) == 2 and all(np.isfinite(x) and x > 0 for x in losses) and t.global_step == 2
    assert len(val_losses) == 1 and np.isfinite(val_losses[0]) and val_losses[0] > 0
    files = sorted(os.listdir(str(tmp_path / "ckpt" / "run")))
    assert "epoch_0000.pth" in files and "latest.pth" in files
