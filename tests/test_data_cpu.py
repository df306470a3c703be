"""The data layer without a GPU: the argument checks of pnr_train_batch_u8 / pnr_views_to_tensor_u8 and their wrappers (made
before any HIP call), and SRNDataset / DVRDataset / get_split_dataset on folders written here with PIL and numpy, every item
field against values this file states on its own."""
import os

import numpy as np
import pytest
import torch

import data_trees as dt

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5


# ------------------------------------------------------------------------------------------------ entry points and wrappers
def test_entry_points_check_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p = 64          # a non-NULL value: the checks below return before anything dereferences or launches
    tb = lambda images=p, poses=p, focal=p, c=None, SB=1, NV=1, W=4, H=4, inds=p, B=8, rays=p, rgb=p, C=3, balanced=1: \
        L.pnr_train_batch_u8(images, poses, focal, c, SB, NV, W, H, 0.1, 1.0, inds, B, rays, rgb, C, balanced, None)
    assert tb(poses=None) == E_NULL and tb(focal=None) == E_NULL and tb(inds=None) == E_NULL and tb(rays=None) == E_NULL
    assert tb(images=None) == E_NULL                      # colours wanted, no images
    assert tb(SB=0) == E_SHAPE and tb(NV=0) == E_SHAPE and tb(W=0) == E_SHAPE and tb(H=-1) == E_SHAPE and tb(B=-1) == E_SHAPE
    assert tb(NV=2, W=32768, H=32768) == E_SHAPE          # NV*H*W = 2^31
    assert tb(C=2) == E_SHAPE and tb(C=5) == E_SHAPE and tb(C=0) == E_SHAPE
    assert tb(balanced=2) == E_SHAPE and tb(balanced=-1) == E_SHAPE
    assert tb(B=0, C=5) == E_SHAPE                        # the checks come before the empty batch's early return
    assert tb(B=0) == 0 and tb(B=0, C=4, balanced=0) == 0  # nothing to do: no launch
    assert tb(images=None, rgb=None, B=0) == 0            # images may be NULL when no colours are asked for

    vt = lambda images=p, ords=p, SB=1, NV=1, NS=1, W=4, H=4, C=3, balanced=1, out=p: \
        L.pnr_views_to_tensor_u8(images, ords, SB, NV, NS, W, H, C, balanced, out, None)
    assert vt(images=None) == E_NULL and vt(ords=None) == E_NULL and vt(out=None) == E_NULL
    assert vt(SB=0) == E_SHAPE and vt(NV=0) == E_SHAPE and vt(NS=0) == E_SHAPE and vt(W=0) == E_SHAPE and vt(H=-3) == E_SHAPE
    assert vt(NV=2, W=32768, H=32768) == E_SHAPE
    assert vt(C=2) == E_SHAPE and vt(C=5) == E_SHAPE and vt(balanced=2) == E_SHAPE
    assert vt(out=66) == E_ALIGN and vt(out=65) == E_ALIGN
    assert vt(out=None, C=5) == E_NULL                    # NULL is reported first, as everywhere in the library


def test_wrappers_check_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import train, util
    u8 = torch.zeros(2, 3, 4, 5, 3, dtype=torch.uint8)
    poses, inds, ords = torch.zeros(2, 3, 4, 4), torch.zeros(2, 8, dtype=torch.long), torch.zeros(2, 1, dtype=torch.long)
    for bad in (u8.float(), u8[0], u8[..., :2], torch.zeros(2, 3, 4, 5, 5, dtype=torch.uint8), u8.numpy()):
        with pytest.raises(ValueError):
            util.train_batch_u8(bad, poses, 10.0, None, inds, 0.5, 2.0)
        with pytest.raises(ValueError):
            util.views_to_tensor_u8(bad, ords)
    with pytest.raises(RuntimeError):                     # well-formed host tensors: refused for where they live, not crashed on
        util.train_batch_u8(u8, poses, 10.0, None, inds, 0.5, 2.0)
    with pytest.raises(RuntimeError):
        util.views_to_tensor_u8(u8, ords)
    # make_batch: a uint8 tensor of any other shape is a ValueError, before anything is uploaded
    kw = dict(ray_batch_size=8, nviews=[1], z_near=0.5, z_far=2.0)
    for bad in (u8.permute(0, 1, 4, 2, 3), u8[0], torch.zeros(2, 3, 4, 5, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            train.make_batch({"images": bad, "poses": poses, "focal": torch.ones(2)}, "cuda", **kw)


# ------------------------------------------------------------------------------------------------------------------ SRN
H, W = 4, 5                                                # "3 views of 5 x 4"
STEMS = ["9", "10", "100"]                                 # written in this order; as STRINGS they sort 10 < 100 < 9
ORDER = [1, 2, 0]                                          # ... so the dataset's view j is written view ORDER[j]
SRN_BOXES = {"obj_b": [(1, 1, 3, 2), (0, 0, 4, 3), (2, 3, 2, 3)],          # (cmin, rmin, cmax, rmax) per written view
             "obj_a": [(0, 1, 0, 2), (3, 0, 4, 0), (1, 1, 2, 2)]}
SRN_INTRINSICS = {"obj_a": (131.25, 2.5, 1.75), "obj_b": (140.5, 2.25, 2.0)}


def _srn_object(name):
    seed = 1 + sorted(SRN_BOXES).index(name)
    images = dt.boxed_views(3, H, W, SRN_BOXES[name], seed)
    if name == "obj_b":
        images[0, 0, 0] = (255, 10, 20)                    # exactly one channel at 255, outside the box: still background
    return images, dt.random_poses(3, 10 + seed)


def _write_srn(root, names=("obj_b", "obj_a")):
    for name in names:
        images, poses = _srn_object(name)
        dt.write_srn_object(os.path.join(root, name), images, poses, *SRN_INTRINSICS[name], STEMS,
                            rgba=(1,) if name == "obj_a" else ())


def _expected_srn(name, world_scale=1.0):
    images, poses = _srn_object(name)
    want = poses[ORDER].copy()
    want[:, :, 1] *= -1.0                                  # pose @ diag(1, -1, -1, 1): columns 1 and 2 change sign
    want[:, :, 2] *= -1.0
    want[:, :3, 3] *= np.float32(world_scale)
    bbox = np.array([SRN_BOXES[name][v] for v in ORDER], np.float32)
    return images[ORDER], want, bbox


@pytest.mark.parametrize("world_scale", [1.0, 0.5])
def test_srn_items_hold_the_stated_values(tmp_path, world_scale):
    from pixel_nerf_multiscale_amd.data import SRNDataset, get_split_dataset
    _write_srn(str(tmp_path / "cars_test"))
    ds = get_split_dataset("srn", str(tmp_path / "cars"), want_split="test", world_scale=world_scale)
    assert isinstance(ds, SRNDataset) and len(ds) == 2
    assert (ds.z_near, ds.z_far, ds.lindisp) == (0.8, 1.8, False) and ds.balanced is True
    for index, name in enumerate(("obj_a", "obj_b")):      # the objects are sorted, not in the order they were written
        item = ds[index]
        images, poses, bbox = _expected_srn(name, world_scale)
        focal, cx, cy = SRN_INTRINSICS[name]
        assert sorted(item) == ["bbox", "c", "focal", "images", "img_id", "masks", "path", "poses"]
        assert item["path"] == str(tmp_path / "cars_test" / name) and item["img_id"] == index
        assert isinstance(item["focal"], float) and item["focal"] == focal * world_scale
        assert item["c"].dtype == torch.float32 and item["c"].tolist() == [cx, cy]
        assert item["poses"].dtype == torch.float32 and np.array_equal(item["poses"].numpy(), poses)
        assert item["bbox"].dtype == torch.float32 and np.array_equal(item["bbox"].numpy(), bbox)
        want = torch.from_numpy(images).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
        assert item["images"].dtype == torch.float32 and torch.equal(item["images"], want)       # the RGBA file lost its alpha
        mask = np.zeros((3, 1, H, W), np.float32)
        for j, (cmin, rmin, cmax, rmax) in enumerate(bbox.astype(int)):
            mask[j, 0, rmin:rmax + 1, cmin:cmax + 1] = 1.0
        assert item["masks"].dtype == torch.float32 and np.array_equal(item["masks"].numpy(), mask)
    assert ds[1]["masks"][ORDER.index(0), 0, 0, 0] == 0.0   # the (255, 10, 20) pixel is background


def test_srn_roots_depth_ranges_and_refusals(tmp_path):
    from pixel_nerf_multiscale_amd.data import SRNDataset, get_split_dataset
    _write_srn(str(tmp_path / "chairs_train" / "chairs_2.0_train"), names=("obj_a",))
    _write_srn(str(tmp_path / "chairs_train"), names=("obj_b",))          # beside the sub-folder: not part of the split
    _write_srn(str(tmp_path / "chairs_val"), names=("obj_b",))
    os.makedirs(str(tmp_path / "chairs_test"))
    train, val, test = get_split_dataset("srn", str(tmp_path / "chairs"))
    assert (train.z_near, train.z_far) == (1.25, 2.75) and (val.z_near, val.z_far) == (1.25, 2.75)
    assert len(train) == 1 and train[0]["path"] == str(tmp_path / "chairs_train" / "chairs_2.0_train" / "obj_a")
    assert len(val) == 1 and val[0]["path"] == str(tmp_path / "chairs_val" / "obj_b") and len(test) == 0
    # without the sub-folder the stage folder itself is the root; a cars name never looks for it
    _write_srn(str(tmp_path / "cars_train" / "chairs_2.0_train"), names=("obj_a",))
    assert len(SRNDataset(str(tmp_path / "cars"), stage="train")) == 0

    # an all-white view has no bounding box
    images, poses = _srn_object("obj_a")
    images[0] = 255                                        # the view written as 9.png
    dt.write_srn_object(str(tmp_path / "white_val" / "o"), images, poses, 100.0, 2.5, 2.0, STEMS)
    with pytest.raises(RuntimeError, match="9.png"):
        SRNDataset(str(tmp_path / "white"), stage="val")[0]
    # more images than poses
    _write_srn(str(tmp_path / "odd_val"), names=("obj_a",))
    os.remove(str(tmp_path / "odd_val" / "obj_a" / "pose" / "10.txt"))
    with pytest.raises(RuntimeError):
        SRNDataset(str(tmp_path / "odd"), stage="val")[0]
    # a foreign image_size would need resampling; the files' own size passes
    with pytest.raises(NotImplementedError):
        SRNDataset(str(tmp_path / "chairs"), stage="val", image_size=(8, 10))[0]
    with pytest.raises(NotImplementedError):
        SRNDataset(str(tmp_path / "chairs"), stage="val", image_size=4)[0]
    assert SRNDataset(str(tmp_path / "chairs"), stage="val", image_size=(H, W))[0]["images"].shape == (3, 3, H, W)


# ------------------------------------------------------------------------------------------------------------------ DVR
CAT_A, CAT_B = "02691156", "02958343"
DVR_BOXES = [(1, 0, 3, 2), (0, 1, 4, 3)]
TW = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
TC = np.diag([1.0, -1.0, -1.0, 1.0])


def _dvr_cameras(seed, NV=2):
    """world_mat_i: invertible 4 x 4 world-to-camera matrices with the bottom row 0 0 0 1; camera_mat_i with fx = fy."""
    rng = np.random.default_rng(seed)
    mats = []
    for _ in range(NV):
        m = np.eye(4)
        m[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        m[:3, 3] = rng.normal(size=3)
        mats.append(m)
    K = np.diag([2.1875, 2.1875, 1.0, 1.0])
    return mats, K


def _write_dvr(root):
    """Category A: softras_train lists inv and raw, softras_val lists skew, gen_train lists raw.  Category B: no softras_
    list at all, gen_train lists other."""
    images = dt.boxed_views(2, H, W, DVR_BOXES, 5)
    masks = np.zeros((2, H, W), np.uint8)
    for v, (cmin, rmin, cmax, rmax) in enumerate(DVR_BOXES):
        masks[v, rmin:rmax + 1, cmin:cmax + 1] = (255, 128)[v]                 # any non-zero value is foreground
    mats, K = _dvr_cameras(3)
    cams = {}
    for i, m in enumerate(mats):
        cams[f"world_mat_{i}"], cams[f"camera_mat_{i}"] = m, K
    with_inv = dict(cams, **{f"world_mat_inv_{i}": np.linalg.inv(m) for i, m in enumerate(mats)})
    only_3x4 = {k: (v[:3] if k.startswith("world_mat_") else v) for k, v in cams.items()}
    skew = dict(cams, camera_mat_1=np.diag([2.1875, 2.25, 1.0, 1.0]))
    dt.write_dvr_object(os.path.join(root, CAT_A, "inv"), images, masks, with_inv)
    dt.write_dvr_object(os.path.join(root, CAT_A, "raw"), images, masks, only_3x4, mask_channels=3)
    dt.write_dvr_object(os.path.join(root, CAT_A, "skew"), images, masks, skew)
    dt.write_dvr_object(os.path.join(root, CAT_B, "other"), images, masks, with_inv)
    for cat, name, lines in ((CAT_A, "softras_train", "inv\nraw\n"), (CAT_A, "softras_val", "skew\n"),
                             (CAT_A, "gen_train", "raw\n\n"), (CAT_B, "gen_train", "other\n")):
        with open(os.path.join(root, cat, name + ".lst"), "w") as f:
            f.write(lines)
    with open(os.path.join(root, "metadata.yaml"), "w") as f:                  # a file beside the categories is no category
        f.write("{}\n")
    return images, masks, mats


def test_dvr_items_lists_and_cameras(tmp_path):
    from pixel_nerf_multiscale_amd.data import DVRDataset, get_split_dataset
    root = str(tmp_path / "NMR")
    images, masks, mats = _write_dvr(root)
    ds = get_split_dataset("dvr", root, want_split="train")
    assert isinstance(ds, DVRDataset) and (ds.z_near, ds.z_far, ds.lindisp) == (1.2, 4.0, False)
    assert ds.all_objs == [(CAT_A, os.path.join(root, CAT_A, "inv")), (CAT_A, os.path.join(root, CAT_A, "raw"))]   # B: no list
    want_pose = np.stack([(TW @ np.linalg.inv(m) @ TC).astype(np.float32) for m in mats])
    want_img = torch.from_numpy(images).permute(0, 3, 1, 2).float().div(255).sub(0.5).div(0.5)
    for index, name in enumerate(("inv", "raw")):          # stored inverse, and 3 x 4 world_mat only: the same cameras
        item = ds[index]
        assert sorted(item) == ["bbox", "focal", "images", "img_id", "masks", "path", "poses"]          # no "c"
        assert item["path"] == os.path.join(root, CAT_A, name) and item["img_id"] == index
        assert item["focal"].dtype == torch.float32 and item["focal"].dim() == 0 and float(item["focal"]) == 2.1875 * W / 2
        assert item["poses"].dtype == torch.float32 and np.array_equal(item["poses"].numpy(), want_pose)
        assert np.array_equal(item["bbox"].numpy(), np.array(DVR_BOXES, np.float32))
        assert torch.equal(item["images"], want_img)
        assert np.array_equal(item["masks"].numpy(), (masks != 0).astype(np.float32)[:, None])
    assert float(DVRDataset(root, stage="train", scale_focal=False)[0]["focal"]) == 2.1875
    with pytest.raises(ValueError):                        # fx != fy in one view
        get_split_dataset("dvr", root, want_split="val")[0]
    gen = get_split_dataset("dvr_gen", root, want_split="train")
    assert gen.all_objs == [(CAT_A, os.path.join(root, CAT_A, "raw")), (CAT_B, os.path.join(root, CAT_B, "other"))]
    assert len(get_split_dataset("dvr_gen", root, want_split="test")) == 0
    triple = get_split_dataset("dvr", root, want_split="all", z_near=0.5)
    assert [len(d) for d in triple] == [2, 1, 0] and triple[0].z_near == 0.5
    with pytest.raises(NotImplementedError):
        get_split_dataset("dvr", root, want_split="train", image_size=(8, 8))[0]
    # more views than max_imgs: a random subset, each view still with its own camera
    np.random.seed(4)
    one = DVRDataset(root, stage="train", max_imgs=1)[0]
    assert one["images"].shape == (1, 3, H, W)
    v = [i for i in range(2) if torch.equal(one["images"][0], want_img[i])]
    assert len(v) == 1 and np.array_equal(one["poses"][0].numpy(), want_pose[v[0]])


def test_refused_dataset_types(tmp_path):
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    with pytest.raises(NotImplementedError, match="cv2"):
        get_split_dataset("dvr_dtu", str(tmp_path))
    with pytest.raises(NotImplementedError, match="multi"):
        get_split_dataset("multi_obj", str(tmp_path))


# ------------------------------------------------------------------------------------------------------- the two item modes
@pytest.mark.parametrize("balanced", [True, False])
def test_byte_items_are_the_float_items(tmp_path, balanced):
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    _write_srn(str(tmp_path / "cars_val"))
    root = str(tmp_path / "NMR")
    _write_dvr(root)
    for kind, path, split in (("srn", str(tmp_path / "cars"), "val"), ("dvr", root, "train")):
        as_float = get_split_dataset(kind, path, want_split=split, balanced=balanced)
        as_bytes = get_split_dataset(kind, path, want_split=split, balanced=balanced, as_bytes=True)
        assert as_bytes.balanced is balanced and as_bytes.as_bytes and not as_float.as_bytes and len(as_bytes) == 2
        for f, b in zip((as_float[i] for i in range(2)), (as_bytes[i] for i in range(2))):
            assert sorted(f) == sorted(b)
            NV = f["images"].shape[0]
            assert b["images"].dtype == torch.uint8 and tuple(b["images"].shape) == (NV, H, W, 3)
            assert b["masks"].dtype == torch.uint8 and tuple(b["masks"].shape) == (NV, H, W)
            assert set(b["masks"].unique().tolist()) <= {0, 255}
            t = b["images"].permute(0, 3, 1, 2).float().div(255)
            if balanced:
                t = t.sub(0.5).div(0.5)
            assert torch.equal(t, f["images"]) and float(f["images"].min()) >= (-1.0 if balanced else 0.0)
            assert torch.equal((b["masks"] != 0).float()[:, None], f["masks"])
            for k in f:
                if k not in ("images", "masks"):
                    same = torch.equal(f[k], b[k]) if torch.is_tensor(f[k]) else f[k] == b[k]
                    assert same, k


def test_default_loader_collates_into_calc_losses_shapes(tmp_path):
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    _write_srn(str(tmp_path / "cars_val"))
    root = str(tmp_path / "NMR")
    _write_dvr(root)
    for kind, path, split, NV in (("srn", str(tmp_path / "cars"), "val", 3), ("dvr", root, "train", 2)):
        for as_bytes in (False, True):
            ds = get_split_dataset(kind, path, want_split=split, as_bytes=as_bytes)
            (batch,) = list(torch.utils.data.DataLoader(ds, batch_size=2, num_workers=0))
            if as_bytes:
                assert batch["images"].dtype == torch.uint8 and tuple(batch["images"].shape) == (2, NV, H, W, 3)
                assert tuple(batch["masks"].shape) == (2, NV, H, W)
            else:
                assert batch["images"].dtype == torch.float32 and tuple(batch["images"].shape) == (2, NV, 3, H, W)
                assert tuple(batch["masks"].shape) == (2, NV, 1, H, W)
            assert tuple(batch["poses"].shape) == (2, NV, 4, 4) and batch["poses"].dtype == torch.float32
            assert tuple(batch["bbox"].shape) == (2, NV, 4) and not batch["bbox"].is_cuda
            assert tuple(batch["focal"].shape) == (2,) and len(batch["path"]) == 2
            assert ("c" in batch) == (kind == "srn")
            if kind == "srn":
                assert tuple(batch["c"].shape) == (2, 2)


def test_resident_split_refuses_what_it_cannot_pool():
    """The refusals come before anything is allocated, so they need no device."""
    from pixel_nerf_multiscale_amd.data import ResidentSplit

    class Items(list):
        as_bytes, balanced, z_near, z_far, lindisp = True, True, 0.8, 1.8, False

    def item(NV):
        return {"path": f"o{NV}", "img_id": 0, "focal": 10.0, "images": torch.zeros(NV, H, W, 3, dtype=torch.uint8),
                "poses": torch.eye(4).repeat(NV, 1, 1), "bbox": torch.zeros(NV, 4)}
    with pytest.raises(ValueError, match="max_bytes"):
        ResidentSplit(Items([item(3), item(3)]), "cuda", max_bytes=2 * 3 * H * W * 3 - 1)
    floats = Items([item(3)])
    floats.as_bytes = False
    with pytest.raises(ValueError, match="as_bytes"):
        ResidentSplit(floats, "cuda")
    with pytest.raises(ValueError):
        ResidentSplit(Items(), "cuda")
