"""Colour jitter on the device against the numpy model of include/pnr.h's section (tests/color_jitter_util.py), bit for bit:
the two jitter gathers under records the test writes, pnr_color_jitter_plan's draws and grey mean, make_batch(jitter=...) on
a host byte batch and on ResidentSplit.batch of a DTU tree without boxes, and a Trainer run with jitter resumed from a
checkpoint; evaluate() on the same tree's test split.

The mean's bound, 1 fp32 ulp of the model's fp64 mean: the device folds the same fp32 greys in fp64 in another order, an error
of at most N * 2^-53 relative — far below half an fp32 ulp — so only the final rounding to fp32 can differ."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import color_jitter_util as cj
import dtu_trees as dtu
import golden_util as gu

pytestmark = pytest.mark.gpu

F = np.float32
Z_NEAR, Z_FAR = 0.75, 3.5
SENTINEL = -777.25
NPX = 97                                                    # the pixel set, one row of a 97 x 1 view
NV = 2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    """torch tensor vs numpy array, NaN payloads included."""
    return np.array_equal(_bits(got.detach().cpu().numpy()), _bits(want))


def _object(C):
    """(NV, 1, 97, C) uint8: view 0 the pixel set, view 1 the pixel set darkened; a fourth channel holds other bytes."""
    px = cj.pixel_set()
    obj = np.stack([px[None], (px // 3)[None]])
    if C == 4:
        obj = np.concatenate([obj, (255 - obj[..., :1])], axis=-1)
    return obj


def _at_offset(arr, off):
    """The bytes of a numpy uint8 array `off` bytes into a larger device allocation, as a tensor of its shape."""
    flat = torch.from_numpy(np.ascontiguousarray(arr).reshape(-1))
    big = torch.zeros(flat.numel() + 8, dtype=torch.uint8, device="cuda")
    big[off:off + flat.numel()] = flat.cuda()
    view = big[off:off + flat.numel()].view(arr.shape)
    assert view.data_ptr() % 4 == off % 4
    return view


def _cams(SB):
    poses = torch.from_numpy(np.stack([np.stack([gu.pose_spherical(31.0 * v + 17.0 * o, -25.0 + 6.0 * v, 1.9) for v in range(NV)])
                                       for o in range(SB)])).float().cuda()
    focal = torch.tensor([[90.0 + o, 70.0 - o] for o in range(SB)]).cuda()
    c = torch.tensor([[48.375, 0.25 + 0.125 * (o % 3)] for o in range(SB)]).cuda()
    return poses, focal, c


# ------------------------------------------------------------------------------------------------------------ gathers
@pytest.fixture(scope="module")
def gather_model():
    """Per C: the records (24 orders and an identity, means from the model) and, per (object, balanced), the model's colours of
    all 2 x 97 pixels — computed once, read by every gather case."""
    out = {}
    for C in (3, 4):
        obj = _object(C)
        recs = np.stack([cj.with_mean(r, obj) for r in cj.written_records()])
        flat = obj[..., :3].reshape(-1, 3)
        rgb = {(o, b): cj.model_rgb_gt(flat, recs[o], b) for o in range(len(recs)) for b in (0, 1)}
        planes = {(o, v, b): cj.model_views(obj[v], recs[o], b) for o in range(len(recs)) for v in range(NV) for b in (0, 1)}
        out[C] = (obj, recs, rgb, planes)
    return out


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("balanced", [1, 0])
@pytest.mark.parametrize("C", [3, 4])
def test_jitter_gathers_equal_the_model(gather_model, C, balanced, off):
    from pixel_nerf_multiscale_amd import _native as N, util
    obj, recs, rgb_model, plane_model = gather_model[C]
    SB, n = len(recs), NV * NPX
    assert SB == 25 and recs[-1].tolist()[:4] == [1, 1, 1, 0]
    images = _at_offset(np.broadcast_to(obj, (SB,) + obj.shape), off)
    rec_d = torch.from_numpy(recs).cuda()
    poses, focal, c = _cams(SB)
    stream = N.current_stream(images.device)

    # ---- the training batch: every pixel of both views, then -1 and NV H W
    inds = torch.cat([torch.arange(n), torch.tensor([-1, n])]).repeat(SB, 1)
    inds = torch.stack([row.roll(o) for o, row in enumerate(inds)])
    ok = (inds >= 0) & (inds < n)
    B = inds.shape[1]
    inds_d = inds.cuda()
    rays0, rgb0 = util.train_batch_u8(images, poses, focal, c, inds_d, Z_NEAR, Z_FAR, balanced=bool(balanced))
    want = np.stack([rgb_model[(o, balanced)][inds[o].clamp(0, n - 1).numpy()] for o in range(SB)])
    for lead in (4, 1):
        rbuf = torch.full((SB * B * 8 + 2 * lead + 8,), SENTINEL, device="cuda")
        gbuf = torch.full((SB * B * 3 + 2 * lead + 8,), SENTINEL, device="cuda")
        rc = N.lib.pnr_train_batch_u8_jitter(images.data_ptr(), poses.data_ptr(), focal.data_ptr(), c.data_ptr(), SB, NV, NPX, 1, Z_NEAR,
                                             Z_FAR, inds_d.data_ptr(), B, rbuf.data_ptr() + 4 * lead, gbuf.data_ptr() + 4 * lead, C,
                                             balanced, rec_d.data_ptr(), stream)
        assert rc == 0
        rbuf, gbuf = rbuf.cpu(), gbuf.cpu()
        rays, rgb = rbuf[lead:lead + SB * B * 8].view(SB, B, 8), gbuf[lead:lead + SB * B * 3].view(SB, B, 3)
        assert torch.equal(rays[ok], rays0.cpu()[ok])                           # the rays of the entry point without a record
        assert bool(torch.isnan(rays[~ok]).all()) and bool(torch.isnan(rgb[~ok]).all()) and int((~ok).sum()) == 2 * SB
        assert np.array_equal(_bits(rgb.numpy())[ok.numpy()], _bits(want)[ok.numpy()])
        assert torch.equal(rgb[-1][ok[-1]], rgb0.cpu()[-1][ok[-1]])             # the identity record: the bits without a record
        assert not torch.equal(rgb[0][ok[0]], rgb0.cpu()[0][ok[0]])
        assert bool((rbuf[:lead] == SENTINEL).all()) and bool((rbuf[lead + SB * B * 8:] == SENTINEL).all())
        assert bool((gbuf[:lead] == SENTINEL).all()) and bool((gbuf[lead + SB * B * 3:] == SENTINEL).all())
    r2, g2 = util.train_batch_u8(images, poses, focal, c, inds_d, Z_NEAR, Z_FAR, balanced=bool(balanced), jitter=rec_d)
    assert _same_bits(r2, rays.numpy()) and _same_bits(g2, rgb.numpy())

    # ---- the source views: both views, a bad index each way, a repeated view
    ords = torch.tensor([[0, 1, -1, 0] if o % 2 == 0 else [1, NV, 0, 1] for o in range(SB)])
    NS = ords.shape[1]
    ords_d = ords.cuda()
    plain = util.views_to_tensor_u8(images, ords_d, balanced=bool(balanced)).cpu()
    size = SB * NS * 3 * NPX
    for lead in (4, 1):
        buf = torch.full((size + 2 * lead + 8,), SENTINEL, device="cuda")
        rc = N.lib.pnr_views_to_tensor_u8_jitter(images.data_ptr(), ords_d.data_ptr(), SB, NV, NS, NPX, 1, C, balanced,
                                                 buf.data_ptr() + 4 * lead, rec_d.data_ptr(), stream)
        assert rc == 0
        buf = buf.cpu()
        got = buf[lead:lead + size].view(SB, NS, 3, 1, NPX)
        assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + size:] == SENTINEL).all())
        for o in range(SB):
            for j, v in enumerate(ords[o].tolist()):
                if 0 <= v < NV:
                    assert np.array_equal(_bits(got[o, j].numpy()), _bits(plane_model[(o, v, balanced)])), (o, j, v)
                else:
                    assert bool(torch.isnan(got[o, j]).all())
        assert _same_bits(got[-1], plain[-1].numpy())                           # identity record
    v2 = util.views_to_tensor_u8(images, ords_d, balanced=bool(balanced), jitter=rec_d)
    assert _same_bits(v2, got.numpy())


@pytest.mark.parametrize("C", [3, 4])
def test_identity_records_give_the_bits_without_a_record(C):
    """Every object under the identity record, images of 8 x 4 pixels (whole pixel groups, float4 stores): all outputs of both
    gathers equal the entry points without a record, NaN rows and planes included."""
    from pixel_nerf_multiscale_amd import util
    SB, H, W = 3, 4, 8
    u8 = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (SB, NV, H, W, C), dtype=np.uint8)).cuda()
    rec = torch.tensor([[1, 1, 1, 0, 0.25, q, 0, 0] for q in (0, 13, 23)], dtype=torch.float32).cuda()
    poses, focal, c = _cams(SB)
    n = NV * H * W
    inds = torch.cat([torch.arange(n), torch.tensor([-1, n])]).repeat(SB, 1).cuda()
    ords = torch.tensor([[0, 1], [1, -1], [NV, 0]]).cuda()
    for balanced in (True, False):
        a = util.train_batch_u8(u8, poses, focal, c, inds, Z_NEAR, Z_FAR, balanced=balanced)
        b = util.train_batch_u8(u8, poses, focal, c, inds, Z_NEAR, Z_FAR, balanced=balanced, jitter=rec)
        assert _same_bits(b[0], a[0].cpu().numpy()) and _same_bits(b[1], a[1].cpu().numpy())
        va = util.views_to_tensor_u8(u8, ords, balanced=balanced)
        vb = util.views_to_tensor_u8(u8, ords, balanced=balanced, jitter=rec)
        assert _same_bits(vb, va.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------ the plan
RANGES = (0.4, 0.3, 0.5, 0.2)


def _seed_with_contrast_at(pos, base):
    """The first seed >= base under which object 0's order has contrast at position `pos` (host model)."""
    for seed in range(base, base + 400):
        if cj.order_of(int(cj.draw_records(seed, 1, RANGES)[0, 5])).index(cj.CONTRAST) == pos:
            return seed
    raise AssertionError("no such seed")


def _check_records(got, images_np, seed, ranges, SB):
    """got (SB, 8) from the device: factors and order bit for bit the host draws, mean within 1 fp32 ulp of the model's."""
    want = cj.draw_records(seed, SB, ranges)
    assert np.array_equal(_bits(got[:, :4]), _bits(want[:, :4])) and np.array_equal(got[:, 5], want[:, 5])
    assert (got[:, 6:] == 0).all()
    worst = 0.0
    for o in range(SB):
        if want[o, 1] == 1:
            assert got[o, 4] == 0
            continue
        m = cj.mean64(images_np[o], want[o])
        worst = max(worst, abs(float(got[o, 4]) - m) / cj.ulp32(m))
    assert worst <= 1.0, worst
    return worst


JB = 4096                                                   # PNR_JITTER_BLOCK (asserted against the package below)
PLAN_SHAPES = [(1, 1, 1), (1, 1, JB - 1), (1, 1, JB), (1, 1, JB + 1), (1, 1, 2 * JB + 3), (3, 5, 7)]


@pytest.mark.parametrize("SB", [1, 3])
@pytest.mark.parametrize("nv,H,W", PLAN_SHAPES)
def test_plan_equals_the_model(nv, H, W, SB):
    """Contrast at each of the four positions of object 0's order; C = 3 at offset 0 and C = 4 at byte offset 1."""
    from pixel_nerf_multiscale_amd import _native as N, util
    assert JB == N.PNR_JITTER_BLOCK
    rng = np.random.default_rng(nv * H * W + SB)
    worst = 0.0
    for pos in range(4):
        seed = _seed_with_contrast_at(pos, 1000 * pos + 17)
        C, off = (3, 0) if pos % 2 == 0 else (4, 1)
        images_np = rng.integers(0, 256, (SB, nv, H, W, C), dtype=np.uint8)
        images = _at_offset(images_np, off)
        got = util.color_jitter_plan(images, RANGES, seed)
        again = util.color_jitter_plan(images, RANGES, seed)
        assert torch.equal(got, again) and tuple(got.shape) == (SB, 8)
        g = got.cpu().numpy()
        assert cj.order_of(int(g[0, 5])).index(cj.CONTRAST) == pos
        worst = max(worst, _check_records(g, images_np, seed, RANGES, SB))
        if SB > 1:                                          # object 1's bytes do not enter object 0's record
            other = images_np.copy()
            other[1] = 255 - other[1]
            g2 = util.color_jitter_plan(_at_offset(other, off), RANGES, seed).cpu().numpy()
            assert np.array_equal(_bits(g2[0]), _bits(g[0])) and np.array_equal(_bits(g2[2]), _bits(g[2]))
            assert g2[1, 4] != g[1, 4] and np.array_equal(_bits(g2[1, :4]), _bits(g[1, :4]))
    print(f"plan {nv} x {H} x {W}, SB {SB}: worst mean error {worst:.3f} ulp")


def test_plan_without_contrast_launches_no_reduction():
    """A contrast range of 0: every contrast factor is exactly 1, the mean is 0, and neither the images nor a workspace is
    looked at (both NULL here)."""
    from pixel_nerf_multiscale_amd import _native as N, util
    import ctypes
    SB = 3
    rec = torch.full((SB, 8), SENTINEL, device="cuda")
    ranges = (0.4, 0.0, 0.5, 0.2)
    rc = N.lib.pnr_color_jitter_plan(None, SB, 2, 8, 4, 3, (ctypes.c_float * 4)(*ranges), 99, rec.data_ptr(), None, 0,
                                     N.current_stream(rec.device))
    assert rc == 0
    g = rec.cpu().numpy()
    want = cj.draw_records(99, SB, ranges)
    assert np.array_equal(_bits(g), _bits(want)) and (g[:, 1] == 1).all() and (g[:, 4] == 0).all()
    u8 = torch.zeros(SB, 2, 4, 8, 3, dtype=torch.uint8, device="cuda")
    assert torch.equal(util.color_jitter_plan(u8, ranges, 99), rec)
    out = torch.empty(SB, 8, device="cuda")
    assert util.color_jitter_plan(u8, ranges, 99, out=out) is out and torch.equal(out, rec)


# ------------------------------------------------------------------------------------------------------------ DTU tree
W16 = H16 = 16
NV3, SBT, RAYS, NVIEWS = 3, 2, 32, [1, 2]
K16 = dtu.intrinsics(16.5, 15.0, 8.3, 7.6)


@pytest.fixture(scope="module")
def dtu_tree(tmp_path_factory):
    """4 training, 2 validation and 2 test scans x 3 views of 16 x 16 pixels, no masks; cameras on a sphere of radius 1.3."""
    root = tmp_path_factory.mktemp("dtu16")
    cat = root / "scans"
    names = {"train": [f"scan{o}" for o in range(4)], "val": ["scan4", "scan5"], "test": ["scan6", "scan7"]}
    for o in range(8):
        images, _, _ = dtu.boxed_scan_images(NV3, H16, W16, seed=40 + o, margin=2)
        cams = {}
        for v in range(NV3):
            R, C = dtu.camera_of_pose(gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3))
            cams[f"world_mat_{v}"] = dtu.world_mat(K16, R, C, -1.5 if v == 1 else 2.0)
        dtu.write_scan(str(cat / f"scan{o}"), images, cams)
    dtu.write_lists(str(cat), names)
    return str(root)


def _byte_batch(seed=0):
    rng = np.random.default_rng(seed)
    images = torch.from_numpy(rng.integers(0, 256, (SBT, NV3, H16, W16, 3), dtype=np.uint8))
    poses = torch.from_numpy(np.stack([np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(NV3)])
                                       for o in range(SBT)])).float()
    return {"images": images, "poses": poses, "focal": torch.tensor([[16.5, 15.0], [17.0, 14.0]]),
            "c": torch.tensor([[8.3, 7.6], [7.9, 8.2]])}


def _check_make_batch(data, images_np):
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.data import ColorJitter
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    jit = ColorJitter()
    kw = dict(ray_batch_size=RAYS, nviews=[2], z_near=0.1, z_far=5.0, balanced=True, draws="device")
    key, key2 = frame_seed(5, 3), frame_seed(5, 4)
    SB = images_np.shape[0]
    out = train.make_batch(data, "cuda", seed=key, jitter=jit, **kw)
    again = train.make_batch(data, "cuda", seed=key, jitter=jit, **kw)
    plain = train.make_batch(data, "cuda", seed=key, **kw)
    assert len(out) == 6
    for a, b in zip(out, again):
        assert torch.equal(a, b)
    for k in (0, 3, 4, 5):                                  # rays, source poses, focal, c: untouched by the augmentation
        assert torch.equal(out[k], plain[k])
    # the record the step's plan wrote, and the draws of the step
    dev_images = data["images"].cuda()
    rec = util.color_jitter_plan(dev_images, jit, key).cpu().numpy()
    _check_records(rec, images_np, key, jit.ranges, SB)
    assert not np.array_equal(rec, util.color_jitter_plan(dev_images, jit, key2).cpu().numpy())
    pix, order = util.train_draw(data.get("bbox_dev"), SB, NV3, W16, H16, RAYS, 2, key)
    pix, order = pix.cpu().numpy(), order.cpu().numpy()
    for o in range(SB):
        flat = images_np[o].reshape(-1, 3)
        assert np.array_equal(_bits(out[1][o].cpu().numpy()), _bits(cj.model_rgb_gt(flat[pix[o]], rec[o], 1)))
        for j in range(2):
            assert np.array_equal(_bits(out[2][o, j].cpu().numpy()), _bits(cj.model_views(images_np[o, order[o, j]], rec[o], 1)))
    assert not torch.equal(out[1], plain[1]) and not torch.equal(out[2], plain[2])
    # jitter=None: the calls and the bits of the gathers without a record
    focal, c = plain[4], plain[5]
    rays, rgb = util.train_batch_u8(dev_images, data["poses"].cuda(), focal, c, torch.from_numpy(pix).cuda(), 0.1, 5.0, balanced=True)
    assert torch.equal(plain[0], rays) and torch.equal(plain[1], rgb)
    assert torch.equal(plain[2], util.views_to_tensor_u8(dev_images, torch.from_numpy(order).cuda(), balanced=True))
    # evaluation ignores it
    ev = train.make_batch(data, "cuda", seed=key, jitter=jit, is_train=False, **kw)
    ev0 = train.make_batch(data, "cuda", seed=key, is_train=False, **kw)
    for a, b in zip(ev, ev0):
        assert torch.equal(a, b)
    return jit, kw, key


def test_make_batch_with_jitter_on_a_host_byte_batch():
    from pixel_nerf_multiscale_amd import train
    data = _byte_batch()
    jit, kw, key = _check_make_batch(data, data["images"].numpy())
    floats = dict(data, images=torch.zeros(SBT, NV3, 3, H16, W16))
    with pytest.raises(ValueError, match="jitter"):
        train.make_batch(floats, "cuda", seed=key, jitter=jit, **kw)
    with pytest.raises(ValueError, match="jitter"):
        train.make_batch(data, "cuda", jitter=jit, **dict(kw, draws="host"))
    assert len(train.make_batch(floats, "cuda", seed=key, jitter=jit, is_train=False, **kw)) == 6


def test_make_batch_with_jitter_on_a_resident_dtu_split(dtu_tree):
    from pixel_nerf_multiscale_amd.data import ResidentSplit, get_split_dataset
    ds = get_split_dataset("dtu", dtu_tree, want_split="train", as_bytes=True)
    assert len(ds) == 4 and ds.max_imgs == 49 and "bbox" not in ds[0]
    with pytest.raises(ValueError, match="bbox"):
        ResidentSplit(ds, "cuda", device_boxes=True)
    split = ResidentSplit(ds, "cuda")
    assert split.bbox is None and split.bbox_dev is None and tuple(split.images.shape) == (4, NV3, H16, W16, 3)
    assert tuple(split.focal.shape) == (4, 2) and tuple(split.c.shape) == (4, 2) and (split.z_near, split.z_far) == (0.1, 5.0)
    data = split.batch([2, 0])
    assert "bbox" not in data and "bbox_dev" not in data and data["images"].is_cuda and not data["focal"].is_cuda
    assert sorted(data) == ["c", "focal", "images", "img_id", "path", "poses"]
    images_np = np.stack([ds[2]["images"].numpy(), ds[0]["images"].numpy()])
    assert np.array_equal(data["images"].cpu().numpy(), images_np)
    _check_make_batch(data, images_np)
    assert len(list(split.batches(2, shuffle=False))) == 2


# ------------------------------------------------------------------------------------------------------------ Trainer
@pytest.fixture()
def deterministic_convolutions():
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


def _trainer(root, train_data, val_data, **kw):
    from test_gpu_trainer import _model
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend = _model()
    conf = dict(name="run", checkpoints_path=os.path.join(root, "ckpt"), logs_path=os.path.join(root, "logs"), batch_size=SBT,
                ray_batch_size=RAYS, nviews=NVIEWS, loss=RenderLoss(1.0, 1.0), num_epochs=2, print_interval=1, seed=5)
    conf.update(kw)
    with contextlib.redirect_stdout(io.StringIO()):
        return train.Trainer(net, rend, train_data, val_data, **conf)


def _start(t):
    with contextlib.redirect_stdout(io.StringIO()):
        t.start()
    return t


def test_a_resumed_run_with_jitter_continues_bit_for_bit(dtu_tree, tmp_path, deterministic_convolutions):
    """Run A: two epochs with jitter.  Run B: one epoch, then a new Trainer resumes from latest.pth.  Every parameter and both
    Adam moments agree exactly: the records depend on the step's key and the bytes only.  A run without jitter differs."""
    from test_gpu_trainer import _assert_same, _state
    from pixel_nerf_multiscale_amd.data import ColorJitter, get_split_dataset
    train_set = get_split_dataset("dtu", dtu_tree, want_split="train", as_bytes=True)
    val_set = get_split_dataset("dtu", dtu_tree, want_split="val", as_bytes=True, training=False)
    jit = ColorJitter()
    with pytest.raises(ValueError, match="jitter"):
        _trainer(str(tmp_path / "x"), train_set, None, jitter=jit, draws="host")
    a = _start(_trainer(str(tmp_path / "a"), train_set, val_set, jitter=jit, eval_interval=1))
    assert np.isfinite(a.best_val_loss)                     # validation ran, without the augmentation
    b1 = _start(_trainer(str(tmp_path / "b"), train_set, val_set, jitter=jit, num_epochs=1, eval_interval=1))
    b2 = _trainer(str(tmp_path / "b"), train_set, val_set, jitter=jit, resume=True, eval_interval=1)
    assert (b2.epoch, b2.global_step) == (1, 2)
    _assert_same(_state(b1), _state(b2))
    _start(b2)
    sa, sb = _state(a), _state(b2)
    assert sa[3] == 4 and sa[4] == 4
    _assert_same(sa, sb)
    plain = _state(_start(_trainer(str(tmp_path / "c"), train_set, None)))
    assert any(not torch.equal(plain[0][k], sa[0][k]) for k in sa[0])


def test_evaluate_takes_the_dtu_test_split(dtu_tree, tmp_path):
    """evaluate() end to end on the tree's test split, with the dataset's focal (2,) and c."""
    from test_gpu_trainer import _model
    from pixel_nerf_multiscale_amd import evalio
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    dataset = get_split_dataset("dtu", dtu_tree, want_split="test", training=False)
    item = dataset[0]
    assert len(dataset) == 2 and tuple(item["focal"].shape) == (2,) and tuple(item["c"].shape) == (2,)
    assert abs(float(item["focal"][0]) - 16.5) <= 1e-4 and abs(float(item["c"][1]) - 7.6) <= 1e-4
    net, rend = _model()
    net.eval(); rend.eval()
    out = str(tmp_path / "eval_out")
    m = evalio.evaluate(net, rend, dataset, out, source="0", verbose=False, seed=5, metrics="device")
    rows = [x.split() for x in open(os.path.join(out, "finish.txt")).read().split("\n") if x]
    assert [r[0] for r in rows] == ["scan6", "scan7"] and m[2] == 2
    assert all(np.isfinite(float(r[1])) and np.isfinite(float(r[2])) for r in rows)
    assert len(os.listdir(os.path.join(out, "scan6"))) == NV3 - 1
