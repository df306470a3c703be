"""The data layer on the device: pnr_train_batch_u8 and pnr_views_to_tensor_u8 against torch's arithmetic on the CPU and
against the fp32 entry points they stand in for (torch.equal throughout: every contract here is bit-exact), the byte batch
through make_batch / calc_losses, ResidentSplit, and evaluate() on an SRN folder."""
import os

import numpy as np
import pytest
import torch

import data_trees as dt
import golden_util as gu

pytestmark = pytest.mark.gpu

SB, NV, NS = 2, 3, 4
Z_NEAR, Z_FAR = 0.75, 3.5
SENTINEL = -777.25
SIZES = [(1, 1), (5, 3), (4, 4), (67, 2)]                  # W x H: see each test for what a size is there for


def _tensor_cpu(u8, balanced):
    """T(b, balanced) in torch's own arithmetic on the CPU."""
    t = u8.float().div(255.0)
    return t.sub(0.5).div(0.5) if balanced else t


def _case(W, H, C):
    """Host side of one shape: bytes (SB, NV, H, W, C) that run through all 256 values, cameras with fx != fy and an
    off-centre c per object."""
    n = SB * NV * H * W * C
    j = torch.arange(n, dtype=torch.int64)
    flat = ((j * 7 + 3 + j // 256) % 256).to(torch.uint8)                       # the shift per 256 bytes: with C = 4 the three
                                                                               # kept channels still meet every value
    poses = torch.from_numpy(np.stack([np.stack([gu.pose_spherical(31.0 * v + 17.0 * o, -25.0 + 6.0 * v, 1.9)
                                                 for v in range(NV)]) for o in range(SB)])).float()
    focal = torch.tensor([[1.3 * W + 2.0, 1.7 * W + 3.0], [2.1 * W + 1.0, 1.1 * W + 4.0]])
    c = torch.tensor([[0.5 * W + 0.375, 0.5 * H - 0.25], [0.5 * W - 0.625, 0.5 * H + 0.125]])
    return flat, flat.view(SB, NV, H, W, C), poses, focal, c


def _indices(W, H, B):
    """(SB, B) pixel indices: the first and last pixel of the first and last view, then -1 and NV H W, then draws."""
    n = NV * H * W
    if B == 1:
        return torch.tensor([[n - 1], [0]])
    head = torch.tensor([0, H * W - 1, (NV - 1) * H * W, n - 1, -1, n])
    g = torch.Generator().manual_seed(5 + W)
    rows = [torch.cat([head.roll(o), torch.randint(0, n, (B - head.numel(),), generator=g)]) for o in range(SB)]
    return torch.stack(rows)


def _at_offset(flat, off, shape):
    """The bytes of `flat` placed `off` bytes into a larger device allocation, as a tensor of `shape`."""
    big = torch.zeros(flat.numel() + 8, dtype=torch.uint8, device="cuda")
    big[off:off + flat.numel()] = flat.cuda()
    view = big[off:off + flat.numel()].view(shape)
    assert view.data_ptr() % 4 == off % 4
    return view


@pytest.mark.parametrize("balanced", [1, 0])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("W,H", SIZES)
def test_train_batch_u8(W, H, C, balanced):
    """5 x 3: a view is 45 (C = 3) bytes, so pixels and views start at every byte phase; 67 x 2 holds every byte value; B = 257
    passes one 256-thread workgroup.  Colours against 0.5 T + 0.5 from torch on the CPU, rays against pnr_train_batch on the
    float image, the buffer at offsets 0..3 of a larger allocation, outputs inside sentinel margins."""
    from pixel_nerf_multiscale_amd import _native as N, util
    flat, u8, poses, focal, c = _case(W, H, C)
    if (W, H) == (67, 2):
        assert len(set(u8[..., :3].reshape(-1).tolist())) == 256
    T = _tensor_cpu(u8[..., :3], balanced)                                     # (SB, NV, H, W, 3)
    colours = (0.5 * T + 0.5).reshape(SB, NV * H * W, 3)
    images_f32 = T.permute(0, 1, 4, 2, 3).contiguous().cuda()
    poses_d, focal_d, c_d = poses.cuda(), focal.cuda(), c.cuda()
    n = NV * H * W
    for B in (1, 257):
        inds = _indices(W, H, B)
        ok = (inds >= 0) & (inds < n)
        assert B == 1 or int((~ok).sum()) == 2 * SB
        inds_d = inds.cuda()
        rays_f32, rgb_f32 = util.train_batch(images_f32, poses_d, focal_d, c_d, inds_d, Z_NEAR, Z_FAR)
        want_rgb = torch.stack([colours[o][inds[o].clamp(0, n - 1)] for o in range(SB)])
        for off in range(4):
            src = _at_offset(flat, off, u8.shape)
            rays, rgb = util.train_batch_u8(src, poses_d, focal_d, c_d, inds_d, Z_NEAR, Z_FAR, balanced=bool(balanced))
            rays, rgb = rays.cpu(), rgb.cpu()
            assert torch.equal(rays[ok], rays_f32.cpu()[ok]) and torch.equal(rgb[ok], want_rgb[ok])
            assert torch.equal(rgb[ok], rgb_f32.cpu()[ok])
            assert bool(torch.isnan(rays[~ok]).all()) and bool(torch.isnan(rgb[~ok]).all())
            assert not bool(torch.isnan(rays[ok]).any())
            # the raw entry point, outputs inside larger buffers: rays 16-byte aligned (float4 stores) and not (scalar)
            for lead in (4, 1):
                rbuf = torch.full((SB * B * 8 + 2 * lead + 8,), SENTINEL, device="cuda")
                gbuf = torch.full((SB * B * 3 + 2 * lead + 8,), SENTINEL, device="cuda")
                rc = N.lib.pnr_train_batch_u8(src.data_ptr(), poses_d.data_ptr(), focal_d.data_ptr(), c_d.data_ptr(), SB, NV, W, H,
                                              Z_NEAR, Z_FAR, inds_d.data_ptr(), B, rbuf.data_ptr() + 4 * lead,
                                              gbuf.data_ptr() + 4 * lead, C, balanced, N.current_stream(rbuf.device))
                assert rc == 0
                rbuf, gbuf = rbuf.cpu(), gbuf.cpu()
                got_r, got_g = rbuf[lead:lead + SB * B * 8].view(SB, B, 8), gbuf[lead:lead + SB * B * 3].view(SB, B, 3)
                assert torch.equal(got_r[ok], rays[ok]) and torch.equal(got_g[ok], rgb[ok])
                assert bool(torch.isnan(got_r[~ok]).all()) and bool(torch.isnan(got_g[~ok]).all())
                assert bool((rbuf[:lead] == SENTINEL).all()) and bool((rbuf[lead + SB * B * 8:] == SENTINEL).all())
                assert bool((gbuf[:lead] == SENTINEL).all()) and bool((gbuf[lead + SB * B * 3:] == SENTINEL).all())
    # rays alone: no images, no colours
    rbuf = torch.full((SB * 8,), SENTINEL, device="cuda")
    one = _indices(W, H, 1).cuda()
    assert N.lib.pnr_train_batch_u8(None, poses_d.data_ptr(), focal_d.data_ptr(), None, SB, NV, W, H, Z_NEAR, Z_FAR, one.data_ptr(),
                                    1, rbuf.data_ptr(), None, C, balanced, N.current_stream(rbuf.device)) == 0
    want, _ = util.train_batch(images_f32, poses_d, focal_d, None, one, Z_NEAR, Z_FAR)
    assert torch.equal(rbuf.view(SB, 1, 8), want)


@pytest.mark.parametrize("balanced", [1, 0])
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("W,H", SIZES)
def test_views_to_tensor_u8(W, H, C, balanced):
    """4 x 4: whole pixel groups, and at offset 0 every view starts on a dword (the dword route; offsets 1..3 take the byte
    route); 5 x 3 and 67 x 2: views at every byte phase, a tail behind the last whole group, 67 past one wave's row; 1 x 1: a
    tail only.  Per view against util.image_to_tensor and torch's division on the CPU; -1 and NV give NaN planes; a view may
    repeat; `out` inside sentinel margins, 16-byte aligned (float4 stores) and not."""
    from pixel_nerf_multiscale_amd import _native as N, util
    flat, u8, _, _, _ = _case(W, H, C)
    T = _tensor_cpu(u8[..., :3], balanced).permute(0, 1, 4, 2, 3).contiguous()             # (SB, NV, 3, H, W)
    ords = torch.tensor([[0, NV - 1, -1, 0], [NV, 1, 1, NV - 1]])
    live = (ords >= 0) & (ords < NV)
    want = torch.stack([T[o][ords[o].clamp(0, NV - 1)] for o in range(SB)])                 # (SB, NS, 3, H, W)
    ords_d = ords.cuda()
    per_view = {(o, v): util.image_to_tensor(u8[o, v, :, :, :3].contiguous(), balanced=bool(balanced)).cpu()
                for o in range(SB) for v in range(NV)}
    numel = SB * NS * 3 * H * W
    for off in range(4):
        src = _at_offset(flat, off, u8.shape)
        got = util.views_to_tensor_u8(src, ords_d, balanced=bool(balanced)).cpu()
        assert tuple(got.shape) == (SB, NS, 3, H, W) and got.dtype == torch.float32
        assert torch.equal(got[live], want[live]) and bool(torch.isnan(got[~live]).all()) and not bool(torch.isnan(got[live]).any())
        for o in range(SB):
            for j in range(NS):
                if live[o, j]:
                    assert torch.equal(got[o, j], per_view[(o, int(ords[o, j]))])
        for lead in (4, 5):
            buf = torch.full((numel + 2 * lead + 8,), SENTINEL, device="cuda")
            rc = N.lib.pnr_views_to_tensor_u8(src.data_ptr(), ords_d.data_ptr(), SB, NV, NS, W, H, C, balanced,
                                              buf.data_ptr() + 4 * lead, N.current_stream(buf.device))
            assert rc == 0
            buf = buf.cpu()
            raw = buf[lead:lead + numel].view(SB, NS, 3, H, W)
            assert torch.equal(raw[live], got[live]) and bool(torch.isnan(raw[~live]).all())
            assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + numel:] == SENTINEL).all())


# --------------------------------------------------------------------------------------------- make_batch, three ways
class _Items(list):
    """An as_bytes dataset as ResidentSplit takes it."""
    as_bytes, z_near, z_far, lindisp = True, Z_NEAR, Z_FAR, False


def _byte_objects(n_obj, n_views, H, W, seed):
    rng = np.random.default_rng(seed)
    items = []
    for o in range(n_obj):
        images = torch.from_numpy(rng.integers(0, 256, (n_views, H, W, 3), dtype=np.uint8))
        poses = torch.from_numpy(np.stack([gu.pose_spherical(25.0 * v + 40.0 * o, -20.0 - 4.0 * v, 2.0) for v in range(n_views)])).float()
        bbox = torch.tensor([[2.0 + o, 1.0, W - 3.0, H - 2.0 - o]] * n_views)
        items.append({"path": f"/data/cat/obj{o}", "img_id": o, "focal": 18.0 + 1.5 * o,
                      "c": torch.tensor([0.5 * W + 0.25 - o, 0.5 * H - 0.5 + o]), "images": images,
                      "masks": torch.zeros(n_views, H, W, dtype=torch.uint8), "bbox": bbox, "poses": poses})
    return items


@pytest.mark.parametrize("with_bbox", [True, False])
@pytest.mark.parametrize("nviews", [[1], [2]])
def test_make_batch_three_ways(nviews, with_bbox):
    """The byte batch, the float batch built from it on the CPU, and ResidentSplit.batch of the same objects: the same draws
    (one seed) and the same bits in all six outputs."""
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    balanced = nviews == [2]                                 # both conventions over the cases
    items = _Items(_byte_objects(3, 4, 12, 16, seed=9))
    items.balanced = balanced
    ids = [2, 0]
    host = {k: torch.stack([torch.as_tensor(items[i][k]) for i in ids]) for k in ("images", "poses", "bbox", "focal", "c")}
    as_float = dict(host, images=_tensor_cpu(host["images"], balanced).permute(0, 1, 4, 2, 3).contiguous())
    split = ResidentSplit(items, "cuda")
    assert len(split) == 3 and split.nbytes == 3 * 4 * 12 * 16 * 3 and split.balanced is balanced
    resident = split.batch(ids)
    assert resident["images"].is_cuda and resident["images"].dtype == torch.uint8 and resident["poses"].is_cuda
    assert not resident["bbox"].is_cuda and not resident["focal"].is_cuda and not resident["c"].is_cuda
    assert torch.equal(resident["images"].cpu(), host["images"]) and resident["path"] == ["/data/cat/obj2", "/data/cat/obj0"]
    assert [b["img_id"].tolist() for b in split.batches(2, shuffle=False)] == [[0, 1]]
    assert sorted(sum((b["img_id"].tolist() for b in split.batches(2, drop_last=False, generator=torch.Generator().manual_seed(1))),
                      [])) == [0, 1, 2]

    outs = []
    for data in (host, as_float, resident):
        if not with_bbox:
            data = {k: v for k, v in data.items() if k != "bbox"}
        torch.manual_seed(21); np.random.seed(21)
        outs.append(train.make_batch(data, torch.device("cuda"), ray_batch_size=37, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR,
                                     use_bbox=with_bbox, balanced=balanced))
    rays, rgb, src_images, src_poses, focal, c = outs[0]
    assert tuple(rays.shape) == (2, 37, 8) and tuple(rgb.shape) == (2, 37, 3) and tuple(src_images.shape) == (2, nviews[0], 3, 12, 16)
    assert tuple(src_poses.shape) == (2, nviews[0], 4, 4) and not bool(torch.isnan(rays).any()) and not bool(torch.isnan(rgb).any())
    assert float(src_images.min()) >= (-1.0 if balanced else 0.0) and float(src_images.max()) <= 1.0
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert a.dtype == b.dtype and torch.equal(a, b)


def test_calc_losses_on_a_byte_batch():
    from test_gpu_train_front import LAM_C, LAM_F, _front_end_setup
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend, data, kept = _front_end_setup()
    _, n_views, _, H, W = data["images"].shape
    rng = np.random.default_rng(3)
    data = dict(data, images=torch.from_numpy(rng.integers(0, 256, (2, n_views, H, W, 3), dtype=np.uint8)))
    render_par = rend.bind_parallel(net, None)
    torch.manual_seed(7); np.random.seed(7)
    loss, d = train.calc_losses(net, render_par, data, ray_batch_size=32, nviews=[2], z_near=1.25, z_far=2.75,
                                loss=RenderLoss(LAM_C, LAM_F), balanced=True)
    loss.backward()
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and float(loss.detach()) > 0.0 and float(d["t"]) == float(loss.detach())
    assert tuple(kept[-1].shape[:1]) == (2 * 2,) and kept[-1].grad is not None
    assert bool(torch.isfinite(kept[-1].grad).all()) and float(kept[-1].grad.abs().max()) > 0.0
    grads = [p.grad for p in net.mlp_coarse.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0.0 for g in grads)


# ------------------------------------------------------------------------------------------------ a folder through evaluate
def test_evaluate_takes_an_srn_folder(tmp_path):
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    W = H = 32
    n_views = 3
    for o, name in enumerate(("a1", "b2")):
        images = dt.boxed_views(n_views, H, W, [(4 + v, 6, 25, 28 - v) for v in range(n_views)], seed=o)
        poses = np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(n_views)]).astype(np.float32)
        poses[:, :, 1:3] *= -1.0                            # stored in the OpenCV convention; the dataset flips it back
        dt.write_srn_object(str(tmp_path / "cars_test" / name), images, poses, 33.0, 16.0, 16.0, ["000000", "000001", "000002"])
    dataset = get_split_dataset("srn", str(tmp_path / "cars"), want_split="test")
    assert len(dataset) == 2 and tuple(dataset[0]["images"].shape) == (n_views, 3, H, W)

    spec = dict(gu.CASES["full_ns1"])
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    rend = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).cuda().eval()
    net.precision = "fp16"
    orig, seen = rend.render_image, []

    def recording(*a, **k):
        seen.append((a[5], a[6]))
        return orig(*a, **k)
    rend.render_image = recording
    out = str(tmp_path / "eval_out")
    try:
        m = evalio.evaluate(net, rend, dataset, out, source="0", verbose=False, seed=5, metrics="device")
    finally:
        rend.render_image = orig
    assert seen == [(dataset.z_near, dataset.z_far)] * (2 * (n_views - 1)) and (dataset.z_near, dataset.z_far) == (0.8, 1.8)
    rows = [x.split() for x in open(os.path.join(out, "finish.txt")).read().split("\n") if x]
    assert [r[0] for r in rows] == ["a1", "b2"] and all(r[3] == "1" for r in rows)
    assert m[2] == 2 and all(np.isfinite(float(r[1])) and np.isfinite(float(r[2])) for r in rows)
    assert sorted(os.listdir(os.path.join(out, "a1"))) == ["000001.png", "000002.png"]
