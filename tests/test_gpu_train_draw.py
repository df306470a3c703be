"""pnr_train_draw on the device against the host model of tests/train_draw_util.py, bit for bit (the arithmetic is all
integer: include/pnr.h), its output bounds, and train.make_batch on top of it: draws="device" equals the gather entry points
called by hand on the model's indices, draws="host" equals what make_batch gave before."""
import numpy as np
import pytest
import torch

import golden_util as gu
import train_draw_util as du

pytestmark = pytest.mark.gpu

W, H = 11, 7
Z_NEAR, Z_FAR = 0.75, 3.5
BOXES = ["none", "one_pixel", "whole", "corner", "one_invalid"]


def _boxes(kind, SB, NV):
    if kind == "none":
        return None
    b = np.empty((SB, NV, 4), np.float32)
    for o in range(SB):
        for v in range(NV):
            if kind == "one_pixel":
                c, r = (3 * o + 2 * v) % W, (o + 5 * v) % H
                b[o, v] = (c, r, c, r)
            elif kind == "whole":
                b[o, v] = (0, 0, W - 1, H - 1)
            elif kind == "corner":
                b[o, v] = (W - 3 + (v % 2), H - 2, W - 1, H - 1)
            else:
                b[o, v] = (1 + o, v % 3, W - 2, H - 1 - o)
    if kind == "one_invalid":
        b[0, NV - 1] = (np.nan, 0, 3, 3)
        if SB > 1:
            b[SB - 1, 0] = (4, 2, 3, 5)                     # inverted
    return b


@pytest.mark.parametrize("kind", BOXES)
def test_draws_match_the_model_bit_for_bit(kind):
    from pixel_nerf_multiscale_amd import util
    checked = minus = 0
    for SB in (1, 3):
        for NV in (1, 2, 5):
            boxes = _boxes(kind, SB, NV)
            dev_boxes = None if boxes is None else torch.from_numpy(boxes).cuda()
            for NS in sorted({0, 1, NV}):
                for B in (1, 255, 256, 257):
                    seed = 1000003 * B + 101 * SB + 7 * NV + NS + (1 << 40)
                    out_pix = torch.full((SB, B), -7, dtype=torch.long, device="cuda")
                    pix, order = util.train_draw(dev_boxes, SB, NV, W, H, B, NS, seed, out_pix=out_pix)
                    want_pix, want_order, _ = du.model_draw(boxes, SB, NV, W, H, B, NS, seed)
                    assert pix is out_pix and pix.dtype == order.dtype == torch.long and tuple(order.shape) == (SB, NS)
                    assert np.array_equal(pix.cpu().numpy(), want_pix), (SB, NV, NS, B)
                    assert np.array_equal(order.cpu().numpy(), want_order), (SB, NV, NS, B)
                    checked += SB * B
                    minus += int((want_pix < 0).sum())
    print(f"{kind}: {checked} pixels compared, {minus} of them -1")
    assert (minus > 0) == (kind == "one_invalid")


def test_many_views_and_the_largest_subset():
    """NS = 64 of NV = 64 and of NV = 200 (the insertion walk at its longest), several blocks of view words."""
    from pixel_nerf_multiscale_amd import util
    for NV in (64, 200):
        pix, order = util.train_draw(None, 5, NV, 3, 2, 4, 64, 99, out_pix=torch.empty(5, 4, dtype=torch.long, device="cuda"))
        want_pix, want_order, _ = du.model_draw(None, 5, NV, 3, 2, 4, 64, 99)
        assert np.array_equal(order.cpu().numpy(), want_order) and np.array_equal(pix.cpu().numpy(), want_pix)
        assert all(len(set(r)) == 64 for r in want_order.tolist())


def test_outputs_keep_their_bounds():
    """Sentinels around both outputs, which sit at odd 8-byte offsets of larger buffers; B = 257: the last workgroup is ragged
    and holds the view work items."""
    from pixel_nerf_multiscale_amd import _native as N
    SB, NV, B, NS, PAD, SENT = 3, 5, 257, 5, 33, -123456789
    boxes = torch.from_numpy(_boxes("corner", SB, NV)).cuda()
    pix = torch.full((PAD + SB * B + PAD,), SENT, dtype=torch.long, device="cuda")
    order = torch.full((PAD + SB * NS + PAD,), SENT, dtype=torch.long, device="cuda")
    rc = N.lib.pnr_train_draw(boxes.data_ptr(), SB, NV, W, H, B, NS, 31337, pix.data_ptr() + 8 * PAD, order.data_ptr() + 8 * PAD,
                              N.current_stream(boxes.device))
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in ((pix, SB * B), (order, SB * NS)):
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all())
    want_pix, want_order, _ = du.model_draw(_boxes("corner", SB, NV), SB, NV, W, H, B, NS, 31337)
    assert np.array_equal(pix[PAD:PAD + SB * B].view(SB, B).cpu().numpy(), want_pix)
    assert np.array_equal(order[PAD:PAD + SB * NS].view(SB, NS).cpu().numpy(), want_order)
    # NS = 0: the view output is not touched (and may be NULL); B = 0: the pixel output is not touched
    order.fill_(SENT)
    assert N.lib.pnr_train_draw(None, SB, NV, W, H, 4, 0, 1, pix.data_ptr(), None, N.current_stream(boxes.device)) == 0
    pix.fill_(SENT)
    assert N.lib.pnr_train_draw(None, SB, NV, W, H, 0, 2, 1, None, order.data_ptr() + 8 * PAD, N.current_stream(boxes.device)) == 0
    torch.cuda.synchronize()
    assert bool((pix == SENT).all()) and bool((order[:PAD] == SENT).all()) and bool((order[PAD + SB * 2:] == SENT).all())
    assert np.array_equal(order[PAD:PAD + SB * 2].view(SB, 2).cpu().numpy(), du.model_draw(None, SB, NV, W, H, 0, 2, 1)[1])


def test_one_seed_one_batch_two_seeds_two_batches():
    from pixel_nerf_multiscale_amd import util
    boxes = torch.from_numpy(_boxes("whole", 2, 5)).cuda()
    a = util.train_draw(boxes, 2, 5, W, H, 300, 3, 12345)
    b = util.train_draw(boxes, 2, 5, W, H, 300, 3, 12345)
    c = util.train_draw(boxes, 2, 5, W, H, 300, 3, 12346)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and float((a[0] == c[0]).float().mean()) < 0.05


# ------------------------------------------------------------------------------------------------------- make_batch
class _Items(list):
    as_bytes, z_near, z_far, lindisp, balanced = True, Z_NEAR, Z_FAR, False, True


def _objects(n_obj, NV, seed):
    rng = np.random.default_rng(seed)
    items = []
    for o in range(n_obj):
        images = torch.from_numpy(rng.integers(0, 256, (NV, H, W, 3), dtype=np.uint8))
        poses = torch.from_numpy(np.stack([gu.pose_spherical(25.0 * v + 40.0 * o, -20.0 - 4.0 * v, 2.0) for v in range(NV)])).float()
        bbox = torch.tensor([[1.0 + o, 1.0, W - 2.0, H - 2.0 - (v % 2)] for v in range(NV)])
        items.append({"path": f"/data/cat/obj{o}", "img_id": o, "focal": 18.0 + 1.5 * o,
                      "c": torch.tensor([0.5 * W + 0.25 - o, 0.5 * H - 0.5 + o]), "images": images,
                      "masks": torch.zeros(NV, H, W, dtype=torch.uint8), "bbox": bbox, "poses": poses})
    return items


def _three_batches(device_boxes=True):
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.data._items import images_to_float
    items = _Items(_objects(3, 4, seed=9))
    ids = [2, 0]
    host = {k: torch.stack([torch.as_tensor(items[i][k]) for i in ids]) for k in ("images", "poses", "bbox", "focal", "c")}
    as_float = dict(host, images=torch.stack([images_to_float(items[i]["images"], True) for i in ids]))
    resident = ResidentSplit(items, "cuda", device_boxes=device_boxes).batch(ids)
    return host, as_float, resident


@pytest.mark.parametrize("use_bbox", [True, False])
def test_make_batch_device_draws(use_bbox):
    """The float batch, the byte batch and ResidentSplit(device_boxes=True).batch under draws="device": the six outputs equal
    train_batch / train_batch_u8 / views_to_tensor_u8 / batched_index_select_nd on the MODEL's indices, for a key of each
    source-view count; neither global generator moves."""
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    host, as_float, resident = _three_batches()
    assert resident["bbox_dev"].is_cuda and torch.equal(resident["bbox_dev"].cpu(), host["bbox"]) and not resident["bbox"].is_cuda
    nviews, B, dev = [1, 2], 37, torch.device("cuda")
    keys = [frame_seed(5, s) for s in range(8)]
    keys = [next(k for k in keys if k % 2 == 0), next(k for k in keys if k % 2 == 1)]
    for key in keys:
        NS = nviews[key % 2]
        want_pix, want_order, _ = du.model_draw(host["bbox"].numpy() if use_bbox else None, 2, 4, W, H, B, NS, key)
        pix, order = torch.from_numpy(want_pix).cuda(), torch.from_numpy(want_order).cuda()
        outs = []
        for data in (as_float, host, resident):
            torch.manual_seed(3); np.random.seed(3)
            t_state, n_state = torch.get_rng_state(), np.random.get_state()[1].copy()
            outs.append(train.make_batch(data, dev, ray_batch_size=B, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR, use_bbox=use_bbox,
                                         balanced=True, draws="device", seed=key))
            assert torch.equal(t_state, torch.get_rng_state()) and np.array_equal(n_state, np.random.get_state()[1])
        images_f, images_b, poses = as_float["images"].cuda(), host["images"].cuda(), host["poses"].cuda()
        rays_f, rgb_f = util.train_batch(images_f, poses, host["focal"], host["c"], pix, Z_NEAR, Z_FAR)
        rays_b, rgb_b = util.train_batch_u8(images_b, poses, host["focal"], host["c"], pix, Z_NEAR, Z_FAR, balanced=True)
        src_f = util.batched_index_select_nd(images_f, order)
        src_b = util.views_to_tensor_u8(images_b, order, balanced=True)
        src_poses = util.batched_index_select_nd(poses, order)
        assert torch.equal(rays_f, rays_b) and torch.equal(rgb_f, rgb_b) and torch.equal(src_f, src_b)      # the data layer's contract
        for got in outs:
            rays, rgb, src_images, sp, focal, c = got
            assert tuple(rays.shape) == (2, B, 8) and tuple(src_images.shape) == (2, NS, 3, H, W)
            assert not bool(torch.isnan(rays).any()) and not bool(torch.isnan(rgb).any())
            assert torch.equal(rays, rays_f) and torch.equal(rgb, rgb_f) and torch.equal(src_images, src_f) and torch.equal(sp, src_poses)
            assert torch.equal(focal.cpu(), host["focal"][:, None].expand(2, 2)) and torch.equal(c.cpu(), host["c"])
    a = train.make_batch(host, dev, ray_batch_size=B, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR, draws="device", seed=keys[0])
    b = train.make_batch(host, dev, ray_batch_size=B, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR, draws="device", seed=keys[0] + 2)
    assert not torch.equal(a[0], b[0])


def test_evaluation_and_missing_boxes_draw_from_the_whole_image(monkeypatch):
    from pixel_nerf_multiscale_amd import train, util
    host, _, _ = _three_batches(device_boxes=False)
    seen = []
    real = util.train_draw

    def spy(bbox, *a, **kw):
        seen.append(bbox)
        return real(bbox, *a, **kw)

    monkeypatch.setattr(util, "train_draw", spy)
    kw = dict(ray_batch_size=8, nviews=[1], z_near=Z_NEAR, z_far=Z_FAR, draws="device", seed=4)
    train.make_batch(host, torch.device("cuda"), **kw)
    train.make_batch(host, torch.device("cuda"), is_train=False, **kw)
    train.make_batch(host, torch.device("cuda"), use_bbox=False, **kw)
    train.make_batch({k: v for k, v in host.items() if k != "bbox"}, torch.device("cuda"), **kw)
    assert seen[0] is not None and seen[0].is_cuda and seen[1:] == [None, None, None]


@pytest.mark.parametrize("nviews", [[1], [2]])
def test_host_draws_are_what_they_were(nviews):
    """make_batch(draws="host") — the default — against the same draws and the same entry points called directly, as
    make_batch did before it had a `draws` keyword: the same bits in all six outputs, both generators left in the same state."""
    from pixel_nerf_multiscale_amd import train, util
    host, as_float, resident = _three_batches(device_boxes=False)
    assert "bbox_dev" not in resident
    dev, B = torch.device("cuda"), 37
    for data, as_bytes in ((host, True), (as_float, False), (resident, True)):
        torch.manual_seed(21); np.random.seed(21)
        got = train.make_batch(data, dev, ray_batch_size=B, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR, balanced=True)
        end = (torch.get_rng_state(), np.random.get_state()[1].copy())

        torch.manual_seed(21); np.random.seed(21)
        images, poses = data["images"].cuda(), data["poses"].cuda()
        SB, NV = poses.shape[:2]
        curr = nviews[int(torch.randint(0, len(nviews), ()))]
        order = torch.randint(0, NV, (SB, 1)) if curr == 1 else torch.empty(SB, curr, dtype=torch.long)
        pix = torch.empty(SB, B, dtype=torch.long)
        for o in range(SB):
            if curr > 1:
                order[o] = torch.from_numpy(np.random.choice(NV, curr, replace=False))
            p = util.bbox_sample(data["bbox"][o], B)
            pix[o] = p[:, 0] * (H * W) + p[:, 1] * W + p[:, 2]
        pix, order = pix.cuda(), order.cuda()
        if as_bytes:
            rays, rgb = util.train_batch_u8(images, poses, data["focal"], data["c"], pix, Z_NEAR, Z_FAR, balanced=True)
            src = util.views_to_tensor_u8(images, order, balanced=True)
        else:
            rays, rgb = util.train_batch(images, poses, data["focal"], data["c"], pix, Z_NEAR, Z_FAR)
            src = util.batched_index_select_nd(images, order)
        want = (rays, rgb, src, util.batched_index_select_nd(poses, order))
        for a, b in zip(got[:4], want):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert torch.equal(end[0], torch.get_rng_state()) and np.array_equal(end[1], np.random.get_state()[1])
