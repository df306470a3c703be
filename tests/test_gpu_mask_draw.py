"""pnr_mask_table_build and pnr_train_draw_masked on the device against the host model of tests/mask_draw_util.py, bit for bit
(the arithmetic is all integer: include/pnr.h), their output bounds, and the layers on top: util.mask_table / train_draw_masked,
data.ResidentSplit(device_masks=True), train.make_batch(prop_inside=...) and a Trainer resumed from a checkpoint.  Every table
the draw kernel is handed here is a consistent one, built by the table kernel or by the model.

The make_batch tests run on an 8 x 8 DVR tree (L-shaped masks: a box is not the mask).  The Trainer run uses the 16 x 16 SRN tree
and the network of test_gpu_trainer.py, the smallest image its three-level encoder takes."""
import numpy as np
import pytest
import torch

import data_trees as dt
import golden_util as gu
import mask_draw_util as mu
import resize_util as R

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A


def _i32(a):
    """A model array of uint32 patterns as the int32 tensor the device hands out."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def _model_tables(masks_u8, thresh=128):
    bits, rows = mu.model_table(mu.inside_of(masks_u8, thresh))
    return _i32(bits), _i32(rows)


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("shape", mu.TABLE_SHAPES)
def test_table_matches_the_model(shape):
    from pixel_nerf_multiscale_amd import util
    N, NV, H, W = shape
    rng = np.random.default_rng(sum(shape))
    cases = [(rng.integers(0, 256, shape, dtype=np.uint8), t) for t in (1, 128, 255)]
    cases += [(np.zeros(shape, np.uint8), 128), (np.full(shape, 255, np.uint8), 128), (mu.random_masks(*shape, 0.5, 2), 128)]
    for masks, thresh in cases:
        bits, rows = util.mask_table(torch.from_numpy(masks).cuda(), thresh=thresh)
        want_bits, want_rows = _model_tables(masks, thresh)
        assert bits.dtype == rows.dtype == torch.int32 and tuple(bits.shape) == (N, NV * H, (W + 31) // 32)
        assert torch.equal(bits.cpu(), want_bits) and torch.equal(rows.cpu(), want_rows), (shape, thresh)
        if W & 31:
            assert not bool((bits[:, :, -1].cpu().numpy().view(np.uint32) >> np.uint32(W & 31)).any())      # tail bits zero
    # one object's table is its slice of the batch's; bool and float masks go through >= 0.5
    m = torch.from_numpy(cases[-1][0]).cuda()
    b0, r0 = util.mask_table(m[0])
    assert torch.equal(b0, bits[:1]) and torch.equal(r0, rows[:1])
    for other in (m >= 128, (m >= 128).float() * 0.75, (m >= 128).float()[:, :, None]):
        b1, r1 = util.mask_table(other)
        assert torch.equal(b1, bits) and torch.equal(r1, rows)


@pytest.mark.parametrize("stride", [1, 4])
def test_table_strides_offsets_and_bounds(stride):
    """The mask byte of pixel p at masks[p * stride] for a pointer at byte offsets 0..3 of its allocation (stride 4 at offset 3:
    an alpha channel where it lies), the bytes between the pixels garbage; sentinel words around both outputs."""
    from pixel_nerf_multiscale_amd import _native as N
    PAD = 19
    for shape in ((2, 2, 3, 33), (1, 1, 4, 65), (1, 3, 100, 5)):
        n, NV, H, W = shape
        R_, Wd, n_pix = NV * H, (W + 31) // 32, n * NV * H * W
        masks = np.random.default_rng(7 + W).integers(0, 256, n_pix, dtype=np.uint8)
        want_bits, want_rows = _model_tables(masks.reshape(shape), 100)
        for off in range(4):
            buf = np.random.default_rng(off).integers(0, 256, off + n_pix * stride + 5, dtype=np.uint8)
            buf[off:off + n_pix * stride:stride] = masks
            dev = torch.from_numpy(buf).cuda()
            bits = torch.full((PAD + n * R_ * Wd + PAD,), SENT, dtype=torch.int32, device="cuda")
            rows = torch.full((PAD + n * (R_ + 1) + PAD,), SENT, dtype=torch.int32, device="cuda")
            rc = N.lib.pnr_mask_table_build(dev.data_ptr() + off, n, NV, H, W, stride, 100, bits.data_ptr() + 4 * PAD,
                                            rows.data_ptr() + 4 * PAD, N.current_stream(dev.device))
            torch.cuda.synchronize()
            assert rc == 0
            for out, count in ((bits, n * R_ * Wd), (rows, n * (R_ + 1))):
                assert bool((out[:PAD] == SENT).all()) and bool((out[PAD + count:] == SENT).all()), (shape, off)
            assert torch.equal(bits[PAD:PAD + n * R_ * Wd].view(n, R_, Wd).cpu(), want_bits), (shape, off)
            assert torch.equal(rows[PAD:PAD + n * (R_ + 1)].view(n, R_ + 1).cpu(), want_rows), (shape, off)


def test_table_of_an_alpha_channel_and_into_a_pool():
    from pixel_nerf_multiscale_amd import util
    rgba = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (3, 2, 4, 37, 4), dtype=np.uint8)).cuda()
    want = _model_tables(rgba[..., 3].cpu().numpy(), 128)
    bits, rows = util.mask_table(rgba[..., 3:], pix_stride=4)
    assert torch.equal(bits.cpu(), want[0]) and torch.equal(rows.cpu(), want[1])
    pool = (torch.full((3, 8, 2), -1, dtype=torch.int32, device="cuda"), torch.full((3, 9), -1, dtype=torch.int32, device="cuda"))
    out = util.mask_table(rgba[1, :, :, :, 3].contiguous(), out=(pool[0][1:2], pool[1][1:2]))
    assert out[0].data_ptr() == pool[0][1:2].data_ptr()
    assert torch.equal(pool[0][1].cpu(), want[0][1]) and torch.equal(pool[1][1].cpu(), want[1][1])
    assert bool((pool[0][[0, 2]] == -1).all()) and bool((pool[1][[0, 2]] == -1).all())
    with pytest.raises(ValueError):
        util.mask_table(rgba[..., 3:], pix_stride=3)
    with pytest.raises(ValueError):
        util.mask_table(rgba[1, :, :, :, 3].contiguous(), out=(pool[0], pool[1]))


# ------------------------------------------------------------------------------------------------------------ the draws
SB, NV, H, W = 2, 3, 5, 37


def _draw_case(masks, B, prop, NS, seed, obj_base=0):
    """The device's draw on the device's table of `masks`, and the model's on the model's: -> (pix, order, want_pix, want_order)."""
    from pixel_nerf_multiscale_amd import util
    sb, nv, h, w = masks.shape
    bits, rows = util.mask_table(torch.from_numpy(masks).cuda())
    pix, order = util.train_draw_masked(bits, rows, sb, nv, w, h, B, NS, seed, prop, obj_base=obj_base)
    mbits, mrows = mu.model_table(mu.inside_of(masks))
    want_pix, want_order, _ = mu.model_draw(mbits, mrows, sb, nv, w, h, B, mu.n_inside(B, prop), NS, seed, obj_base=obj_base)
    return pix, order, torch.from_numpy(want_pix), torch.from_numpy(want_order)


@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
def test_draws_match_the_model_bit_for_bit(density):
    from pixel_nerf_multiscale_amd import util
    masks = mu.random_masks(SB, NV, H, W, density, 3)
    flat = torch.from_numpy(mu.inside_of(masks).reshape(SB, -1))
    checked = 0
    for B in (1, 255, 256, 257):
        for prop in (0.0, 1.0, 0.3):
            for NS in (0, 1, NV):
                seed = 1000003 * B + 7 * NS + int(100 * prop) + (1 << 40)
                pix, order, want_pix, want_order = _draw_case(masks, B, prop, NS, seed)
                assert pix.dtype == order.dtype == torch.long and tuple(pix.shape) == (SB, B) and tuple(order.shape) == (SB, NS)
                assert torch.equal(pix.cpu(), want_pix) and torch.equal(order.cpu(), want_order), (B, prop, NS)
                B_in = util.num_inside(B, prop)
                got = torch.gather(flat, 1, pix.cpu())
                assert bool(got[:, :B_in].all()) and not bool(got[:, B_in:].any())      # set bits, then clear bits
                if NS:
                    assert torch.equal(order, util.train_draw(None, SB, NV, W, H, 0, NS, seed, out_views=torch.empty_like(order))[1])
                checked += SB * B
    print(f"density {density}: {checked} pixels compared")


def test_five_pixels_at_one_half_are_three_inside():
    masks = mu.random_masks(SB, NV, H, W, 0.5, 4)
    pix, _, want_pix, _ = _draw_case(masks, 5, 0.5, 0, 11)
    assert torch.equal(pix.cpu(), want_pix)
    got = torch.gather(torch.from_numpy(mu.inside_of(masks).reshape(SB, -1)), 1, pix.cpu())
    assert got.tolist() == [[True, True, True, False, False]] * SB


def test_single_pixels_and_empty_populations():
    n = NV * H * W
    last_in = np.zeros((1, NV, H, W), np.uint8)
    last_in.reshape(-1)[n - 1] = 255                    # one inside pixel at the very last index
    first_out = np.full((1, NV, H, W), 255, np.uint8)
    first_out.reshape(-1)[0] = 0                        # one outside pixel at index 0
    for masks, B_in_value, B_out_value in ((last_in, n - 1, None), (first_out, None, 0)):
        pix, _, want_pix, _ = _draw_case(masks, 64, 0.5, 0, 21)
        assert torch.equal(pix.cpu(), want_pix)
        if B_in_value is not None:
            assert pix[0, :32].tolist() == [B_in_value] * 32 and B_in_value not in pix[0, 32:].tolist()
        else:
            assert pix[0, 32:].tolist() == [B_out_value] * 32 and B_out_value not in pix[0, :32].tolist()
    # an empty population: its slots draw from the other one, nothing is -1
    for value in (0, 255):
        masks = np.full((2, NV, H, W), value, np.uint8)
        pix, order, want_pix, want_order = _draw_case(masks, 300, 0.5, 2, 22)
        assert torch.equal(pix.cpu(), want_pix) and torch.equal(order.cpu(), want_order)
        assert int(pix.min()) >= 0 and int(pix.max()) < n and len(set(pix[0, :150].tolist())) > 100 and len(set(pix[0, 150:].tolist())) > 100


def test_an_object_base_places_a_slice_inside_its_batch():
    masks = mu.random_masks(5, NV, H, W, 0.4, 6)
    whole, whole_order, want_pix, want_order = _draw_case(masks, 257, 0.6, 2, 31337)
    assert torch.equal(whole.cpu(), want_pix) and torch.equal(whole_order.cpu(), want_order)
    for k, m in ((0, 2), (2, 3), (4, 1)):
        pix, order, _, _ = _draw_case(masks[k:k + m], 257, 0.6, 2, 31337, obj_base=k)
        assert torch.equal(pix, whole[k:k + m]) and torch.equal(order, whole_order[k:k + m])


def test_draw_outputs_keep_their_bounds():
    """Sentinels around both outputs, which sit at odd 8-byte offsets of larger buffers; B = 257: the last workgroup is ragged and
    holds the view work items.  NS = 0 leaves the view output alone, B = 0 the pixel output."""
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd import util
    B, NS, PAD, S = 257, 3, 33, -123456789
    masks = mu.random_masks(SB, NV, H, W, 0.5, 8)
    bits, rows = util.mask_table(torch.from_numpy(masks).cuda())
    mbits, mrows = mu.model_table(mu.inside_of(masks))
    pix = torch.full((PAD + SB * B + PAD,), S, dtype=torch.long, device="cuda")
    order = torch.full((PAD + SB * NS + PAD,), S, dtype=torch.long, device="cuda")
    stream = N.current_stream(bits.device)
    rc = N.lib.pnr_train_draw_masked(bits.data_ptr(), rows.data_ptr(), SB, NV, W, H, B, 100, NS, 99, pix.data_ptr() + 8 * PAD,
                                     order.data_ptr() + 8 * PAD, stream)
    torch.cuda.synchronize()
    assert rc == 0
    for buf, n in ((pix, SB * B), (order, SB * NS)):
        assert bool((buf[:PAD] == S).all()) and bool((buf[PAD + n:] == S).all())
    want_pix, want_order, _ = mu.model_draw(mbits, mrows, SB, NV, W, H, B, 100, NS, 99)
    assert np.array_equal(pix[PAD:PAD + SB * B].view(SB, B).cpu().numpy(), want_pix)
    assert np.array_equal(order[PAD:PAD + SB * NS].view(SB, NS).cpu().numpy(), want_order)
    order.fill_(S)
    assert N.lib.pnr_train_draw_masked(bits.data_ptr(), rows.data_ptr(), SB, NV, W, H, 4, 2, 0, 1, pix.data_ptr(), None, stream) == 0
    pix.fill_(S)
    assert N.lib.pnr_train_draw_masked(None, None, SB, NV, W, H, 0, 0, 2, 1, None, order.data_ptr() + 8 * PAD, stream) == 0
    torch.cuda.synchronize()
    assert bool((pix == S).all()) and bool((order[:PAD] == S).all()) and bool((order[PAD + SB * 2:] == S).all())


# ------------------------------------------------------------------------------------------------------------ make_batch
CAT = "02691156"
SIZE = 8


@pytest.fixture(scope="module")
def dvr_tree(tmp_path_factory):
    """Three objects of three 8 x 8 views; the masks are L-shaped, so a box is not the mask."""
    root = tmp_path_factory.mktemp("nmr8")
    rng = np.random.default_rng(4)
    for o, name in enumerate(("a", "b", "c")):
        images = rng.integers(0, 256, (3, SIZE, SIZE, 3), dtype=np.uint8)
        masks = np.zeros((3, SIZE, SIZE), np.uint8)
        for v in range(3):
            masks[v, 1 + o % 2:6, 2:3 + v] = 255
            masks[v, 5:6 + v % 2, 2:7 - o % 2] = 255
        cams = {}
        for v in range(3):
            m = np.eye(4)
            m[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            m[:3, 3] = rng.normal(size=3)
            cams[f"world_mat_{v}"], cams[f"camera_mat_{v}"] = m, np.diag([2.1875, 2.1875, 1.0, 1.0])
        dt.write_dvr_object(str(root / CAT / name), images, masks, cams)
    with open(str(root / CAT / "softras_train.lst"), "w") as f:
        f.write("a\nb\nc\n")
    return str(root)


def _dvr(tree, as_bytes):
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    return get_split_dataset("dvr", tree, want_split="train", as_bytes=as_bytes)


def _stack(dset, ids):
    keys = [k for k in ("images", "masks", "poses", "bbox", "focal", "c") if k in dset[0]]
    return {k: torch.stack([torch.as_tensor(dset[i][k]) for i in ids]) for k in keys}


def _same(a, b):
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        assert (x is None and y is None) or (x.dtype == y.dtype and torch.equal(x, y))


def test_make_batch_three_ways_equals_the_gathers_on_the_models_indices(dvr_tree):
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    as_float, as_bytes = _dvr(dvr_tree, False), _dvr(dvr_tree, True)
    ids, B, nviews, dev = [2, 0], 37, [1, 2], torch.device("cuda")
    split = ResidentSplit(as_bytes, "cuda", device_masks=True, device_boxes=True)
    float_batch, byte_batch, resident = _stack(as_float, ids), _stack(as_bytes, ids), split.batch(ids)
    assert resident["mask_bits"].is_cuda and tuple(resident["mask_bits"].shape) == (2, 24, 1) and tuple(resident["mask_rows"].shape) == (2, 25)
    masks = byte_batch["masks"].numpy()
    assert tuple(float_batch["masks"].shape) == (2, 3, 1, SIZE, SIZE) and masks.dtype == np.uint8
    mbits, mrows = mu.model_table(mu.inside_of(masks))
    assert torch.equal(resident["mask_bits"].cpu(), _i32(mbits)) and torch.equal(resident["mask_rows"].cpu(), _i32(mrows))
    z = dict(z_near=as_bytes.z_near, z_far=as_bytes.z_far)
    for key in [next(k for k in (frame_seed(5, s) for s in range(16)) if k % 2 == r) for r in (0, 1)]:
        NS = nviews[key % 2]
        for prop in (0.75, 0.0):
            want_pix, want_order, _ = mu.model_draw(mbits, mrows, 2, 3, SIZE, SIZE, B, mu.n_inside(B, prop), NS, key)
            pix, order = torch.from_numpy(want_pix).cuda(), torch.from_numpy(want_order).cuda()
            images, poses = byte_batch["images"].cuda(), byte_batch["poses"].cuda()
            rays, rgb = util.train_batch_u8(images, poses, byte_batch["focal"], None, pix, balanced=as_bytes.balanced, **z)
            want = (rays, rgb, util.views_to_tensor_u8(images, order, balanced=as_bytes.balanced), util.batched_index_select_nd(poses, order))
            outs = []
            for data in (float_batch, byte_batch, resident):
                torch.manual_seed(3); np.random.seed(3)
                t_state, n_state = torch.get_rng_state(), np.random.get_state()[1].copy()
                outs.append(train.make_batch(data, dev, ray_batch_size=B, nviews=nviews, balanced=as_bytes.balanced, draws="device",
                                             seed=key, prop_inside=prop, **z))
                assert torch.equal(t_state, torch.get_rng_state()) and np.array_equal(n_state, np.random.get_state()[1])
            for got in outs:
                _same(got, outs[0])
                assert not bool(torch.isnan(got[0]).any()) and tuple(got[0].shape) == (2, B, 8) and tuple(got[2].shape) == (2, NS, 3, SIZE, SIZE)
                for x, y in zip(got[:4], want):
                    assert torch.equal(x, y)
        # None: the parent's calls, the parent's bits; use_bbox=False and evaluation never see prop_inside
        for data in (float_batch, byte_batch, resident):
            kw = dict(ray_batch_size=B, nviews=nviews, balanced=as_bytes.balanced, draws="device", seed=key, **z)
            _same(train.make_batch(data, dev, prop_inside=None, **kw), train.make_batch(data, dev, **kw))
            for off in (dict(use_bbox=False), dict(is_train=False)):
                _same(train.make_batch(data, dev, prop_inside=0.75, **kw, **off), train.make_batch(data, dev, **kw, **off))
            assert not torch.equal(train.make_batch(data, dev, prop_inside=0.75, **kw)[0], train.make_batch(data, dev, **kw)[0])
    # a slice of the batch under its object base: the rows of the whole batch's outputs
    kw = dict(ray_batch_size=B, nviews=nviews, balanced=as_bytes.balanced, draws="device", seed=77, prop_inside=0.5, **z)
    whole = train.make_batch(split.batch([2, 0, 1]), dev, **kw)
    part = train.make_batch(split.batch([0, 1]), dev, obj_base=1, **kw)
    for x, y in zip(part, whole):
        assert (x is None and y is None) or torch.equal(x, y[1:])


def test_resident_split_builds_the_table_of_resized_masks(dvr_tree):
    from pixel_nerf_multiscale_amd.data import ResidentSplit, get_split_dataset
    dset = _dvr(dvr_tree, True)
    items = [dset[i] for i in range(len(dset))]
    N = len(items)
    split = ResidentSplit(dset, "cuda", image_size=4, device_masks=True)
    small = np.stack([R.model_u8(it["masks"].numpy()[..., None], 4, 4)[..., 0] for it in items])
    assert small.shape == (N, 3, 4, 4) and 0 < (small >= 128).sum() < small.size and ((small > 0) & (small < 255)).any()
    want_bits, want_rows = _model_tables(small)
    assert torch.equal(split.mask_bits.cpu(), want_bits) and torch.equal(split.mask_rows.cpu(), want_rows)
    b = split.batch([1, 2])
    assert torch.equal(b["mask_bits"].cpu(), want_bits[[1, 2]]) and torch.equal(b["mask_rows"].cpu(), want_rows[[1, 2]])
    # max_bytes is judged on pool + tables; without the keyword nothing changes
    pool, tables = N * 3 * 4 * 4 * 3, 4 * N * (12 * 1 + 13)
    assert split.nbytes == pool + tables
    assert ResidentSplit(dset, "cuda", image_size=4, device_masks=True, max_bytes=pool + tables).nbytes == pool + tables
    with pytest.raises(ValueError, match="max_bytes"):
        ResidentSplit(dset, "cuda", image_size=4, device_masks=True, max_bytes=pool + tables - 1)
    plain = ResidentSplit(dset, "cuda", image_size=4, max_bytes=pool)
    assert plain.nbytes == pool and plain.mask_bits is None and "mask_bits" not in plain.batch([0]) and "mask_rows" not in plain.batch([0])
    assert torch.equal(plain.images, split.images)

    class NoMasks(list):
        as_bytes, z_near, z_far, lindisp, balanced = True, 0.5, 2.0, False, True

    with pytest.raises(ValueError, match="masks"):
        ResidentSplit(NoMasks({k: v for k, v in it.items() if k != "masks"} for it in items), "cuda", device_masks=True)


def test_the_step_reads_nothing_back_and_uploads_nothing_more(dvr_tree, monkeypatch):
    """make_batch on a resident batch, boxes against masks: the same host-to-device moves (the intrinsics' block), no device
    tensor read on the host in either."""
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    dset = _dvr(dvr_tree, True)
    data = ResidentSplit(dset, "cuda", device_masks=True, device_boxes=True).batch([0, 1])
    log = []
    real_upload, real_to = util.upload, torch.Tensor.to

    def upload(t, device):
        log.append(("upload", t.is_cuda, tuple(t.shape)))
        return real_upload(t, device)

    def to(self, *a, **k):
        out = real_to(self, *a, **k)
        if self.is_cuda != out.is_cuda:
            log.append(("to_device" if out.is_cuda else "read", tuple(self.shape)))
        return out

    def read(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                log.append(("read", name))
            return real(self, *a, **k)
        return f

    monkeypatch.setattr(util, "upload", upload)
    monkeypatch.setattr(torch.Tensor, "to", to)
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__"):
        monkeypatch.setattr(torch.Tensor, name, read(name))
    kw = dict(ray_batch_size=16, nviews=[2], z_near=dset.z_near, z_far=dset.z_far, balanced=dset.balanced, draws="device", seed=5)
    train.make_batch(data, torch.device("cuda"), **kw)
    boxes, log[:] = list(log), []
    train.make_batch(data, torch.device("cuda"), prop_inside=0.75, **kw)
    masked = list(log)
    monkeypatch.undo()
    assert masked == boxes and not any(e[0] == "read" for e in masked)
    assert len(masked) >= 2                                 # the spies saw the step: images and poses went through util.upload


# ------------------------------------------------------------------------------------------------------------ the Trainer
def test_a_resumed_mask_weighted_run_continues_bit_for_bit(tmp_path, monkeypatch):
    """test_gpu_trainer's resumed-run test under prop_inside = 0.75 on a ResidentSplit with tables: run A two epochs, run B one
    epoch and a resumed second; every parameter and both Adam moments agree exactly, and the mask draw was the one every
    training step before no_bbox_step made."""
    import test_gpu_trainer as tg
    from pixel_nerf_multiscale_amd import util
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    root = tmp_path / "srn"
    for stage, n_obj in (("train", 4), ("val", 2)):
        for o in range(n_obj):
            images = dt.boxed_views(tg.NV, tg.H, tg.W, [(2 + v, 3, 12, 13 - v - o % 2) for v in range(tg.NV)], seed=10 * o + (stage == "val"))
            poses = np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(tg.NV)]).astype(np.float32)
            poses[:, :, 1:3] *= -1.0
            dt.write_srn_object(str(root / f"cars_{stage}" / f"obj{o}"), images, poses, 16.5, 8.0, 8.0, ["000000", "000001", "000002"])
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    seen, real = [], util.train_draw_masked

    def spy(*a, **k):
        seen.append(a[9])
        return real(*a, **k)

    monkeypatch.setattr(util, "train_draw_masked", spy)
    try:
        train_set, _ = tg._datasets(str(root / "cars"), as_bytes=True)
        split = ResidentSplit(train_set, "cuda", device_masks=True)
        a = tg._trainer(str(tmp_path / "a"), split, None, prop_inside=0.75, no_bbox_step=3)
        a.start()
        assert seen == [0.75] * 3                          # four training steps, the last past no_bbox_step: masks off as boxes are
        b1 = tg._trainer(str(tmp_path / "b"), split, None, num_epochs=1, prop_inside=0.75, no_bbox_step=3)
        b1.start()
        half = tg._state(b1)
        b2 = tg._trainer(str(tmp_path / "b"), split, None, resume=True, prop_inside=0.75, no_bbox_step=3)
        assert (b2.epoch, b2.global_step) == (1, 2)
        b2.start()
        sa, sb = tg._state(a), tg._state(b2)
        assert sa[3] == 4 and sa[4] == 4
        tg._assert_same(sa, sb)
        assert not torch.equal(half[1], sa[1])
    finally:
        torch.backends.cudnn.deterministic = was
