"""The pieces of the data-parallel training step on one device, in one process: the object base of the keyed draws
(pnr_train_draw_at, pnr_color_jitter_plan_at, train.make_batch(obj_base=...)) — a call over objects [k, k + m) of a batch gives
rows k .. k + m - 1 of the whole batch's call, bit for bit — and the divisor folded into the optimiser's step
(pnr_adam_step_div, DeviceAdam.step(grad_div=...) / DeviceAdam.allreduce())."""
import numpy as np
import pytest
import torch

import data_parallel_util as dpu
import golden_util as gu
import optim_util as ou
import train_draw_util as du

pytestmark = pytest.mark.gpu

W = H = 16
SB_TOTAL, NV = 4, 4
SLICES = [(1, 2), (3, 1)]                                   # (obj_base, SB) of the calls compared with the base-0 call's rows
BOXES = ["none", "one_pixel", "whole", "corner", "one_invalid"]


def _boxes(kind, SB, NV):
    """The box kinds of the draw test, for a 16 x 16 image."""
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
        b[SB - 1, 0] = (4, 2, 3, 5)                         # inverted
        b[1, 1] = (0, 0, W, 3)                              # outside the image: inside the (1, 2) slice
    return b


# ------------------------------------------------------------------------------------------------------------ draws
@pytest.mark.parametrize("kind", BOXES)
def test_a_slice_draws_its_rows_of_the_whole_batch(kind):
    from pixel_nerf_multiscale_amd import util
    boxes = _boxes(kind, SB_TOTAL, NV)
    dev_boxes = None if boxes is None else torch.from_numpy(boxes).cuda()
    minus = 0
    for B in (1, 255, 256, 257):
        for NS in (0, 1, 4):
            seed = 1000003 * B + NS + (1 << 40)
            whole_pix, whole_ord = util.train_draw(dev_boxes, SB_TOTAL, NV, W, H, B, NS, seed,
                                                   out_pix=torch.empty(SB_TOTAL, B, dtype=torch.long, device="cuda"))
            same_pix, same_ord = util.train_draw(dev_boxes, SB_TOTAL, NV, W, H, B, NS, seed, obj_base=0,
                                                 out_pix=torch.empty(SB_TOTAL, B, dtype=torch.long, device="cuda"))
            assert torch.equal(whole_pix, same_pix) and torch.equal(whole_ord, same_ord)
            want_pix, want_ord, _ = du.model_draw(boxes, SB_TOTAL, NV, W, H, B, NS, seed)      # the base-0 call is pnr_train_draw's
            assert np.array_equal(whole_pix.cpu().numpy(), want_pix) and np.array_equal(whole_ord.cpu().numpy(), want_ord)
            minus += int((want_pix < 0).sum())
            for k, m in SLICES:
                part = None if dev_boxes is None else dev_boxes[k:k + m].contiguous()
                out_pix = torch.full((m, B), -7, dtype=torch.long, device="cuda")
                pix, order = util.train_draw(part, m, NV, W, H, B, NS, seed, out_pix=out_pix, obj_base=k)
                assert pix is out_pix and tuple(order.shape) == (m, NS)
                assert torch.equal(pix, whole_pix[k:k + m]), (B, NS, k, m)
                assert torch.equal(order, whole_ord[k:k + m]), (B, NS, k, m)
    assert (minus > 0) == (kind == "one_invalid")


def test_draw_counters_past_32_bits():
    """The pixel counter r = (obj_base + o) * B + j with its high word in use: a base whose first counter is 2^32 - 1 (the carry
    happens inside the first object's row), one far past 2^32, and one whose OBJECT index is past 2^32 (the view counter's high
    word), against the host model written from the header."""
    from pixel_nerf_multiscale_amd import util
    boxes = _boxes("corner", 2, NV)
    dev_boxes = torch.from_numpy(boxes).cuda()
    cases = [(16711935, 257), ((1 << 31) + 5, 3), ((1 << 32) + 1, 255), ((1 << 40) + 123, 256)]
    assert cases[0][0] * cases[0][1] == (1 << 32) - 1
    for obj_base, B in cases:
        assert (obj_base + 2) * B >= 1 << 32
        for bx, dbx in ((None, None), (boxes, dev_boxes)):
            pix, order = util.train_draw(dbx, 2, NV, W, H, B, 3, 99 + (7 << 33), obj_base=obj_base,
                                         out_pix=torch.empty(2, B, dtype=torch.long, device="cuda"))
            want_pix, want_ord = dpu.model_draw_at(bx, 2, NV, W, H, B, 3, 99 + (7 << 33), obj_base)
            assert np.array_equal(pix.cpu().numpy(), want_pix), (obj_base, B)
            assert np.array_equal(order.cpu().numpy(), want_ord), (obj_base, B)
        low = util.train_draw(None, 2, NV, W, H, B, 3, 99 + (7 << 33), obj_base=obj_base & 0xFFFFFFFF if obj_base >> 32 else 0,
                              out_pix=torch.empty(2, B, dtype=torch.long, device="cuda"))
        assert not torch.equal(low[0], pix)                 # the high word took part


# ------------------------------------------------------------------------------------------------------------ jitter
def test_a_slice_plans_its_records_of_the_whole_batch():
    """SB_total = 3 objects of 2 x 9 x 11 x 3 bytes = 594 each: object 1 starts at a byte offset that is no multiple of 4 in the
    whole batch and at 0 in its slice, so the grey mean is reduced through both load paths."""
    from pixel_nerf_multiscale_amd import util
    rng = np.random.default_rng(4)
    images = torch.from_numpy(rng.integers(0, 256, (3, 2, 9, 11, 3), dtype=np.uint8)).cuda()
    for ranges in ((0.4, 0.4, 0.4, 0.1), (0.15, 0.0, 0.15, 0.15)):          # with and without the mean's reduction
        for seed in (7, 12345 + (5 << 34)):
            whole = util.color_jitter_plan(images, ranges, seed)
            assert torch.equal(whole, util.color_jitter_plan(images, ranges, seed, obj_base=0))
            assert len({tuple(r) for r in whole[:, :4].tolist()}) == 3      # three objects, three draws
            for k, m in ((1, 2), (2, 1), (0, 1)):
                part = util.color_jitter_plan(images[k:k + m].contiguous(), ranges, seed, obj_base=k)
                assert torch.equal(part.view(torch.int32), whole[k:k + m].view(torch.int32)), (ranges, seed, k, m)
            if ranges[1] != 0.0:
                assert bool((whole[:, 4] > 0).all())                        # the means were computed
    moved = util.color_jitter_plan(images[1:2].contiguous(), (0.4, 0.4, 0.4, 0.1), 7, obj_base=0)
    assert not torch.equal(moved, util.color_jitter_plan(images, (0.4, 0.4, 0.4, 0.1), 7)[1:2])    # the base is what places a slice


# ------------------------------------------------------------------------------------------------------------ make_batch
Z_NEAR, Z_FAR = 0.75, 3.5
MW, MH = 11, 7


class _Items(list):
    as_bytes, z_near, z_far, lindisp, balanced = True, Z_NEAR, Z_FAR, False, True


def _objects(n_obj, n_views, seed):
    rng = np.random.default_rng(seed)
    items = []
    for o in range(n_obj):
        images = torch.from_numpy(rng.integers(0, 256, (n_views, MH, MW, 3), dtype=np.uint8))
        poses = torch.from_numpy(np.stack([gu.pose_spherical(25.0 * v + 40.0 * o, -20.0 - 4.0 * v, 2.0) for v in range(n_views)])).float()
        bbox = torch.tensor([[1.0 + o, 1.0, MW - 2.0, MH - 2.0 - (v % 2)] for v in range(n_views)])
        items.append({"path": f"/data/cat/obj{o}", "img_id": o, "focal": 18.0 + 1.5 * o,
                      "c": torch.tensor([0.5 * MW + 0.25 - o, 0.5 * MH - 0.5 + o]), "images": images,
                      "masks": torch.zeros(n_views, MH, MW, dtype=torch.uint8), "bbox": bbox, "poses": poses})
    return items


def _batches(ids):
    """-> {kind: data dict} of the objects `ids` as a float batch, a byte batch and a ResidentSplit batch."""
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.data._items import images_to_float
    items = _Items(_objects(4, 4, seed=9))
    host = {k: torch.stack([torch.as_tensor(items[i][k]) for i in ids]) for k in ("images", "poses", "bbox", "focal", "c")}
    as_float = dict(host, images=torch.stack([images_to_float(items[i]["images"], True) for i in ids]))
    return {"float": as_float, "bytes": host, "resident": ResidentSplit(items, "cuda", device_boxes=True).batch(ids)}


@pytest.mark.parametrize("kind,jitter", [("float", False), ("bytes", False), ("bytes", True), ("resident", False), ("resident", True)])
def test_make_batch_of_a_slice_is_the_rows_of_the_whole_batch(kind, jitter):
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.data import ColorJitter
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    ids = [2, 0, 3]
    dev = torch.device("cuda")
    keys = [frame_seed(5, s) for s in range(8)]
    keys = [next(k for k in keys if k % 2 == 0), next(k for k in keys if k % 2 == 1)]       # one key per source-view count
    whole_data = _batches(ids)[kind]
    for key in keys:
        kw = dict(ray_batch_size=37, nviews=[1, 2], z_near=Z_NEAR, z_far=Z_FAR, balanced=True, draws="device", seed=key,
                  jitter=ColorJitter(0.4, 0.4, 0.4, 0.1) if jitter else None)
        whole = train.make_batch(whole_data, dev, **kw)
        assert not bool(torch.isnan(whole[0]).any()) and not bool(torch.isnan(whole[1]).any())
        for a, b in zip(whole, train.make_batch(whole_data, dev, obj_base=0, **kw)):
            assert torch.equal(a, b)
        for k, m in ((1, 2), (2, 1), (0, 1)):
            part = train.make_batch(_batches(ids[k:k + m])[kind], dev, obj_base=k, **kw)
            assert len(part) == 6
            for name, a, b in zip(("rays", "rgb_gt", "src_images", "src_poses", "focal", "c"), part, whole):
                assert a.shape[0] == m and a.dtype == b.dtype
                assert torch.equal(a.contiguous().view(torch.int32), b[k:k + m].contiguous().view(torch.int32)), (name, key, k, m)
        if jitter:                                          # the records took part: the same slice without them differs
            plain = train.make_batch(whole_data, dev, **dict(kw, jitter=None))
            assert not torch.equal(plain[1], whole[1]) and torch.equal(plain[0], whole[0])
        moved = train.make_batch(_batches(ids[1:3])[kind], dev, obj_base=0, **kw)
        assert not torch.equal(moved[0], whole[0][1:3])     # without the base a slice draws other pixels


def test_render_noise_of_a_slice_is_the_rows_of_the_whole_render():
    """What calc_losses(obj_base=k) sets: ray_index_base = k * ray_batch_size under the step's key."""
    from pixel_nerf_multiscale_amd import NeRFRenderer
    rend = NeRFRenderer(n_coarse=8, n_fine=0).cuda()
    B, key = 37, 123456789
    rays = torch.rand(3 * B, 8, device="cuda")
    rays[:, 6], rays[:, 7] = 0.8, 1.8
    with rend.keyed(key):
        whole = rend.sample_coarse(rays)
    for k, m in ((1, 2), (2, 1)):
        with rend.keyed(key, base=k * B):
            part = rend.sample_coarse(rays[k * B:(k + m) * B].contiguous())
        assert torch.equal(part, whole[k * B:(k + m) * B])
    assert rend.ray_index_base == 0 and rend.forced_seed is None


# ------------------------------------------------------------------------------------------------------------ the divisor
LR, BETAS, EPS, MAX_NORM = ou.LR, ou.BETAS, ou.EPS, ou.MAX_NORM
SCALER = dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)


def _edge_sizes():
    from pixel_nerf_multiscale_amd import _native as N
    chunk = int(N.lib.pnr_optim_chunk_elems())
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 1]


def _edge_case(seed, steps):
    """The segment and chunk-edge sizes of the optimiser's edge test, one more parameter that is a view one float into its
    storage (the scalar body), and `steps` gradient sets."""
    rng = np.random.default_rng(seed)
    sizes = _edge_sizes() + [300]
    params = [rng.normal(0, 0.05, n).astype(np.float32) for n in sizes]
    grads = [[rng.normal(0, 10.0 ** rng.uniform(-3, -1), n).astype(np.float32) for n in sizes] for _ in range(steps)]
    return sizes, params, grads


def _device_adam(params, view_at=None, **kw):
    from pixel_nerf_multiscale_amd.optim import DeviceAdam
    tp = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float32).copy()).cuda()) for p in params]
    if view_at is not None:
        storage = torch.zeros(params[view_at].size + 2, device="cuda")
        storage[1:-1] = torch.from_numpy(params[view_at]).cuda()
        tp[view_at] = torch.nn.Parameter(storage[1:-1])
        assert tp[view_at].data_ptr() % 16 == 4
    kw.setdefault("lr", LR)
    return tp, DeviceAdam(tp, betas=BETAS, eps=EPS, **kw)


def _set_grads(tp, opt, G, times=1.0):
    for i, (t, g) in enumerate(zip(tp, G)):
        if t.grad is None:
            t.grad = opt._slices[i]
        t.grad.copy_(torch.from_numpy((np.asarray(g, dtype=np.float32) * np.float32(times)).astype(np.float32)).view_as(t))


def _state(tp, opt):
    p = [t.detach().cpu().numpy() for t in tp]
    m = [opt.moments(i)[0].cpu().numpy() for i in range(len(tp))]
    v = [opt.moments(i)[1].cpu().numpy() for i in range(len(tp))]
    return p, m, v


def _same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("with_scaler", [False, True])
@pytest.mark.parametrize("max_norm", [None, MAX_NORM])
@pytest.mark.parametrize("div", [2, 8])
def test_a_power_of_two_divisor_is_exact(div, max_norm, with_scaler):
    """The step on div * g with grad_div = div against the step on g with grad_div = 1, three steps: multiplying by a power of two
    and by its inverse are both exact (nothing here is near the ends of fp32's range), so every bit agrees."""
    sizes, params, grads = _edge_case(21, 3)
    kw = dict(max_norm=max_norm, scaler=SCALER if with_scaler else None, view_at=len(sizes) - 1)
    tp_a, opt_a = _device_adam(params, **kw)
    tp_b, opt_b = _device_adam(params, **kw)
    s = 1024.0 if with_scaler else 1.0
    for k, G in enumerate(grads):
        _set_grads(tp_a, opt_a, G, times=s * div)
        _set_grads(tp_b, opt_b, G, times=s)
        opt_a.step(grad_div=div)
        opt_b.step()
        assert float(opt_a.grad_norm) == float(opt_b.grad_norm) and float(opt_a.grad_norm) > 0.0
        assert float(opt_a.clip_coef) == float(opt_b.clip_coef)
        for a, b in zip(_state(tp_a, opt_a), _state(tp_b, opt_b)):
            assert _same_bits(a, b), (k, div)
    assert int(opt_a.step_count) == int(opt_b.step_count) == 3 and float(opt_a.scale_value) == float(opt_b.scale_value)
    # the divisor took part: the same gradients without it give another step
    tp_c, opt_c = _device_adam(params, **kw)
    _set_grads(tp_c, opt_c, grads[0], times=s * div)
    opt_c.step()
    assert float(opt_c.grad_norm) == pytest.approx(div * float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads[0]))),
                                                   rel=1e-6)


@pytest.mark.parametrize("max_norm", [None, MAX_NORM])
def test_divisor_three_against_the_fp64_model(max_norm):
    """grad_div = 3 is no power of two.  include/pnr.h defines the divided gradient as u = fp32(fp32(grad * inv_scale) * inv_div),
    inv_div = fp32(1 / 3): that fp32 array is the model's input (optim_util: everything after the roundings that DEFINE the inputs
    is fp64) and torch's, and the kernel's worst |x - model| over p, m, v may be at most 2x that of torch's own fp32 Adam on the
    CPU in the same case — the bound of the optimiser's tests."""
    sizes, params, grads = _edge_case(22, 3)
    inv_div = np.float32(1.0) / np.float32(3.0)
    tp, opt = _device_adam(params, max_norm=max_norm, view_at=len(sizes) - 1)
    model = ou.AdamModel(params, LR, BETAS, EPS, max_norm)
    ttp, topt, tstep = ou.torch_adam_cpu(params, max_norm=max_norm)
    for k, G in enumerate(grads):
        third = [(g * inv_div).astype(np.float32) for g in G]
        _set_grads(tp, opt, G)
        opt.step(grad_div=3)
        model.step(third)
        tstep(third)
        assert float(opt.clip_coef) == float(model.clip_coef), k
        assert abs(float(opt.grad_norm) - model.grad_norm) <= 64 * 2.0 ** -53 * model.grad_norm
    assert int(opt.step_count) == 3
    for q, a, t, r in zip("pmv", _state(tp, opt), ou.torch_state(ttp, topt), (model.p, model.m, model.v)):
        ek, et = ou.worst(a, r), ou.worst(t, r)
        print(f"grad_div 3, max_norm {max_norm}: max |{q} - model|  kernel {ek:.3e}  torch fp32 {et:.3e}  ratio {ek / et:.2f}")
        assert ek <= 2.0 * et, (q, ek, et)


@pytest.mark.parametrize("with_scaler", [False, True])
@pytest.mark.parametrize("div", [1, 2, 3])
def test_a_non_finite_gradient_skips_the_step_under_any_divisor(div, with_scaler):
    sizes, params, grads = _edge_case(23, 2)
    tp, opt = _device_adam(params, max_norm=MAX_NORM, scaler=SCALER if with_scaler else None)
    s = 1024.0 if with_scaler else 1.0
    _set_grads(tp, opt, grads[0], times=s)
    opt.step(grad_div=div)
    assert int(opt.step_count) == 1 and int(opt.found_inf) == 0
    before = _state(tp, opt)
    for where, value in ((0, np.nan), (len(sizes) - 1, np.inf)):
        bad = [g.copy() for g in grads[1]]
        bad[where].reshape(-1)[-1] = value
        _set_grads(tp, opt, bad, times=s)
        opt.step(grad_div=div)
        assert int(opt.found_inf) == 1 and int(opt.step_count) == 1 and not np.isfinite(float(opt.grad_norm))
        assert float(opt.clip_coef) == 0.0
        for a, b in zip(before, _state(tp, opt)):
            assert _same_bits(a, b)
    assert int(opt.skipped) == 2
    if with_scaler:
        assert float(opt.scale_value) == 256.0


def test_allreduce_without_a_group_is_a_plain_step(monkeypatch):
    """No process group: allreduce() issues no collective and arms a divisor of 1 — the bits of a plain step — and it re-adopts
    a replaced gradient as step() does.  A missing gradient stays missing (there is no other rank to agree with)."""
    import torch.distributed as dist
    calls = []
    monkeypatch.setattr(dist, "all_reduce", lambda *a, **kw: calls.append(a))
    assert not dist.is_initialized()
    sizes, params, grads = _edge_case(24, 2)
    tp_a, opt_a = _device_adam(params, max_norm=MAX_NORM)
    tp_b, opt_b = _device_adam(params, max_norm=MAX_NORM)
    for k, G in enumerate(grads):
        _set_grads(tp_a, opt_a, G)
        _set_grads(tp_b, opt_b, G)
        if k == 1:
            tp_a[3].grad = tp_a[3].grad.clone()             # replaced: re-adopted by allreduce()
            tp_a[5].grad = None
            tp_b[5].grad = None
        opt_a.allreduce()
        assert opt_a._grad_div == 1
        if k == 1:
            assert tp_a[3].grad.data_ptr() == opt_a._slice_ptr[3] and tp_a[5].grad is None
        opt_a.step()
        opt_b.step()
        assert float(opt_a.grad_norm) == float(opt_b.grad_norm)
        for a, b in zip(_state(tp_a, opt_a), _state(tp_b, opt_b)):
            assert _same_bits(a, b)
    assert calls == []
    opt_a._grad_div = 2                                     # what allreduce() arms under two ranks holds for ONE step
    _set_grads(tp_a, opt_a, grads[0], times=2.0)
    _set_grads(tp_b, opt_b, grads[0])
    opt_a.step()
    opt_b.step()
    assert opt_a._grad_div == 1 and float(opt_a.grad_norm) == float(opt_b.grad_norm)
    with pytest.raises(ValueError, match="grad_div"):
        opt_a.step(grad_div=0)
