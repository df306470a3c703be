"""Visualisation on the device: pnr_cmap and pnr_vis_panel against the numpy model of tests/vis_util.py, and train.vis_step,
train.eval_step / validate and evaluate(depth_png=True) on top of them.

Bounds, none of them taken from what the kernels give:
  bytes, minmax, panel (as bit patterns), alpha, stats   exact: include/pnr.h fixes every rounding, the model restates it
  mse vs the model's fp64 value     relative 3 H W 2^-52: two fp64 summation orders over 3 H W non-negative terms
  psnr (device log10) vs the model  the mse bound in dB (10 / ln 10 per unit of relative error) + 2^-50 max(1, |psnr|) for
                                    the two log10 implementations
  alpha vs torch's fp32 sum         K 2^-24 alpha element-wise: K non-negative terms, one fp32 rounding per addition
  vis_step psnr vs util.psnr        1e-5 dB: the reference's value comes from an fp32 numpy mean
"""
import math
import os

import numpy as np
import pytest
import torch

import eval_util as eu
import golden_util as gu
import hip_util as hu
import vis_util as vu

pytestmark = pytest.mark.gpu

# one tile, exact tiles, one extra column, ragged, several tiles; 257 tiles of one ragged row: thread 0 of the one-workgroup
# folds takes two partials
SHAPES = [(1, 1), (16, 16), (17, 16), (19, 13), (33, 17), (4097, 1)]
COMBOS = [(K, NS, n_pass) for K in (1, 3, 24, 65) for NS in (1, 3) for n_pass in (1, 2)]
IDENT = np.arange(256, dtype=np.uint8)[:, None].repeat(3, axis=1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _cmap_dev(m, lut=None):
    from pixel_nerf_multiscale_amd import util
    u8, mm = util.cmap_device(m, lut)
    assert u8.dtype == torch.uint8 and mm.dtype == torch.float32 and tuple(mm.shape) == (2,)
    return u8.cpu().numpy(), mm.cpu().numpy()


def _check_cmap(name, m, lut_np, lut):
    got, mm = _cmap_dev(torch.from_numpy(m).cuda(), lut)
    want = vu.cmap(m, lut_np)
    lo, hi = vu.minmax(m)
    n_diff = int((got != want).any(-1).sum())
    print(f"cmap {name} {m.shape[1]}x{m.shape[0]}: bytes differing {n_diff}, minmax {mm.tolist()} vs {[float(lo), float(hi)]}")
    assert got.shape == m.shape + (3,) and n_diff == 0
    assert np.array_equal(mm, np.array([lo, hi], np.float32), equal_nan=True)
    return got


# ------------------------------------------------------------------------------------------------------------ pnr_cmap
@pytest.mark.parametrize("W,H", SHAPES)
def test_cmap_matches_the_model(W, H):
    from pixel_nerf_multiscale_amd import util
    rng = np.random.default_rng(W * 100 + H)
    lut_np = util.hot_lut()
    maps = {
        "uniform": rng.uniform(0, 1, (H, W)).astype(np.float32),
        "depth": rng.uniform(1.25, 2.75, (H, W)).astype(np.float32),
        "normal": rng.normal(0, 50, (H, W)).astype(np.float32),
        "constant": np.full((H, W), 0.7, np.float32),
        "zeros": np.zeros((H, W), np.float32),
    }
    for special, v in (("nan", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        m = rng.uniform(0, 1, (H, W)).astype(np.float32)
        m[H // 2, W - 1] = v
        maps[special] = m
    for name, m in maps.items():
        got = _check_cmap(name, m, lut_np, None)
        if name in ("constant", "zeros", "nan") or W * H == 1:
            assert (got == lut_np[0]).all()
        elif name in ("uniform", "depth", "normal"):
            assert (got[np.unravel_index(np.argmax(m), m.shape)] == lut_np[255]).all()
    # a strided view: column 2 of an (H*W, 4) per-pixel record; an explicit table (numpy, then a device tensor)
    rec = rng.uniform(-3, 3, (H * W, 4)).astype(np.float32)
    rec_d = torch.from_numpy(rec).cuda()
    for lut in (IDENT, torch.from_numpy(IDENT).cuda()):
        got, mm = _cmap_dev(rec_d.view(H, W, 4)[:, :, 2], lut)
        assert np.array_equal(got, vu.cmap(rec[:, 2].reshape(H, W), IDENT))
        assert np.array_equal(mm, np.array(vu.minmax(rec[:, 2]), np.float32))
    assert np.array_equal(rec_d.cpu().numpy(), rec)                          # the record around the view is untouched


def test_cmap_matches_the_reference_fixture():
    for name, (m, want) in vu.load_quantize_fixture().items():
        got = _check_cmap(name, m, IDENT, IDENT)
        assert np.array_equal(got[..., 0], want) and np.array_equal(got[..., 1], want), name


def test_cmap_is_bit_reproducible_and_keeps_its_bounds():
    """Canaries around the output and the workspace of a ragged, several-tile map; two calls, the same bytes."""
    from pixel_nerf_multiscale_amd import _native as N, util
    W, H, PAD = 33, 17, 64
    m = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (H, W)).astype(np.float32)).cuda()
    lut = torch.from_numpy(util.hot_lut()).cuda()
    need = int(N.lib.pnr_cmap_workspace_bytes(W, H))
    outs = []
    for _ in range(2):
        out = torch.full((PAD + H * W * 3 + PAD,), 77, dtype=torch.uint8, device="cuda")
        ws = torch.full((PAD + need + PAD,), 77, dtype=torch.uint8, device="cuda")
        mm = torch.full((4,), -5.0, device="cuda")
        assert N.lib.pnr_cmap(m.data_ptr(), 0, W, H, lut.data_ptr(), out.data_ptr() + PAD, mm.data_ptr() + 4, ws.data_ptr() + PAD,
                              need, N.current_stream(m.device)) == 0
        torch.cuda.synchronize()
        for buf in (out, ws):
            assert bool((buf[:PAD] == 77).all()) and bool((buf[-PAD:] == 77).all())
        assert mm.cpu().tolist()[0] == -5.0 and mm.cpu().tolist()[3] == -5.0
        outs.append((out.cpu().numpy(), mm.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][0][PAD:-PAD].reshape(H, W, 3), vu.cmap(m.cpu().numpy(), util.hot_lut()))


# ------------------------------------------------------------------------------------------------------- pnr_vis_panel
def _panel_inputs(W, H, K, NS, n_pass, seed):
    rng = np.random.default_rng(seed)
    NV = NS + 2
    images = rng.uniform(-1, 1, (NV, 3, H, W)).astype(np.float32)
    passes = []
    for _ in range(n_pass):
        w = rng.uniform(0, 1, (H * W, K)).astype(np.float32) ** 3
        w = (w / w.sum(-1, keepdims=True) * rng.uniform(0.02, 1.0, (H * W, 1))).astype(np.float32)     # alpha spread over (0, 1]
        w[rng.integers(0, H * W)] = 0.0                                    # an empty ray: alpha 0
        passes.append((rng.uniform(-0.2, 1.2, (H * W, 3)).astype(np.float32),
                       rng.uniform(1.25, 2.75, H * W).astype(np.float32), w))
    src = sorted(rng.choice(NV, NS, replace=False).tolist())
    gt = [v for v in range(NV) if v not in src][int(rng.integers(0, 2))]
    return images, src, gt, passes


def _device_passes(passes, packed):
    """Dense tensors, or views into one packed record of 4 + K floats per ray: [rgb(3), depth(1), weights(K)]."""
    out, keep = [], []
    for rgb, depth, w in passes:
        if packed:
            rec = torch.from_numpy(np.concatenate((rgb, depth[:, None], w), axis=1)).cuda()
            keep.append(rec)
            out.append((rec[:, :3], rec[:, 3], rec[:, 4:]))
        else:
            out.append(tuple(torch.from_numpy(x).cuda() for x in (rgb, depth, w)))
    return out, keep


def _compare_panel(tag, res, m, H, W):
    got_mse = float(res.mse)
    rel = abs(got_mse - m["mse"]) / m["mse"]
    got_psnr, want_psnr = float(res.psnr), -10.0 * math.log10(m["mse"])
    psnr_tol = 10.0 / math.log(10.0) * 3 * H * W * 2.0 ** -52 + 2.0 ** -50 * max(1.0, abs(want_psnr))
    print(f"vis_panel {tag}: mse rel err {rel:.2e} (bound {3 * H * W * 2.0 ** -52:.2e}), |d psnr| {abs(got_psnr - want_psnr):.2e} dB")
    assert res.panel.dtype == torch.float32 and res.panel_u8.dtype == torch.uint8
    assert tuple(res.panel.shape) == m["panel"].shape == tuple(res.panel_u8.shape)
    assert np.array_equal(res.panel_u8.cpu().numpy(), m["panel_u8"])
    assert np.array_equal(_bits(res.panel.cpu().numpy()), _bits(m["panel"]))
    assert np.array_equal(res.alpha.cpu().numpy(), m["alpha"]) and np.array_equal(res.stats.cpu().numpy(), m["stats"])
    assert res.mse.dtype == torch.float64 and res.mse.dim() == 0 and rel <= 3 * H * W * 2.0 ** -52
    assert res.psnr.dtype == torch.float64 and res.psnr.dim() == 0 and res.psnr.is_cuda
    assert abs(got_psnr - want_psnr) <= psnr_tol


@pytest.mark.parametrize("W,H", SHAPES)
def test_vis_panel_matches_the_model(W, H):
    from pixel_nerf_multiscale_amd import util
    lut_np = util.hot_lut()
    for K, NS, n_pass in COMBOS:
        images, src, gt, passes = _panel_inputs(W, H, K, NS, n_pass, seed=W * 1000 + H * 10 + K + 100000 * NS + 1000000 * n_pass)
        m = vu.panel_model(images, src, gt, passes, lut_np)
        img_d = torch.from_numpy(images).cuda()
        for packed in (False, True):
            dev_passes, keep = _device_passes(passes, packed)
            res = util.vis_panel(img_d, src, gt, dev_passes, want_f32=True, want_u8=True, want_alpha=True)
            _compare_panel(f"{W}x{H} K={K} NS={NS} n_pass={n_pass} packed={packed}", res, m, H, W)
            for p in range(n_pass):                       # the colour-map tiles of panel_u8 are the LUT bytes themselves
                for col, src_map in ((NS + 1, passes[p][1].reshape(H, W)), (NS + 3, m["alpha"][p])):
                    tile = res.panel_u8[p * H:(p + 1) * H, col * W:(col + 1) * W].cpu().numpy()
                    assert np.array_equal(tile, vu.cmap(src_map, lut_np))
            # again: the same bits in every output
            res2 = util.vis_panel(img_d, src, gt, dev_passes, want_f32=True, want_u8=True, want_alpha=True)
            for name in ("panel", "panel_u8", "alpha", "stats", "mse", "psnr"):
                a, b = getattr(res, name), getattr(res2, name)
                assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), name
            assert res.mse.view(torch.int64).item() == res2.mse.view(torch.int64).item()
            # mse alone, both panels NULL: the same value
            res3 = util.vis_panel(img_d, src, gt, dev_passes, want_f32=False, want_u8=False)
            assert res3.panel is None and res3.panel_u8 is None and res3.alpha is None
            assert res3.mse.view(torch.int64).item() == res.mse.view(torch.int64).item()
            assert torch.equal(res3.stats, res.stats)
            for rec, (rgb, depth, w) in zip(keep, passes):                  # the records are read, never written
                assert np.array_equal(rec.cpu().numpy(), np.concatenate((rgb, depth[:, None], w), axis=1))


def test_vis_panel_mse_only_through_the_c_interface_keeps_its_bounds():
    """Only `mse` asked for (panels, alpha and stats NULL), canaries around the workspace; then everything asked for, canaries
    around every output."""
    from pixel_nerf_multiscale_amd import _native as N, util
    import ctypes as C
    W, H, K, NS, PAD = 33, 17, 5, 3, 64
    images, src, gt, passes = _panel_inputs(W, H, K, NS, 2, seed=42)
    m = vu.panel_model(images, src, gt, passes, util.hot_lut())
    img_d, lut = torch.from_numpy(images).cuda(), torch.from_numpy(util.hot_lut()).cuda()
    dev_passes, _ = _device_passes(passes, False)
    arr = (N.pnr_vis_pass * 2)()
    for i, (rgb, depth, w) in enumerate(dev_passes):
        arr[i].rgb, arr[i].depth, arr[i].weights, arr[i].K = rgb.data_ptr(), depth.data_ptr(), w.data_ptr(), K
    need = int(N.lib.pnr_vis_panel_workspace_bytes(W, H, 2))
    srcs = (C.c_int32 * NS)(*src)

    def canary(nbytes):
        return torch.full((PAD + nbytes + PAD,), 77, dtype=torch.uint8, device="cuda")

    def intact(buf):
        return bool((buf[:PAD] == 77).all()) and bool((buf[-PAD:] == 77).all())

    n_panel = 2 * H * (NS + 4) * W * 3
    for everything in (False, True):
        ws, mse = canary(need), canary(8)
        f32, u8, alpha, stats = canary(4 * n_panel), canary(n_panel), canary(4 * 2 * H * W), canary(4 * 12)
        at = lambda b: b.data_ptr() + PAD if everything else None
        assert N.lib.pnr_vis_panel(img_d.data_ptr(), NS + 2, srcs, NS, gt, arr, 2, W, H, lut.data_ptr(), at(f32), at(u8), at(alpha),
                                   at(stats), mse.data_ptr() + PAD, ws.data_ptr() + PAD, need, N.current_stream(img_d.device)) == 0
        torch.cuda.synchronize()
        for buf in (ws, mse, f32, u8, alpha, stats):
            assert intact(buf)
        got = float(mse[PAD:-PAD].view(torch.float64)[0])
        assert abs(got - m["mse"]) <= 3 * H * W * 2.0 ** -52 * m["mse"]
        if everything:
            assert np.array_equal(u8[PAD:-PAD].cpu().numpy().reshape(m["panel_u8"].shape), m["panel_u8"])
            assert np.array_equal(f32[PAD:-PAD].view(torch.int32).cpu().numpy().reshape(m["panel"].shape), _bits(m["panel"]))
        else:
            for buf in (f32, u8, alpha, stats):
                assert bool((buf == 77).all())


@pytest.mark.parametrize("K", [1, 3, 24, 65])
def test_alpha_beside_torch(K):
    from pixel_nerf_multiscale_amd import util
    W, H = 33, 17
    images, src, gt, passes = _panel_inputs(W, H, K, 1, 1, seed=K)
    dev_passes, _ = _device_passes(passes, False)
    res = util.vis_panel(torch.from_numpy(images).cuda(), src, gt, dev_passes, want_f32=False, want_alpha=True)
    alpha = res.alpha[0].reshape(-1)
    t_sum = dev_passes[0][2].sum(-1)
    d = (alpha.double() - t_sum.double()).abs()
    bound = K * 2.0 ** -24 * alpha.double()
    a_bytes = vu.cmap(alpha.cpu().numpy().reshape(H, W), IDENT)[..., 0]
    t_bytes = vu.cmap(t_sum.cpu().numpy().reshape(H, W), IDENT)[..., 0]
    print(f"alpha vs torch K={K}: worst |d| / alpha = {float((d / alpha.double().clamp_min(1e-30)).max()):.2e} "
          f"(bound {K * 2.0 ** -24:.2e}); colour-map bytes differing: {int((a_bytes != t_bytes).sum())} of {H * W}")
    assert bool((d <= bound).all())


# ------------------------------------------------------------------------------------------------- train.py on the device
Z_NEAR, Z_FAR = 1.25, 2.75
SB, NV, H, W = 2, 5, 12, 16


def _setup(case="tiny_ns2_codeview"):
    """A tiny fixture net (hip_util.build_net on a tiny spec; coarse 8 + fine 6 samples) whose encoder is a fixed function of
    the source images, as tests/test_gpu_train_front.py stubs it, and a loader-style batch of host tensors."""
    fx, spec, net, rend = hu.setup(case)
    rend.fixed_noise = None
    C_lat, Hl, Wl = spec["lat"][0]

    def encoder(images):
        pooled = torch.nn.functional.adaptive_avg_pool2d(images, (Hl, Wl))
        net.encoder.set_latents([torch.relu(pooled.repeat(1, (C_lat + 2) // 3, 1, 1)[:, :C_lat] * 2.0 + 0.5).detach()])

    net.encoder.forward = encoder
    rng = np.random.default_rng(78)
    data = {
        "images": torch.from_numpy(rng.uniform(-1, 1, (SB, NV, 3, H, W)).astype(np.float32)),
        "poses": torch.from_numpy(np.stack([np.stack([gu.pose_spherical(25.0 * v + 40.0 * o, -20.0 - 4.0 * v, spec["radius"])
                                                      for v in range(NV)]) for o in range(SB)])),
        "focal": torch.tensor([18.0, 19.5]),
        "c": torch.tensor([[8.25, 5.5], [7.5, 6.25]]),
    }
    return net, rend, data


def _host_panel(net, render_par, data, nviews, seed, idx=None):
    """vis_step the reference's way (train.py:429-531) on this package's renderer: the same draws, an independent render_par
    call on the same rays, copies to the host, the model's cmap, np.hstack / np.vstack, util.psnr."""
    from pixel_nerf_multiscale_amd import util
    torch.manual_seed(seed); np.random.seed(seed)
    b = np.random.randint(0, data["images"].shape[0]) if idx is None else idx
    k = nviews[torch.randint(0, len(nviews), (1,)).item()]
    views_src = np.sort(np.random.choice(NV, k, replace=False))
    view_dest = np.random.randint(0, NV - k)
    for vs in range(k):
        view_dest += view_dest >= views_src[vs]
    images = data["images"][b]
    rays = util.gen_rays_device(data["poses"][b][view_dest], W, H, data["focal"][b], Z_NEAR, Z_FAR, c=data["c"][b])
    with torch.no_grad():
        net.encode(images[views_src].cuda()[None], data["poses"][b][views_src].cuda()[None], data["focal"][b:b + 1].cuda(),
                   c=data["c"][b:b + 1].cuda())
        rd = render_par(rays[None], want_weights=True)
    lv = [rd["coarse"]] + ([rd["fine"]] if rd.get("fine") is not None and len(rd["fine"]) > 0 else [])
    passes = [(p["rgb"][0].cpu().numpy(), p["depth"][0].cpu().numpy(), p["weights"][0].cpu().numpy()) for p in lv]
    rows, _ = vu.pieces(images.numpy(), views_src.tolist(), int(view_dest), passes, vu.model_lut(), W, H)
    vis = np.hstack(rows[0])
    if len(rows) == 2:
        vis = np.vstack((vis, np.hstack(rows[1])))
    gt = (images * 0.5 + 0.5)[view_dest].permute(1, 2, 0).numpy().reshape(H, W, 3)
    return vis, util.psnr(passes[-1][0].reshape(H, W, 3), gt), len(views_src)


@pytest.mark.parametrize("nviews", [[1], [3]])
def test_vis_step_end_to_end(nviews):
    from pixel_nerf_multiscale_amd import train
    net, rend, data = _setup()
    render_par = rend.bind_parallel(net, None)
    for seed, rend_mode, net_mode in ((5, True, False), (6, False, True)):
        want, want_psnr, NS = _host_panel(net, render_par, data, nviews, seed)
        rend.train(rend_mode); net.train(net_mode)
        torch.manual_seed(seed); np.random.seed(seed)
        vis, vals = train.vis_step(net, rend, render_par, data, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR)
        assert rend.training is rend_mode and net.training is net_mode
        assert NS == nviews[0] and tuple(vis.shape) == (2 * H, (NS + 4) * W, 3) == want.shape and vis.dtype == torch.float32
        n_diff = int((_bits(vis.cpu().numpy()) != _bits(want)).sum())
        psnr = vals["psnr"]
        print(f"vis_step nviews={nviews} seed={seed}: panel elements differing {n_diff}, psnr {float(psnr):.6f} vs host {want_psnr:.6f}")
        assert n_diff == 0
        assert sorted(vals) == ["psnr"] and psnr.is_cuda and psnr.dim() == 0 and psnr.dtype == torch.float64
        assert abs(float(psnr) - want_psnr) <= 1e-5
        torch.manual_seed(seed); np.random.seed(seed)
        vis8, _ = train.vis_step(net, rend, render_par, data, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR, out="uint8")
        assert vis8.dtype == torch.uint8 and np.array_equal(vis8.cpu().numpy(), vu.to_u8(want))
    rend.eval(); net.eval()
    # idx picks the object: no batch draw is consumed
    want, want_psnr, _ = _host_panel(net, render_par, data, nviews, 11, idx=1)
    torch.manual_seed(11); np.random.seed(11)
    vis, vals = train.vis_step(net, rend, render_par, data, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR, idx=1, verbose=True)
    assert np.array_equal(_bits(vis.cpu().numpy()), _bits(want)) and abs(float(vals["psnr"]) - want_psnr) <= 1e-5


def test_vis_step_without_a_fine_pass():
    from pixel_nerf_multiscale_amd import train
    net, rend, data = _setup("tiny_ns1_coarse_only")
    assert not rend.using_fine
    render_par = rend.bind_parallel(net, None)
    want, want_psnr, NS = _host_panel(net, render_par, data, [2], 21)
    torch.manual_seed(21); np.random.seed(21)
    vis, vals = train.vis_step(net, rend, render_par, data, nviews=[2], z_near=Z_NEAR, z_far=Z_FAR)
    assert tuple(vis.shape) == (H, (2 + 4) * W, 3) == want.shape                      # one row
    assert np.array_equal(_bits(vis.cpu().numpy()), _bits(want))
    assert abs(float(vals["psnr"]) - want_psnr) <= 1e-5                               # PSNR of the coarse colours


def test_vis_step_does_not_wait_for_the_device():
    from pixel_nerf_multiscale_amd import train
    net, rend, data = _setup()
    render_par = rend.bind_parallel(net, None)
    kw = dict(nviews=[3], z_near=Z_NEAR, z_far=Z_FAR)
    torch.manual_seed(3); np.random.seed(3)
    train.vis_step(net, rend, render_par, data, **kw)           # warm-up: allocations, code objects, the cached table
    works = eu.sync_debug_mode_works()
    print(f'torch.cuda.set_sync_debug_mode("error") works under this build: {works}')
    if not works:
        print("vis_step's freedom from host waits could not be checked under this build")
    torch.manual_seed(3); np.random.seed(3)
    if works:
        torch.cuda.set_sync_debug_mode("error")
    try:
        vis, vals = train.vis_step(net, rend, render_par, data, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert vis.is_cuda and vals["psnr"].is_cuda and math.isfinite(float(vals["psnr"]))


def test_eval_step_and_validate():
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend, data = _setup()
    render_par = rend.bind_parallel(net, None)
    rng = np.random.default_rng(79)
    data2 = dict(data, images=torch.from_numpy(rng.uniform(-1, 1, (SB, NV, 3, H, W)).astype(np.float32)))
    kw = dict(ray_batch_size=32, nviews=[2], z_near=Z_NEAR, z_far=Z_FAR, loss=RenderLoss(0.7, 1.3))
    loader = [data, None, {"poses": data["poses"]}, data2]

    torch.manual_seed(13); np.random.seed(13)
    rend.eval()
    want = []
    with torch.no_grad():
        for d in (data, data2):
            want.append(float(train.calc_losses(net, render_par, d, is_train=False, **kw)[1]["t"]))
    for rend_mode, net_mode in ((True, True), (False, False)):
        rend.train(rend_mode); net.train(net_mode)
        if net_mode:
            net.train_precision = "fp32"
        for p in net.parameters():
            p.grad = None
        torch.manual_seed(13); np.random.seed(13)
        got = train.validate(net, rend, render_par, loader, **kw)
        print(f"validate: {got!r} vs mean of two calc_losses(is_train=False) {(want[0] + want[1]) / 2!r}")
        assert isinstance(got, float) and got == (want[0] + want[1]) / 2
        assert rend.training is rend_mode and net.training is net_mode
        assert all(p.grad is None for p in net.parameters())
    torch.manual_seed(13); np.random.seed(13)
    d = train.eval_step(net, rend, render_par, data, **kw)
    assert sorted(d) == ["rc", "rf", "t"] and all(v.is_cuda and v.dim() == 0 and not v.requires_grad for v in d.values())
    assert float(d["t"]) == want[0]
    assert train.validate(net, rend, render_par, [None, {}], **kw) == float("inf")


# ---------------------------------------------------------------------------------------------- evaluate(depth_png=True)
@pytest.mark.parametrize("metrics", ["host", "device"])
def test_evaluate_writes_the_depth_png(metrics, tmp_path):
    from pixel_nerf_multiscale_amd import evalio, util
    net, rend, data = _setup()
    toy = eu.Objects([dict(path="/data/cat0/obj000", images=data["images"][0][:2], poses=data["poses"][0][:2], focal=18.0)])
    kw = dict(source="0", verbose=False, seed=777, metrics=metrics, no_compare_gt=True)
    plain = str(tmp_path / "plain")
    evalio.evaluate(net, rend, toy, plain, write_depth=True, **kw)
    assert sorted(os.listdir(os.path.join(plain, "obj000"))) == ["000001.png", "000001_depth.npy"]      # today's files
    out = str(tmp_path / "with_png")
    evalio.evaluate(net, rend, toy, out, write_depth=True, depth_png=True, **kw)
    assert sorted(os.listdir(os.path.join(out, "obj000"))) == ["000001.png", "000001_depth.npy", "000001_depth_norm.png"]
    dn = np.load(os.path.join(out, "obj000", "000001_depth.npy"))
    assert dn.shape == (H, W) and np.array_equal(dn, np.load(os.path.join(plain, "obj000", "000001_depth.npy")))
    png = eu.read_png(os.path.join(out, "obj000", "000001_depth_norm.png"))
    assert png.shape == (H, W, 3) and np.array_equal(png, util.cmap(dn)) and len(np.unique(png.reshape(-1, 3), axis=0)) >= 2
    # an explicit table; and depth_png without write_depth writes nothing new
    out2 = str(tmp_path / "ident")
    evalio.evaluate(net, rend, toy, out2, write_depth=True, depth_png=True, lut=IDENT, **kw)
    png2 = eu.read_png(os.path.join(out2, "obj000", "000001_depth_norm.png"))
    assert np.array_equal(png2, util.cmap(np.load(os.path.join(out2, "obj000", "000001_depth.npy")), IDENT))
    out3 = str(tmp_path / "no_depth")
    evalio.evaluate(net, rend, toy, out3, depth_png=True, **kw)
    assert sorted(os.listdir(os.path.join(out3, "obj000"))) == ["000001.png"]
