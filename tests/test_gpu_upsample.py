"""Upstream pixelNeRF's latent map on the device (csrc/upsample.hip; include/pnr.h fixes the arithmetic): the forward kernels
bit for bit against the numpy restatement (tests/upsample_util.py model32) and its round-to-nearest-even 16-bit conversion,
the gather backward inside its derived bound of the fp64 adjoint and reproducible to the bit, util.upsample_concat under
autograd, and a PixelNeRFNet with encoder.latent_mode = "upstream" rendering and training through the unchanged kernels.

What is pinned: torch's own F.interpolate + cat in fp64 (tests/test_upsample_cpu.py ties model64 / adjoint64 to it) and the
oracle's lookup on the map built that way.  Parity against upstream pixelNeRF itself is unpinned (its code is not at hand)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import upsample_util as U
from oracle_util import maxdiff
from test_gpu_parity import FINE_E2E_FLOOR_DB, FLOOR_DB, _psnr
from test_gpu_train import RTOL

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def _sizes(shapes):
    arr = lambda k: (C.c_int32 * len(shapes))(*[int(s[k]) for s in shapes])
    return arr(1), arr(2), arr(3)


def kernel_forward(levels, want_out=True, half=None):
    """pnr_upsample_concat on device tensors -> (out (N, sumC, H0, W0) or None, out16 as a flat (N, H0, W0, sumC) buffer or None)."""
    from pixel_nerf_multiscale_amd import _native as N
    shapes = [tuple(l.shape) for l in levels]
    n, (h0, w0), sum_c = shapes[0][0], shapes[0][2:], sum(s[1] for s in shapes)
    out = torch.full((n, sum_c, h0, w0), float("nan"), device="cuda") if want_out else None
    out16 = torch.full((n, h0, w0, sum_c), float("nan"), device="cuda", dtype=half) if half is not None else None
    ptrs = (C.c_void_p * len(levels))(*[l.data_ptr() for l in levels])
    dt = {None: N.PNR_F32, torch.float16: N.PNR_F16, torch.bfloat16: N.PNR_BF16}[half]
    N.check(N.lib.pnr_upsample_concat(ptrs, *_sizes(shapes), len(levels), n, None if out is None else out.data_ptr(),
                                      None if out16 is None else out16.data_ptr(), dt, N.current_stream(levels[0].device)),
            "pnr_upsample_concat")
    return out, out16


def kernel_backward(g, shapes, skip=(), fill=None):
    """pnr_upsample_concat_bwd -> one gradient per level; the levels in `skip` get a NULL entry (and return None)."""
    from pixel_nerf_multiscale_amd import _native as N
    fill = float("nan") if fill is None else fill
    outs = [None if i in skip else torch.full(tuple(s), fill, device="cuda") for i, s in enumerate(shapes)]
    ptrs = (C.c_void_p * len(shapes))(*[None if o is None else o.data_ptr() for o in outs])
    N.check(N.lib.pnr_upsample_concat_bwd(g.data_ptr(), *_sizes(shapes), len(shapes), shapes[0][0], ptrs,
                                          N.current_stream(g.device)), "pnr_upsample_concat_bwd")
    return outs


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_forward_equals_the_fp32_model_bit_for_bit(name):
    levels = U.make_levels(name)
    dev = [torch.from_numpy(l).cuda() for l in levels]
    out, _ = kernel_forward(dev)
    want = U.model32(levels)
    got = out.cpu().numpy()
    assert got.shape == want.shape
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    print(f"{name}: kernel vs model32 max abs difference {diff:.3e}")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for d, l in zip(dev, levels):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), l.view(np.uint32))        # the levels are left as they were


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16])
def test_out16_is_the_rounded_fp32_value_in_channels_last_order(half):
    levels = U.make_levels("B")
    dev = [torch.from_numpy(l).cuda() for l in levels]
    want = torch.from_numpy(U.model32(levels)).to(half).permute(0, 2, 3, 1).contiguous()   # torch rounds to nearest even
    out, both = kernel_forward(dev, True, half)
    _, alone = kernel_forward(dev, False, half)
    assert torch.equal(_bits(both.cpu()), _bits(want))
    assert torch.equal(_bits(alone), _bits(both))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), U.model32(levels).view(np.uint32))


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_backward_is_inside_its_bound_skips_null_and_repeats_to_the_bit(name):
    """|kernel - adjoint64| <= 8 x 2^-24 x adjoint_abs64 elementwise: at most 5 roundings in w = fl(wy wx) (lam and mu of two
    axes, the product), fp64 products and sums, one final rounding."""
    levels = U.make_levels(name)
    shapes = [l.shape for l in levels]
    g_np = U.make_cotangent(name)
    g = torch.from_numpy(g_np).cuda()
    got = kernel_backward(g, shapes)
    again = kernel_backward(g, shapes, fill=7.0)
    ref, scale = U.adjoint64(g_np, shapes), U.adjoint_abs64(g_np, shapes)
    # torch's own fp32 backward (atomics on the device) for the record
    leaves = [torch.from_numpy(l).cuda().requires_grad_(True) for l in levels]
    size = tuple(shapes[0][2:])
    torch.cat([F.interpolate(l, size=size, mode="bilinear", align_corners=True) for l in leaves], dim=1).backward(g)
    for i, (k, k2, a, s, lf) in enumerate(zip(got, again, ref, scale, leaves)):
        kn = k.cpu().numpy().astype(np.float64)
        rel = lambda v: float((np.abs(v - a) / np.maximum(s, 1e-300)).max()) / EPS
        print(f"{name} level {i}: kernel {rel(kn):.2f} x 2^-24, torch fp32 backward {rel(lf.grad.cpu().numpy().astype(np.float64)):.2f} x 2^-24")
        assert (np.abs(kn - a) <= 8 * EPS * s).all(), (name, i)
        assert torch.equal(_bits(k), _bits(k2)), (name, i)                      # written (=), whatever the buffer held
    skipped = kernel_backward(g, shapes, skip=(len(shapes) - 1,))
    assert skipped[-1] is None
    for k, k3 in zip(got[:-1], skipped[:-1]):
        assert torch.equal(_bits(k), _bits(k3))
    if len(shapes) > 2:
        only = kernel_backward(g, shapes, skip=(0, 1))
        assert only[0] is None and only[1] is None and torch.equal(_bits(only[2]), _bits(got[2]))


def test_upsample_concat_under_autograd():
    from pixel_nerf_multiscale_amd import util
    levels = U.make_levels("B")
    shapes = [l.shape for l in levels]
    g = torch.from_numpy(U.make_cotangent("B")).cuda()
    leaves = [torch.from_numpy(l).cuda().requires_grad_(i != 2) for i, l in enumerate(levels)]
    out = util.upsample_concat(leaves)
    assert np.array_equal(out.detach().cpu().numpy().view(np.uint32), U.model32(levels).view(np.uint32))
    out.backward(g)
    want = kernel_backward(g, shapes)
    assert leaves[2].grad is None                                              # no requires_grad: no gradient, no launch for it
    for i in (0, 1, 3):
        assert torch.equal(_bits(leaves[i].grad), _bits(want[i])), i
    # both outputs; the 16-bit one is channels-last and carries no graph
    out32, out16 = util.upsample_concat(leaves, torch.bfloat16)
    assert out32.requires_grad and not out16.requires_grad
    assert out16.shape == out32.shape and out16.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(out16.cpu(), torch.from_numpy(U.model32(levels)).to(torch.bfloat16))
    with torch.no_grad():
        assert not util.upsample_concat(leaves).requires_grad
    with pytest.raises(ValueError):
        util.upsample_concat([leaves[0], leaves[1][:, :7]], torch.float16)       # sumC % 8 != 0 with a 16-bit output
    with pytest.raises(ValueError):
        util.upsample_concat([leaves[0].double()])
    with pytest.raises(RuntimeError):
        util.upsample_concat([leaves[0].detach().cpu()])                         # no CPU fall-back


# ------------------------------------------------------------------------------------------------- end to end
def _spec():
    spec = dict(gu.CASES["full_multiscale_ns2"])
    spec.update(lat=[(512, 16, 16)], image=(32, 32), NS=2, N=64, Kc=8, Kf=6, Kfd=2, seed=77, depth_std=0.01)
    return spec


def _upstream_net(spec, precision, poses=None):
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import PixelNeRFNet
    conf = model_conf(spec, precision)
    conf["encoder"] = dict(backbone="resnet34", pretrained=False, num_layers=4, use_first_pool=True, latent_mode="upstream")
    torch.manual_seed(0)                                                         # the trunk's initialisation
    net = PixelNeRFNet(conf)
    assert net.d_latent == 512 and net.mlp_coarse.d_hidden == 512 and net.encoder.uv_scale == "image"
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()}, strict=True)
    return net.cuda().eval()


def _inputs(spec, n_rays):
    spec = dict(spec, N=n_rays)
    rays, poses = gu.make_inputs(spec)
    g = torch.Generator().manual_seed(spec["seed"])
    W, H = spec["image"]
    images = torch.rand(spec["SB"], spec["NS"], 3, H, W, generator=g) * 2 - 1
    n_imp = spec["Kf"] - spec["Kfd"]
    noise = dict(noise_c=torch.rand(n_rays, spec["Kc"], generator=g), u=torch.rand(n_rays, n_imp, generator=g),
                 r=torch.rand(n_rays, n_imp, generator=g), g=torch.randn(n_rays, spec["Kfd"], generator=g))
    return torch.from_numpy(rays), torch.from_numpy(poses), images, noise


def _torch_map(feats, dtype):
    size = tuple(feats[0].shape[2:])
    return torch.cat([F.interpolate(f.to(dtype), size=size, mode="bilinear", align_corners=True) for f in feats], dim=1)


def test_upstream_mode_renders_through_the_unchanged_kernels():
    """Expected values: the oracle's render on the ONE map the test builds itself — level_features, then torch's fp64
    F.interpolate + cat — with focal and principal point scaled by 16 / 32: uv s = -x/z (s f) + s c, so the fork's lookup
    under the scaled camera is upstream's lookup (uv_scale = "image") under the original one (tests/test_gpu_uv_scale.py);
    the x and y ratios are equal here.  fp32 path: the 1e-4 of test_gpu_parity.  fp16 kernel against the fp32 path: FLOOR_DB on
    the coarse pass and FINE_E2E_FLOOR_DB end to end on the fine pass, as everywhere in test_gpu_parity."""
    from hip_util import build_renderer, camera_tensors
    from oracle import pixelnerf_oracle as orc
    spec = _spec()
    rays, poses, images, noise = _inputs(spec, 64)
    W, H = spec["image"]
    focal = camera_tensors(spec)[0]
    outs, nets = {}, {}
    for p in ("fp32", "fp16"):
        net = _upstream_net(spec, p)
        with torch.no_grad():
            net.encode(images.cuda(), poses.cuda(), focal)
        assert tuple(net.encoder.latent.shape) == (2, 512, 16, 16) and len(net.encoder.level_maps()) == 1
        assert net.resolved_precision(net.mlp_coarse, net.mlp_fine) == p
        rend = build_renderer(spec)
        rend.fixed_noise = {k: v.cuda() for k, v in noise.items()}
        outs[p] = rend(net, rays.cuda(), want_weights=True)
        nets[p] = (net, rend)
    net = nets["fp32"][0]
    with torch.no_grad():
        feats = [f.cpu() for f in net.encoder.level_features(images.reshape(-1, 3, H, W).cuda())]
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 16, 16), (64, 8, 8), (128, 4, 4), (256, 2, 2)]
    lat = _torch_map(feats, torch.float64)
    # the kernel is exact to 8 x 2^-24 (bit tests above); the rest of the allowance is for the trunk, which ran a second time
    # here and may have taken another convolution algorithm (fp32 sums of up to 2304 terms in another order)
    assert maxdiff(net.encoder.latent.cpu(), lat.float()) <= 1e-5 * float(lat.max())
    s = 16.0 / 32.0
    cam = orc.encode_cameras(poses, *gu.intrinsics(spec), W, H)
    sd = {w: {k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, w).items()} for w in ("coarse", "fine")}
    with torch.no_grad():
        ref = orc.render(sd["coarse"], sd["fine"], (cam[0], cam[1] * s, cam[2] * s), [lat.float()], rays, spec["NS"],
                         spec["Kc"], spec["Kf"], spec["Kfd"], spec["depth_std"], spec["white_bkgd"], spec["lindisp"], noise,
                         use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"],
                         combine_layer=spec["combine_layer"], combine_type=spec["combine_type"])
    for lvl in ("coarse", "fine"):
        d = maxdiff(outs["fp32"][lvl].rgb.cpu(), ref[lvl]["rgb"])
        print(f"fp32 path vs oracle, {lvl} rgb: {d:.2e}")
        assert d <= 1e-4, lvl
    # the latents matter: without them the picture is another one
    net.encoder.set_latents([torch.zeros_like(net.encoder.latent)])
    assert maxdiff(nets["fp32"][1](net, rays.cuda()).coarse.rgb.cpu(), ref["coarse"]["rgb"]) > 1e-2
    db_c = _psnr(outs["fp16"].coarse.rgb.cpu(), outs["fp32"].coarse.rgb.cpu())
    db_f = _psnr(outs["fp16"].fine.rgb.cpu(), outs["fp32"].fine.rgb.cpu())
    print(f"fp16 kernel vs fp32 path: coarse {db_c:.1f} dB, fine {db_f:.1f} dB")
    assert db_c >= FLOOR_DB["fp16"] and db_f >= FINE_E2E_FLOOR_DB["fp16"]
    # half_dtype: the kernel's own 16-bit output is what the render kernel gathers from — by pointer, no repack
    net16, rend16 = nets["fp16"]
    net16.encoder.half_dtype = torch.float16
    with torch.no_grad():
        net16.encode(images.cuda(), poses.cuda(), focal)
    m16 = net16.encoder.level_maps16(torch.float16)
    assert m16 is not None and len(m16) == 1 and m16[0].dtype == torch.float16 and tuple(m16[0].shape) == (2, 512, 16, 16)
    assert m16[0].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(m16[0].cpu(), net16.encoder.latent.cpu().to(torch.float16))      # RNE of the fp32 map of the same call
    v, keep = net16.views_struct("fp16")
    assert v.latent_packed[0] == m16[0].data_ptr()
    out16 = rend16(net16, rays.cuda()).coarse.rgb.cpu()
    assert _psnr(out16, outs["fp32"].coarse.rgb.cpu()) >= 45.0       # the trunk ran under autocast: test_gpu_parity's N2 figure


def test_upstream_mode_trains_through_the_unchanged_kernels():
    """The same net in train(), L2 loss on 32 rays.  A twin with the same weights builds its map with torch's F.interpolate +
    cat: the gradients that reach the first and the last convolution below the map agree within RTOL of each tensor's maximum.
    What the map's adjoint hands to the four levels is the same to the bit from run to run.  That gradient is taken on a view
    of each level, so that nothing the convolutions below add is in it, and the repeated runs start from the level tensors the
    first run's trunk produced: the trunk's convolutions and batch norms are MIOpen's, forward as well as backward, and are not
    claimed reproducible — from the levels onwards (map, render, loss, render backward, the map's adjoint) everything is."""
    from hip_util import build_renderer, camera_tensors
    spec = _spec()
    rays, poses, images, noise = _inputs(spec, 32)
    focal = camera_tensors(spec)[0]
    target = torch.rand(1, 32, 3, generator=torch.Generator().manual_seed(8))
    net = _upstream_net(spec, "fp32").train()
    twin = copy.deepcopy(net)
    rend = build_renderer(spec).train()
    rend.fixed_noise = {k: v.cuda() for k, v in noise.items()}
    x = images.reshape(-1, *images.shape[2:]).cuda()
    names = ("conv1.weight", "layer3.5.conv2.weight")

    def loss_of(n):
        out = rend(n, rays.cuda())
        return ((out.coarse.rgb - target.cuda()) ** 2).mean() + ((out.fine.rgb - target.cuda()) ** 2).mean()

    def run_kernel():
        taps = []
        plain = type(net.encoder).level_features

        def tapped(x_):
            views = [f.view_as(f) for f in plain(net.encoder, x_)]
            for v in views:
                v.retain_grad()
            taps.extend(views)
            return views
        net.encoder.level_features = tapped
        try:
            net.zero_grad(set_to_none=True)
            net.encode(images.cuda(), poses.cuda(), focal)
            assert net.encoder.latent.requires_grad
            loss = loss_of(net)
            loss.backward()
        finally:
            del net.encoder.level_features
        params = dict(net.encoder.model.named_parameters())
        return (float(loss.detach()), [t.detach().clone() for t in taps], [t.grad.clone() for t in taps],
                {k: params[k].grad.clone() for k in names})

    def run_from_levels(levels):
        from pixel_nerf_multiscale_amd import util
        leaves = [l.clone().requires_grad_(True) for l in levels]
        net.encoder.set_latents([util.upsample_concat(leaves)])
        loss_of(net).backward()
        return [l.grad.clone() for l in leaves]

    loss1, levels, lv1, g1 = run_kernel()
    assert len(lv1) == 4 and [tuple(t.shape[1:]) for t in lv1] == [(64, 16, 16), (64, 8, 8), (128, 4, 4), (256, 2, 2)]
    lv2, lv3 = run_from_levels(levels), run_from_levels(levels)
    for a, b, c in zip(lv1, lv2, lv3):
        assert float(a.abs().max()) > 0
        assert torch.equal(_bits(b), _bits(c))                   # two runs from the same levels
        assert torch.equal(_bits(a), _bits(b))                   # and the run through encode(), whose levels these were

    twin.zero_grad(set_to_none=True)
    twin.encoder.set_latents([_torch_map(twin.encoder.level_features(x), torch.float32)])
    twin.num_objs, twin.num_views_per_obj = 1, spec["NS"]
    twin.set_cameras(poses.reshape(-1, 4, 4).cuda(), focal, None, *spec["image"])
    loss_t = loss_of(twin)
    loss_t.backward()
    assert abs(loss1 - float(loss_t)) <= 1e-4 * max(1.0, abs(float(loss_t)))
    tp = dict(twin.encoder.model.named_parameters())
    for k in names:
        ref = tp[k].grad
        d, scale = float((g1[k] - ref).abs().max()), float(ref.abs().max())
        print(f"d {k}: kernel map vs torch map {d:.2e} of max {scale:.2e}")
        assert scale > 0 and d <= RTOL * scale, k
