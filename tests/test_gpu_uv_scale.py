"""Opt-in upstream texel mapping ("expose upstream scaling only as an opt-in flag").

The reference fork's SpatialEncoder.index (encoder.py:152-164) normalises uv by the latent size and ignores image_size —
the default here, pinned by every fixture.  `encoder.uv_scale = "image"` selects upstream pixelNeRF's mapping
(texel = uv * latent_size / image_size per level; pnr_views.uv_scale_x / _y in the C ABI) for checkpoints trained with
upstream semantics.  PARITY UNPINNED against the reference (it holds no fixture for that mapping); what IS checked: a pure
rescaling of uv is a rescaling of (focal, c), so the oracle restatement of the FORK's lookup with a scaled camera must
agree with the scaled lookup on the original camera — module call, fp32 render path, fused 16-bit kernel, gradients.
"""
import numpy as np
import pytest
import torch

import golden_util as gu
from oracle_util import maxdiff
from test_gpu_parity import FLOOR_DB, _psnr

pytestmark = pytest.mark.gpu


def test_index_with_image_scaling_matches_the_per_level_rescaled_lookup():
    from hip_util import setup
    from oracle import pixelnerf_oracle as orc
    fx, spec, net, rend = setup("tiny_multiscale_ns2")
    maps = [m.cpu() for m in net.encoder.level_maps()]
    nv = maps[0].shape[0]
    W, H = spec["image"]
    g = torch.Generator().manual_seed(9)
    uv = (torch.rand(nv, 57, 2, generator=g) * 1.3 - 0.15) * torch.tensor([float(W), float(H)])
    base = net.encoder.index(uv.cuda(), image_size=(W, H)).cpu()          # default: image_size ignored, like the reference
    assert maxdiff(base, orc.index_latent(uv, maps)) <= 1e-5 * max(1.0, float(base.abs().max()))
    net.encoder.uv_scale = "image"
    out = net.encoder.index(uv.cuda(), image_size=(W, H)).cpu()
    ref = torch.cat([orc.index_latent(uv * torch.tensor([m.shape[3] / W, m.shape[2] / H]), [m]) for m in maps], dim=1)
    assert maxdiff(out, ref) <= 1e-5 * max(1.0, float(ref.abs().max()))
    assert float((out - base).abs().max()) > 1e-3                          # it is a different lookup
    with pytest.raises(ValueError):
        net.encoder.index(uv.cuda())                                       # the scaled lookup needs the image size
    net.encoder.uv_scale = "latent"


@pytest.mark.parametrize("name", ["full_ns1", "full_ns3"])
def test_render_with_image_scaling_equals_the_fork_lookup_under_a_scaled_camera(name):
    """Single-level shapes: uv * s = -x/z * (s f) + s c, so the oracle (fork lookup) with focal and principal point scaled
    by s = latent_size / image_size is the upstream lookup on the original camera."""
    from hip_util import build_net, build_renderer
    from oracle import pixelnerf_oracle as orc
    from oracle_util import noise_from_fixture
    fx = gu.load_fixture(name)
    spec = fx["spec"]
    W, H = spec["image"]
    C_, Hl, Wl = spec["lat"][0]
    sx, sy = Wl / W, Hl / H
    assert sx == sy
    cam = orc.encode_cameras(torch.from_numpy(fx["poses"]), *gu.intrinsics(spec), W, H)
    cam_s = (cam[0], cam[1] * sx, cam[2] * sx)
    noise = noise_from_fixture(fx)
    sd_c = {k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, "coarse").items()}
    sd_f = {k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, "fine").items()}
    rays = torch.from_numpy(fx["rays"])
    with torch.no_grad():
        ref = orc.render(sd_c, sd_f, cam_s, [torch.from_numpy(x) for x in gu.make_latents(spec)], rays, spec["NS"],
                         spec["Kc"], spec["Kf"], spec["Kfd"], spec["depth_std"], spec["white_bkgd"], spec["lindisp"], noise,
                         use_code_viewdirs=spec["use_code_viewdirs"])
    outs = {}
    for p in ("fp32", "fp16", "bf16"):
        net = build_net(spec, fx["poses"], "cuda", p)
        net.encoder.uv_scale = "image"
        rend = build_renderer(spec)
        rend.fixed_noise = {k: v.cuda() for k, v in noise.items()}
        outs[p] = rend(net, rays.cuda(), want_weights=True)
        if p == "fp32":
            net.encoder.uv_scale = "latent"
            plain = rend(net, rays.cuda())
            assert float((plain.coarse.rgb - outs[p].coarse.rgb).abs().max()) > 1e-3
    assert maxdiff(outs["fp32"].coarse.rgb.cpu(), ref["coarse"]["rgb"]) <= 1e-4
    assert maxdiff(outs["fp32"].coarse.weights.cpu(), ref["coarse"]["weights"]) <= 1e-4
    assert maxdiff(outs["fp32"].fine.rgb.cpu(), ref["fine"]["rgb"]) <= 1e-4
    for p in ("fp16", "bf16"):           # the fused kernel (projected stream: the tap-weight image is built from the scaled uv)
        assert _psnr(outs[p].coarse.rgb.cpu(), ref["coarse"]["rgb"]) >= FLOOR_DB[p], p


def test_image_scaling_carries_into_the_gradients():
    """d(lookup)/d(uv) picks up the scale: gradients w.r.t. the sample positions of the scaled lookup equal autograd's
    through the oracle with the scaled camera."""
    from hip_util import build_net, build_renderer
    from oracle import pixelnerf_oracle as orc
    name = "tiny_ns1"
    fx = gu.load_fixture(name)
    spec = fx["spec"]
    W, H = spec["image"]
    C_, Hl, Wl = spec["lat"][0]
    sx, sy = Wl / W, Hl / H
    net = build_net(spec, fx["poses"], "cuda", "fp32")
    net.encoder.uv_scale = "image"
    net.train()
    rays = torch.from_numpy(fx["rays"]).cuda()
    g = torch.Generator().manual_seed(2)
    K = 6
    z = (spec["z_near"] + (spec["z_far"] - spec["z_near"]) * torch.rand(rays.shape[1], K, generator=g)).cuda().requires_grad_(True)
    from pixel_nerf_multiscale_amd.render.autograd import point_mlp_rays
    out = point_mlp_rays(net, net.mlp_coarse, rays.reshape(-1, 8), z)
    G = torch.randn(out.shape, generator=g).cuda()
    (out * G).sum().backward()
    # oracle: same points, fork lookup, camera scaled per axis (uv_x * sx, uv_y * sy)
    cam = orc.encode_cameras(torch.from_numpy(fx["poses"]), *gu.intrinsics(spec), W, H)
    s2 = torch.tensor([sx, sy])
    cam_s = (cam[0], cam[1] * s2, cam[2] * s2)
    zc = z.detach().cpu().double().requires_grad_(True)
    r = rays.reshape(-1, 8).cpu().double()
    xyz = (r[:, None, :3] + zc[..., None] * r[:, None, 3:6]).reshape(1, -1, 3)
    vd = r[:, None, 3:6].expand(-1, K, -1).reshape(1, -1, 3)
    sd = {k: torch.from_numpy(v).double() for k, v in gu.make_mlp_state(spec, "coarse").items()}
    o = orc.point_forward(sd, tuple(t.double() for t in cam_s), [torch.from_numpy(x).double() for x in gu.make_latents(spec)],
                          xyz, vd, spec["NS"])
    (o.reshape(-1, K, 4) * G.cpu().double()).sum().backward()
    assert maxdiff(out.detach().cpu(), o.detach().reshape(-1, K, 4)) <= 1e-4
    scale = float(zc.grad.abs().max())
    assert maxdiff(z.grad.cpu(), zc.grad) <= 5e-4 * scale


def test_reference_profiler_labels_and_fp16_saturation():
    """the reference's record_function labels exist as ranges around the same entry points
    (renderer_forward nerf.py:264, model_inference models.py.backup2:165, resnetfc_infer resnetfc.py:180, positional_enc
    code.py:40).  And: the fp16 kernel saturates its activations at +-65504 inside the conversion (MODE.FP16_OVFL, no
    v_pk_min per pair since round 4) — weights scaled until the hidden activations leave the fp16 range must still give
    finite pixels where the fp32 path gives finite pixels."""
    from hip_util import setup
    fx, spec, net, rend = setup("full_ns1", precision="fp16")
    rays = torch.from_numpy(fx["rays"]).cuda()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        rend(net, rays)
        pts = torch.from_numpy(fx["pts_xyz_coarse"]).cuda()
        net(pts, coarse=True, viewdirs=torch.from_numpy(fx["pts_dirs_coarse"]).cuda())
        zx = torch.randn(8, net.mlp_coarse.d_latent + net.mlp_coarse.d_in, device="cuda")
        net.mlp_coarse(zx)
        net.code(torch.randn(5, 3, device="cuda"))
    names = {e.key for e in prof.key_averages()}
    for label in ("renderer_forward", "model_inference", "resnetfc_infer", "positional_enc"):
        assert label in names, (label, sorted(n for n in names if "::" not in n))
    # saturation: blow the first block's fc_0 up by 2^14 — relu(h) overflows fp16's range, fc_1 (scaled down by the same
    # factor, so that the fp32 network computes the same function) brings it back
    fx32, spec32, net32, rend32 = setup("full_ns1", precision="fp32")
    for n_ in (net, net32):
        with torch.no_grad():
            n_.mlp_coarse.blocks[0].fc_0.weight.mul_(16384.0)
            n_.mlp_coarse.blocks[0].fc_0.bias.mul_(16384.0)
            n_.mlp_coarse.blocks[0].fc_1.weight.mul_(1.0 / 16384.0)
    a = rend(net, rays).coarse.rgb
    b = rend32(net32, rays).coarse.rgb
    assert torch.isfinite(b).all() and torch.isfinite(a).all()
