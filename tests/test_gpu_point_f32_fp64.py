"""The fp32 point path (precision="fp32": point_f32, k_features_f32, chain_f32, k_combine_f32, k_out_act, and k_index_latent
behind SpatialEncoder.index), point by point against float64, on points INSIDE the latent maps.

This path is what the fp16 / bf16 PSNR floors, bench.py's meets_8c and the fused kernel's interior tests in test_gpu_parity.py
are measured against; the fixtures hold it at 256 points that clamp to one border texel of weight 1.  Here every case goes
through build_net(spec, poses, "cuda", "fp32") and net(xyz, viewdirs=dirs) and is held to tests/point_f32_util.f32_compare:
the kernels' error against the oracle in float64, per group (rgb, sigma), over all points, per tile row / 128-row GEMM tile
(of every view) / chunk / object / tap class, and per point, against the errors of an ensemble of fp32 restatements of the
same network that differ only in summation order.  Cases and rule are checked on the CPU by tests/test_point_f32_cpu.py.
Each case prints one line: case, interior fraction, the four worst ratios (kernel figure / ensemble figure, the factor not
applied: every bound is 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_fp64_util as fu
import point_f32_util as pu
import train_fp64_util as tu
from oracle import pixelnerf_oracle as orc

pytestmark = pytest.mark.gpu


def _net(case):
    from hip_util import build_net
    net = build_net(case["spec"], case["poses"], "cuda", "fp32")
    if case["uv_scale"]:
        net.encoder.uv_scale = "image"
        assert np.allclose(np.asarray(net.uv_scales()), np.asarray(case["uv_scale"]))
    assert net.resolved_precision() == "fp32"
    return net


def _points(net, case, coarse=True, P=None):
    xyz = torch.from_numpy(np.ascontiguousarray(case["xyz"][:, :P], dtype=np.float32)).cuda()
    dirs = torch.from_numpy(np.ascontiguousarray(case["dirs"][:, :P], dtype=np.float32)).cuda()
    out = net(xyz, coarse=coarse, viewdirs=dirs)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _rays(net, case):
    """pnr_point_mlp with (rays, z, K): the feature build forms o + z d itself."""
    from pixel_nerf_multiscale_amd import _native as N
    n_rays, K = case["z"].shape
    prm = net.params_struct(None, "fp32")
    v, keep_v = net.views_struct("fp32")
    m, keep_m = net.mlp_struct(net.mlp_coarse, "fp32", v)
    r = torch.from_numpy(case["rays"]).cuda().contiguous()
    z = torch.from_numpy(case["z"]).cuda().contiguous()
    out = torch.empty(n_rays * K, 4, device="cuda")
    ws = net.workspace(N.lib.pnr_workspace_bytes(C.byref(prm), C.byref(m), C.byref(v), n_rays), r.device)
    N.check(N.lib.pnr_point_mlp(C.byref(prm), C.byref(m), C.byref(v), N.ptr(r), N.ptr(z), K, None, None, n_rays * K, n_rays * K,
                                N.ptr(out), ws.data_ptr(), ws.numel(), N.current_stream(r.device)), "pnr_point_mlp")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _index(net, uv, image_size=()):
    out = net.encoder.index(uv.cuda(), image_size=image_size)
    torch.cuda.synchronize()
    return out.cpu()


def _hold(what, case, got, truth, errs, P=None, every_point=False):
    """Print the ratio line, then assert the rule."""
    cls = pu.f32_classes(case, P)
    frac = fu.interior_fraction(case["spec"], case["poses"], case["xyz"][:, :P], uv_scale=case["uv_scale"])
    r = pu.f32_compare(got, truth, errs, cls, every_point=every_point, what=what, check=False)
    print("\n" + fu.ratio_line(what, frac, r))
    pu.f32_compare(got, truth, errs, cls, every_point=every_point, what=what)


@pytest.mark.parametrize("name", list(pu.INSIDE))
def test_fp32_path_matches_fp64_inside_the_map(name):
    """point_f32_util.INSIDE at d_hidden 512, 3089 points or fewer (k_features_f32 reads the NCHW maps): one view, the fine
    MLP, three views (mean and max), coded view dirs, a 19 x 25 map, the 4-level map under both uv mappings, two levels of
    512 + 256 channels under the image mapping, the n_blocks / combine_layer corners, three objects."""
    case = pu.make_case(name)
    assert case["xyz"].shape[0] * case["xyz"].shape[1] < pu.CL_POINTS
    truth, errs = pu.ensemble(name)
    got = _points(_net(case), case, pu.coarse_of(name))
    _hold(name, case, got, truth, errs)


@pytest.mark.parametrize("name", list(pu.SWITCH))
def test_fp32_path_matches_fp64_on_both_sides_of_the_channels_last_switch(name):
    """One point set called with its first 4095 points (NCHW reads) and with all 4129 (the channels-last copies: t.off[i] * C
    + ch from the view base view * H W * C): d_hidden 512 on one 8 x 8 view, and d_hidden 64 on two views of the 4-level map
    under the image mapping (another C per level, views of two kinds).  Both calls sit under the rule, and the first 4095
    outputs of the two calls agree within the per-point bound."""
    case = pu.make_case(name)
    assert case["spec"]["SB"] == 1 and pu.P_BELOW < pu.CL_POINTS <= pu.P_ABOVE == case["xyz"].shape[1]
    truth, errs = pu.ensemble(name)
    net = _net(case)
    below, above = _points(net, case, P=pu.P_BELOW), _points(net, case)
    assert below.shape == (1, pu.P_BELOW, 4) and above.shape == (1, pu.P_ABOVE, 4)
    agree = pu.prefix_agreement(below, above, errs)
    print(f"\n{name}: first {pu.P_BELOW} outputs of the two calls, |difference| over the per-point bound: "
          + "  ".join(f"{k} {v:.3f}" for k, v in agree.items()))
    _hold(f"{name} P {pu.P_BELOW}", case, below, truth[:, :pu.P_BELOW], {k: e[:, :pu.P_BELOW] for k, e in errs.items()}, P=pu.P_BELOW)
    _hold(f"{name} P {pu.P_ABOVE}", case, above, truth, errs)
    assert all(v <= 1.0 for v in agree.values()), agree


@pytest.mark.parametrize("name", list(pu.CHUNKED))
def test_fp32_path_matches_fp64_across_the_chunk(name):
    """More than F32_CHUNK = 49152 points in one call at d_hidden 64: three objects of two views with a tail chunk of 132
    (chunk 0 mixes three objects; the tail moves view 1's rows to 132 + pl), one object of three views under max with coded
    view dirs on three levels under the image mapping and a tail of 129, and two objects of one view where object 1 is
    exactly chunk 1.  Chunk, every view's GEMM tile and the object are classes of the rule."""
    case = pu.make_case(name)
    assert case["xyz"].shape[0] * case["xyz"].shape[1] > pu.CHUNK
    truth, errs = pu.ensemble(name)
    got = _points(_net(case), case)
    _hold(name, case, got, truth, errs)


@pytest.mark.parametrize("name", list(pu.RAYS))
def test_fp32_path_matches_fp64_in_rays_mode(name):
    """pnr_point_mlp with (rays, z, K = 37) in fp32: 83 rays (3071 points, NCHW reads) and 131 rays (4847 points, the
    channels-last copies).  Truth and ensemble evaluate o + z d of the fp32 inputs, formed in float64."""
    case = pu.make_case(name)
    truth, errs = pu.ensemble(name)
    got = _rays(_net(case), case)
    _hold(name, case, got, truth, errs)


def test_fp32_path_matches_fp64_on_the_lattice():
    """Points planned exactly on texel centres, lines and corners, the borders, outside and behind the camera
    (fused_fp64_util.lattice_case).  Every point is held to the per-point bound."""
    case = pu.make_case("lattice")
    truth, errs = pu.ensemble("lattice")
    got = _points(_net(case), case)
    _hold("lattice", case, got, truth, errs, every_point=True)


# ----------------------------------------------------------------------------- SpatialEncoder.index / pnr_index_latent
INDEX_MAPS = {"one_level": [fu.LATTICE_MAP], "ms4": fu.MS4}
INDEX_VIEWS, INDEX_CLOUD = 3, 700


def _texel_f32(uv, s, size):
    """The texel coordinate as the oracle's lookup and bilinear_taps form it in float32, up to the clip."""
    g = ((uv * s) / (size - 1)) * 2 - 1
    return ((g + 1) / 2) * (size - 1)


@pytest.mark.parametrize("mapping", ["latent", "image"])
@pytest.mark.parametrize("maps", list(INDEX_MAPS))
def test_index_latent_matches_fp64_and_returns_texel_centres_exactly(maps, mapping):
    """SpatialEncoder.index on three views: the exact-geometry lattice of level 0 (another roll of it per view) followed by a
    cloud that is mostly inside the map, on one level and on the 4-level map, under both uv mappings (image = twice the
    level-0 map: every scale a power of two), uv per view and broadcast.  Against orc.index_latent in float64 the largest
    error over all points is at most 4 x that of orc.index_latent in float32 on the same points, and where a level's texel
    coordinate is exactly an in-range texel centre the output IS the map entry, bit for bit (weight 1 times the value, plus
    zeros)."""
    lat = INDEX_MAPS[maps]
    case = fu.interior_case(lat, NS=INDEX_VIEWS, P=16, seed=551)
    net = _net(case)
    _, H0, W0 = lat[0]
    image = (2 * W0, 2 * H0) if mapping == "image" else ()
    net.encoder.uv_scale = mapping
    scales = [(w / image[0], h / image[1]) if image else (1.0, 1.0) for _, h, w in lat]
    assert all(np.log2(s).is_integer() for sc in scales for s in sc)
    _, plan = tu.lattice_points(W0, H0)
    plan = plan[~np.isnan(plan[:, 0])] / np.asarray(scales[0])
    rng = np.random.default_rng(552)
    span = np.array([W0 - 1, H0 - 1]) / np.asarray(scales[0])
    cloud = rng.uniform(-0.1, 1.1, size=(INDEX_VIEWS, INDEX_CLOUD, 2)) * span
    uv = np.concatenate([np.stack([np.roll(plan, 17 * v, axis=0) for v in range(INDEX_VIEWS)]), cloud], axis=1)
    uv = torch.from_numpy(uv.astype(np.float32))
    maps32 = [torch.from_numpy(m) for m in case["maps"]]
    inside = ((cloud > 0) & (cloud < span)).all(-1).mean()
    assert inside >= 0.6, inside
    for q in (uv, uv[:1]):
        out = _index(net, q, image)
        ref64 = torch.cat([orc.index_latent(q.double() * torch.tensor(s, dtype=torch.float64), [m.double()]) for s, m in zip(scales, maps32)], dim=1)
        ref32 = torch.cat([orc.index_latent(q * torch.tensor(s, dtype=torch.float32), [m]) for s, m in zip(scales, maps32)], dim=1)
        assert tuple(out.shape) == tuple(ref64.shape) and torch.isfinite(out).all()
        err, unit = float((out.double() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
        print(f"\nindex {maps} {mapping} uv views {q.shape[0]}: max error {err:.3e}, the fp32 oracle's {unit:.3e}, ratio {err / unit:.2f}")
        assert unit > 0 and err <= pu.FACTOR * unit, (err, unit)
        # texel centres: bit for bit
        qb = q.expand(INDEX_VIEWS, -1, -1)
        c0 = 0
        for (Cl, Hl, Wl), s, m in zip(lat, scales, maps32):
            ix, iy = _texel_f32(qb[..., 0], np.float32(s[0]), Wl), _texel_f32(qb[..., 1], np.float32(s[1]), Hl)
            centre = (ix == ix.round()) & (iy == iy.round()) & (ix >= 0) & (ix <= Wl - 1) & (iy >= 0) & (iy <= Hl - 1)
            assert centre.sum() >= INDEX_VIEWS * Wl * Hl // 4, (maps, mapping, Wl, Hl, int(centre.sum()))
            vi, ni = torch.nonzero(centre, as_tuple=True)
            want = m[vi, :, iy[vi, ni].long(), ix[vi, ni].long()]                     # (hits, C)
            assert torch.equal(out[vi, c0:c0 + Cl, ni].contiguous().view(torch.int32), want.contiguous().view(torch.int32)), (maps, mapping, Wl, Hl)
            c0 += Cl
