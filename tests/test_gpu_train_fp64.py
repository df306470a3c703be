"""The training backward (csrc/train_f32.hip) against the oracle in float64, every entry of every gradient: whole training steps
at the training schedule (Kc 64, Kf 32, Kfd 16, d_hidden 512), and the stage kernels at their edges — an exact-geometry lookup
lattice (texel lines, borders), the latent-gradient routes and block boundaries, view-max ties, fixed-point magnitude and
non-finite cotangents, compositing and depth-sample extremes.  Truth and rules: tests/train_fp64_util.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu
import hip_util as hu
import train_fp64_util as tu
from oracle import pixelnerf_oracle as orc

pytestmark = pytest.mark.gpu
RTOL = 5e-4             # the suite's training tolerance (test_gpu_train.py)

SCHED = tu.TRAIN_SCHEDULE
STEP_CASES = {
    "srn": gu._case(seed=101, lat=[(256, 8, 8)], image=(128, 128), focal=131.25, NS=1, SB=2, N=96, **SCHED),
    "two_view": gu._case(seed=102, lat=[(256, 16, 16)], image=(128, 128), focal=131.25, NS=2, SB=2, N=64, **SCHED),
    "dtu": gu._case(seed=103, lat=[(256, 19, 25)], image=(400, 300), focal=360.0, NS=3, SB=1, N=96, lindisp=True,
                    white_bkgd=False, z_near=0.1, z_far=5.0, radius=2.0, **SCHED),
    "multiscale": gu._case(seed=104, lat=[(64, 16, 16), (64, 16, 16), (128, 8, 8), (256, 4, 4)], image=(32, 32), focal=33.0,
                           NS=2, SB=1, N=96, use_code_viewdirs=True, depth_std=1.0, z_near=0.8, z_far=1.8, radius=1.3, **SCHED),
    "max3": gu._case(seed=105, lat=[(256, 8, 8)], image=(128, 128), focal=131.25, NS=3, SB=1, N=96, combine_type="max",
                     z_near=1.2, z_far=4.0, radius=2.7, **SCHED),
}
STEP_ROUTE = {"srn": 1, "two_view": 2, "dtu": 2, "multiscale": 2, "max3": 1}


def _route(net, n_points):
    from pixel_nerf_multiscale_amd import _native as N
    v, _ = net.views_struct("fp32")
    return int(N.lib.pnr_debug_latent_grad_route(C.byref(v), n_points))


def _grads_of(net, maps):
    g = {}
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        if mlp is not None:
            for k, p in mlp.named_parameters():
                if p.grad is not None:
                    g[f"{which}.{k}"] = p.grad.cpu().numpy()
    for i, m in enumerate(maps):
        g[f"latent.{i}"] = m.grad.cpu().numpy()
    return g


def _step(spec, precision="fp32", coarse_only=False, seed=7):
    """One training step of the HIP path and of the fp64 oracle on the same inputs; returns (got, truth, info)."""
    rays_np, poses_np = gu.make_inputs(spec)
    maps_np = gu.make_latents(spec)
    noise = tu.make_noise(spec, seed)
    cot = gu.make_loss_weights(spec)
    if coarse_only:
        cot = {k: v for k, v in cot.items() if k.startswith("coarse")}
    net = hu.build_net(spec, poses_np).train()
    net.train_precision = precision
    maps = [torch.from_numpy(m).cuda().requires_grad_(True) for m in maps_np]
    net.encoder.set_latents(maps)
    rend = hu.build_renderer(spec)
    rend.fixed_noise = {k: v.cuda() for k, v in noise.items()}
    rend.keep_samples = True
    rays = torch.from_numpy(rays_np).cuda()
    out = rend(net, rays, want_weights=True)
    route = _route(net, spec["SB"] * spec["N"] * spec["Kc"])
    assert route == STEP_ROUTE[[k for k, v in STEP_CASES.items() if v is spec][0]]
    if coarse_only:         # the coarse pass alone in fp64 (the fine pass carries no cotangent)
        spec64 = dict(spec, Kf=0, Kfd=0)
        t = tu.fp64_step(spec64, {"noise_c": noise["noise_c"]}, poses_np, maps_np, cot, None, rays_np)
    else:
        zf = out.fine.z.cpu().numpy()
        dc = out.coarse.depth.detach().cpu().numpy()
        t = tu.fp64_step(spec, noise, poses_np, maps_np, cot,
                         lambda o64: tu.step_ray_mask(spec, rays_np, noise, o64, zf, dc), rays_np)
    keep = t["keep"]
    ref32 = None if coarse_only else tu.fp64_step(spec, noise, poses_np, maps_np, cot, keep, rays_np, dtype=torch.float32)["grads"]
    c = {k: torch.from_numpy(v).cuda() for k, v in tu.masked_cotangents(cot, keep).items()}
    tu.step_loss(out, c).backward()
    got = _grads_of(net, maps)
    truth = t["grads"]
    if coarse_only:
        truth = {k: v for k, v in truth.items() if not k.startswith("fine")}
    return got, truth, dict(out=out, out64=t["out"], keep=keep, route=route, ref32=ref32)


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_training_step_matches_fp64(name):
    """The default fp32 training step at the training schedule against fp64, after the ray mask (at most 5 % of the rays).
    Outputs: rgb within 1e-4, weights within 4e-4.  Gradients: every latent map and every MLP tensor under l2_compare at 5e-4,
    or 4x the fp32 restatement's own distance where a ReLU-dominated tensor puts that higher (train_fp64_util.l2_compare
    says why every entry cannot be held to 5e-4 in fp32).  Prints the route, the masked rays and the worst ratios."""
    spec = STEP_CASES[name]
    got, truth, info = _step(spec)
    keep = info["keep"]
    masked = int((~keep).sum())
    assert masked <= tu.MASK_MAX_FRACTION * keep.size, masked
    out, o64 = info["out"], info["out64"]
    for tag in ("coarse", "fine"):
        sel = np.ones_like(keep) if tag == "coarse" else keep
        rgb = out[tag].rgb.detach().cpu().numpy()[sel]
        w = out[tag].weights.detach().cpu().numpy()[sel]
        assert np.abs(rgb - o64[tag]["rgb"].detach().numpy()[sel]).max() <= 1e-4, tag
        assert np.abs(w - o64[tag]["weights"].detach().numpy()[sel]).max() <= 4e-4, tag
    ref32 = info["ref32"]
    l2 = tu.group_worst(tu.l2_compare(got, truth, RTOL, name, ref32=ref32))
    l2_ref = tu.group_worst(tu.rel_l2(ref32, truth))
    entry = tu.group_worst(tu.entry_ratios(got, truth))
    entry_ref = tu.group_worst(tu.entry_ratios(ref32, truth))
    print(f"\n{name}: route {info['route']}, masked rays {masked} / {keep.size}; " + "; ".join(
        f"{g} l2 {l2[g]:.1e} (fp32 restatement {l2_ref[g]:.1e}) max/scale {entry[g]:.1e} ({entry_ref[g]:.1e})" for g in l2))


@pytest.mark.parametrize("name", ["srn", "dtu"])
def test_bf16x3_training_step_vs_fp64(name):
    """train_precision='bf16x3' with coarse-pass cotangents (as test_bf16x3_gradients, for its reason): every gradient tensor
    within 1e-2 in relative l2 of the float64 truth."""
    got, truth, info = _step(STEP_CASES[name], precision="bf16x3", coarse_only=True)
    for k, t in truth.items():
        a, b = np.asarray(got[k], np.float64).reshape(-1), t.reshape(-1)
        nb = float(np.linalg.norm(b))
        if nb == 0:
            continue
        rel = float(np.linalg.norm(a - b)) / nb
        assert rel <= 1e-2, (k, rel)


# ----------------------------------------------------------------------------- explicit points (PointMLP)
_pt_spec = tu.point_spec


def _pt_run(spec, poses, maps_np, xyz, dirs, cot, uv_scale=None, sd=None):
    """HIP explicit-point forward + backward: (out (SB,P,4), grads dict incl. 'xyz', net)."""
    net = hu.build_net(spec, poses).train()
    if sd is not None:
        net.mlp_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    if uv_scale:
        net.encoder.uv_scale = "image"
    maps = [torch.from_numpy(m).cuda().requires_grad_(True) for m in maps_np]
    net.encoder.set_latents(maps)
    xh = torch.from_numpy(xyz).cuda().requires_grad_(True)
    out = net(xh, coarse=True, viewdirs=torch.from_numpy(dirs).cuda())
    (out * torch.from_numpy(cot).cuda()).sum().backward()
    g = {f"coarse.{k}": p.grad.cpu().numpy() for k, p in net.mlp_coarse.named_parameters() if p.grad is not None}
    g.update({f"latent.{i}": m.grad.cpu().numpy() for i, m in enumerate(maps)})
    g["xyz"] = xh.grad.cpu().numpy()
    return out.detach().cpu().numpy(), g, net


_pt_fp64 = tu.point_grads_fp64


_random_points = tu.random_points


LATTICE_MAPS = {
    "lds_c96": ([(96, 5, 9)], None, 1),
    "fixed_c512": ([(512, 5, 9)], None, 2),
    "two_levels": ([(64, 5, 9), (64, 3, 5)], None, 2),
    "uv_image": ([(96, 5, 9)], (18, 10), 1),
}


@pytest.mark.parametrize("case", list(LATTICE_MAPS))
def test_lookup_lattice_gradients_match_fp64(case):
    """Points planned exactly on texel centres, texel lines and corners, the four borders and corners, half a texel and far
    outside, and behind the camera (tests/train_fp64_util.lattice_points; the landing is checked on the CPU by
    test_train_fp64_cpu.py).  d(xyz), every map and every parameter against fp64 with ATen's border rule."""
    lat, image, route = LATTICE_MAPS[case]
    image = image or tu.LATTICE_IMAGE
    spec = _pt_spec(lat, image=image, focal=tu.LATTICE_FOCAL, n_blocks=2, combine_layer=1)
    W, H = lat[0][2], lat[0][1]
    scale = (W / image[0], H / image[1]) if case == "uv_image" else (1.0, 1.0)
    xyz, plan = tu.lattice_points(W, H, image=image, scale=scale)
    P = xyz.shape[0]
    xyz = xyz[None]
    dirs = np.tile(np.array([[0.0, 0.6, -0.8]], np.float32), (1, P, 1))
    poses = tu.lattice_c2w()[None, None]
    maps = gu.make_latents(spec)
    cot = np.random.default_rng(3).standard_normal((1, P, 4)).astype(np.float32)
    uvs = [(m[2] / image[0], m[1] / image[1]) for m in lat] if case == "uv_image" else None
    out, got, net = _pt_run(spec, poses, maps, xyz, dirs, cot, uv_scale=uvs is not None)
    assert _route(net, P) == route
    o64, truth = _pt_fp64(spec, poses, maps, xyz, dirs, cot, uv_scale=uvs)
    assert np.abs(out - o64).max() <= 1e-4 * max(1.0, np.abs(o64).max())
    r = tu.full_compare(got, truth, RTOL, case)
    print(f"\nlattice {case}: route {route}, worst " + ", ".join(f"{g} {v:.2e}" for g, v in tu.group_worst(r).items()))


@pytest.mark.parametrize("lat,route,NS", [((256, 8, 8), 1, 1), ((256, 8, 8), 1, 4), ((256, 8, 9), 2, 1)])
def test_route_and_block_boundaries_match_fp64(lat, route, NS):
    """Maps at the LDS / fixed-point switch (exactly 64 KiB; one column more), SB 3, and points per object around the
    256-point LDS block and off the (P+3)/4 grid of k_features_bwd.  One view: the latent maps (what the routes compute) every
    entry within 5e-4.  Every case: all gradients under l2_compare with the fp32 restatement.  With four views a ReLU input
    within rounding of 0 moves single entries of the MLP tensors, d(xyz) and, through d(zx), the maps by up to ~2e-3 of scale;
    the fp32 restatement shows the same (at 256 points per object the same entries to two digits);
    test_several_views_match_fp64_at_every_entry takes those points out and holds every entry, four views on the fixed-point
    map included."""
    for P in (1, 255, 256, 257, 1001):
        spec = _pt_spec([lat], NS=NS, SB=3, image=(128, 128), focal=131.25, seed=211 + P)
        _, poses = gu.make_inputs(dict(spec, N=1))
        xyz, dirs = _random_points(spec, P, P)
        maps = gu.make_latents(spec)
        cot = np.random.default_rng(P).standard_normal((3, P, 4)).astype(np.float32)
        out, got, net = _pt_run(spec, poses, maps, xyz, dirs, cot)
        assert _route(net, 3 * P) == route
        o64, truth = _pt_fp64(spec, poses, maps, xyz, dirs, cot)
        ref32 = _pt_fp64(spec, poses, maps, xyz, dirs, cot, dtype=torch.float32)[1]
        assert np.abs(out - o64).max() <= 1e-4 * max(1.0, np.abs(o64).max())
        what = f"{lat} NS {NS} P {P}"
        lat_keys = [k for k in truth if k.startswith("latent")]
        if NS == 1:
            tu.full_compare({k: got[k] for k in lat_keys}, {k: truth[k] for k in lat_keys}, RTOL, what)
        l2 = tu.l2_compare(got, truth, RTOL, what, ref32=ref32)
        r = tu.entry_ratios(got, {k: truth[k] for k in lat_keys})
        entry = tu.entry_ratios(got, {k: v for k, v in truth.items() if k not in lat_keys})
        print(f"\n{what}: route {route}, latent max/scale {max(r.values()):.1e}, l2 "
              + ", ".join(f"{g} {v:.1e}" for g, v in tu.group_worst(l2).items())
              + ", max/scale " + ", ".join(f"{g} {v:.1e}" for g, v in tu.group_worst(entry).items()))


@pytest.mark.parametrize("name", list(tu.MARGIN_CASES))
def test_several_views_match_fp64_at_every_entry(name):
    """Two to four views on both latent-gradient routes, the four-level map with and without uv_scale = "image": EVERY
    gradient (maps, MLP tensors, d(xyz)) at every entry within 5e-4 of fp64, at 1 … 1001 points per object.  What made that
    impossible before (test_route_and_block_boundaries_match_fp64) is taken out of the comparison, not averaged: the points
    with a ReLU input, or a view maximum, within rounding of its decision get no cotangent on either side
    (train_fp64_util.relu_margin_mask, from the oracle in fp64 and fp32 alone; at most 5 % of the points).  Prints the route,
    the masked points and per group the worst error / scale beside the fp32 restatement's."""
    for P in tu.MARGIN_POINTS:
        c = tu.margin_case(name, P)
        spec, uvs = c["spec"], c["uvs"]
        args = (spec, c["poses"], c["maps"], c["xyz"], c["dirs"])
        info = {}
        keep = tu.relu_margin_mask(*args, uv_scale=uvs, info=info)
        masked = int((~keep).sum())
        assert masked <= tu.MASK_MAX_FRACTION * keep.size, (name, P, masked)
        cot = tu.mask_points(c["cot"], keep)
        out, got, net = _pt_run(*args, cot, uv_scale=uvs is not None)
        route = _route(net, spec["SB"] * P)
        assert route == c["route"]
        o64, truth = _pt_fp64(*args, cot, uv_scale=uvs)
        ref32 = _pt_fp64(*args, cot, uv_scale=uvs, dtype=torch.float32)[1]
        ours, ref = tu.group_worst(tu.entry_ratios(got, truth)), tu.group_worst(tu.entry_ratios(ref32, truth))
        print(f"\n{name} P {P}: route {route}, masked {masked} / {keep.size} (argmax rule {info['argmax']}), max/scale "
              + ", ".join(f"{g} {v:.1e} ({ref[g]:.1e})" for g, v in ours.items()))
        assert np.abs(out - o64).max() <= 1e-4 * max(1.0, np.abs(o64).max())
        tu.full_compare(got, truth, RTOL, f"{name} P {P}")


@pytest.mark.parametrize("P", [257, 1001])
def test_both_latent_routes_sum_the_same_contributions(P):
    """The map (256, 8, 8), four views, SB 3, takes the LDS route; cut along its channels into two levels of (128, 8, 8) it
    takes the fixed-point route (n_levels == 2) with the same points, weights and cotangents.  The interpolated latent vector
    is the same list of numbers, so outputs, MLP gradients and d(xyz) are bit-identical: both runs made the same ReLU
    decisions and fed the same d(zx) to their route, and no rounding event can enter.  The maps may then differ by the order
    of summation alone: per entry |LDS - fixed point| <= n 2^-24 sum|g w| + n 2^-s, n the contributions to the entry and
    sum|g w| their absolute scatter from the fp64 d(zx), s of k_latq_scale.  (Measured: worst |d| / bound 0.975 and 0.999, at
    entries of two contributions whose two sums lie one ulp apart: the bound has no slack there.)"""
    c = tu.margin_case("lds_ns4", P)
    spec, maps = c["spec"], c["maps"]
    spec2 = dict(spec, lat=[(128, 8, 8), (128, 8, 8)])
    maps2 = [np.ascontiguousarray(maps[0][:, :128]), np.ascontiguousarray(maps[0][:, 128:])]
    sd = gu.make_mlp_state(spec, "coarse")
    out1, g1, net1 = _pt_run(spec, c["poses"], maps, c["xyz"], c["dirs"], c["cot"], sd=sd)
    assert _route(net1, 3 * P) == 1
    out2, g2, net2 = _pt_run(spec2, c["poses"], maps2, c["xyz"], c["dirs"], c["cot"], sd=sd)
    assert _route(net2, 3 * P) == 2
    same = {"out": (out1, out2)}
    same.update({k: (g1[k], g2[k]) for k in g1 if not k.startswith("latent")})
    differs = {k: float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(a).max(), 1e-30))
               for k, (a, b) in same.items() if not np.array_equal(a, b)}
    _, _, dzx = _pt_fp64(spec, c["poses"], maps, c["xyz"], c["dirs"], c["cot"], sd=sd, stages=True)
    with torch.no_grad():
        uv = tu.point_forward_oracle(spec, c["poses"], maps, c["xyz"], c["dirs"], sd=sd)[1]["uv"].numpy()
    tot, cnt = tu.latent_scatter(dzx, uv, spec["lat"])[0]
    L = gu.d_latent_of(spec)
    frac, _ = np.frexp(float(np.abs(dzx[:, :L]).max()))
    # (a maximum within 1e-3 of a power of two may sit on its other side in fp32: then the smaller scale)
    s = tu.latq_scale_bits(float(np.abs(dzx[:, :L]).max()), 4 * spec["NS"] * 3 * P) - (1 if frac < 0.5005 or frac > 0.9995 else 0)
    bound = cnt * 2.0 ** -24 * tot + cnt * 2.0 ** -s
    diff = np.abs(g1["latent.0"].astype(np.float64) - np.concatenate([g2["latent.0"], g2["latent.1"]], axis=1))
    live = bound > 0
    ratio = np.where(live, diff / np.where(live, bound, 1.0), 0.0)
    worst, at = float(ratio.max()), np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"\nroute equivalence P {P}: s = {s}, not bit-identical {differs or 'none'}, maps max |d| {diff.max():.3e} "
          f"(scale {np.abs(g1['latent.0']).max():.3e}), worst |d| / bound {worst:.3e} (an entry of "
          f"{int(cnt[at[0], 0, at[2], at[3]])} contributions), entries no point reaches {int((~live).sum())}")
    assert not differs, f"not bit-identical between the routes' runs (max |d| / max): {differs}"
    assert (diff <= bound).all(), worst


@pytest.mark.parametrize("NS,combine", [(3, "max"), (4, "average")])
def test_tied_views_match_fp64(NS, combine):
    """Views 0 and 2 share pose and map: bitwise-equal per-view streams.  max sends a tie to the first view, as torch.max(dim)
    does, so view 2 gets no gradient at all."""
    spec = _pt_spec([(256, 8, 8)], NS=NS, SB=1, d_hidden=128, combine_type=combine, image=(128, 128), focal=131.25)
    _, poses = gu.make_inputs(dict(spec, N=1))
    poses[:, 2] = poses[:, 0]
    maps = gu.make_latents(spec)
    maps[0][2] = maps[0][0]
    xyz, dirs = _random_points(spec, 300, 9)
    cot = np.random.default_rng(9).standard_normal((1, 300, 4)).astype(np.float32)
    out, got, net = _pt_run(spec, poses, maps, xyz, dirs, cot)
    o64, truth = _pt_fp64(spec, poses, maps, xyz, dirs, cot)
    tu.full_compare(got, truth, RTOL, f"ties {combine}")
    if combine == "max":
        assert np.abs(got["latent.0"][0]).max() > 0
        assert not np.any(got["latent.0"][2]), "view 2 tied with view 0 took gradient"
        assert not np.any(truth["latent.0"][2])


def _fixed_point_case(P=400, seed=221):
    spec = _pt_spec([(256, 8, 9)], NS=2, SB=2, image=(128, 128), focal=131.25, seed=seed)
    _, poses = gu.make_inputs(dict(spec, N=1))
    xyz, dirs = _random_points(spec, P, seed)
    return spec, poses, gu.make_latents(spec), xyz, dirs


def test_fixed_point_resolution_and_exact_scaling():
    """One point's cotangent 2^20 times the rest's: the map entries only the small points reach keep their value to fp32
    accuracy plus the resolution k_latq_scale's formula implies (n_terms 2^-s).  Losses scaled by 2^40 and 2^-60 give exactly
    scaled maps (the scale follows the gradient's magnitude), on both routes.  An inf cotangent gives a NaN map."""
    spec, poses, maps, xyz, dirs = _fixed_point_case()
    SB, P = xyz.shape[:2]
    rng = np.random.default_rng(1)
    cot_small = rng.standard_normal((SB, P, 4)).astype(np.float32)
    cot_big = np.zeros_like(cot_small)
    cot_big[0, 17] = cot_small[0, 17] * 2.0 ** 20
    cot_small[0, 17] = 0.0
    cot = cot_small + cot_big
    _, got, net = _pt_run(spec, poses, maps, xyz, dirs, cot)
    assert _route(net, SB * P) == 2
    _, t_small, dzx_small = _pt_fp64(spec, poses, maps, xyz, dirs, cot_small, stages=True)
    _, t_big, dzx_big = _pt_fp64(spec, poses, maps, xyz, dirs, cot_big, stages=True)
    L = gu.d_latent_of(spec)
    n_terms = 4 * spec["NS"] * SB * P
    # (one bit of slack: the fp32 maximum may sit on the other side of a power of two than the fp64 one)
    s = tu.latq_scale_bits(float(np.abs(dzx_small[:, :L] + dzx_big[:, :L]).max()), n_terms) - 1
    truth = t_small["latent.0"] + t_big["latent.0"]
    tu.full_compare({"latent.0": got["latent.0"]}, {"latent.0": truth}, RTOL, "big point")
    only_small = t_big["latent.0"] == 0
    ts = t_small["latent.0"][only_small]
    bound = RTOL * max(float(np.abs(ts).max()), float(np.linalg.norm(ts)) / np.sqrt(ts.size)) + n_terms * 2.0 ** -s
    err = float(np.abs(got["latent.0"][only_small] - ts).max())
    print(f"\nfixed point: s = {s}, small-only entries err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    # exact scaling, both routes
    for lat, lat_route in (((256, 8, 9), 2), ((256, 8, 8), 1)):
        sp = dict(spec, lat=[lat])
        mp = gu.make_latents(sp)
        _, g0, net0 = _pt_run(sp, poses, mp, xyz, dirs, cot_small)
        assert _route(net0, SB * P) == lat_route
        base = g0["latent.0"]
        for k in (40, -60):
            g = _pt_run(sp, poses, mp, xyz, dirs, (cot_small * np.float32(2.0 ** k)).astype(np.float32))[1]["latent.0"]
            assert np.array_equal(g * 2.0 ** -k, base), (lat, k)
    bad = cot_small.copy()
    bad[1, 5, 1] = np.inf                       # an rgb channel: the sigmoid passes it on
    g = _pt_run(spec, poses, maps, xyz, dirs, bad)[1]["latent.0"]
    assert np.isnan(g).all()                    # k_latq_finalize: the whole map says so


def test_latent_column_gradient_up_to_flt_max_stays_finite():
    """A finite latent-column gradient in (3.4e38, FLT_MAX] sets the fixed-point scale like any other: the map is finite and
    equal to fp64 (k_abs_max_cols once read it as non-finite and turned the whole map into NaN).  One point per object, one
    view; lin_z scaled up 2^20 and the maps down 2^20 (the forward is unchanged, d(zx) becomes the largest backward
    intermediate); the cotangent scale taken from the fp64 d(zx)."""
    spec = _pt_spec([(512, 5, 9)], NS=1, SB=2, d_hidden=64, image=(128, 128), focal=131.25, seed=231)
    _, poses = gu.make_inputs(dict(spec, N=1))
    xyz, dirs = _random_points(spec, 1, 231)
    sd = gu.make_mlp_state(spec, "coarse")
    for b in range(spec["combine_layer"]):
        sd[f"lin_z.{b}.weight"] = (sd[f"lin_z.{b}.weight"] * np.float32(2.0 ** 20)).astype(np.float32)
    maps = [(m * np.float32(2.0 ** -20)).astype(np.float32) for m in gu.make_latents(spec)]
    cot = np.zeros((2, 1, 4), np.float32)
    cot[:, :, 0] = 1.0                          # red only: the sigmoid passes every cotangent on
    o64, _, dzx = _pt_fp64(spec, poses, maps, xyz, dirs, cot, sd=sd, stages=True)
    L = gu.d_latent_of(spec)
    target = 3.4014e38
    cot[:, :, 0] = np.float32(target / float(np.abs(dzx[:, :L]).max()))
    o64, truth, dzx = _pt_fp64(spec, poses, maps, xyz, dirs, cot, sd=sd, stages=True)
    m = float(np.abs(dzx[:, :L]).max())
    assert 3.4e38 * (1 + 2e-5) < m < 3.4028234e38 * (1 - 2e-5), m
    _, got, net = _pt_run(spec, poses, maps, xyz, dirs, cot, sd=sd)
    assert _route(net, 2) == 2
    assert np.isfinite(got["latent.0"]).all(), "a finite latent-column gradient turned the map into NaN"
    tu.full_compare({"latent.0": got["latent.0"]}, {"latent.0": truth["latent.0"]}, RTOL, "FLT_MAX")


# ----------------------------------------------------------------------------- per-ray stages
def _composite_case(K, kind, white, seed):
    g = torch.Generator().manual_seed(seed)
    B = 48
    near, far = 1.25, 2.75
    z, _ = torch.sort(torch.rand(B, K, generator=g) * (far - near) + near, dim=-1)
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), near), torch.full((B, 1), far)], -1)
    sig = torch.relu(torch.randn(B, K, generator=g) * 8 + 2)
    if kind == "repeat":
        z[:, 1::3] = z[:, 0::3][:, :z[:, 1::3].shape[1]]
        z[:, -1] = far
        z, _ = torch.sort(z, dim=-1)
    elif kind == "opaque":
        sig[:, K // 3: K // 3 + 4] = 1e9          # sigma delta >= 104 unless delta < 1e-7: 1 - alpha = 0 in fp32, T at the floor
    elif kind == "sign":
        sig[:, 0::3] = 0.0
        sig[:, 1::3] = -torch.rand(B, len(range(1, K, 3)), generator=g) * 5
    out = torch.cat([torch.rand(B, K, 3, generator=g), sig[..., None]], -1)
    cot = [torch.randn(B, K, generator=g), torch.randn(B, 3, generator=g), torch.randn(B, generator=g)]
    return rays, z, out, cot


@pytest.mark.parametrize("K", [1, 63, 64, 65, 112, 129])
@pytest.mark.parametrize("kind", ["plain", "repeat", "opaque", "sign"])
def test_composite_backward_edges_vs_fp64(K, kind):
    from pixel_nerf_multiscale_amd.render.autograd import Composite
    for white in (True, False):
        rays, z, out, cot = _composite_case(K, kind, white, K * 7 + len(kind))
        for present in ((True, True, True), (False, True, False), (True, False, True)):
            zo = z.to(tu.F64).requires_grad_(True)
            oo = out.to(tu.F64).requires_grad_(True)
            res = orc.composite(rays.to(tu.F64), zo, oo, white)
            sum(((r * c.to(tu.F64)).sum() for r, c, p in zip(res, cot, present) if p)).backward()
            zh, oh = z.cuda().requires_grad_(True), out.cuda().requires_grad_(True)
            res2 = Composite.apply(rays.cuda(), zh, oh, white)
            sum(((r * c.cuda()).sum() for r, c, p in zip(res2, cot, present) if p)).backward()
            for r, r64, what in zip(res2, res, ("weights", "rgb", "depth")):
                assert float((r.detach().cpu().double() - r64.detach()).abs().max()) <= 1e-5, (K, kind, white, what)
            for a, b, what in ((oh.grad, oo.grad, "d_out"), (zh.grad, zo.grad, "d_z")):
                a, b = a.cpu().double(), b.detach()
                # per ray: the scale of the ray's own gradient (an opaque run makes d_z of one ray 1e10 times another's)
                scale = torch.maximum(b.abs().flatten(1).max(1).values, b.flatten(1).norm(dim=1) / b[0].numel() ** 0.5)
                err = (a - b).abs().flatten(1).max(1).values
                assert bool((err <= 2e-4 * scale + 1e-6).all()), (K, kind, white, present, what, float((err / (scale + 1e-30)).max()))


@pytest.mark.parametrize("Kfd,Kf", [(1, 1), (16, 32), (64, 80), (65, 65), (100, 116)])
@pytest.mark.parametrize("std", [0.3, 0.0])
def test_depth_sample_backward_vs_fp64(Kfd, Kf, std):
    """SampleFine's d(depth): the sum over unclamped depth samples of d(z_sorted) at their slots, against fp64 sort autograd.
    Depths outside [near, far] on both sides (clamped samples give zero); std 0 makes every depth sample of a ray tie."""
    from pixel_nerf_multiscale_amd import NeRFRenderer
    from pixel_nerf_multiscale_amd.render.autograd import SampleFine
    Kc, B = 64, 40
    g = torch.Generator().manual_seed(Kfd * 31 + Kf)
    near, far = 1.25, 2.75
    rays = torch.cat([torch.randn(B, 6, generator=g), torch.full((B, 1), near), torch.full((B, 1), far)], -1)
    zc, _ = torch.sort(torch.rand(B, Kc, generator=g) * (far - near) + near, dim=-1)
    w = torch.rand(B, Kc, generator=g)
    depth = torch.rand(B, generator=g) * (far - near) + near
    depth[0], depth[1] = near - 0.5, far + 0.5
    noise = {"u": torch.rand(B, Kf - Kfd, generator=g), "r": torch.rand(B, Kf - Kfd, generator=g),
             "g": torch.randn(B, Kfd, generator=g)}
    rend = NeRFRenderer(n_coarse=Kc, n_fine=Kf, n_fine_depth=Kfd, depth_std=std, white_bkgd=True, lindisp=False).cuda()
    noise = {k: v for k, v in noise.items() if v.shape[1] > 0}
    dh = depth.cuda().requires_grad_(True)
    zf = SampleFine.apply(rend, rays.cuda(), zc.cuda(), w.cuda(), dh, 0, {k: v.cuda() for k, v in noise.items()})
    dz = torch.randn(B, Kc + Kf, generator=g)
    (zf * dz.cuda()).sum().backward()
    # fp64: cat + sort of the same values, autograd through the sort
    d64 = depth.to(tu.F64).requires_grad_(True)
    r64 = rays.to(tu.F64)
    parts = [zc.to(tu.F64)]
    if Kf - Kfd > 0:
        parts.append(orc.sample_fine(r64, w.to(tu.F64), Kc, False, noise["u"].to(tu.F64), noise["r"].to(tu.F64)))
    zd = orc.sample_fine_depth(r64, d64, std, noise["g"].to(tu.F64))
    z64, idx = torch.sort(torch.cat(parts + [zd], -1), dim=-1)
    same = (zf.detach().cpu().double() - z64.detach()).abs().max(-1).values <= 1e-5      # else an importance sample changed bin
    assert int((~same).sum()) <= 1
    (z64 * dz.to(tu.F64)).sum().backward()
    # |terms|: d(z_sorted) at the slots of the unclamped depth samples
    slot = torch.argsort(idx, dim=-1)[:, -Kfd:]
    raw = depth.to(tu.F64)[:, None] + noise["g"].to(tu.F64) * std
    live = (raw > near) & (raw < far)
    terms = (torch.gather(dz.to(tu.F64), 1, slot).abs() * live).sum(-1)
    got = dh.grad.cpu().double()
    assert tu.depth_grad_ok(got[same], d64.grad[same], terms[same]), float(((got - d64.grad).abs() - 1e-6 * terms).max())
    if std == 0:            # clamped on both sides: no gradient
        assert float(dh.grad[0]) == 0 and float(dh.grad[1]) == 0 and float(d64.grad[0]) == 0 and float(d64.grad[1]) == 0
