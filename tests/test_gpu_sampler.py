"""The samplers on the device against the host model of tests/sampler_util.py (pinned on the CPU by tests/test_sampler_cpu.py):
the in-kernel Philox draws of k_sample_coarse, k_sample_fine and the fused render launch equal the model's draws, and the
resampling forward (cdf, inverse-cdf search, depth samples, bitonic merge) equals the fp64 resampling at its edges."""
import itertools

import numpy as np
import pytest
import torch

import golden_util as gu
import sampler_util as su

pytestmark = pytest.mark.gpu

SEEDS = [0, 1234, 2 ** 63 + 5, 2 ** 64 - 1]
BASES = [0, 7, 2 ** 32 - 3, 2 ** 40 + 1]         # the third straddles the 32-bit boundary inside the call
NR = 67


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _rays(n, near, far):
    r = torch.zeros(n, 8, device="cuda")
    r[:, 5], r[:, 6], r[:, 7] = 1.0, near, far
    return r


def _coarse(rays, Kc, lindisp, noise, seed, base):
    from pixel_nerf_multiscale_amd import _native as N
    z = torch.full((rays.shape[0], Kc), float("nan"), device="cuda")
    N.check(N.lib.pnr_sample_coarse(N.ptr(rays), rays.shape[0], Kc, int(lindisp), N.ptr(noise), seed, base, N.ptr(z),
                                    N.current_stream(rays.device)), "pnr_sample_coarse")
    return z


def _fine(rays, zc, w, depth, Kc, n_imp, n_dep, std, lindisp, u, r, g, seed, base):
    from pixel_nerf_multiscale_amd import _native as N
    z = torch.full((rays.shape[0], Kc + n_imp + n_dep), float("nan"), device="cuda")
    N.check(N.lib.pnr_sample_fine(N.ptr(rays), N.ptr(zc), N.ptr(w), N.ptr(depth), rays.shape[0], Kc, n_imp + n_dep, n_dep,
                                  float(std), int(lindisp), N.ptr(u), N.ptr(r), N.ptr(g), seed, base, N.ptr(z),
                                  N.current_stream(rays.device)), "pnr_sample_fine")
    return z


# ----------------------------------------------------------------------------- the in-kernel generator equals the model
@pytest.mark.parametrize("seed", SEEDS)
def test_coarse_draws_equal_the_model(seed):
    """noise_c = NULL: with Kc = 1 on [0, 1] the position IS the draw, bit for bit; for Kc around the quad (3, 4, 5), one
    wave (64) and a ragged tail (130) the in-kernel result equals the same call given the model's draws."""
    for base in BASES:
        gr = su.global_ray(base, NR)
        z = _coarse(_rays(NR, 0.0, 1.0), 1, 0, None, seed, base)
        assert np.array_equal(z.cpu().numpy(), su.draws(seed, gr, "noise_c", 1)), (seed, base)
        rays = _rays(NR, 0.8, 1.8)
        for Kc, lindisp in itertools.product((3, 4, 5, 64, 130), (0, 1)):
            a = _coarse(rays, Kc, lindisp, None, seed, base)
            b = _coarse(rays, Kc, lindisp, _dev(su.draws(seed, gr, "noise_c", Kc)), seed ^ 1, 0)
            assert torch.equal(a, b), (seed, base, Kc, lindisp)


@pytest.mark.parametrize("seed", SEEDS)
def test_importance_draws_equal_the_model(seed):
    """u = r = NULL against the model's u and r handed in: the merged rows are bit-identical; with one bin on [0, 1] the
    importance sample IS r."""
    g = torch.Generator().manual_seed(3)
    for base, (Kc, n_imp) in itertools.product(BASES, ((1, 1), (64, 3), (64, 65), (37, 130))):
        gr = su.global_ray(base, NR)
        rays = _rays(NR, 0.0, 1.0) if Kc == 1 else _rays(NR, 0.8, 1.8)
        zc = _coarse(rays, Kc, 0, None, seed, base)
        w = torch.rand(NR, Kc, generator=g).cuda()
        u, r = su.draws(seed, gr, "u", n_imp), su.draws(seed, gr, "r", n_imp)
        a = _fine(rays, zc, w, None, Kc, n_imp, 0, 0.0, 0, None, None, None, seed, base)
        b = _fine(rays, zc, w, None, Kc, n_imp, 0, 0.0, 0, _dev(u), _dev(r), None, seed ^ 1, 0)
        assert torch.equal(a, b), (seed, base, Kc, n_imp)
        if Kc == 1:
            rows, zcn = a.cpu().numpy(), zc.cpu().numpy()
            for i in range(NR):
                assert np.array_equal(su.remove_coarse(rows[i], zcn[i]), r[i]), (seed, base, i)


@pytest.mark.parametrize("seed", SEEDS)
def test_depth_draws_equal_the_model(seed):
    """g = NULL: depth 0, std 1 on (-8, 8) leaves the normals themselves.  |g_kernel - g_model| <= 8 * 2^-23 * R with
    R = sqrt(-2 ln a): logf, sqrtf and cosf within 2 ulp each (the model takes a and the fp32 product fp32(2 pi) * b as the
    kernel forms them, and everything after them in fp64).  Even the 1e-5 * R the bound must never be widened to separates a
    wrong counter, word or draw id, but not the lowest bits of b.  The worst ratio to 2^-23 * R is printed per case (-s) and
    stands in the assertion message (rounding the model's fp64 normal to fp32 alone gives 0.49)."""
    for base, Kfd in itertools.product(BASES, (1, 5, 64, 100)):
        gr = su.global_ray(base, NR)
        rays = _rays(NR, -8.0, 8.0)
        zc = torch.full((NR, 1), -8.0, device="cuda")
        depth = torch.zeros(NR, device="cuda")
        got = _fine(rays, zc, None, depth, 1, 0, Kfd, 1.0, 0, None, None, None, seed, base).cpu().numpy()
        assert (got[:, 0] == -8.0).all() and (np.diff(got, axis=1) >= 0).all()
        a, arg, R = su.normal_parts(seed, gr, Kfd)
        want = R * np.cos(arg.astype(np.float64))
        order = np.argsort(want, axis=1)
        want, R = np.take_along_axis(want, order, 1), np.take_along_axis(R, order, 1)
        err = np.abs(got[:, 1:].astype(np.float64) - want)
        assert (err[R == 0] == 0).all()
        ratio = float((err[R > 0] / (2.0 ** -23 * R[R > 0])).max()) if (R > 0).any() else 0.0
        print(f"g draws seed {seed} base {base} Kfd {Kfd}: worst |dg| / (2^-23 R) = {ratio:.3f}")
        assert ratio <= 8.0, (seed, base, Kfd, ratio)


def _model_noise(seed, gr, Kc, n_imp):
    return {"noise_c": _dev(su.draws(seed, gr, "noise_c", Kc)), "u": _dev(su.draws(seed, gr, "u", n_imp)),
            "r": _dev(su.draws(seed, gr, "r", n_imp))}


def _same(a, b, what):
    for lvl in ("coarse", "fine"):
        for k in ("z", "rgb", "depth"):
            assert torch.equal(a[lvl][k], b[lvl][k]), (what, lvl, k)


def _both(rend, run, seed, gr, what):
    """run() with everything in-kernel, then with noise_c, u, r from the model (g stays in-kernel): the same bits."""
    Kc, n_imp = int(rend.n_coarse), int(rend.n_fine) - int(rend.n_fine_depth)
    rend.keep_samples, rend.fixed_noise, rend.forced_seed = True, None, seed
    a = run()
    rend.fixed_noise = _model_noise(seed, gr, Kc, n_imp)
    b = run()
    rend.fixed_noise = None
    _same(a, b, what)
    assert not torch.isnan(a.fine.rgb).any()


@pytest.mark.parametrize("name,prec,n_rays", [("tiny_multiscale_ns2", "fp32", 16), ("full_ns1", "bf16", 131)])
def test_whole_path_draws_equal_the_model(name, prec, n_rays):
    """pnr_render (the stages in sequence in fp32, the fused launch in bf16) and pnr_render_camera with pix0 > 0: positions,
    colours and depths with the in-kernel generator are bit-identical to the same call fed the model's noise_c, u, r."""
    from hip_util import setup
    from pixel_nerf_multiscale_amd import util
    fx, spec, net, rend = setup(name, precision=prec)
    W, H = spec["image"]
    pix = torch.randperm(W * H, generator=torch.Generator().manual_seed(n_rays))[:n_rays].numpy()
    tgt = gu.pose_spherical(50.0, -20.0, spec["radius"])
    rays = torch.from_numpy(gu.pinhole_rays(tgt, W, H, spec["focal"], spec["z_near"], spec["z_far"], pix))[None].cuda()
    for seed, base in ((1234, 0), (2 ** 63 + 5, 2 ** 32 - 60), (2 ** 64 - 1, 2 ** 40 + 1)):
        rend.ray_index_base = base
        _both(rend, lambda: rend(net, rays), seed, su.global_ray(base, n_rays), (name, "render", seed, base))
        # rays of one camera, generated in the launch: pixels pix0 .. pix0 + n of a 24 x 17 image
        pix0, n = 37, 131
        cam = util.camera(tgt, 24, 17, (spec["focal"], spec["focal"] * 1.1), spec["z_near"], spec["z_far"], c=(12.0, 8.5),
                          pix0=pix0, n=n)
        _both(rend, lambda: rend._forward_fused(net, None, False, camera=cam), seed, su.global_ray(base, n),
              (name, "camera", seed, base))
    rend.ray_index_base = 0


def test_sharded_ray_key_equals_the_model():
    """A shard that holds a range of two objects' rays (ray_index_obj_stride = 2 B, base = B / 2): ray i of object o draws as
    global ray base + o * stride + i — the model applies the formula, the kernel's draws follow it bit for bit."""
    from hip_util import setup
    fx, spec, net, rend = setup("tiny_sb2_ns2")
    rays = _dev(fx["rays"])
    SB, B = rays.shape[:2]
    assert SB == 2
    rend.ray_index_obj_stride, rend.ray_index_base = 2 * B, B // 2
    gr = su.global_ray(B // 2, SB * B, B, 2 * B)
    assert gr.tolist() == [B // 2 + i for i in range(B)] + [B // 2 + 2 * B + i for i in range(B)]
    _both(rend, lambda: rend(net, rays), 1234, gr, "sharded key")
    rend.ray_index_obj_stride, rend.ray_index_base = 0, 0


# ----------------------------------------------------------------------------- resampling forward against fp64
def test_resampling_cases_are_not_vacuous():
    """The intervals [lo, hi] of the cases below, from the model alone: with random weights and random u, 0.040 % of the draws
    have lo < hi for Kc <= 300 (6.6 % for Kc >= 2048, whose bins are as narrow as 30 margins), and 91.7 % of the random-weight
    rays have lo == hi for every draw, so they are compared with the fp64 row directly."""
    draws = amb = rays = clean = 0
    for (Kc, n_imp, n_dep), (near, far), lindisp in itertools.product(su.SHAPES, su.BOUNDS, (False, True)):
        case = su.make_case(Kc, n_imp, n_dep, near, far, lindisp)
        lo, hi = su.fine_bins_fp64(case["w"], case["u_rand"], Kc)
        for i in (i for i, f in enumerate(case["fam"]) if f == "random"):
            rays += 1
            clean += int((lo[i] == hi[i]).all())
            if Kc <= 300:
                draws += n_imp
                amb += int((lo[i] < hi[i]).sum())
    assert amb <= 0.005 * draws and clean >= 0.9 * rays, (amb, draws, clean, rays)


@pytest.mark.parametrize("Kc,n_imp,n_dep", su.SHAPES)
def test_resampling_forward_against_fp64(Kc, n_imp, n_dep):
    """pnr_sample_fine with explicit draws against the fp64 resampling, per ray family (random, all zero, one bin at 0 / 63 /
    64 / Kc - 1, both ends, all 1e-9, an opaque composited profile), with u planted on 0, 1 - 2^-24 and on cdf entries and
    their fp32 neighbours (the last entry included: from there on the bin is Kc, beyond far), tags in r that name every draw,
    and a second run with random u and r.  Every coarse value once, ascending, every bin inside [lo, hi], every position
    within 8 * 2^-24 * max(|near|, |far|) (lindisp: * far^2 / near) of its bin's fp64 position, depth samples to 1 ulp.
    (2048, 1, 0) and (4000, 64, 32) take the launch with more than 64 KiB of dynamic LDS; the latter has P2 = 4096."""
    from pixel_nerf_multiscale_amd import _native as N
    top = 0
    for (near, far), lindisp in itertools.product(su.BOUNDS, (False, True)):
        case = su.make_case(Kc, n_imp, n_dep, near, far, lindisp)
        rays, zc, w, depth, g = (_dev(case[k]) for k in ("rays", "zc", "w", "depth", "g"))
        for std in (case["stds"] if n_dep else case["stds"][:1]):
            for tagged, u, r in ((True, case["u"], case["r_tag"]), (False, case["u_rand"], case["r_rand"])):
                got = _fine(rays, zc, w, depth, Kc, n_imp, n_dep, std, lindisp, _dev(u), _dev(r), g if n_dep else None, 0, 0)
                st = su.check_rows(case, got.cpu().numpy(), u, r, std, tagged)
                top += st["top_bin"]
    assert top > 0 or n_imp < 40         # the unclamped top bin was reached
    if Kc == 4000:      # one sample more than the merge network holds: refused before any launch
        z = torch.empty(1, 4097, device="cuda")
        assert N.lib.pnr_sample_fine(N.ptr(rays), N.ptr(zc), N.ptr(w), N.ptr(depth), 1, Kc, 97, 0, 0.0, 0, None, None, None, 0, 0,
                                     N.ptr(z), N.current_stream(z.device)) == -3
