"""Per-view source intrinsics through the kernels — fx != fy, off-centre c, one row per object (which the host repeats per
view) or per view, n_focal = 1 with n_c = SB*NS — against something independent on geometry where they matter.

Every other comparison of this suite with the reference fixtures, the fp32 oracle or float64 runs on a scalar focal and the
image centre shared by all views; load_cam(vw, view) with n_focal > 1 / n_c > 1 (k_features_f32, k_point_mfma with its
scalar-cache and per-lane branches, k_features_bwd, k_latent_grad_lds) was compared with itself only.  The cases here put the
image over a map of its own size, so the texel a point reads depends on f and c (tests/test_intrinsics_cpu.py: interior
fraction >= 0.6, and every mistake with the intrinsics moves the float64 truth by >= 12 x what the rules below accept).
Rules and bounds are the existing ones, unchanged: the reference fixtures at 1e-4, fused_fp64_util.class_compare,
point_f32_util.f32_compare, train_fp64_util.l2_compare and compare_grads at 5e-4, bit identity of the fused launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_fp64_util as fu
import golden_util as gu
import hip_util as hu
import point_f32_util as pu
import train_fp64_util as tu
from oracle_util import maxdiff, oracle_render
from test_gpu_parity import _staged_render
from test_gpu_train import hip_grads
from test_gpu_train_fp64 import RTOL, _pt_fp64, _pt_run, _route
from test_oracle_grad import compare_grads, oracle_grads

pytestmark = pytest.mark.gpu
PRECS = ["fp16", "bf16"]
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _views_rows(net, prec, SB, NS, n_focal, n_c):
    """The struct the kernels get carries the row counts the case is about."""
    v, _ = net.views_struct(prec)
    assert (v.n_objs, v.n_views, v.n_focal, v.n_c) == (SB, NS, n_focal, n_c), (v.n_objs, v.n_views, v.n_focal, v.n_c)


# ----------------------------------------------------------------------------- fp32 render: reference fixture and oracle
@pytest.mark.parametrize("name", sorted(gu.INTRINSICS_CASES))
def test_render_fp32_matches_reference_and_oracle(name):
    """rend(net, rays) at precision fp32 on per-object (fx, fy) and c against the reference's own outputs and against
    orc.render, at test_render_fp32_matches_reference's bounds; the stage kernels on the oracle's intermediates at
    test_stage_kernels_match_oracle's."""
    fx, spec, net, rend = hu.setup(name, precision="fp32")
    SB, NS = spec["SB"], spec["NS"]
    _views_rows(net, "fp32", SB, NS, SB * NS, SB * NS)
    rays = _dev(fx["rays"])
    out = rend(net, rays, want_weights=True)
    res = oracle_render(fx)
    span = max(spec["z_far"] - spec["z_near"], 1.0)
    for lvl in ("coarse", "fine"):
        for what, ref in (("reference", lambda k: fx[f"{lvl}_{k}"]), ("oracle", lambda k: res[lvl][k])):
            d = [maxdiff(out[lvl][k].cpu(), np.asarray(ref(k)).reshape(tuple(out[lvl][k].shape))) for k in ("rgb", "weights", "depth")]
            print(f"\n{name} {lvl} vs {what}: rgb {d[0]:.2e} weights {d[1]:.2e} depth {d[2]:.2e}")
            assert d[0] <= 1e-4 and d[1] <= 1e-4 and d[2] <= 1e-4 * span * 4, (lvl, what, d)
    r = rays.reshape(-1, 8)
    z = rend.sample_coarse(r)
    assert maxdiff(z.cpu(), res["coarse"]["z"]) <= 2e-6 * max(1.0, spec["z_far"])
    zc = res["coarse"]["z"].cuda()
    w, rgb, depth = rend._composite_native(r, zc.contiguous(), res["coarse"]["pts_out"].cuda().contiguous())
    assert maxdiff(w.cpu(), res["coarse"]["weights"].reshape(w.shape)) <= 2e-6
    assert maxdiff(rgb.cpu(), res["coarse"]["rgb"].reshape(rgb.shape)) <= 5e-6
    assert maxdiff(depth.cpu(), res["coarse"]["depth"].reshape(-1)) <= 2e-5
    rend.last_seed = 0
    zf = rend.sample_fine_sorted(r, zc, res["coarse"]["weights"].reshape(w.shape).cuda(), res["coarse"]["depth"].reshape(-1).cuda())
    assert maxdiff(zf.cpu(), res["fine"]["z"]) <= 5e-6 * max(1.0, spec["z_far"])


# ----------------------------------------------------------------------------- fp32 point path per point
def _f32_points(net, case, P):
    out = net(_dev(case["xyz"][:, :P]), coarse=True, viewdirs=_dev(case["dirs"][:, :P]))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(pu.INTR))
def test_fp32_path_matches_fp64_with_per_view_intrinsics(name):
    """k_features_f32 with view > 0 under per-object rows, SB*NS distinct rows, and a scalar focal with SB*NS rows of c: the
    first 2047 points per object (4094 in the call: NCHW reads) and all 2065 (4130: the channels-last copies), each under
    point_f32_util.f32_compare with the case's ensemble."""
    case = pu.make_case(name)
    spec = case["spec"]
    SB, NS = spec["SB"], spec["NS"]
    assert SB * pu.P_INTR_BELOW < pu.CL_POINTS <= SB * pu.P_INTR_ABOVE and case["xyz"].shape[1] == pu.P_INTR_ABOVE
    truth, errs = pu.ensemble(name)
    net = hu.build_net(spec, case["poses"], "cuda", "fp32")
    assert net.resolved_precision() == "fp32"
    _views_rows(net, "fp32", SB, NS, 1 if spec.get("focal_xy") is None else SB * NS, SB * NS)
    for P in (pu.P_INTR_BELOW, pu.P_INTR_ABOVE):
        got = _f32_points(net, case, P)
        assert got.shape == (SB, P, 4)
        t, e = truth[:, :P], {k: v[:, :P] for k, v in errs.items()}
        cls = pu.f32_classes(case, P)
        frac = fu.interior_fraction(spec, case["poses"], case["xyz"][:, :P])
        r = pu.f32_compare(got, t, e, cls, what=f"{name} P {P}", check=False)
        print("\n" + fu.ratio_line(f"{name} P {SB} x {P}", frac, r))
        pu.f32_compare(got, t, e, cls, what=f"{name} P {P}")


# ----------------------------------------------------------------------------- fused 16-bit kernel per point
def _truth_emu(name, case, prec):
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    geometry = repr(sorted(fu.INTR_FUSED_CASES[name]["make"].items(), key=str)) if name in fu.INTR_FUSED_CASES else name
    return (_memo(("truth", geometry), lambda: fu.truth_fp64(*a)), _memo(("emu", geometry, prec), lambda: fu.emulate_16bit(*a, prec)))


def _fused_net(case, prec, proj, stream):
    spec = case["spec"]
    net = hu.build_net(spec, case["poses"], "cuda", prec)
    net.project_latent = proj
    assert net.resolved_precision() == prec
    v, _ = net.views_struct(prec)
    m, _ = net.mlp_struct(net.mlp_coarse, prec, v)
    projected = m.packed_texels > 0
    assert projected == (stream == "proj"), (stream, m.packed_texels)
    nv = spec["SB"] * spec["NS"]
    assert (v.n_focal, v.n_c) == (nv, nv), (v.n_focal, v.n_c)
    return net, projected and spec["SB"] > 1


def _hold(what, case, got, truth, emu, per_obj):
    cls = fu.point_classes(case["spec"], case["poses"], case["xyz"], per_obj)
    frac = fu.interior_fraction(case["spec"], case["poses"], case["xyz"])
    r = fu.class_compare(got, truth, emu, cls, what=what, check=False)
    print("\n" + fu.ratio_line(what, frac, r))
    fu.class_compare(got, truth, emu, cls, what=what)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(fu.INTR_FUSED_CASES))
def test_fused_kernel_matches_fp64_with_per_view_intrinsics(name, prec):
    """fused_fp64_util.INTR_FUSED_CASES under class_compare against emulate_16bit: one object of one view with an anisotropic
    focal and an off-centre c on both streams (n_objs == 1: load_cam's scalar-cache branch), three views with a row each
    (mean and max), three objects of two views with a row per object and P off a tile multiple on both streams (per-object
    projected streams; view_of where a tile straddles two objects)."""
    cfg = fu.INTR_FUSED_CASES[name]
    case = fu.intr_case(name)
    net, per_obj = _fused_net(case, prec, cfg["proj"], cfg["stream"])
    out = net(_dev(case["xyz"]), coarse=True, viewdirs=_dev(case["dirs"]))
    torch.cuda.synchronize()
    truth, emu = _truth_emu(name, case, prec)
    _hold(f"{name} {prec}", case, out.cpu().numpy(), truth, emu, per_obj)


@pytest.mark.parametrize("prec", PRECS)
def test_fused_kernel_matches_fp64_in_rays_mode_with_per_view_intrinsics(prec):
    """pnr_point_mlp with (rays, z, K = 37) on one object of two views, a row per view."""
    from pixel_nerf_multiscale_amd import _native as N
    case = fu.intr_case("rays_sb1_ns2")
    n_rays, K = case["z"].shape
    net, _ = _fused_net(case, prec, True, "proj")
    prm = net.params_struct(None, prec)
    v, keep_v = net.views_struct(prec)
    m, keep_m = net.mlp_struct(net.mlp_coarse, prec, v)
    r, z = _dev(case["rays"]), _dev(case["z"])
    out = torch.empty(n_rays * K, 4, device="cuda")
    ws = net.workspace(N.lib.pnr_workspace_bytes(C.byref(prm), C.byref(m), C.byref(v), n_rays), r.device)
    N.check(N.lib.pnr_point_mlp(C.byref(prm), C.byref(m), C.byref(v), N.ptr(r), N.ptr(z), K, None, None, n_rays * K, n_rays * K,
                                N.ptr(out), ws.data_ptr(), ws.numel(), N.current_stream(r.device)), "pnr_point_mlp")
    torch.cuda.synchronize()
    truth, emu = _truth_emu("rays_sb1_ns2", case, prec)
    _hold(f"rays_sb1_ns2 {prec}", case, out.cpu().numpy(), truth, emu, False)


# ----------------------------------------------------------------------------- fused render launch
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_fused_render_launch_is_bit_identical_with_per_object_intrinsics(prec):
    """full_sb2_ns2_intr: pnr_render's one launch per pass against the staged launches, bit for bit."""
    fx, spec, net, rend = hu.setup("full_sb2_ns2_intr", precision=prec)
    assert net.resolved_precision() == prec
    rend.keep_samples = True
    rays = _dev(fx["rays"])
    n = spec["SB"] * spec["N"]
    fused = rend(net, rays, want_weights=True)
    staged = _staged_render(net, rend, rays)
    assert sorted(staged) == ["coarse", "fine"]
    for lvl, (w, rgb, depth, z) in staged.items():
        assert torch.equal(fused[lvl].z.reshape(n, -1), z), (lvl, "z")
        assert torch.equal(fused[lvl].weights.reshape(n, -1), w), (lvl, "weights")
        assert torch.equal(fused[lvl].rgb.reshape(n, 3), rgb), (lvl, "rgb")
        assert torch.equal(fused[lvl].depth.reshape(n), depth), (lvl, "depth")


# ----------------------------------------------------------------------------- training backward
def test_point_backward_matches_fp64_with_per_object_intrinsics():
    """k_features_bwd (d(xyz) uses fx and fy separately) and k_latent_grad_lds on two objects of two views with a row per
    object: d(xyz) and the latent map against float64 on every entry (full_compare at 5e-4), they and every MLP tensor under
    l2_compare at 5e-4 with the fp32 restatement, the forward within 1e-4 as in test_gpu_train_fp64.py."""
    case = fu.interior_case(**fu.INTR_TRAIN)
    spec, poses, maps, xyz, dirs = case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"]
    SB, P = xyz.shape[:2]
    cot = np.random.default_rng(582).standard_normal((SB, P, 4)).astype(np.float32)
    out, got, net = _pt_run(spec, poses, maps, xyz, dirs, cot)
    _views_rows(net, "fp32", SB, spec["NS"], SB * spec["NS"], SB * spec["NS"])
    assert _route(net, SB * P) == 1                                     # the LDS route: k_latent_grad_lds
    o64, truth = _pt_fp64(spec, poses, maps, xyz, dirs, cot)
    ref32 = _pt_fp64(spec, poses, maps, xyz, dirs, cot, dtype=torch.float32)[1]
    assert set(truth) == set(got) and "xyz" in truth and "latent.0" in truth
    assert np.abs(out - o64).max() <= 1e-4 * max(1.0, np.abs(o64).max())
    entry = tu.entry_ratios(got, truth)
    print("\ntrain_sb2_ns2_per_object: max/scale " + ", ".join(f"{g} {v:.1e}" for g, v in tu.group_worst(entry).items())
          + "; fp32 restatement " + ", ".join(f"{g} {v:.1e}" for g, v in tu.group_worst(tu.entry_ratios(ref32, truth)).items()))
    direct = ("xyz", "latent.0")          # written by the kernels that read the intrinsics: every entry (the lattice test's rule)
    tu.full_compare({k: got[k] for k in direct}, {k: truth[k] for k in direct}, RTOL, "train_sb2_ns2_per_object")
    l2 = tu.l2_compare(got, truth, RTOL, "train_sb2_ns2_per_object", ref32=ref32)
    print("train_sb2_ns2_per_object: l2 " + ", ".join(f"{g} {v:.1e}" for g, v in tu.group_worst(l2).items()))


def test_training_step_matches_reference_gradients_with_per_object_intrinsics():
    """One whole training step of full_sb2_ns2_intr against the reference's own gradients (compare_grads at 5e-4, float64 the
    arbiter where the two fp32 results differ), as test_gradients_match_reference holds the other fixtures."""
    name = "full_sb2_ns2_intr"
    gfx = gu.load_grad_fixture(name)
    fx, out, loss, grads = hip_grads(name)
    assert np.abs(out.coarse.rgb.detach().cpu().numpy() - fx["coarse_rgb"]).max() <= 1e-4
    assert abs(loss - float(gfx["loss"])) <= 1e-3 * max(1.0, abs(float(gfx["loss"])))
    compare_grads(grads, gfx, RTOL, name, truth=lambda: oracle_grads(fx, torch.float64)[1])
