"""Camera gradients on the device (csrc/cam_grad.hip through render/autograd.py) against float64 autograd through the oracle:
the view directions, the rays, and the stored source poses / focal / c; from section 8 on with more than one chunk of 1024
points per (object, view).  Cases, truth, the restated arithmetic and the rules are tests/cam_grad_util.py's; tests/test_cam_grad_cpu.py shows what the rules reject.  Every comparison prints
kernel figure / fp32-restatement figure (pytest -s): DESIGN §4.14's table."""
import ctypes as C

import numpy as np
import pytest
import torch

import cam_grad_util as cg
import golden_util as gu
import hip_util as hu
import train_fp64_util as tu

pytestmark = pytest.mark.gpu
_memo = {}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def _net(case, precision="fp32", cam_leaves=True):
    spec = case["spec"]
    net = hu.build_net(spec, case["poses"]).train()
    net.train_precision = precision
    if case.get("uv_scale"):
        net.encoder.uv_scale = "image"
    maps = [_dev(m).requires_grad_(True) for m in case["maps"]]
    net.encoder.set_latents(maps)
    if cam_leaves:                                   # the stored cameras as leaves
        net.poses, net.focal, net.c = (t.detach().clone().requires_grad_(True) for t in (net.poses, net.focal, net.c))
    return net, maps


def _collect(net, maps, extra):
    g = {f"coarse.{k}": p.grad.clone() for k, p in net.mlp_coarse.named_parameters() if p.grad is not None}
    g.update({f"latent.{i}": m.grad.clone() for i, m in enumerate(maps)})
    for k, t in extra.items():
        g[k] = None if t.grad is None else t.grad.clone()
    return g


def _run_points(case, cot, P=None, precision="fp32", want=("xyz", "dirs", "cam")):
    """HIP explicit-point forward + backward -> every gradient as a device tensor (None where not asked)."""
    net, maps = _net(case, precision, "cam" in want)
    P = case["xyz"].shape[1] if P is None else P
    xyz = _dev(case["xyz"][:, :P]).requires_grad_("xyz" in want)
    dirs = _dev(case["dirs"][:, :P]).requires_grad_("dirs" in want)
    out = net(xyz, coarse=True, viewdirs=dirs)
    (out * _dev(cot[:, :P])).sum().backward()
    return _collect(net, maps, dict(xyz=xyz, dirs=dirs, poses=net.poses, focal=net.focal, c=net.c))


def _run_rays(case, cot, want=("rays", "cam"), want_z=True, precision="fp32"):
    from pixel_nerf_multiscale_amd.render.autograd import point_mlp_rays
    net, maps = _net(case, precision, "cam" in want)
    rays = _dev(case["rays"]).requires_grad_("rays" in want)
    z = _dev(case["z"]).requires_grad_(want_z)
    out = point_mlp_rays(net, net.mlp_coarse, rays, z)
    (out * _dev(cot).reshape(out.shape)).sum().backward()
    return _collect(net, maps, dict(rays=rays, z=z, poses=net.poses, focal=net.focal, c=net.c))


def _np(g, keys):
    return {k: g[k].cpu().numpy() for k in keys}


def _truths(key, case, cot, rays_mode=False):
    if key not in _memo:
        _memo[key] = (cg.point_truth(case, cot, rays_mode=rays_mode)[1],
                      cg.point_truth(case, cot, dtype=torch.float32, rays_mode=rays_mode)[1])
    return _memo[key]


# ----------------------------------------------------------------------------- 1. explicit points
@pytest.mark.parametrize("name", list(cg.POINT_CASES))
def test_point_camera_gradients_match_fp64(name):
    """d(xyz), d(viewdirs) on every entry at 5e-4; d(poses), d(focal), d(c) under l2_compare(5e-4, fp32 restatement)."""
    case = cg.point_case(name)
    frac, clamped, behind = cg.class_counts(case)
    assert frac >= cg.MIN_INTERIOR and clamped > 0 and behind > 0, (frac, clamped, behind)
    cot = cg.cotangent(case)
    assert (~cg.relu_keep(case)).mean() <= cg.MAX_MASKED
    got = _np(_run_points(case, cot), ("xyz", "dirs", "poses", "focal", "c"))
    truth, ref32 = _truths(("p", name), case, cot)
    assert all(got[k].shape == truth[k].shape for k in got), {k: (got[k].shape, truth[k].shape) for k in got}
    print("\n" + cg.table_line(name, got, truth, ref32))
    cg.compare(got, truth, ref32, name)
    cg.compare_per_view(got, truth, ref32, name)


def test_three_points_less_than_one_block():
    case = dict(cg.point_case("ns1_raw"))
    case["xyz"], case["dirs"] = case["xyz"][:, :cg.P_SMALL], case["dirs"][:, :cg.P_SMALL]
    cot = cg.cotangent(case)
    got = _np(_run_points(case, cot), ("xyz", "dirs", "poses", "focal", "c"))
    truth, ref32 = _truths(("p3",), case, cot)
    print("\n" + cg.table_line("ns1_raw, 3 points", got, truth, ref32))
    cg.compare(got, truth, ref32, "3 points")


# ----------------------------------------------------------------------------- 2. rays mode
@pytest.mark.parametrize("K", list(cg.RAY_CASES))
def test_ray_gradients_match_fp64(K):
    """d(rays)[:, :6] on every entry and the per-view sums against float64; columns 6:8 exact zeros; d(z) the bits of today's call."""
    case = cg.ray_case(K)
    n = case["rays"].shape[0]
    cot = cg.cotangent(case, n_points=n * K, rays_mode=True)
    g = _run_rays(case, cot)
    got = _np(g, ("rays", "poses", "focal", "c"))
    assert got["rays"].shape == (n, 8) and np.array_equal(got["rays"][:, 6:], np.zeros((n, 2), np.float32))
    truth, ref32 = _truths(("r", K), case, cot, rays_mode=True)
    print("\n" + cg.table_line(f"rays K {K}", got, truth, ref32))
    cg.compare(got, truth, ref32, f"rays K {K}")
    cg.compare_per_view(got, truth, ref32, f"rays K {K}")
    today = _run_rays(case, cot, want=())
    assert today["rays"] is None and today["poses"] is None
    assert torch.equal(g["z"], today["z"])


# ----------------------------------------------------------------------------- 4. nothing else moves
def _calls(monkeypatch):
    """Record the backward entry point taken and the scratch sizes asked for."""
    from pixel_nerf_multiscale_amd import _native as N
    log = dict(entries=[], scratch=[])
    for name in ("pnr_point_mlp_bwd", "pnr_point_mlp_bwd_cam"):
        fn = getattr(N.lib, name)
        monkeypatch.setattr(N.lib, name, (lambda *a, _fn=fn, _n=name: (log["entries"].append(_n), _fn(*a))[1]))
    scratch = N.scratch
    monkeypatch.setattr(N, "scratch", lambda nbytes, dev: (log["scratch"].append(int(nbytes)), scratch(nbytes, dev))[1])
    return log


def test_other_gradients_do_not_move_and_runs_repeat(monkeypatch):
    from pixel_nerf_multiscale_amd import _native as N
    case = cg.point_case("sb2_per_object")
    cot = cg.cotangent(case)
    log = _calls(monkeypatch)
    a = _run_points(case, cot)
    assert log["entries"] == ["pnr_point_mlp_bwd_cam"]
    b = _run_points(case, cot)
    for k in ("xyz", "dirs", "poses", "focal", "c"):
        assert torch.equal(a[k], b[k]), k                                    # two runs, the same bits
    log["entries"].clear(), log["scratch"].clear()
    plain = _run_points(case, cot, want=("xyz",))
    assert log["entries"] == ["pnr_point_mlp_bwd"]                           # nothing new asked for: today's call ..
    net, _ = _net(case)
    v, _k = net.views_struct("fp32")
    m, _k2 = net.mlp_struct(net.mlp_coarse, "fp32", v)
    n_points = case["xyz"].shape[0] * case["xyz"].shape[1]
    assert log["scratch"][-1] == N.lib.pnr_train_bwd_workspace_bytes(C.byref(m), C.byref(v), n_points)   # .. today's workspace
    assert all(plain[k] is None for k in ("dirs", "poses", "focal", "c"))
    for k in plain:
        if plain[k] is not None:
            assert torch.equal(plain[k], a[k]), k                            # MLP, latent maps, d(xyz): unmoved
    only = _run_points(case, cot, want=("cam",))
    assert only["xyz"] is None and only["dirs"] is None
    for k in ("poses", "focal", "c"):
        assert torch.equal(only[k], a[k]), k


def test_only_poses_requiring_grad():
    case = cg.ray_case(5)
    cot = cg.cotangent(case, n_points=case["rays"].shape[0] * 5, rays_mode=True)
    from pixel_nerf_multiscale_amd.render.autograd import point_mlp_rays
    full = _run_rays(case, cot)
    net, maps = _net(case, cam_leaves=False)
    net.poses = net.poses.detach().clone().requires_grad_(True)
    z = _dev(case["z"]).requires_grad_(True)
    out = point_mlp_rays(net, net.mlp_coarse, _dev(case["rays"]), z)
    (out * _dev(cot).reshape(out.shape)).sum().backward()
    assert net.focal.grad is None and net.c.grad is None
    assert torch.equal(net.poses.grad, full["poses"]) and torch.equal(z.grad, full["z"])
    for k, p in net.mlp_coarse.named_parameters():
        assert torch.equal(p.grad, full[f"coarse.{k}"]), k
    assert torch.equal(maps[0].grad, full["latent.0"])


# ----------------------------------------------------------------------------- 5. the bf16 product modes
def test_bf16x3_and_bf16_camera_gradients():
    """bf16x3 against the fp32 path within 1e-2 in l2, the bound test_gpu_train.test_bf16x3_gradients holds that mode's
    gradients to; plain bf16 under test_gpu_train.test_bf16_product_mode_gradients' rule for that mode, per tensor: relative
    l2 <= 0.15 and cosine >= 0.99 against the fp32 path (the camera gradients read the dzx rows the latent gradients read).
    "P 3089": SB 3, four chunks per (object, view)."""
    keys = ("xyz", "dirs", "poses", "focal", "c")
    for name, case in (("sb2_per_view_coded", cg.point_case("sb2_per_view_coded")), ("P 3089", cg.multi_case(3089))):
        cot = cg.cotangent(case)
        g32 = _run_points(case, cot)
        for prec in ("bf16x3", "bf16"):
            g = _run_points(case, cot, precision=prec)
            a, b = {k: g[k].double().flatten() for k in keys}, {k: g32[k].double().flatten() for k in keys}
            rel = {k: float((a[k] - b[k]).norm() / b[k].norm()) for k in keys}
            cos = {k: float((a[k] @ b[k]) / (a[k].norm() * b[k].norm())) for k in keys}
            print(f"\n{name}, {prec} vs fp32, relative l2: " + ", ".join(f"{k} {v:.1e}" for k, v in rel.items())
                  + "; 1 - cosine: " + ", ".join(f"{k} {1 - v:.1e}" for k, v in cos.items()))
            assert all(bool(torch.isfinite(g[k]).all()) for k in keys)
            if prec == "bf16x3":
                assert all(v <= 1e-2 for v in rel.values()), (name, rel)
            else:
                assert all(rel[k] <= 0.15 and cos[k] >= 0.99 for k in keys), (name, rel, cos)


# ----------------------------------------------------------------------------- 3. a whole step through render_train
def test_whole_step_camera_gradients_match_fp64():
    """Coarse + fine with depth samples (16 / 8 / 4), 64 rays, SB 2, NS 2: the rays, a c2w leaf handed to set_cameras, a focal
    and a c leaf against the oracle's render in float64, under step_ray_mask (at most 5 % of the rays)."""
    spec = cg.STEP_SPEC
    rays_np, poses_np = gu.make_inputs(spec)
    maps_np = gu.make_latents(spec)
    noise = tu.make_noise(spec, cg.STEP_NOISE_SEED)
    cot = gu.make_loss_weights(spec)
    W, H = spec["image"]
    net = hu.build_net(spec, poses_np).train()
    focal_np, c_np = gu.intrinsics(spec)
    c2w = _dev(poses_np.reshape(-1, 4, 4)).requires_grad_(True)
    focal, c = _dev(focal_np).requires_grad_(True), _dev(c_np).requires_grad_(True)
    net.set_cameras(c2w, focal, c, W, H)
    rend = hu.build_renderer(spec)
    rend.fixed_noise = {k: v.cuda() for k, v in noise.items()}
    rend.keep_samples = True
    rays = _dev(rays_np).requires_grad_(True)
    out = rend(net, rays, want_weights=True)
    zf, dc = out.fine.z.cpu().numpy(), out.coarse.depth.detach().cpu().numpy()
    t = cg.step_truth(spec, rays_np, poses_np, maps_np, noise, cot, lambda o64: tu.step_ray_mask(spec, rays_np, noise, o64, zf, dc))
    keep = t["keep"]
    masked = int((~keep).sum())
    assert masked <= tu.MASK_MAX_FRACTION * keep.size, masked
    ref32 = cg.step_truth(spec, rays_np, poses_np, maps_np, noise, cot, keep, dtype=torch.float32)["grads"]
    cm = {k: torch.from_numpy(v).cuda() for k, v in tu.masked_cotangents(cot, keep).items()}
    tu.step_loss(out, cm).backward()
    got = dict(rays=rays.grad.reshape(-1, 8).cpu().numpy(), poses=c2w.grad.cpu().numpy(), focal=focal.grad.cpu().numpy(),
               c=c.grad.cpu().numpy())
    assert np.array_equal(got["rays"][:, 6:], np.zeros_like(got["rays"][:, 6:]))
    print(f"\nwhole step, masked rays {masked} / {keep.size}; " + cg.table_line("step", got, t["grads"], ref32))
    cg.compare(got, t["grads"], ref32, "whole step")


# ----------------------------------------------------------------------------- 6. the reference itself
@pytest.mark.parametrize("name", cg.CAMGRAD_FIXTURES)
def test_camera_gradients_match_reference(name):
    """The reference's own gradients at the rays, the c2w source poses, focal and c (tools/gen_golden_cam_grad.py) under
    test_gpu_train.py's rule: within 5e-4 of the reference, or of float64 where the two fp32 results differ.  Columns 6:8 of
    d(rays) are left out: the reference's are not zero."""
    from test_oracle_grad import compare_grads
    gfx = cg.load_camgrad_fixture(name)
    fx, spec, net, rend = hu.setup(name)
    net.train()
    W, H = spec["image"]
    f_np, c_np = gu.intrinsics(spec)
    c2w = _dev(fx["poses"].reshape(-1, 4, 4)).requires_grad_(True)
    focal = _dev(np.asarray(f_np, np.float32)).requires_grad_(True)           # 0-dim, or a row per object
    c = None if c_np is None else _dev(c_np).requires_grad_(True)
    net.set_cameras(c2w, focal, c, W, H)
    rays = _dev(fx["rays"]).requires_grad_(True)
    out = rend(net, rays, want_weights=True)
    G = {k: torch.from_numpy(v).cuda() for k, v in gu.make_loss_weights(spec).items()}
    loss = tu.step_loss(out, G)
    assert abs(float(loss.detach()) - float(gfx["loss"])) <= 1e-3 * max(1.0, abs(float(gfx["loss"])))
    loss.backward()
    got = dict(rays=rays.grad.cpu().numpy(), poses=c2w.grad.cpu().numpy(), focal=focal.grad.cpu().numpy())
    if c is not None:
        got["c"] = c.grad.cpu().numpy()
    got = cg.fixture_keys(got)
    assert np.array_equal(got["rays_nf"], np.zeros_like(got["rays_nf"]))
    ref = {k: v for k, v in gfx.items() if not k.startswith("rays_nf")}
    compare_grads(got, ref, cg.RTOL, name, truth=lambda: cg.oracle_cam_grads(fx, torch.float64))


# ----------------------------------------------------------------------------- 7. pose.py
def test_rays_at_matches_reference_fixture():
    """rays_at on the device against the reference's own util.gen_rays outputs, at test_gen_rays_kernel_matches_reference_fixture's
    2e-6."""
    from pixel_nerf_multiscale_amd import pose
    for cs in gu.load_rays_fixture():
        W, H = cs["W"], cs["H"]
        for i in range(cs["poses"].shape[0]):
            got = pose.rays_at(_dev(cs["poses"][i]), torch.arange(W * H, device="cuda"), W, H, _dev(cs["focal"]),
                               cs["z_near"], cs["z_far"], c=None if cs["c"] is None else _dev(cs["c"]))
            assert float((got.cpu() - torch.from_numpy(cs["rays"][i]).reshape(-1, 8)).abs().max()) <= 2e-6


def test_refine_pose_first_step_gradient_matches_fp64():
    """d(loss) / d(xi) at xi = 0 through se3_exp -> rays_at -> the renderer -> the rgb loss, with explicit draws, against the same
    chain through the oracle's render in float64; the pixels are the step's set less the rays step_ray_mask takes out."""
    from pixel_nerf_multiscale_amd import pose
    pc = cg.pose_case()
    spec, noise = pc["spec"], pc["noise"]
    net = hu.build_net(spec, pc["poses"]).train()
    rend = hu.build_renderer(spec)
    rend.fixed_noise = {k: v.cuda() for k, v in noise.items()}
    rend.keep_samples = True
    W, H = spec["image"]
    pix = pc["pix"]
    tgt, pose0 = _dev(pc["target"]), _dev(pc["pose0"])

    def hip(sel):
        xi = torch.zeros(6, device="cuda", requires_grad=True)
        rays = pose.rays_at(pose.se3_exp(xi) @ pose0, torch.from_numpy(pix[sel]).cuda(), W, H, spec["focal"], spec["z_near"], spec["z_far"])
        rend.fixed_noise = {k: v[sel].cuda() for k, v in noise.items()}
        out = rend(net, rays[None], want_weights=True)
        loss, _ = pose.rgb_loss(out, tgt.reshape(-1, 3)[torch.from_numpy(pix[sel]).cuda()][None])
        return xi, out, loss

    every = np.arange(pix.size)
    xi, out, loss = hip(every)
    o64 = cg.pose_step_fp64(pc, every)["out"]
    rays_np = pose.rays_at(torch.from_numpy(pc["pose0"]).double(), torch.from_numpy(pix), W, H, spec["focal"], spec["z_near"], spec["z_far"]).numpy()
    keep = tu.step_ray_mask(dict(spec, SB=1, N=pix.size), rays_np, noise, o64, out.fine.z.cpu().numpy(),
                            out.coarse.depth.detach().cpu().numpy()).reshape(-1)
    assert (~keep).sum() <= tu.MASK_MAX_FRACTION * keep.size, int((~keep).sum())
    sel = every[keep]
    xi, out, loss = hip(sel)
    g, = torch.autograd.grad(loss, xi)
    t64, t32 = cg.pose_step_fp64(pc, sel), cg.pose_step_fp64(pc, sel, dtype=torch.float32)
    got, truth, ref32 = dict(xi=g.cpu().numpy()), dict(xi=t64["grad"]), dict(xi=t32["grad"])
    r, rr = tu.rel_l2(got, truth)["xi"], tu.rel_l2(ref32, truth)["xi"]
    print(f"\nrefine_pose first step: loss {float(loss):.6f} vs {t64['loss']:.6f}; d(xi) l2 {r:.1e} / {rr:.1e}")
    assert abs(float(loss) - t64["loss"]) <= 1e-4 * max(1.0, abs(t64["loss"]))
    tu.l2_compare(got, truth, cg.RTOL, "d(xi)", ref32=ref32)


def test_refine_pose_ten_steps():
    from pixel_nerf_multiscale_amd import pose
    pc = cg.pose_case()
    spec = pc["spec"]
    net = hu.build_net(spec, pc["poses"])
    rend = hu.build_renderer(spec)
    args = (net, rend, _dev(pc["target"]), _dev(pc["pose0"]), spec["focal"], spec["z_near"], spec["z_far"])
    kw = dict(steps=10, rays_per_step=cg.POSE_RAYS, lr=cg.POSE_LR, seed=cg.POSE_SEED)
    p1, l1 = pose.refine_pose(*args, **kw)
    p2, l2 = pose.refine_pose(*args, **kw)
    assert l1.is_cuda and l1.shape == (10,) and p1.shape == (4, 4)
    print("\nrefine_pose losses: " + " ".join(f"{v:.5f}" for v in l1.tolist()))
    assert bool(torch.isfinite(l1).all()) and float(l1[-1]) < float(l1[0])
    assert torch.equal(l1, l2) and torch.equal(p1, p2)
    assert all(p.grad is None for p in net.parameters())


# ----------------------------------------------------------------------------- 8. more than one chunk of 1024 points per (object, view)
CAM_KEYS = ("poses", "focal", "c")


def _multi_run(kind, key, cot, **kw):
    return _run_rays(cg.multi_ray_case(*key), cot, **kw) if kind == "rays" else _run_points(cg.multi_case(key), cot, **kw)


@pytest.mark.parametrize("cot_name", ["full", "tail"])
@pytest.mark.parametrize("P", cg.MULTI_P)
def test_multi_chunk_point_camera_gradients_match_fp64(P, cot_name):
    """SB 3, NS 2, P per object one short of a chunk, a chunk, a chunk and one point, three chunks and 17: d(xyz), d(viewdirs)
    on every entry, the per-view sums per stored view and row (compare_per_view) as well as per tensor.  "tail": the cotangent
    lives on the last chunk of one object alone, and the other objects' rows are exact zeros."""
    case, cot, truth, ref32 = cg.multi_truth("points", P, cot_name)
    frac, clamped, behind = cg.class_counts(case)
    keep = cg.relu_keep(case)
    assert frac >= cg.MIN_INTERIOR and clamped > 0 and behind > 0, (frac, clamped, behind)
    assert (~keep).mean() <= cg.MAX_MASKED and (P <= cg.CHUNK or keep[:, P // cg.CHUNK * cg.CHUNK:].all())
    got = _np(_run_points(case, cot), ("xyz", "dirs") + CAM_KEYS)
    assert all(got[k].shape == truth[k].shape for k in got), {k: (got[k].shape, truth[k].shape) for k in got}
    what = f"P {P} {cot_name}"
    print("\n" + cg.table_line(what, got, truth, ref32))
    if cot_name == "tail":
        obj = cg.TAIL_OBJ[P]
        others = [o for o in range(3) if o != obj]
        assert np.linalg.norm(truth["poses"].reshape(3, -1)[obj]) > 10
        for k in CAM_KEYS:                                     # a row per object (focal, c); two views of 12 (poses)
            assert np.array_equal(got[k].reshape(3, -1)[others], np.zeros_like(got[k].reshape(3, -1)[others])), k
    cg.compare(got, truth, ref32, what)
    cg.compare_per_view(got, truth, ref32, what)


@pytest.mark.parametrize("cot_name", ["full", "tail"])
@pytest.mark.parametrize("n,K", cg.MULTI_RAYS)
def test_multi_chunk_ray_gradients_match_fp64(n, K, cot_name):
    """Rays mode with two objects of two views and more than 1024 points per object (a ray across the chunk boundary; an odd K
    with a 31-point tail).  "tail": the cotangent lives on object 1's points from 1024 on; every other ray's row is exact zeros."""
    case, cot, truth, ref32 = cg.multi_truth("rays", (n, K), cot_name)
    g = _run_rays(case, cot)
    got = _np(g, ("rays",) + CAM_KEYS)
    assert got["rays"].shape == (2 * n, 8) and np.array_equal(got["rays"][:, 6:], np.zeros((2 * n, 2), np.float32))
    what = f"rays {n} x {K} {cot_name}"
    print("\n" + cg.table_line(what, got, truth, ref32))
    if cot_name == "tail":
        touched = (np.abs(cot).sum(-1) > 0).reshape(2 * n, K).any(1)
        assert not touched[:n].any() and 0 < touched[n:].sum() == n - cg.CHUNK // K
        assert np.array_equal(got["rays"][~touched, :6], np.zeros((int((~touched).sum()), 6), np.float32))
        for k in CAM_KEYS:
            assert np.array_equal(got[k].reshape(2, -1)[0], np.zeros_like(got[k].reshape(2, -1)[0])), k
    else:
        today = _run_rays(case, cot, want=())
        assert today["rays"] is None and today["poses"] is None
        assert torch.equal(g["z"], today["z"])
    cg.compare(got, truth, ref32, what)
    cg.compare_per_view(got, truth, ref32, what)


MULTI_REPEAT = [("points", 3089), ("rays", (43, 24))]


@pytest.mark.parametrize("kind,key", MULTI_REPEAT, ids=["points-3089", "rays-43x24"])
def test_multi_chunk_runs_repeat(kind, key):
    """Four chunks (two in rays mode) folded in chunk order: two runs give the same bits in every camera output."""
    _, cot, _, _ = cg.multi_truth(kind, key, "full")
    a, b = _multi_run(kind, key, cot), _multi_run(kind, key, cot)
    for k in CAM_KEYS + (("rays", "z") if kind == "rays" else ("xyz", "dirs")):
        assert torch.equal(a[k], b[k]), k


GUARD = 4096


@pytest.mark.parametrize("kind,key", MULTI_REPEAT, ids=["points-3089", "rays-43x24"])
def test_camera_workspace_stays_inside_its_size(kind, key, monkeypatch):
    """The backward's workspace handed over as a slice of a larger buffer, 4096 bytes of 0xA5 in front and behind: the size
    asked for is pnr_train_bwd_cam_workspace_bytes with every camera output wanted, both guards keep their pattern, and
    the gradients are the bits of the same call on the ordinary scratch (the slice itself starts as 0xA5 too: nothing is
    read before it is written)."""
    from pixel_nerf_multiscale_amd import _native as N
    case, cot, _, _ = cg.multi_truth(kind, key, "full")
    plain = _multi_run(kind, key, cot)
    net, _ = _net(case)
    v, _k = net.views_struct("fp32")
    m, _k2 = net.mlp_struct(net.mlp_coarse, "fp32", v)
    n_points = cot.shape[0] * cot.shape[1]
    size_of = N.lib.pnr_train_bwd_cam_workspace_bytes
    expect = int(size_of(C.byref(m), C.byref(v), n_points, 1, 1))
    assert expect > int(N.lib.pnr_train_bwd_workspace_bytes(C.byref(m), C.byref(v), n_points))
    log = dict(pending=None, flags=[], held=[])

    def sized(*a):
        log["pending"] = int(size_of(*a))
        log["flags"].append((int(a[2]), int(a[3]), int(a[4])))
        return log["pending"]

    scratch = N.scratch

    def guarded(nbytes, dev):
        pending, log["pending"] = log["pending"], None
        if pending is None or int(nbytes) != pending:
            return scratch(nbytes, dev)
        big = torch.full((GUARD + pending + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ws = big[GUARD:GUARD + pending]
        assert ws.data_ptr() % 256 == 0
        log["held"].append((big, pending))
        return ws

    monkeypatch.setattr(N.lib, "pnr_train_bwd_cam_workspace_bytes", sized)
    monkeypatch.setattr(N, "scratch", guarded)
    got = _multi_run(kind, key, cot)
    torch.cuda.synchronize()
    assert log["flags"] == [(n_points, 1, 1)] and len(log["held"]) == 1
    big, nbytes = log["held"][0]
    assert nbytes == expect
    pattern = torch.full((GUARD,), 0xA5, dtype=torch.uint8, device=big.device)
    assert torch.equal(big[:GUARD], pattern), "bytes in front of the workspace were written"
    assert torch.equal(big[GUARD + nbytes:], pattern), "bytes behind the workspace were written"
    assert plain.keys() == got.keys()
    for k in plain:
        assert (plain[k] is None) == (got[k] is None) and (plain[k] is None or torch.equal(plain[k], got[k])), k
