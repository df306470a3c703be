"""Camera gradients without a GPU: the new exports and their refusals, the workspace size, the oracle against the reference's
own camera gradients, the conditions the GPU cases (tests/test_gpu_cam_grad.py) rest on, and what the comparison rules reject —
the kernels' arithmetic restated in float64 (cam_grad_util.formula) with one mistake planted, handed over as "kernel output"."""
import ctypes as C

import numpy as np
import pytest
import torch

import cam_grad_util as cg
import golden_util as gu
import train_fp64_util as tu
from test_oracle_grad import compare_grads

_memo = {}


# ----------------------------------------------------------------------------- the C ABI
def test_new_exports_and_argtypes():
    from pixel_nerf_multiscale_amd import _native as N
    res, args = N.PROTOTYPES["pnr_point_mlp_bwd_cam"]
    old = N.PROTOTYPES["pnr_point_mlp_bwd"][1]
    assert res is C.c_int32 and args[:18] == old[:18] and args[18:21] == [C.c_void_p] * 3 and args[21:] == old[18:]
    assert N.PROTOTYPES["pnr_train_bwd_cam_workspace_bytes"] == (
        C.c_uint64, N.PROTOTYPES["pnr_train_bwd_workspace_bytes"][1] + [C.c_int32, C.c_int32])
    assert N.lib._cdll.pnr_point_mlp_bwd_cam.argtypes == args
    assert N.lib.pnr_version() == 102


def _structs(SB=1, NS=1):
    """Descriptors that pass the argument checks, over addresses nothing dereferences before the checks are through."""
    from pixel_nerf_multiscale_amd import _native as N
    fake = 0x10000
    prm, m, v = N.pnr_params(), N.pnr_mlp(), N.pnr_views()
    prm.num_freqs, prm.freq_factor, prm.precision = 6, 1.5, 0
    m.d_in, m.d_latent, m.d_hidden, m.d_out, m.n_blocks, m.combine_layer = 42, 8, 64, 4, 5, 3
    for f in ("lin_in_w", "lin_in_b", "lin_out_w", "lin_out_b"):
        setattr(m, f, fake)
    for b in range(5):
        for f in ("fc0_w", "fc0_b", "fc1_w", "fc1_b", "lin_z_w", "lin_z_b"):
            getattr(m, f)[b] = fake
    v.n_objs, v.n_views, v.n_focal, v.n_c, v.n_levels = SB, NS, 1, 1, 1
    v.w2c = v.focal = v.c = fake
    v.latent[0], v.lat_c[0], v.lat_h[0], v.lat_w[0] = fake, 8, 4, 4
    return prm, m, v, fake


def test_mode_mismatch_and_cpu_tensors_are_refused():
    from pixel_nerf_multiscale_amd import _native as N
    prm, m, v, p = _structs()
    g = N.pnr_mlp_grads()
    head = (C.byref(prm), C.byref(m), C.byref(v))
    tail = (p, p, p, 1 << 20, C.byref(g), None)
    explicit, rays = (None, None, 0, p, p, 8, 8), (p, p, 2, None, None, 8, 8)
    # d_rays with explicit points, d_dirs with rays: PNR_E_SHAPE, before any launch
    assert N.lib.pnr_point_mlp_bwd_cam(*head, *explicit, *tail, None, None, None, p, None, p, 1 << 30, None) == -2
    assert N.lib.pnr_point_mlp_bwd_cam(*head, *rays, *tail, None, None, p, None, None, p, 1 << 30, None) == -2
    assert N.lib.pnr_point_mlp_bwd_cam(*head, *rays, *tail, p, None, None, None, None, p, 1 << 30, None) == -2     # d_xyz with rays, as today
    assert N.lib.pnr_point_mlp_bwd_cam(*head, *explicit, *tail, None, None, None, None, p + 4, p, 1 << 30, None) == -5   # d_cam alignment
    assert N.lib.pnr_point_mlp_bwd_cam(*head, *explicit, *tail, None, None, None, None, None, None, 0, None) == -1
    with pytest.raises(RuntimeError):
        N.ptr(torch.zeros(4, 16))                     # the autograd layer hands every output through N.ptr: CPU tensors stop there


def test_workspace_size_is_monotone_and_zero_extra_without_camera_outputs():
    from pixel_nerf_multiscale_amd import _native as N
    for SB, NS in ((1, 1), (2, 3)):
        prm, m, v, _ = _structs(SB, NS)
        size = lambda n, a, b: N.lib.pnr_train_bwd_cam_workspace_bytes(C.byref(m), C.byref(v), n, a, b)
        last = None
        for n in (SB, 6 * SB, 1001 * SB, 1024 * SB, 1025 * SB, 40000 * SB):
            base = N.lib.pnr_train_bwd_workspace_bytes(C.byref(m), C.byref(v), n)
            s = [size(n, a, b) for a, b in ((0, 0), (1, 0), (0, 1), (1, 1))]
            assert s[0] == base and base < s[1] < s[3] and base < s[2] < s[3], (n, base, s)
            assert s[3] - base >= n * 24 + NS * n * 64                          # the per-point and per-(point, view) records
            assert last is None or all(x >= y for x, y in zip(s, last)), (n, s, last)
            last = s
    assert N.lib.pnr_train_bwd_cam_workspace_bytes(None, None, 4, 1, 1) == 0


# ----------------------------------------------------------------------------- the reference's own camera gradients
@pytest.mark.parametrize("name", cg.CAMGRAD_FIXTURES)
def test_oracle_matches_reference_camera_gradients(name):
    """At test_oracle_grad.py's tolerance (2e-4; the loss 1e-4), near / far included."""
    fx, gfx = gu.load_fixture(name), cg.load_camgrad_fixture(name)
    assert set(k for k in gfx if not k.endswith("__norm")) >= {"loss", "rays_od", "rays_nf", "poses", "focal"}
    assert ("c" in gfx) == (name == "tiny_sb2_ns2_intr") and all(v.dtype != object for v in gfx.values())
    compare_grads(cg.oracle_cam_grads(fx), gfx, 2e-4, name)
    assert float(gfx["rays_nf__norm"]) > 0        # the reference's near / far gradient is not zero: the documented deviation


# ----------------------------------------------------------------------------- the conditions the GPU cases rest on
@pytest.mark.parametrize("name", list(cg.POINT_CASES))
def test_point_cases_are_interior_with_clamped_and_behind_pairs(name):
    case = cg.point_case(name)
    frac, clamped, behind = cg.class_counts(case)
    masked = float((~cg.relu_keep(case)).mean())
    print(f"\n{name}: interior {frac:.2f}, clamped pairs {clamped}, behind {behind}, points masked for a ReLU margin {masked:.4f}")
    assert frac >= cg.MIN_INTERIOR and clamped > 0 and behind > 0
    assert masked <= cg.MAX_MASKED
    SB, P = case["xyz"].shape[:2]
    assert P % 4 == 1 and (SB == 1 or (P % 4 != 0 and P == 1001))       # a tail wave; a block that holds points of both objects


@pytest.mark.parametrize("K", list(cg.RAY_CASES))
def test_ray_cases(K):
    case = cg.ray_case(K)
    n = case["rays"].shape[0]
    assert n == 37 and case["z"].shape == (n, K) and (np.diff(case["z"], axis=1) >= 0).all()
    if K == 24:
        assert (np.diff(case["z"], axis=1) == 0).sum() >= 8 * n         # repeated depths
    xyz, _ = cg.ray_points(case)
    frac, clamped, behind = cg.class_counts(case, xyz)
    assert frac >= cg.MIN_INTERIOR and float((~cg.relu_keep(case, True)).mean()) <= cg.MAX_MASKED


def test_step_case_stays_within_the_mask_cap_in_the_fp32_restatement():
    spec = cg.STEP_SPEC
    assert (spec["Kc"], spec["Kf"], spec["Kfd"], spec["N"], spec["SB"], spec["NS"]) == (16, 8, 4, 64, 2, 2)
    rays, poses = gu.make_inputs(spec)
    maps, noise, cot = gu.make_latents(spec), tu.make_noise(spec, cg.STEP_NOISE_SEED), gu.make_loss_weights(spec)
    o32 = cg.step_truth(spec, rays, poses, maps, noise, cot, np.ones((2, 64), bool), dtype=torch.float32)["out"]
    zf, dc = o32["fine"]["z"].detach().numpy(), o32["coarse"]["depth"].detach().numpy()
    t = cg.step_truth(spec, rays, poses, maps, noise, cot, lambda o64: tu.step_ray_mask(spec, rays, noise, o64, zf, dc))
    assert (~t["keep"]).sum() <= tu.MASK_MAX_FRACTION * t["keep"].size
    ref32 = cg.step_truth(spec, rays, poses, maps, noise, cot, t["keep"], dtype=torch.float32)["grads"]
    cg.compare(ref32, t["grads"], ref32, "fp32 restatement of the step")
    assert np.abs(t["grads"]["rays"][:, 6:]).max() > 0                  # the oracle's near / far gradient: what the kernels leave out


def test_pose_case_loop_converges_in_float64():
    """The restated refinement loop ends at <= 0.5 x its first loss, so that the device's `last < first` has room."""
    losses = cg.pose_loop_fp64(cg.pose_case())
    print("\nfloat64 refinement losses: " + " ".join(f"{v:.5f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] <= 0.5 * losses[0]


def test_se3_exp_and_rays_at():
    from pixel_nerf_multiscale_amd import pose
    xi = torch.tensor([[0.3, -0.2, 0.5, 1.0, 2.0, -1.0], [0.0, 0.0, 0.0, 0.5, 0.0, 0.0], [1e-6, 0.0, 0.0, 0.0, 1.0, 0.0]], dtype=torch.float64)
    T = pose.se3_exp(xi)
    tw = torch.zeros(3, 4, 4, dtype=torch.float64)
    tw[:, :3, :3], tw[:, :3, 3] = pose._hat(xi[:, :3]), xi[:, 3:]
    assert float((T - torch.linalg.matrix_exp(tw)).abs().max()) <= 1e-12
    g = torch.autograd.functional.jacobian(lambda x: pose.se3_exp(x)[:3].reshape(-1), torch.zeros(6, dtype=torch.float64))
    assert bool(torch.isfinite(g).all()) and float(g.abs().sum()) == 9.0      # the six generators at the origin: 2 + 2 + 2 + 1 + 1 + 1 entries
    for cs in gu.load_rays_fixture():
        W, H = cs["W"], cs["H"]
        for i in range(cs["poses"].shape[0]):
            got = pose.rays_at(torch.from_numpy(cs["poses"][i]), torch.arange(W * H), W, H, torch.from_numpy(cs["focal"]), cs["z_near"],
                               cs["z_far"], c=None if cs["c"] is None else torch.from_numpy(cs["c"]))
            assert float((got - torch.from_numpy(cs["rays"][i]).reshape(-1, 8)).abs().max()) <= 2e-6, (cs["name"], i)


# ----------------------------------------------------------------------------- what the rules reject
def _truth(kind, key):
    if (kind, key) not in _memo:
        rays_mode = kind == "rays"
        case = cg.ray_case(key) if rays_mode else cg.point_case(key)
        cot = cg.cotangent(case, n_points=case["z"].size if rays_mode else None, rays_mode=rays_mode)
        _memo[kind, key] = (case, cot, cg.point_truth(case, cot, rays_mode=rays_mode)[1],
                            cg.point_truth(case, cot, dtype=torch.float32, rays_mode=rays_mode)[1])
    return _memo[kind, key]


CASE_IDS = [("points", n) for n in cg.POINT_CASES] + [("rays", K) for K in cg.RAY_CASES]


@pytest.mark.parametrize("kind,key", CASE_IDS)
def test_restated_arithmetic_passes_and_every_planted_mistake_is_rejected(kind, key):
    case, cot, truth, ref32 = _truth(kind, key)
    rays_mode = kind == "rays"
    cg.compare(cg.formula(case, cot, rays_mode), truth, ref32, f"{kind} {key}")          # include/pnr.h's arithmetic holds
    lines = []
    for mutant in cg.MUTANTS:
        if not cg.mutant_acts(mutant, case, rays_mode):
            continue
        r = cg.compare(cg.formula(case, cot, rays_mode, mutant=mutant), truth, ref32, mutant, check=False)
        worst = max(r[k] for k in cg.mutant_keys(mutant) if k in r)
        lines.append(f"{mutant}: {worst:.0f} x")
        assert worst >= cg.MUTANT_FACTOR, (kind, key, mutant, r)
    print(f"\n{kind} {key}: " + "; ".join(lines))
    assert len(lines) >= 5
