"""Camera gradients without a GPU: the new exports and their refusals, the workspace size, the oracle against the reference's
own camera gradients, the conditions the GPU cases (tests/test_gpu_cam_grad.py) rest on, and what the comparison rules reject —
the kernels' arithmetic restated in float64 (cam_grad_util.formula) with one mistake planted, handed over as "kernel output";
the same for the three-stage sum past one chunk of 1024 points (cam_grad_util.fold) under the per-view rule."""
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


# ----------------------------------------------------------------------------- more than one chunk of 1024 points
@pytest.mark.parametrize("P", cg.MULTI_P)
def test_multi_chunk_cases_meet_their_conditions(P):
    case = cg.multi_case(P)
    spec = case["spec"]
    assert (spec["SB"], spec["NS"]) == (3, 2) and case["xyz"].shape == (3, P, 3)
    assert np.shape(gu.intrinsics(spec)[0]) == (3, 2) and np.shape(gu.intrinsics(spec)[1]) == (3, 2)        # a row per object
    frac, clamped, behind = cg.class_counts(case)
    keep = cg.relu_keep(case)
    first = (P - 1) // cg.CHUNK * cg.CHUNK
    tail = keep[:, first:]
    print(f"\nP {P}: interior {frac:.2f}, clamped pairs {clamped}, behind {behind}, masked {(~keep).mean():.4f}, "
          f"tail points kept {tail.sum(1).tolist()} of {P - first}")
    assert frac >= cg.MIN_INTERIOR and clamped > 0 and behind > 0
    assert (~keep).mean() <= cg.MAX_MASKED
    assert {1023: (1, 1023), 1024: (1, 1024), 1025: (2, 1), 3089: (4, 17)}[P] == (-(-P // cg.CHUNK), P - first)
    if P > cg.CHUNK:
        assert tail.all()                                     # every tail point of every object carries a cotangent
    cot = cg.tail_cotangent(case, cg.TAIL_OBJ[P])
    nz = np.abs(cot).sum(-1) > 0
    assert nz[cg.TAIL_OBJ[P], first:].sum() == tail[cg.TAIL_OBJ[P]].sum() and nz.sum() == nz[cg.TAIL_OBJ[P], first:].sum()


@pytest.mark.parametrize("n,K", cg.MULTI_RAYS)
def test_multi_ray_cases_meet_their_conditions(n, K):
    case = cg.multi_ray_case(n, K)
    spec = case["spec"]
    P = n * K
    assert (spec["SB"], spec["NS"]) == (2, 2) and case["rays"].shape == (2 * n, 8) and case["z"].shape == (2 * n, K)
    assert case["rays"].dtype == np.float32 and (np.diff(case["z"], axis=1) >= 0).all()
    assert P > cg.CHUNK and {(43, 24): 1032, (211, 5): 1055}[n, K] == P
    if (n, K) == (43, 24):
        assert 42 * K < cg.CHUNK < 43 * K                     # ray 42 holds points 1008 .. 1031: across the chunk boundary
    xyz, _ = cg.ray_points(case)
    frac, clamped, _ = cg.class_counts(case, xyz)
    keep = cg.relu_keep(case, True)
    assert xyz.shape == (2, P, 3) and frac >= cg.MIN_INTERIOR and clamped > 0 and (~keep).mean() <= cg.MAX_MASKED
    assert keep[cg.RAY_TAIL_OBJ, cg.CHUNK:].all()
    cot = cg.tail_cotangent(case, cg.RAY_TAIL_OBJ, True)
    nz = np.abs(cot).sum(-1) > 0
    assert nz[cg.RAY_TAIL_OBJ, cg.CHUNK:].all() and nz.sum() == P - cg.CHUNK


def test_sb1_ray_cases_are_unchanged_by_the_object_count():
    """ray_points / point_truth take the object count from the spec now: one object gives the shapes they always gave."""
    case = cg.ray_case(5)
    xyz, dirs = cg.ray_points(case)
    assert xyz.shape == dirs.shape == (1, 37 * 5, 3)


@pytest.mark.parametrize("kind,key", cg.MULTI_IDS, ids=[f"{k}-{v}" if k == "points" else f"rays-{v[0]}x{v[1]}" for k, v in cg.MULTI_IDS])
def test_fold_matches_autograd_and_every_planted_index_mistake_is_rejected(kind, key):
    """cam_grad_util.fold — k_cam_partial and k_cam_fold restated — on the restated records equals autograd to 1e-12; each
    mistake planted in its index arithmetic sits at MUTANT_FACTOR or more above compare_per_view's bound under the cotangent
    FOLD_MUTANT_COTANGENT names for it, on every case it acts on.  Under the other cotangent the figure is printed: 0 x where
    the mistake cannot show there (see FOLD_MUTANT_COTANGENT)."""
    rays_mode = kind == "rays"
    lines, seen = [], {}
    for cname in ("full", "tail"):
        case, cot, truth, ref32 = cg.multi_truth(kind, key, cname)
        spec = case["spec"]
        SB, NS = spec["SB"], spec["NS"]
        ppo = cot.shape[1]
        rec = cg.records(case, cot, rays_mode)
        assert rec.shape == (NS * SB * ppo, 16)
        good = cg.cam_from_sums(case, cg.fold(rec, SB, NS, ppo))
        for k in cg.VIEW_KEYS:
            assert good[k].shape == truth[k].shape
            assert np.abs(good[k] - truth[k]).max() <= 1e-12 * np.abs(truth[k]).max(), (cname, k)
        assert cg.compare_per_view(good, truth, ref32, f"{kind} {key} {cname}, restated fold")["ratio"] <= 1e-6
        if cname == "tail":                                   # the other objects' rows: exact zeros in the truth itself
            obj = cg.RAY_TAIL_OBJ if rays_mode else cg.TAIL_OBJ[key]
            others = [o for o in range(SB) if o != obj]
            assert not truth["poses"].reshape(SB, -1)[others].any() and not truth["focal"][others].any()
            assert all(np.linalg.norm(truth["poses"].reshape(SB, NS, 12)[obj, v]) > 10 for v in range(NS))
        for mutant in cg.FOLD_MUTANTS:
            if not cg.fold_mutant_acts(mutant, SB, NS, ppo):
                continue
            got = cg.cam_from_sums(case, cg.fold(rec, SB, NS, ppo, mutant=mutant))
            r = cg.compare_per_view(got, truth, ref32, f"{cname}, {mutant}", check=False)["ratio"]
            seen.setdefault(mutant, {})[cname] = r
            if cg.FOLD_MUTANT_COTANGENT[mutant] == cname:
                assert r >= cg.MUTANT_FACTOR, (kind, key, cname, mutant, r)
    for mutant, r in seen.items():
        lines.append(f"{mutant}: full {r['full']:.0f} x, tail {r['tail']:.0f} x")
    print(f"\n{kind} {key}: " + "; ".join(lines))
    assert len(seen) >= (4 if key in (1023, 1024) else 8)


def test_every_planted_index_mistake_acts_on_some_case():
    sizes = [(3, 2, P) for P in cg.MULTI_P] + [(2, 2, n * K) for n, K in cg.MULTI_RAYS]
    for mutant in cg.FOLD_MUTANTS:
        assert sum(cg.fold_mutant_acts(mutant, *s) for s in sizes) >= 4, mutant
        assert cg.FOLD_MUTANT_COTANGENT[mutant] in ("full", "tail")


def test_per_view_rule_rejects_what_the_whole_tensor_rule_lets_through():
    """One view of six 1e-3 off is 4e-4 of the whole tensor: cg.compare passes it, compare_per_view names the view; a piece
    that is not zero where the truth is fails whatever its size."""
    rng = np.random.default_rng(5)
    truth = dict(poses=rng.standard_normal((6, 3, 4)), focal=rng.standard_normal((3, 2)), c=rng.standard_normal((3, 2)))
    got = {k: v.copy() for k, v in truth.items()}
    got["poses"][4] *= 1.0 + 1e-3
    assert tu.rel_l2(got, truth)["poses"] < cg.RTOL
    cg.compare(got, truth, truth, "one view 1e-3 off")
    with pytest.raises(AssertionError, match=r"poses\[4\]"):
        cg.compare_per_view(got, truth, truth, "one view 1e-3 off")
    worst = cg.compare_per_view(got, truth, truth, "one view 1e-3 off", check=False)
    assert worst["piece"] == "poses[4]" and abs(worst["ratio"] - 2.0) < 1e-6
    truth["focal"][1] = 0.0
    got = {k: v.copy() for k, v in truth.items()}
    assert cg.compare_per_view(got, truth, truth, "zero row")["ratio"] == 0.0
    got["focal"][1, 0] = 1e-30
    with pytest.raises(AssertionError, match="exactly zero"):
        cg.compare_per_view(got, truth, truth, "zero row")


def test_camera_workspace_terms():
    """DESIGN §4.14's terms on top of the backward's own workspace, each rounded up to 256 bytes behind 256 bytes of alignment
    slack: 24 B per point, 64 B per (point, view), 128 B per (object, view, chunk of 1024 points) — the only term that
    grows with the chunk count."""
    from pixel_nerf_multiscale_amd import _native as N
    r256 = lambda x: (x + 255) // 256 * 256
    for SB, NS in ((1, 1), (2, 2), (3, 2)):
        prm, m, v, _ = _structs(SB, NS)
        for ppo in (3, 1023, 1024, 1025, 1032, 3089, 8193):
            n = SB * ppo
            base = N.lib.pnr_train_bwd_workspace_bytes(C.byref(m), C.byref(v), n)
            pt, rec, part = r256(24 * n), r256(64 * NS * n), r256(128 * SB * NS * (-(-ppo // cg.CHUNK)))
            for a, b in ((1, 0), (0, 1), (1, 1)):
                got = N.lib.pnr_train_bwd_cam_workspace_bytes(C.byref(m), C.byref(v), n, a, b)
                assert got == r256(base) + 256 + a * pt + b * (rec + part), (SB, NS, ppo, a, b, got, base)
