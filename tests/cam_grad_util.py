"""Camera gradients (csrc/cam_grad.hip, pnr_point_mlp_bwd_cam): cases, float64 truth and the kernels' arithmetic restated.

Truth is torch autograd through the oracle in float64 with the cameras, the view directions or the rays as leaves.  The
restatement (formula) forms the same gradients the way include/pnr.h states the kernels do — from the gradient at the
assembled rows d(zx), the lookup's slope and the closed forms of dR, dt, dfx .. — and takes a `mutant`: one planted mistake,
handed to the comparison rules as "kernel output" by tests/test_cam_grad_cpu.py.  The three-stage sum of the per-view
outputs is restated apart from it (records, fold) with mistakes planted in its index arithmetic, for the cases with more than
one chunk of 1024 points per (object, view).  Nothing here touches a GPU."""
import numpy as np
import torch

import fused_fp64_util as fu
import golden_util as gu
import train_fp64_util as tu
from oracle import pixelnerf_oracle as orc

F64 = torch.float64
RTOL = 5e-4                  # the suite's training tolerance (tests/test_gpu_train_fp64.py)
MIN_INTERIOR = 0.6
MUTANT_FACTOR = 5.0          # a planted mistake must sit at >= 5 x the bound (tests/test_intrinsics_cpu.py)
_L8 = [(256, 8, 8)]

# explicit points: interior_case arguments.  P = 257: 64 blocks of four points and a tail wave; 1001 per object at SB 2: block 250
# holds point 1000 of object 0 and points 0..2 of object 1.  The three-point call (less than one block) is the first three
# points of "ns1_raw" (P_SMALL): three (view, point) pairs cannot meet the interior / clamped / behind condition themselves.
POINT_CASES = {
    "ns1_raw": dict(lat=_L8, NS=1, P=257, seed=701, d_hidden=64),
    "ns3_mean_coded": dict(lat=_L8, NS=3, P=257, seed=702, d_hidden=64, use_code_viewdirs=True, **fu.intr_rows(3)),
    "ns3_max_raw": dict(lat=_L8, NS=3, P=257, seed=703, d_hidden=64, combine_type="max"),
    "sb2_per_object": dict(lat=_L8, SB=2, NS=2, P=1001, seed=704, d_hidden=64, **fu.intr_rows(2)),
    "sb2_per_view_coded": dict(lat=_L8, SB=2, NS=2, P=1001, seed=705, d_hidden=64, use_code_viewdirs=True, **fu.intr_rows(4)),
    "sb2_scalar_focal": dict(lat=_L8, SB=2, NS=2, P=1001, seed=706, d_hidden=64, c_xy=fu.intr_rows(4)["c_xy"]),
    "two_level_uv_image": dict(lat=[(192, 8, 8), (64, 4, 4)], NS=2, P=257, seed=707, d_hidden=64, uv_image=True),
}
P_SMALL = 3
# rays mode: 37 rays (not a multiple of the four points a block holds once K is odd); K 24 = a sorted 16 + 8 set with repeated z
RAY_CASES = {K: dict(lat=_L8, n_rays=37, K=K, seed=720 + K, NS=2, **fu.intr_rows(2)) for K in (1, 5, 24)}
# more than one chunk of CAMG_CHUNK points per (object, view) (k_cam_partial / k_cam_fold): three objects of two views, so that
# the object offset and the view stride are no power of two; a chunk one short of full, a full one, a one-point tail, and 17
# points behind three full chunks.  TAIL_OBJ: the object whose last chunk alone carries the tail-only cotangent.
CHUNK = 1024
MULTI_P = (1023, 1024, 1025, 3 * CHUNK + 17)
TAIL_OBJ = {1023: 1, 1024: 1, 1025: 2, 3 * CHUNK + 17: 2}
# rays mode, two objects of two views, a row per object: (rays per object, K).  43 x 24 = 1032 points: ray 42 holds points
# 1008 .. 1031, across the chunk boundary; 211 x 5 = 1055: an odd K and a 31-point tail.  The tail-only cotangent is object 1's.
MULTI_RAYS = ((43, 24), (211, 5))
RAY_TAIL_OBJ = 1
_cache = {}


def point_case(name):
    if ("p", name) not in _cache:
        _cache["p", name] = fu.interior_case(**POINT_CASES[name])
    return _cache["p", name]


def multi_case(P):
    """SB 3, NS 2, P points per object, a focal and a c row per object."""
    if ("m", P) not in _cache:
        _cache["m", P] = fu.interior_case(lat=_L8, SB=3, NS=2, P=P, d_hidden=64, seed=770, **fu.intr_rows(3))
    return _cache["m", P]


def multi_ray_case(n_rays, K, SB=2, seed=780):
    """fused_fp64_util.rays_case for SB objects: n_rays rays per object towards the object's own target camera (interior_case's),
    K sorted depths each; rays (SB n_rays, 8), z (SB n_rays, K), object-major as render_train hands them over."""
    if ("mr", n_rays, K, SB) not in _cache:
        case = fu.interior_case(lat=_L8, SB=SB, NS=2, P=n_rays, d_hidden=64, seed=seed + K, **fu.intr_rows(SB))
        spec = case["spec"]
        W, H = spec["image"]
        rng = np.random.default_rng((seed + K) * 1000 + 8)
        rays = [gu.pinhole_rays(gu.pose_spherical(75.0 + 5.0 * sb, -25.0, spec["radius"]), W, H, spec["focal"], spec["z_near"],
                                spec["z_far"], rng.integers(0, W * H, size=n_rays)) for sb in range(SB)]
        z = np.sort(rng.uniform(spec["z_near"], spec["z_far"], size=(SB * n_rays, K)).astype(np.float32), axis=1)
        case.update(rays=np.concatenate(rays).astype(np.float32), z=z)
        case.pop("xyz"), case.pop("dirs")
        _cache["mr", n_rays, K, SB] = case
    return _cache["mr", n_rays, K, SB]


def ray_case(K):
    """fused_fp64_util.rays_case at d_hidden 64; K = 24: the last 8 depths of a ray repeat 8 of its first 16, then sorted."""
    if ("r", K) not in _cache:
        case = fu.rays_case(**RAY_CASES[K])
        case["spec"] = dict(case["spec"], d_hidden=64)
        if K == 24:
            z = case["z"].copy()
            z[:, 16:] = z[:, 4:12]
            case["z"] = np.sort(z, axis=1)
        case.pop("xyz"), case.pop("dirs")
        _cache["r", K] = case
    return _cache["r", K]


MULTI_IDS = [("points", P) for P in MULTI_P] + [("rays", nk) for nk in MULTI_RAYS]


def multi_truth(kind, key, cot_name):
    """(case, cotangent, float64 truth, fp32 restatement) of a multi-chunk case under its "full" or "tail" cotangent, computed
    once per process."""
    if ("mt", kind, key, cot_name) not in _cache:
        rays_mode = kind == "rays"
        case = multi_ray_case(*key) if rays_mode else multi_case(key)
        if cot_name == "tail":
            cot = tail_cotangent(case, RAY_TAIL_OBJ if rays_mode else TAIL_OBJ[key], rays_mode)
        else:
            cot = cotangent(case, n_points=key[0] * key[1] if rays_mode else None, rays_mode=rays_mode)
        _cache["mt", kind, key, cot_name] = (case, cot, point_truth(case, cot, rays_mode=rays_mode)[1],
                                             point_truth(case, cot, dtype=torch.float32, rays_mode=rays_mode)[1])
    return _cache["mt", kind, key, cot_name]


def ray_points(case):
    """(xyz (SB, n K, 3), dirs) of a ray case in float64 from its fp32 rays and depths."""
    SB = case["spec"]["SB"]
    r, z = case["rays"].astype(np.float64), case["z"].astype(np.float64)
    xyz = r[:, None, :3] + z[..., None] * r[:, None, 3:6]
    return xyz.reshape(SB, -1, 3), np.ascontiguousarray(np.broadcast_to(r[:, None, 3:6], xyz.shape)).reshape(SB, -1, 3)


RELU_MARGIN = 2.0 ** -20       # 16 ulp of fp32, relative to the layer's largest input
MAX_MASKED = tu.MASK_MAX_FRACTION


def relu_keep(case, rays_mode=False):
    """(SB, P) bool, the points to KEEP: those none of whose ReLU inputs (every layer, every view, the density head) lies within
    RELU_MARGIN of zero in the float64 forward.  An fp32 forward — the kernels' as much as the fp32 restatement's — may decide
    such a unit the other way, and that point's gradient is then another function's (train_fp64_util.l2_compare says the same
    of the sums); it is no property of the backward.  The mask comes from float64 alone and zeroes the point's cotangent
    (cotangent()), as masked_cotangents does for the renderer's discontinuities; at most MAX_MASKED of a case's points."""
    key = "_keep_rays" if rays_mode else "_keep"
    if key not in case:
        spec = case["spec"]
        xyz, dirs = ray_points(case) if rays_mode else (case["xyz"], case["dirs"])
        SB, NS, P = spec["SB"], spec["NS"], np.asarray(xyz).shape[1]
        seen, orig = [], torch.relu

        def spy(x):
            seen.append(x.detach())
            return orig(x)
        torch.relu = spy
        try:
            sd = {k: torch.from_numpy(np.asarray(v)).to(F64) for k, v in gu.make_mlp_state(spec, "coarse").items()}
            with fu._scaled_lookup(case.get("uv_scale")), torch.no_grad():
                orc.point_forward(sd, tu.fp64_camera(spec, case["poses"]), [torch.from_numpy(m).to(F64) for m in case["maps"]],
                                  torch.from_numpy(np.asarray(xyz)).to(F64), torch.from_numpy(np.asarray(dirs)).to(F64), NS, **_kw(spec))
        finally:
            torch.relu = orig
        margin = np.full(SB * P, np.inf)
        for x in seen:
            rows = x.reshape(-1, x.shape[-1])
            m = (rows.abs().min(1).values / rows.abs().max()).numpy()
            assert m.size in (SB * NS * P, SB * P), (m.size, SB, NS, P)
            margin = np.minimum(margin, m.reshape(SB, NS, P).min(1).reshape(-1) if m.size == SB * NS * P and NS > 1 else m)
        assert len(seen) >= 2 * spec["n_blocks"] + 1, len(seen)
        case[key] = (margin >= RELU_MARGIN).reshape(SB, P)
    return case[key]


def cotangent(case, n_points=None, seed=9, rays_mode=False):
    """Seeded (SB, P, 4) cotangent of the network's outputs, zero at the points relu_keep takes out."""
    SB = case["spec"]["SB"]
    P = n_points if n_points is not None else case["xyz"].shape[1]
    cot = np.random.default_rng(case["spec"]["seed"] * 10 + seed).standard_normal((SB, P, 4)).astype(np.float32)
    cot[~relu_keep(case, rays_mode)[:, :P]] = 0.0
    return cot


def tail_cotangent(case, obj, rays_mode=False):
    """cotangent() with everything zeroed but the points of the last chunk of CHUNK points of object `obj`: the only records
    that are not exact zeros are that one chunk's, so a sum that leaves them out, or takes them into another object's or
    view's row, has nothing else to hide the difference in."""
    cot = cotangent(case, n_points=case["z"].size // case["spec"]["SB"] if rays_mode else None, rays_mode=rays_mode)
    first = (cot.shape[1] - 1) // CHUNK * CHUNK
    out = np.zeros_like(cot)
    out[obj, first:] = cot[obj, first:]
    return out


def class_counts(case, xyz=None):
    """(interior fraction, clamped pairs, pairs behind a camera) of a case's (view, point) pairs, from the float64 geometry."""
    cls = fu.tap_class(case["spec"], case["poses"], case["xyz"] if xyz is None else xyz, None, case.get("uv_scale"))
    return float((cls == 0).mean()), int(((cls > 0) & (cls < 4)).sum()), int((cls == 4).sum())


# ----------------------------------------------------------------------------- truth: autograd with the cameras as leaves
def _leaf(t, dtype):
    return torch.as_tensor(np.asarray(t)).to(dtype).clone().requires_grad_(True)


def _kw(spec):
    return dict(use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"], combine_layer=spec["combine_layer"],
                combine_type=spec["combine_type"])


def stored_cameras(spec, poses, dtype=F64):
    """(w2c (SB*NS, 3, 4), focal rows with fy negated, c rows) as PixelNeRFNet.set_cameras stores them, each a leaf."""
    return tuple(t.detach().clone().requires_grad_(True) for t in tu.fp64_camera(spec, poses, dtype))


def point_truth(case, cot, dtype=F64, rays_mode=False, sd=None):
    """The oracle's point_forward under autograd with (w2c, focal, c) and xyz + viewdirs (or the rays) as leaves:
    (out, dict(poses, focal, c, xyz, dirs | rays)).  dtype = torch.float32: the restatement the per-view sums are measured in."""
    spec = case["spec"]
    sd = sd if sd is not None else gu.make_mlp_state(spec, "coarse")
    sd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    lat = [torch.from_numpy(np.asarray(m)).to(dtype) for m in case["maps"]]
    cam = stored_cameras(spec, case["poses"], dtype)
    if rays_mode:
        rays = _leaf(case["rays"], dtype)
        z = torch.from_numpy(case["z"]).to(dtype)
        xyz = (rays[:, None, :3] + z.unsqueeze(2) * rays[:, None, 3:6]).reshape(spec["SB"], -1, 3)
        dirs = rays[:, None, 3:6].expand(-1, z.shape[1], -1).reshape(spec["SB"], -1, 3)
        leaves = dict(rays=rays)
    else:
        xyz, dirs = _leaf(case["xyz"], dtype), _leaf(case["dirs"], dtype)
        leaves = dict(xyz=xyz, dirs=dirs)
    with fu._scaled_lookup(case.get("uv_scale")):
        out = orc.point_forward(sd, cam, lat, xyz, dirs, spec["NS"], **_kw(spec))
    (out * torch.from_numpy(np.asarray(cot)).to(dtype).reshape(out.shape)).sum().backward()
    leaves.update(poses=cam[0], focal=cam[1], c=cam[2])
    g = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).double().numpy() for k, t in leaves.items()}
    return out.detach().double().numpy(), g


# ----------------------------------------------------------------------------- the kernels' arithmetic, restated
MUTANTS = ("dt := dxr", "dR transposed", "no ddr x d in dR", "d_d without sum d_dir", "d_d without z", "record of the next view",
           "dfy sign", "per-object rows folded as per-view", "du without usx", "slope on clamped taps")


def mutant_acts(mutant, case, rays_mode):
    """Whether the planted mistake changes anything on this case (a per-object fold needs per-object rows, ...)."""
    spec = case["spec"]
    nv = spec["SB"] * spec["NS"]
    if mutant in ("d_d without sum d_dir", "d_d without z"):
        return rays_mode
    if mutant == "record of the next view":
        return nv > 1
    if mutant == "per-object rows folded as per-view":
        f, c = gu.intrinsics(spec)
        rows = [np.shape(t)[0] for t in (f, c) if t is not None and np.ndim(t) == 2]
        return spec["NS"] > 1 and spec["SB"] > 1 and spec["SB"] in rows
    if mutant == "du without usx":
        return bool(case.get("uv_scale"))
    return True


def mutant_keys(mutant):
    """The gradients the mistake shows in."""
    return {"dt := dxr": ("poses",), "dR transposed": ("poses",), "no ddr x d in dR": ("poses",),
            "d_d without sum d_dir": ("rays",), "d_d without z": ("rays",),
            "record of the next view": ("poses", "focal", "c"), "dfy sign": ("focal",),
            "per-object rows folded as per-view": ("focal", "c"), "du without usx": ("poses", "focal", "c"),
            "slope on clamped taps": ("poses", "focal", "c")}[mutant]


def _fold_rows(per_view, rows, SB, NS, as_per_view=False):
    nv = SB * NS
    if rows == nv:
        return per_view
    if rows == 1:
        return per_view.sum(0, keepdims=True)
    assert rows == SB
    return per_view[:SB] if as_per_view else per_view.reshape(SB, NS, 2).sum(1)


def formula(case, cot, rays_mode=False, mutant=None):
    """include/pnr.h's arithmetic in float64 from the oracle's d(zx): dict(poses, focal, c, xyz, dirs | rays)."""
    return _formula(case, cot, rays_mode, mutant)[0]


def records(case, cot, rays_mode=False):
    """k_cam_grad's records in float64, in the workspace's layout: (NS * SB * P, 16), row v * (SB P) + obj * P + point holds
    [dR 9 | dt 3 | dfx dfy dcx dcy] of view v of the point's object — what fold() sums."""
    spec = case["spec"]
    rec = _formula(case, cot, rays_mode, None)[1]                       # (SB NS, P, 16), stored-view major
    return rec.reshape(spec["SB"], spec["NS"], -1, 16).permute(1, 0, 2, 3).reshape(-1, 16).numpy()


def cam_from_sums(case, sums):
    """dict(poses, focal, c) from the (SB NS, 16) per-view sums: the stored w2c's layout and the intrinsics rows the case
    stores (render/autograd.py's _rows_as_stored)."""
    spec = case["spec"]
    SB, NS = spec["SB"], spec["NS"]
    focal, c = (t for t in tu.fp64_camera(spec, case["poses"], F64)[1:])
    rec = np.asarray(sums, np.float64)
    return dict(poses=np.concatenate((rec[:, :9].reshape(-1, 3, 3), rec[:, 9:12].reshape(-1, 3, 1)), axis=2),
                focal=_fold_rows(rec[:, 12:14], focal.shape[0], SB, NS), c=_fold_rows(rec[:, 14:16], c.shape[0], SB, NS))


def _formula(case, cot, rays_mode, mutant):
    """(formula's dict, the per-(view, point) records (SB NS, P, 16) as a tensor)."""
    spec = case["spec"]
    SB, NS = spec["SB"], spec["NS"]
    nv = SB * NS
    uv_scale = case.get("uv_scale")
    if rays_mode:
        xyz_np, dirs_np = ray_points(case)
    else:
        xyz_np, dirs_np = case["xyz"], case["dirs"]
    P = xyz_np.shape[1]
    sd = {k: torch.from_numpy(np.asarray(v)).to(F64) for k, v in gu.make_mlp_state(spec, "coarse").items()}
    lat = [torch.from_numpy(np.asarray(m)).to(F64) for m in case["maps"]]
    w2c, focal, c = (t.detach() for t in tu.fp64_camera(spec, case["poses"], F64))
    xyz, dirs = torch.from_numpy(np.asarray(xyz_np)).to(F64), torch.from_numpy(np.asarray(dirs_np)).to(F64)
    with fu._scaled_lookup(uv_scale):
        out, st = orc.point_forward(sd, (w2c, focal, c), lat, xyz, dirs, NS, return_stages=True, **_kw(spec))
    L = sum(ch for ch, _, _ in spec["lat"])
    zx = st["mlp_in"].detach().requires_grad_(True)                   # d(zx): the network behind the assembled rows
    o = orc.resnetfc(sd, zx, L, NS, P, spec["n_blocks"], spec["combine_layer"], spec["combine_type"]).reshape(-1, P, 4)
    o = torch.cat([torch.sigmoid(o[..., :3]), torch.relu(o[..., 3:4])], dim=-1).reshape(SB, P, 4)
    dzx, = torch.autograd.grad((o * torch.from_numpy(np.asarray(cot)).to(F64).reshape(o.shape)).sum(), zx)
    dzx = dzx.reshape(nv, P, -1)
    rep = lambda t: t.unsqueeze(1).expand(-1, NS, *t.shape[1:]).reshape(-1, *t.shape[1:])
    R, t = w2c[:, :, :3], w2c[:, :, 3]
    p, d = rep(xyz), rep(dirs)                                         # (nv, P, 3)
    xr = torch.einsum("vij,vpj->vpi", R, p)
    dr = torch.einsum("vij,vpj->vpi", R, d)
    xc = xr + t[:, None, :]
    per_view = lambda a: a if a.shape[0] == nv else (a.expand(nv, 2) if a.shape[0] == 1 else rep(a.unsqueeze(1)).reshape(nv, 2))
    fv, cv = per_view(focal), per_view(c)                              # (nv, 2), fy negated
    uv = -xc[..., :2] / xc[..., 2:] * fv[:, None, :] + cv[:, None, :]
    # the lookup's slope per level, with the level's uv scale
    du = torch.zeros(nv, P, dtype=F64)
    dv = torch.zeros(nv, P, dtype=F64)
    c0 = 0
    for lvl, (ch, h, w) in enumerate(spec["lat"]):
        sx, sy = uv_scale[lvl] if uv_scale else (1.0, 1.0)
        tex = (uv * torch.tensor([sx, sy], dtype=F64)).detach()
        if mutant == "slope on clamped taps":                            # the slope just inside the border instead of zero
            eps = 1e-3
            tex = torch.stack((tex[..., 0].clamp(eps, w - 1 - eps), tex[..., 1].clamp(eps, h - 1 - eps)), dim=-1)
            tex = torch.where(torch.isfinite(tex), tex, torch.zeros_like(tex))
        tex.requires_grad_(True)
        val = orc.index_latent(tex, [lat[lvl]])                        # (nv, C, P)
        g, = torch.autograd.grad((val.transpose(1, 2) * dzx[..., c0:c0 + ch]).sum(), tex)
        du = du + g[..., 0] * (1.0 if mutant == "du without usx" else sx)
        dv = dv + g[..., 1] * sy
        c0 += ch
    # the positional code
    dcode = dzx[..., L:]
    dd = 6 if spec["use_code_viewdirs"] else 3
    nf, ff = 6, 1.5
    x = torch.cat((xr, dr), dim=-1) if dd == 6 else xr
    dx = dcode[..., :dd].clone()
    half_pi = float(np.float32(np.pi * 0.5))
    for q in range(2 * nf):
        f = ff * 2.0 ** (q // 2)
        dx = dx + dcode[..., dd + q * dd: dd + (q + 1) * dd] * (f * torch.cos(x * f + (half_pi if q & 1 else 0.0)))
    n_code = dd + 2 * nf * dd
    ddr = dx[..., 3:6] if dd == 6 else dcode[..., n_code:n_code + 3]
    zc = xc[..., 2]
    dt = torch.stack((du * (-fv[:, None, 0] / zc), dv * (-fv[:, None, 1] / zc),
                      du * xc[..., 0] * fv[:, None, 0] / zc ** 2 + dv * xc[..., 1] * fv[:, None, 1] / zc ** 2), dim=-1)
    dxr = dx[..., :3] + dt
    dR = torch.einsum("vpi,vpj->vpij", dxr, p)
    if mutant != "no ddr x d in dR":
        dR = dR + torch.einsum("vpi,vpj->vpij", ddr, d)
    if mutant == "dR transposed":
        dR = dR.transpose(-1, -2)
    dt_out = dxr if mutant == "dt := dxr" else dt
    intr = torch.stack((du * (-xc[..., 0] / zc), dv * (-xc[..., 1] / zc) * (-1.0 if mutant == "dfy sign" else 1.0), du, dv), dim=-1)
    rec_pv = torch.cat((dR.reshape(nv, P, 9), dt_out, intr), dim=-1)              # (nv, P, 16)
    rec = rec_pv.sum(1)                                                           # (nv, 16)
    if mutant == "record of the next view":
        rec = torch.roll(rec, -1, dims=0)
    rec = rec.numpy()
    as_pv = mutant == "per-object rows folded as per-view"
    g = dict(poses=np.concatenate((rec[:, :9].reshape(nv, 3, 3), rec[:, 9:12].reshape(nv, 3, 1)), axis=2),
             focal=_fold_rows(rec[:, 12:14], focal.shape[0], SB, NS, as_pv), c=_fold_rows(rec[:, 14:16], c.shape[0], SB, NS, as_pv))
    dp = torch.einsum("vij,vpi->vpj", R, dxr).reshape(SB, NS, P, 3).sum(1)
    ddir = torch.einsum("vij,vpi->vpj", R, ddr).reshape(SB, NS, P, 3).sum(1)
    if rays_mode:
        n, K = case["z"].shape
        z = torch.from_numpy(case["z"]).to(F64)
        dp, ddir = dp.reshape(n, K, 3), ddir.reshape(n, K, 3)
        d_d = (dp if mutant == "d_d without z" else z[..., None] * dp).sum(1)
        if mutant != "d_d without sum d_dir":
            d_d = d_d + ddir.sum(1)
        g["rays"] = torch.cat((dp.sum(1), d_d, torch.zeros(n, 2, dtype=F64)), dim=-1).numpy()
    else:
        g["xyz"], g["dirs"] = dp.numpy(), ddir.numpy()
    return g, rec_pv


# ----------------------------------------------------------------------------- k_cam_partial and k_cam_fold, restated
FOLD_MUTANTS = ("tail chunk dropped", "tail chunk read at a full chunk's length", "no object offset", "view stride pts_per_obj",
                "chunk count and length from P", "partials indexed chunk * views + view", "fold stops one chunk early",
                "second chunk in place of the first")


def fold_mutant_acts(mutant, SB, NS, pts_per_obj, chunk=CHUNK):
    """Whether the planted mistake changes a sum at these sizes."""
    n_chunks = -(-pts_per_obj // chunk)
    return {"tail chunk dropped": pts_per_obj % chunk != 0, "tail chunk read at a full chunk's length": pts_per_obj % chunk != 0,
            "no object offset": SB > 1, "view stride pts_per_obj": SB > 1 and NS > 1, "chunk count and length from P": SB > 1,
            "partials indexed chunk * views + view": n_chunks > 1 and SB * NS > 1, "fold stops one chunk early": True,
            "second chunk in place of the first": n_chunks > 1}[mutant]


# the cotangent under which a planted mistake must sit at MUTANT_FACTOR or more on EVERY case it acts on (the other one is
# printed).  "full" only: under the tail-only cotangent of the LAST object the records a mistaken index reaches instead are
# exact zeros (the next view's first objects, or nothing at all behind the last view), and at four chunks the first and the
# second chunk are both zero.  "tail" only: a tail of 1 or 17 points is a share of the full sum that shrinks with P.
FOLD_MUTANT_COTANGENT = {"tail chunk dropped": "tail", "tail chunk read at a full chunk's length": "full", "no object offset": "tail",
                         "view stride pts_per_obj": "tail", "chunk count and length from P": "tail",
                         "partials indexed chunk * views + view": "tail", "fold stops one chunk early": "tail",
                         "second chunk in place of the first": "full"}


def fold(records, SB, NS, pts_per_obj, chunk=CHUNK, mutant=None):
    """k_cam_partial and k_cam_fold in float64 on records() -> the (SB NS, 16) per-view sums: per (object, view) and chunk, 16
    sub-sums of the records s, s + 16, .. in that order, added in order s = 0 .. 15; the chunk sums folded in chunk order.
    mutant: one mistake planted in the index arithmetic.  A read past the end of the records or of the partials gives zeros
    here (on the device: whatever the workspace holds behind them).
    "chunk count and length from P": in the kernel as it stands a block past an object's last chunk finds nothing left and
    adds nothing, so a chunk count from P alone could never show; the planted form takes the length left from P as well and
    runs on into the records that follow."""
    rec = np.asarray(records, np.float64).reshape(-1, 16)
    P = SB * pts_per_obj
    assert rec.shape[0] == NS * P, (rec.shape, SB, NS, pts_per_obj)
    views = SB * NS
    per_obj = P if mutant == "chunk count and length from P" else pts_per_obj
    n_chunks = -(-per_obj // chunk)
    stride = pts_per_obj if mutant == "view stride pts_per_obj" else P
    part = np.zeros((views * n_chunks + n_chunks + 1, 16))
    for view in range(views):
        obj, v = divmod(view, NS)
        for ch in range(n_chunks):
            first = ch * chunk
            n = min(per_obj - first, chunk)
            if mutant == "tail chunk dropped" and n < chunk:
                continue
            if mutant == "tail chunk read at a full chunk's length":
                n = chunk
            r0 = v * stride + (0 if mutant == "no object offset" else obj * pts_per_obj) + first
            blk = np.zeros((-(-n // 16) * 16, 16))
            got = rec[r0:r0 + n]
            blk[:got.shape[0]] = got
            blk = blk.reshape(-1, 16, 16)                                # [j, sub, comp]: record j * 16 + sub
            sub = np.zeros((16, 16))
            for j in range(blk.shape[0]):
                sub += blk[j]
            total = sub[0].copy()
            for k in range(1, 16):
                total += sub[k]
            part[ch * views + view if mutant == "partials indexed chunk * views + view" else view * n_chunks + ch] = total
    sums = np.zeros((views, 16))
    for view in range(views):
        for k in range(n_chunks - (1 if mutant == "fold stops one chunk early" else 0)):
            sums[view] += part[view * n_chunks + (1 if mutant == "second chunk in place of the first" and k == 0 else k)]
    return sums


# ----------------------------------------------------------------------------- the rules
POINT_KEYS = ("xyz", "dirs", "rays")          # per point / per ray: every entry
VIEW_KEYS = ("poses", "focal", "c")           # sums over all points of an object through ReLUs: l2 with the fp32 restatement


def _sel(g, keys):
    out = {}
    for k in keys:
        if k in g:
            out[k] = np.asarray(g[k])[:, :6] if k == "rays" else g[k]
    return out


def compare(got, truth, ref32, what, check=True):
    """The issue's rules: full_compare at 5e-4 on d_xyz / d_dirs / d_rays[:, :6], l2_compare(5e-4, ref32) on d_poses / d_focal /
    d_c.  Returns {key: figure / bound} (> 1 fails); check=False reports only."""
    ratios = {k: v / RTOL for k, v in tu.entry_ratios(_sel(got, POINT_KEYS), _sel(truth, POINT_KEYS)).items()}
    ours = tu.rel_l2(_sel(got, VIEW_KEYS), _sel(truth, VIEW_KEYS))
    ref = tu.rel_l2(_sel(ref32, VIEW_KEYS), _sel(truth, VIEW_KEYS)) if ref32 is not None else {}
    for k, r in ours.items():
        ratios[k] = r / max(RTOL, tu.L2_REF32_FACTOR * ref.get(k, 0.0))
    if check:
        tu.full_compare(_sel(got, POINT_KEYS), _sel(truth, POINT_KEYS), RTOL, what)
        tu.l2_compare(_sel(got, VIEW_KEYS), _sel(truth, VIEW_KEYS), RTOL, what, ref32=None if ref32 is None else _sel(ref32, VIEW_KEYS))
    return ratios


def view_pieces(g):
    """{label: array}: d(poses) split into the stored views (12 numbers each), d(focal) and d(c) into their stored rows."""
    out = {}
    for k in VIEW_KEYS:
        if k in g:
            a = np.asarray(g[k], dtype=np.float64)
            a = a.reshape(-1, 12) if k == "poses" else a.reshape(-1, 2)
            out.update({f"{k}[{i}]": a[i] for i in range(a.shape[0])})
    return out


def compare_per_view(got, truth, ref32, what, check=True):
    """l2_compare(RTOL, ref32) on every stored view of d(poses) and every stored row of d(focal), d(c) on its own: a whole
    tensor's l2 lets a view, or a short tail chunk of one, hide behind the others.  A piece whose truth is exactly zero (the
    tail-only cotangent) must be exactly zero.  Prints and returns the worst piece: dict(piece, figure, ref, ratio) with
    figure / ref the kernel's and the fp32 restatement's relative l2 and ratio = figure / bound (inf: not zero where the truth
    is).  check=False asserts and prints nothing (the planted mistakes)."""
    gp, tp, rp = view_pieces(got), view_pieces(truth), view_pieces(ref32)
    assert gp.keys() == tp.keys() == rp.keys() and len(tp) > 0, (what, list(gp), list(tp))
    worst, bad = dict(piece=None, figure=0.0, ref=0.0, ratio=-1.0), []
    for k, t in tp.items():
        if not t.any():
            fig, ref = float(np.linalg.norm(gp[k])), float(np.linalg.norm(rp[k]))
            ratio = 0.0 if not np.asarray(gp[k]).any() else np.inf              # a NaN is not zero either
            if ratio:
                bad.append(f"{k}: norm {fig:.3e} where the truth is exactly zero")
        else:
            fig, ref = tu.rel_l2({k: gp[k]}, {k: t})[k], tu.rel_l2({k: rp[k]}, {k: t})[k]
            ratio = fig / max(RTOL, tu.L2_REF32_FACTOR * ref) if np.isfinite(fig) else np.inf
            if check:
                try:
                    tu.l2_compare({k: gp[k]}, {k: t}, RTOL, what, ref32={k: rp[k]})
                except AssertionError as e:
                    bad.append(str(e))
        if not ratio <= worst["ratio"]:
            worst = dict(piece=k, figure=fig, ref=ref, ratio=ratio)
    if check:
        print(f"{what}: worst per view {worst['piece']} {worst['figure']:.1e} / {worst['ref']:.1e}")
    assert not (check and bad), f"{what}, per view: " + "; ".join(bad)
    return worst


def table_line(what, got, truth, ref32):
    """kernel figure / restatement figure per tensor, for DESIGN §4.14's table."""
    pe, pr = tu.entry_ratios(_sel(got, POINT_KEYS), _sel(truth, POINT_KEYS)), tu.entry_ratios(_sel(ref32, POINT_KEYS), _sel(truth, POINT_KEYS))
    ve, vr = tu.rel_l2(_sel(got, VIEW_KEYS), _sel(truth, VIEW_KEYS)), tu.rel_l2(_sel(ref32, VIEW_KEYS), _sel(truth, VIEW_KEYS))
    cells = [f"{k} {pe[k]:.1e} / {pr[k]:.1e}" for k in pe] + [f"{k} {ve[k]:.1e} / {vr[k]:.1e}" for k in ve]
    return f"{what}: " + ", ".join(cells)


# ----------------------------------------------------------------------------- a whole step (render_train)
# coarse + fine with depth samples on the 8 x 8 interior geometry, a focal and a c row per object.  Seeds: the fp32
# restatement against float64 masks at most MASK_MAX_FRACTION of the rays (tests/test_cam_grad_cpu.py).
STEP_SPEC = gu._case(seed=741, d_hidden=64, lat=_L8, image=(8, 8), focal=fu.F8, SB=2, NS=2, N=64, Kc=16, Kf=8, Kfd=4,
                     **gu.scaled_intrinsics(fu.F8, (8, 8)))
STEP_NOISE_SEED = 7


def _render_kw(spec):
    return dict(use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"], combine_layer=spec["combine_layer"],
                combine_type=spec["combine_type"])


def step_truth(spec, rays_np, poses_np, maps_np, noise, cot, mask, dtype=F64):
    """train_fp64_util.fp64_step with the rays, the c2w source poses, focal and c (as a caller hands them to set_cameras) as
    leaves: dict(out, keep, grads = {rays (n, 8), poses (SB*NS, 4, 4), focal, c})."""
    sd_c, sd_f, lat = tu.fp64_leaves(spec, maps_np, None, dtype)
    rays, c2w = _leaf(rays_np, dtype), _leaf(np.asarray(poses_np).reshape(-1, 4, 4), dtype)
    f_np, c_np = gu.intrinsics(spec)
    W, H = spec["image"]
    focal = _leaf(f_np, dtype)                                         # a 0-dim leaf or rows of (fx, fy), fy positive
    c = None if c_np is None else _leaf(c_np, dtype)
    rot = c2w[:, :3, :3].transpose(1, 2)                               # encode_cameras' statements, in dtype
    w2c = torch.cat((rot, -torch.bmm(rot, c2w[:, :3, 3:])), dim=-1)
    f2 = focal[None, None].repeat(1, 2) if focal.dim() == 0 else focal
    cam = (w2c, f2 * torch.tensor([1.0, -1.0], dtype=dtype), torch.tensor([[W * 0.5, H * 0.5]], dtype=dtype) if c is None else c)
    out = orc.render(sd_c, sd_f, cam, lat, rays, spec["NS"], spec["Kc"], spec["Kf"], spec["Kfd"], spec["depth_std"],
                     spec["white_bkgd"], spec["lindisp"], {k: v.to(dtype) for k, v in noise.items()}, **_render_kw(spec))
    keep = mask(out) if callable(mask) else np.asarray(mask)
    cm = {k: torch.from_numpy(v).to(dtype) for k, v in tu.masked_cotangents(cot, keep).items()}
    tu.step_loss(out, cm).backward()
    grads = dict(rays=rays.grad.reshape(-1, 8), poses=c2w.grad, focal=focal.grad)
    if c is not None:
        grads["c"] = c.grad
    return dict(out=out, keep=keep, grads={k: v.double().numpy() for k, v in grads.items()})


# ----------------------------------------------------------------------------- the reference's own camera gradients
CAMGRAD_FIXTURES = ("tiny_sb2_ns2", "tiny_sb2_ns2_intr")          # tools/gen_golden_cam_grad.py; the second: (fx, fy), off-centre c


def load_camgrad_fixture(name):
    import os
    z = np.load(os.path.join(gu.GOLDEN_DIR, name + "_camgrad.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def fixture_keys(grads):
    """step_truth's / the device's gradients under the fixture's keys: rays_od = columns 0:6, rays_nf = columns 6:8."""
    g = {k: np.asarray(v) for k, v in grads.items() if k != "rays"}
    r = np.asarray(grads["rays"]).reshape(-1, 8)
    g["rays_od"], g["rays_nf"] = r[:, :6], r[:, 6:]
    return g


def oracle_cam_grads(fx, dtype=torch.float32):
    """The oracle's render on a forward fixture's inputs and recorded draws with the cameras and rays as leaves."""
    spec = fx["spec"]
    keep = np.ones((spec["SB"], spec["N"]), bool)
    t = step_truth(spec, fx["rays"], fx["poses"], gu.make_latents(spec), gu.noise_from_fixture(fx), gu.make_loss_weights(spec),
                   keep, dtype)
    return fixture_keys(t["grads"])


# ----------------------------------------------------------------------------- pose refinement
# one MLP for both passes: the coarse and the fine colour both approach the photograph as the pose does
POSE_SPEC = gu._case(seed=761, d_hidden=64, lat=_L8, image=(8, 8), focal=fu.F8, SB=1, NS=2, N=64, Kc=16, Kf=8, Kfd=4, fine_mlp=False)
POSE_RAYS, POSE_LR, POSE_SEED = 48, 2e-2, 5
POSE_OFFSET = (0.06, -0.05, 0.04, 0.08, -0.06, 0.05)        # xi of the start pose relative to the target's camera


def _pose_render(spec, sd_c, sd_f, lat, cam, rays, noise, dtype):
    return orc.render(sd_c, sd_f, cam, lat, rays[None], spec["NS"], spec["Kc"], spec["Kf"], spec["Kfd"], spec["depth_std"],
                      spec["white_bkgd"], spec["lindisp"], {k: v.to(dtype) for k, v in noise.items()}, **_render_kw(spec))


def _pose_parts(spec, poses, maps, dtype):
    sd_c = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in gu.make_mlp_state(spec, "coarse").items()}
    return sd_c, None, [torch.from_numpy(m).to(dtype) for m in maps], tu.fp64_camera(spec, poses, dtype)


def pose_case():
    """A photograph of the synthetic scene (the oracle's float64 fine render of every pixel from the target camera) and a start
    pose POSE_OFFSET away from it; pix / noise: the first step's pixel set and explicit draws."""
    if "pose" not in _cache:
        from pixel_nerf_multiscale_amd import pose
        spec = POSE_SPEC
        _, poses = gu.make_inputs(spec)
        maps = gu.make_latents(spec)
        W, H = spec["image"]
        true = torch.from_numpy(gu.pose_spherical(75.0, -25.0, spec["radius"])).double()
        parts = _pose_parts(spec, poses, maps, F64)
        n = W * H
        with torch.no_grad():
            rays = pose.rays_at(true, torch.arange(n), W, H, spec["focal"], spec["z_near"], spec["z_far"])
            out = _pose_render(spec, *parts[:3], parts[3], rays, tu.make_noise(dict(spec, SB=1, N=n), 3), F64)
            pose0 = pose.se3_exp(torch.tensor(POSE_OFFSET, dtype=F64)) @ true
        pix = pose.step_pixels(POSE_SEED, 10, POSE_RAYS, n).numpy()
        _cache["pose"] = dict(spec=spec, poses=poses, maps=maps, target=out["fine"]["rgb"].reshape(H, W, 3).float().numpy(),
                              pose0=pose0.float().numpy(), pix=pix[0], pix_steps=pix,
                              noise=tu.make_noise(dict(spec, SB=1, N=POSE_RAYS), 11))
    return _cache["pose"]


def pose_loss(pc, parts, xi, pix, noise, dtype):
    """se3_exp -> rays_at -> the oracle's render -> RenderLoss(1, 1) (coarse + fine mean squared error) in dtype."""
    from pixel_nerf_multiscale_amd import pose
    spec = pc["spec"]
    W, H = spec["image"]
    rays = pose.rays_at(pose.se3_exp(xi) @ torch.from_numpy(pc["pose0"]).to(dtype), torch.from_numpy(pix), W, H, spec["focal"],
                        spec["z_near"], spec["z_far"])
    out = _pose_render(spec, *parts[:3], parts[3], rays, noise, dtype)
    gt = torch.from_numpy(pc["target"]).to(dtype).reshape(-1, 3)[torch.from_numpy(pix)][None]
    return out, ((out["coarse"]["rgb"] - gt) ** 2).mean() + ((out["fine"]["rgb"] - gt) ** 2).mean()


def pose_step_fp64(pc, sel, dtype=F64):
    """The first refinement step on the pixels pix[sel] with the case's explicit draws: dict(out, loss, grad d(loss)/d(xi))."""
    parts = _pose_parts(pc["spec"], pc["poses"], pc["maps"], dtype)
    xi = torch.zeros(6, dtype=dtype, requires_grad=True)
    out, loss = pose_loss(pc, parts, xi, pc["pix"][sel], {k: v[sel] for k, v in pc["noise"].items()}, dtype)
    g, = torch.autograd.grad(loss, xi)
    return dict(out=out, loss=float(loss.detach()), grad=g.double().numpy())


def pose_loop_fp64(pc, steps=10):
    """refine_pose's loop restated in float64 (Adam on xi, the same pixel sets, numpy draws per step): the losses."""
    spec = pc["spec"]
    parts = _pose_parts(spec, pc["poses"], pc["maps"], F64)
    xi = torch.zeros(6, dtype=F64, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=POSE_LR)
    losses = []
    for i in range(steps):
        noise = tu.make_noise(dict(spec, SB=1, N=POSE_RAYS), 100 + i)
        _, loss = pose_loss(pc, parts, xi, pc["pix_steps"][i], noise, F64)
        xi.grad, = torch.autograd.grad(loss, xi)
        opt.step()
        losses.append(float(loss.detach()))
    return losses
