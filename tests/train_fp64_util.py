"""fp64 truth for the training path (tests/test_gpu_train_fp64.py, tests/test_train_fp64_cpu.py): the oracle restatement
(oracle/pixelnerf_oracle.py) run in float64 under torch autograd, an every-entry comparison rule, and the ray mask that keeps
renderer discontinuities (a fine sample changing bin, a depth sample changing sort slot) out of a backward comparison.

Nothing here touches a GPU: the GPU file drives the HIP side and hands its results to these functions."""
import numpy as np
import torch

import golden_util as gu
from oracle import pixelnerf_oracle as orc

F64 = torch.float64
TRAIN_SCHEDULE = dict(d_hidden=512, n_blocks=5, combine_layer=3, Kc=64, Kf=32, Kfd=16)     # tools/bench_train.py
MASK_MAX_FRACTION = 0.05


def make_noise(spec, seed):
    """Fixed draws (reference draw order) for every ray of a spec: noise_c, u, r, g as fp32 (SB*N, .) tensors."""
    rng = np.random.default_rng(seed)
    n, Kc, Kf, Kfd = spec["SB"] * spec["N"], spec["Kc"], spec["Kf"], spec["Kfd"]
    noise = {"noise_c": rng.random((n, Kc))}
    if Kf > 0:
        if Kf - Kfd > 0:
            noise["u"], noise["r"] = rng.random((n, Kf - Kfd)), rng.random((n, Kf - Kfd))
        if Kfd > 0:
            noise["g"] = rng.standard_normal((n, Kfd))
    return {k: torch.from_numpy(v.astype(np.float32)) for k, v in noise.items()}


def fp64_leaves(spec, maps, sds=None, dtype=F64):
    """float64 leaf copies of both MLPs' parameters (make_mlp_state unless `sds` = (coarse, fine) state-dicts) and the maps."""
    if sds is None:
        sds = (gu.make_mlp_state(spec, "coarse"), gu.make_mlp_state(spec, "fine") if spec["fine_mlp"] else None)
    leaf = lambda v: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(True)
    sd_c = {k: leaf(v) for k, v in sds[0].items()}
    sd_f = None if sds[1] is None else {k: leaf(v) for k, v in sds[1].items()}
    return sd_c, sd_f, [leaf(m) for m in maps]


def fp64_camera(spec, poses, dtype=F64):
    W, H = spec["image"]
    return tuple(t.to(dtype) for t in orc.encode_cameras(torch.as_tensor(np.asarray(poses)), *gu.intrinsics(spec), W, H))


def fp64_forward(spec, rays, poses, maps, noise, sds=None, dtype=F64):
    """The oracle render of one training batch in float64: (outputs, (sd_c, sd_f, latent leaves))."""
    sd_c, sd_f, lat = fp64_leaves(spec, maps, sds, dtype)
    out = orc.render(sd_c, sd_f, fp64_camera(spec, poses, dtype), lat, torch.as_tensor(np.asarray(rays)).to(dtype), spec["NS"],
                     spec["Kc"], spec["Kf"], spec["Kfd"], spec["depth_std"], spec["white_bkgd"], spec["lindisp"],
                     {k: v.to(dtype) for k, v in noise.items()}, use_code_viewdirs=spec["use_code_viewdirs"],
                     n_blocks=spec["n_blocks"], combine_layer=spec["combine_layer"], combine_type=spec["combine_type"])
    return out, (sd_c, sd_f, lat)


def masked_cotangents(cot, keep):
    """cot: {coarse_rgb (SB,N,3), coarse_depth (SB,N), coarse_weights (SB,N,K), fine_*} numpy; every entry of a ray with
    keep False set to zero."""
    out = {}
    for k, v in cot.items():
        v = np.array(v, dtype=np.float32, copy=True)
        v[~keep] = 0.0
        out[k] = v
    return out


def step_loss(out, cot, get=lambda lvl, what: lvl[what]):
    """sum over the cotangent's passes of <rgb, G_rgb> + <depth, G_depth> + <weights, G_weights> (as hip_grads builds it);
    `out` the oracle's dict or the renderer's AttrDict, cot torch tensors of matching dtype / device."""
    loss = 0.0
    for tag in ("coarse", "fine"):
        if f"{tag}_rgb" not in cot:
            continue
        lvl = out[tag]
        for what in ("rgb", "depth", "weights"):
            loss = loss + (get(lvl, what).reshape(cot[f"{tag}_{what}"].shape) * cot[f"{tag}_{what}"]).sum()
    return loss


def fp64_grads(leaves, loss):
    sd_c, sd_f, lat = leaves
    loss.backward()
    grads = {}
    for which, sd in (("coarse", sd_c), ("fine", sd_f)):
        if sd is not None:
            for k, p in sd.items():
                if p.grad is not None:
                    grads[f"{which}.{k}"] = p.grad.numpy()
    for i, m in enumerate(lat):
        grads[f"latent.{i}"] = m.grad.numpy() if m.grad is not None else np.zeros(tuple(m.shape))
    return grads


def fp64_step(spec, noise, poses, maps, cot, mask, rays, sds=None, dtype=F64):
    """One training step of the oracle in float64: dict(out, z={coarse, fine}, keep, grads).  `mask`: a (SB,N) bool array of
    the rays to keep, or a callable out64 -> that array (the ray mask needs the float64 sample positions).  The loss is built
    after the mask, so the caller differentiates the same function on its side with masked_cotangents(cot, keep).
    dtype=torch.float32: the same restatement in fp32, what any fp32 implementation of the renderer can be expected to reach."""
    out, leaves = fp64_forward(spec, rays, poses, maps, noise, sds, dtype)
    keep = mask(out) if callable(mask) else (np.ones((spec["SB"], spec["N"]), bool) if mask is None else np.asarray(mask))
    c = {k: torch.from_numpy(v).to(dtype) for k, v in masked_cotangents(cot, keep).items()}
    grads = fp64_grads(leaves, step_loss(out, c))
    z = {t: out[t]["z"].detach().numpy() for t in ("coarse", "fine") if t in out}
    return dict(out=out, z=z, keep=keep, grads=grads)


def point_forward_oracle(spec, poses, maps_np, xyz, dirs, uv_scale=None, sd=None, dtype=F64, rec=None):
    """The oracle's point_forward at explicit points (SB,P,3) on fresh leaves: (out (SB,P,4), stages, (sd, maps, xyz) leaves).
    uv_scale: per level (sx, sy) applied to the pixel coordinates, as encoder.uv_scale = "image" makes the kernels do.
    rec: the oracle's ReLU-input recorder."""
    sd = sd if sd is not None else gu.make_mlp_state(spec, "coarse")
    sdo = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}
    lo = [torch.from_numpy(np.asarray(m)).to(dtype).requires_grad_(True) for m in maps_np]
    xo = torch.from_numpy(np.asarray(xyz)).to(dtype).requires_grad_(True)
    orig = orc.index_latent
    if uv_scale:
        def scaled(uv, latents):
            return torch.cat([orig(uv * torch.tensor(s, dtype=uv.dtype), [m]) for s, m in zip(uv_scale, latents)], dim=1)
        orc.index_latent = scaled
    hook = {} if rec is None else dict(rec=rec)
    try:
        o, st = orc.point_forward(sdo, fp64_camera(spec, poses, dtype), lo, xo, torch.from_numpy(np.asarray(dirs)).to(dtype), spec["NS"],
                                  use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"],
                                  combine_layer=spec["combine_layer"], combine_type=spec["combine_type"], return_stages=True,
                                  **hook)
    finally:
        orc.index_latent = orig
    return o, st, (sdo, lo, xo)


def point_grads_fp64(spec, poses, maps_np, xyz, dirs, cot, uv_scale=None, sd=None, stages=False, dtype=F64):
    """point_forward_oracle in float64 under autograd with cotangent cot (SB,P,4):
    (out, {coarse.*, latent.*, xyz}) [, d(zx) (SB*NS*P, L + d_in)]."""
    o, st, (sdo, lo, xo) = point_forward_oracle(spec, poses, maps_np, xyz, dirs, uv_scale, sd, dtype)
    zx = st["mlp_in"]
    zx.retain_grad()
    (o * torch.from_numpy(np.asarray(cot)).to(dtype)).sum().backward()
    g = {f"coarse.{k}": p.grad.numpy() for k, p in sdo.items()}
    g.update({f"latent.{i}": m.grad.numpy() for i, m in enumerate(lo)})
    g["xyz"] = xo.grad.numpy()
    if stages:
        return o.detach().numpy(), g, zx.grad.numpy()
    return o.detach().numpy(), g


# ----------------------------------------------------------------------------- explicit-point cases and the ReLU-margin mask
def point_spec(lat, NS=1, SB=1, d_hidden=64, combine_type="average", image=(8, 4), focal=2.0, seed=201, **kw):
    return gu._case(seed=seed, d_hidden=d_hidden, lat=lat, image=image, focal=focal, NS=NS, SB=SB, combine_type=combine_type, **kw)


def random_points(spec, P, seed):
    """P points per object inside the source frusta (what the renderer feeds the MLP), and their view directions."""
    rng = np.random.default_rng(seed)
    rays, _ = gu.make_inputs(dict(spec, N=max(P, 1), edge=False))
    xyz = np.zeros((spec["SB"], P, 3), np.float32)
    dirs = np.zeros_like(xyz)
    for sb in range(spec["SB"]):
        r = rays[sb, :P]
        t = spec["z_near"] + (spec["z_far"] - spec["z_near"]) * rng.random((P, 1))
        xyz[sb] = r[:, :3] + t * r[:, 3:6]
        dirs[sb] = r[:, 3:6]
    return xyz, dirs


# A unit is at risk when its fp64 ReLU input lies within RELU_MARGIN_FACTOR row deviations of 0 (relu_margin_mask).  Measured
# on the CPU with the oracle in fp64 and in fp32 alone, over every (case, P) of MARGIN_CASES x MARGIN_POINTS: the smallest
# power of two at which the fp32 restatement's worst entry error / scale over every gradient is <= 1e-5 is 1/2 (worst
# 7.6e-6, as at 1, 2 and 8; with no mask and at 1/4 up to 1.1e-2); times 4 for a correct fp32 implementation that sums
# in another order than torch.  Masked points at 2, of SB * P, P = 1001: lds_ns4 14 / 3003 (0.5 %), fix_ns2 5 (0.2 %),
# fix_ns3 12 (0.4 %), fix_ns4 9 (0.3 %), fix_ns4_max 10 (0.3 %), c512_ns3 8 (0.3 %), ms4_ns3 15 / 2002 (0.7 %),
# ms4_ns3_uv 5 / 2002 (0.2 %); at most 1.2 % at 255 .. 257 points per object (ms4_ns3, 6 / 510) and none at P = 1.  The
# argmax rule of fix_ns4_max adds no point at 2 (1 of 771 at 4, up to 3 of 3003 at 8).  At 8 the largest share is 4.1 %.
RELU_MARGIN_FACTOR = 2.0
MS4 = [(64, 16, 16), (64, 16, 16), (128, 8, 8), (256, 4, 4)]
# name -> (lat, route of the latent gradient, NS, SB, d_hidden, combine_type, uv_scale = "image")
MARGIN_CASES = {
    "lds_ns4": ([(256, 8, 8)], 1, 4, 3, 64, "average", False),
    "fix_ns2": ([(256, 8, 9)], 2, 2, 3, 64, "average", False),
    "fix_ns3": ([(256, 8, 9)], 2, 3, 3, 64, "average", False),
    "fix_ns4": ([(256, 8, 9)], 2, 4, 3, 64, "average", False),
    "fix_ns4_max": ([(256, 8, 9)], 2, 4, 3, 64, "max", False),
    "c512_ns3": ([(512, 5, 9)], 2, 3, 3, 64, "average", False),
    "ms4_ns3": (MS4, 2, 3, 2, 128, "average", False),
    "ms4_ns3_uv": (MS4, 2, 3, 2, 128, "average", True),
}
MARGIN_POINTS = (1, 255, 256, 257, 1001)


def margin_case(name, P, lat=None):
    """Inputs of one (case, points per object): dict(spec, poses, maps, xyz, dirs, cot, uvs, route).  The spec, the points
    and the cotangent are test_route_and_block_boundaries_match_fp64's (seed 211 + P, default_rng(P)).  lat: other levels
    for the same points (the route-equivalence test cuts a map along its channels)."""
    lat0, route, NS, SB, d_hidden, combine, uv_image = MARGIN_CASES[name]
    spec = point_spec(lat or lat0, NS=NS, SB=SB, d_hidden=d_hidden, combine_type=combine, image=(128, 128), focal=131.25,
                      seed=211 + P)
    _, poses = gu.make_inputs(dict(spec, N=1))
    xyz, dirs = random_points(spec, P, P)
    cot = np.random.default_rng(P).standard_normal((SB, P, 4)).astype(np.float32)
    uvs = [(w / spec["image"][0], h / spec["image"][1]) for _, h, w in spec["lat"]] if uv_image else None
    return dict(spec=spec, poses=poses, maps=gu.make_latents(spec), xyz=xyz, dirs=dirs, cot=cot, uvs=uvs, route=route)


def _relu_inputs(spec, poses, maps, xyz, dirs, uv_scale, sd, dtype):
    recs = {}
    with torch.no_grad():
        point_forward_oracle(spec, poses, maps, xyz, dirs, uv_scale, sd, dtype,
                             rec=lambda t, name: recs.__setitem__(name, t.detach().to(F64).numpy()))
    return recs


def relu_margin_mask(spec, poses, maps, xyz, dirs, uv_scale=None, sd=None, factor=RELU_MARGIN_FACTOR, info=None):
    """The points whose gradient term is a property of the backward and not of forward rounding, as a (SB, P) bool array of
    points to KEEP; computed from the oracle in fp64 and in fp32 alone, never from a kernel's output.
    Every ReLU input is recorded in both precisions: per block the block input and the fc_0 output, the lin_out input, the
    sigma head.  Row r of a tensor deviates by d_r = max_j |x32_rj - x64_rj|; a unit is at risk when |x64_rj| < factor d_r
    (the one-column sigma head takes d_r from the same row of the lin_out input): an fp32 forward may decide it the other way,
    which moves that point's term of every gradient sum by O(1).  With combine_type "max" a unit of the parked per-view stream
    is at risk as well when its largest and second-largest view lie within factor d_r (the largest d_r of the point's views):
    the argmax may flip and send the gradient to another view.  Rows in front of the view reduction are (object, view, point);
    a point is masked through any of its views.  The caller zeroes a masked point's cotangent row on both sides.
    info: a dict that receives the counts {"relu": points by the ReLU rule, "argmax": points the argmax rule adds}."""
    SB, P, NS = spec["SB"], np.asarray(xyz).shape[1], spec["NS"]
    x64 = _relu_inputs(spec, poses, maps, xyz, dirs, uv_scale, sd, F64)
    x32 = _relu_inputs(spec, poses, maps, xyz, dirs, uv_scale, sd, torch.float32)
    dev = {k: np.abs(x32[k] - x64[k]).max(axis=1) for k in x64}
    bad = np.zeros((SB, P), bool)
    for k, a in x64.items():
        if k == "park":
            continue
        d = dev["lin_out.in"] if k == "sigma" else dev[k]
        risk = (np.abs(a) < factor * d[:, None]).any(axis=1)
        bad |= risk.reshape(SB, NS, P).any(axis=1) if risk.size == SB * NS * P and NS > 1 else risk.reshape(SB, P)
    n_relu = int(bad.sum())
    if spec["combine_type"] == "max" and NS > 1:
        a = np.sort(x64["park"].reshape(SB, NS, P, -1), axis=1)
        d = dev["park"].reshape(SB, NS, P).max(axis=1)
        bad |= ((a[:, -1] - a[:, -2]) < factor * d[..., None]).any(axis=-1)
    if info is not None:
        info.update(relu=n_relu, argmax=int(bad.sum()) - n_relu)
    return ~bad


def mask_points(cot, keep):
    """cot (SB,P,4) with the rows of masked points zeroed (a copy)."""
    out = np.array(cot, dtype=np.float32, copy=True)
    out[~keep] = 0.0
    return out


def latent_scatter(dzx, uv, lat, uv_scale=None):
    """What reaches every latent-map entry, from the d(zx) rows (SB*NS*P, >= L) and the pixel coordinates uv (SB*NS, P, 2)
    of point_grads_fp64(stages=True) / point_forward_oracle's stages, with index_latent's taps in float64: per level
    (sum |g w| (SB*NS, C, H, W), number of contributions with w != 0 (SB*NS, 1, H, W))."""
    uv = np.asarray(uv, np.float64)
    B, P = uv.shape[:2]
    out, c0 = [], 0
    for lvl, (C, H, W) in enumerate(lat):
        s = uv_scale[lvl] if uv_scale else (1.0, 1.0)
        ix, iy = np.clip(uv[..., 0] * s[0], 0, W - 1), np.clip(uv[..., 1] * s[1], 0, H - 1)
        x0, y0 = np.floor(ix), np.floor(iy)
        g = np.abs(np.asarray(dzx, np.float64)[:, c0:c0 + C]).reshape(B, P, C)
        tot, cnt = np.zeros((B, H * W, C)), np.zeros((B, H * W))
        for xx, yy, ww in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                           (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
            live = (xx <= W - 1) & (yy <= H - 1) & (ww != 0)
            idx = np.where(live, yy * W + xx, 0).astype(np.int64)
            for b in range(B):
                np.add.at(tot[b], idx[b][live[b]], g[b][live[b]] * ww[b][live[b]][:, None])
                np.add.at(cnt[b], idx[b][live[b]], 1.0)
        out.append((tot.transpose(0, 2, 1).reshape(B, C, H, W), cnt.reshape(B, 1, H, W)))
        c0 += C
    return out


# ----------------------------------------------------------------------------- comparison
def full_compare(got, truth, rtol, what=""):
    """test_oracle_grad.compare_grads's rule on EVERY entry: per tensor, scale = max(|t| / sqrt(n), max |t|), max error
    <= rtol * scale + 1e-7 and the norm within rtol.  Returns {key: max error / scale}; raises AssertionError naming every
    tensor that fails (a NaN fails)."""
    ratios, bad = {}, []
    for k, t in truth.items():
        assert k in got, f"{what}: no gradient for {k}"
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        g = np.asarray(got[k], dtype=np.float64).reshape(-1)
        assert g.shape == t.shape, (what, k, g.shape, t.shape)
        nt = float(np.linalg.norm(t))
        scale = max(nt / np.sqrt(max(t.size, 1)), float(np.abs(t).max()) if t.size else 0.0)
        err = float(np.abs(g - t).max()) if t.size else 0.0
        ratios[k] = err / scale if scale > 0 else err
        ok = err <= rtol * scale + 1e-7 and abs(float(np.linalg.norm(g)) - nt) <= rtol * nt + 1e-7
        if not ok:
            bad.append(f"{k}: max err {err:.3e} vs scale {scale:.3e}, norm {np.linalg.norm(g):.6e} vs {nt:.6e}")
    assert not bad, f"{what}: " + "; ".join(bad)
    return ratios


def entry_ratios(got, truth):
    """{key: max |got - truth| / scale} with full_compare's scale, without asserting (reports)."""
    out = {}
    for k, t in truth.items():
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        g = np.asarray(got[k], dtype=np.float64).reshape(-1)
        scale = max(float(np.linalg.norm(t)) / np.sqrt(max(t.size, 1)), float(np.abs(t).max()) if t.size else 0.0)
        err = float(np.abs(g - t).max()) if t.size else 0.0
        out[k] = err / scale if scale > 0 else err
    return out


def rel_l2(got, truth):
    """{key: |got - truth| / |truth|} (l2 over the whole tensor)."""
    out = {}
    for k, t in truth.items():
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        g = np.asarray(got[k], dtype=np.float64).reshape(-1)
        nt = float(np.linalg.norm(t))
        out[k] = float(np.linalg.norm(g - t)) / nt if nt > 0 else float(np.linalg.norm(g))
    return out


L2_REF32_FACTOR = 4.0       # measured: at most 3.04x (the dtu case's coarse lin_in, disparity sampling from z = 0.1)


def l2_compare(got, truth, rtol, what="", ref32=None):
    """The rule for gradients that sum many points through ReLUs: per tensor, |got - truth| / |truth| (l2) <= rtol, or, given
    ref32 (the same step through the oracle restatement in fp32, a correct fp32 implementation), <= L2_REF32_FACTOR times
    that restatement's own l2 distance from fp64 where that is larger.
    Why not every entry: an fp32 forward decides a ReLU whose input lies within rounding of 0 differently from fp64, and each
    such unit moves one point's term in a sum over ~1e4 points by O(1) — a few 1e-3 … 1e-2 of a tensor's largest entry, in
    the fp32 restatement as much as in the kernels, and at the training schedule every ray has such units.  The l2 error
    averages those isolated terms; a dropped block, a misrouted tie or a wrong fixed-point scale moves it by far more
    (tests/test_train_fp64_cpu.py).  Returns {key: relative l2}; raises AssertionError naming every tensor that fails."""
    ours = rel_l2(got, truth)
    ref = rel_l2(ref32, truth) if ref32 is not None else {}
    bad = []
    for k, r in ours.items():
        lim = max(rtol, L2_REF32_FACTOR * ref.get(k, 0.0))
        if not r <= lim:
            bad.append(f"{k}: relative l2 {r:.3e} > {lim:.3e}" + (f" (fp32 restatement {ref[k]:.3e})" if k in ref else ""))
    assert not bad, f"{what}: " + "; ".join(bad)
    return ours


def group_worst(ratios):
    """{group: worst ratio} over coarse.* / fine.* / latent.* (the PR's table)."""
    out = {}
    for k, r in ratios.items():
        g = k.split(".")[0]
        out[g] = max(out.get(g, 0.0), r)
    return out


# ----------------------------------------------------------------------------- ray mask
def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def ray_mask(zf_hip, zf64, depth_hip, depth64, zd_raw64, z_other64, near, far, lindisp):
    """Rays whose fine-pass gradient is not a property of the backward, as a (n_rays,) bool array of rays to KEEP.
      (a) a slot of the HIP fine z differs from the fp64 one by more than 1e-4 (far - near) (1/z and 1/near - 1/far for
          lindisp): an importance sample changed bin;
      (b) a depth-guided sample lies within tol = 4 |d depth| + 4 ulp(z) of a coarse or importance sample, or its unclamped
          value lies within tol of near / far (where the clamp starts): d depth = HIP - fp64 coarse depth of the ray, enough
          to swap the two in the sort.  A sample clamped by more than tol sits on the bound on both sides (gradient 0).
    zf_* (n, Kt), depth_* (n,), zd_raw64 (n, Kfd) depth + g std before the clamp, z_other64 (n, Kc + Kf - Kfd)."""
    zf_hip, zf64 = np.asarray(zf_hip, np.float64), np.asarray(zf64, np.float64)
    near, far = np.asarray(near, np.float64).reshape(-1), np.asarray(far, np.float64).reshape(-1)
    if lindisp:
        bad_a = (np.abs(1.0 / zf_hip - 1.0 / zf64) > (1e-4 * (1.0 / near - 1.0 / far))[:, None]).any(-1)
    else:
        bad_a = (np.abs(zf_hip - zf64) > (1e-4 * (far - near))[:, None]).any(-1)
    bad_b = np.zeros_like(bad_a)
    if zd_raw64 is not None and zd_raw64.shape[1] > 0:
        raw = np.asarray(zd_raw64, np.float64)
        dd = np.abs(np.asarray(depth_hip, np.float64) - np.asarray(depth64, np.float64)).reshape(-1)
        zd = np.minimum(np.maximum(raw, near[:, None]), far[:, None])
        tol = 4.0 * dd[:, None] + 4.0 * _ulp32(zd)
        at_bound = (np.abs(raw - near[:, None]) <= tol) | (np.abs(raw - far[:, None]) <= tol)
        inside = (raw > near[:, None]) & (raw < far[:, None]) & ~at_bound
        gap = np.abs(zd[:, :, None] - np.asarray(z_other64, np.float64)[:, None, :]).min(-1)      # (n, Kfd)
        bad_b = (at_bound | (inside & (gap <= tol))).any(-1)
    return ~(bad_a | bad_b)


def step_ray_mask(spec, rays, noise, out64, zf_hip, depth_c_hip):
    """ray_mask for one rendered batch: the fp64 sample positions recomputed from out64 (oracle.render's outputs)."""
    r = torch.as_tensor(np.asarray(rays)).to(F64).reshape(-1, 8)
    n = r.shape[0]
    with torch.no_grad():
        zc = out64["coarse"]["z"].detach()
        w = out64["coarse"]["weights"].detach().reshape(n, -1)
        d64 = out64["coarse"]["depth"].detach().reshape(-1)
        others = [zc]
        if spec["Kf"] - spec["Kfd"] > 0:
            others.append(orc.sample_fine(r, w, spec["Kc"], spec["lindisp"], noise["u"].to(F64), noise["r"].to(F64)))
        raw = (d64[:, None] + noise["g"].to(F64) * spec["depth_std"]) if spec["Kfd"] > 0 else None
    return ray_mask(np.asarray(zf_hip).reshape(n, -1), out64["fine"]["z"].detach().numpy(), np.asarray(depth_c_hip).reshape(-1),
                    d64.numpy(), None if raw is None else raw.numpy(), torch.cat(others, -1).numpy(), r[:, 6].numpy(),
                    r[:, 7].numpy(), spec["lindisp"]).reshape(spec["SB"], spec["N"])


def depth_grad_ok(got, truth, terms):
    """d(depth) of the depth-sample backward within 1e-6 sum|terms| (+1e-12) of the truth, per ray."""
    return bool(((torch.as_tensor(got, dtype=F64) - torch.as_tensor(truth, dtype=F64)).abs()
                 <= 1e-6 * torch.as_tensor(terms, dtype=F64) + 1e-12).all())


# ----------------------------------------------------------------------------- fixed point (k_latq_scale's formula)
def latq_scale_bits(max_abs, n_terms):
    """k_latq_scale: s = 61 - ex - ceil(log2(n_terms)), max|g| < 2^ex (frexp), clamped to +-1000."""
    ex = int(np.frexp(np.float32(max_abs))[1]) if max_abs > 0 else 0
    lg = 0
    while (1 << lg) < n_terms and lg < 62:
        lg += 1
    return int(min(1000, max(-1000, 61 - ex - lg)))


def fixed_point_sum(contrib, index, n_out, scale_bits):
    """The fixed-point route in numpy: each fp32 contribution rounded to an integer multiple of 2^-s, summed exactly, scaled
    back.  contrib (m,) fp32 products, index (m,) their map entries."""
    q = np.rint(np.asarray(contrib, np.float64) * 2.0 ** scale_bits).astype(np.int64)
    acc = np.zeros(n_out, np.int64)
    np.add.at(acc, index, q)
    return acc.astype(np.float64) * 2.0 ** -scale_bits


# ----------------------------------------------------------------------------- exact-geometry lattice
def lattice_c2w():
    """A camera-to-world with entries 0 / +-1 (so rot3 is exact): 90 degrees about z, at (1, -1, 3), looking down -z."""
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    m[:3, 3] = np.array([1, -1, 3], np.float32)
    return m


LATTICE_FOCAL = 2.0
LATTICE_IMAGE = (8, 4)          # c = (4, 2)


def lattice_points(W, H, image=LATTICE_IMAGE, scale=(1.0, 1.0)):
    """World points whose texel coordinate on a (W, H) map is a planned value: (xyz (P,3) fp32, planned (P,2) texel
    coordinates, NaN for points behind the camera).  The camera is lattice_c2w, focal 2, the image centre c; every point sits
    at z_cam = -2 so u = x_cam + cx, v = cy - y_cam; `scale` = the per-axis uv scale of encoder.uv_scale = "image"."""
    cx, cy = image[0] * 0.5, image[1] * 0.5
    tx = [0.5, 1.5, W - 1.5] + [float(i) for i in range(W)] + [-0.5, W - 0.5, -40.0, W + 40.0, 0.25, W - 1.25]
    ty = [0.5, H - 1.5] + [float(j) for j in range(H)] + [-0.5, H - 0.5, -30.0, H + 30.0, 0.75]
    ij = [(a, b) for a in tx for b in ty]
    pts, plan = [], []
    c2w = lattice_c2w().astype(np.float64)
    for a, b in ij:
        u, v = a / scale[0], b / scale[1]
        xc = np.array([(u - cx), (cy - v), -2.0])
        pts.append(c2w[:3, :3] @ xc + c2w[:3, 3])
        plan.append((a, b))
    for xc in ([0.5, 0.25, 2.0], [-1.0, 0.5, 0.5], [0.0, 0.0, 2.0 ** -10]):        # behind the camera
        pts.append(c2w[:3, :3] @ np.array(xc) + c2w[:3, 3])
        plan.append((np.nan, np.nan))
    pts = np.asarray(pts)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts), "lattice points must be exact in fp32"
    return pts.astype(np.float32), np.asarray(plan, np.float64)


def kernel_texel_coords(xyz, c2w, focal, image, W, H, scale=(1.0, 1.0)):
    """float32 numpy in the kernels' order of operations (pnr_common.h: rot3, project, bilinear_taps up to the clip): the
    unclipped texel coordinates (ix, iy) of points xyz (P,3)."""
    f = np.float32
    c2w = np.asarray(c2w, np.float32)
    R = c2w[:3, :3].T.copy()                                           # w2c, as PixelNeRFNet.set_cameras builds it
    t = (-(R.astype(np.float64) @ c2w[:3, 3].astype(np.float64))).astype(np.float32)
    fx, fy, cx, cy = f(focal), f(-focal), f(image[0] * 0.5), f(image[1] * 0.5)
    out = []
    for p in np.asarray(xyz, np.float32):
        xr = [f(f(R[i, 2] * p[2]) + f(f(R[i, 1] * p[1]) + f(R[i, 0] * p[0]))) for i in range(3)]      # fmaf chains, exact here
        xc, yc, zc = f(xr[0] + t[0]), f(xr[1] + t[1]), f(xr[2] + t[2])
        with np.errstate(divide="ignore", invalid="ignore"):
            u = f(f(f(-xc) / zc) * fx) + cx
            v = f(f(f(-yc) / zc) * fy) + cy
        u, v = f(f(u) * f(scale[0])), f(f(v) * f(scale[1]))
        gx = f(f(u / f(W - 1)) * f(2)) - f(1)
        gy = f(f(v / f(H - 1)) * f(2)) - f(1)
        out.append((f(f(f(gx + f(1)) * f(0.5)) * f(W - 1)), f(f(f(gy + f(1)) * f(0.5)) * f(H - 1)), zc))
    return np.asarray(out, np.float64)
