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


def point_grads_fp64(spec, poses, maps_np, xyz, dirs, cot, uv_scale=None, sd=None, stages=False, dtype=F64):
    """The oracle's point_forward at explicit points (SB,P,3) in float64 under autograd with cotangent cot (SB,P,4):
    (out, {coarse.*, latent.*, xyz}) [, d(zx) (SB*NS*P, L + d_in)].  uv_scale: per level (sx, sy) applied to the pixel
    coordinates, as encoder.uv_scale = "image" makes the kernels do."""
    sd = sd if sd is not None else gu.make_mlp_state(spec, "coarse")
    sdo = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in sd.items()}
    lo = [torch.from_numpy(np.asarray(m)).to(dtype).requires_grad_(True) for m in maps_np]
    xo = torch.from_numpy(np.asarray(xyz)).to(dtype).requires_grad_(True)
    orig = orc.index_latent
    if uv_scale:
        def scaled(uv, latents):
            return torch.cat([orig(uv * torch.tensor(s, dtype=uv.dtype), [m]) for s, m in zip(uv_scale, latents)], dim=1)
        orc.index_latent = scaled
    try:
        o, st = orc.point_forward(sdo, fp64_camera(spec, poses, dtype), lo, xo, torch.from_numpy(np.asarray(dirs)).to(dtype), spec["NS"],
                                  use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"],
                                  combine_layer=spec["combine_layer"], combine_type=spec["combine_type"], return_stages=True)
    finally:
        orc.index_latent = orig
    zx = st["mlp_in"]
    zx.retain_grad()
    (o * torch.from_numpy(np.asarray(cot)).to(dtype)).sum().backward()
    g = {f"coarse.{k}": p.grad.numpy() for k, p in sdo.items()}
    g.update({f"latent.{i}": m.grad.numpy() for i, m in enumerate(lo)})
    g["xyz"] = xo.grad.numpy()
    if stages:
        return o.detach().numpy(), g, zx.grad.numpy()
    return o.detach().numpy(), g


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
