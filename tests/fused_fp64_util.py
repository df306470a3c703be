"""Per-point fp64 truth, a generic 16-bit emulation and the comparison rule for the fused kernel k_point_mfma
(tests/test_gpu_fused_fp64.py drives the HIP side, tests/test_fused_fp64_cpu.py checks the inputs and the rule on the CPU).

The fused kernel is not modelled bit for bit.  Its error against float64 is compared with the error of `emulate_16bit`, the
oracle's point_forward restated in float32 with the operand roundings the kernel header documents (the ones
tools/dev/mixed_precision_emul.py applies), with the margins of `class_compare`.  The bound comes from the emulation and
float64 only, never from kernel output.

Geometry: the reference fork's lookup makes the texel coordinate equal to the image-pixel coordinate, and the
full-width fixtures put 64 .. 400-pixel images over 8 x 8 .. 19 x 25 maps, so nearly every fixture point clamps to a border
texel with one tap of weight 1 (test_fused_fp64_cpu.py keeps that measured).  The cases here make the image as large as the
map (`interior_case`), so most points carry four distinct taps with fractional weights, and add an exact-geometry lattice.

No point has z_cam exactly 0: -x / 0 * f + c is NaN for x = 0, and the oracle's lookup and ATen's grid_sampler_2d (which the
kernels follow: fmaxf drops a NaN to the bound) disagree on what a NaN coordinate samples.  Everywhere else the forward map is
continuous, so no point is masked or left out of a comparison.

Nothing here touches a GPU."""
import contextlib

import numpy as np
import torch

import golden_util as gu
import train_fp64_util as tu
from oracle import pixelnerf_oracle as orc

F64 = torch.float64
FMT = {"fp16": torch.float16, "bf16": torch.bfloat16}
TILE = 128                       # points per workgroup tile of k_point_mfma; a wave owns 32 = two 16-column groups


# ----------------------------------------------------------------------------- truth and emulation
@contextlib.contextmanager
def _scaled_lookup(uv_scale):
    """train_fp64_util.point_grads_fp64's uv_scale route: per level (sx, sy) applied to the pixel coordinates."""
    orig = orc.index_latent
    if uv_scale:
        def scaled(uv, latents):
            return torch.cat([orig(uv * torch.tensor(s, dtype=uv.dtype), [m]) for s, m in zip(uv_scale, latents)], dim=1)
        orc.index_latent = scaled
    try:
        yield
    finally:
        orc.index_latent = orig


def _forward(spec, poses, maps, xyz, dirs, dtype, rnd=None, uv_scale=None, coarse=True, sd=None):
    sd = sd if sd is not None else gu.make_mlp_state(spec, "coarse" if coarse else "fine")
    sd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    lat = [torch.from_numpy(np.asarray(m)).to(dtype) for m in maps]
    if rnd is not None:
        lat = [rnd(m, "map") for m in lat]
    with torch.no_grad(), _scaled_lookup(uv_scale):
        o = orc.point_forward(sd, tu.fp64_camera(spec, poses, dtype), lat, torch.from_numpy(np.asarray(xyz)).to(dtype),
                              torch.from_numpy(np.asarray(dirs)).to(dtype), spec["NS"],
                              use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"],
                              combine_layer=spec["combine_layer"], combine_type=spec["combine_type"], rnd=rnd)
    return o.double().numpy()


def truth_fp64(spec, poses, maps, xyz, dirs, uv_scale=None, coarse=True, sd=None):
    """orc.point_forward in float64, no rounding: (SB, P, 4)."""
    return _forward(spec, poses, maps, xyz, dirs, F64, None, uv_scale, coarse, sd)


def rounder(fmt, park16=True, skip=()):
    """The rounding hook of orc.resnetfc / orc.point_forward for a 16-bit format: torch's own casts (round to nearest even).
    Kinds: map (latent maps at pack time), latent (the interpolated latent vector), sine (the 12 D sine features), weight
    (every weight matrix), act (every layer input behind its ReLU), park (the residual stream in front of the view reduction,
    iff park16).  `skip` names kinds left unrounded (a second legitimate rounding placement, test_fused_fp64_cpu.py)."""
    if fmt == "fp32":
        return None
    dt = FMT[fmt]
    off = set(skip) | (set() if park16 else {"park"})

    def rnd(t, kind):
        return t if kind in off else t.to(dt).to(t.dtype)
    return rnd


def emulate_16bit(spec, poses, maps, xyz, dirs, fmt, park16=True, uv_scale=None, coarse=True, skip=(), sd=None):
    """orc.point_forward in float32 with the operand roundings of the fused kernel (csrc/point_mfma.hip's header), fmt in
    {"fp16", "bf16"} ("fp32": the plain float32 restatement).  Latent maps, the interpolated latent vector, the sine
    features, every weight matrix and every layer input behind its ReLU go to fmt; raw coordinates and view dirs (the kernel
    carries hi + lo), biases, the accumulation, sigmoid and relu stay fp32; with several views the residual stream goes to fmt
    in front of the view reduction iff park16 (net.park_precision "16bit" / "fp32")."""
    return _forward(spec, poses, maps, xyz, dirs, torch.float32, rounder(fmt, park16, skip), uv_scale, coarse, sd)


# ----------------------------------------------------------------------------- interior geometry
def uv_scales(spec):
    """Per level (sx, sy) of encoder.uv_scale = "image" (PixelNeRFNet.uv_scales)."""
    W, H = spec["image"]
    return [(w / W, h / H) for _, h, w in spec["lat"]]


BEHIND_EVERY = 97


def interior_spec(lat, image=None, focal=None, **kw):
    """full_ns1 with the image as large as the covered latent level (default: level 0) and the focal scaled by the same
    factor (131.25 / 128 per pixel unless given): texel coordinate = pixel coordinate now runs over the map's interior."""
    lat = [tuple(l) for l in lat]
    W, H = image if image is not None else (lat[0][2], lat[0][1])
    spec = dict(gu.CASES["full_ns1"])
    spec.update(lat=lat, image=(W, H), focal=float(focal) if focal is not None else 131.25 / 128.0 * W,
                use_code_viewdirs=kw.pop("use_code_viewdirs", len(lat) == 4), **kw)
    return spec


def interior_case(lat, NS=1, SB=1, P=TILE * 24 + 17, seed=500, image=None, focal=None, uv_image=False, focal_xy=None, c_xy=None,
                  **kw):
    """An interior_spec, source poses as golden_util.make_inputs places them, and P points per object along target rays at
    random depths — rays drawn WITH replacement (make_inputs is limited to N <= W H).  The target rays never pass behind a
    source camera, so every BEHIND_EVERY-th point (from index 41 on) is put on its ray's direction from source camera 0's
    centre instead, on the side behind that camera, at the same depth.
    focal_xy / c_xy: the source cameras' own intrinsics (golden_util.intrinsics), SB or SB*NS rows.  The target rays keep the
    scalar focal and the image centre.
    Returns dict(spec, poses, maps, xyz (SB,P,3), dirs (SB,P,3), uv_scale)."""
    spec = interior_spec(lat, image, focal, NS=NS, SB=SB, N=P, seed=seed, **kw)
    for key, val in (("focal_xy", focal_xy), ("c_xy", c_xy)):
        if val is not None:
            spec[key] = [[float(a), float(b)] for a, b in val]
    W, H = spec["image"]
    rng = np.random.default_rng(seed * 1000 + 7)
    poses = np.zeros((SB, NS, 4, 4), np.float32)
    xyz = np.zeros((SB, P, 3), np.float32)
    dirs = np.zeros((SB, P, 3), np.float32)
    for sb in range(SB):
        for v in range(NS):
            poses[sb, v] = gu.pose_spherical(30.0 * v + 11.0 * sb, -20.0, spec["radius"])
        tgt = gu.pose_spherical(75.0 + 5.0 * sb, -25.0, spec["radius"])
        r = gu.pinhole_rays(tgt, W, H, spec["focal"], spec["z_near"], spec["z_far"], rng.integers(0, W * H, size=P))
        z = rng.uniform(spec["z_near"], spec["z_far"], size=(P, 1)).astype(np.float32)
        xyz[sb] = r[:, :3] + z * r[:, 3:6]
        dirs[sb] = r[:, 3:6]
        b = np.arange(41, P, BEHIND_EVERY)
        c2w = poses[sb, 0]
        side = np.where(r[b, 3:6] @ c2w[:3, 2] >= 0, 1.0, -1.0).astype(np.float32)       # z_cam = (x - C) . c2w[:, 2] > 0
        xyz[sb, b] = c2w[:3, 3] + z[b] * side[:, None] * r[b, 3:6]
    return dict(spec=spec, poses=poses, maps=gu.make_latents(spec), xyz=xyz, dirs=dirs,
                uv_scale=uv_scales(spec) if uv_image else None)


def rays_case(lat, n_rays, K, seed=520, NS=1, focal_xy=None, c_xy=None):
    """Rays-mode input (pnr_point_mlp with rays and z): n_rays rays drawn with replacement, K random depths per ray.  The
    points are o + z d of the FP32 inputs, formed in float64 (what the kernel is asked to evaluate) and handed to truth and
    emulation as they are."""
    case = interior_case(lat, NS=NS, P=n_rays, seed=seed, focal_xy=focal_xy, c_xy=c_xy)
    spec = case["spec"]
    W, H = spec["image"]
    rng = np.random.default_rng(seed * 1000 + 8)
    tgt = gu.pose_spherical(75.0, -25.0, spec["radius"])
    rays = gu.pinhole_rays(tgt, W, H, spec["focal"], spec["z_near"], spec["z_far"], rng.integers(0, W * H, size=n_rays))
    z = np.sort(rng.uniform(spec["z_near"], spec["z_far"], size=(n_rays, K)).astype(np.float32), axis=1)
    xyz = (rays[:, None, :3].astype(np.float64) + z[..., None].astype(np.float64) * rays[:, None, 3:6].astype(np.float64))
    dirs = np.broadcast_to(rays[:, None, 3:6], (n_rays, K, 3))
    case.update(rays=rays, z=z, xyz=xyz.reshape(1, -1, 3), dirs=np.ascontiguousarray(dirs).reshape(1, -1, 3))
    return case


def covered_level(spec, uv_scale=None):
    """The level the case's image covers: the last one under the image mapping (every level spans the image) or on a
    single-level map, else the first level as large as the image."""
    if uv_scale is None:
        for i, (_, h, w) in enumerate(spec["lat"]):
            if (w, h) == tuple(spec["image"]):
                return i
    return len(spec["lat"]) - 1


def texel_coords(spec, poses, xyz, level, uv_scale=None):
    """float64 texel coordinates on `level`: (ix, iy, z_cam), each (SB, NS, P).  The fork's lookup normalises by the latent
    size and unnormalises again: texel coordinate = (scaled) pixel coordinate."""
    f, c = gu.view_intrinsics(spec)                                        # (SB, NS, 2) each: the case's own, per view
    c2w = np.asarray(poses, np.float64)
    R = np.swapaxes(c2w[..., :3, :3], -1, -2)                              # (SB, NS, 3, 3) world -> camera
    t = -np.einsum("bvij,bvj->bvi", R, c2w[..., :3, 3])
    xc = np.einsum("bvij,bpj->bvpi", R, np.asarray(xyz, np.float64)) + t[:, :, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = -xc[..., 0] / xc[..., 2] * f[:, :, None, 0] + c[:, :, None, 0]
        v = -xc[..., 1] / xc[..., 2] * -f[:, :, None, 1] + c[:, :, None, 1]
    sx, sy = uv_scale[level] if uv_scale else (1.0, 1.0)
    return u * sx, v * sy, xc[..., 2]


TAP_CLASSES = ("interior", "clamped_x", "clamped_y", "clamped_xy", "behind")


def tap_class(spec, poses, xyz, level=None, uv_scale=None):
    """(SB, NS, P) index into TAP_CLASSES on `level` (default: covered_level): behind the camera (z_cam >= 0; the cameras look
    down -z), else by which texel coordinate leaves the open range (0, W-1) x (0, H-1)."""
    level = covered_level(spec, uv_scale) if level is None else level
    _, h, w = spec["lat"][level]
    ix, iy, zc = texel_coords(spec, poses, xyz, level, uv_scale)
    cx = ~((ix > 0) & (ix < w - 1))
    cy = ~((iy > 0) & (iy < h - 1))
    cls = cx.astype(np.int64) + 2 * cy.astype(np.int64)
    cls[zc >= 0] = 4
    return cls


def interior_fraction(spec, poses, xyz, level=None, uv_scale=None):
    """Fraction of (view, point) pairs strictly inside `level`'s texel range, in front of the camera."""
    return float((tap_class(spec, poses, xyz, level, uv_scale) == 0).mean())


def four_tap_fraction(spec, poses, xyz, level=None, uv_scale=None, lo=0.05, hi=0.95):
    """Fraction of (view, point) pairs that are interior AND have all four bilinear weights in (lo, hi)."""
    level = covered_level(spec, uv_scale) if level is None else level
    ix, iy, _ = texel_coords(spec, poses, xyz, level, uv_scale)
    inside = tap_class(spec, poses, xyz, level, uv_scale) == 0
    with np.errstate(invalid="ignore"):
        fx, fy = ix - np.floor(ix), iy - np.floor(iy)
        w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy])
        ok = ((w > lo) & (w < hi)).all(0)
    return float((inside & ok).mean())


def point_classes(spec, poses, xyz, per_object_tiles=False, level=None, uv_scale=None):
    """{name: (SB*P,) integer labels} of the classes class_compare looks at.  i = the point's index in the kernel's tiling:
    the flat index of the call (a tile may cross objects: the general stream, one object) or the index inside its object
    (per_object_tiles: the projected stream assigns workgroups per object).  tile row i % 128, wave (i % 128) // 32, column
    group (i % 32) // 16, tile (the tail tile is its own class, like every tile), object, and per source view the tap class."""
    xyz = np.asarray(xyz)
    SB, P = xyz.shape[:2]
    gi = np.arange(SB * P)
    ob = gi // P
    i = gi % P if per_object_tiles else gi
    tiles = (P + TILE - 1) // TILE
    cls = {"row": i % TILE, "wave": (i % TILE) // 32, "colgroup": (i % 32) // 16,
           "tile": ob * tiles + i // TILE if per_object_tiles else i // TILE, "object": ob}
    tc = tap_class(spec, poses, xyz, level, uv_scale)
    for v in range(tc.shape[1]):
        cls[f"tap_view{v}"] = tc[:, v].reshape(-1)
    return cls


# ----------------------------------------------------------------------------- the lattice
LATTICE_MAP = (256, 5, 9)
LATTICE_SHIFTS = (0, 60, 61, 178, 192)


def lattice_case(seed=540):
    """train_fp64_util's exact-geometry lattice on a (256, 5, 9) map (texel centres, lines and corners, the borders, half a
    texel and far outside, behind the camera) at d_hidden 512, the list repeated once per entry of LATTICE_SHIFTS, rolled by
    that shift: every lattice point sits in several tile rows and in both 16-column groups, and the total is off a 128
    multiple (test_fused_fp64_cpu.py asserts all three).  Returns the case dict plus plan (P,2) and lattice_index (P,)."""
    C, H, W = LATTICE_MAP
    spec = dict(gu.CASES["full_ns1"])
    spec.update(lat=[LATTICE_MAP], image=tu.LATTICE_IMAGE, focal=tu.LATTICE_FOCAL, seed=seed, NS=1, SB=1)
    pts, plan = tu.lattice_points(W, H)
    n = pts.shape[0]
    idx = np.concatenate([np.roll(np.arange(n), s) for s in LATTICE_SHIFTS])
    spec["N"] = idx.size
    xyz = pts[idx][None]
    dirs = np.tile(np.array([[0.0, 0.6, -0.8]], np.float32), (1, idx.size, 1))
    return dict(spec=spec, poses=tu.lattice_c2w()[None, None], maps=gu.make_latents(spec), xyz=xyz, dirs=dirs, uv_scale=None,
                plan=plan[idx], lattice_index=idx)


# ----------------------------------------------------------------------------- the rule
RMS_ALL_FACTOR = 2.0        # the kernel adds at most one rounding step (the tap weights, or the projected W_z . Lat) to a chain
                            # of about a dozen equal-sized ones: sqrt(13 / 12) of the emulation's rms, and a second legitimate
                            # rounding placement measures 1.0 - 1.6 x (test_fused_fp64_cpu.py); 2 x covers both
CLASS_FACTOR = 4.0          # the project's factor over a restatement's own distance from fp64 (train_fp64_util.L2_REF32_FACTOR,
                            # test_point_mlp_fp32_matches_reference); also covers the 1.3 - 1.6 x sampling spread of a 24-point class
MIN_CLASS = 16
GROUPS = {"rgb": slice(0, 3), "sigma": slice(3, 4)}


def _rms(e):
    return float(np.sqrt(np.mean(np.square(e)))) if e.size else 0.0


def class_compare(got, truth, emu, classes, every_point=False, emu_ref=None, what="", check=True):
    """got, truth, emu: (..., 4) outputs of the kernel, float64 and the emulation on the same points; err = x - truth.  For
    the groups rgb and sigma separately:
      * every output is finite;
      * rms_all(got) <= 2 rms_all(emu);          * max |got| <= 4 max |emu|;
      * for every class of >= 16 points: rms_class(got) <= 4 rms_all(emu);
      * for every point of a smaller class, and for every point at all with every_point (the lattice): |err| <= 4 max |emu|.
    emu_ref = (truth, emu) of a larger population the points are a prefix of: its rms_all(emu) and max |emu| take the place of
    the call's own — for calls of a handful of points, whose own emulation error is one draw and no level.  A call of fewer
    than 16 points is itself a small class: the per-point bound holds in place of the rms_all one.
    No point is masked.  Returns {group: {rms_all, max, rms_class, point}}: each the worst got figure over its emulation
    figure (the margins not applied); raises AssertionError naming everything that fails (check=False: reports only)."""
    got, truth, emu = (np.asarray(t, np.float64).reshape(-1, 4) for t in (got, truth, emu))
    assert got.shape == truth.shape == emu.shape, (what, got.shape, truth.shape, emu.shape)
    n = got.shape[0]
    ref_t, ref_e = (truth, emu) if emu_ref is None else (np.asarray(t, np.float64).reshape(-1, 4) for t in emu_ref)
    bad, ratios = [], {}
    if not np.isfinite(got).all():
        bad.append(f"{int((~np.isfinite(got)).sum())} non-finite outputs")
    for grp, sl in GROUPS.items():
        e_got, e_emu = got[:, sl] - truth[:, sl], ref_e[:, sl] - ref_t[:, sl]
        rms_emu, max_emu = _rms(e_emu), float(np.abs(e_emu).max())
        assert rms_emu > 0 and max_emu > 0, (what, grp, "the emulation is exact: no bound")
        r = dict(rms_all=_rms(e_got) / rms_emu, max=float(np.abs(e_got).max()) / max_emu, rms_class=0.0, point=0.0)
        if n >= MIN_CLASS and not r["rms_all"] <= RMS_ALL_FACTOR:
            bad.append(f"{grp}: rms_all {r['rms_all']:.2f} x the emulation's {rms_emu:.3e}")
        if not r["max"] <= CLASS_FACTOR:
            bad.append(f"{grp}: max {r['max']:.2f} x the emulation's {max_emu:.3e}")
        pt = np.abs(e_got).max(axis=1) / max_emu                                  # per point
        small = np.full(n, every_point or n < MIN_CLASS)
        for name, lab in classes.items():
            lab = np.asarray(lab).reshape(-1)
            assert lab.shape[0] == n, (what, name, lab.shape, n)
            for k in np.unique(lab):
                m = lab == k
                if m.sum() >= MIN_CLASS:
                    rc = _rms(e_got[m]) / rms_emu
                    r["rms_class"] = max(r["rms_class"], rc)
                    if not rc <= CLASS_FACTOR:
                        bad.append(f"{grp}: class {name}={k} ({int(m.sum())} points) rms {rc:.2f} x the emulation's rms_all")
                else:
                    small |= m
        if small.any():
            r["point"] = float(pt[small].max())
            for i in np.nonzero(small & ~(pt <= CLASS_FACTOR))[0][:8]:
                bad.append(f"{grp}: point {i} |err| {pt[i]:.2f} x the emulation's max")
        ratios[grp] = r
    assert not (bad and check), f"{what}: " + "; ".join(bad[:24]) + (f" (+{len(bad) - 24} more)" if len(bad) > 24 else "")
    return ratios


def ratio_line(what, frac, ratios):
    """One report line: case, interior fraction (None: left out), the four worst ratios (over rgb and sigma)."""
    w = {k: max(r[k] for r in ratios.values()) for k in ("rms_all", "max", "rms_class", "point")}
    return (f"{what}: " + ("" if frac is None else f"interior {frac:.2f}  ") + f"rms_all {w['rms_all']:.2f}  max {w['max']:.2f}  rms_class {w['rms_class']:.2f}  "
            f"point {w['point']:.2f}")


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_fused_fp64.py
MS4 = [(64, 16, 16), (64, 16, 16), (128, 8, 8), (256, 4, 4)]           # test_gpu_parity._SHAPES' 4-level row: d_latent 512
P_FULL = TILE * 24 + 17
P_SWEEP = (1, 127, 128, 129, P_FULL)


def _c(stream, proj=True, park="16bit", coarse=True, **kw):
    return dict(stream=stream, proj=proj, park=park, coarse=coarse, make=kw)


# name -> dict(make = interior_case's arguments, proj = net.project_latent, stream = the stream the kernel must then run
# ("proj": lin_z pre-multiplied with the last level, the tap-weight image; "general": gather + lin_z; None: not checked), park =
# net.park_precision, coarse = which MLP)
INTERIOR_CASES = {
    "8x8_ns1_proj": _c("proj", lat=[(256, 8, 8)], seed=501),
    "8x8_ns1_general": _c("general", proj=False, lat=[(256, 8, 8)], seed=501),
    "8x8_ns1_fine_mlp": _c("proj", coarse=False, lat=[(256, 8, 8)], seed=501),
    "8x8_ns3_average_park16": _c("proj", lat=[(256, 8, 8)], NS=3, seed=502),
    "8x8_ns3_average_park32": _c("proj", park="fp32", lat=[(256, 8, 8)], NS=3, seed=502),
    "8x8_ns3_max_park16": _c("proj", lat=[(256, 8, 8)], NS=3, seed=503, combine_type="max"),
    "8x8_ns3_max_park32": _c("proj", park="fp32", lat=[(256, 8, 8)], NS=3, seed=503, combine_type="max"),
    "8x8_ns3_general_park16": _c("general", proj=False, lat=[(256, 8, 8)], NS=3, seed=502),
    "8x8_ns2_codeview": _c("proj", lat=[(256, 8, 8)], NS=2, seed=504, use_code_viewdirs=True),
    "19x25_ns3": _c("general", lat=[(256, 19, 25)], NS=3, seed=505, focal=22.5),                  # 475 texels: too large to project
    "5x7": _c("proj", lat=[(256, 5, 7)], seed=506),                                              # 35 texels: a padded k-step
    "multiscale_default": _c("proj", lat=MS4, seed=507, n_blocks=4, combine_layer=2),
    "multiscale_uv_image": _c("proj", lat=MS4, seed=507, n_blocks=4, combine_layer=2, uv_image=True),
    "d768_two_groups_uv_image": _c("proj", lat=[(512, 8, 8), (256, 4, 4)], NS=2, seed=508, uv_image=True),
    "d768_three_groups": _c("general", lat=[(256, 8, 8), (256, 8, 8), (256, 19, 25)], NS=2, seed=509),
    "d1024": _c("general", proj=False, lat=[(256, 8, 8)] * 4, seed=510, n_blocks=3, combine_layer=2),
    "blocks5_combine0": _c(None, lat=[(256, 8, 8)], seed=511, n_blocks=5, combine_layer=0),      # no lin_z: either stream
    "blocks5_combine5_proj": _c("proj", lat=[(256, 8, 8)], seed=512, n_blocks=5, combine_layer=5),
    "blocks5_combine5_general": _c("general", proj=False, lat=[(256, 8, 8)], seed=512, n_blocks=5, combine_layer=5),
    "blocks8_combine3_ns3_proj": _c("proj", lat=[(256, 6, 6)], NS=3, seed=513, n_blocks=8, combine_layer=3),
    "blocks8_combine3_ns3_general": _c("general", proj=False, lat=[(256, 6, 6)], NS=3, seed=513, n_blocks=8, combine_layer=3),
    "sb3_proj": _c("proj", lat=[(256, 8, 8)], SB=3, P=1000, seed=514),                           # workgroups per object
    "sb3_general": _c("general", proj=False, lat=[(256, 8, 8)], SB=3, P=1000, seed=514),         # a tile crosses objects
}


def make_case(name):
    return interior_case(**INTERIOR_CASES[name]["make"])


# ----------------------------------------------------------------------------- per-view intrinsics (tests/test_gpu_intrinsics.py)
F8 = 131.25 / 128.0 * 8                      # interior_spec's scalar focal on an 8 x 8 map
INTR_F_ROWS = gu.INTR_F_ROWS + [[1.13, 0.93], [0.95, 1.18]]          # fx != fy, every row another pair
INTR_C_ROWS = gu.INTR_C_ROWS + [[+0.4, +0.5], [-0.35, -0.6]]         # off the centre (4, 4), every row another offset


def intr_rows(n, first=0):
    """focal_xy / c_xy of n rows (from row `first` of the tables) on the 8 x 8 interior geometry."""
    return gu.scaled_intrinsics(F8, (8, 8), INTR_F_ROWS[first:first + n], INTR_C_ROWS[first:first + n])


_L8 = [(256, 8, 8)]
# fused kernel: _c's fields as in INTERIOR_CASES.  One object of one view is the scalar-cache load_cam branch (n_objs == 1); three
# views carry one row per VIEW; three objects of two views carry one row per OBJECT, which the host repeats per view, with P off a
# tile multiple (per-object projected streams; on the general stream a tile straddles two objects and view_of picks per lane)
INTR_FUSED_CASES = {
    "sb1_ns1_proj": _c("proj", lat=_L8, seed=561, **intr_rows(1)),
    "sb1_ns1_general": _c("general", proj=False, lat=_L8, seed=561, **intr_rows(1)),
    "sb1_ns3_per_view_mean": _c("proj", lat=_L8, NS=3, seed=562, **intr_rows(3)),
    "sb1_ns3_per_view_max": _c("proj", lat=_L8, NS=3, seed=563, combine_type="max", **intr_rows(3)),
    "sb3_ns2_per_object_proj": _c("proj", lat=_L8, SB=3, NS=2, P=1000, seed=564, **intr_rows(3)),
    "sb3_ns2_per_object_general": _c("general", proj=False, lat=_L8, SB=3, NS=2, P=1000, seed=564, **intr_rows(3)),
}
# training backward at explicit points (k_features_bwd, k_latent_grad_lds): two objects of two views, one row per object
INTR_TRAIN = dict(lat=_L8, SB=2, NS=2, P=700, seed=581, d_hidden=64, **intr_rows(2))
INTR_RAYS = dict(lat=_L8, n_rays=83, K=37, seed=565, NS=2, **intr_rows(2))       # rays mode: one object, a row per view


def intr_case(name):
    return rays_case(**INTR_RAYS) if name == "rays_sb1_ns2" else interior_case(**INTR_FUSED_CASES[name]["make"])


def _rows_of(spec):
    """(focal rows (n, 2), c rows (m, 2)) of a spec as float arrays, the defaults written out as one row."""
    W, H = spec["image"]
    focal, c = gu.intrinsics(spec)
    f = np.full((1, 2), float(focal)) if np.ndim(focal) == 0 else np.asarray(focal, np.float64)
    return f, (np.array([[W * 0.5, H * 0.5]]) if c is None else np.asarray(c, np.float64))


def intrinsics_mutants(spec):
    """{name: spec with deliberately wrong source intrinsics}: the mistakes a kernel or the host layer can make with (fx, fy),
    (cx, cy) and the row a view reads.  A mutant that leaves this spec's intrinsics as they are (one row cannot be given to
    the wrong object; a scalar focal has no axes to swap) is left out: it is no mistake on that case."""
    f, c = _rows_of(spec)
    W, H = spec["image"]
    centre = np.array([[W * 0.5, H * 0.5]])
    m = {
        "fy := fx": (f[:, [0, 0]], c), "fx <-> fy": (f[:, ::-1], c),
        "c := centre": (f, np.broadcast_to(centre, c.shape)), "cx <-> cy": (f, c[:, ::-1]),
        "row 0 for every row": (np.broadcast_to(f[:1], f.shape), np.broadcast_to(c[:1], c.shape)),
        "rows rolled by one": (np.roll(f, 1, axis=0), np.roll(c, 1, axis=0)),
        "only focal broadcast": (np.broadcast_to(f[:1], f.shape), c), "only c broadcast": (f, np.broadcast_to(c[:1], c.shape)),
    }
    out = {}
    for name, (mf, mc) in m.items():
        if not (np.array_equal(mf, f) and np.array_equal(mc, c)):
            out[name] = dict(spec, **({} if np.array_equal(mf, f) else dict(focal_xy=np.asarray(mf).tolist())),
                             **({} if np.array_equal(mc, c) else dict(c_xy=np.asarray(mc).tolist())))
    return out


MUTANT_FACTOR = 5.0          # a mutant must move the fp64 truth's rgb by 5 x what class_compare accepts for bf16 (2 x emulation rms)
