"""The fp32 point path (point_f32, k_features_f32, chain_f32, k_combine_f32, k_out_act in csrc/point_f32.hip and
csrc/f32_kernels.h) point by point against float64: the cases, the classes and the comparison rule
(tests/test_gpu_point_f32_fp64.py drives the HIP side, tests/test_point_f32_cpu.py checks cases and rule on the CPU).

Geometry, truth and the restatement are fused_fp64_util's: interior_case puts the points inside the maps with four live taps,
truth_fp64 is the oracle's point_forward in float64, emulate_16bit(fmt="fp32") the same function in float32.

Why fused_fp64_util.class_compare is not the rule here.  It holds a kernel to ONE emulation's rms over all points, which
works for a 16-bit format: rounding O(1) activations to 8 or 11 bits gives every class of points about the same error.  An
fp32 evaluation's error follows the size of its intermediates instead — the restatement's own "behind the camera" class has
2.5 - 2.8 x its all-points rms on rgb, single tile rows reach 8.9 x on sigma — and a second legitimate fp32 evaluation (the
same GEMMs summed in another order) scores up to 9.5 x under class_compare's class bound of 4.  So the unit of every bound
here is taken from an ENSEMBLE of fp32 restatements that differ only in the order the GEMMs sum over k (fp32_ensemble), and a
class is held to the larger of the ensemble's rms in that same class and its rms over all points.  sigma is a ReLU output:
where it is 0 in float64 every evaluation's error is exactly 0, so a case must have sigma > 0 on at least half of its points
(sigma_positive_fraction) or its sigma statistics are a handful of draws.

Nothing here touches a GPU."""
import contextlib
import os
import re

import numpy as np
import torch

import fused_fp64_util as fu
import train_fp64_util as tu

HERE = os.path.dirname(os.path.abspath(__file__))
POINT_F32_SOURCE = os.path.join(HERE, "..", "pixel_nerf_multiscale_amd", "csrc", "point_f32.hip")

CHUNK = 49152                    # F32_CHUNK of csrc/point_f32.hip: points per pass of point_f32 / resnetfc_f32
CL_POINTS = 4096                 # point_f32 builds the channels-last copies of the maps from this many points of a call on
GEMM_TILE = 128                  # rows per workgroup tile of linear_f32_mfma (csrc/train_f32.hip)
FACTOR = tu.L2_REF32_FACTOR      # the project's factor over a restatement's own distance from fp64
MIN_CLASS = fu.MIN_CLASS
MIN_INTERIOR, MIN_FOUR_TAP, MIN_SIGMA_POSITIVE = 0.6, 0.3, 0.5


def source_constants(path=POINT_F32_SOURCE):
    """(F32_CHUNK, the n_points threshold of the channels-last route) as csrc/point_f32.hip states them."""
    with open(path) as f:
        src = f.read()
    chunk = re.search(r"static const int F32_CHUNK = (\d+);", src)
    cl = re.search(r"n_points >= (\d+)\) \? latent_cl_build", src)
    assert chunk and cl, "csrc/point_f32.hip no longer states F32_CHUNK / the channels-last threshold in the form read here"
    return int(chunk.group(1)), int(cl.group(1))


# ----------------------------------------------------------------------------- the ensemble
@contextlib.contextmanager
def summation_order(block=None, reverse=False):
    """Inside: torch.addmm(b, x, w) sums over k in blocks of `block` columns, first to last or last to first, the blocks' partial
    products added one after the other and the bias last.  block=None: torch.addmm as it is."""
    if block is None:
        yield
        return
    orig = torch.addmm

    def addmm(bias, x, wt):
        starts = list(range(0, x.shape[1], block))
        acc = None
        for k0 in (reversed(starts) if reverse else starts):
            part = torch.mm(x[:, k0:k0 + block], wt[k0:k0 + block])
            acc = part if acc is None else acc + part
        return acc + bias
    torch.addmm = addmm
    try:
        yield
    finally:
        torch.addmm = orig


# torch's own order, and three blocked ones.  Blocks of 8 stand for long chains of short partial sums, the shape of the fp32 MFMA
# GEMM's accumulation (k in steps of 2 into one accumulator): without a member of that kind torch's own order, held against
# blocks of 16 and 32 alone, scores up to 2.0 of the bound's 4 on the 512-wide cases, with it at most 1.8.
ORDERS = {"default": dict(), "k8": dict(block=8), "k16": dict(block=16), "k32_reversed": dict(block=32, reverse=True)}


def case_args(case, P=None):
    return case["spec"], case["poses"], case["maps"], case["xyz"][:, :P], case["dirs"][:, :P]


def restate_f32(case, order="default", coarse=True, **over):
    """The oracle's point_forward in float32 on the case's points with one of ORDERS; `over` replaces entries of the case
    (poses, maps, xyz, dirs) for a planted defect."""
    c = dict(case, **over)
    with summation_order(**ORDERS[order]):
        return fu.emulate_16bit(*case_args(c), "fp32", uv_scale=case["uv_scale"], coarse=coarse)


def fp32_ensemble(case, coarse=True):
    """(truth, {order: error}): the float64 truth (SB, P, 4) and, per entry of ORDERS, the error against it of the fp32
    restatement summed in that order."""
    truth = fu.truth_fp64(*case_args(case), uv_scale=case["uv_scale"], coarse=coarse)
    return truth, {name: restate_f32(case, name, coarse) - truth for name in ORDERS}


def sigma_positive_fraction(truth):
    return float((np.asarray(truth)[..., 3] > 0).mean())


# ----------------------------------------------------------------------------- classes
def f32_classes(case, P=None, chunk=CHUNK):
    """fused_fp64_util.point_classes on the call's flat point index g (tile row, wave, column group, 128-point tile, object,
    tap class per view) plus what point_f32 adds: the chunk g // 49152, and per source view v >= 1 the 128-row GEMM tile
    that holds the point's row v CH + g % 49152 of its chunk (CH = the chunk's own length: a tail chunk moves every later
    view's rows).  point_classes' "tile", g // 128, IS view 0's GEMM tile inside the chunk, the chunk being a multiple of 128;
    tile ids are unique over the call, so a tail tile is a class of its own."""
    spec, poses, xyz = case["spec"], case["poses"], np.asarray(case["xyz"])[:, :P]
    cls = fu.point_classes(spec, poses, xyz, uv_scale=case["uv_scale"])
    n = xyz.shape[0] * xyz.shape[1]
    g = np.arange(n)
    ck = g // chunk
    cls["chunk"] = ck
    CH = np.minimum(chunk, n - ck * chunk)
    tiles = (chunk * spec["NS"]) // GEMM_TILE + 1
    for v in range(1, spec["NS"]):
        cls[f"gemm_tile_view{v}"] = ck * tiles + (v * CH + g % chunk) // GEMM_TILE
    return cls


# ----------------------------------------------------------------------------- the rule
def _rms(e):
    return float(np.sqrt(np.mean(np.square(e)))) if e.size else 0.0


def _by_class(sq, inv, cnt, width):
    """rms per class from per-point sums of squares over `width` components."""
    return np.sqrt(np.bincount(inv, weights=sq, minlength=cnt.size) / (cnt * width))


def f32_compare(got, truth, errs, classes, every_point=False, what="", check=True):
    """got, truth (..., 4); errs = the ensemble's errors against truth ({order: (..., 4)} or a list).  err = got - truth.  For
    the groups rgb and sigma separately, with E_j the ensemble members:
      * every output is finite;
      * rms_all(err) <= 4 max_j rms_all(E_j);
      * max |err| <= 4 max_j max |E_j| — this holds every point: it is the per-point bound;
      * for every class of >= 16 points: rms_class(err) <= 4 max(max_j rms_class(E_j), max_j rms_all(E_j));
      * the points of smaller classes, and every point with every_point (the lattice), are reported against the per-point bound.
    No point is masked; every bound is formed from float64 and the ensemble.  Returns {group: {rms_all, max, rms_class,
    point}}: each the worst figure of `got` over its unit (the factor 4 not applied); raises AssertionError naming everything
    that fails (check=False: reports only)."""
    got, truth = (np.asarray(t, np.float64).reshape(-1, 4) for t in (got, truth))
    E = [np.asarray(e, np.float64).reshape(-1, 4) for e in (errs.values() if isinstance(errs, dict) else errs)]
    assert E and all(e.shape == got.shape == truth.shape for e in E), (what, got.shape, truth.shape, [e.shape for e in E])
    n = got.shape[0]
    bad, ratios = [], {}
    if not np.isfinite(got).all():
        bad.append(f"{int((~np.isfinite(got)).sum())} non-finite outputs")
    groups = {}
    for name, lab in classes.items():
        lab = np.asarray(lab).reshape(-1)
        assert lab.shape[0] == n, (what, name, lab.shape, n)
        groups[name] = np.unique(lab, return_inverse=True, return_counts=True)
    for grp, sl in fu.GROUPS.items():
        e_got, e_ens = got[:, sl] - truth[:, sl], [e[:, sl] for e in E]
        width = e_got.shape[1]
        rms_u, max_u = max(_rms(e) for e in e_ens), max(float(np.abs(e).max()) for e in e_ens)
        assert rms_u > 0 and max_u > 0, (what, grp, "the ensemble is exact: no bound")
        r = dict(rms_all=_rms(e_got) / rms_u, max=float(np.abs(e_got).max()) / max_u, rms_class=0.0, point=0.0)
        if not r["rms_all"] <= FACTOR:
            bad.append(f"{grp}: rms_all {r['rms_all']:.2f} x the ensemble's {rms_u:.3e}")
        if not r["max"] <= FACTOR:
            bad.append(f"{grp}: max {r['max']:.2f} x the ensemble's {max_u:.3e}")
        pt = np.abs(e_got).max(axis=1) / max_u
        small = np.full(n, bool(every_point))
        sq_got, sq_ens = np.square(e_got).sum(1), [np.square(e).sum(1) for e in e_ens]
        for name, (keys, inv, cnt) in groups.items():
            unit = np.maximum(np.max([_by_class(s, inv, cnt, width) for s in sq_ens], axis=0), rms_u)
            with np.errstate(invalid="ignore"):
                rc = np.where(cnt >= MIN_CLASS, _by_class(sq_got, inv, cnt, width) / unit, 0.0)
            rc = np.where(np.isnan(rc), np.inf, rc)
            r["rms_class"] = max(r["rms_class"], float(rc.max()))
            for k in np.nonzero(~(rc <= FACTOR))[0][:8]:
                bad.append(f"{grp}: class {name}={keys[k]} ({int(cnt[k])} points) rms {rc[k]:.2f} x the ensemble's "
                           f"{unit[k]:.3e} there")
            small |= (cnt < MIN_CLASS)[inv]
        if small.any():
            r["point"] = float(pt[small].max())
        for i in np.nonzero(~(pt <= FACTOR))[0][:8]:
            bad.append(f"{grp}: point {i} |err| {pt[i]:.2f} x the ensemble's max {max_u:.3e}")
        ratios[grp] = r
    assert not (bad and check), f"{what}: " + "; ".join(bad[:24]) + (f" (+{len(bad) - 24} more)" if len(bad) > 24 else "")
    return ratios


def worst(ratios):
    return max(max(r.values()) for r in ratios.values())


def leave_one_out(truth, errs, classes, every_point=False, what="", check=True):
    """Every ensemble member held against the others: {order: ratios}."""
    out = {}
    for name, e in errs.items():
        others = [v for k, v in errs.items() if k != name]
        out[name] = f32_compare(truth + e, truth, others, classes, every_point, f"{what} {name} against the others", check)
    return out


def prefix_agreement(short, whole, errs):
    """The outputs of a call on the first points of a set against the same points of the call on the whole set: the worst
    |difference| over 4 max_j max |E_j| per group (<= 1 passes: the per-point bound)."""
    short, whole = np.asarray(short, np.float64).reshape(-1, 4), np.asarray(whole, np.float64).reshape(-1, 4)
    n = short.shape[0]
    out = {}
    for grp, sl in fu.GROUPS.items():
        max_u = max(float(np.abs(np.asarray(e, np.float64).reshape(-1, 4)[:, sl]).max()) for e in errs.values())
        out[grp] = float(np.abs(short[:, sl] - whole[:n, sl]).max()) / (FACTOR * max_u)
    return out


# ----------------------------------------------------------------------------- the cases
# UPDATE THIS TABLE if F32_CHUNK or the channels-last threshold of csrc/point_f32.hip moves (test_point_f32_cpu.py compares the
# source with CHUNK and CL_POINTS above): SWITCH straddles CL_POINTS, CHUNKED straddles CHUNK, INSIDE stays below CL_POINTS.
def _inside(name, coarse=True, **over):
    """A geometry of fused_fp64_util.INTERIOR_CASES; `over`: another seed where that one's sigma is positive on too few points."""
    return dict(make=dict(fu.INTERIOR_CASES[name]["make"], **over), coarse=coarse)


def _make(coarse=True, **kw):
    return dict(make=kw, coarse=coarse)


INSIDE = {                      # the NCHW route at production width: fused_fp64_util.INTERIOR_CASES' geometries, 3089 points or fewer
    "8x8_ns1": _inside("8x8_ns1_proj"),
    "8x8_ns1_fine_mlp": _inside("8x8_ns1_fine_mlp", coarse=False),
    "8x8_ns3_average": _inside("8x8_ns3_average_park16", seed=702),
    "8x8_ns3_max": _inside("8x8_ns3_max_park16"),
    "8x8_ns2_codeview": _inside("8x8_ns2_codeview"),
    "19x25_ns3": _inside("19x25_ns3", seed=545),
    "multiscale_default": _inside("multiscale_default"),
    "multiscale_uv_image": _inside("multiscale_uv_image"),
    "d768_two_groups_uv_image": _inside("d768_two_groups_uv_image"),
    "blocks5_combine0": _inside("blocks5_combine0"),
    "blocks8_combine3_ns3": _inside("blocks8_combine3_ns3_proj", seed=653),
    "sb3": _inside("sb3_proj"),
}
P_BELOW, P_ABOVE = CL_POINTS - 1, CL_POINTS + 33
SWITCH = {                      # one point set each, called at P_BELOW (NCHW reads) and P_ABOVE (channels-last copies)
    "cl_d512_8x8": _make(lat=[(256, 8, 8)], P=P_ABOVE, seed=521),
    "cl_d64_ms4_ns2_uv_image": _make(lat=fu.MS4, NS=2, d_hidden=64, uv_image=True, P=P_ABOVE, seed=523),
}
CHUNKED = {                     # d_hidden 64: the chunk logic does not depend on the width
    "chunk_sb3_ns2_tail132": _make(lat=[(64, 16, 16)], d_hidden=64, NS=2, SB=3, P=16428, seed=531),
    "chunk_ns3_max_codeview_3lvl_tail129": _make(lat=[(32, 16, 16), (64, 8, 8), (16, 4, 4)], d_hidden=64, NS=3, P=CHUNK + 129,
                                                 seed=593, combine_type="max", use_code_viewdirs=True, uv_image=True),
    "chunk_sb2_ns1_no_tail": _make(lat=[(64, 16, 16)], d_hidden=64, SB=2, P=CHUNK, seed=815),
}
RAYS_K, RAYS_SEED, LATTICE_SEED = 37, 620, 620
RAYS = {"rays_83": 83, "rays_131": 131}          # 3071 points (NCHW) and 4847 (channels-last)
POINT_CASES = {**INSIDE, **SWITCH, **CHUNKED}
# per-view intrinsics (tests/test_gpu_intrinsics.py): two objects of two views, one point set each, called with its first
# P_INTR_BELOW points per object (4094 points: NCHW reads) and with all P_INTR_ABOVE (4130: the channels-last copies) — both
# with view > 0.  One row per object (the host repeats it per view), SB*NS distinct rows, and n_focal = 1 with n_c = SB*NS.
P_INTR_BELOW, P_INTR_ABOVE = CL_POINTS // 2 - 1, CL_POINTS // 2 + 17
_intr = dict(lat=[(256, 8, 8)], SB=2, NS=2, P=P_INTR_ABOVE)
INTR = {
    "intr_per_object": _make(seed=571, **_intr, **fu.intr_rows(2)),
    "intr_per_view": _make(seed=572, **_intr, **fu.intr_rows(4)),
    "intr_scalar_focal_per_view_c": _make(seed=573, **_intr, c_xy=fu.intr_rows(4)["c_xy"]),
}
_MAKE = {**POINT_CASES, **INTR}
_cases, _ensembles = {}, {}


def make_case(name):
    """The case dict of a name in POINT_CASES / RAYS, or "lattice"; built once (nothing may write into it)."""
    if name not in _cases:
        if name == "lattice":
            _cases[name] = fu.lattice_case(seed=LATTICE_SEED)
        elif name in RAYS:
            _cases[name] = fu.rays_case([(256, 8, 8)], RAYS[name], RAYS_K, seed=RAYS_SEED)
        else:
            _cases[name] = fu.interior_case(**_MAKE[name]["make"])
    return _cases[name]


def coarse_of(name):
    return _MAKE[name]["coarse"] if name in _MAKE else True


def ensemble(name):
    """fp32_ensemble of a named case, computed once per process and left unchanged."""
    if name not in _ensembles:
        _ensembles[name] = fp32_ensemble(make_case(name), coarse_of(name))
    return _ensembles[name]


def conditions(name):
    """(interior fraction, four-tap fraction, fraction of points with sigma > 0 in float64) of a named case."""
    case = make_case(name)
    a = (case["spec"], case["poses"], case["xyz"])
    return (fu.interior_fraction(*a, uv_scale=case["uv_scale"]), fu.four_tap_fraction(*a, uv_scale=case["uv_scale"]),
            sigma_positive_fraction(ensemble(name)[0]))
