"""The fused 16-bit kernel k_point_mfma, point by point against float64, on points INSIDE the latent maps.

Every case goes through build_net(spec, poses, "cuda", prec) and net(xyz, coarse=..., viewdirs=...) in fp16 and bf16, and is
held to tests/fused_fp64_util.class_compare: the kernel's error against the oracle in float64, per group (rgb, sigma), over
all points, per tile row / wave / column group / tile / object / tap class, and per point in small classes, against the error
of a generic 16-bit emulation of the same network on the same points (emulate_16bit), with margins that come from the
emulation and the number formats alone.  The inputs and the rule are checked on the CPU by tests/test_fused_fp64_cpu.py.
Each case prints one line: case, interior fraction, the four worst ratios (kernel figure / emulation figure, margins not
applied: the bounds are rms_all 2, max 4, rms_class 4, point 4)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_fp64_util as fu

pytestmark = pytest.mark.gpu
PRECS = ["fp16", "bf16"]
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _truth_emu(key, case, prec, park16=True, coarse=True):
    """fp64 truth (once per point set) and the emulation (once per format and park precision)."""
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    truth = _memo(("truth", key, coarse), lambda: fu.truth_fp64(*a, uv_scale=case["uv_scale"], coarse=coarse))
    emu = _memo(("emu", key, coarse, prec, park16 or case["spec"]["NS"] == 1),
                lambda: fu.emulate_16bit(*a, prec, park16=park16, uv_scale=case["uv_scale"], coarse=coarse))
    return truth, emu


def _net(case, prec, proj=True, park="16bit", stream=None, coarse=True):
    """The net of a case, and whether the kernel tiles per object (projected streams of several objects)."""
    from hip_util import build_net
    spec = case["spec"]
    net = build_net(spec, case["poses"], "cuda", prec)
    net.project_latent = proj
    net.park_precision = park
    if case["uv_scale"]:
        net.encoder.uv_scale = "image"
        assert np.allclose(np.asarray(net.uv_scales()), np.asarray(case["uv_scale"]))
    assert net.resolved_precision() == prec
    v, _ = net.views_struct(prec)
    m, _ = net.mlp_struct(net.mlp_coarse if coarse else net.mlp_fine, prec, v)
    projected = m.packed_texels > 0
    if stream is not None:
        assert projected == (stream == "proj"), (stream, m.packed_texels)
    return net, projected and spec["SB"] > 1


def _points(net, case, coarse=True, P=None):
    xyz = torch.from_numpy(np.ascontiguousarray(case["xyz"][:, :P], dtype=np.float32)).cuda()
    dirs = torch.from_numpy(np.ascontiguousarray(case["dirs"][:, :P], dtype=np.float32)).cuda()
    out = net(xyz, coarse=coarse, viewdirs=dirs)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _classes(case, per_object_tiles=False):
    return fu.point_classes(case["spec"], case["poses"], case["xyz"], per_object_tiles, uv_scale=case["uv_scale"])


def _frac(case):
    return fu.interior_fraction(case["spec"], case["poses"], case["xyz"], uv_scale=case["uv_scale"])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", sorted(fu.INTERIOR_CASES))
def test_fused_kernel_matches_fp64_inside_the_map(name, prec):
    """fused_fp64_util.INTERIOR_CASES: one view on both streams and the fine MLP, three views (mean and max, both park
    precisions, both streams), coded view dirs, a map too large to project (475 texels), 35 texels (a padded k-step of the
    projected part), the 4-level map under both uv mappings, d_latent 768 and 1024, the n_blocks / combine_layer corners,
    three objects with P off a tile multiple on both streams."""
    cfg = fu.INTERIOR_CASES[name]
    case = fu.make_case(name)
    net, per_obj = _net(case, prec, cfg["proj"], cfg["park"], cfg["stream"], cfg["coarse"])
    got = _points(net, case, cfg["coarse"])
    truth, emu = _truth_emu(repr(sorted(cfg["make"].items(), key=str)), case, prec, cfg["park"] == "16bit", cfg["coarse"])
    r = fu.class_compare(got, truth, emu, _classes(case, per_obj), what=f"{name} {prec}", check=False)
    print("\n" + fu.ratio_line(f"{name} {prec}", _frac(case), r))
    fu.class_compare(got, truth, emu, _classes(case, per_obj), what=f"{name} {prec}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stream", ["proj", "general"])
def test_fused_kernel_matches_fp64_at_every_call_size(stream, prec):
    """P in {1, 127, 128, 129, 128 * 24 + 17}: the first P points of one point set.  Truth and emulation are computed once on
    the whole set; a short call is held to the whole set's emulation figures (class_compare's emu_ref) — one point's own
    emulation error is one draw, not a level."""
    name = "8x8_ns1_proj" if stream == "proj" else "8x8_ns1_general"
    cfg = fu.INTERIOR_CASES[name]
    case = fu.make_case(name)
    net, _ = _net(case, prec, cfg["proj"], stream=stream)
    truth, emu = _truth_emu(repr(sorted(cfg["make"].items(), key=str)), case, prec)
    cls = _classes(case)
    for P in fu.P_SWEEP:
        got = _points(net, case, P=P)
        assert got.shape == (1, P, 4)
        args = (got, truth[:, :P], emu[:, :P], {k: v[:P] for k, v in cls.items()})
        r = fu.class_compare(*args, emu_ref=(truth, emu), what=f"P {P} {stream} {prec}", check=False)
        print("\n" + fu.ratio_line(f"P {P} {stream} {prec}", _frac(case), r))
        fu.class_compare(*args, emu_ref=(truth, emu), what=f"P {P} {stream} {prec}")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("stream", ["proj", "general"])
def test_fused_kernel_matches_fp64_on_the_lattice(stream, prec):
    """Points planned exactly on texel centres, lines and corners, the borders, outside and behind the camera, each in several
    tile rows and both column groups (fused_fp64_util.lattice_case; 45 texels: a padded k-step when projected).  Every point
    is held to the per-point bound."""
    case = fu.lattice_case()
    net, _ = _net(case, prec, stream == "proj", stream=stream)
    got = _points(net, case)
    truth, emu = _truth_emu("lattice", case, prec)
    r = fu.class_compare(got, truth, emu, _classes(case), every_point=True, what=f"lattice {stream} {prec}", check=False)
    print("\n" + fu.ratio_line(f"lattice {stream} {prec}", _frac(case), r))
    fu.class_compare(got, truth, emu, _classes(case), every_point=True, what=f"lattice {stream} {prec}")


@pytest.mark.parametrize("prec", PRECS)
def test_fused_kernel_matches_fp64_in_rays_mode(prec):
    """pnr_point_mlp with (rays, z, K) as test_gpu_parity._staged_render.one_pass calls it: the kernel forms o + z d itself.
    K = 37, so rays straddle tiles; truth and emulation evaluate o + z d of the fp32 inputs."""
    from pixel_nerf_multiscale_amd import _native as N
    n_rays, K = 83, 37
    case = fu.rays_case([(256, 8, 8)], n_rays, K)
    net, _ = _net(case, prec, stream="proj")
    prm = net.params_struct(None, prec)
    v, keep_v = net.views_struct(prec)
    m, keep_m = net.mlp_struct(net.mlp_coarse, prec, v)
    r = torch.from_numpy(case["rays"]).cuda().contiguous()
    z = torch.from_numpy(case["z"]).cuda().contiguous()
    out = torch.empty(n_rays * K, 4, device="cuda")
    ws = net.workspace(N.lib.pnr_workspace_bytes(C.byref(prm), C.byref(m), C.byref(v), n_rays), r.device)
    N.check(N.lib.pnr_point_mlp(C.byref(prm), C.byref(m), C.byref(v), N.ptr(r), N.ptr(z), K, None, None, n_rays * K, n_rays * K,
                                N.ptr(out), ws.data_ptr(), ws.numel(), N.current_stream(r.device)), "pnr_point_mlp")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    truth, emu = _truth_emu("rays", case, prec)
    res = fu.class_compare(got, truth, emu, _classes(case), what=f"rays mode {prec}", check=False)
    print("\n" + fu.ratio_line(f"rays mode {prec}", _frac(case), res))
    fu.class_compare(got, truth, emu, _classes(case), what=f"rays mode {prec}")
