"""CPU checks of tests/fused_fp64_util.py (what tests/test_gpu_fused_fp64.py relies on): the interior cases do put their points
inside the maps with four live taps, every class the rule looks at is populated, the lattice lands exactly and is spread over
tile rows and column groups, the shipped fixtures' geometry clamps (the hole this file documents), and the comparison rule at
its margins rejects planted kernel defects and accepts a second legitimate rounding placement — with emulation output
standing in for the kernel."""
import contextlib

import numpy as np
import pytest
import torch

import fused_fp64_util as fu
import golden_util as gu
import train_fp64_util as tu
from oracle import pixelnerf_oracle as orc


def _views(case):
    return fu.point_classes(case["spec"], case["poses"], case["xyz"], uv_scale=case["uv_scale"])


@pytest.mark.parametrize("name", sorted(fu.INTERIOR_CASES))
def test_interior_cases_are_inside_the_map_and_fill_every_class(name):
    case = fu.make_case(name)
    spec, poses, xyz, uvs = case["spec"], case["poses"], case["xyz"], case["uv_scale"]
    inside = fu.interior_fraction(spec, poses, xyz, uv_scale=uvs)
    four = fu.four_tap_fraction(spec, poses, xyz, uv_scale=uvs)
    ix, iy, zc = fu.texel_coords(spec, poses, xyz, fu.covered_level(spec, uvs), uvs)
    print(f"\n{name}: interior {inside:.3f}, four live taps {four:.3f}, min |z_cam| {np.abs(zc).min():.3e}")
    assert inside >= 0.6 and four >= 0.3
    assert (zc != 0).all() and np.isfinite(ix).all() and np.isfinite(iy).all()
    SB, P = xyz.shape[:2]
    for per_obj in (False, True):
        cls = fu.point_classes(spec, poses, xyz, per_object_tiles=per_obj, uv_scale=uvs)
        n = SB * P if not per_obj else P
        assert set(np.unique(cls["row"])) == set(range(min(n, fu.TILE)))
        assert set(np.unique(cls["wave"])) == set(range(4)) and set(np.unique(cls["colgroup"])) == {0, 1}
        assert set(np.unique(cls["object"])) == set(range(SB))
        tiles = np.unique(cls["tile"])
        assert tiles.size == (SB * -(-P // fu.TILE) if per_obj else -(-SB * P // fu.TILE))
        assert (cls["tile"] == tiles[-1]).sum() == (P if per_obj else SB * P) % fu.TILE != 0       # a tail tile, its own class
        for v in range(spec["NS"]):
            assert set(np.unique(cls[f"tap_view{v}"])) >= {0, 1, 2, 3}, (v, np.bincount(cls[f"tap_view{v}"]))
        assert (cls["tap_view0"] == 4).sum() >= 8                                                  # behind the camera


def test_sweep_and_rays_inputs():
    assert fu.P_FULL % fu.TILE == 17 and fu.make_case("8x8_ns1_proj")["xyz"].shape[1] == fu.P_FULL
    case = fu.rays_case([(256, 8, 8)], 83, 37)
    assert case["xyz"].shape == (1, 83 * 37, 3) and (83 * 37) % fu.TILE != 0 and fu.TILE % 37 != 0    # rays straddle tiles
    assert fu.interior_fraction(case["spec"], case["poses"], case["xyz"]) >= 0.6
    # the points are o + z d of the fp32 inputs, exactly
    r, z = case["rays"].astype(np.float64), case["z"].astype(np.float64)
    assert np.array_equal(case["xyz"].reshape(83, 37, 3), r[:, None, :3] + z[..., None] * r[:, None, 3:6])


def test_lattice_lands_exactly_and_is_spread_over_the_tile():
    case = fu.lattice_case()
    spec, idx, plan = case["spec"], case["lattice_index"], case["plan"]
    C, H, W = fu.LATTICE_MAP
    got = tu.kernel_texel_coords(case["xyz"][0], tu.lattice_c2w(), tu.LATTICE_FOCAL, tu.LATTICE_IMAGE, W, H)
    front = ~np.isnan(plan[:, 0])
    assert np.array_equal(got[front, :2], plan[front]) and (got[front, 2] == -2.0).all()
    assert (got[~front, 2] > 0).all() and (~front).sum() == 3 * len(fu.LATTICE_SHIFTS)
    n, total = idx.max() + 1, idx.size
    assert total % fu.TILE != 0 and total == n * len(fu.LATTICE_SHIFTS)
    pos = np.arange(total)
    for j in range(n):
        p = pos[idx == j]
        assert len(set((p % fu.TILE).tolist())) >= 3 and set(((p % 32) // 16).tolist()) == {0, 1}, j
    tc = fu.tap_class(spec, case["poses"], case["xyz"])
    assert set(np.unique(tc)) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("name", ["full_ns1", "full_ns3", "full_dtu_ns3"])
def test_the_fixtures_geometry_clamps(name):
    """The hole, kept measured: the full-width fixtures' points all but never land strictly inside their latent map, so a test
    built on them sees one border texel of weight 1 per point."""
    fx = gu.load_fixture(name)
    frac = fu.interior_fraction(fx["spec"], fx["poses"], fx["pts_xyz_coarse"])
    print(f"\n{name}: interior fraction {frac:.4f}")
    assert frac < 0.01


def test_emulation_levels():
    """The emulation's own distance from fp64 (the figures the bounds are multiples of): fp32 restatement, fp16, bf16."""
    case = fu.make_case("8x8_ns3_average_park16")
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    truth = fu.truth_fp64(*a)
    lev = {}
    for fmt in ("fp32", "fp16", "bf16"):
        e = fu.emulate_16bit(*a, fmt) - truth
        lev[fmt] = (fu._rms(e[..., :3]), fu._rms(e[..., 3]))
        print(f"\n{fmt}: rgb rms {lev[fmt][0]:.2e}, sigma rms {lev[fmt][1]:.2e}")
    assert lev["fp32"][0] < 1e-5 and 10 * lev["fp32"][0] < lev["fp16"][0] < lev["bf16"][0] / 3
    assert 0.5e-4 < lev["fp16"][0] < 3e-4 and 0.5e-3 < lev["bf16"][0] < 3e-3


# ----------------------------------------------------------------------------- planted defects
def _lookup(uv, latents, swap=False, shift=(0.0, 0.0)):
    """orc.index_latent's bilinear lookup (equal to it for swap=False, shift=0: asserted below) with two planted defects:
    the weights of taps 1 (x1, y0) and 2 (x0, y1) swapped, the texel coordinate shifted."""
    outs = []
    for lat in latents:
        B, C, H, W = lat.shape
        uvb = uv.expand(B, -1, -1) if uv.shape[0] == 1 and B > 1 else uv
        ix = (uvb[..., 0] + shift[0]).clamp(0, W - 1)
        iy = (uvb[..., 1] + shift[1]).clamp(0, H - 1)
        x0, y0 = ix.floor(), iy.floor()
        fx, fy = ix - x0, iy - y0
        w = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
        x1 = x0 + 1
        y1 = y0 + 1
        for i, inb in ((1, x1 <= W - 1), (2, y1 <= H - 1), (3, (x1 <= W - 1) & (y1 <= H - 1))):
            w[i] = torch.where(inb, w[i], torch.zeros_like(w[i]))
        if swap:
            w[1], w[2] = w[2], w[1]
        x1, y1 = x1.clamp(max=W - 1), y1.clamp(max=H - 1)
        flat = lat.reshape(B, C, H * W)
        acc = 0
        for (xx, yy), ww in zip(((x0, y0), (x1, y0), (x0, y1), (x1, y1)), w):
            idx = (yy * W + xx).long()[:, None, :].expand(-1, C, -1)
            acc = acc + torch.gather(flat, 2, idx) * ww[:, None, :]
        outs.append(acc)
    return torch.cat(outs, dim=1)


@contextlib.contextmanager
def _patched(**attrs):
    old = {k: getattr(orc, k) for k in attrs}
    for k, v in attrs.items():
        setattr(orc, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(orc, k, v)


class _SkipOneRelu:
    """Stands in for the oracle module's `torch`: the n-th relu call leaves channel `ch` as it is."""
    def __init__(self, n, ch):
        self.n, self.ch, self.calls = n, ch, 0

    def __getattr__(self, k):
        return getattr(torch, k)

    def relu(self, x):
        out = torch.relu(x)
        if self.calls == self.n:
            out = out.clone()
            out[:, self.ch] = x[:, self.ch]
        self.calls += 1
        return out


def _report(what, got, truth, emu, cls):
    r = fu.class_compare(got, truth, emu, cls, what=what, check=False)
    print("\n" + fu.ratio_line(what, None, r))
    return r


def _rejected(what, got, truth, emu, cls):
    _report(what, got, truth, emu, cls)
    with pytest.raises(AssertionError):
        fu.class_compare(got, truth, emu, cls, what=what)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_rule_rejects_planted_geometry_defects(fmt):
    case = fu.make_case("8x8_ns1_proj")
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    cls = _views(case)
    truth, emu = fu.truth_fp64(*a), fu.emulate_16bit(*a, fmt)
    uv = torch.rand(1, 50, 2) * 9 - 1
    m = [torch.from_numpy(case["maps"][0])]
    assert torch.allclose(_lookup(uv, m), orc.index_latent(uv, m), atol=1e-6)
    fu.class_compare(emu, truth, emu, cls)                          # the emulation against itself passes
    # u shifted by one texel on tile row 77 only
    with _patched(index_latent=lambda uv, lat: _lookup(uv, lat, shift=(1.0, 0.0))):
        bad = fu.emulate_16bit(*a, fmt)
    row77 = (cls["row"] == 77).reshape(1, -1, 1)
    assert row77.sum() >= fu.MIN_CLASS
    _rejected(f"{fmt} u + 1 texel on tile row 77", np.where(row77, bad, emu), truth, emu, cls)
    # taps 1 and 2 swapped, on the points clamped in y only
    with _patched(index_latent=lambda uv, lat: _lookup(uv, lat, swap=True)):
        bad = fu.emulate_16bit(*a, fmt)
    cy = (cls["tap_view0"] == 2).reshape(1, -1, 1)
    _rejected(f"{fmt} taps 1, 2 swapped where clamped in y", np.where(cy, bad, emu), truth, emu, cls)
    # the swap everywhere (the mutation run of the GPU file) — and invisible on points clamped in both (the fixtures' geometry)
    _rejected(f"{fmt} taps 1, 2 swapped", bad, truth, emu, cls)
    cxy = (cls["tap_view0"] == 3).reshape(-1)
    assert np.array_equal(bad.reshape(-1, 4)[cxy], emu.reshape(-1, 4)[cxy])


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_rule_rejects_a_swapped_view_on_the_tail_and_a_swapped_object(fmt):
    case = fu.make_case("8x8_ns3_average_park16")
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    cls = _views(case)
    truth, emu = fu.truth_fp64(*a), fu.emulate_16bit(*a, fmt)
    maps = [m.copy() for m in case["maps"]]
    maps[0][1] = maps[0][0]                                         # view 1 reads view 0's latent
    bad = fu.emulate_16bit(a[0], a[1], maps, a[3], a[4], fmt)
    tail = (cls["tile"] == cls["tile"].max()).reshape(1, -1, 1)
    assert tail.sum() == 17
    _rejected(f"{fmt} view 1 <- view 0 on the 17-point tail", np.where(tail, bad, emu), truth, emu, cls)

    case = fu.make_case("sb3_general")
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    cls = _views(case)
    truth, emu = fu.truth_fp64(*a), fu.emulate_16bit(*a, fmt)
    maps = [m.copy() for m in case["maps"]]
    maps[0][2] = maps[0][0]                                         # object 2 reads object 0's map
    bad = fu.emulate_16bit(a[0], a[1], maps, a[3], a[4], fmt)
    assert not np.array_equal(bad[2], emu[2]) and np.array_equal(bad[:2], emu[:2])
    _rejected(f"{fmt} object 2 <- object 0's map", bad, truth, emu, cls)


def test_rule_rejects_a_skipped_relu_on_one_hidden_channel():
    case = fu.make_case("8x8_ns1_proj")
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    cls = _views(case)
    truth, emu = fu.truth_fp64(*a), fu.emulate_16bit(*a, "fp16")
    proxy = _SkipOneRelu(n=2 * 3, ch=201)                           # relu calls: block b's fc_0 input is call 2 b
    with _patched(torch=proxy):
        bad = fu.emulate_16bit(*a, "fp16")
    assert proxy.calls == 2 * case["spec"]["n_blocks"] + 2
    _rejected("fp16 relu skipped on channel 201 of block 3", bad, truth, emu, cls)


@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
def test_rule_accepts_a_second_legitimate_rounding_placement(fmt):
    case = fu.make_case("8x8_ns3_average_park16")
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    cls = _views(case)
    truth, emu = fu.truth_fp64(*a), fu.emulate_16bit(*a, fmt)
    r = fu.class_compare(fu.emulate_16bit(*a, fmt, park16=False), truth, emu, cls, what="park fp32 against park 16 bit")
    print("\n" + fu.ratio_line(f"{fmt} park fp32 against park 16 bit", None, r))
    r = fu.class_compare(fu.emulate_16bit(*a, fmt, skip=("latent",)), truth, emu, cls, what="lin_z on the unrounded latent")
    print(fu.ratio_line(f"{fmt} lin_z on the unrounded latent", None, r))
    case = fu.lattice_case()
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    truth, emu = fu.truth_fp64(*a), fu.emulate_16bit(*a, fmt)
    r = fu.class_compare(fu.emulate_16bit(*a, fmt, skip=("latent",)), truth, emu, _views(case), every_point=True,
                         what="lattice, lin_z on the unrounded latent")
    print(fu.ratio_line(f"{fmt} lattice, lin_z on the unrounded latent", None, r))


def test_rule_small_calls_and_non_finite_outputs():
    case = fu.make_case("8x8_ns1_proj")
    a = (case["spec"], case["poses"], case["maps"], case["xyz"], case["dirs"])
    truth, emu = fu.truth_fp64(*a), fu.emulate_16bit(*a, "fp16")
    cls = _views(case)
    other = fu.emulate_16bit(*a, "fp16", skip=("latent",))
    for P in fu.P_SWEEP:
        c = {k: v[:P] for k, v in cls.items()}
        fu.class_compare(other[:, :P], truth[:, :P], emu[:, :P], c, emu_ref=(truth, emu), what=f"P {P}")
    bad = other[:, :1].copy(); bad[0, 0, 1] += 10 * np.abs(emu - truth)[..., :3].max()
    with pytest.raises(AssertionError):
        fu.class_compare(bad, truth[:, :1], emu[:, :1], {k: v[:1] for k, v in cls.items()}, emu_ref=(truth, emu))
    nan = emu.copy(); nan[0, 5, 3] = np.nan
    with pytest.raises(AssertionError):
        fu.class_compare(nan, truth, emu, cls)
