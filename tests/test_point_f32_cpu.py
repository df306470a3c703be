"""CPU checks of tests/point_f32_util.py (what tests/test_gpu_point_f32_fp64.py relies on): the case table straddles the two
constants csrc/point_f32.hip states, every case puts its points inside the maps with four live taps and a sigma that is
positive on most of them, the chunked cases cut where they say, every legitimate fp32 summation order passes the rule at half
its bound when held against the others, and the rule rejects planted defects of the fp32 path — each made by perturbing the
oracle's evaluation on the points the defect would touch, with restatement output standing in for the kernels."""
import contextlib

import numpy as np
import pytest
import torch

import fused_fp64_util as fu
import golden_util as gu
import point_f32_util as pu
import train_fp64_util as tu
from oracle import pixelnerf_oracle as orc

ALL_CASES = list(pu.POINT_CASES) + list(pu.RAYS)
ACCEPT_AT = 2.0                  # a legitimate reordering scores at most half the bound of 4


def test_case_table_straddles_the_source_constants():
    """If this fails, F32_CHUNK or the channels-last threshold moved in csrc/point_f32.hip: set point_f32_util.CHUNK /
    CL_POINTS to the new values and check the tables INSIDE, SWITCH, CHUNKED and RAYS there still sit on the sides they name."""
    assert pu.source_constants() == (pu.CHUNK, pu.CL_POINTS) == (49152, 4096)
    n = lambda name: int(np.prod(pu.make_case(name)["xyz"].shape[:2]))
    assert all(n(k) < pu.CL_POINTS for k in pu.INSIDE)
    assert pu.P_BELOW == pu.CL_POINTS - 1 and all(n(k) == pu.P_ABOVE > pu.CL_POINTS for k in pu.SWITCH)
    assert all(pu.make_case(k)["spec"]["SB"] == 1 for k in pu.SWITCH)           # n_points of the call = P
    assert n("rays_83") < pu.CL_POINTS <= n("rays_131") and pu.GEMM_TILE % pu.RAYS_K != 0
    assert all(n(k) >= pu.CHUNK for k in pu.CHUNKED) and pu.CHUNK % pu.GEMM_TILE == 0


def test_chunked_cases_cut_where_they_say():
    c = pu.make_case("chunk_sb3_ns2_tail132")
    SB, P = c["xyz"].shape[:2]
    assert (SB, c["spec"]["NS"]) == (3, 2) and 2 * P < pu.CHUNK < 3 * P          # chunk 0: two whole objects and part of a third
    assert SB * P - pu.CHUNK == 132 and 132 % pu.GEMM_TILE != 0 and 132 > pu.GEMM_TILE
    cls = pu.f32_classes(c)
    assert set(np.unique(cls["object"][cls["chunk"] == 0])) == {0, 1, 2} and set(np.unique(cls["object"][cls["chunk"] == 1])) == {2}
    # view 1's rows of the tail chunk start at row 132 of the GEMM: its tiles are cut elsewhere than view 0's
    tail = cls["chunk"] == 1
    assert len(np.unique(cls["tile"][tail])) == 2 and len(np.unique(cls["gemm_tile_view1"][tail])) == 2
    assert (cls["tile"][tail] == cls["tile"][tail].max()).sum() == 4 and (cls["gemm_tile_view1"][tail] == cls["gemm_tile_view1"][tail].min()).sum() == 124
    c = pu.make_case("chunk_ns3_max_codeview_3lvl_tail129")
    s = c["spec"]
    assert (s["SB"], s["NS"], s["combine_type"], s["use_code_viewdirs"], len(s["lat"])) == (1, 3, "max", True, 3) and c["uv_scale"]
    assert len({ch for ch, _, _ in s["lat"]}) == 3 and c["xyz"].shape[1] - pu.CHUNK == 129
    c = pu.make_case("chunk_sb2_ns1_no_tail")
    cls = pu.f32_classes(c)
    assert (c["spec"]["SB"], c["spec"]["NS"], c["xyz"].shape[1]) == (2, 1, pu.CHUNK) and np.array_equal(cls["chunk"], cls["object"])
    c = pu.make_case("cl_d64_ms4_ns2_uv_image")
    assert len({ch for ch, _, _ in c["spec"]["lat"]}) == 3 and c["spec"]["NS"] == 2 and c["spec"]["d_hidden"] == 64


@pytest.mark.parametrize("name", ALL_CASES + ["lattice"])
def test_cases_meet_the_conditions_and_every_summation_order_is_accepted(name):
    """Interior fraction >= 0.6, four live taps on >= 0.3, sigma > 0 in float64 on >= half of the points (the lattice is exact
    geometry, not a cloud: only the sigma condition applies); then each ensemble member against the others: worst ratio
    <= 2, half the bound."""
    inside, four, sig = pu.conditions(name)
    print(f"\n{name}: interior {inside:.3f}, four live taps {four:.3f}, sigma > 0 on {sig:.3f}")
    if name != "lattice":
        assert inside >= pu.MIN_INTERIOR and four >= pu.MIN_FOUR_TAP
    assert sig >= pu.MIN_SIGMA_POSITIVE
    case = pu.make_case(name)
    _, _, zc = fu.texel_coords(case["spec"], case["poses"], case["xyz"], 0, case["uv_scale"])
    assert (zc != 0).all()
    truth, errs = pu.ensemble(name)
    assert len(errs) >= 3 and {"default", "k16", "k32_reversed"} <= set(errs)
    loo = pu.leave_one_out(truth, errs, pu.f32_classes(case), every_point=name == "lattice", what=name)
    for order, r in loo.items():
        print(fu.ratio_line(f"{name} {order} against the others", None, r))
        assert pu.worst(r) <= ACCEPT_AT, (name, order, r)


# ----------------------------------------------------------------------------- planted defects
@contextlib.contextmanager
def _lookup(fn):
    orig = orc.index_latent
    orc.index_latent = lambda uv, latents: fn(orig, uv, latents)
    try:
        yield
    finally:
        orc.index_latent = orig


def _taps_1_2_swapped(orig, uv, latents):
    """The lookup with the weights of taps 1 (x1, y0) and 2 (x0, y1) swapped: the same as looking up (x0 + fy, y0 + fx)."""
    outs = []
    for lat in latents:
        H, W = lat.shape[2:]
        ix, iy = uv[..., 0].clamp(0, W - 1), uv[..., 1].clamp(0, H - 1)
        x0, y0 = ix.floor(), iy.floor()
        outs.append(orig(torch.stack([x0 + (iy - y0), y0 + (ix - x0)], dim=-1), [lat]))
    return torch.cat(outs, dim=1)


def _rows_f32(case):
    """(state dict, the MLP's input rows (SB, NS, P, L + d_in)) of the default fp32 restatement."""
    spec = case["spec"]
    sd = {k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, "coarse").items()}
    SB, P = case["xyz"].shape[:2]
    with torch.no_grad(), fu._scaled_lookup(case["uv_scale"]):
        _, st = orc.point_forward(sd, tu.fp64_camera(spec, case["poses"], torch.float32), [torch.from_numpy(m) for m in case["maps"]],
                                  torch.from_numpy(np.asarray(case["xyz"], np.float32)), torch.from_numpy(np.asarray(case["dirs"], np.float32)),
                                  spec["NS"], use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"],
                                  combine_layer=spec["combine_layer"], combine_type=spec["combine_type"], return_stages=True)
    return sd, st["mlp_in"].reshape(SB, spec["NS"], P, -1)


def _mlp(spec, sd, rows, rnd=None):
    """chain_f32 + k_out_act on one object's rows (NS, p, E): (p, 4)."""
    NS, p, E = rows.shape
    with torch.no_grad():
        o = orc.resnetfc(sd, rows.reshape(-1, E), gu.d_latent_of(spec), NS, p, n_blocks=spec["n_blocks"],
                         combine_layer=spec["combine_layer"], combine_type=spec["combine_type"], rnd=rnd)
    return torch.cat([torch.sigmoid(o[:, :3]), torch.relu(o[:, 3:])], dim=-1).double().numpy()


def _scores(what, name, bad):
    """The defect's ratios, printed; the rule must reject it."""
    truth, errs = pu.ensemble(name)
    cls = pu.f32_classes(pu.make_case(name))
    r = pu.f32_compare(bad, truth, errs, cls, what=what, check=False)
    print("\n" + fu.ratio_line(f"{what} [{name}]", None, r))
    with pytest.raises(AssertionError):
        pu.f32_compare(bad, truth, errs, cls, what=what)
    return r


def _good(name):
    truth, errs = pu.ensemble(name)
    return truth + errs["default"]


def test_rule_rejects_two_tap_weights_swapped_on_one_gemm_tile():
    name = "cl_d512_8x8"
    case, good = pu.make_case(name), _good(name)
    with _lookup(_taps_1_2_swapped):
        bad = pu.restate_f32(case)
    tile = (pu.f32_classes(case)["tile"] == 21).reshape(1, -1, 1)
    assert tile.sum() == pu.GEMM_TILE
    _scores("taps 1, 2 swapped on GEMM tile 21 only", name, np.where(tile, bad, good))
    _scores("taps 1, 2 swapped everywhere (the mutation run)", name, bad)


def test_rule_rejects_a_tail_chunk_read_with_the_full_chunk_stride():
    """View 1's rows of the 129-point tail read at 49152 + pl instead of 129 + pl: what the full chunk before left there, view
    1's features of chunk 0's first 129 points."""
    name = "chunk_ns3_max_codeview_3lvl_tail129"
    case, good = pu.make_case(name), _good(name).copy()
    sd, rows = _rows_f32(case)
    tail = rows[0, :, pu.CHUNK:].clone()
    assert tail.shape[1] == 129
    honest = _mlp(case["spec"], sd, tail)
    assert np.abs(honest - good[0, pu.CHUNK:]).max() < 1e-4                     # the tail alone restates the tail
    tail[1] = rows[0, 1, :129]
    good[0, pu.CHUNK:] = _mlp(case["spec"], sd, tail)
    _scores("tail chunk: view 1 at stride 49152", name, good)


def test_rule_rejects_the_object_of_the_chunks_first_point():
    """obj = g0 / pts_per_obj in place of g / pts_per_obj: in chunk 0 the points of objects 1 and 2 see object 0's cameras and
    maps; the tail chunk starts inside object 2 and stays right."""
    name = "chunk_sb3_ns2_tail132"
    case, good = pu.make_case(name), _good(name)
    SB, NS = case["spec"]["SB"], case["spec"]["NS"]
    poses = case["poses"].copy()
    poses[1:] = poses[0]
    maps = [m.reshape(SB, NS, *m.shape[1:]).copy() for m in case["maps"]]
    for m in maps:
        m[1:] = m[0]
    bad = pu.restate_f32(case, poses=poses, maps=[m.reshape(SB * NS, *m.shape[2:]) for m in maps])
    cls = pu.f32_classes(case)
    hit = ((cls["chunk"] == 0) & (cls["object"] > 0)).reshape(good.shape[0], -1, 1)
    _scores("object of the chunk's first point", name, np.where(hit, bad, good))
    only2 = ((cls["chunk"] == 0) & (cls["object"] == 2)).reshape(good.shape[0], -1, 1)
    _scores("object of the chunk's first point, object 2 only", name, np.where(only2, bad, good))


def test_rule_rejects_a_view_mean_over_the_wrong_count_on_the_tail_chunk():
    name = "chunk_sb3_ns2_tail132"
    case, good = pu.make_case(name), _good(name).copy()
    NS = case["spec"]["NS"]
    sd, rows = _rows_f32(case)
    tail = rows[2, :, -132:]
    wrong = lambda t, kind: t * (NS / (NS + 1.0)) if kind == "park" else t      # the sum over NS views divided by NS + 1
    good[2, -132:] = _mlp(case["spec"], sd, tail, rnd=wrong)
    _scores("tail chunk: view mean divided by NS + 1", name, good)


def test_rule_rejects_one_level_rounded_to_bf16():
    name = "multiscale_default"
    case = pu.make_case(name)
    maps = list(case["maps"])
    maps[1] = torch.from_numpy(maps[1]).bfloat16().float().numpy()
    _scores("level 1 of 4 rounded to bf16", name, pu.restate_f32(case, maps=maps))


def test_rule_rejects_one_layer_with_operands_cut_to_10_mantissa_bits():
    name = "8x8_ns1"
    case = pu.make_case(name)
    cut = lambda t: (t.contiguous().view(torch.int32) & ~0x1FFF).view(torch.float32)
    orig, calls = torch.addmm, []

    def addmm(b, x, wt):
        calls.append(1)
        return orig(b, cut(x), cut(wt)) if len(calls) == 9 else orig(b, x, wt)      # lin_in, 2 x (lin_z, fc_0, fc_1), lin_z, fc_0
    torch.addmm = addmm
    try:
        bad = pu.restate_f32(case)
    finally:
        torch.addmm = orig
    assert len(calls) == 1 + 3 * 3 + 2 * 2 + 1
    _scores("block 2's fc_0 on operands of 10 mantissa bits", name, bad)


def test_rule_rejects_non_finite_outputs_and_one_bad_point():
    name = "8x8_ns1"
    truth, errs = pu.ensemble(name)
    cls = pu.f32_classes(pu.make_case(name))
    bad = _good(name).copy()
    bad[0, 5, 3] = np.nan
    with pytest.raises(AssertionError):
        pu.f32_compare(bad, truth, errs, cls)
    bad = _good(name).copy()
    bad[0, 1234, 1] += 6 * max(np.abs(e[..., :3]).max() for e in errs.values())
    with pytest.raises(AssertionError, match="point 1234"):
        pu.f32_compare(bad, truth, errs, cls)
