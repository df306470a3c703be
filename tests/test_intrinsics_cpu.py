"""CPU checks behind tests/test_gpu_intrinsics.py: per-view source intrinsics (fx != fy, off-centre c, one row per object or
per view) from the caller's tensors to the rows a kernel's load_cam reads, and the teeth of the cases the GPU file runs.

  * every form PixelNeRFNet.set_cameras accepts, through models.views_from, against orc.encode_cameras and against the values
    written out by hand: fy negated once, n_focal / n_c in {1, SB*NS}, a per-object row repeated per view in object-major order;
  * every GPU case puts at least 0.6 of its (view, point) pairs inside the map under its OWN intrinsics, and every mistake with
    the intrinsics that can be made on it moves the fp64 truth's rgb by at least 5 x what class_compare accepts for bf16;
  * class_compare and f32_compare refuse such a mutant handed to them as kernel output."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_fp64_util as fu
import golden_util as gu
import point_f32_util as pu
from oracle import pixelnerf_oracle as orc

# ----------------------------------------------------------------------------- camera forms
W_IMG, H_IMG = 8, 6


def _form(kind, SB, NS, base, axis_step):
    """(the caller's value, the (SB*NS, 2) rows every view must end up with) for one accepted form; base: the first entry,
    axis_step: what the second column adds (0.0 for the forms that have one value for both axes)."""
    nv = SB * NS
    if kind == "none":
        return None, np.tile(np.array([[W_IMG * 0.5, H_IMG * 0.5]], np.float32), (nv, 1))
    if kind == "scalar":
        return torch.tensor(base), np.full((nv, 2), base, np.float32)
    if kind == "per_object":                    # (SB,): one value per object, both axes
        v = (base + 0.25 * np.arange(SB)).astype(np.float32)
        return torch.from_numpy(v), np.repeat(np.stack([v, v], 1), NS, axis=0)
    if kind == "per_object_xy":                 # (SB, 2)
        v = (base + 0.25 * np.arange(SB)[:, None] + np.array([[0.0, axis_step]])).astype(np.float32)
        return torch.from_numpy(v), np.repeat(v, NS, axis=0)
    assert kind == "per_view_xy"                # (SB*NS, 2), object-major
    v = (base + 0.125 * np.arange(nv)[:, None] + np.array([[0.0, axis_step]])).astype(np.float32)
    return torch.from_numpy(v), v


def _struct_rows(vs, field, count_field):
    """The float pairs behind a pnr_views pointer, and per view the pair load_cam reads (pnr_common.h: row `view` when the
    count is above 1, else row 0)."""
    n = getattr(vs, count_field)
    rows = np.ctypeslib.as_array((C.c_float * (2 * n)).from_address(getattr(vs, field))).reshape(n, 2).copy()
    nv = vs.n_objs * vs.n_views
    return n, np.stack([rows[view if n > 1 else 0] for view in range(nv)])


_nets = {}


def _net(spec):
    """One CPU PixelNeRFNet per (SB, NS): set_cameras replaces the camera buffers on every call."""
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import PixelNeRFNet
    key = (spec["SB"], spec["NS"])
    if key not in _nets:
        _nets[key] = PixelNeRFNet(model_conf(spec))
    return _nets[key]


FOCAL_FORMS = ["scalar", "per_object", "per_object_xy", "per_view_xy"]
C_FORMS = ["none", "scalar", "per_object", "per_object_xy", "per_view_xy"]


@pytest.mark.parametrize("SB,NS", [(3, 2), (3, 1)])
@pytest.mark.parametrize("c_kind", C_FORMS)
@pytest.mark.parametrize("f_kind", FOCAL_FORMS)
def test_every_camera_form_reaches_the_kernel_rows_the_oracle_uses(f_kind, c_kind, SB, NS, monkeypatch):
    """set_cameras + views_from on CPU tensors (the struct's pointers then address host memory, read back here the way
    load_cam indexes them) for focal in {(), (SB,), (SB, 2), (SB*NS, 2)} x c in {None, (), (SB,), (SB, 2), (SB*NS, 2)} —
    the mixed n_focal = 1 / n_c = SB*NS cases and the reverse among them — at SB = 3 != NS = 2 and at NS = 1."""
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.model import models
    monkeypatch.setattr(N, "ptr", lambda t: None if t is None else t.data_ptr())
    nv = SB * NS
    focal, want_f = _form(f_kind, SB, NS, 7.5, 1.75)
    c, want_c = _form(c_kind, SB, NS, 3.25, -0.5)
    want_f = want_f * np.array([[1.0, -1.0]], np.float32)                              # fy negated, once
    spec = dict(gu.CASES["tiny_sb2_ns2"], SB=SB, NS=NS)
    poses = torch.from_numpy(gu.make_inputs(dict(spec, N=1))[1])
    net = _net(spec)
    net.num_objs, net.num_views_per_obj = SB, NS
    keep_in = [None if t is None else t.clone() for t in (focal, c)]
    net.set_cameras(poses.reshape(-1, 4, 4), focal, c, W_IMG, H_IMG)
    for t, k in zip((focal, c), keep_in):
        assert t is None or torch.equal(t, k), "set_cameras wrote into the caller's tensor"
    # the oracle's camera record: the same tensors
    w2c, o_f, o_c = orc.encode_cameras(poses, focal, c, W_IMG, H_IMG)
    assert torch.equal(net.focal, o_f) and torch.equal(net.c, o_c) and torch.equal(net.poses, w2c)
    # the rows behind the struct
    maps = [torch.zeros(nv, 4, 5, 7)]
    vs, keep = models.views_from(net.poses, net.focal, net.c, NS, maps)
    assert (vs.n_objs, vs.n_views) == (SB, NS)
    n_f, got_f = _struct_rows(vs, "focal", "n_focal")
    n_c, got_c = _struct_rows(vs, "c", "n_c")
    assert n_f == (1 if f_kind == "scalar" else nv) and n_c == (1 if c_kind in ("none", "scalar") else nv), (n_f, n_c)
    assert np.array_equal(got_f, want_f), (got_f, want_f)
    assert np.array_equal(got_c, want_c), (got_c, want_c)
    # ... and the oracle projects every view with the same pair: one point per view at x_cam = (-1, -1, 1) gives uv = f + c
    xyz = torch.zeros(SB, 1, 3)
    cam = (torch.cat([torch.eye(3), torch.tensor([[-1.0], [-1.0], [1.0]])], 1).expand(nv, 3, 4).contiguous(), o_f, o_c)
    sd = {k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, "coarse").items()}
    lat = [torch.zeros(nv, 8, 5, 7)]
    _, st = orc.point_forward(sd, cam, lat, xyz, torch.zeros(SB, 1, 3), NS, return_stages=True)
    assert np.array_equal(st["uv"].reshape(nv, 2).numpy(), want_f + want_c)


def test_intrinsics_helper_defaults_and_forms():
    """golden_util.intrinsics: the scalar focal and None unless the spec says otherwise; view_intrinsics writes SB rows out per
    view and takes SB*NS rows object-major."""
    spec = gu.CASES["tiny_sb2_ns2"]
    assert gu.intrinsics(spec) == (spec["focal"], None)
    f, c = gu.view_intrinsics(spec)
    assert f.shape == c.shape == (2, 2, 2) and (f == 45.0).all() and (c == np.array([20.0, 15.0])).all()
    spec = gu.INTRINSICS_CASES["full_sb2_ns2_intr"]
    focal, c = gu.intrinsics(spec)
    assert focal.shape == c.shape == (2, 2) and focal.dtype == c.dtype == np.float32
    assert np.array_equal(focal, (np.array(gu.INTR_F_ROWS) * spec["focal"]).astype(np.float32)) and (focal[:, 0] != focal[:, 1]).all()
    assert np.allclose(c - 4.0, gu.INTR_C_ROWS) and (focal > 0).all()
    f, c = gu.view_intrinsics(spec)
    assert np.array_equal(f[:, 0], f[:, 1]) and np.array_equal(f[:, 0], focal) and not np.array_equal(f[0], f[1])
    rows4 = dict(spec, **fu.intr_rows(4))
    f, c = gu.view_intrinsics(rows4)
    assert np.array_equal(f.reshape(4, 2), gu.intrinsics(rows4)[0]) and np.array_equal(c.reshape(4, 2), gu.intrinsics(rows4)[1])


# ----------------------------------------------------------------------------- the cases have teeth
MUTANT_POINTS = 512          # per object: the mutants' fp64 truths are formed on a prefix of the case's points


def _train_case():
    return fu.interior_case(**fu.INTR_TRAIN)


def _fixture_case(name):
    """The reference fixture's coarse points as a point case."""
    fx = gu.load_fixture(name)
    spec = fx["spec"]
    return dict(spec=spec, poses=fx["poses"], maps=gu.make_latents(spec), xyz=fx["pts_xyz_coarse"], dirs=fx["pts_dirs_coarse"],
                uv_scale=None)


TEETH = {**{k: (lambda k=k: fu.intr_case(k)) for k in list(fu.INTR_FUSED_CASES) + ["rays_sb1_ns2"]},
         **{k: (lambda k=k: pu.make_case(k)) for k in pu.INTR},
         "train_sb2_ns2_per_object": _train_case,
         **{k: (lambda k=k: _fixture_case(k)) for k in gu.INTRINSICS_CASES}}
ALL_MUTANTS = {"fy := fx", "fx <-> fy", "c := centre", "cx <-> cy", "row 0 for every row", "rows rolled by one",
               "only focal broadcast", "only c broadcast"}
ONE_ROW = {"fy := fx", "fx <-> fy", "c := centre", "cx <-> cy"}                       # one row: no second row to confuse it with
# a scalar focal has no axes to swap and no rows; "row 0 for every row" is then "only c broadcast"
SCALAR_FOCAL = {"c := centre", "cx <-> cy", "row 0 for every row", "rows rolled by one", "only c broadcast"}
EXPECTED_MUTANTS = {k: ALL_MUTANTS for k in TEETH}
EXPECTED_MUTANTS.update(sb1_ns1_proj=ONE_ROW, sb1_ns1_general=ONE_ROW, intr_scalar_focal_per_view_c=SCALAR_FOCAL)
_teeth = {}


def _measure(name):
    """(interior fraction, bf16 emulation rgb rms, {mutant: rgb rms of the change of the fp64 truth}) — once per case."""
    if name not in _teeth:
        case = TEETH[name]()
        spec, poses, maps = case["spec"], case["poses"], case["maps"]
        xyz, dirs = np.asarray(case["xyz"])[:, :MUTANT_POINTS], np.asarray(case["dirs"])[:, :MUTANT_POINTS]
        frac = fu.interior_fraction(spec, poses, case["xyz"], uv_scale=case["uv_scale"])
        truth = fu.truth_fp64(spec, poses, maps, xyz, dirs)
        emu = fu.emulate_16bit(spec, poses, maps, xyz, dirs, "bf16")
        moved = {m: fu._rms((fu.truth_fp64(ms, poses, maps, xyz, dirs) - truth)[..., :3])
                 for m, ms in fu.intrinsics_mutants(spec).items()}
        _teeth[name] = (frac, fu._rms((emu - truth)[..., :3]), moved)
    return _teeth[name]


@pytest.mark.parametrize("name", list(TEETH))
def test_cases_are_interior_and_every_intrinsics_mistake_moves_the_truth(name):
    frac, rms_emu, moved = _measure(name)
    bar = fu.MUTANT_FACTOR * fu.RMS_ALL_FACTOR * rms_emu
    print(f"\n{name}: interior {frac:.2f}, bf16 emulation rgb rms {rms_emu:.2e}, bar {bar:.2e}; "
          + "; ".join(f"{m} {d:.2e} ({d / (fu.RMS_ALL_FACTOR * rms_emu):.0f} x)" for m, d in moved.items()))
    assert frac >= pu.MIN_INTERIOR, frac
    assert set(moved) == EXPECTED_MUTANTS[name], sorted(moved)
    for m, d in moved.items():
        assert d >= bar, (m, d, bar)


# ----------------------------------------------------------------------------- the rules refuse a mutant
@pytest.mark.parametrize("fmt", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["sb1_ns1_proj", "sb3_ns2_per_object_general"])
def test_class_compare_rejects_every_mutant(name, fmt):
    """The fp64 truth under wrong intrinsics, handed to class_compare as the kernel's output."""
    case = fu.intr_case(name)
    a = (case["poses"], case["maps"], case["xyz"], case["dirs"])
    truth, emu = fu.truth_fp64(case["spec"], *a), fu.emulate_16bit(case["spec"], *a, fmt)
    cls = fu.point_classes(case["spec"], case["poses"], case["xyz"])
    fu.class_compare(emu, truth, emu, cls)
    for m, ms in fu.intrinsics_mutants(case["spec"]).items():
        with pytest.raises(AssertionError):
            fu.class_compare(fu.truth_fp64(ms, *a), truth, emu, cls, what=m)


def test_f32_compare_rejects_every_mutant():
    name = "intr_per_object"
    case = pu.make_case(name)
    truth, errs = pu.ensemble(name)
    cls = pu.f32_classes(case)
    a = (case["poses"], case["maps"], case["xyz"], case["dirs"])
    pu.leave_one_out(truth, errs, cls, what=name)
    for m, ms in fu.intrinsics_mutants(case["spec"]).items():
        with pytest.raises(AssertionError):
            pu.f32_compare(fu.emulate_16bit(ms, *a, "fp32"), truth, errs, cls, what=m)
