"""Procedural datasets without a GPU: the float32 model of include/pnr.h's section (tests/synth_util.py) against an independent
fp64 analytic ray cast, the surface residual of its depth under util.gen_rays' own rays, planted mistakes that these checks must
reject, and the host side — random_scenes, view_poses, write_srn_tree read back through SRNDataset, util.synth_render's
argument contract."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth_util as su  # noqa: E402

from pixel_nerf_multiscale_amd import util  # noqa: E402
from pixel_nerf_multiscale_amd.data import SRNDataset, get_split_dataset, synthetic  # noqa: E402

W = H = 32
FOCAL = 40.0
CX = CY = 16.0
NAMES = ("sphere", "box", "two")
MARGIN = 1e-4             # the issue's: a pixel may be left out only where the fp64 discriminant or slab gap is below this
DEPTH_REL = 1e-5
SURFACE = 1e-4
# Colour: within 1 byte everywhere (the issue's bound).  Tighter, from the formats: where the fp64 value w = mean * 255 + 0.5 is
# further than W_EPS from an integer, the fp32 byte must EQUAL the fp64 byte.  The model's w carries a few dozen fp32 roundings of
# O(1) quantities times 255 (the saturating albedo 1.7 included): 255 * 1.7 * 30 * 6e-8 < 1e-3; W_EPS doubles that.
W_EPS = 2e-3


@functools.lru_cache(maxsize=None)
def _frames(ss):
    """(scene ids, poses) of the comparison: every named scene under the three cameras of the issue."""
    poses = su.issue_poses()
    ids = np.repeat(np.arange(3), 3)
    return ids, np.concatenate([poses] * 3)


@functools.lru_cache(maxsize=None)
def _reference(ss):
    ids, poses = _frames(ss)
    return su.reference_render(su.named_scenes(), ids, poses, W, H, FOCAL, FOCAL, CX, CY, ss=ss)


@functools.lru_cache(maxsize=None)
def _model(ss, mistake=None):
    ids, poses = _frames(ss)
    return su.model_render(su.named_scenes(), ids, poses, W, H, FOCAL, FOCAL, CX, CY, ss=ss, mistake=mistake)


def _surface_residual(depth):
    """max |implicit function| of the hit primitive at o + depth * d, d from util.gen_rays, over the finite depths (ss = 1)."""
    ids, poses = _frames(1)
    ref = _reference(1)
    rays = util.gen_rays(torch.from_numpy(poses), W, H, FOCAL, 0.8, 1.8, c=torch.tensor([CX, CY])).numpy().astype(np.float64)
    worst = 0.0
    for f in range(len(ids)):
        keep = np.isfinite(depth[f]) & (ref["margin"][f] >= MARGIN) & (ref["winner"][f] >= 0)
        pts = rays[f, ..., :3] + np.where(keep, depth[f], 0.0)[..., None].astype(np.float64) * rays[f, ..., 3:6]
        for p in np.unique(ref["winner"][f][keep]):
            sel = keep & (ref["winner"][f] == p)
            worst = max(worst, float(np.abs(su.implicit(su.named_scenes(), ids[f], p, pts[sel])).max()))
    return worst


def _failures(ss, mistake=None):
    """Every way in which the model's frames (with a planted mistake, if any) miss the fp64 ray cast: a list of strings."""
    rgb, mask, depth = _model(ss, mistake)
    ref = _reference(ss)
    keep = ref["margin"] >= MARGIN
    bad = []
    excluded = 1.0 - keep.mean()
    if excluded > 0.01:
        bad.append(f"ss {ss}: {excluded:.4f} of the pixels excluded, above 1 %")
    if not np.array_equal((mask != 0)[keep], ref["mask"][keep]):
        bad.append(f"ss {ss}: masks differ at {int(((mask != 0) != ref['mask'])[keep].sum())} pixels")
    if not np.array_equal(np.isin(mask, (0, 255)), np.ones_like(mask, dtype=bool)):
        bad.append(f"ss {ss}: a mask byte that is neither 0 nor 255")
    if not np.array_equal((rgb != 255).all(-1)[keep], ref["mask"][keep]):
        bad.append(f"ss {ss}: SRNDataset's rule (img != 255).all(-1) does not read the mask back from the bytes")
    hit = keep & np.isfinite(ref["depth"])
    if not np.array_equal(np.isfinite(depth)[keep], np.isfinite(ref["depth"])[keep]):
        bad.append(f"ss {ss}: depth finite where the reference misses, or the other way round")
    else:
        rel = np.abs(depth[hit] - ref["depth"][hit]) / ref["depth"][hit]
        if rel.size and rel.max() > DEPTH_REL:
            bad.append(f"ss {ss}: depth off by {rel.max():.3g} relative")
        if not np.all(np.isposinf(depth[keep & ~np.isfinite(ref["depth"])])):
            bad.append(f"ss {ss}: a missed first sub-sample without depth +inf")
    diff = np.abs(rgb.astype(np.int64) - ref["rgb"].astype(np.int64))
    if diff[keep].max() > 1:
        bad.append(f"ss {ss}: colour off by {int(diff[keep].max())} bytes")
    off_tie = np.abs(ref["value"] - np.round(ref["value"])) > W_EPS
    if (diff[keep[..., None] & off_tie] != 0).any():
        bad.append(f"ss {ss}: {int((diff[keep[..., None] & off_tie] != 0).sum())} bytes differ away from a rounding tie")
    if ss == 1:
        worst = _surface_residual(depth)
        if worst > SURFACE:
            bad.append(f"surface residual {worst:.3g}")
    return bad


@pytest.mark.parametrize("ss", [1, 2])
def test_model_against_fp64(ss):
    """The issue's cases are ss = 1: three scenes, three cameras, 32 x 32, f = 40.  ss = 2 adds the mean over the sub-samples,
    the any-hit mask and the clamp, on the same frames."""
    ref = _reference(ss)
    for s, name in enumerate(NAMES):
        m = ref["margin"][3 * s:3 * s + 3]
        print(f"ss {ss} {name}: excluded share {(m < MARGIN).mean():.5f}, foreground share {ref['mask'][3 * s:3 * s + 3].mean():.3f}")
        assert ref["mask"][3 * s:3 * s + 3].any(axis=(1, 2)).all(), name
    rgb, mask, depth = _model(ss)
    hit = np.isfinite(ref["depth"]) & (ref["margin"] >= MARGIN) & np.isfinite(depth)
    print(f"ss {ss}: worst depth error {np.max(np.abs(depth[hit] - ref['depth'][hit]) / ref['depth'][hit]):.3g} relative, "
          f"{int((np.abs(rgb.astype(int) - ref['rgb'].astype(int)) != 0).sum())} bytes differ")
    assert _failures(ss) == []
    assert (ref["rgb"][..., 0][ref["mask"]] == 254).any() or ss == 1, "the saturating albedo never reached the clamp"


def test_sphere_and_box_exclude_nothing():
    """The issue's own figure: for the sphere and the box at these cameras no pixel falls under the margin, so the cap of 1 % is
    met by the reference alone."""
    assert (_reference(1)["margin"][:6] >= MARGIN).all()


def test_surface_residual():
    worst = _surface_residual(_model(1)[2])
    print(f"worst surface residual {worst:.3g} (bound {SURFACE})")
    assert worst <= SURFACE


@pytest.mark.parametrize("mistake", su.MISTAKES)
def test_planted_mistakes_are_rejected(mistake):
    bad = _failures(1, mistake) + _failures(2, mistake)
    print(mistake, "->", bad)
    assert bad, f"the checks accept the planted mistake {mistake!r}"


# ------------------------------------------------------------------------------------------- the host side
def test_random_scenes():
    a = synthetic.random_scenes(12, 3, "train", max_prims=4)
    assert a.dtype == np.float32 and a.shape == (12, 4, synthetic.REC)
    assert np.array_equal(a, synthetic.random_scenes(12, 3, "train", max_prims=4))               # determinism
    assert np.array_equal(a[:5], synthetic.random_scenes(5, 3, "train", max_prims=4))            # object i does not depend on n
    assert not np.array_equal(a, synthetic.random_scenes(12, 4, "train", max_prims=4))
    stages = [synthetic.random_scenes(12, 3, s) for s in ("train", "val", "test")]
    keys = [{r.tobytes() for r in s} for s in stages]
    assert all(len(k) == 12 for k in keys) and not (keys[0] & keys[1]) and not (keys[0] & keys[2]) and not (keys[1] & keys[2])
    d = a.astype(np.float64)
    kind = d[..., 0]
    assert np.isin(kind, (0, 1, 2)).all() and (kind != 0).any(axis=1).all()                      # at least one primitive
    present = kind != 0
    reach = np.linalg.norm(d[..., 1:4], axis=-1) + np.linalg.norm(d[..., 13:16], axis=-1)
    assert (reach[present] <= 0.5).all()
    assert (d[..., 13:16][present] > 0).all()
    alb = a[..., 16:19][present]
    assert (alb >= np.float32(0.1)).all() and (alb <= np.float32(0.9)).all() and (d[..., 16:19][present] >= 0.1 - 1e-8).all()
    R = d[..., 4:13][present].reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and np.allclose(np.linalg.det(R), 1.0, atol=1e-6)
    assert (a[~present] == 0).all()
    assert {1.0, 2.0} <= set(np.unique(synthetic.random_scenes(40, 0)[..., 0]))                  # both kinds occur
    assert synthetic.random_scenes(2, 0, max_prims=8).shape == (2, 8, synthetic.REC)
    with pytest.raises(ValueError):
        synthetic.random_scenes(2, 0, max_prims=9)
    with pytest.raises(ValueError):
        synthetic.random_scenes(2, 0, stage="other")


@pytest.mark.parametrize("stage", ["train", "val", "test"])
def test_view_poses(stage):
    p = synthetic.view_poses(20, 5, stage, 2)
    assert p.dtype == np.float32 and p.shape == (20, 4, 4)
    assert np.array_equal(p, synthetic.view_poses(20, 5, stage, 2))
    d = p.astype(np.float64)
    R, t = d[:, :3, :3], d[:, :3, 3]
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() < 1e-6 and np.allclose(np.linalg.det(R), 1.0, atol=1e-6)
    assert np.allclose(np.linalg.norm(t, axis=-1), 1.3, atol=1e-6)
    assert np.array_equal(d[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (20, 1)))
    # the camera looks down its -z: the central ray of util.gen_rays passes through the origin
    rays = util.gen_rays(torch.from_numpy(p), 3, 3, 2.0, 0.8, 1.8, c=torch.tensor([1.0, 1.0]))[:, 1, 1].double().numpy()
    assert np.abs(np.cross(rays[:, :3], rays[:, 3:6])).max() < 1e-6 and ((rays[:, :3] * rays[:, 3:6]).sum(-1) < -1.29).all()
    if stage == "test":
        assert np.array_equal(p, synthetic.view_poses(20, 99, stage, 7))                         # a deterministic spiral
        assert (t[:, 2] > 0).all() and (np.diff(t[:, 2]) > 0).all()
    else:
        assert not np.array_equal(p, synthetic.view_poses(20, 5, stage, 3))
        assert (t[:, 2] < 0).any() and (t[:, 2] > 0).any()                                       # the whole sphere


def _model_item(sid, name):
    """A byte item of SRNDataset's form made by the model (ss = 2) from a named scene."""
    poses = su.issue_poses()
    rgb, mask, _ = su.model_render(su.named_scenes(), [sid] * 3, poses, W, H, FOCAL, FOCAL, CX, CY, ss=2)
    return {"path": f"synthetic/train/{name}", "img_id": sid, "focal": FOCAL, "c": torch.tensor([CX, CY]),
            "images": torch.from_numpy(rgb), "masks": torch.from_numpy(mask), "poses": torch.from_numpy(poses)}


def test_write_srn_tree_reads_back_exactly(tmp_path):
    items = [_model_item(s, f"{s:06d}") for s in range(3)]
    root = synthetic.write_srn_tree(items, str(tmp_path / "shapes"), "train")
    assert root == str(tmp_path / "shapes") + "_train"
    back = SRNDataset(str(tmp_path / "shapes"), stage="train", as_bytes=True)
    assert len(back) == 3 and (back.z_near, back.z_far) == (0.8, 1.8)
    for item, got in zip(items, (back[i] for i in range(3))):
        assert got["focal"] == item["focal"] and torch.equal(got["c"], item["c"])
        assert torch.equal(got["images"], item["images"]) and torch.equal(got["masks"], item["masks"])
        assert torch.equal(got["poses"], item["poses"])
        m = item["masks"].numpy() != 0
        for v in range(3):
            rows, cols = np.flatnonzero(m[v].any(1)), np.flatnonzero(m[v].any(0))
            assert got["bbox"][v].tolist() == [cols[0], rows[0], cols[-1], rows[-1]]
    with pytest.raises(ValueError):
        synthetic.write_srn_tree([dict(items[0], images=items[0]["images"].float())], str(tmp_path / "floats"), "train")


def test_get_split_dataset_synthetic_counts():
    train, val, test = get_split_dataset("synthetic", None, n_objects=20, n_views=3, image_size=16, device="cpu")
    assert (len(train), len(val), len(test)) == (20, 2, 2)
    assert [d.stage for d in (train, val, test)] == ["train", "val", "test"]
    assert len(get_split_dataset("synthetic", None, want_split="val", n_objects=4, device="cpu")) == 1
    one = get_split_dataset("synthetic", None, want_split="test", n_objects=4, n_test=3, as_bytes=True, device="cpu")
    assert len(one) == 3 and one.as_bytes and one.balanced and not one.lindisp and (one.z_near, one.z_far) == (0.8, 1.8)
    assert one.focal == 131.25 and get_split_dataset("synthetic", None, "train", n_objects=1, image_size=64, device="cpu").focal == 65.625
    with pytest.raises(ValueError):
        get_split_dataset("synthetic", None)


def test_synth_render_argument_contract_on_host_tensors():
    """DESIGN.md's order: what is wrong with an argument by itself is a ValueError, a given output included; well-formed host
    tensors reach same_device, which raises RuntimeError."""
    scenes = torch.from_numpy(su.named_scenes())
    ids = torch.tensor([0, 1], dtype=torch.int32)
    poses = torch.from_numpy(su.issue_poses()[:2])
    with pytest.raises(RuntimeError, match="HIP device"):
        util.synth_render(scenes, ids, poses, 8, 8, 10.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        util.synth_render(scenes, ids, poses, 8, 8, 10.0, out=torch.empty(2, 8, 8, 3, dtype=torch.uint8), mask_out=True,
                          depth_out=torch.empty(2, 8, 8))
    bad = [dict(scenes=scenes.double()), dict(scenes=scenes[..., :19]), dict(scenes=scenes[0]), dict(scene_ids=ids.long()),
           dict(scene_ids=ids[None]), dict(poses=poses[:1]), dict(poses=poses.double()), dict(poses=poses[:, :3]), dict(W=0),
           dict(H=-1), dict(out=torch.empty(2, 8, 8, 3)), dict(out=torch.empty(2, 8, 8, 4, dtype=torch.uint8)),
           dict(out=torch.empty(2, 8, 8, 6, dtype=torch.uint8)[..., ::2]), dict(mask_out=torch.empty(2, 8, 8)),
           dict(mask_out=torch.empty(2, 8, 9, dtype=torch.uint8)), dict(depth_out=torch.empty(2, 8, 8, dtype=torch.float64)),
           dict(depth_out=torch.empty(2, 8, 16)[..., ::2]), dict(light=(1.0, 0.0)), dict(scenes=None)]
    for change in bad:
        kw = dict(scenes=scenes, scene_ids=ids, poses=poses, W=8, H=8, focal=10.0)
        kw.update(change)
        with pytest.raises(ValueError):
            util.synth_render(**kw)


def test_entry_point_refusals_come_before_any_launch():
    """Every refusal of pnr_synth_render is a host-side check made before the launch, so the addresses are never read: the
    sizes the wrapper could only reach with gigabytes of tensors (F H W >= 2^31) are tried here, on made-up aligned addresses."""
    from pixel_nerf_multiscale_amd import _native as N
    a = 1 << 20
    good = dict(scenes=a, n=3, P=4, ids=a, poses=a, F=2, W=8, H=8, fx=10.0, fy=10.0, cx=4.0, cy=4.0, ss=2, ambient=0.3, lx=0.3, ly=0.5,
                lz=0.8, rgb=a, stride=192, mask=None, depth=None)

    def rc(**change):
        return N.lib.pnr_synth_render(*dict(good, **change).values(), None)

    for change in (dict(scenes=None), dict(ids=None), dict(poses=None), dict(rgb=None)):
        assert rc(**change) == -1, change
    for change in (dict(P=9), dict(P=0), dict(n=-1), dict(F=0), dict(W=0), dict(H=-3), dict(ss=3), dict(ss=8), dict(stride=191),
                   dict(F=1 << 15, W=1 << 8, H=1 << 8, stride=3 << 16), dict(W=1 << 16, H=1 << 15, F=1, stride=3 << 31),
                   dict(F=(1 << 31) - 1, W=1, H=1, stride=3), dict(fx=0.0), dict(fy=float("inf")), dict(cx=float("nan")),
                   dict(ambient=1.0001), dict(ambient=-1e-9), dict(ambient=float("nan")), dict(lx=0.0, ly=0.0, lz=0.0),
                   dict(lx=float("nan"))):
        assert rc(**change) == -2, change
    for change in (dict(scenes=a + 2), dict(ids=a + 1), dict(poses=a + 3), dict(depth=a + 2)):
        assert rc(**change) == -5, change
    with pytest.raises(ValueError, match="pnr_synth_render"):
        N.check(rc(P=9), "pnr_synth_render")
    assert N.PNR_SYNTH_MAX_PRIMS == synthetic.MAX_PRIMS == 8 and N.PNR_SYNTH_REC == synthetic.REC == su.REC
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "pnr.h")).read()
    assert "#define PNR_SYNTH_MAX_PRIMS 8" in hdr and "#define PNR_SYNTH_REC 20" in hdr
