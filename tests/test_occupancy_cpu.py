"""Empty-space culling without a GPU: the three entry points' declarations and every argument check (all made before any
launch), the numpy models of tests/occupancy_util.py against independent brute forces — the build against a shifted maximum,
the traversal against 8192 fp64 samples per ray —, the compaction, planted mistakes that the same checks must reject, and the
refusals the Python layer makes before it touches a device."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import occupancy_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -4, -5
NAMES = ("pnr_occ_build", "pnr_ray_bounds_workspace_bytes", "pnr_ray_bounds", "pnr_frame_from_hits")


# ------------------------------------------------------------------------------------------------------------ the C surface
def test_prototypes_are_declared_bound_and_exported():
    from pixel_nerf_multiscale_amd import NeRFRenderer, _native as N, evalio, video
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    import inspect
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    assert "occupancy.hip" in __import__("pixel_nerf_multiscale_amd.build_native", fromlist=["SOURCES"]).SOURCES
    assert N.lib.pnr_version() == 102
    for name in ("OccupancyGrid", "ray_bounds", "frame_from_hits"):
        assert hasattr(occ, name), name
    assert hasattr(NeRFRenderer, "render_frames_bounded")
    for fn in (video.render_video, video.gen_video, evalio.evaluate):
        assert inspect.signature(fn).parameters["occupancy"].default is None, fn.__name__


def test_occ_build_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    p = 64

    def build(field=p, stride=1, nx=3, ny=4, nz=5, thresh=1.0, dilate=1, accumulate=0, bits=p):
        return N.lib.pnr_occ_build(field, stride, nx, ny, nz, thresh, dilate, accumulate, bits, None)

    assert build(field=None) == E_NULL and build(bits=None) == E_NULL
    for name in ("nx", "ny", "nz"):
        assert build(**{name: 1}) == E_SHAPE and build(**{name: -3}) == E_SHAPE, name
        assert build(**{name: 2 ** 20 + 2}) == E_SHAPE, name
    assert build(stride=0) == E_SHAPE and build(dilate=-1) == E_SHAPE and build(dilate=5) == E_SHAPE
    assert build(nx=2 ** 16, ny=2 ** 16, nz=2) == E_SHAPE            # 2^31 samples and more
    assert build(field=p + 2) == E_ALIGN and build(bits=p + 1) == E_ALIGN
    assert build(field=p + 2, nx=1) == E_SHAPE                        # sizes are judged before the alignment
    with pytest.raises(ValueError):
        N.check(build(dilate=9), "pnr_occ_build")


def test_ray_bounds_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p = 256
    box = dict(c1=(-1.0, -1.0, -1.0), c2=(1.0, 1.0, 1.0), cells=(4, 5, 6))

    def bounds(rays=p, n=12, R=4, c1=box["c1"], c2=box["c2"], cells=box["cells"], bits=p, pad=0.1, ws=p, ws_bytes=None,
               rays_out=p, slot=p, counts=p):
        ws_bytes = L.pnr_ray_bounds_workspace_bytes(n, R) if ws_bytes is None else ws_bytes
        arr = lambda t, v: None if v is None else (t * 3)(*v)
        return L.pnr_ray_bounds(rays, n, R, arr(C.c_double, c1), arr(C.c_double, c2), arr(C.c_int32, cells), bits, pad, ws, ws_bytes,
                                rays_out, slot, counts, None)

    for name in ("rays", "c1", "c2", "cells", "bits", "ws", "rays_out", "slot", "counts"):
        assert bounds(**{name: None}) == E_NULL, name
    assert L.pnr_ray_bounds_workspace_bytes(12, 4) >= 12 * 8 and L.pnr_ray_bounds_workspace_bytes(12, 5) == 0
    assert L.pnr_ray_bounds_workspace_bytes(-1, 1) == 0 and L.pnr_ray_bounds_workspace_bytes(4, 0) == 0
    assert L.pnr_ray_bounds_workspace_bytes(2 ** 31, 2 ** 31) == 0
    assert bounds(n=12, R=5, ws_bytes=4096) == E_SHAPE and bounds(n=-4, ws_bytes=4096) == E_SHAPE and bounds(R=0, ws_bytes=4096) == E_SHAPE
    assert bounds(cells=(0, 5, 6)) == E_SHAPE and bounds(cells=(4, 5, 2 ** 20 + 1)) == E_SHAPE
    assert bounds(c2=(1.0, -1.0, 1.0)) == E_SHAPE and bounds(c1=(float("nan"), -1.0, -1.0)) == E_SHAPE
    assert bounds(c2=(float("inf"), 1.0, 1.0)) == E_SHAPE and bounds(c1=(1.0, -1.0, -1.0), c2=(1.0 + 1e-12, 1.0, 1.0)) == E_SHAPE
    assert bounds(pad=-0.1) == E_SHAPE and bounds(pad=float("nan")) == E_SHAPE and bounds(pad=float("inf")) == E_SHAPE
    assert bounds(ws_bytes=L.pnr_ray_bounds_workspace_bytes(12, 4) - 1) == E_WORKSPACE
    for name in ("rays", "rays_out", "ws"):
        assert bounds(**{name: p + 8}) == E_ALIGN, name
    assert bounds(slot=p + 2) == E_ALIGN and bounds(counts=p + 4) == E_ALIGN and bounds(bits=p + 1) == E_ALIGN
    assert bounds(rays=p + 8, pad=-1.0) == E_SHAPE                    # sizes are judged before the alignment
    assert bounds(n=0, R=4) == 0                                      # nothing to do: no launch


def test_frame_from_hits_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    p = 64

    def gather(rec=p, rec_stride=4, slot=p, n=12, R=4, bg=1.0, out=p, out_stride=4):
        return N.lib.pnr_frame_from_hits(rec, rec_stride, slot, n, R, bg, out, out_stride, None)

    assert gather(rec=None) == E_NULL and gather(slot=None) == E_NULL and gather(out=None) == E_NULL
    assert gather(rec_stride=3) == E_SHAPE and gather(out_stride=0) == E_SHAPE
    assert gather(n=12, R=5) == E_SHAPE and gather(n=-1) == E_SHAPE and gather(R=0) == E_SHAPE
    assert gather(rec=p + 2) == E_ALIGN and gather(slot=p + 1) == E_ALIGN and gather(out=p + 3) == E_ALIGN
    assert gather(n=0) == 0


# ------------------------------------------------------------------------------------------------------------ the build model
def _sigma(shape, seed):
    rng = np.random.default_rng(seed)
    s = (rng.normal(size=shape) * 10.0).astype(np.float32)
    flat = s.reshape(-1)
    flat[rng.integers(0, flat.size, max(flat.size // 40, 1))] = np.nan
    flat[rng.integers(0, flat.size, max(flat.size // 40, 1))] = np.inf
    flat[rng.integers(0, flat.size, max(flat.size // 40, 1))] = -np.inf
    return s


def _build_rejects(sigma, thresh, dilate, mistake=None):
    """The build checks: the model's cells are the brute force's, and the words are the layout the header states."""
    cells = U.build_brute(sigma, thresh, dilate)
    words = U.build_model(sigma, thresh, dilate, mistake=mistake)
    cx, cy, cz = cells.shape
    wz = (cz + 31) // 32
    want = np.zeros(cx * cy * wz, dtype=np.uint32)
    for i, j, k in np.argwhere(cells):
        want[(i * cy + j) * wz + (k >> 5)] |= np.uint32(1) << np.uint32(k & 31)
    return not np.array_equal(words, want)


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_build_model_equals_the_shifted_maximum(dilate):
    for shape in ((2, 2, 2), (3, 5, 34), (7, 6, 9)):
        sigma = _sigma(shape, seed=shape[2])
        assert not _build_rejects(sigma, 14.0, dilate), shape
    # NaN and +Inf corners are hot, -Inf is not: one of each alone in a field of zeros
    for value, hot in ((np.nan, True), (np.inf, True), (-np.inf, False), (0.5, False), (1.0, True)):
        sigma = np.zeros((4, 4, 4), np.float32)
        sigma[2, 1, 3] = value
        cells = U.unpack_words(U.build_model(sigma, 1.0, 0), (3, 3, 3))
        want = np.zeros((3, 3, 3), bool)
        if hot:
            want[1:3, 0:2, 2:3] = True                                # the cells that have sample (2, 1, 3) as a corner
        assert np.array_equal(cells, want), value
    assert U.unpack_words(U.build_model(np.zeros((3, 3, 3), np.float32), -np.inf, 0), (2, 2, 2)).all()
    prev = U.build_model(_sigma((3, 5, 34), 1), 14.0, 0)
    both = U.build_model(_sigma((3, 5, 34), 2), 14.0, 1, prev=prev)
    assert np.array_equal(both, prev | U.build_model(_sigma((3, 5, 34), 2), 14.0, 1))


@pytest.mark.parametrize("cz", [1, 31, 32, 33, 64])
def test_bit_layout(cz):
    from pixel_nerf_multiscale_amd.render.occupancy import OccupancyGrid
    rng = np.random.default_rng(cz)
    cells = rng.random((2, 3, cz)) < 0.5
    cells[1, 2, cz - 1] = True
    words = U.pack_cells(cells)
    wz = (cz + 31) // 32
    assert words.shape == (2 * 3 * wz,)
    for i, j, k in np.ndindex(2, 3, cz):
        assert bool(words[(i * 3 + j) * wz + (k >> 5)] >> np.uint32(k & 31) & np.uint32(1)) == bool(cells[i, j, k])
    if cz % 32:                                                       # the padding bits are zero
        assert not (words.reshape(2, 3, wz)[:, :, -1] >> np.uint32(cz % 32)).any()
    assert np.array_equal(U.unpack_words(words, cells.shape), cells)
    grid = OccupancyGrid.from_cells(torch.from_numpy(cells), (-1, -1, -1), (1, 1, 1))          # the host packing of the package
    assert np.array_equal(grid.bits.numpy().view(np.uint32), words) and torch.equal(grid.cells(), torch.from_numpy(cells))
    assert grid.reso == (3, 4, cz + 1) and abs(grid.occupied_fraction() - cells.mean()) < 1e-6
    sigma = np.zeros((3, 4, cz + 1), np.float32)                      # and the build model at this size
    sigma[1, 2, cz] = 2.0
    assert not _build_rejects(sigma, 1.0, 0) and not _build_rejects(sigma, 1.0, 1)


# ------------------------------------------------------------------------------------------------------------ the traversal model
@pytest.fixture(scope="module")
def brute():
    """The brute force of every case grid on the shared rays, computed once."""
    rays = U.case_rays()
    return rays, {name: (cells, U.brute_force(rays, *U.BOX, cells)) for name, cells in U.case_grids().items()}


def _traversal_failures(rays, cells, samples, mistake=None, pad=0.0):
    """The traversal checks of one grid -> list of (ray, what failed)."""
    hit, near2, far2 = U.trace_model(rays, *U.BOX, cells, pad, mistake)
    bad = []
    r = rays.astype(np.float64)
    slack = pad * (1.0 - 1e-3)
    for i, (ts, _) in enumerate(samples):
        if len(ts):
            if not hit[i]:
                bad.append((i, "a ray with a counted sample is a miss"))
                continue
            if not (near2[i] <= ts.min() and ts.max() <= far2[i]):
                bad.append((i, "a counted sample outside [near', far']"))
            if pad > 0.0 and not (near2[i] <= max(r[i, 6], ts.min() - slack) and far2[i] >= min(r[i, 7], ts.max() + slack)):
                bad.append((i, "pad missing at an end"))
        if hit[i] and not (r[i, 6] <= near2[i] <= far2[i] <= r[i, 7]):
            bad.append((i, "bounds outside the ray's own"))
    idx = np.nonzero(hit)[0]
    if pad == 0.0 and len(idx):
        for t, what in ((near2, "t_in"), (far2, "t_out")):
            pts = r[idx, 0:3] + t[idx, None].astype(np.float64) * r[idx, 3:6]
            far_off = U.distance_to_occupied(pts, *U.BOX, cells) > U.EXCLUDE
            bad += [(int(i), f"the point at {what} is not at an occupied cell") for i in idx[far_off]]
    return bad


@pytest.mark.parametrize("grid_name", ["shell", "single", "full", "empty"])
def test_traversal_model_against_the_brute_force(brute, grid_name):
    rays, cases = brute
    cells, samples = cases[grid_name]
    assert _traversal_failures(rays, cells, samples) == []
    assert _traversal_failures(rays, cells, samples, pad=0.06) == []
    in_cell = sum(n for _, n in samples)
    counted = sum(len(ts) for ts, _ in samples)
    if grid_name == "empty":
        assert in_cell == 0 and not U.trace_model(rays, *U.BOX, cells, 0.0)[0].any()
    else:
        print(f"{grid_name}: {in_cell} in-cell samples, {in_cell - counted} dropped by the {U.EXCLUDE} exclusion")
        assert in_cell > 0 and in_cell - counted <= 0.01 * in_cell    # the brute force alone stays inside its budget
    hit = U.trace_model(rays, *U.BOX, cells, 0.0)[0]
    assert not hit[-5:].any()                                         # no direction, near > far, NaN, Inf, far in front of the box
    if grid_name == "full":
        r = rays.astype(np.float64)
        grazing = len(rays) - 10
        assert hit[grazing] and hit[grazing + 1] and not hit[grazing + 2]        # on the face, inside it, outside it
        assert hit[grazing + 4]
        with np.errstate(invalid="ignore"):
            start = np.abs(r[:, 0:3] + r[:, 6:7] * r[:, 3:6])
        inside = np.nonzero((start < 1).all(axis=1) & np.isfinite(r).all(axis=1) & hit)[0]
        near2 = U.trace_model(rays, *U.BOX, cells, 0.0)[1]
        assert len(inside) >= 40 and np.array_equal(near2[inside], rays[inside, 6])          # a start inside an occupied cell


def test_compaction_model():
    cells = U.case_grids()["shell"]
    base = U.case_rays(seed=3)
    R, F = 70, 3                                                      # frame boundaries at 70, 140: no multiples of 64
    rays = np.ascontiguousarray(np.tile(base, (2, 1))[:R * F])
    rows, slot, counts = U.bounds_model(rays, R, *U.BOX, cells, 0.0)
    hit, near2, far2 = U.trace_model(rays, *U.BOX, cells, 0.0)
    assert counts.dtype == np.int64 and slot.dtype == np.int32 and counts.tolist() == [int(hit[f * R:(f + 1) * R].sum()) for f in range(F)]
    assert 0 < counts.min() and counts.max() < R
    for f in range(F):
        mine = slot[f * R:(f + 1) * R]
        assert np.array_equal(mine[mine >= 0], np.arange(counts[f]))  # ascending within the frame, from 0
        assert np.array_equal(mine >= 0, hit[f * R:(f + 1) * R])
        idx = np.nonzero(mine >= 0)[0] + f * R
        assert np.array_equal(rows[f][:, :6], rays[idx, :6]) and np.array_equal(rows[f][:, 6], near2[idx])
        assert np.array_equal(rows[f][:, 7], far2[idx])
    rec = np.random.default_rng(0).normal(size=(R * F, 5)).astype(np.float32)
    frame = U.frame_model(rec, slot, R, 1.0)
    assert (frame[slot < 0] == np.array([1, 1, 1, 0], np.float32)).all()
    assert np.array_equal(frame[R + idx_of(slot, R, 1)], rec[R:R + counts[1], :4])


def idx_of(slot, R, f):
    return np.nonzero(slot[f * R:(f + 1) * R] >= 0)[0]


# ------------------------------------------------------------------------------------------------------------ planted mistakes
@pytest.mark.parametrize("mistake", ["last_cell_dropped", "negative_as_positive", "pad_one_end"])
def test_traversal_checks_reject_planted_mistakes(brute, mistake):
    rays, cases = brute
    failures = sum(len(_traversal_failures(rays, cells, samples, mistake, pad=0.06 if mistake == "pad_one_end" else 0.0))
                   for cells, samples in cases.values())
    assert failures > 0


@pytest.mark.parametrize("mistake", ["dilate_skips_axis", "bit_reversed"])
def test_build_checks_reject_planted_mistakes(mistake):
    sigma = _sigma((3, 5, 34), seed=34)
    assert _build_rejects(sigma, 14.0, 1, mistake)


# ------------------------------------------------------------------------------------------------------------ refusals
def _cpu_grid():
    from pixel_nerf_multiscale_amd.render.occupancy import OccupancyGrid
    return OccupancyGrid.from_cells(torch.ones(2, 2, 2, dtype=torch.bool), (-1, -1, -1), (1, 1, 1))


def test_sigma_thresh_is_required_and_several_objects_are_refused(tmp_path):
    from pixel_nerf_multiscale_amd import NeRFRenderer, evalio, video
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    net = torch.nn.Linear(2, 2)
    with pytest.raises(TypeError, match="sigma_thresh"):
        occ.OccupancyGrid.from_net(net)
    with pytest.raises(TypeError, match="sigma_thresh"):
        occ.resolve(dict(reso=8), net)
    with pytest.raises(TypeError, match="sigma_thresh"):
        evalio.evaluate(net, None, [], str(tmp_path / "out"), occupancy=dict(reso=8))
    with pytest.raises(TypeError):
        evalio.evaluate(net, None, [], str(tmp_path / "out"), occupancy=_cpu_grid())       # one grid per object: a dict
    with pytest.raises(TypeError):
        occ.resolve(3.0, net)
    assert not os.path.exists(tmp_path / "out")
    net.num_objs = 2
    with pytest.raises(ValueError, match="one encoded object"):
        occ.OccupancyGrid.from_net(net, sigma_thresh=1.0)
    with pytest.raises(ValueError, match="one encoded object"):
        NeRFRenderer().render_frames_bounded(net, torch.eye(4)[None], 4, 4, 3.0, 1.0, 2.0, _cpu_grid())
    with pytest.raises(TypeError):
        NeRFRenderer().render_frames_bounded(net, torch.eye(4)[None], 4, 4, 3.0, 1.0, 2.0, dict(sigma_thresh=1.0))
    with pytest.raises(ValueError):
        occ.OccupancyGrid.from_cells(torch.ones(2, 2, dtype=torch.bool), (-1, -1, -1), (1, 1, 1))
    with pytest.raises(ValueError):
        occ.OccupancyGrid.from_cells(torch.ones(2, 2, 2, dtype=torch.bool), (-1, -1, -1), (1, -1, 1))
    with pytest.raises(RuntimeError):
        occ.ray_bounds(_cpu_grid(), torch.zeros(4, 8))                # host tensors: there is no CPU fall-back
    with pytest.raises(ValueError):
        occ.ray_bounds(_cpu_grid(), torch.zeros(4, 7))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, root, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pixel_nerf_multiscale_amd import evalio, video
        msgs = []
        calls = (lambda: evalio.evaluate(None, None, [], os.path.join(root, "eval"), occupancy=dict(sigma_thresh=1.0)),
                 lambda: video.render_video(None, None, torch.eye(4)[None], 4, 4, 3.0, 1.0, 2.0, occupancy=dict(sigma_thresh=1.0)),
                 lambda: video.gen_video(None, None, {}, os.path.join(root, "video"), [0], z_near=1.0, z_far=2.0,
                                         occupancy=dict(sigma_thresh=1.0)))
        for call in calls:
            try:
                call()
                msgs.append("no error")
            except ValueError as e:
                msgs.append(str(e))
        q.put((rank, msgs))
    finally:
        dist.destroy_process_group()


def test_occupancy_under_two_ranks_is_refused_before_anything_is_written(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r for r, _ in res) == [0, 1]
    for _, msgs in res:
        assert len(msgs) == 3 and all("occupancy" in m and "2 ranks" in m for m in msgs), msgs
    assert os.listdir(tmp_path) == []
