"""Mesh extraction, host side: the derived case table and the committed header, the CPU oracle on fields that meet every
case, the reference's own grid / scaling / OBJ arithmetic (tests/golden/recon_wrapper.npz, save_obj_*.obj, written by
tools/gen_golden_recon.py from the reference's recon.py), and every argument check of the four entry points (all made
before any launch, so they run without a GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mc_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
E_NULL, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -4, -5
gen = M._gen


def test_generated_table_equals_committed_header():
    assert open(gen.HEADER).read() == gen.header_text()


def test_table_properties():
    table = gen.build_table()
    assert len(table) == 256 and max(len(t) for t in table) <= 5 and sum(len(t) for t in table) == 820
    assert table[0] == [] and table[255] == []
    n_loops = 0
    for mask in range(256):
        loops = gen.loops_of(mask)                       # asserts inside: the segments form closed loops over the crossed edges
        crossed = {e for e, (a, b) in enumerate(gen.EDGE_CORNERS) if ((mask >> a) ^ (mask >> b)) & 1}
        assert sorted(e for l in loops for e in l) == sorted(crossed)
        assert all(len(l) >= 3 for l in loops)
        assert len(table[mask]) == sum(len(l) - 2 for l in loops)
        n_loops += len(loops)
        # no triangle side that is a fan diagonal joins two edges of a common cube face; loop sides always do
        for loop in loops:
            sides = {frozenset((loop[i], loop[(i + 1) % len(loop)])) for i in range(len(loop))}
            members = set(loop)
            for tri in table[mask]:
                if set(tri) <= members:
                    for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[2], tri[0])):
                        if frozenset((a, b)) not in sides:
                            assert not gen.edges_share_face(a, b), (mask, tri)
    assert sum(gen.rotation_census()) == n_loops


def test_single_corner_case_points_outward():
    # corner 0 inside: the triangle over edges 0, 4, 8 (the three edges at corner 0) has its normal pointing away from corner 0
    (tri,) = gen.build_table()[1]
    mid = {0: (0.5, 0, 0), 4: (0, 0.5, 0), 8: (0, 0, 0.5)}
    a, b, c = (np.array(mid[e]) for e in tri)
    assert np.dot(np.cross(b - a, c - a), np.ones(3)) > 0


@pytest.mark.parametrize("n", [16, 18, 22])
def test_oracle_noise_is_a_closed_oriented_manifold(n):
    v, t, met = M.marching_cubes(M.noise_field(n), 0.0)
    if n == 16:
        assert len(met) == 256                           # every case occurs
    assert len(t) > 0 and t.dtype == np.int32 and v.dtype == np.float64
    chi = M.check_closed_manifold(v, t)
    assert chi % 2 == 0                                  # closed orientable surfaces
    assert M.signed_volume(v, t) > 0


@pytest.mark.parametrize("n,tol", [(20, 0.02), (39, 0.005)])
def test_oracle_sphere(n, tol):
    v, t, _ = M.marching_cubes(M.sphere_field(n), 0.0)
    assert M.check_closed_manifold(v, t) == 2
    s = 2.0 / (n - 1)
    vol = M.signed_volume(M.scale_vertices(v, (s, s, s), (-1, -1, -1)), t)
    exact = 4.0 * np.pi * 0.7 ** 3 / 3.0
    print(f"sphere n={n}: volume error {(vol - exact) / exact:+.4%}")
    assert vol > 0 and abs(vol - exact) / exact <= tol


def test_oracle_nan_is_outside_and_ties_are_inside():
    f = np.full((3, 3, 3), -1.0, dtype=np.float32)
    f[1, 1, 1] = 0.0                                     # exactly on the level: inside
    v, t, _ = M.marching_cubes(f, 0.0)
    assert len(v) == 6 and len(t) == 8 and M.check_closed_manifold(v, t) == 2
    f[1, 1, 1] = np.nan
    v, t, _ = M.marching_cubes(f, 0.0)
    assert len(v) == 0 and len(t) == 0


def test_gen_grid_and_reference_scaling_equal_the_fixture():
    import torch
    from pixel_nerf_multiscale_amd import util
    fx = np.load(os.path.join(GOLDEN, "recon_wrapper.npz"))
    c1, c2, reso = fx["c1"].tolist(), fx["c2"].tolist(), fx["reso"].tolist()
    assert tuple(reso) == (6, 5, 4) and fx["chunks"].tolist() == [50, 50, 20]
    grid = util.gen_grid(*zip(c1, c2, reso), ij_indexing=True)
    assert grid.dtype == torch.float32 and np.array_equal(grid.numpy().view(np.uint32), fx["xyz"].view(np.uint32))
    # ij layout: the volume handed to the extractor is the (6, 5, 4) reshape of the per-point sigmas
    assert fx["volume"].shape == (6, 5, 4)
    # the default "xy" order of the reference swaps the first two axes
    gxy = util.gen_grid((0, 1, 2), (0, 1, 3)).numpy()
    assert gxy.shape == (6, 2) and np.array_equal(gxy[:, 0], [0, 1, 0, 1, 0, 1]) and np.array_equal(gxy[:, 1], [0, 0, .5, .5, 1, 1])
    # the oracle on the reference's volume, then the reference's scaling (c2 - c1) / reso and shift, bit for bit
    v, t, _ = M.marching_cubes(fx["volume"], float(fx["iso"]))
    assert np.array_equal(t, fx["triangles"]) and np.array_equal(v, fx["vertices_index"])
    final = M.scale_vertices(v, (fx["c2"] - fx["c1"]) / fx["reso"], fx["c1"])
    assert np.array_equal(final.view(np.uint64), fx["vertices"].view(np.uint64))
    # fake view directions: -p / |p|, unit length
    d = fx["viewdirs"]
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-6)
    assert np.allclose(d, -fx["xyz"] / np.linalg.norm(fx["xyz"], axis=-1, keepdims=True), atol=1e-6)


def test_save_obj_equals_the_reference_bytes(tmp_path):
    from pixel_nerf_multiscale_amd import recon
    mesh = np.load(os.path.join(GOLDEN, "save_obj_mesh.npz"))
    for name, rgb in (("save_obj_plain.obj", None), ("save_obj_rgb.obj", mesh["rgb"])):
        out = tmp_path / name
        recon.save_obj(mesh["vertices"], mesh["triangles"], str(out), vert_rgb=rgb)
        assert out.read_bytes() == open(os.path.join(GOLDEN, name), "rb").read(), name
    with pytest.raises(ValueError):
        recon.save_obj(mesh["vertices"], mesh["triangles"], str(tmp_path / "x.obj"), vert_rgb=mesh["rgb"][:3])


def test_prototypes_are_declared_bound_and_exported():
    import pixel_nerf_multiscale_amd as pkg
    from pixel_nerf_multiscale_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("pnr_grid_points", "pnr_mc_workspace_bytes", "pnr_mc_count", "pnr_mc_emit"):
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    assert "mesh.hip" in __import__("pixel_nerf_multiscale_amd.build_native", fromlist=["SOURCES"]).SOURCES
    assert N.lib.pnr_version() == 102
    assert all(hasattr(pkg.recon, n) for n in ("marching_cubes", "save_obj", "vertex_colors", "extract_mesh"))
    assert hasattr(pkg.util, "gen_grid") and hasattr(pkg.util, "gen_grid_device")


def test_mc_workspace_bytes():
    from pixel_nerf_multiscale_amd import _native as N
    wb = N.lib.pnr_mc_workspace_bytes
    assert wb(2, 2, 2) > 0 and wb(2, 2, 2) == wb(8, 8, 16)             # one workgroup of 1024 points either way
    assert wb(8, 8, 16) < wb(8, 8, 17) == wb(16, 16, 8)
    sizes = [wb(n, n, n) for n in (2, 10, 11, 16, 24, 64, 128, 129)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert wb(5, 6, 7) == wb(7, 5, 6)
    n = 128 ** 3
    assert 10 * n <= wb(128, 128, 128) <= 10 * n + (1 << 16)           # about 10 bytes per grid point
    assert wb(1024, 1024, 256) > 0 and wb(1024, 1024, 257) == 0        # 2^28 points is the limit
    assert wb(1, 8, 8) == 0 and wb(8, 0, 8) == 0 and wb(8, 8, -2) == 0 and wb(1 << 30, 1 << 30, 2) == 0


def test_mc_entry_points_check_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p, big = 64, 1 << 40          # a non-NULL, 16-byte aligned value: the checks return before anything dereferences it
    d3 = (C.c_double * 3)(0.0, 0.0, 0.0)

    def count(field=p, stride=1, nx=4, ny=4, nz=4, iso=0.0, ws=p, ws_bytes=big, counts=p):
        return L.pnr_mc_count(field, stride, nx, ny, nz, iso, ws, ws_bytes, counts, None)

    def emit(field=p, stride=1, nx=4, ny=4, nz=4, iso=0.0, origin=d3, scale=d3, ws=p, ws_bytes=big, nv=3, nt=1, v=p, t=p):
        return L.pnr_mc_emit(field, stride, nx, ny, nz, iso, origin, scale, ws, ws_bytes, nv, nt, v, t, None)

    for fn in (count, emit):
        assert fn(field=None) == E_NULL and fn(ws=None) == E_NULL
        assert fn(nx=1) == E_SHAPE and fn(ny=1) == E_SHAPE and fn(nz=0) == E_SHAPE and fn(nx=-4) == E_SHAPE
        assert fn(stride=0) == E_SHAPE and fn(stride=-1) == E_SHAPE
        assert fn(nx=1024, ny=1024, nz=257) == E_SHAPE                 # above 2^28 points
        assert fn(nx=1 << 30, ny=1 << 30, nz=1 << 30) == E_SHAPE       # products that would overflow
        need = L.pnr_mc_workspace_bytes(4, 4, 4)
        assert fn(ws_bytes=need - 1) == E_WORKSPACE and fn(ws_bytes=0) == E_WORKSPACE
        assert fn(ws=p + 8) == E_ALIGN
    assert count(counts=None) == E_NULL
    assert emit(origin=None) == E_NULL and emit(scale=None) == E_NULL
    assert emit(v=None) == E_NULL and emit(t=None) == E_NULL
    assert emit(nv=-1) == E_SHAPE and emit(nt=-1) == E_SHAPE
    assert emit(nv=0, nt=0, v=None, t=None) == 0                       # an empty mesh: no launch
    with pytest.raises(ValueError):
        N.check(count(nx=1), "pnr_mc_count")


def test_grid_points_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p = 64
    lo, hi = (C.c_double * 3)(-1, -1, -1), (C.c_double * 3)(1, 1, 1)

    def gp(c1=lo, c2=hi, reso=(4, 5, 6), first=0, count=120, fake=0, xyz=p, vd=None):
        r = None if reso is None else (C.c_int32 * 3)(*reso)
        return L.pnr_grid_points(c1, c2, r, first, count, fake, xyz, vd, None)

    assert gp(c1=None) == E_NULL and gp(c2=None) == E_NULL and gp(reso=None) == E_NULL and gp(xyz=None) == E_NULL
    assert gp(fake=1, vd=None) == E_NULL
    assert gp(reso=(0, 5, 6)) == E_SHAPE and gp(reso=(4, -1, 6)) == E_SHAPE
    assert gp(reso=(2048, 1024, 1024), count=1) == E_SHAPE             # 2^31 points
    assert gp(first=-1) == E_SHAPE and gp(count=-1) == E_SHAPE and gp(count=121) == E_SHAPE and gp(first=100, count=21) == E_SHAPE
    assert gp(first=121, count=0) == E_SHAPE
    assert gp(first=120, count=0) == 0 and gp(count=0) == 0            # nothing to write: no launch


def test_python_surface_refusals():
    import torch
    from pixel_nerf_multiscale_amd import recon, util

    class Net(torch.nn.Module):
        use_viewdirs = True
        num_objs = 2

        def __init__(self):
            super().__init__()
            self.p = torch.nn.Parameter(torch.zeros(1))

    net = Net()
    with pytest.raises(ValueError, match="exactly one"):
        recon.marching_cubes(net)
    with pytest.raises(ValueError, match="exactly one"):
        recon.vertex_colors(net, np.zeros((2, 3)))
    net.num_objs = 1
    with pytest.raises(ValueError, match="device"):
        recon.marching_cubes(net, device="cuda:0")                     # the net lives on the CPU
    with pytest.raises(ValueError, match="scale"):
        recon.marching_cubes(net, scale="cells")
    with pytest.raises(ValueError):
        recon.marching_cubes(net, reso=[8, 8])
    with pytest.raises(ValueError):
        recon.extract_mesh(torch.zeros(4, 4), 0.0)
    with pytest.raises(ValueError):
        recon.extract_mesh(torch.zeros(4, 4, 4, dtype=torch.float64), 0.0)
    with pytest.raises(ValueError):
        util.gen_grid_device([0, 0], [1, 1], [2, 2], device="cpu")
