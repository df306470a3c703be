"""Marching cubes on the CPU with the semantics and the ORDER of csrc/mesh.hip (include/pnr.h, pnr_mc_count / pnr_mc_emit), in
vectorised numpy, and a checker for closed oriented manifolds.  The case table comes from tools/gen_mc_tables.py."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool(name):
    spec = importlib.util.spec_from_file_location("_tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_gen = load_tool("gen_mc_tables")
_TABLE = _gen.build_table()
N_TRIS = np.array([len(t) for t in _TABLE], dtype=np.int64)
TRI_EDGES = np.full((256, 15), 0, dtype=np.int64)
for _m, _t in enumerate(_TABLE):
    _flat = [e for tri in _t for e in tri]
    TRI_EDGES[_m, :len(_flat)] = _flat
EDGE_AXIS = np.array(_gen.EDGE_AXIS, dtype=np.int64)
EDGE_LOWER = np.array([_gen.corner_offset(lo) for lo, _ in _gen.EDGE_CORNERS], dtype=np.int64)     # (12, 3)


def marching_cubes(field, iso):
    """field (nx, ny, nz) float32 -> (vertices (V, 3) float64 in index coordinates, triangles (T, 3) int32, cases (cells,) met).
    Inside iff float64(f) >= iso (a NaN is outside); one vertex per grid edge whose ends differ, numbered in linear
    grid-point order then by axis; triangles by linear cell index then in table order."""
    f = np.ascontiguousarray(field, dtype=np.float32)
    nx, ny, nz = f.shape
    f64 = f.astype(np.float64).ravel()
    with np.errstate(invalid="ignore"):
        inside = (f.astype(np.float64) >= float(iso))
    flags = np.zeros((3, nx, ny, nz), dtype=bool)
    flags[0, :-1] = inside[:-1] != inside[1:]
    flags[1, :, :-1] = inside[:, :-1] != inside[:, 1:]
    flags[2, :, :, :-1] = inside[:, :, :-1] != inside[:, :, 1:]
    fl = flags.reshape(3, -1)
    cnt = fl.sum(axis=0, dtype=np.int64)
    voff = np.cumsum(cnt) - cnt
    strides = (ny * nz, nz, 1)
    verts = np.empty((int(cnt.sum()), 3), dtype=np.float64)
    for a in range(3):
        idx = np.flatnonzero(fl[a])
        co = np.stack(np.unravel_index(idx, (nx, ny, nz)), axis=-1).astype(np.float64)
        fa, fb = f64[idx], f64[idx + strides[a]]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            co[:, a] = co[:, a] + (float(iso) - fa) / (fb - fa)
        verts[voff[idx] + fl[:a, idx].sum(axis=0)] = co
    case = np.zeros((nx, ny, nz), dtype=np.int64)
    ins = inside.astype(np.int64)
    for c in range(8):
        di, dj, dk = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case[:nx - 1, :ny - 1, :nz - 1] |= ins[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk] << c
    case = case.ravel()
    nt = N_TRIS[case]
    cells = np.flatnonzero(nt)
    rep = np.repeat(cells, nt[cells])
    start = np.cumsum(nt[cells]) - nt[cells]
    within = np.arange(rep.size) - np.repeat(start, nt[cells])
    tris = np.empty((rep.size, 3), dtype=np.int64)
    for m in range(3):
        e = TRI_EDGES[case[rep], within * 3 + m]
        lo = EDGE_LOWER[e]
        owner = rep + lo[:, 0] * strides[0] + lo[:, 1] * strides[1] + lo[:, 2]
        ax = EDGE_AXIS[e]
        lower = np.where(ax > 0, fl[0, owner], 0) + np.where(ax > 1, fl[1, owner], 0)
        tris[:, m] = voff[owner] + lower
    met = np.unique(case.reshape(nx, ny, nz)[:nx - 1, :ny - 1, :nz - 1])
    return verts, tris.astype(np.int32), met


def scale_vertices(vertices, scale, origin):
    """numpy's `vertices *= s; vertices + c1` of the reference (recon.py:74-78): two separately rounded fp64 operations."""
    v = np.array(vertices, dtype=np.float64, copy=True)
    v *= np.asarray(scale, dtype=np.float64)
    return v + np.asarray(origin, dtype=np.float64)


def signed_volume(vertices, triangles):
    v = np.nan_to_num(np.asarray(vertices, dtype=np.float64))
    a, b, c = (v[triangles[:, m]] for m in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def check_closed_manifold(vertices, triangles):
    """Every directed edge occurs exactly once and its reverse exactly once, every vertex is used, and no triangle repeats a
    vertex index.  Returns the Euler characteristic V - E + F."""
    t = np.asarray(triangles, dtype=np.int64)
    V = len(vertices)
    assert t.size == 0 or (t.min() >= 0 and t.max() < V), "triangle index out of range"
    assert not ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 2] == t[:, 0])).any(), "triangle repeats a vertex"
    a = np.concatenate((t[:, 0], t[:, 1], t[:, 2]))
    b = np.concatenate((t[:, 1], t[:, 2], t[:, 0]))
    fwd, rev = a * V + b, b * V + a
    uf = np.unique(fwd)
    assert uf.size == fwd.size, f"{fwd.size - uf.size} directed edges occur more than once"
    assert np.array_equal(uf, np.unique(rev)), "some directed edge has no reverse"
    assert np.unique(t).size == V, "unused vertices"
    return V - fwd.size // 2 + len(t)


def noise_field(n, seed=0):
    """standard_normal((n, n, n)) in fp32 with every border face set to -9: all surfaces are closed inside the grid."""
    f = np.random.default_rng(seed).standard_normal((n, n, n)).astype(np.float32)
    for sl in ((0,), (-1,)):
        f[sl[0]] = -9.0
        f[:, sl[0]] = -9.0
        f[:, :, sl[0]] = -9.0
    return f


def sphere_field(n, radius=0.7):
    x = np.linspace(-1.0, 1.0, n)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (radius - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
