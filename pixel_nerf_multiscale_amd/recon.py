"""
Mesh extraction (reference src/util/recon.py): marching cubes over the network's density on a regular grid, and OBJ output.
The grid, the density and the extraction all stay on the GPU (libpnr_hip: pnr_grid_points, pnr_point_mlp, pnr_mc_count /
pnr_mc_emit); the host reads two counts and, at the end, the mesh.  Names and defaults follow the reference so callers can
switch imports.
"""
import ctypes as C
import warnings

import numpy as np
import torch

from . import util


def extract_mesh(field, iso, origin=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """Marching cubes on the GPU (pnr_mc_count / pnr_mc_emit, include/pnr.h): field (nx, ny, nz) float32 on the device, dense or
    a regularly strided view (column `sigma_idx` of an (N, 4) record is read where it lies) -> (vertices (V, 3) float64 =
    index coordinate * scale + origin, triangles (T, 3) int32) on the device.  A grid point is inside iff field >= iso;
    normals point from inside to outside.  One host read (the two counts) sits between the two calls."""
    from . import _native as N
    s = util._field_stride(field, "field")
    nx, ny, nz = (int(n) for n in field.shape)
    if len(origin) != 3 or len(scale) != 3:
        raise ValueError("origin and scale must have 3 entries each")
    dev = N.same_device(field)
    nbytes = int(N.lib.pnr_mc_workspace_bytes(nx, ny, nz))
    ws = N.scratch(nbytes, dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    stream = N.current_stream(dev)
    N.check(N.lib.pnr_mc_count(field.data_ptr(), s, nx, ny, nz, float(iso), ws.data_ptr(), nbytes, counts.data_ptr(), stream),
            "pnr_mc_count")
    n_v, n_t = (int(v) for v in counts.cpu().tolist())         # the one wait: the output sizes depend on the data
    vertices = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
    triangles = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    N.check(N.lib.pnr_mc_emit(field.data_ptr(), s, nx, ny, nz, float(iso), (C.c_double * 3)(*[float(v) for v in origin]),
                              (C.c_double * 3)(*[float(v) for v in scale]), ws.data_ptr(), nbytes, n_v, n_t,
                              vertices.data_ptr() if n_v else None, triangles.data_ptr() if n_t else None, stream),
            "pnr_mc_emit")
    return vertices, triangles


def _fake_viewdirs(xyz):
    """-p / |p| (recon.py:54), (0, 0, 0) for a point of length 0."""
    n = xyz.norm(dim=-1, keepdim=True)
    return torch.where(n > 0, -xyz / n, torch.zeros_like(xyz))


def _single_object_device(net, device):
    dev = next(net.parameters()).device
    if device is not None and torch.device(device) != dev and torch.device(device) != torch.device(dev.type):
        raise ValueError(f"device must be the network's device {dev}, got {device}")
    if getattr(net, "num_objs", 1) != 1:
        raise ValueError(f"mesh extraction needs exactly one encoded object, the network holds {net.num_objs}")
    return dev


def marching_cubes(occu_net, c1=[-1, -1, -1], c2=[1, 1, 1], reso=[128, 128, 128], isosurface=50.0, sigma_idx=3,
                   eval_batch_size=100000, coarse=True, device=None, *, scale="reference"):
    """Marching cubes on the network's density (reference recon.py:12-78) -> (vertices (V, 3) float64, triangles (T, 3) int32)
    as numpy arrays.  c1, c2: corners of the bounds (all c2 > c1); reso: grid points per axis; isosurface: the sigma level;
    sigma_idx: the output column that holds sigma; coarse: which MLP.  The whole grid is ONE forward call — eval_batch_size was
    the reference's memory limit and is accepted and ignored; device, if given, must be the network's.
    scale="reference" multiplies index coordinates by (c2 - c1) / reso as the reference does, although the samples lie
    (c2 - c1) / (reso - 1) apart; scale="grid" uses the latter, which puts the vertices on the sampled positions.
    Inside is sigma >= isosurface, normals point out of the dense region; a grid point at the origin gets the view direction
    (0, 0, 0) where the reference's 0 / 0 gives NaN."""
    if scale not in ("reference", "grid"):
        raise ValueError(f"scale must be 'reference' or 'grid', got {scale!r}")
    if len(c1) != 3 or len(c2) != 3 or len(reso) != 3:
        raise ValueError("c1, c2 and reso must have 3 entries each")
    dev = _single_object_device(occu_net, device)
    if occu_net.use_viewdirs:
        warnings.warn("Running marching cubes with fake view dirs (pointing to origin), output may be invalid")
    reso = [int(r) for r in reso]
    is_train = occu_net.training
    occu_net.eval()
    try:
        with torch.no_grad():
            xyz, dirs = util.gen_grid_device(c1, c2, reso, fake_viewdirs=True, device=dev)
            out = occu_net(xyz[None], coarse=coarse, viewdirs=dirs[None])
            out = out.reshape(-1, out.shape[-1])
            if not 0 <= int(sigma_idx) < out.shape[-1]:
                raise ValueError(f"sigma_idx {sigma_idx} outside the network's {out.shape[-1]} output columns")
            lo, hi = np.asarray(c1, dtype=np.float64), np.asarray(c2, dtype=np.float64)
            div = np.asarray(reso, dtype=np.float64) - (1.0 if scale == "grid" else 0.0)
            vertices, triangles = extract_mesh(out[:, int(sigma_idx)].view(*reso), isosurface, origin=lo, scale=(hi - lo) / div)
            return vertices.cpu().numpy(), triangles.cpu().numpy()
    finally:
        if is_train:
            occu_net.train()


def vertex_colors(net, vertices, coarse=True):
    """The network's rgb at mesh vertices (V, 3) under the same fake view directions, for save_obj's vert_rgb -> (V, 3) float32
    numpy."""
    dev = _single_object_device(net, None)
    xyz = torch.as_tensor(np.asarray(vertices), dtype=torch.float32).reshape(-1, 3).to(dev)
    if xyz.shape[0] == 0:
        return np.zeros((0, 3), dtype=np.float32)
    is_train = net.training
    net.eval()
    try:
        with torch.no_grad():
            out = net(xyz[None], coarse=coarse, viewdirs=_fake_viewdirs(xyz)[None])
            return out.reshape(-1, out.shape[-1])[:, :3].cpu().numpy()
    finally:
        if is_train:
            net.train()


def save_obj(vertices, triangles, path, vert_rgb=None):
    """OBJ file with the reference's line formats (recon.py:81-106): "v x y z" or "v x y z r g b" with 4 decimals, then
    1-based "f a b c"."""
    vertices, triangles = np.asarray(vertices), np.asarray(triangles)
    if vert_rgb is None:
        rows = ["v %.4f %.4f %.4f\n" % (v[0], v[1], v[2]) for v in vertices]
    else:
        vert_rgb = np.asarray(vert_rgb)
        if len(vert_rgb) != len(vertices):
            raise ValueError(f"vert_rgb has {len(vert_rgb)} rows for {len(vertices)} vertices")
        rows = ["v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (v[0], v[1], v[2], c[0], c[1], c[2]) for v, c in zip(vertices, vert_rgb)]
    rows += ["f %d %d %d\n" % (f[0] + 1, f[1] + 1, f[2] + 1) for f in triangles]
    with open(path, "w") as fh:
        fh.writelines(rows)
