"""
Empty-space culling in front of the render launch (libpnr_hip: pnr_occ_build, pnr_ray_bounds, pnr_frame_from_hits; the
arithmetic is written out in include/pnr.h).  The reference has no counterpart: it evaluates every sample of every ray.

* OccupancyGrid            a bit grid over a box: which cells hold density, from sigma samples, from the network itself, or
                           from a bool tensor
* ray_bounds               rays of F frames -> each frame's ordered list of the rays that pass through an occupied cell, with
                           [near, far] tightened to the occupied stretch; per-ray slots and per-frame counts, all on the device
* frame_from_hits          rendered records of the lists -> whole frames, background where a ray missed
* NeRFRenderer.render_frames_bounded (render/nerf.py) strings them together around the existing render call.

Everything is opt-in: nothing here runs unless a caller passes occupancy=... .

NOT MEASURED: no sigma threshold has been tried on a trained model (no checkpoint or dataset is at hand where this package is
developed), which is why from_net has no default for sigma_thresh.  The network's density also depends on the view direction,
so a grid built under the fake radial directions of recon.marching_cubes is an approximation of what a camera sees; dilate,
pad and a (D, 3) set of view directions are the safeguards.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import util

MAX_DILATE = 4


def _triple(v, name, cast=float):
    v = [cast(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != 3:
        raise ValueError(f"{name} must have 3 entries, got {len(v)}")
    return tuple(v)


def _words(reso):
    cx, cy, cz = (r - 1 for r in reso)
    return cx * cy * ((cz + 31) // 32)


def read_counts(counts):
    """The per-frame counts on the host, as a list: ONE asynchronous copy into pinned memory and one wait for it."""
    host = torch.empty(counts.shape, dtype=counts.dtype, pin_memory=True)
    host.copy_(counts, non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(counts.device))
    done.synchronize()
    return host.tolist()


class OccupancyGrid:
    """Occupied cells of the box c1 .. c2.  reso = (nx, ny, nz) SAMPLES per axis on the util.gen_grid(ij_indexing=True) lattice,
    so there are (nx - 1, ny - 1, nz - 1) cells; bits: int32 words, cell (i, j, k) is bit k & 31 of word
    (i cy + j) wz + (k >> 5), wz = ceil(cz / 32), padding bits zero (include/pnr.h)."""

    def __init__(self, c1, c2, reso, bits):
        self.c1, self.c2 = _triple(c1, "c1"), _triple(c2, "c2")
        self.reso = _triple(reso, "reso", int)
        if any(r < 2 for r in self.reso):
            raise ValueError(f"every axis needs at least 2 samples, got {self.reso}")
        if any(not (math.isfinite(a) and math.isfinite(b) and b > a) for a, b in zip(self.c1, self.c2)):
            raise ValueError(f"the box needs finite corners with c2 > c1 on every axis, got {self.c1} {self.c2}")
        if bits.dtype != torch.int32 or bits.dim() != 1 or bits.numel() != _words(self.reso) or not bits.is_contiguous():
            raise ValueError(f"bits must be {_words(self.reso)} contiguous int32 words, got {bits.dtype} {tuple(bits.shape)}")
        self.bits = bits

    @property
    def cell_counts(self):
        return tuple(r - 1 for r in self.reso)

    @property
    def cell_size(self):
        """Edge lengths of a cell, fp64 on the host."""
        return tuple((b - a) / n for a, b, n in zip(self.c1, self.c2, self.cell_counts))

    def cell_diagonal(self):
        return math.sqrt(sum(h * h for h in self.cell_size))

    # ------------------------------------------------------------------------------------------------ constructors
    @classmethod
    def from_sigma(cls, sigma, c1, c2, *, thresh, dilate=1, into=None):
        """sigma (nx, ny, nz) float32 on the device, dense or a regularly strided view (the sigma column of an (N, 4) network
        output is read where it lies) -> the grid of the cells with a corner sample >= thresh (or NaN), grown by `dilate`
        cells (0 .. 4, Chebyshev).  into: a grid of the same box and size to OR the result into (it is returned)."""
        from .. import _native as N
        s = util._field_stride(sigma, "sigma")
        nx, ny, nz = (int(n) for n in sigma.shape)
        if not 0 <= int(dilate) <= MAX_DILATE:
            raise ValueError(f"dilate must be 0 .. {MAX_DILATE}, got {dilate}")
        dev = N.same_device(sigma)
        if into is None:
            grid = cls(c1, c2, (nx, ny, nz), torch.empty(_words((nx, ny, nz)), dtype=torch.int32, device=dev))
        else:
            grid = into
            if grid.reso != (nx, ny, nz) or grid.c1 != _triple(c1, "c1") or grid.c2 != _triple(c2, "c2") or grid.bits.device != dev:
                raise ValueError("into must be a grid of the same box, size and device")
        N.check(N.lib.pnr_occ_build(sigma.data_ptr(), s, nx, ny, nz, float(thresh), int(dilate), int(into is not None),
                                    grid.bits.data_ptr(), N.current_stream(dev)), "pnr_occ_build")
        return grid

    @classmethod
    def from_net(cls, net, *, sigma_thresh, c1=(-1, -1, -1), c2=(1, 1, 1), reso=64, dilate=1, mlps=("coarse",), viewdirs="radial"):
        """The grid of an encoded network: its density on the reso^3 (or (nx, ny, nz)) lattice of the box, one forward call per
        MLP and view-direction set, with util.gen_grid_device and net(...) exactly as recon.marching_cubes uses them.
        sigma_thresh is REQUIRED: no value has been measured on a trained model.  viewdirs: "radial" = the fake directions
        -p / |p| of marching_cubes, or a (D, 3) tensor: the grid is then the OR over the D directions, each given to every
        point.  mlps=("coarse", "fine") ORs both MLPs.  The network must hold exactly one encoded object."""
        from ..recon import _single_object_device
        dev = _single_object_device(net, None)
        reso = (int(reso),) * 3 if np.isscalar(reso) else _triple(reso, "reso", int)
        mlps = tuple(mlps)
        if not mlps or any(m not in ("coarse", "fine") for m in mlps):
            raise ValueError(f"mlps must name 'coarse' and / or 'fine', got {mlps}")
        radial = isinstance(viewdirs, str)
        if radial and viewdirs != "radial":
            raise ValueError(f"viewdirs must be 'radial' or a (D, 3) tensor, got {viewdirs!r}")
        if not radial:
            viewdirs = torch.as_tensor(viewdirs, dtype=torch.float32).to(dev)
            if viewdirs.dim() != 2 or viewdirs.shape[1] != 3 or viewdirs.shape[0] < 1:
                raise ValueError(f"viewdirs must be (D, 3) with D >= 1, got {tuple(viewdirs.shape)}")
        grid = None
        was_training = net.training
        net.eval()
        try:
            with torch.no_grad():
                xyz, dirs = util.gen_grid_device(c1, c2, reso, fake_viewdirs=True, device=dev)
                dir_sets = [dirs] if radial else [v[None].expand(xyz.shape[0], 3).contiguous() for v in viewdirs]
                for which in mlps:
                    for d in dir_sets:
                        out = net(xyz[None], coarse=which == "coarse", viewdirs=d[None])
                        out = out.reshape(-1, out.shape[-1])
                        grid = cls.from_sigma(out[:, 3].view(*reso), c1, c2, thresh=sigma_thresh, dilate=dilate, into=grid)
        finally:
            net.train(was_training)
        return grid

    @classmethod
    def from_cells(cls, cells, c1, c2, device=None):
        """cells (cx, cy, cz) bool -> the grid with exactly these cells, packed on the host (tests, synthetic benchmarks).
        device: where the bits go, default the tensor's."""
        cells = torch.as_tensor(cells)
        if cells.dim() != 3 or cells.dtype != torch.bool or min(cells.shape) < 1:
            raise ValueError(f"cells must be a bool (cx, cy, cz) tensor, got {cells.dtype} {tuple(cells.shape)}")
        dev = cells.device if device is None else torch.device(device)
        a = cells.cpu().numpy()
        cx, cy, cz = a.shape
        wz = (cz + 31) // 32
        padded = np.zeros((cx, cy, wz * 32), dtype=bool)
        padded[:, :, :cz] = a
        words = np.packbits(padded.reshape(cx, cy, wz, 32), axis=-1, bitorder="little").view("<u4").reshape(-1)
        bits = torch.from_numpy(words.astype("<u4").view(np.int32).copy())
        return cls(c1, c2, (cx + 1, cy + 1, cz + 1), bits.to(dev))

    # ------------------------------------------------------------------------------------------------ readers
    def cells(self):
        """(cx, cy, cz) bool, on the device of the bits."""
        cx, cy, cz = self.cell_counts
        wz = (cz + 31) // 32
        sh = torch.arange(32, dtype=torch.int32, device=self.bits.device)
        return (((self.bits.view(cx, cy, wz, 1) >> sh) & 1) != 0).reshape(cx, cy, wz * 32)[:, :, :cz]

    def occupied_fraction(self):
        """Share of occupied cells, a host float (it waits for the device)."""
        return float(self.cells().float().mean())


def ray_bounds(grid, rays, rays_per_frame=None, pad=None):
    """rays (n, 8) float32 on the grid's device, frame f = rows f R .. f R + R - 1 (R = rays_per_frame, None: one frame) ->
    (rays_out (n, 8), slot (n) int32, counts (F) int64), all on the device, nothing read back: rows f R .. f R + counts[f] - 1 of
    rays_out hold frame f's rays that pass through an occupied cell, in ascending ray order, columns 6:8 tightened to
    [max(near, t_in - pad), min(far, t_out + pad)]; the rows past a count are not written.  slot[i]: ray i's place in its
    frame's list, or -1.  pad=None: one cell diagonal, computed in fp64 on the host."""
    from .. import _native as N
    if not N.arg(rays, "rays", torch.float32, (None, 8)).is_contiguous():
        raise ValueError(f"rays must be contiguous, got strides {rays.stride()}")
    n = int(rays.shape[0])
    R = n if rays_per_frame is None else int(rays_per_frame)
    if R < 1 or n % R:
        raise ValueError(f"{n} rays are no whole number of frames of {R}")
    dev = N.same_device(rays, grid.bits)
    pad = grid.cell_diagonal() if pad is None else float(pad)
    rays_out = torch.empty_like(rays)
    slot = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(n // R, dtype=torch.int64, device=dev)
    nbytes = int(N.lib.pnr_ray_bounds_workspace_bytes(n, R))
    ws = N.scratch(nbytes, dev)
    N.check(N.lib.pnr_ray_bounds(rays.data_ptr(), n, R, (C.c_double * 3)(*grid.c1), (C.c_double * 3)(*grid.c2),
                                 (C.c_int32 * 3)(*grid.cell_counts), grid.bits.data_ptr(), pad, ws.data_ptr(), nbytes,
                                 rays_out.data_ptr(), slot.data_ptr(), counts.data_ptr(), N.current_stream(dev)), "pnr_ray_bounds")
    return rays_out, slot, counts


def frame_from_hits(rec, slot, rays_per_frame, bg, out=None):
    """rec (n, >= 4) float32 rows [rgb, depth, ...] with row stride rec.stride(0), frame f's list from row f R on; slot (n) int32
    -> out (n, 4): [bg, bg, bg, 0] where slot < 0, the record's first four floats otherwise."""
    from .. import _native as N
    if not N.arg(slot, "slot", torch.int32, (None,)).is_contiguous():
        raise ValueError(f"slot must be contiguous, got stride {slot.stride()}")
    n, R = int(slot.shape[0]), int(rays_per_frame)
    # records and frames are rows of at least 4 floats at any row stride: a rule of this call's own, not N.out's exact shape
    if N.arg(rec, "rec", torch.float32, (n, None)).shape[1] < 4 or rec.stride(1) != 1:
        raise ValueError(f"rec must be float32 ({n}, >= 4) with unit column stride, got {tuple(rec.shape)} strides {rec.stride()}")
    if out is not None and (N.arg(out, "out", torch.float32, (n, None)).shape[1] < 4 or out.stride(1) != 1):
        raise ValueError(f"out must be float32 ({n}, >= 4) with unit column stride, got {tuple(out.shape)} strides {out.stride()}")
    dev = N.same_device(rec, slot, out)
    if out is None:
        out = torch.empty(n, 4, dtype=torch.float32, device=dev)
    N.check(N.lib.pnr_frame_from_hits(rec.data_ptr(), max(int(rec.stride(0)), 4), slot.data_ptr(),
                                      n, R, float(bg), out.data_ptr(), max(int(out.stride(0)), 4),
                                      N.current_stream(dev)), "pnr_frame_from_hits")
    return out


def resolve(occupancy, net):
    """What the drivers' `occupancy` argument means -> (OccupancyGrid, pad): a grid as it is (pad None), or a dict of
    OccupancyGrid.from_net's keywords plus an optional "pad", built from `net` as it is encoded now."""
    if isinstance(occupancy, OccupancyGrid):
        return occupancy, None
    if isinstance(occupancy, dict):
        kw = dict(occupancy)
        pad = kw.pop("pad", None)
        if "sigma_thresh" not in kw:
            raise TypeError("occupancy needs sigma_thresh: no default has been measured on a trained model")
        return OccupancyGrid.from_net(net, **kw), pad
    raise TypeError(f"occupancy must be an OccupancyGrid or a dict of OccupancyGrid.from_net keywords, got {type(occupancy).__name__}")


def refuse_sharded(what):
    """occupancy under a process group of several ranks: sharding the compact list is out of scope."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError(f"{what}: occupancy is not available under a process group of {dist.get_world_size()} ranks "
                         "(the compact ray lists are not sharded)")
