"""
Host-side helpers around the render path: config access, camera/ray construction and the two tensor
helpers the model protocol uses.  Names follow the reference's src/util/util.py so callers can switch
imports; the implementations are this package's own.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch


class Conf:
    """Uniform read access to a pyhocon ConfigTree (reference configs) or a plain dict."""

    def __init__(self, obj=None):
        self._o = obj if obj is not None else {}

    def _raw(self, key, default):
        o = self._o
        if isinstance(o, Conf):
            return o._raw(key, default)
        try:
            return o[key] if key in o else default
        except TypeError:
            return getattr(o, key, default)

    def get(self, key, default=None):
        return self._raw(key, default)

    def get_int(self, key, default=None):
        return int(self._raw(key, default))

    def get_float(self, key, default=None):
        return float(self._raw(key, default))

    def get_bool(self, key, default=None):
        v = self._raw(key, default)
        return v.lower() in ("1", "true", "yes", "on") if isinstance(v, str) else bool(v)

    def get_string(self, key, default=None):
        return str(self._raw(key, default))

    def get_list(self, key, default=None):
        return self._raw(key, default)

    def __contains__(self, key):
        return self._raw(key, _MISSING) is not _MISSING

    def __getitem__(self, key):
        v = self._raw(key, _MISSING)
        if v is _MISSING:
            raise KeyError(key)
        return Conf(v) if isinstance(v, dict) or hasattr(v, "get_int") else v


_MISSING = object()


def as_conf(c):
    return c if isinstance(c, Conf) else Conf(c)


def repeat_interleave(t, repeats, dim=0):
    """(B, ...) -> (B*repeats, ...) with each row repeated consecutively (reference util.py:58-65)."""
    assert dim == 0
    return t[:, None].expand(t.shape[0], repeats, *t.shape[1:]).reshape(-1, *t.shape[1:])


def combine_interleaved(t, inner_dims=(1,), agg_type="average"):
    """(-1, *inner_dims, C): reduce the first inner dim (views) by mean or max (reference util.py:466-476)."""
    if len(inner_dims) == 1 and inner_dims[0] == 1:
        return t
    t = t.reshape(-1, *inner_dims, *t.shape[1:])
    if agg_type == "average":
        return t.mean(dim=1)
    if agg_type == "max":
        return t.max(dim=1)[0]
    raise NotImplementedError("Unsupported combine type " + agg_type)


def psnr(pred, target):
    mse = float(((pred - target) ** 2).mean())
    return -10.0 * math.log10(mse)


def pose_spherical(theta, phi, radius, reference_order=False):
    """c2w (4,4) of a camera at spherical position (theta, phi in degrees) looking at the origin
    (reference util.py:314-328 conventions: camera looks down -z, world z up after the axis flip).
    reference_order=True (the camera paths of video.py): the reference's own operation order — angle / 180 * pi in fp64,
    numpy's cos / sin rounded to fp32, the four fp32 matrices multiplied from the right, flip @ (rot_theta @ (rot_phi @
    trans)) — which reproduces its poses bit for bit (tests/golden/video_paths.npz); the default is within an ulp of it."""
    if reference_order:
        th, ph = theta / 180.0 * np.pi, phi / 180.0 * np.pi
        t = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1]], dtype=torch.float32)
        rp = torch.tensor([[1, 0, 0, 0], [0, np.cos(ph), -np.sin(ph), 0], [0, np.sin(ph), np.cos(ph), 0], [0, 0, 0, 1]],
                          dtype=torch.float32)
        rt = torch.tensor([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]],
                          dtype=torch.float32)
        flip = torch.tensor([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=torch.float32)
        return flip @ (rt @ (rp @ t))
    th, ph = math.radians(theta), math.radians(phi)
    t = torch.eye(4)
    t[2, 3] = radius
    rp = torch.eye(4)
    rp[1, 1], rp[1, 2], rp[2, 1], rp[2, 2] = math.cos(ph), -math.sin(ph), math.sin(ph), math.cos(ph)
    rt = torch.eye(4)
    rt[0, 0], rt[0, 2], rt[2, 0], rt[2, 2] = math.cos(th), -math.sin(th), math.sin(th), math.cos(th)
    flip = torch.tensor([[-1.0, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    return (flip @ rt @ rp @ t).float()


def coord_from_blender(dtype=torch.float32, device="cpu"):
    """(4, 4) Blender (x right, y in, z up) -> standard (x right, y up, z out of the screen) axes (reference util.py:151-162)."""
    return torch.tensor([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], dtype=dtype, device=device)


def coord_to_blender(dtype=torch.float32, device="cpu"):
    """(4, 4) standard -> Blender axes, the inverse of coord_from_blender (reference util.py:165-176)."""
    return torch.tensor([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=dtype, device=device)


def quat_to_rot(q):
    """q (B, 4) = (r, i, j, k), any length -> rotation matrices (B, 3, 3) of the normalised quaternions (reference
    util.py:489-509): F.normalize along dim 1, then the entries in the reference's operation order, so the bits are its bits."""
    q = torch.nn.functional.normalize(q, dim=1)
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = ((1 - 2 * (j ** 2 + k ** 2), 2 * (j * i - k * r), 2 * (i * k + r * j)),
            (2 * (j * i + k * r), 1 - 2 * (i ** 2 + k ** 2), 2 * (j * k - i * r)),
            (2 * (k * i - j * r), 2 * (j * k + i * r), 1 - 2 * (i ** 2 + j ** 2)))
    return torch.stack([torch.stack(row, dim=-1) for row in rows], dim=1)


def intrinsics(focal, c, W, H):
    """(fx, fy, cx, cy) as host floats: focal a scalar or (fx, fy), c = (cx, cy) or None for the image centre (W/2, H/2)."""
    f = torch.as_tensor(focal, dtype=torch.float32).flatten()
    if c is None:
        return float(f[0]), float(f[-1]), W * 0.5, H * 0.5
    c = torch.as_tensor(c, dtype=torch.float32).flatten()
    return float(f[0]), float(f[-1]), float(c[0]), float(c[1])


class Camera(namedtuple("Camera", "c2w16 W H fx fy cx cy z_near z_far pix0 n")):
    """The camera of a fused render, host values only: c2w as 16 floats row-major, the image size, the intrinsics, the depth
    range, and the pixels [pix0, pix0 + n) of the W x H image that the call renders."""
    __slots__ = ()

    def c_args(self):
        """The camera arguments of pnr_render_camera and pnr_gen_rays, in the order both take them."""
        return ((C.c_float * 16)(*self.c2w16), self.W, self.H, self.fx, self.fy, self.cx, self.cy, self.z_near, self.z_far,
                self.pix0, self.n)


def camera(pose, W, H, focal, z_near, z_far, c=None, pix0=0, n=None):
    """Camera from a (4, 4) camera-to-world pose (tensor, array or nested list) and the intrinsics as intrinsics() takes
    them; n=None: the whole image."""
    W, H = int(W), int(H)
    return Camera(torch.as_tensor(pose, dtype=torch.float32).cpu().flatten().tolist(), W, H, *intrinsics(focal, c, W, H),
                  float(z_near), float(z_far), int(pix0), W * H if n is None else int(n))


def unproj_map(width, height, f, c=None, device="cpu"):
    """(H, W, 3) unit camera-space ray directions of a pinhole camera (reference util.py:118-148)."""
    fx, fy, cx, cy = intrinsics(f, c, width, height)
    ys = (torch.arange(height, dtype=torch.float32, device=device) - cy) / fy
    xs = (torch.arange(width, dtype=torch.float32, device=device) - cx) / fx
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    d = torch.stack((X, -Y, -torch.ones_like(X)), dim=-1)
    return d / d.norm(dim=-1, keepdim=True)


def gen_rays(poses, width, height, focal, z_near, z_far, c=None, ndc=False):
    """poses (B,4,4) c2w -> rays (B, H, W, 8) = [origin, direction, near, far] (reference util.py:243-281)."""
    if ndc:
        raise NotImplementedError("NDC rays are not part of the accelerated path")
    dev = poses.device
    dirs = unproj_map(width, height, torch.as_tensor(focal).squeeze(), c=c, device=dev)      # (H,W,3)
    dirs = torch.einsum("bij,hwj->bhwi", poses[:, :3, :3].float(), dirs)
    orig = poses[:, None, None, :3, 3].float().expand(-1, height, width, -1)
    near = torch.full((poses.shape[0], height, width, 1), float(z_near), device=dev)
    far = torch.full((poses.shape[0], height, width, 1), float(z_far), device=dev)
    return torch.cat((orig, dirs, near, far), dim=-1)


class AttrDict(dict):
    """Nested result container with attribute access and toDict(), standing in for dotmap.DotMap in
    the renderer's return value (reference nerf.py:278-316)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def toDict(self):
        return {k: (v.toDict() if isinstance(v, AttrDict) else v) for k, v in self.items()}


def seed_from_torch():
    """A 63-bit seed drawn from torch's global CPU generator, so kernel-side noise follows
    torch.manual_seed like the reference's torch.rand calls do."""
    hi, lo = torch.randint(0, 2 ** 31 - 1, (2,)).tolist()
    return (hi << 31) | lo


def gen_rays_device(pose, width, height, focal, z_near, z_far, c=None, device="cuda", out=None):
    """gen_rays for ONE camera, computed on the GPU by libpnr_hip (pnr_gen_rays): pose (4,4) c2w on the host ->
    rays (H*W, 8) on `device`, never materialised on the host.  out: a contiguous float32 (H*W, 8) device tensor
    to write into — one row of an (SB, H*W, 8) batch of cameras — which is then returned; `device` is out's."""
    from . import _native as N
    cam = camera(pose, width, height, focal, z_near, z_far, c=c)
    if out is None:
        dev = torch.device(device)
        out = torch.empty(cam.n, 8, device=dev, dtype=torch.float32)
    else:
        if tuple(out.shape) != (cam.n, 8) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 ({cam.n}, 8), got {out.dtype} {tuple(out.shape)}")
        dev = N.same_device(out)
    N.check(N.lib.pnr_gen_rays(*cam.c_args(), N.ptr(out), N.current_stream(dev)), "pnr_gen_rays")
    return out


def gen_grid(*args, ij_indexing=False):
    """Grid points of len(args) axes, each arg (lo, hi, size) sampled at np.linspace(lo, hi, size) in fp32 ->
    (prod sizes, len(args)) float32 on the host (reference util.py:98-115).  ij_indexing=True: the first axis varies
    slowest, linear index (i ny + j) nz + k; False: numpy's "xy" meshgrid order, the reference's default."""
    axes = [np.linspace(lo, hi, int(size), dtype=np.float32) for lo, hi, size in args]
    mesh = np.meshgrid(*axes, indexing="ij" if ij_indexing else "xy")
    return torch.from_numpy(np.stack([m.reshape(-1) for m in mesh], axis=-1))


def gen_grid_device(c1, c2, reso, first=0, count=None, fake_viewdirs=False, device="cuda"):
    """Points [first, first + count) of gen_grid(*zip(c1, c2, reso), ij_indexing=True), written on the GPU by libpnr_hip
    (pnr_grid_points) with the bits of the host version -> xyz (count, 3) [, viewdirs (count, 3) = -p / |p|, the fake view
    directions of recon.marching_cubes; (0, 0, 0) for a point of length 0] on `device`."""
    from . import _native as N
    if len(c1) != 3 or len(c2) != 3 or len(reso) != 3:
        raise ValueError("c1, c2 and reso must have 3 entries each")
    reso = [int(r) for r in reso]
    n = reso[0] * reso[1] * reso[2]
    count = n - int(first) if count is None else int(count)
    dev = torch.device(device)
    xyz = torch.empty(max(count, 0), 3, device=dev, dtype=torch.float32)
    dirs = torch.empty_like(xyz) if fake_viewdirs else None
    N.check(N.lib.pnr_grid_points((C.c_double * 3)(*[float(v) for v in c1]), (C.c_double * 3)(*[float(v) for v in c2]),
                                  (C.c_int32 * 3)(*reso), int(first), count, int(bool(fake_viewdirs)), xyz.data_ptr(),
                                  N.dptr(dirs), N.current_stream(dev)), "pnr_grid_points")
    return (xyz, dirs) if fake_viewdirs else xyz


def batched_index_select_nd(t, inds):
    """t (batch, n, ...), inds (batch, k) long -> (batch, k, ...): row inds[b, j] of t[b] (reference util.py:33-42)."""
    rows = torch.arange(t.shape[0], device=inds.device)[:, None].expand_as(inds)
    return t[rows, inds]


def bbox_sample(bboxes, num_pix):
    """num_pix pixels drawn inside the bounding boxes of random views (reference util.py:225-240): bboxes (NV, 4) =
    cmin, rmin, cmax, rmax on the host -> (num_pix, 3) long rows (view, row, col).  Consumes torch's global CPU generator in
    the reference's order — randint for the views, rand for the columns, rand for the rows, truncated by .long() — so the
    same torch.manual_seed gives the same pixels (tests/golden/train_batch.npz)."""
    view = torch.randint(0, bboxes.shape[0], (num_pix,))
    box = bboxes[view]
    col = (torch.rand(num_pix) * (box[:, 2] + 1 - box[:, 0]) + box[:, 0]).long()
    row = (torch.rand(num_pix) * (box[:, 3] + 1 - box[:, 1]) + box[:, 1]).long()
    return torch.stack((view, row, col), dim=-1)


def upload(t, device):
    """Host tensor -> device through pinned memory, asynchronously.  A copy from pageable memory makes the host wait until
    the stream has drained, which would put a bubble into every training step; a device tensor passes through."""
    if t.is_cuda:
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


def train_batch(images, poses, focal, c, pix_inds, z_near, z_far):
    """Rays and ground-truth colours of sampled pixels, gathered on the GPU by libpnr_hip (pnr_train_batch) in place of
    gen_rays over every view + indexing (train/train.py:280-311).  images (SB, NV, 3, H, W) in [-1, 1] and poses
    (SB, NV, 4, 4) c2w on the device; focal (SB,) or (SB, 2) and c None or (SB, 2) as the data loader gives them (host or
    device); pix_inds (SB, B) long on the device, view * H * W + row * W + col.  -> rays (SB, B, 8), rgb_gt (SB, B, 3) in
    [0, 1].  An index outside [0, NV*H*W) gives a NaN row (the indices are never read on the host)."""
    from . import _native as N
    images = N.arg(images, "images", None, (None, None, 3, None, None))
    SB, NV, _, H, W = images.shape
    return _gather_batch(N, "pnr_train_batch", N.f32c(images), (SB, NV, H, W), poses, focal, c, pix_inds, z_near, z_far)


def _gather_batch(N, entry, images, dims, poses, focal, c, pix_inds, z_near, z_far, *tail, jitter=None):
    """What train_batch and train_batch_u8 share, from the checked image batch to the call of `entry`: poses and pix_inds are
    checked, focal / c uploaded and expanded to (SB, 2), rays and rgb_gt allocated.  tail: the entry point's arguments behind
    rgb_gt; a jitter record goes behind those.  N: the caller's _native."""
    SB, NV, H, W = dims
    poses = N.arg(poses, "poses", None, (SB, NV, 4, 4))
    pix_inds = N.arg(pix_inds, "pix_inds", torch.long, (SB, None), contiguous=True)
    if jitter is not None:
        jitter = N.arg(jitter, "jitter", torch.float32, (SB, 8), contiguous=True)
    dev = N.same_device(images, poses, pix_inds, jitter)
    poses = N.f32c(poses)
    focal = upload(torch.as_tensor(focal, dtype=torch.float32), dev)
    if focal.dim() <= 1:
        focal = focal.reshape(-1, 1).expand(-1, 2)
    focal = focal.expand(SB, 2).contiguous()
    if c is not None:
        c = upload(torch.as_tensor(c, dtype=torch.float32), dev).reshape(-1, 2).expand(SB, 2).contiguous()
    B = pix_inds.shape[1]
    rays = torch.empty(SB, B, 8, device=dev)
    rgb_gt = torch.empty(SB, B, 3, device=dev)
    if jitter is not None:
        tail += (N.ptr(jitter),)
    N.check(getattr(N.lib, entry)(N.ptr(images), N.ptr(poses), N.ptr(focal), N.ptr(c), SB, NV, W, H, float(z_near), float(z_far),
                                  pix_inds.data_ptr(), B, N.ptr(rays), N.ptr(rgb_gt), *tail, N.current_stream(dev)), entry)
    return rays, rgb_gt


_U8_BATCH = (None, None, None, None, (3, 4))     # N.arg's shape of a uint8 batch (SB, NV, H, W, 3 | 4); a pool's slice is made contiguous
_OBJ_BASE_END = 1 << 63                         # obj_base, the first object of a call over a slice of a step's batch, travels as int64


def color_jitter_plan(images_u8, ranges, seed, out=None, obj_base=0):
    """The colour-jitter records of one step (pnr_color_jitter_plan; include/pnr.h writes the arithmetic down): per object of
    the uint8 batch images_u8 (SB, NV, H, W, 3 | 4) on the device, one brightness / contrast / saturation factor and hue shift
    inside `ranges` (four host floats, or a data.ColorJitter), the order of the four operations, and — where contrast takes
    part — the object's grey mean over ALL its views, all keyed by `seed` alone (the per-step key).  -> float32 (SB, 8) on the
    device: [brightness, contrast, saturation, hue, mean, order code, 0, 0], what train_batch_u8 / views_to_tensor_u8 take as
    `jitter`.  Reads nothing back; `out` (SB, 8) float32 contiguous is filled when given.
    obj_base: images_u8 holds objects obj_base .. obj_base + SB - 1 of the step's batch (pnr_color_jitter_plan_at): the records
    are those rows of the whole batch's plan, bit for bit."""
    from . import _native as N
    import ctypes
    images_u8 = N.arg(images_u8, "images_u8", torch.uint8, _U8_BATCH, contiguous=True)
    SB, NV, H, W, C = images_u8.shape
    ranges = tuple(float(r) for r in getattr(ranges, "ranges", ranges))
    seed, obj_base = N.key64(seed, "seed"), N.key64(obj_base, "obj_base", _OBJ_BASE_END)
    if len(ranges) != 4:
        raise ValueError(f"ranges must be (brightness, contrast, saturation, hue), got {ranges}")
    rec = N.out(out, "out", torch.float32, (SB, 8), images_u8.device)
    dev = N.same_device(images_u8, rec)
    nbytes = int(N.lib.pnr_color_jitter_workspace_bytes(SB, NV, W, H)) if ranges[1] != 0.0 else 0
    ws = N.scratch(nbytes, dev)
    N.check(N.lib.pnr_color_jitter_plan_at(N.ptr(images_u8), SB, NV, W, H, C, (ctypes.c_float * 4)(*ranges), seed, obj_base,
                                           N.ptr(rec), ws.data_ptr(), nbytes, N.current_stream(dev)), "pnr_color_jitter_plan_at")
    return rec


def train_batch_u8(images_u8, poses, focal, c, pix_inds, z_near, z_far, balanced=True, jitter=None):
    """train_batch for a batch whose images stay 8-bit on the device (pnr_train_batch_u8): images_u8 (SB, NV, H, W, 3 | 4)
    uint8, interleaved as the files hold them (a fourth channel is stepped over), at any byte offset of a larger allocation;
    the other arguments as train_batch takes them.  balanced says what the FLOAT image of the loader would have been —
    (b / 255 - 0.5) / 0.5 in [-1, 1] (True) or b / 255 (False) — and rgb_gt = 0.5 * that + 0.5, bit for bit what train_batch
    gives on that float image; the rays are train_batch's bits.  -> rays (SB, B, 8), rgb_gt (SB, B, 3).
    jitter: color_jitter_plan's record (SB, 8) — each sampled pixel goes through its object's colour chain between the
    division by 255 and the balanced map (pnr_train_batch_u8_jitter); None: the call and the bits without it."""
    from . import _native as N
    images_u8 = N.arg(images_u8, "images_u8", torch.uint8, _U8_BATCH, contiguous=True)
    SB, NV, H, W, C = images_u8.shape
    return _gather_batch(N, "pnr_train_batch_u8" if jitter is None else "pnr_train_batch_u8_jitter", images_u8, (SB, NV, H, W), poses,
                         focal, c, pix_inds, z_near, z_far, C, int(bool(balanced)), jitter=jitter)


def views_to_tensor_u8(images_u8, view_ord, balanced=True, jitter=None):
    """The selected views of an 8-bit batch as the network's input, converted where they lie (pnr_views_to_tensor_u8):
    images_u8 (SB, NV, H, W, 3 | 4) uint8 and view_ord (SB, NS) long, both on the device -> (SB, NS, 3, H, W) float32, per view
    what image_to_tensor gives on it, bit for bit.  In place of batched_index_select_nd over float images.  A view index
    outside [0, NV) gives NaN planes (the indices are never read on the host); a repeated view is allowed.
    jitter: color_jitter_plan's record (SB, 8) — every pixel of a selected view goes through its object's colour chain
    (pnr_views_to_tensor_u8_jitter); None: the call and the bits without it."""
    from . import _native as N
    images_u8 = N.arg(images_u8, "images_u8", torch.uint8, _U8_BATCH, contiguous=True)
    SB, NV, H, W, C = images_u8.shape
    view_ord = N.arg(view_ord, "view_ord", torch.long, (SB, None), contiguous=True)
    NS = int(view_ord.shape[1])
    if NS < 1:
        raise ValueError(f"view_ord must name at least one view per object, got {tuple(view_ord.shape)}")
    if jitter is not None:
        jitter = N.arg(jitter, "jitter", torch.float32, (SB, 8), contiguous=True)
    dev = N.same_device(images_u8, view_ord, jitter)
    out = torch.empty(SB, NS, 3, H, W, dtype=torch.float32, device=dev)
    args = (N.ptr(images_u8), view_ord.data_ptr(), SB, NV, NS, W, H, C, int(bool(balanced)), N.ptr(out))
    if jitter is None:
        N.check(N.lib.pnr_views_to_tensor_u8(*args, N.current_stream(dev)), "pnr_views_to_tensor_u8")
    else:
        N.check(N.lib.pnr_views_to_tensor_u8_jitter(*args, N.ptr(jitter), N.current_stream(dev)), "pnr_views_to_tensor_u8_jitter")
    return out


def train_draw(bbox, SB, NV, W, H, B, NS, seed, out_pix=None, out_views=None, obj_base=0):
    """The draws of one training step on the device (pnr_train_draw; include/pnr.h writes the arithmetic down): B pixels per
    object — a uniform view, then a uniform cell of its box, or of the whole image when bbox is None — and an ordered
    subset of NS of its NV views, all keyed by `seed` alone (the caller's per-step key, parallel.frame_seed(base, step)).
    bbox (SB, NV, 4) = cmin, rmin, cmax, rmax float32 on the device, or None; out_pix (SB, B) / out_views (SB, NS) int64 on
    the device are filled when given (out_pix names the device when there are no boxes), else allocated on bbox's device or
    the current one.  -> (pix_inds, view_ord) for train_batch / train_batch_u8 / views_to_tensor_u8 / batched_index_select_nd.
    An invalid box (NaN, inverted, outside the image) gives index -1, a NaN row downstream.  Reads nothing back.
    obj_base: the call draws objects obj_base .. obj_base + SB - 1 of the step's batch (pnr_train_draw_at; bbox and the outputs
    are those SB objects' rows): what it writes are those rows of the whole batch's draw, bit for bit."""
    from . import _native as N
    SB, NV, W, H, B, NS = int(SB), int(NV), int(W), int(H), int(B), int(NS)
    if bbox is not None:
        bbox = N.arg(bbox, "bbox", torch.float32, (SB, NV, 4), contiguous=True)
    seed, obj_base, pix, views, dev = _draw_setup(N, "train_draw", SB, NV, W, H, B, NS, seed, obj_base, out_pix, out_views, bbox)
    N.check(N.lib.pnr_train_draw_at(N.dptr(bbox), SB, NV, W, H, B, NS, seed, obj_base,
                                    pix.data_ptr() if B else None, views.data_ptr() if NS else None, N.current_stream(dev)),
            "pnr_train_draw_at")
    return pix, views


def _draw_setup(N, what, SB, NV, W, H, B, NS, seed, obj_base, out_pix, out_views, t0, t1=None):
    """What train_draw and train_draw_masked share, on sizes that are host ints already and input tensors (t0, t1; None where
    there is none) that are checked already: the sizes' ranges, the two keys, the outputs, given or new, and the device of the
    call: the one its tensors share, or the current one when there is none (no boxes, no outputs).  N: the caller's _native.
    -> (seed, obj_base, pix, views, dev)."""
    if SB < 1 or NV < 1 or W < 1 or H < 1 or B < 0:
        raise ValueError(f"{what} needs SB, NV, W, H >= 1 and B >= 0, got {(SB, NV, W, H, B)}")
    if not 0 <= NS <= min(NV, 64):
        raise ValueError(f"NS must lie in [0, min(NV, 64)] = [0, {min(NV, 64)}], got {NS}")
    seed, obj_base = N.key64(seed, "seed"), N.key64(obj_base, "obj_base", _OBJ_BASE_END)
    first = t0 if t0 is not None else out_pix if out_pix is not None else out_views
    where = torch.device("cuda", torch.cuda.current_device()) if first is None else getattr(first, "device", None)
    pix = N.out(out_pix, "out_pix", torch.long, (SB, B), where)
    views = N.out(out_views, "out_views", torch.long, (SB, NS), where)
    return seed, obj_base, pix, views, N.same_device(t0, t1, pix, views)


def masked_sample(masks, num_pix, prop_inside, thresh=0.5):
    """num_pix pixels of which int(num_pix * prop_inside + 0.5) lie inside the mask and the rest outside, each uniform over all
    views' pixels of its kind (reference util.py:210-222): masks (NV, H, W) or (NV, 1, H, W) on the host, inside where
    masks >= thresh -> (num_pix, 3) long rows (view, row, col), the insides first.  Consumes torch's global CPU generator in the
    reference's order — one randint for the insides, one for the outsides — so the same torch.manual_seed gives the same pixels
    (tests/golden/masked_sample.npz).  An empty population raises ValueError (the reference's randint(0, 0) raises too)."""
    masks = torch.as_tensor(masks)
    if masks.dim() == 4 and masks.shape[1] == 1:
        masks = masks[:, 0]
    if masks.dim() != 3:
        raise ValueError(f"masks must be (NV, H, W) or (NV, 1, H, W), got {tuple(masks.shape)}")
    num_pix = int(num_pix)
    num_inside = int(num_pix * prop_inside + 0.5)
    if not 0 <= num_inside <= num_pix:
        raise ValueError(f"prop_inside must lie in [0, 1], got {prop_inside}")
    inside = (masks >= thresh).nonzero(as_tuple=False)
    outside = (masks < thresh).nonzero(as_tuple=False)
    if inside.shape[0] == 0 or outside.shape[0] == 0:
        raise ValueError(f"masked_sample needs pixels inside and outside the mask, got {inside.shape[0]} and {outside.shape[0]}")
    pix_inside = inside[torch.randint(0, inside.shape[0], (num_inside,))]
    pix_outside = outside[torch.randint(0, outside.shape[0], (num_pix - num_inside,))]
    return torch.cat((pix_inside, pix_outside))


def num_inside(B, prop_inside):
    """The inside slots of B mask-weighted draws: int(B * prop_inside + 0.5), as reference util.py:214 rounds."""
    prop_inside = float(prop_inside)
    if not 0.0 <= prop_inside <= 1.0:
        raise ValueError(f"prop_inside must lie in [0, 1], got {prop_inside}")
    return min(int(int(B) * prop_inside + 0.5), int(B))


def mask_bytes(masks):
    """Masks as the bytes mask_table thresholds: uint8 is used as it lies, bool / float becomes 0 / 255 by `>= 0.5`.  A float
    BATCH with the channel axis the datasets give their float masks, (SB, NV, 1, H, W), loses that axis; anything else keeps its
    shape.  -> uint8 (.., NV, H, W)."""
    if not torch.is_tensor(masks):
        raise ValueError(f"masks must be a tensor, got {type(masks).__name__}")
    if masks.dim() == 5 and masks.shape[2] == 1 and masks.is_floating_point():
        masks = masks.squeeze(2)
    if masks.dtype == torch.uint8:
        return masks
    if masks.dtype == torch.bool:
        return masks.to(torch.uint8) * 255
    return (masks >= 0.5).to(torch.uint8) * 255


def mask_table(masks, thresh=128, pix_stride=1, out=None):
    """The bit table mask-weighted draws select from (pnr_mask_table_build; include/pnr.h writes the layout down): masks
    (N, NV, H, W) or (NV, H, W) on the device — uint8 as it lies, bool / float through mask_bytes first — a pixel inside iff
    byte >= thresh (1..255).  -> (bits (N, NV * H, ceil(W / 32)), rows (N, NV * H + 1)), int32 device tensors holding the uint32
    patterns: the pixels' bits LSB first with a zero tail, and the prefix of the rows' popcounts.
    pix_stride > 1: masks is (N, NV, H, W, pix_stride) uint8 (or without N) and the byte of channel 0 of each pixel is read where
    it lies — hand in images[..., 3:] (a view, not copied) for an alpha channel.  out: (bits, rows) contiguous int32 tensors of
    those shapes to fill, e.g. an object's slot of a pool.  Reads nothing back."""
    from . import _native as N
    thresh, pix_stride = int(thresh), int(pix_stride)
    if not 1 <= thresh <= 255:
        raise ValueError(f"thresh must lie in 1..255, got {thresh}")
    if pix_stride < 1:
        raise ValueError(f"pix_stride must be >= 1, got {pix_stride}")
    if pix_stride == 1:
        masks = mask_bytes(masks)
        if masks.dim() == 3:
            masks = masks[None]
        masks = N.arg(masks, "masks", torch.uint8, (None, None, None, None), contiguous=True)
        n, NV, H, W = (int(s) for s in masks.shape)
    else:
        if torch.is_tensor(masks) and masks.dim() == 4:
            masks = masks[None]
        masks = N.arg(masks, "masks", torch.uint8, (None, None, None, None, None))
        n, NV, H, W = (int(s) for s in masks.shape[:4])
        want = (NV * H * W * pix_stride, H * W * pix_stride, W * pix_stride, pix_stride)
        if masks.shape[4] < 1 or any(masks.shape[d] > 1 and masks.stride(d) != want[d] for d in range(4)):
            raise ValueError(f"masks must view pixels {pix_stride} bytes apart in a contiguous (N, NV, H, W, {pix_stride}) buffer, "
                             f"got strides {masks.stride()}")
    if min(n, NV, H, W) < 1 or NV * H * W >= 1 << 31:
        raise ValueError(f"mask_table needs N, NV, H, W >= 1 and NV * H * W < 2^31, got {(n, NV, H, W)}")
    R, Wd = NV * H, (W + 31) // 32
    bits, rows = (None, None) if out is None else out
    if out is not None and (bits is None or rows is None):
        raise ValueError("out must be a (bits, rows) pair of tensors")
    bits = N.out(bits, "out bits", torch.int32, (n, R, Wd), masks.device)
    rows = N.out(rows, "out rows", torch.int32, (n, R + 1), masks.device)
    dev = N.same_device(masks, bits, rows)
    N.check(N.lib.pnr_mask_table_build(masks.data_ptr(), n, NV, H, W, pix_stride, thresh, bits.data_ptr(), rows.data_ptr(),
                                       N.current_stream(dev)), "pnr_mask_table_build")
    return bits, rows


def train_draw_masked(bits, rows, SB, NV, W, H, B, NS, seed, prop_inside, out_pix=None, out_views=None, obj_base=0):
    """train_draw with a mask in place of the boxes (pnr_train_draw_masked_at; include/pnr.h writes the arithmetic down): of the B
    pixels of an object the first num_inside(B, prop_inside) are uniform over its INSIDE pixels, the rest over its OUTSIDE
    pixels, all NV views pooled — the reference's masked_sample, keyed by `seed` alone.  bits (SB, NV * H, ceil(W / 32)) and
    rows (SB, NV * H + 1): mask_table's int32 tensors on the device.  The views, the outputs, out_pix / out_views and obj_base
    are train_draw's.  An object without inside (or without outside) pixels draws every slot from the population it has.
    Reads nothing back."""
    from . import _native as N
    SB, NV, W, H, B, NS = int(SB), int(NV), int(W), int(H), int(B), int(NS)
    B_inside = num_inside(B, prop_inside)
    bits = N.arg(bits, "bits", torch.int32, (SB, NV * H, (W + 31) // 32), contiguous=True)
    rows = N.arg(rows, "rows", torch.int32, (SB, NV * H + 1), contiguous=True)
    seed, obj_base, pix, views, dev = _draw_setup(N, "train_draw_masked", SB, NV, W, H, B, NS, seed, obj_base, out_pix, out_views,
                                                  bits, rows)
    N.check(N.lib.pnr_train_draw_masked_at(bits.data_ptr(), rows.data_ptr(), SB, NV, W, H, B, B_inside, NS, seed, obj_base,
                                           pix.data_ptr() if B else None, views.data_ptr() if NS else None,
                                           N.current_stream(dev)), "pnr_train_draw_masked_at")
    return pix, views


def mask_gather(bits, pix_inds, NV, H, W, out=None):
    """The mask's value at sampled pixels, read from the bit table the mask-weighted draws use (pnr_mask_gather): bits
    (SB, NV * H, ceil(W / 32)) int32 (mask_table, or data.ResidentSplit(device_masks=True)) and pix_inds (SB, B) int64, both on
    the device -> float32 (SB, B): 1.0 where the pixel's bit is set, else 0.0; NaN for an index outside [0, NV * H * W), as
    train_batch gives such a row.  out: a contiguous float32 (SB, B) tensor to fill.  One launch; reads nothing back."""
    from . import _native as N
    NV, H, W = int(NV), int(H), int(W)
    if min(NV, H, W) < 1 or NV * H * W >= 1 << 31:
        raise ValueError(f"mask_gather needs NV, H, W >= 1 and NV * H * W < 2^31, got {(NV, H, W)}")
    pix_inds = N.arg(pix_inds, "pix_inds", torch.long, (None, None), contiguous=True)
    SB, B = (int(x) for x in pix_inds.shape)
    if SB < 1:
        raise ValueError(f"pix_inds must hold at least one object, got {tuple(pix_inds.shape)}")
    bits = N.arg(bits, "bits", torch.int32, (SB, NV * H, (W + 31) // 32), contiguous=True)
    mask = N.out(out, "out", torch.float32, (SB, B), bits.device)
    dev = N.same_device(bits, pix_inds, mask)
    N.check(N.lib.pnr_mask_gather(bits.data_ptr(), SB, NV, H, W, pix_inds.data_ptr(), B, mask.data_ptr(), N.current_stream(dev)),
            "pnr_mask_gather")
    return mask


def _record_stride(t, lead, last, name):
    """Floats per element of a tensor of shape lead [+ (last,)] — lead = (H, W) for a frame, (n,) for per-ray outputs — that is
    dense or a regular view into a packed per-element record: unit stride inside the element and, for a frame, row-major
    pixels ((H, W, 3) with strides (W s, s, 1), (H, W) with (W s, s); (n, last) with (s, 1), (n,) with s)."""
    from . import _native as N
    N.arg(t, name, torch.float32, (*lead, last) if last else tuple(lead))
    if t.is_contiguous():
        return max(last, 1)
    st, k = t.stride(), len(lead)
    s = st[k - 1]
    if s < max(last, 1) or (last > 1 and st[k] != 1) or (k == 2 and lead[0] > 1 and st[0] != lead[1] * s):
        raise ValueError(f"{name} must be dense or a view into a per-{'pixel' if k == 2 else 'ray'} record, got strides {st}")
    return s


def _field_stride(t, name):
    """Floats per sample of a float32 (nx, ny, nz) field that is dense or a regularly strided view — one column of a per-point
    record, read where it lies —: strides (ny nz s, nz s, s) with s >= 1.  What recon.extract_mesh and
    OccupancyGrid.from_sigma take."""
    from . import _native as N
    _, ny, nz = N.arg(t, name, torch.float32, (None, None, None)).shape
    st = t.stride()
    s = int(st[2])
    if s < 1 or st[1] != nz * s or st[0] != ny * nz * s:
        raise ValueError(f"{name} must be dense or a regularly strided view of a per-point record, got strides {st}")
    return s


def eval_frame(rgb, depth=None, gt=None, *, z_near=0.0, z_far=1.0, want_u8=True, want_compare=False, want_depth=False,
               want_metrics=True, metrics_out=None):
    """What the evaluation loop does with a rendered frame (eval/eval.py:286-347), on the GPU by libpnr_hip (pnr_eval_frame):
    rgb (H, W, 3) UNclamped, depth (H, W), both float32, dense or views into the packed (H*W, 4) per-ray record; gt (3, H, W)
    in [-1, 1] as the data loader gives it.  -> (rgb_u8 (H, W, 3) uint8, compare_u8 (H, 2W, 3) uint8, depth_norm (H, W)
    float32, metrics (2,) float64 = [mean squared error, mean SSIM]) on the device, None for what was not asked for.
    metrics_out: a contiguous (2,) float64 device tensor to write the pair into (one row of a per-object buffer).  Nothing
    here waits for the device; PSNR = 10 log10(1 / metrics[0]) is the caller's, on the host."""
    from . import _native as N
    H, W = (int(s) for s in N.arg(rgb, "rgb", torch.float32, (None, None, 3)).shape[:2])
    if (want_compare or want_metrics) and gt is None:
        raise ValueError("want_compare / want_metrics need the ground truth gt")
    if want_depth and depth is None:
        raise ValueError("want_depth needs depth")
    if not want_depth:
        depth = None
    if not (want_compare or want_metrics):
        gt = None
    rs = _record_stride(rgb, (H, W), 3, "rgb")
    ds = 0 if depth is None else _record_stride(depth, (H, W), 0, "depth")
    if gt is not None:
        gt = N.arg(gt, "gt", torch.float32, (3, H, W), contiguous=True)
    metrics = N.out(metrics_out, "metrics_out", torch.float64, (2,), rgb.device) if want_metrics else None
    dev = N.same_device(rgb, depth, gt, metrics_out)
    rgb_u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    compare_u8 = torch.empty(H, 2 * W, 3, dtype=torch.uint8, device=dev) if want_compare else None
    depth_norm = torch.empty(H, W, dtype=torch.float32, device=dev) if want_depth else None
    ws = None
    nbytes = 0
    if want_metrics:
        nbytes = int(N.lib.pnr_eval_frame_workspace_bytes(W, H))
        ws = N.scratch(nbytes, dev)
    N.check(N.lib.pnr_eval_frame(rgb.data_ptr(), rs, N.dptr(depth), ds, N.dptr(gt), W, H, float(z_near), float(z_far),
                                 N.dptr(rgb_u8), N.dptr(compare_u8), N.dptr(depth_norm), N.dptr(metrics), N.dptr(ws), nbytes,
                                 N.current_stream(dev)), "pnr_eval_frame")
    return rgb_u8, compare_u8, depth_norm, metrics


def eval_frames(rgb, gt, *, clamp=False, metrics_out=None):
    """The metrics of eval_frame for F frames in ONE call, on the GPU by libpnr_hip (pnr_eval_frames): what the approximate
    evaluation does with the SB target views of a batch (eval/eval_approx.py:136-148).  rgb (F, H, W, 3) or (F, H*W, 3) float32
    as the render left it — dense, or a regular view into a packed per-ray record such as the (N, 4) record, with any gap between
    the frames; gt (F, 3, H, W) float32 in [-1, 1].  clamp=False compares the render as it is, as eval_approx.py does;
    clamp=True clamps it to [0, 1] first, and row f is then bit for bit eval_frame's pair of frame f.
    -> (F, 2) float64 on the device, rows [mean squared error, mean SSIM]; metrics_out: a contiguous (F, 2) float64 device
    tensor to write into.  Nothing here waits for the device; PSNR = 10 log10(1 / mse) is the caller's, on the host."""
    from . import _native as N
    gt = N.arg(gt, "gt", torch.float32, (None, 3, None, None), contiguous=True)
    F, _, H, W = (int(s) for s in gt.shape)
    if F < 1:
        raise ValueError(f"gt must hold at least one frame, got {tuple(gt.shape)}")
    N.arg(rgb, "rgb", torch.float32, (F, H * W, 3) if torch.is_tensor(rgb) and rgb.dim() == 3 else (F, H, W, 3))
    rs = _record_stride(rgb[0], (H, W) if rgb.dim() == 4 else (H * W,), 3, "a frame of rgb")
    fs = 0
    if F > 1:
        fs = int(rgb.stride(0))
        if fs < H * W * rs:
            raise ValueError(f"the frames of rgb must follow each other at >= {H * W * rs} floats, got strides {rgb.stride()}")
    metrics = N.out(metrics_out, "metrics_out", torch.float64, (F, 2), gt.device)
    dev = N.same_device(rgb, gt, metrics)
    nbytes = int(N.lib.pnr_eval_frames_workspace_bytes(F, W, H))
    ws = N.scratch(nbytes, dev)
    N.check(N.lib.pnr_eval_frames(rgb.data_ptr(), rs, fs, gt.data_ptr(), F, W, H, int(bool(clamp)), metrics.data_ptr(),
                                  ws.data_ptr(), nbytes, N.current_stream(dev)), "pnr_eval_frames")
    return metrics


def eval_frames_u8(pred_u8, gt_u8, *, want_planar=False, metrics_out=None):
    """The metrics of eval_frames for F pairs of saved 8-bit images, on the GPU by libpnr_hip (pnr_eval_frames_u8): what
    eval/calc_metrics.py:218-234 does with the PNGs eval.py wrote.  pred_u8, gt_u8: uint8 device tensors (F, H, W, 3 | 4),
    interleaved as a PNG decoder returns them (a non-dense view is made dense); a fourth channel is never read into a result.
    x = p / 255 in fp32 (the bits of imread(..).astype(np.float32) / 255.0), then the arithmetic of eval_frames.
    -> (F, 2) float64 on the device, rows [mean squared error, mean SSIM]; with want_planar -> (metrics, pred_planar,
    gt_planar), the two (F, 3, H, W) float32 tensors x * 2 - 1, the LPIPS inputs of :232-233.  metrics_out: a contiguous
    (F, 2) float64 device tensor to write into.  Nothing here waits for the device; PSNR is the caller's, on the host."""
    from . import _native as N
    pred_u8 = N.arg(pred_u8, "pred_u8", torch.uint8, (None, None, None, (3, 4)), contiguous=True)
    F, H, W, pc = (int(s) for s in pred_u8.shape)
    if F < 1:
        raise ValueError(f"pred_u8 must hold at least one frame, got {tuple(pred_u8.shape)}")
    gt_u8 = N.arg(gt_u8, "gt_u8", torch.uint8, (F, H, W, (3, 4)), contiguous=True)
    metrics = N.out(metrics_out, "metrics_out", torch.float64, (F, 2), pred_u8.device)
    dev = N.same_device(pred_u8, gt_u8, metrics)
    pred_planar = torch.empty(F, 3, H, W, dtype=torch.float32, device=dev) if want_planar else None
    gt_planar = torch.empty(F, 3, H, W, dtype=torch.float32, device=dev) if want_planar else None
    nbytes = int(N.lib.pnr_eval_frames_u8_workspace_bytes(F, W, H))
    ws = N.scratch(nbytes, dev)
    N.check(N.lib.pnr_eval_frames_u8(pred_u8.data_ptr(), pc, gt_u8.data_ptr(), int(gt_u8.shape[3]), F, W, H, N.dptr(pred_planar),
                                     N.dptr(gt_planar), metrics.data_ptr(), ws.data_ptr(), nbytes, N.current_stream(dev)),
            "pnr_eval_frames_u8")
    return (metrics, pred_planar, gt_planar) if want_planar else metrics


def _upsample_sizes(shapes):
    arr = lambda k: (C.c_int32 * len(shapes))(*[int(s[k]) for s in shapes])
    return arr(1), arr(2), arr(3)


class _UpsampleConcat(torch.autograd.Function):
    """pnr_upsample_concat and its adjoint pnr_upsample_concat_bwd.  Saves nothing but the level shapes: the map is linear in
    the levels and its weights depend on the sizes alone."""

    @staticmethod
    def forward(ctx, half_dtype, *levels):
        from . import _native as N
        dev = N.same_device(*levels)
        shapes = [tuple(l.shape) for l in levels]
        n, (h0, w0) = shapes[0][0], shapes[0][2:]
        sum_c = sum(s[1] for s in shapes)
        out = torch.empty(n, sum_c, h0, w0, device=dev, dtype=torch.float32)
        out16 = None
        if half_dtype is not None:
            out16 = torch.empty((n, sum_c, h0, w0), device=dev, dtype=half_dtype, memory_format=torch.channels_last)
        if n > 0:
            lat_c, lat_h, lat_w = _upsample_sizes(shapes)
            ptrs = (C.c_void_p * len(levels))(*[N.ptr(l) for l in levels])
            dt = N.PNR_F32 if half_dtype is None else (N.PNR_F16 if half_dtype == torch.float16 else N.PNR_BF16)
            N.check(N.lib.pnr_upsample_concat(ptrs, lat_c, lat_h, lat_w, len(levels), n, N.ptr(out),
                                              N.dptr(out16), dt, N.current_stream(dev)), "pnr_upsample_concat")
        ctx.shapes, ctx.device = shapes, dev
        if out16 is None:
            return out
        ctx.mark_non_differentiable(out16)
        return out, out16

    @staticmethod
    def backward(ctx, d_out, *_):
        from . import _native as N
        shapes, dev = ctx.shapes, ctx.device
        grads = [torch.empty(s, device=dev, dtype=torch.float32) if need else None
                 for s, need in zip(shapes, ctx.needs_input_grad[1:])]
        if shapes[0][0] > 0 and any(g is not None for g in grads):
            lat_c, lat_h, lat_w = _upsample_sizes(shapes)
            ptrs = (C.c_void_p * len(shapes))(*[N.dptr(g) for g in grads])
            d_out = N.f32c(d_out)
            N.check(N.lib.pnr_upsample_concat_bwd(N.ptr(d_out), lat_c, lat_h, lat_w, len(shapes), shapes[0][0], ptrs,
                                                  N.current_stream(dev)), "pnr_upsample_concat_bwd")
        return (None, *grads)


def upsample_concat(levels, half_dtype=None):
    """The tail of upstream pixelNeRF's SpatialEncoder.forward on the GPU by libpnr_hip (pnr_upsample_concat): levels, a list
    of (N, C_i, H_i, W_i) float32 device tensors, each resized to level 0's size (bilinear, align_corners=True) and
    concatenated along the channels -> out (N, sum C_i, H_0, W_0) float32.  half_dtype = torch.float16 / torch.bfloat16:
    -> (out, out16), out16 the same values rounded to nearest even, channels-last — the image the 16-bit render kernels
    gather from (sum C_i % 8 == 0).  Differentiable in the levels; the backward is the deterministic gather kernel
    (pnr_upsample_concat_bwd) and runs only for the levels that require grad.  include/pnr.h fixes the arithmetic."""
    from . import _native as N
    levels = list(levels)
    if not levels or len(levels) > N.PNR_MAX_LEVELS:
        raise ValueError(f"upsample_concat takes 1..{N.PNR_MAX_LEVELS} levels, got {len(levels)}")
    if half_dtype not in (None, torch.float16, torch.bfloat16):
        raise ValueError(f"half_dtype must be None, torch.float16 or torch.bfloat16, got {half_dtype}")
    levels = [N.arg(l, f"level {i} (all of one N)", torch.float32, (levels[0].shape[0] if i else None, None, None, None), contiguous=True)
              for i, l in enumerate(levels)]
    return _UpsampleConcat.apply(half_dtype, *levels)


# ------------------------------------------------------------------------------------------- colour map and the vis_step panel
def hot_lut():
    """The package's default colour table, (256, 3) uint8 in RGB order: the "hot" ramp black - red - yellow - white,
    r = min(1, x / 0.375), g = clamp((x - 0.375) / 0.375, 0, 1), b = clamp((x - 0.75) / 0.25, 0, 1) for x = i / 255 in fp64,
    each byte floor(255 v + 0.5).  PARITY UNPINNED: the reference indexes cv2.COLORMAP_HOT (src/util/util.py:26-30), cv2 is
    not importable where this package is developed, OpenCV's own table may differ from this ramp, and OpenCV returns BGR, which
    the reference shows unswapped.  With cv2 at hand pass
    lut=cv2.applyColorMap(np.arange(256, dtype=np.uint8), cv2.COLORMAP_HOT)[:, 0] to cmap / cmap_device / vis_panel."""
    x = np.arange(256, dtype=np.float64) / 255.0
    r = np.minimum(1.0, x / 0.375)
    g = np.clip((x - 0.375) / 0.375, 0.0, 1.0)
    b = np.clip((x - 0.75) / 0.25, 0.0, 1.0)
    return np.floor(255.0 * np.stack((r, g, b), axis=-1) + 0.5).astype(np.uint8)


def image_float_to_uint8(img):
    """The reference's image_float_to_uint8 (src/util/util.py:13-23) for a float32 map, as include/pnr.h states it: whole-frame
    fp32 min / max (a NaN anywhere makes both NaN), vmax widened by 1e-10 when the range is below 1e-10, (x - vmin) /
    (vmax - vmin) in fp32, ONE fp32 product with 255, truncation; a product that is not finite gives byte 0."""
    img = np.asarray(img, dtype=np.float32)
    vmin, vmax = np.float32(np.min(img)), np.float32(np.max(img))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if float(vmax - vmin) < 1e-10:
            vmax = np.float32(float(vmax) + 1e-10)
        p = ((img - vmin) / np.float32(vmax - vmin)) * np.float32(255.0)
    out = np.zeros(img.shape, np.uint8)
    ok = np.isfinite(p)
    out[ok] = p[ok].astype(np.int32).astype(np.uint8)
    return out


def cmap(img, lut=None):
    """The reference's util.cmap (src/util/util.py:26-30) on the host in pure numpy, with the colour table as data:
    lut[image_float_to_uint8(img)] -> (H, W, 3) uint8.  lut (256, 3) uint8; None = hot_lut() (parity unpinned, see there)."""
    lut = hot_lut() if lut is None else _checked_lut(np.asarray(lut), np.uint8)
    return lut[image_float_to_uint8(img)]


def _checked_lut(lut, uint8):
    """A colour table, array or tensor, that is (256, 3) of its library's uint8."""
    if tuple(lut.shape) != (256, 3) or lut.dtype != uint8:
        raise ValueError(f"lut must be uint8 (256, 3), got {lut.dtype} {tuple(lut.shape)}")
    return lut


_LUT_CACHE = {}


def _device_lut(lut, dev):
    """(256, 3) uint8 table on `dev`: a device tensor passes through; the default table is uploaded once per device."""
    if lut is None:
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        t = _LUT_CACHE.get(key)
        if t is None:
            t = _LUT_CACHE[key] = upload(torch.from_numpy(hot_lut()), dev)
        return t
    if not torch.is_tensor(lut):
        lut = torch.from_numpy(np.ascontiguousarray(lut))
    return upload(_checked_lut(lut, torch.uint8), dev).contiguous()


def cmap_device(map, lut=None):
    """util.cmap on the GPU by libpnr_hip (pnr_cmap): map (H, W) float32, dense or a view into a per-pixel record ->
    (u8 (H, W, 3) uint8 = lut[image_float_to_uint8(map)], minmax (2,) float32 = the map's min and max), both on the device.
    lut: (256, 3) uint8, numpy or tensor; None = hot_lut(), uploaded once per device (parity unpinned, see hot_lut).  Nothing
    here waits for the device."""
    from . import _native as N
    H, W = (int(s) for s in N.arg(map, "map", torch.float32, (None, None)).shape)
    stride = _record_stride(map, (H, W), 0, "map")
    dev = N.same_device(map)
    lut = _device_lut(lut, dev)
    N.same_device(map, lut)
    u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
    minmax = torch.empty(2, dtype=torch.float32, device=dev)
    nbytes = int(N.lib.pnr_cmap_workspace_bytes(W, H))
    ws = N.scratch(nbytes, dev)
    N.check(N.lib.pnr_cmap(map.data_ptr(), stride, W, H, lut.data_ptr(), u8.data_ptr(), minmax.data_ptr(), ws.data_ptr(),
                           nbytes, N.current_stream(dev)), "pnr_cmap")
    return u8, minmax


class VisPanel:
    """What vis_panel leaves on the device: panel (n_pass H, (NS + 4) W, 3) float32, panel_u8 the same as uint8, alpha
    (n_pass, H, W), stats (n_pass, 6) = rgb min max, alpha min max, depth min max, mse and psnr = -10 log10(mse) as 0-dim
    float64 tensors.  None for what was not asked for."""
    __slots__ = ("panel", "panel_u8", "alpha", "stats", "mse", "psnr")

    def __init__(self, panel, panel_u8, alpha, stats, mse, psnr):
        self.panel, self.panel_u8, self.alpha, self.stats, self.mse, self.psnr = panel, panel_u8, alpha, stats, mse, psnr


def vis_panel(images, src_views, gt_view, passes, *, lut=None, want_f32=True, want_u8=False, want_alpha=False):
    """The picture of the reference's vis_step (train/train.py:497-526) for one target view, on the GPU by libpnr_hip
    (pnr_vis_panel): per pass one row [source views | ground truth | cmap(depth) | rgb | cmap(alpha)], coarse over fine.
    images (NV, 3, H, W) float32 in [-1, 1] on the device; src_views 1..8 view indices and gt_view, on the host; passes a list
    of one or two (rgb (H W, 3), depth (H W), weights (H W, K)), float32, dense or views into a packed per-ray record.
    -> VisPanel; everything stays on the device and nothing waits.  lut as in cmap_device.  include/pnr.h fixes the arithmetic
    (alpha is an fp64 sum in ascending k, not torch's .sum(-1); the default table is parity unpinned)."""
    from . import _native as N
    images = N.arg(images, "images", torch.float32, (None, 3, None, None), contiguous=True)
    NV, _, H, W = (int(s) for s in images.shape)
    src = [int(v) for v in (src_views.tolist() if hasattr(src_views, "tolist") else src_views)]
    NS, n_pass = len(src), len(passes)
    if not 1 <= NS <= N.PNR_VIS_MAX_SRC:
        raise ValueError(f"vis_panel takes 1..{N.PNR_VIS_MAX_SRC} source views, got {NS}")
    if n_pass not in (1, 2):
        raise ValueError(f"vis_panel takes one or two passes, got {n_pass}")
    arr = (N.pnr_vis_pass * n_pass)()
    for i, (rgb, depth, weights) in enumerate(passes):
        K = arr[i].K = int(N.arg(weights, "weights", torch.float32, (H * W, None)).shape[1])
        arr[i].rgb_stride = _record_stride(rgb, (H * W,), 3, "rgb")
        arr[i].depth_stride = _record_stride(depth, (H * W,), 0, "depth")
        arr[i].weights_stride = _record_stride(weights, (H * W,), K, "weights")
        arr[i].rgb, arr[i].depth, arr[i].weights = rgb.data_ptr(), depth.data_ptr(), weights.data_ptr()
    dev = N.same_device(images, *[t for ps in passes for t in ps])
    lut = _device_lut(lut, dev)
    N.same_device(images, lut)
    panel = torch.empty(n_pass * H, (NS + 4) * W, 3, dtype=torch.float32, device=dev) if want_f32 else None
    panel_u8 = torch.empty(n_pass * H, (NS + 4) * W, 3, dtype=torch.uint8, device=dev) if want_u8 else None
    alpha = torch.empty(n_pass, H, W, dtype=torch.float32, device=dev) if want_alpha else None
    stats = torch.empty(n_pass, 6, dtype=torch.float32, device=dev)
    mse = torch.empty((), dtype=torch.float64, device=dev)
    nbytes = int(N.lib.pnr_vis_panel_workspace_bytes(W, H, n_pass))
    ws = N.scratch(nbytes, dev)
    N.check(N.lib.pnr_vis_panel(images.data_ptr(), NV, (C.c_int32 * NS)(*src), NS, int(gt_view), arr, n_pass, W, H,
                                lut.data_ptr(), N.dptr(panel), N.dptr(panel_u8), N.dptr(alpha), stats.data_ptr(),
                                mse.data_ptr(), ws.data_ptr(), nbytes, N.current_stream(dev)), "pnr_vis_panel")
    return VisPanel(panel, panel_u8, alpha, stats, mse, -10.0 * torch.log10(mse))


# ------------------------------------------------------------------------------------------- the ends of the video drivers
def video_frames(rgb, F, H, W, out=None, count=None):
    """(frames * 255).astype(np.uint8) of the video drivers (eval/gen_video.py:236, eval/eval_real.py:151) for a stack of F
    rendered frames, on the GPU by libpnr_hip in ONE launch (pnr_video_frames).  rgb: F*H*W pixels, float32, UNclamped — a
    contiguous tensor of 3 F H W elements in any shape, or (F*H*W, 3) as a view into the packed (F*H*W, 4) per-ray record.
    -> (frames_u8 (F, H, W, 3) uint8, n_out_of_range 0-dim int64), both on the device.  In range (-1 < x * 255 < 256) the
    byte is numpy's; elsewhere (NaN included) numpy's cast is undefined, the byte saturates to 0 / 255 and the component is
    counted.  out: a contiguous uint8 tensor of 3 F H W elements to write into, at any byte offset of a larger buffer;
    count: a contiguous int64 device tensor of one element, set by the call.  Nothing here waits for the device."""
    from . import _native as N
    F, H, W = int(F), int(H), int(W)
    P = F * H * W
    if N.arg(rgb, "rgb", torch.float32, (...,)).is_contiguous() and rgb.numel() == 3 * P:
        stride = 3
    else:
        stride = _record_stride(rgb, (P,), 3, "rgb")
    # out and count are "N elements of any shape", which N.out's exact shape does not say: their rule stays written out here
    if out is not None and (out.dtype != torch.uint8 or out.numel() != 3 * P or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 tensor of {3 * P} elements, got {out.dtype} {tuple(out.shape)}")
    if count is not None and (count.dtype != torch.int64 or count.numel() != 1 or not count.is_contiguous()):
        raise ValueError(f"count must be a contiguous int64 tensor of one element, got {count.dtype} {tuple(count.shape)}")
    dev = N.same_device(rgb, out, count)
    if out is None:
        out = torch.empty(F, H, W, 3, dtype=torch.uint8, device=dev)
    if count is None:
        count = torch.empty((), dtype=torch.int64, device=dev)
    N.check(N.lib.pnr_video_frames(rgb.data_ptr(), stride, F, W, H, out.data_ptr(), count.data_ptr(), N.current_stream(dev)),
            "pnr_video_frames")
    return out.view(F, H, W, 3), count


def view_strip(images, scale=0.5, lo=0.5, out=None):
    """The picture of the source views the reference writes next to a video (eval/gen_video.py:239-241), on the GPU by
    libpnr_hip (pnr_view_strip): images (NS, 3, H, W) float32 on the device -> (H, NS*W, 3) uint8 =
    np.hstack of ((x * scale + lo) * 255).astype(np.uint8) over the views, with video_frames' saturation outside numpy's
    range.  scale = lo = 0.5 for a [-1, 1] input, scale = 1, lo = 0 for [0, 1]."""
    from . import _native as N
    images = N.arg(images, "images", torch.float32, (None, 3, None, None), contiguous=True)
    NS, _, H, W = (int(s) for s in images.shape)
    out = N.out(out, "out", torch.uint8, (H, NS * W, 3), images.device)
    dev = N.same_device(images, out)
    N.check(N.lib.pnr_view_strip(images.data_ptr(), NS, W, H, float(scale), float(lo), out.data_ptr(), N.current_stream(dev)),
            "pnr_view_strip")
    return out


def image_to_tensor(img_u8, balanced=False, device="cuda"):
    """An 8-bit RGB image (H, W, 3) -> the network's input (3, H, W) float32 on the device, by libpnr_hip
    (pnr_image_to_tensor).  balanced=False: byte / 255 in [0, 1], torchvision's ToTensor, which is what the reference fork's
    get_image_to_tensor_balanced does (src/util/util.py:68-79); balanced=True: (byte / 255 - 0.5) / 0.5 in [-1, 1], upstream
    pixelNeRF's ToTensor + Normalize(0.5, 0.5).  Pinned to torch's own division; parity unpinned against torchvision itself.
    img_u8: a uint8 device tensor, or a numpy array / host tensor that is uploaded to `device` first."""
    from . import _native as N
    if not torch.is_tensor(img_u8):
        img_u8 = torch.from_numpy(np.ascontiguousarray(img_u8))
    N.arg(img_u8, "img_u8", torch.uint8, (None, None, 3))
    if not img_u8.is_cuda:
        img_u8 = upload(img_u8.contiguous(), torch.device(device))
    img_u8 = img_u8.contiguous()
    dev = N.same_device(img_u8)
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
    N.check(N.lib.pnr_image_to_tensor(img_u8.data_ptr(), W, H, int(bool(balanced)), out.data_ptr(), N.current_stream(dev)),
            "pnr_image_to_tensor")
    return out


# ------------------------------------------------------------------------------------------- procedural datasets
def synth_render(scenes, scene_ids, poses, W, H, focal, c=None, *, ss=2, ambient=0.3, light=(0.3, 0.5, 0.8), out=None,
                 mask_out=None, depth_out=None):
    """F frames of analytic scenes, ray-cast on the GPU by libpnr_hip in ONE launch (pnr_synth_render; include/pnr.h writes the
    scene records and every operation down).  scenes (n, P, 20) float32: P <= 8 primitive records per scene (kind, centre,
    world -> local rotation, half-extents, albedo), data.synthetic.random_scenes or a hand-written table; scene_ids (F,) int32:
    the scene of each frame (an index outside [0, n) gives a background frame); poses (F, 4, 4) float32 camera-to-world, the
    convention of gen_rays; focal / c as intrinsics() takes them.  ss: 1, 2 or 4 sub-samples per pixel and axis; ambient in
    [0, 1] and light, a direction fixed in the world, shade albedo * (ambient + (1 - ambient) * max(0, n . l)).
    -> (rgb_u8 (F, H, W, 3), mask_u8 (F, H, W) or None, depth (F, H, W) float32 or None) on the device.  Background pixels are
    255, 255, 255 with mask 0, and no channel of a foreground pixel is 255, so SRNDataset's rule reads the masks back from the
    bytes; depth is the ray parameter at the pixel's first sub-sample (its centre for ss = 1), +inf where that one missed.
    out: a contiguous uint8 (F, H, W, 3) to write into, at any byte offset of a larger buffer (a pool's slot).  mask_out /
    depth_out: None = not wanted, True = allocated here, or a contiguous uint8 (F, H, W) / float32 (F, H, W) to write into.
    Nothing here waits for the device."""
    from . import _native as N
    scenes = N.arg(scenes, "scenes", torch.float32, (None, None, N.PNR_SYNTH_REC), contiguous=True)
    scene_ids = N.arg(scene_ids, "scene_ids", torch.int32, (None,), contiguous=True)
    F, W, H = int(scene_ids.shape[0]), int(W), int(H)
    poses = N.arg(poses, "poses", torch.float32, (F, 4, 4), contiguous=True)
    if min(F, W, H) < 1:
        raise ValueError(f"frames and image sizes must be positive, got F = {F}, W = {W}, H = {H}")
    out = N.out(out, "out", torch.uint8, (F, H, W, 3), scenes.device)
    if mask_out is not None:
        mask_out = N.out(None if mask_out is True else mask_out, "mask_out", torch.uint8, (F, H, W), scenes.device)
    if depth_out is not None:
        depth_out = N.out(None if depth_out is True else depth_out, "depth_out", torch.float32, (F, H, W), scenes.device)
    light = tuple(float(v) for v in light)
    if len(light) != 3:
        raise ValueError(f"light must be three numbers, got {light}")
    dev = N.same_device(scenes, scene_ids, poses, out, mask_out, depth_out)
    fx, fy, cx, cy = intrinsics(focal, c, W, H)
    N.check(N.lib.pnr_synth_render(scenes.data_ptr(), int(scenes.shape[0]), int(scenes.shape[1]), scene_ids.data_ptr(),
                                   poses.data_ptr(), F, W, H, fx, fy, cx, cy, int(ss), float(ambient), *light, out.data_ptr(),
                                   3 * H * W, N.dptr(mask_out), N.dptr(depth_out), N.current_stream(dev)), "pnr_synth_render")
    return out, mask_out, depth_out


# ------------------------------------------------------------------------------------------- area resampling to an image_size
def _target_size(size):
    """(Ht, Wt) of a `size` argument: a pair, or one int for a square target."""
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    size = tuple(int(s) for s in size)
    if len(size) != 2:
        raise ValueError(f"size must be (Ht, Wt) or an int, got {size}")
    return size


def resize_area_u8(images_u8, size, out=None):
    """8-bit images at another size, by area resampling on the GPU by libpnr_hip (pnr_resize_area_u8; include/pnr.h writes the
    arithmetic down): images_u8 (..., H, W, C) uint8 on the device, C = 1..4 and any leading dimensions — (H, W, C),
    (NV, H, W, C), (N, NV, H, W, C) — -> (..., Ht, Wt, C) uint8.  A target byte is the exact mean of the source bytes under its
    window [floor(i n_in / n_out), ceil((i + 1) n_in / n_out)) per axis — the windows of F.interpolate(mode="area"), which
    upstream pixelNeRF applies to its float images — rounded to the nearest byte, a tie up.  Every channel is kept; a mask is
    the C = 1 case.  The target may be larger than the source, or equal to it (a copy).  size: (Ht, Wt), or an int for a square
    target.  out: a contiguous uint8 tensor of the result's shape to write into, at any byte offset of a larger buffer (a
    pool's slot).  Nothing here waits for the device."""
    from . import _native as N
    images_u8 = N.arg(images_u8, "images_u8", torch.uint8, (..., None, None, (1, 2, 3, 4)), contiguous=True)
    Ht, Wt = _target_size(size)
    lead = tuple(int(s) for s in images_u8.shape[:-3])
    H, W, C = (int(s) for s in images_u8.shape[-3:])
    F = math.prod(lead)
    out = N.out(out, "out", torch.uint8, lead + (Ht, Wt, C), images_u8.device)
    dev = N.same_device(images_u8, out)
    N.check(N.lib.pnr_resize_area_u8(images_u8.data_ptr(), H * W * C, F, H, W, C, out.data_ptr(), Ht * Wt * C, Ht, Wt,
                                     N.current_stream(dev)), "pnr_resize_area_u8")
    return out


def resize_area(images, size, out=None):
    """Float images at another size, by area resampling on the GPU by libpnr_hip (pnr_resize_area_f32): images (..., H, W)
    float32 on the device, any leading dimensions (views, channels) -> (..., Ht, Wt) float32, each value the mean of its
    window (resize_area_u8's windows) summed in fp64 and rounded to fp32 once — F.interpolate(mode="area") to within one fp32
    rounding.  A NaN or Inf reaches exactly the windows that contain it.  size and out as for resize_area_u8 (out float32).
    Nothing here waits for the device."""
    from . import _native as N
    images = N.arg(images, "images", torch.float32, (..., None, None), contiguous=True)
    Ht, Wt = _target_size(size)
    lead = tuple(int(s) for s in images.shape[:-2])
    H, W = int(images.shape[-2]), int(images.shape[-1])
    out = N.out(out, "out", torch.float32, lead + (Ht, Wt), images.device)
    dev = N.same_device(images, out)
    N.check(N.lib.pnr_resize_area_f32(images.data_ptr(), math.prod(lead), H, W, out.data_ptr(), Ht, Wt, N.current_stream(dev)),
            "pnr_resize_area_f32")
    return out


def _sizes(src, dst):
    (H, W), (Ht, Wt) = _target_size(src), _target_size(dst)
    if min(H, W, Ht, Wt) < 1:
        raise ValueError(f"image sizes must be positive, got {(H, W)} -> {(Ht, Wt)}")
    return H, W, Ht, Wt


def resize_bbox(bbox, src_size, dst_size):
    """Boxes (..., 4) = cmin, rmin, cmax, rmax (whole numbers, corners included) of images (H, W) = src_size, at
    (Ht, Wt) = dst_size after area resampling, on the host in integer arithmetic:
        cmin' = floor(cmin Wt / W),   cmax' = ceil((cmax + 1) Wt / W) - 1,   the rows with H, Ht in the same way
    — exactly the box of the mask "a target pixel is foreground when ANY source pixel under its window is".  -> float32, a
    tensor for a tensor and an array for an array, like _items.mask_bbox.
    A deliberate difference from upstream pixelNeRF, which multiplies the boxes by the ROW scale as floats (fractional corners,
    and the wrong columns when the two scales differ)."""
    H, W, Ht, Wt = _sizes(src_size, dst_size)
    is_tensor = torch.is_tensor(bbox)
    b = np.asarray(bbox.cpu() if is_tensor else bbox)
    if b.shape[-1:] != (4,):
        raise ValueError(f"bbox must be (..., 4), got {b.shape}")
    q = b.astype(np.int64)
    if not np.array_equal(q, b):
        raise ValueError("bbox must hold whole numbers")
    n_in = np.array([W, H, W, H], dtype=np.int64)
    n_out = np.array([Wt, Ht, Wt, Ht], dtype=np.int64)
    lo = (q * n_out) // n_in
    hi = -((-(q + 1) * n_out) // n_in) - 1
    res = np.where(np.array([True, True, False, False]), lo, hi).astype(np.float32)
    return torch.from_numpy(res) if is_tensor else res


def resize_intrinsics(focal, c, src_size, dst_size):
    """The intrinsics of images (H, W) = src_size at (Ht, Wt) = dst_size: sx = Wt / W, sy = Ht / H.  focal — a float, or a
    tensor that is one focal length per entry, or (..., 2) = (fx, fy) — keeps its form and is multiplied by sx when
    sx == sy; otherwise it becomes (..., 2) = (fx sx, fy sy) float32.  c (..., 2) becomes (cx sx, cy sy); None stays None (the
    default centre scales to the centre).  The products are made in fp64 and rounded once.  -> (focal, c).
    A tensor whose LAST dimension is 2 is read as (fx, fy) pairs.
    Deliberate differences from upstream pixelNeRF: it uses the row scale alone for everything; like upstream, the half-pixel
    shift of c under pixel-centre-at-integer coordinates is ignored."""
    H, W, Ht, Wt = _sizes(src_size, dst_size)
    sx, sy = Wt / W, Ht / H
    if c is not None:
        ct = torch.as_tensor(c)
        if ct.shape[-1:] != (2,):
            raise ValueError(f"c must be (..., 2), got {tuple(ct.shape)}")
        c = (ct.double() * torch.tensor([sx, sy], dtype=torch.float64, device=ct.device)).to(ct.dtype if ct.is_floating_point() else torch.float32)
    if not torch.is_tensor(focal):
        if Wt * H == Ht * W:
            return float(focal) * sx, c
        focal = torch.tensor(float(focal), dtype=torch.float32)
    dtype = focal.dtype if focal.is_floating_point() else torch.float32
    if Wt * H == Ht * W:
        return (focal.double() * sx).to(dtype), c
    pair = focal if focal.shape[-1:] == (2,) else torch.stack((focal, focal), dim=-1)
    return (pair.double() * torch.tensor([sx, sy], dtype=torch.float64, device=pair.device)).to(dtype), c
