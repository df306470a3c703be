"""
The reference's two demo drivers on this package's renderer: eval/gen_video.py (encode the source views of one object, render
a 360 degree or DTU-style camera path) and eval/eval_real.py (the same from a photograph).

* orbit_poses / quat_path     the camera paths (gen_video.py:124-172, eval_real.py:100-107), on the host
* render_video                one fused render launch per pose into ONE packed (F*H*W, 4) record, then ONE pnr_video_frames
                              launch: (F, H, W, 3) bytes on the device, and the count of components outside numpy's cast range
* gen_video / eval_real       the drivers' bodies: encode, render_video, 3 bytes per pixel to the host once, PNG frames

Pinned: the pose helpers, bit for bit against the reference's own (tests/golden/video_paths.npz); the byte quantisation,
against numpy's cast wherever that is defined; image_to_tensor, against torch's division.  PARITY UNPINNED: torchvision's
ToTensor / T.Resize against PIL's resize used here (torchvision is not importable where this package is developed), and
imageio's mp4 and GIF encoders (imageio is not importable either: no mp4 is written, the GIF comes from PIL).
"""
import os
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import util
from .parallel import frame_seed

VideoResult = namedtuple("VideoResult", "frames n_out_of_range frame_paths view_path video_path")
VideoResult.__doc__ = """What gen_video / eval_real return: frames (F, H, W, 3) uint8 numpy, n_out_of_range int, the PNG paths
in frame order, the view strip's path (None for eval_real) and the GIF's path (None unless write="gif")."""


# ----------------------------------------------------------------------------------------------------------- camera paths
def orbit_poses(num_views, elevation, radius, from_blender=False):
    """(num_views, 4, 4) float32 c2w on the host: util.pose_spherical at np.linspace(-180, 180, num_views + 1)[:-1], the
    360 degree loop of eval/gen_video.py:166-172, with the reference's bits.  from_blender=True left-multiplies every pose
    by util.coord_from_blender(), as eval/eval_real.py:100-107 does."""
    poses = [util.pose_spherical(angle, elevation, radius, reference_order=True)
             for angle in np.linspace(-180, 180, int(num_views) + 1)[:-1]]
    if from_blender:
        m = util.coord_from_blender()
        poses = [m @ p for p in poses]
    return torch.stack(poses, 0)


def dtu_frame_count(num_views):
    """Frames of the reference's DTU trajectory for --num_views (gen_video.py:134-136): n_inter * int(t_in[-1]) with
    n_inter = num_views // 5 and the last knot at 6 — six per interval, not five."""
    return (int(num_views) // 5) * 6


def quat_path(t_in, quats, scales, n_out):
    """The DTU camera trajectory of eval/gen_video.py:124-156 with the key table as an argument: t_in (K,) knots, quats
    (K, 4) key rotations (r, i, j, k) and scales (K,) camera distances, first key = last key -> (n_out, 4, 4) float32 c2w on
    the host.  Periodic cubic splines over the scales and over the quaternions, evaluated at np.linspace(t_in[0], t_in[-1],
    n_out) in fp32, renormalised, util.quat_to_rot, translation R[:, :, 2] * scale.  The reference's own table is data:
    np.load("tests/golden/video_dtu_keys.npz") -> t_in, quats, scales; n_out = dtu_frame_count(num_views)."""
    try:
        from scipy.interpolate import CubicSpline
    except ImportError as e:
        raise ImportError("quat_path needs scipy (scipy.interpolate.CubicSpline), as the reference's gen_video.py does") from e
    t_in = np.asarray(t_in).astype(np.float32)
    quats = np.asarray(quats, dtype=np.float32)
    scales = np.asarray(scales).astype(np.float32)
    if t_in.ndim != 1 or quats.shape != (len(t_in), 4) or scales.shape != t_in.shape:
        raise ValueError(f"quat_path takes t_in (K,), quats (K, 4), scales (K,), got {t_in.shape} {quats.shape} {scales.shape}")
    t_out = np.linspace(t_in[0], t_in[-1], int(n_out)).astype(np.float32)
    s_new = CubicSpline(t_in, scales, bc_type="periodic")(t_out)
    q_new = CubicSpline(t_in, quats, bc_type="periodic")(t_out)
    q_new = q_new / np.linalg.norm(q_new, 2, 1)[:, None]
    R = util.quat_to_rot(torch.from_numpy(q_new).float())
    poses = torch.eye(4, dtype=torch.float32).repeat(len(t_out), 1, 1)
    poses[:, :3, :3] = R
    poses[:, :3, 3] = R[:, :, 2] * torch.from_numpy(s_new).float()[:, None]      # an fp32 product, as tensor * scalar is
    return poses


# ----------------------------------------------------------------------------------------------------------- the render
def render_video(net, renderer, poses, W, H, focal, z_near, z_far, c=None, seed=None, occupancy=None):
    """poses (F, 4, 4) c2w on the host, rendered from the views `net` has encoded -> (frames_u8 (F, H, W, 3) uint8,
    n_out_of_range 0-dim int64), both on the device.  One fused render launch per pose (pnr_render_camera: the rays are made
    inside the launch), each writing its pixels into its slice of ONE packed (F*H*W, 4) [rgb, depth] record — the mechanism
    the sharded renderer gathers frames with — then ONE util.video_frames launch over the whole stack.  Frame f is rendered
    under parallel.frame_seed(seed, f) (seed=None: drawn from torch's generator), so it is the frame render_image gives
    under that seed.  Nothing here reads the device: the call passes under torch.cuda.set_sync_debug_mode("error").  A model
    that render_image routes through the generic path (not a PixelNeRFNet, several objects) is rendered by render_image
    frame by frame, which may wait.
    occupancy (None: everything above, unchanged): an OccupancyGrid, or a dict of OccupancyGrid.from_net's keywords plus an
    optional "pad", built here from the encoded network — the frames are then NeRFRenderer.render_frames_bounded's (empty
    space culled, ONE host read of the per-frame counts; see there for the noise) under the same per-frame seeds.  A
    ValueError under a process group of several ranks."""
    from .model.models import PixelNeRFNet
    if occupancy is not None:
        from .render import occupancy as occ
        occ.refuse_sharded("render_video")
    poses = torch.as_tensor(poses, dtype=torch.float32)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] < 1:
        raise ValueError(f"poses must be (F, 4, 4) with F >= 1, got {tuple(poses.shape)}")
    if poses.is_cuda:
        poses = poses.cpu()
    F, W, H = int(poses.shape[0]), int(W), int(H)
    HW = H * W
    seed = util.seed_from_torch() if seed is None else int(seed)
    dev = net.poses.device
    with torch.no_grad():
        if occupancy is not None:
            grid, pad = occ.resolve(occupancy, net)
            rgb = renderer.render_frames_bounded(net, poses, W, H, focal, z_near, z_far, grid, c=c, pad=pad, seed=seed)[0]
            rgb = rgb.reshape(F * HW, 3)                              # still a view into the (F H W, 4) record
        elif isinstance(net, PixelNeRFNet) and net.num_objs == 1 and not net.wants_grad(net.poses):
            renderer._apply_sched()
            fx, fy, cx, cy = util.intrinsics(focal, c, W, H)          # read once: focal and c may live on the device
            level = ("fine",) if renderer.using_fine else ("coarse",)
            record = torch.empty(F * HW, 4, device=dev, dtype=torch.float32)
            for i in range(F):
                cam = util.camera(poses[i], W, H, (fx, fy), z_near, z_far, c=(cx, cy))
                with renderer.keyed(frame_seed(seed, i)):
                    renderer._forward_fused(net, None, False, camera=cam,
                                            packed=(record[i * HW:(i + 1) * HW].view(1, HW, 4), level))
            rgb = record[:, :3]
        else:
            frames = []
            for i in range(F):
                with renderer.keyed(frame_seed(seed, i)):
                    frames.append(renderer.render_image(net, poses[i], W, H, focal, z_near, z_far, c=c)[0])
            rgb = torch.stack(frames, 0).contiguous()
        return util.video_frames(rgb, F, H, W)


# ----------------------------------------------------------------------------------------------------------- the drivers
def video_name(source, subset=0, split="train"):
    """The reference's file stem (gen_video.py:225-230): "{subset:04}", "t" / "v" in front for the test / val split, then
    "_v" and the source views as "{:03}" joined by "_" — e.g. "t0003_v000_002"."""
    name = "{:04}".format(int(subset))
    if split == "test":
        name = "t" + name
    elif split == "val":
        name = "v" + name
    return name + "_v" + "_".join("{:03}".format(int(x)) for x in source)


def _to_host(frames_u8, count):
    """The ONE copy of a video to the host, 3 bytes per pixel, through pinned memory; waits for it."""
    frames_h = torch.empty(frames_u8.shape, dtype=torch.uint8, pin_memory=True)
    count_h = torch.empty((), dtype=torch.int64, pin_memory=True)
    frames_h.copy_(frames_u8, non_blocking=True)
    count_h.copy_(count, non_blocking=True)
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(frames_u8.device))
    done.synchronize()
    return frames_h.numpy().copy(), int(count_h)


def write_gif(path, frames, fps=30):
    """Animated GIF of (F, H, W, 3) uint8 frames through PIL.  PARITY UNPINNED against imageio.mimwrite, the reference's
    writer (palette and timing are the encoder's); the PNG frames are the pinned output."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError('write="gif" needs PIL; the PNG frames need nothing') from e
    imgs = [Image.fromarray(np.ascontiguousarray(f)) for f in frames]
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=max(int(round(1000.0 / fps)), 1), loop=0)
    return path


def _write_frames(frames_dir, frames):
    from .evalio import write_png
    os.makedirs(frames_dir, exist_ok=True)
    paths = [os.path.join(frames_dir, "{:04}.png".format(i)) for i in range(len(frames))]
    for p, fr in zip(paths, frames):
        write_png(p, fr)
    return paths


def gen_video(net, renderer, data, out_dir, source, num_views=40, elevation=-10.0, radius=0.0, scale=1.0, *, z_near, z_far,
              path=None, write="png", ensure_resolution=True, subset=0, split="train", fps=30, seed=None, occupancy=None):
    """The body of eval/gen_video.py for one object.  data: a dataset item — "images" (NV, 3, H, W) in [-1, 1], "poses"
    (NV, 4, 4) c2w, "focal" (float | tensor), optional "c"; source: the list of source views ([-1]: one random view).
    The path is orbit_poses(num_views, elevation, radius) with radius 0 = (z_near + z_far) / 2 (:159-172), or `path`, any
    (F, 4, 4) poses such as quat_path's.  focal and c are multiplied by `scale` and the frames are (H scale, W scale), with
    the reference's inexact-scale warning (:92-101).  ensure_resolution=True keeps :192-195: a renderer with n_coarse < 64
    renders at 64 coarse and 128 fine samples; its own counts are restored afterwards.  The source views are encoded,
    render_video leaves the bytes on the device, ONE copy of 3 bytes per pixel brings them to the host, and
    <out_dir>/video<name>_frames/0000.png .. and <out_dir>/video<name>_view.png (the source views side by side,
    util.view_strip; the reference writes a .jpg through imageio) are written with evalio.write_png, <name> =
    video_name(source, subset, split).  write="gif" adds <out_dir>/video<name>.gif through PIL (parity unpinned against
    imageio; no mp4 is written).  occupancy: as render_video takes it; a dict is turned into a grid after the source views
    are encoded.  -> VideoResult."""
    from .evalio import _render_size, write_png
    if occupancy is not None:
        from .render import occupancy as occ
        occ.refuse_sharded("gen_video")
    if write not in ("png", "gif"):
        raise ValueError(f"write must be 'png' or 'gif', got {write!r}")
    dev = net.poses.device
    images = torch.as_tensor(data["images"]).float()
    NV = images.shape[0]
    H, W = _render_size(images, float(scale))
    focal = data["focal"]
    focal = torch.tensor(focal, dtype=torch.float32) if isinstance(focal, float) else torch.as_tensor(focal).float()
    c = data.get("c")
    c = None if c is None else torch.as_tensor(c).float()
    src = [int(v) for v in (source.tolist() if hasattr(source, "tolist") else source)]
    if src == [-1]:
        src = torch.randint(0, NV, (1,)).tolist()
    if not src or any(v < 0 or v >= NV for v in src):
        raise ValueError(f"source views {src} outside [0, {NV})")
    if path is None:
        if radius == 0.0:
            radius = (float(z_near) + float(z_far)) * 0.5
        path = orbit_poses(num_views, elevation, radius)
    name = "video" + video_name(src, subset, split)
    keep_counts = (renderer.n_coarse, renderer.n_fine)
    was_training = net.training
    net.eval()
    try:
        if ensure_resolution and renderer.n_coarse < 64:
            renderer.n_coarse, renderer.n_fine = 64, 128
        with torch.no_grad():
            src_images = util.upload(images[src].contiguous(), dev)
            net.encode(src_images.unsqueeze(0), torch.as_tensor(data["poses"]).float()[src].to(dev).unsqueeze(0), focal[None].to(dev),
                       c=None if c is None else c.to(dev).unsqueeze(0))
            frames_u8, count = render_video(net, renderer, path, W, H, focal * scale, z_near, z_far,
                                            c=None if c is None else c * scale, seed=seed, occupancy=occupancy)
            strip = util.view_strip(src_images)
            strip_h = torch.empty(strip.shape, dtype=torch.uint8, pin_memory=True)
            strip_h.copy_(strip, non_blocking=True)               # in front of the frames on the stream: their wait covers it
            frames, n_out = _to_host(frames_u8, count)
    finally:
        renderer.n_coarse, renderer.n_fine = keep_counts
        net.train(was_training)
    os.makedirs(out_dir, exist_ok=True)
    frame_paths = _write_frames(os.path.join(out_dir, name + "_frames"), frames)
    view_path = os.path.join(out_dir, name + "_view.png")
    write_png(view_path, strip_h.numpy())
    video_path = write_gif(os.path.join(out_dir, name + ".gif"), frames, fps) if write == "gif" else None
    return VideoResult(frames, n_out, frame_paths, view_path, video_path)


def _load_image(image, size):
    """-> (H, W, 3) uint8 numpy with the smaller edge `size`: PIL open + convert("RGB") for a path, PIL's bilinear resize where
    the size differs (the reference resizes with torchvision's T.Resize: parity unpinned)."""
    if isinstance(image, (str, os.PathLike)):
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError("eval_real needs PIL to open an image file; pass an (H, W, 3) uint8 array instead") from e
        arr = np.asarray(Image.open(image).convert("RGB"))
    else:
        arr = image.cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if arr.ndim != 3 or arr.shape[2] != 3 or arr.dtype != np.uint8:
        raise ValueError(f"the image must be uint8 (H, W, 3), got {arr.dtype} {arr.shape}")
    h, w = arr.shape[:2]
    if size and min(h, w) != int(size):
        try:
            from PIL import Image
        except ImportError as e:
            raise ImportError(f"eval_real needs PIL to resize a {h} x {w} image to {size}; pass one of that size instead") from e
        size = int(size)
        nh, nw = (size, int(size * w / h)) if h <= w else (int(size * h / w), size)
        arr = np.asarray(Image.fromarray(arr).resize((nw, nh), Image.BILINEAR))
    return np.array(arr, order="C")             # a writable copy of its own: PIL's buffers are read-only


def eval_real(net, renderer, image, out_dir, size=128, out_size=128, *, focal, radius, elevation, num_views=24, z_near, z_far,
              balanced=False, name=None, write="png", fps=15, seed=None):
    """eval/eval_real.py:85-171 for one photograph.  image: a path (PIL opens it) or an (H, W, 3) uint8 array; its smaller edge
    is brought to `size` on the host, util.image_to_tensor makes the network's input on the device (balanced=False: [0, 1],
    what the reference fork feeds; True: upstream's [-1, 1]), the dummy camera is eye(4) with [2, 3] = radius (:127-128), the
    path orbit_poses(num_views, elevation, radius, from_blender=True) (:100-107), out_size = side or (W, H).  Writes
    <out_dir>/<name>_frames/0000.png .. (name: the file's stem, "image" for an array) and, with write="gif",
    <out_dir>/<name>_vid.gif through PIL (parity unpinned against imageio; no mp4).  -> VideoResult (view_path None)."""
    if write not in ("png", "gif"):
        raise ValueError(f"write must be 'png' or 'gif', got {write!r}")
    dev = net.poses.device
    if name is None:
        name = os.path.basename(os.path.splitext(os.fspath(image))[0]) if isinstance(image, (str, os.PathLike)) else "image"
    W, H = (int(out_size), int(out_size)) if np.isscalar(out_size) else (int(out_size[0]), int(out_size[1]))
    arr = _load_image(image, size)
    focal = torch.as_tensor(focal, dtype=torch.float32)
    cam_pose = torch.eye(4)
    cam_pose[2, 3] = float(radius)
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            x = util.image_to_tensor(arr, balanced=balanced, device=dev)
            net.encode(x[None, None], cam_pose.to(dev)[None, None], focal.reshape(-1)[:1].to(dev))
            frames_u8, count = render_video(net, renderer, orbit_poses(num_views, elevation, radius, from_blender=True), W, H,
                                            focal, z_near, z_far, seed=seed)
            frames, n_out = _to_host(frames_u8, count)
    finally:
        net.train(was_training)
    os.makedirs(out_dir, exist_ok=True)
    frame_paths = _write_frames(os.path.join(out_dir, name + "_frames"), frames)
    video_path = write_gif(os.path.join(out_dir, name + "_vid.gif"), frames, fps) if write == "gif" else None
    return VideoResult(frames, n_out, frame_paths, None, video_path)
