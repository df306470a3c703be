"""
On-disk / wire formats around the render path, so an evaluation driver built on this package reads
and writes what the reference's eval scripts do.  Parsing and arithmetic on the host; evaluate(metrics="device") leaves the
per-frame work (clamp, quantisation, PSNR / SSIM sums, normalised depth) to the HIP back end, util.eval_frame.

* finish.txt resume log      reference eval/eval.py:113-133,360-362   one line per object: "<name> <psnr> <ssim> <cnt>"
* source-view look-up table   reference eval/eval.py:156-165           viewlist/src_*.txt: "<cat> <obj> <view> [<view> ...]"
* eval view list              reference eval/eval.py:170-176           first line: target view indices
* PNG quantisation            reference eval/eval.py:301               (rgb * 255).astype(uint8) after clamp to [0,1]
* PSNR / SSIM                 reference eval/eval.py:324-332           skimage.measure.compare_psnr / compare_ssim
                              (data_range=1, multichannel): restated from the published definitions — skimage is not
                              installed here and the reference's own numbers need its dataset, so SSIM is "parity unpinned".
* checkpoints                 three mutually incompatible schemas in the reference tree
* evaluate()                  reference eval/eval.py:186-362           the per-object loop that composes the above with
                              encode -> render -> clamp -> metrics -> finish.txt (resume), on this package's renderer
* evaluate_approx()           reference eval/eval_approx.py:89-153     the development loop: one random target view per
                              object, a loader batch of objects per render call, metrics on the UNclamped frames
"""
import math
import os
import warnings
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

from . import util
from .parallel import frame_seed


class FinishLog:
    """finish.txt: append-only per-object results with resume (objects already listed are skipped by the driver)."""

    def __init__(self, path, state=None):
        """state = (finished, total_psnr, total_ssim, cnt): a follower of a multi-rank evaluation — it starts from the
        owner's view of the file (broadcast once) and never opens it: the file has ONE writer."""
        self.path = path
        self.finished, self.total_psnr, self.total_ssim, self.cnt = set(), 0.0, 0.0, 0
        self._f = None
        if state is not None:
            self.finished, self.total_psnr, self.total_ssim, self.cnt = set(state[0]), float(state[1]), float(state[2]), int(state[3])
            return
        if os.path.exists(path):
            with open(path) as f:
                rows = [x.strip().split() for x in f.readlines()]
            rows = [x for x in rows if len(x) == 4]
            self.finished = {x[0] for x in rows}
            self.total_psnr = sum(float(x[1]) for x in rows)
            self.total_ssim = sum(float(x[2]) for x in rows)
            self.cnt = sum(int(x[3]) for x in rows)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self._f = open(path, "a", buffering=1)

    def state(self):
        return (sorted(self.finished), self.total_psnr, self.total_ssim, self.cnt)

    def append(self, obj_name, psnr, ssim, cnt=1):
        if self._f is not None:
            self._f.write("{} {} {} {}\n".format(obj_name, psnr, ssim, cnt))
        self.finished.add(obj_name)
        self.total_psnr += psnr
        self.total_ssim += ssim
        self.cnt += cnt

    def mean(self):
        return (self.total_psnr / self.cnt, self.total_ssim / self.cnt) if self.cnt else (0.0, 0.0)

    def close(self):
        if self._f is not None:
            self._f.close()


def read_source_view_lut(path):
    """{"<cat>/<obj>": LongTensor(source view indices)}"""
    lut = {}
    with open(path) as f:
        for line in f:
            x = line.strip().split()
            if len(x) >= 3:
                lut[x[0] + "/" + x[1]] = torch.tensor(list(map(int, x[2:])), dtype=torch.long)
    return lut


def read_eval_view_list(path):
    with open(path) as f:
        return torch.tensor(list(map(int, f.readline().split())), dtype=torch.long)


def quantize_uint8(rgb):
    """float image in [0,1] (clamped) -> uint8 the way the reference writes PNGs (truncation, not rounding)."""
    a = np.clip(np.asarray(rgb, dtype=np.float32), 0.0, 1.0)
    return (a * 255).astype(np.uint8)


def psnr(img, gt, data_range=1.0):
    err = np.mean((np.asarray(img, np.float64) - np.asarray(gt, np.float64)) ** 2)
    return 10.0 * np.log10((data_range ** 2) / err)


def _psnr_of_mse(mse):
    """PSNR (data_range 1) of a mean squared error read back from the device: inf for identical images, NaN for a NaN."""
    return float("inf") if mse == 0.0 else 10.0 * math.log10(1.0 / mse) if mse > 0.0 else float("nan")


def ssim(img, gt, data_range=1.0, win_size=7, K1=0.01, K2=0.03):
    """Mean structural similarity, uniform 7x7 window, sample covariance, per channel then averaged, borders cropped
    (Wang et al. 2004 as implemented by skimage.measure.compare_ssim with multichannel=True)."""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(img, np.float64), np.asarray(gt, np.float64)
    if x.ndim == 3:
        return float(np.mean([ssim(x[..., c], y[..., c], data_range, win_size, K1, K2) for c in range(x.shape[-1])]))
    NP = win_size ** 2
    cov_norm = NP / (NP - 1.0)
    ux, uy = uniform_filter(x, win_size), uniform_filter(y, win_size)
    uxx, uyy, uxy = uniform_filter(x * x, win_size), uniform_filter(y * y, win_size), uniform_filter(x * y, win_size)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (win_size - 1) // 2
    return float(S[pad:-pad, pad:-pad].mean())


def load_checkpoint(net, path, device=None, strict=False):
    """Load any of the reference tree's three checkpoint schemas into a PixelNeRFNet, executing nothing
    from the file (weights_only):  a bare state-dict (models.py.backup2:293-305, upstream pixelNeRF);
    {"net_state_dict": ...} (train/trainlib/trainer.py:593-600);  {"model_state_dict"| "model": ...} (models.py:331-336).
    Returns the (missing, unexpected) key lists of load_state_dict."""
    ck = torch.load(path, map_location=device or "cpu", weights_only=True)
    for key in ("net_state_dict", "model_state_dict", "model", "state_dict"):
        if isinstance(ck, dict) and key in ck and isinstance(ck[key], dict):
            ck = ck[key]
            break
    ck = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ck.items()}   # DataParallel prefix
    res = net.load_state_dict(ck, strict=strict)
    return list(res.missing_keys), list(res.unexpected_keys)


def write_png(path, rgb_u8):
    """8-bit RGB PNG from an (H, W, 3) uint8 array with the standard library only (the reference writes through imageio,
    eval/eval.py:301; the pixel values are what matters for calc_metrics.py, not the encoder)."""
    import struct
    import zlib
    a = np.ascontiguousarray(rgb_u8, dtype=np.uint8)
    h, w, c = a.shape
    assert c == 3
    raw = b"".join(b"\x00" + a[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


# ------------------------------------------------------------------------------------------------- the parts of evaluate()
def _open_log(output_dir, sharded, rank):
    """The FinishLog of an evaluation; without an output directory one that has no file and holds the running sums alone
    (path None).  Under a process group every rank runs the loop
    (each call's rays are cut over the ranks and every rank gets the whole frame back), but the output directory has ONE
    writer: rank 0 owns finish.txt and the PNGs; the other ranks start from rank 0's view of the file — broadcast once, so
    all ranks skip the same objects whatever the file system shows them — and keep their running means in memory."""
    if not (output_dir and str(output_dir).strip()):
        return FinishLog(None, state=((), 0.0, 0.0, 0))
    path = os.path.join(output_dir, "finish.txt")
    log = FinishLog(path) if rank == 0 else None
    if sharded:
        box = [log.state() if rank == 0 else None]
        dist.broadcast_object_list(box, src=0)
        if rank != 0:
            log = FinishLog(path, state=box[0])
    return log


def _base_seed(seed, sharded):
    """One base seed per call: `seed`, else drawn from torch's generator on every rank; rank 0's draw is the one kept."""
    if seed is not None:
        return int(seed)
    box = [util.seed_from_torch()]
    if sharded:
        dist.broadcast_object_list(box, src=0)
    return int(box[0])


def target_views(NV, src, eval_view_list, include_src):
    """-> (src_mask (NV,) bool, tgt_mask (NV,) bool, novel = the target view indices, ascending): the targets are
    eval_view_list (None = every view) minus the source views `src` unless include_src (eval.py:170-178, :246-248)."""
    src_mask = torch.zeros(NV, dtype=torch.bool)
    src_mask[src] = True
    tgt_mask = torch.ones(NV, dtype=torch.bool)
    if eval_view_list is not None:
        tgt_mask = torch.zeros(NV, dtype=torch.bool)
        tgt_mask[torch.as_tensor(eval_view_list, dtype=torch.long)] = True
    if not include_src:
        tgt_mask = tgt_mask & ~src_mask
    return src_mask, tgt_mask, tgt_mask.nonzero(as_tuple=False).reshape(-1)


def _render_size(images, scale):
    H, W = images.shape[-2:]
    if scale == 1.0:
        return H, W
    Ht, Wt = int(H * scale), int(W * scale)
    if abs(Ht / scale - H) > 1e-10 or abs(Wt / scale - W) > 1e-10:
        warnings.warn(f"Inexact scaling, please check {scale} times ({H}, {W}) is integral")
    return Ht, Wt


def _encode_object(net, data, src_mask, dev, sharded):
    """net.encode on the object's source views (eval.py:271-276) -> its (poses, focal, c) as float tensors on the host."""
    focal = data["focal"]
    focal = torch.tensor(focal, dtype=torch.float32) if isinstance(focal, float) else torch.as_tensor(focal).float()
    c = data.get("c")
    c = None if c is None else torch.as_tensor(c).float()
    poses = torch.as_tensor(data["poses"]).float()
    net.encode(data["images"][src_mask].to(dev).unsqueeze(0), poses[src_mask].to(dev).unsqueeze(0), focal[None].to(dev),
               c=None if c is None else c.to(dev).unsqueeze(0))
    if sharded:
        # every rank ran the trunk on the same images, but a convolution library may pick different algorithms in
        # different processes (last-bit differences): rank 0's maps are THE maps, so that the gathered frame is one
        # consistent render (64 KB ... 6 MB per object, once — SURVEY 8e)
        maps = [m.detach().clone() for m in net.encoder.level_maps()]
        for m in maps:
            if dist.get_backend() == "nccl":
                dist.broadcast(m, src=0)
            else:
                h = m.cpu()
                dist.broadcast(h, src=0)
                m.copy_(h)
        net.encoder.set_latents(maps)
    return poses, focal, c


def _sharded_renderer(net, renderer):
    # built directly: bind_parallel() only shards when the caller lists several gpu ids (eval.py:151 passes args.gpu_id),
    # and a rank of a one-process-per-GPU job has exactly one
    from .render.nerf import _ShardedRenderWrapper
    return _ShardedRenderWrapper(net, renderer, simple_output=True).eval()


def _render_view(net, renderer, render_par, view_seed, pose, W, H, focal, c, z_near, z_far, ray_batch_size):
    """-> (rgb (H, W, 3), depth (H, W)) of one view on the device: ONE renderer.render_image call (looked up here, per call:
    a caller may have wrapped it on the instance), or chunks of ray_batch_size through the sharded wrapper render_par."""
    if render_par is None:
        with renderer.keyed(view_seed):
            return renderer.render_image(net, pose, W, H, focal, z_near, z_far, c=c)
    rays = util.gen_rays_device(pose, W, H, focal, z_near, z_far, c=c, device=net.poses.device)
    parts, at = [], 0
    for r in torch.split(rays, ray_batch_size, dim=0):
        parts.append(render_par(r[None], ray_index_base=at, seed=view_seed))
        at += r.shape[0]
    return (torch.cat([p[0][0] for p in parts], 0).reshape(H, W, 3),
            torch.cat([p[1][0] for p in parts], 0).reshape(H, W))


class _BackEnd:
    """What becomes of an object's rendered frames: begin(obj_out, images, tgt_mask, views, H, W) per object — obj_out the
    object's directory, None on a rank that writes nothing —, frame(i, vi, rgb, depth) for the i-th target view vi as the
    render left it on the device, finish() -> the object's (psnr, ssim), after it has waited and written the object's files.
    o: what evaluate() was asked for (z_near, z_far, compare_gt, write_images, write_compare, write_depth, depth_png, lut)."""

    def check_size(self, H, W, images):
        pass

    def _write(self, vi, u8=None, depth_norm=None, depth_png=None, compare=None):
        """The files of view vi from host arrays, None = not written; the object's directory is made with its first file."""
        files = ((".png", u8), ("_depth.npy", depth_norm), ("_depth_norm.png", depth_png), ("_compare.png", compare))
        for suffix, a in files:
            if a is not None:
                os.makedirs(self.obj_out, exist_ok=True)
                (np.save if suffix.endswith(".npy") else write_png)(os.path.join(self.obj_out, "{:06}{}".format(vi, suffix)), a)


class _HostBackEnd(_BackEnd):
    """metrics="host", the reference's recipe: every frame goes to the host as fp32 — to_host(rgb, depth) -> (rgb_host,
    depth_host, event), the renderer's frame_to_host_async — and numpy / scipy do the rest."""

    def __init__(self, o, to_host):
        self.o, self.to_host = o, to_host

    def begin(self, obj_out, images, tgt_mask, views, H, W):
        self.obj_out, self.images, self.tgt_mask, self.views, self.shape = obj_out, images, tgt_mask, views, (H, W)
        self.copies = []                                            # (rgb_host, depth_host, event) per view

    def frame(self, i, vi, rgb, depth):
        self.copies.append(self.to_host(rgb, depth))                # D2H overlaps the next view's render:
        if i > 0:
            self.copies[i - 1][2].synchronize()                     # the host waits for the view before, not for this one

    def finish(self):
        o, views, n_gen, writes = self.o, self.views, len(self.copies), self.obj_out is not None
        all_rgb = np.zeros((0, *self.shape, 3), np.float32)
        if n_gen:
            self.copies[-1][2].synchronize()
            all_rgb = torch.clamp(torch.stack([c[0] for c in self.copies]), 0.0, 1.0).numpy()
        if writes and o.write_images:
            os.makedirs(self.obj_out, exist_ok=True)                # as the reference: also for an object without target views
            for i in range(n_gen):
                self._write(views[i], u8=quantize_uint8(all_rgb[i]))
        if writes and o.write_depth and n_gen:
            all_depth = ((torch.stack([c[1] for c in self.copies]) - o.z_near) / (o.z_far - o.z_near)).numpy()      # eval.py:288-289
            for i in range(n_gen):
                self._write(views[i], depth_norm=all_depth[i], depth_png=util.cmap(all_depth[i], o.lut) if o.depth_png else None)
        if not (o.compare_gt and n_gen):
            return 0.0, 0.0
        curr_psnr = curr_ssim = 0.0
        gt = (self.images * 0.5 + 0.5)[self.tgt_mask].permute(0, 2, 3, 1).contiguous().numpy()
        for i in range(n_gen):
            curr_ssim += ssim(all_rgb[i], gt[i], data_range=1)
            curr_psnr += psnr(all_rgb[i], gt[i], data_range=1)
            if writes and o.write_compare:
                self._write(views[i], compare=quantize_uint8(np.hstack((all_rgb[i], gt[i]))))
        return curr_psnr / n_gen, curr_ssim / n_gen


class _DeviceBackEnd(_BackEnd):
    """metrics="device": util.eval_frame on each frame where the render left it; the object's ground truth is uploaded once,
    the (mse, ssim) pairs collect in one device buffer, what will be written travels to pinned host buffers asynchronously
    and finish() holds the one wait of the object.  The pinned buffers are kept for the next object of the same shape."""

    def __init__(self, o, dev):
        self.o, self.dev, self.pin = o, dev, {}

    def check_size(self, H, W, images):
        if self.o.compare_gt and (H, W) != tuple(images.shape[-2:]):
            raise ValueError(f"metrics='device' compares a {H} x {W} render with {tuple(images.shape[-2:])} ground truth: "
                             "use scale=1 or no_compare_gt")

    def _pinned(self, name, wanted, shape, dtype):
        if not wanted:
            return None
        t = self.pin.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self.pin[name] = torch.empty(shape, dtype=dtype, pin_memory=True)
        return t

    def begin(self, obj_out, images, tgt_mask, views, H, W):
        o, n_gen, writes = self.o, len(views), obj_out is not None
        self.obj_out, self.views = obj_out, views
        self.compare = compare = o.compare_gt and n_gen > 0
        self.gt_dev = util.upload(images[tgt_mask].float().contiguous(), self.dev) if compare else None
        self.pairs = torch.empty(n_gen, 2, dtype=torch.float64, device=self.dev) if compare else None
        want_dn = writes and o.write_depth
        self.u8_h = self._pinned("u8", writes and o.write_images, (n_gen, H, W, 3), torch.uint8)
        self.cmp_h = self._pinned("cmp", writes and o.write_compare and compare, (n_gen, H, 2 * W, 3), torch.uint8)
        self.dn_h = self._pinned("dn", want_dn, (n_gen, H, W), torch.float32)
        self.dpng_h = self._pinned("dpng", want_dn and o.depth_png, (n_gen, H, W, 3), torch.uint8)

    def frame(self, i, vi, rgb, depth):
        o, compare, want_dn = self.o, self.compare, self.dn_h is not None
        u8, cmp, dn, _ = util.eval_frame(rgb, depth if want_dn else None, self.gt_dev[i] if compare else None,
                                         z_near=o.z_near, z_far=o.z_far, want_u8=self.u8_h is not None,
                                         want_compare=self.cmp_h is not None, want_depth=want_dn, want_metrics=compare,
                                         metrics_out=self.pairs[i] if compare else None)
        dpng = util.cmap_device(dn, o.lut)[0] if self.dpng_h is not None else None
        for dst, src_t in ((self.u8_h, u8), (self.cmp_h, cmp), (self.dn_h, dn), (self.dpng_h, dpng)):
            if dst is not None:
                dst[i].copy_(src_t, non_blocking=True)

    def finish(self):
        views, compare, n_gen = self.views, self.compare, len(self.views)
        if compare:
            pairs_h = self._pinned("pairs", True, (n_gen, 2), torch.float64)
            pairs_h.copy_(self.pairs, non_blocking=True)
        if n_gen:
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(self.dev))
            done.synchronize()                                  # the one wait of this object
        curr_psnr = curr_ssim = 0.0
        for i, vi in enumerate(views):
            self._write(vi, *(None if h is None else h[i].numpy() for h in (self.u8_h, self.dn_h, self.dpng_h, self.cmp_h)))
            if compare:
                mse, s = (float(x) for x in pairs_h[i])
                curr_ssim += s
                curr_psnr += _psnr_of_mse(mse)
        return (curr_psnr / n_gen, curr_ssim / n_gen) if compare else (0.0, 0.0)


def evaluate(net, renderer, dataset, output_dir="", *, source="", viewlist=None, eval_view_list=None,
             include_src=False, scale=1.0, multicat=False, gpu_id=None, ray_batch_size=50000, no_compare_gt=False,
             write_compare=False, write_images=True, max_objects=50, z_near=None, z_far=None,
             verbose=True, seed=None, metrics="host", write_depth=False, depth_png=False, lut=None):
    """The per-object evaluation loop of the reference (eval/eval.py:186-362) on this package's renderer.

    dataset: a sequence of per-object dicts as the reference's datasets yield them (unbatched): "path", "images"
    (NV, 3, H, W) in [-1, 1], "poses" (NV, 4, 4) camera-to-world, "focal" (float | tensor), optional "c"; z_near / z_far
    from the arguments or the dataset's attributes (eval.py:153-154).  net / renderer as the driver sets them up
    (eval.py:136-151: caller-side overrides of n_coarse / n_fine / mlp_fine stay with the caller).

    Per object (eval.py:186-362): resume — objects already in <output_dir>/finish.txt are skipped (:113-133, :203-205);
    source views from `source` ("0 1 2") or the look-up table file / dict `viewlist` keyed "<cat>/<obj>" (:156-165,
    :224-231); target views = eval_view_list (file / indices) minus the source views unless include_src (:170-178,
    :246-248); net.encode on the source images (:271-276); every target view rendered — as ONE call per view with the rays
    generated inside the render launch (NeRFRenderer.render_image) on one device, or, when a process group is up, through the
    sharded form of renderer.bind_parallel(net, gpu_id, simple_output=True) in chunks of ray_batch_size (:151, :267,
    :279-284: every chunk cut over the ranks, one all_gather each; rank 0 alone writes finish.txt and the PNGs, the other
    ranks take the resume state from it by one broadcast) — with the
    frames brought to the host asynchronously (frame_to_host_async) while the next view renders; clamp to [0, 1] and
    reshape (:286-293); PNGs "<obj>/<view:06>.png" quantised by truncation (:294-301); PSNR / SSIM per view against
    images * 0.5 + 0.5, averaged per object (:318-347); running means and a "<obj> <psnr> <ssim> 1" line appended to
    finish.txt (:348-362).  Returns (mean_psnr, mean_ssim, n_objects_counted) over everything in finish.txt.

    Deliberate differences: the rays of all target views are not concatenated and re-split (:250-267) — a view is the unit;
    the random jitter is keyed by (seed, ray): one base seed per call (`seed`, else drawn from torch's generator on rank 0
    and broadcast) and a seed derived per (object, view), so neither the chunk size, nor the number of ranks, nor a resume changes a pixel; SSIM is this module's restatement
    (skimage is not importable here: parity unpinned); the depth EXR (:304-306, :312) is not written (it needs cv2, which
    this package does not depend on).

    write_depth=True writes "<obj>/<view:06>_depth.npy" instead: float32 (H, W), (depth - z_near) / (z_far - z_near)
    (:288-289), with either back end.  With depth_png=True as well it also writes the reference's colour-mapped
    "<obj>/<view:06>_depth_norm.png" (:307-313) = cmap(normalised depth): util.cmap on the host with metrics="host",
    util.cmap_device (pnr_cmap) where the frame lies with metrics="device".  lut: the (256, 3) uint8 colour table, None =
    util.hot_lut() (parity unpinned against cv2.COLORMAP_HOT, see there).  Without depth_png the written files are unchanged.

    metrics="host" (the default) is the reference's recipe: every frame is copied to the host as fp32 and numpy / scipy do
    the rest.  metrics="device": util.eval_frame (pnr_eval_frame) runs on each frame where the render left it — the object's
    ground-truth views are uploaded once, the per-view (mse, ssim) pairs collect in one (n_views, 2) fp64 device buffer, and
    only what will be written (uint8 frames, compare strips, normalised depth: 3 bytes per pixel instead of 16) travels to
    pinned host buffers, asynchronously; the host waits ONCE per object, before it writes that object's files and its
    finish.txt line.  PSNR is 10 log10(1 / mse) on the host in fp64.  Under a process group every rank computes the metrics
    (the return value is the same everywhere) and rank 0 alone copies bytes out and writes.  A ground truth whose size differs
    from the render's (scale != 1 with comparison) is a ValueError: there is no resampling on the device."""
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics must be 'host' or 'device', got {metrics!r}")
    dev = net.poses.device
    z_near = float(getattr(dataset, "z_near", None) if z_near is None else z_near)
    z_far = float(getattr(dataset, "z_far", None) if z_far is None else z_far)
    sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank = dist.get_rank() if sharded else 0
    log = _open_log(output_dir, sharded, rank)
    resumes = log.path is not None
    writes_files = resumes and rank == 0
    base_seed = _base_seed(seed, sharded)
    if log.cnt > 0 and verbose:
        print("resume psnr", log.mean()[0], "ssim", log.mean()[1])

    if isinstance(viewlist, str) and viewlist:
        viewlist = read_source_view_lut(viewlist)
    fixed_source = None if viewlist else torch.tensor(sorted(int(x) for x in str(source).split()), dtype=torch.long)
    if isinstance(eval_view_list, str):
        eval_view_list = read_eval_view_list(eval_view_list)
    render_par = _sharded_renderer(net, renderer) if sharded else None
    o = SimpleNamespace(z_near=z_near, z_far=z_far, compare_gt=not no_compare_gt, write_images=write_images,
                        write_compare=write_compare, write_depth=write_depth, depth_png=depth_png, lut=lut)
    back = _DeviceBackEnd(o, dev) if metrics == "device" else _HostBackEnd(o, renderer.frame_to_host_async)
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            for obj_idx in range(len(dataset)):
                if max_objects is not None and obj_idx >= max_objects:      # eval.py:187 stops after 50 objects
                    break
                data = dataset[obj_idx]
                dpath = data["path"]
                obj_base, cat_name = os.path.basename(dpath), os.path.basename(os.path.dirname(dpath))
                obj_name = cat_name + "_" + obj_base if multicat else obj_base
                if verbose:
                    print("OBJECT", obj_idx, "OF", len(dataset), dpath)
                if resumes and obj_name in log.finished:
                    if verbose:
                        print("(skip)")
                    continue
                images = data["images"]                                       # (NV, 3, H, W)
                H, W = _render_size(images, scale)
                back.check_size(H, W, images)                                 # before anything is rendered or created
                src = viewlist[cat_name + "/" + obj_base] if viewlist else fixed_source
                src_mask, tgt_mask, novel = target_views(images.shape[0], src, eval_view_list, include_src)
                poses, focal, c = _encode_object(net, data, src_mask, dev, sharded)
                focal, c = focal * scale, None if c is None else c * scale
                # the jitter is keyed by (object, view), not by a running count: a resumed run draws what the uninterrupted run drew
                obj_seed = frame_seed(base_seed, obj_idx)
                views = novel.tolist()
                back.begin(os.path.join(output_dir, obj_name) if writes_files else None, images, tgt_mask, views, H, W)
                for i, vi in enumerate(views):
                    rgb, depth = _render_view(net, renderer, render_par, frame_seed(obj_seed, vi), poses[vi], W, H, focal, c,
                                              z_near, z_far, ray_batch_size)
                    back.frame(i, vi, rgb, depth)
                curr_psnr, curr_ssim = back.finish()
                log.append(obj_name, curr_psnr, curr_ssim, 1)
                if verbose and not no_compare_gt:
                    print("curr psnr", curr_psnr, "ssim", curr_ssim, "running psnr", log.mean()[0], "running ssim", log.mean()[1])
    finally:
        net.train(was_training)
        log.close()
    if sharded:
        dist.barrier()              # rank 0's files are complete when any rank returns
    if verbose and log.cnt:
        print("final psnr", log.mean()[0], "ssim", log.mean()[1])
    return (*log.mean(), log.cnt)


# ------------------------------------------------------------------------------------ the approximate evaluation (eval_approx.py)
def _approx_source(source):
    """`source` as eval_approx.py:96 parses --source ("0 2 5", "-1"), or a sequence of view indices -> LongTensor (NS,)."""
    views = source.split() if isinstance(source, str) else (source.tolist() if torch.is_tensor(source) else list(source))
    return torch.tensor([int(v) for v in views], dtype=torch.long).reshape(-1)


def draw_approx_views(SB, NV, source):
    """The view draws of eval/eval_approx.py:111-118 for one loader batch of SB objects with NV views each, on torch's global
    CPU generator and in the reference's order, so that one torch.random.manual_seed gives the reference's views batch after
    batch (tests/golden/eval_approx_views.npz): source "-1" draws randint(0, NV, (SB, 1)) as the one source view of each
    object, any other source ("0 2 5", or a sequence) is used for every object; then dest_view = randint(0, NV - NS, (SB, 1)),
    moved past the source views by dest_view += dest_view >= src_view[:, i:i+1] for i in 0 .. NS - 1.
    -> (src_view (SB, NS), dest_view (SB, 1)), int64 on the host.
    ValueError, before anything is drawn, where the reference leaves the result undefined: a source list that is not strictly
    increasing (the skips then land on source views), a source index outside [0, NV), no view left for a target (NV - NS < 1)."""
    source = _approx_source(source)
    SB, NV, NS = int(SB), int(NV), int(source.numel())
    random_source = NS == 1 and int(source[0]) == -1
    if NS < 1:
        raise ValueError("source must name at least one view, or be -1")
    if not random_source:
        if NS > 1 and not bool((source[1:] > source[:-1]).all()):
            raise ValueError(f"source views must be strictly increasing, got {source.tolist()}")
        if int(source.min()) < 0 or int(source.max()) >= NV:
            raise ValueError(f"source views {source.tolist()} outside [0, {NV})")
    if NV - NS < 1:
        raise ValueError(f"{NS} source views of {NV} leave no target view")
    if random_source:
        src_view = torch.randint(0, NV, (SB, 1))
    else:
        src_view = source.unsqueeze(0).expand(SB, -1)
    dest_view = torch.randint(0, NV - NS, (SB, 1))
    for i in range(NS):
        dest_view += dest_view >= src_view[:, i:i + 1]
    return src_view, dest_view


def evaluate_approx(net, renderer, loader, *, source="64", seed=1234, z_near=None, z_far=None, metrics="host",
                    render_par=None, max_batches=None, per_object=None, verbose=True):
    """The approximate evaluation of the reference (eval/eval_approx.py:89-153, "since eval.py is too slow") on this package's
    renderer: ONE random target view per object, a loader batch of objects per render call.  -> (mean_psnr, mean_ssim, count).

    loader: an iterable of batched dicts as the reference's DataLoader yields them (:68-70), host tensors: "images"
    (SB, NV, 3, H, W) in [-1, 1], "poses" (SB, NV, 4, 4) camera-to-world, "focal", optional "c"; "masks" is ignored.  z_near /
    z_far from the arguments or loader.dataset's attributes (:86-87).  net / renderer as the driver sets them up: the overrides
    of :62-64 and :76-82 (--coarse, n_coarse >= 64) stay with the caller, as in evaluate().

    torch.random.manual_seed(seed) once before the loop (:89).  Per batch (:101-152): focal = data["focal"][0] serves the
    whole batch (:105); the views from draw_approx_views (:111-118); the rays of the SB target cameras (:120-123) built on
    the device into one (SB, H*W, 8) tensor (util.gen_rays_device, the bits of pnr_gen_rays); net.encode on the (SB, NS, ..)
    selection of source images and poses (:125-132) — only the selection and the SB ground-truth views are uploaded
    (util.upload, pinned and asynchronous), never all NV views; ONE render call for all SB objects (:134) through render_par,
    or a _RenderWrapper(net, renderer, simple_output=True) when none is given; SSIM and PSNR per object on the UNCLAMPED frames
    against images * 0.5 + 0.5 (:136-150); the running "curr psnr .. ssim .." line (:152) when verbose, and the final line (:153).

    metrics="host" is the reference's tail: one D2H copy of the batch's fp32 frames, evalio.ssim / evalio.psnr per object.
    metrics="device": one util.eval_frames(.., clamp=False) call per batch (pnr_eval_frames) on the frames where the render
    left them; the (SB, 2) [mse, ssim] pairs stay on the device and PSNR is 10 log10(1 / mse) on the host in fp64, inf for
    mse == 0 and NaN for a NaN, as in evaluate(metrics="device").  The host reads one batch's pairs per batch when verbose (the
    running line needs them) and everything in a single read after the last batch otherwise.
    per_object: a list that receives (batch, index_in_batch, src_views, dest_view, psnr, ssim) per object.
    max_batches: stop after that many batches.

    Deliberate differences: data["c"][0] is used as the principal point of the batch when the loader gives one (the
    reference ignores "c", :120-132, and so renders every dataset about the image centre; without the key this is the
    reference's behaviour).  The render does not consume torch's generator — util.seed_from_torch would change every
    later view draw relative to the reference: batch b renders under renderer.keyed(frame_seed(seed, b)), with object
    stride 0, so the objects of a batch follow each other in the ray key and share no jitter.  SSIM is this module's
    restatement (skimage is not importable here: parity unpinned); the view draws are pinned by fixture.  min(H, W) < 7 (no
    whole SSIM window) is a ValueError before anything is rendered.  Under an initialised process group of more than one
    rank the function raises NotImplementedError: evaluate() is the sharded driver."""
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics must be 'host' or 'device', got {metrics!r}")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("evaluate_approx runs in one process; evaluate() is the driver that shards over ranks")
    source = _approx_source(source)
    dset = getattr(loader, "dataset", None)
    z_near = getattr(dset, "z_near", None) if z_near is None else z_near
    z_far = getattr(dset, "z_far", None) if z_far is None else z_far
    torch.random.manual_seed(seed)
    total_psnr = total_ssim = 0.0
    cnt = 0
    dev = was_training = None
    views, pairs = [], []                # per batch: (src_view, dest_view); device back end: the (SB, 2) device pairs

    def account(b, numbers):
        """numbers: (psnr, ssim) per object of batch b, in order."""
        nonlocal total_psnr, total_ssim, cnt
        for sb, (p, s) in enumerate(numbers):
            total_ssim += s
            total_psnr += p
            if per_object is not None:
                per_object.append((b, sb, views[b][0][sb].tolist(), int(views[b][1][sb, 0]), p, s))
        cnt += len(numbers)

    def read_pairs(dev_pairs):
        """One read of device pairs (n, 2) -> [(psnr, ssim)] * n."""
        host = torch.empty(dev_pairs.shape, dtype=torch.float64, pin_memory=True)
        host.copy_(dev_pairs, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        done.synchronize()
        return [(_psnr_of_mse(float(m)), float(s)) for m, s in host.tolist()]

    try:
        with torch.no_grad():
            for b, data in enumerate(loader):
                if max_batches is not None and b >= max_batches:
                    break
                images = data["images"]                                        # (SB, NV, 3, H, W)
                poses = data["poses"]                                          # (SB, NV, 4, 4)
                SB, NV, _, H, W = images.shape
                if min(H, W) < 7:
                    raise ValueError(f"{H} x {W} frames hold no whole 7 x 7 SSIM window")
                if dev is None:                                                # the first batch: before it nothing touches net
                    dev, was_training = net.poses.device, net.training
                    net.eval()
                    z_near, z_far = float(z_near), float(z_far)
                    if render_par is None:
                        from .render.nerf import _RenderWrapper
                        render_par = _RenderWrapper(net, renderer, simple_output=True).eval()
                focal = torch.as_tensor(data["focal"][0]).float()              # :105
                focal = focal.reshape(()) if focal.numel() == 1 else focal.reshape(2)
                c = torch.as_tensor(data["c"][0]).float() if data.get("c") is not None else None
                src_view, dest_view = draw_approx_views(SB, NV, source)        # :111-118
                views.append((src_view, dest_view))

                dest_poses = util.batched_index_select_nd(poses, dest_view).reshape(SB, 4, 4).float()
                all_rays = torch.empty(SB, H * W, 8, device=dev, dtype=torch.float32)
                for sb in range(SB):
                    util.gen_rays_device(dest_poses[sb], W, H, focal, z_near, z_far, c=c, out=all_rays[sb])

                pri_images = util.batched_index_select_nd(images, src_view)    # (SB, NS, 3, H, W)
                pri_poses = util.batched_index_select_nd(poses, src_view)      # (SB, NS, 4, 4)
                net.encode(util.upload(pri_images.float().contiguous(), dev), util.upload(pri_poses.float().contiguous(), dev),
                           util.upload(focal[None] if focal.dim() else focal, dev),
                           c=None if c is None else util.upload(c.reshape(1, -1), dev))

                with renderer.keyed(frame_seed(seed, b)):
                    rgb_fine, _depth = render_par(all_rays)
                _depth = None
                images_gt = util.batched_index_select_nd(images, dest_view).reshape(SB, 3, H, W).float()
                if metrics == "device":
                    gt_dev = util.upload(images_gt.contiguous(), dev)
                    pairs.append(util.eval_frames(rgb_fine.reshape(SB, H * W, 3), gt_dev, clamp=False))
                    if verbose:
                        account(b, read_pairs(pairs[-1]))
                else:
                    rgb_dev = rgb_fine.reshape(SB, H, W, 3)
                    rgb_h = torch.empty(rgb_dev.shape, dtype=torch.float32, pin_memory=True)
                    rgb_h.copy_(rgb_dev, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(torch.cuda.current_stream(dev))
                    done.synchronize()
                    rgb_np = rgb_h.numpy()
                    rgb_gt_all = (images_gt * 0.5 + 0.5).permute(0, 2, 3, 1).contiguous().numpy()
                    numbers = []
                    for sb in range(SB):
                        s = ssim(rgb_np[sb], rgb_gt_all[sb], data_range=1)
                        numbers.append((float(psnr(rgb_np[sb], rgb_gt_all[sb], data_range=1)), s))
                    account(b, numbers)
                if verbose:
                    print("curr psnr", total_psnr / cnt, "ssim", total_ssim / cnt)
            if metrics == "device" and not verbose and pairs:
                numbers, at = read_pairs(torch.cat(pairs, 0)), 0               # the single read of the run
                for b, p in enumerate(pairs):
                    account(b, numbers[at:at + p.shape[0]])
                    at += p.shape[0]
    finally:
        if was_training is not None:
            net.train(was_training)
    if not cnt:
        return 0.0, 0.0, 0
    if verbose:
        print("final psnr", total_psnr / cnt, "ssim", total_ssim / cnt)
    return total_psnr / cnt, total_ssim / cnt, cnt
