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
* calc_metrics()              reference eval/calc_metrics.py:119-340   PSNR / SSIM (and an LPIPS hook) of the SAVED PNGs against
                              the dataset's image files: metrics.txt per object (map), all_metrics.txt (reduce)
"""
import json
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
             verbose=True, seed=None, metrics="host", write_depth=False, depth_png=False, lut=None, occupancy=None):
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
    from the render's (scale != 1 with comparison) is a ValueError: there is no resampling on the device.

    occupancy (None: everything above, unchanged): a dict of render.occupancy.OccupancyGrid.from_net's keywords
    (sigma_thresh is required) plus an optional "pad".  The grid is built once per object, after encode, and ALL target
    views of the object are bounded in one NeRFRenderer.render_frames_bounded call (empty space culled, one host read of the
    counts per object; see there for the noise) under the seeds the views have without it; the back ends get the frames
    unchanged.  A ValueError under a process group of several ranks, before anything is written.

    finish.txt holds the metrics of the unquantised frames; calc_metrics() recomputes them on the PNGs written here."""
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics must be 'host' or 'device', got {metrics!r}")
    if occupancy is not None:
        from .render import occupancy as occ
        occ.refuse_sharded("evaluate")
        if not isinstance(occupancy, dict):
            raise TypeError("evaluate builds one grid per object: occupancy must be a dict of OccupancyGrid.from_net keywords")
        if "sigma_thresh" not in occupancy:
            raise TypeError("occupancy needs sigma_thresh: no default has been measured on a trained model")
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
                if occupancy is not None and views:
                    grid, pad = occ.resolve(occupancy, net)
                    all_rgb, all_depth = renderer._render_frames_bounded(net, poses[views], W, H, focal, z_near, z_far, grid, c, pad,
                                                                         None, [frame_seed(obj_seed, vi) for vi in views])
                for i, vi in enumerate(views):
                    if occupancy is not None:
                        rgb, depth = all_rgb[i], all_depth[i]
                    else:
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


# ------------------------------------------------------------------------------------ metrics of the saved PNGs (calc_metrics.py)
DTU_BAD_VIEWS = (3, 4, 5, 6, 7, 16, 17, 18, 19, 20, 21, 36, 37, 38, 39)        # calc_metrics.py:143-145
METRIC_NAMES = ("psnr", "ssim", "lpips")                                      # calc_metrics.py:275, the order of every line


def _image_layout(dataset_format, list_name):
    """-> (name of the object list file or "", name of an object's image folder or ""), calc_metrics.py:101-112."""
    if dataset_format == "dvr":
        return list_name + ".lst", "image"
    if dataset_format == "srn":
        return "", "rgb"
    if dataset_format == "nerf":
        warnings.warn("test split not implemented for NeRF synthetic data format")
        return "", ""
    raise NotImplementedError("Not supported data format " + str(dataset_format))


def _view_ids(x):
    """"0 1 2", a sequence or a tensor of view indices, or None -> list of int."""
    if x is None:
        return []
    if isinstance(x, str):
        return [int(v) for v in x.split()]
    return [int(v) for v in (x.tolist() if torch.is_tensor(x) else x)]


def _metric_objects(datadir, output, list_file, multicat, verbose):
    """Object discovery of calc_metrics.py:159-183 -> [(dataset folder, render folder)] of the objects whose render folder
    exists, categories in sorted order and the objects sorted inside each."""
    cats = sorted(os.listdir(datadir)) if multicat else ["."]
    all_objs, total = [], 0
    if verbose:
        print("CATEGORICAL SUMMARY")
    for cat in cats:
        cat_root = os.path.join(datadir, cat)
        if not os.path.isdir(cat_root):
            continue
        objs = sorted(os.listdir(cat_root))
        if list_file:
            with open(os.path.join(cat_root, list_file)) as f:
                split = {x.strip() for x in f.readlines()}
            objs = [x for x in objs if x in split]
        pairs = [(os.path.join(cat_root, x), os.path.join(output, cat + "_" + x if multicat else x)) for x in objs]
        pairs = [p for p in pairs if os.path.isdir(p[0])]
        avail = [p for p in pairs if os.path.exists(p[1])]
        if verbose:
            print(cat, "TOTAL", len(pairs), "AVAILABLE", len(avail))
        total += len(pairs)
        all_objs.extend(avail)
    if verbose:
        print(">>> USING", len(all_objs), "OF", total, "OBJECTS")
    return all_objs


def _counted_views(im_root, rend_path, exclude, eval_views):
    """The (ground-truth file, render file) pairs calc_metrics.py:205, :218-225 counts, in its order."""
    pairs = []
    for im_name in sorted(os.listdir(im_root)):
        stem, ext = os.path.splitext(im_name)
        if ext != ".jpg" and ext != ".png":
            continue
        view = int(stem)
        rend = os.path.join(rend_path, "{:06}.png".format(view))
        if os.path.exists(rend) and view not in exclude and (eval_views is None or view in eval_views):
            pairs.append((os.path.join(im_root, im_name), rend))
    return pairs


def _read_u8(path, modes):
    """(H, W, 3 | 4) uint8 of an 8-bit image file whose PIL mode is one of `modes`."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in modes:
            raise ValueError(f"{path}: image mode {im.mode!r}, expected 8-bit {' or '.join(modes)}")
        return np.asarray(im, dtype=np.uint8)


def _lpips_mean(lpips, preds, gts, batch):
    """calc_metrics.py:238-246: the callable on batches of `batch` pairs, the mean of everything it returned."""
    vals = [torch.as_tensor(lpips(p, g)).reshape(-1).double() for p, g in zip(torch.split(preds, batch, 0), torch.split(gts, batch, 0))]
    return torch.cat(vals).mean().item()


class _PngMetrics:
    """One object's pairs -> (psnr_sum, ssim_sum, lpips mean or None); name: the object, for the messages."""

    def _pair(self, name, gt_path, rend_path, shape):
        gt, pred = _read_u8(gt_path, ("RGB", "RGBA")), _read_u8(rend_path, ("RGB",))
        if gt.shape[:2] != pred.shape[:2]:
            raise ValueError(f"{name}: {rend_path} is {pred.shape[1]} x {pred.shape[0]}, {gt_path} is {gt.shape[1]} x {gt.shape[0]}")
        if shape is not None and pred.shape[:2] != shape:
            raise ValueError(f"{name}: images of two sizes, {shape[1]} x {shape[0]} and {pred.shape[1]} x {pred.shape[0]}")
        return gt, pred


class _PngHost(_PngMetrics):
    """metrics="host", the reference's recipe (:226-233): fp32 / 255 arrays, psnr and ssim one pair at a time."""

    def __init__(self, lpips, lpips_batch_size, device):
        self.lpips, self.batch, self.dev = lpips, lpips_batch_size, device

    def __call__(self, name, pairs):
        psnr_sum = ssim_sum = 0.0
        shape, gts, preds = None, [], []
        for gt_path, rend_path in pairs:
            gt, pred = self._pair(name, gt_path, rend_path, shape)
            shape = pred.shape[:2]
            gt = gt.astype(np.float32)[..., :3] / 255.0
            pred = pred.astype(np.float32) / 255.0
            psnr_sum += float(psnr(pred, gt, data_range=1))
            ssim_sum += ssim(pred, gt, data_range=1)
            if self.lpips is not None:
                gts.append(torch.from_numpy(np.ascontiguousarray(gt)).permute(2, 0, 1) * 2.0 - 1.0)
                preds.append(torch.from_numpy(pred).permute(2, 0, 1) * 2.0 - 1.0)
        if self.lpips is None:
            return psnr_sum, ssim_sum, None
        gts, preds = torch.stack(gts), torch.stack(preds)
        if self.dev is not None:
            gts, preds = gts.to(self.dev), preds.to(self.dev)
        return psnr_sum, ssim_sum, _lpips_mean(self.lpips, preds, gts, self.batch)


class _PngDevice(_PngMetrics):
    """metrics="device": the object's pairs are decoded into two pinned byte buffers, uploaded once per chunk of frames_per_call
    frames, one util.eval_frames_u8 call per chunk writes its rows of the object's (n, 2) buffer, and the host reads that
    buffer once.  A frame's row depends on that frame's bytes alone, so the chunk size does not change a bit."""

    def __init__(self, lpips, lpips_batch_size, device, frames_per_call):
        self.lpips, self.batch, self.dev, self.chunk, self.pin = lpips, lpips_batch_size, device, int(frames_per_call), {}
        if self.chunk < 1:
            raise ValueError(f"frames_per_call must be >= 1, got {frames_per_call}")

    def _pinned(self, key, shape, dtype):
        t = self.pin.get(key)
        if t is None or tuple(t.shape) != tuple(shape):
            t = self.pin[key] = torch.empty(shape, dtype=dtype, pin_memory=True)
        return t

    def __call__(self, name, pairs):
        n, shape, pred_h, gt_h, gt_np = len(pairs), None, None, None, []
        for i, (gt_path, rend_path) in enumerate(pairs):
            gt, pred = self._pair(name, gt_path, rend_path, shape)
            if shape is None:
                shape = pred.shape[:2]
                if min(shape) < 7:
                    raise ValueError(f"{name}: {shape[1]} x {shape[0]} images hold no whole 7 x 7 SSIM window")
                pred_h = self._pinned("pred", (n, *shape, 3), torch.uint8)
            pred_h[i].numpy()[...] = pred
            gt_np.append(gt)
        gc = 4 if all(g.shape[2] == 4 for g in gt_np) else 3              # RGBA travels as it is; a mix is cut to RGB here
        gt_h = self._pinned("gt%d" % gc, (n, *shape, gc), torch.uint8)
        for i, g in enumerate(gt_np):
            gt_h[i].numpy()[...] = g[..., :gc]
        rows = torch.empty(n, 2, dtype=torch.float64, device=self.dev)
        planar = []
        for a in range(0, n, self.chunk):
            b = min(n, a + self.chunk)
            out = util.eval_frames_u8(pred_h[a:b].to(self.dev, non_blocking=True), gt_h[a:b].to(self.dev, non_blocking=True),
                                      want_planar=self.lpips is not None, metrics_out=rows[a:b])
            if self.lpips is not None:
                planar.append(out[1:])
        rows_h = self._pinned("rows", (n, 2), torch.float64)
        rows_h.copy_(rows, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.dev))
        done.synchronize()                                                  # the one wait of this object
        psnr_sum = ssim_sum = 0.0
        for mse, s in rows_h.tolist():
            psnr_sum += _psnr_of_mse(mse)
            ssim_sum += s
        if self.lpips is None:
            return psnr_sum, ssim_sum, None
        preds, gts = torch.cat([p[0] for p in planar]), torch.cat([p[1] for p in planar])
        return psnr_sum, ssim_sum, _lpips_mean(self.lpips, preds, gts, self.batch)


def metrics_map(datadir, output, *, dataset_format="dvr", list_name="softras_test", multicat=False, viewlist="",
                eval_view_list=None, primary="", exclude_dtu_bad=False, overwrite=False, lpips=None, lpips_batch_size=32,
                metrics="host", device=None, frames_per_call=256, verbose=True, rank=0, world=1):
    """The map step of the reference's eval/calc_metrics.py (run_map, :119-254): "<output>/<obj>/metrics.txt" for every object
    of the dataset folder `datadir` that has a render folder under `output` (evaluate(write_images=True) writes those).
    The keyword arguments are the script's flags.  -> the list of metrics.txt paths this call wrote.

    Objects (:159-183): the folders of datadir — of every category folder with multicat, the render folder is then
    "<cat>_<obj>" — kept when the "<list_name>.lst" file of a "dvr" dataset names them and when their render folder exists;
    the images of an object lie in "image" (dvr), "rgb" (srn) or the object folder itself (nerf) (:101-112).  An object whose
    metrics.txt exists is skipped unless overwrite (:203-204).  Views (:205, :218-225): ground-truth files ending in .png or
    .jpg, matched to "<view:06>.png" in the render folder, minus the excluded views, restricted to eval_view_list (a file or
    indices).  PSNR and SSIM of every pair on the 8-bit values / 255 in fp32, against the first three channels of the ground
    truth (:226-231); the per-object means go to metrics.txt as "psnr {}\nssim {}" (:247-251).

    metrics="host": evalio.psnr / evalio.ssim, one pair at a time.  metrics="device": util.eval_frames_u8
    (pnr_eval_frames_u8), frames_per_call pairs per call on `device` (None = the current HIP device); the host waits once per
    object and PSNR is 10 log10(1 / mse) on the host in fp64.
    lpips: a callable (pred, gt) -> n values for two (n, 3, H, W) float32 tensors in [-1, 1], called per batch of
    lpips_batch_size pairs (:238-246) — on the kernel's planar outputs with the device back end, on host tensors moved to
    `device` with the host back end; its mean is written as a third line "lpips {}".  None: no such line (the reference always
    writes one; its lpips package and weights are not part of this project).
    rank, world: this call takes the objects i of the list with i % world == rank.

    Images are read with PIL: 8-bit RGB, or RGBA for the ground truth; the render must be RGB.  ValueError for any other
    mode (naming the file), for a pair or an object of two sizes, for an object without a counted view (the reference
    divides by zero there) and for an object the viewlist does not list.

    Deliberate difference: with viewlist (a file or a dict as read_source_view_lut returns it) the excluded views are the
    union of the table's views for "<cat>/<obj>" (:212-213), `primary` and the DTU list; the reference itself raises there
    (:216 calls .extend on a tensor).  This step follows the reference by reading only: it cannot run here (it needs lpips and
    a CUDA device), so it is unpinned, and SSIM is this module's restatement of skimage as everywhere else."""
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics must be 'host' or 'device', got {metrics!r}")
    list_file, img_dir = _image_layout(dataset_format, list_name)
    lut = None
    if isinstance(viewlist, str):
        if viewlist:
            if verbose:
                print("Excluding views from list", viewlist)
            lut = read_source_view_lut(viewlist)
    elif viewlist is not None:
        lut = viewlist
    base_exclude = set(_view_ids(primary)) | (set(DTU_BAD_VIEWS) if exclude_dtu_bad else set())
    eval_views = None
    if eval_view_list is not None:
        eval_views = set(_view_ids(read_eval_view_list(eval_view_list) if isinstance(eval_view_list, str) else eval_view_list))
        if verbose:
            print("Only using views", sorted(eval_views))
    if metrics == "device":
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        back = _PngDevice(lpips, lpips_batch_size, dev, frames_per_call)
    else:
        back = _PngHost(lpips, lpips_batch_size, device)
    written = []
    with torch.no_grad():
        for i, (path, rend_path) in enumerate(_metric_objects(datadir, output, list_file, multicat, verbose and rank == 0)):
            out_path = os.path.join(rend_path, "metrics.txt")
            if i % world != rank or (os.path.exists(out_path) and not overwrite):
                continue
            name = os.path.basename(rend_path)
            exclude = set(base_exclude)
            if lut is not None:
                key = name.replace("_", "/")                                # :212
                if key not in lut:
                    raise ValueError(f"{name}: the viewlist has no line for {key!r}")
                exclude |= set(_view_ids(lut[key]))
            pairs = _counted_views(os.path.join(path, img_dir) if img_dir else path, rend_path, exclude, eval_views)
            if not pairs:
                raise ValueError(f"{name}: no view to compare in {rend_path}")
            psnr_sum, ssim_sum, lp = back(name, pairs)
            txt = "psnr {}\nssim {}".format(psnr_sum / len(pairs), ssim_sum / len(pairs))
            if lp is not None:
                txt += "\nlpips {}".format(lp)
            with open(out_path, "w") as f:
                f.write(txt)
            written.append(out_path)
    return written


def metrics_reduce(datadir, output, *, multicat=False, metadata="metadata.yaml", dtu_sort=False, verbose=True):
    """The reduce step of the reference's eval/calc_metrics.py (run_reduce, :257-340), pinned byte for byte by
    tests/golden/calc_metrics_reduce.npz: the metrics.txt of every folder of `output` whose name does not start with "_", in
    sorted order — by the scan number of "scan<N>" with dtu_sort (:264-271) —, running sums per metric and, with multicat, per
    category (the part of the folder name before the first "_"), divided by the counts; "<output>/all_metrics.txt" holds, with
    multicat, one line "{:12s} psnr: {:.6f} .. n_inst: {}" per category that has objects — its name from the first entry of
    datadir/<metadata>["<cat>"]["name"], a file read as JSON as the reference does — then "---" and the "total" line, and
    the line of totals alone otherwise.  -> the dict of means (name -> mean, and "<cat>.<name>" with multicat); its .text is what
    was written.

    The metric names are those found in the files, in the reference's order psnr, ssim, lpips (the reference always has all
    three; metrics_map writes no lpips line without an lpips callable).  ValueError for files that disagree about the names,
    for a name outside those three, for a category the metadata does not list, and for no object at all."""
    if multicat:
        with open(os.path.join(datadir, metadata)) as f:
            meta = json.load(f)
        cats = sorted(meta.keys())
        cat_description = {cat: meta[cat]["name"].split(",")[0] for cat in cats}
    objs = [x for x in os.listdir(output) if x[0] != "_" and os.path.isdir(os.path.join(output, x))]
    objs = sorted(objs, key=lambda x: int(x[4:])) if dtu_sort else sorted(objs)
    if not objs:
        raise ValueError(f"{output}: no object folder to reduce")
    if verbose:
        print(">>> PROCESSING", len(objs), "OBJECTS")
    names, sums, cat_sz = None, {}, {cat: 0 for cat in cats} if multicat else {}
    for obj in objs:
        with open(os.path.join(output, obj, "metrics.txt")) as f:
            rows = [line.split() for line in f.readlines()]
        found = [r[0] for r in rows]
        if names is None:
            if any(n not in METRIC_NAMES for n in found) or len(set(found)) != len(found) or not found:
                raise ValueError(f"{obj}/metrics.txt: metric names {found}, expected some of {list(METRIC_NAMES)}")
            names = [n for n in METRIC_NAMES if n in found]
            for n in names:
                sums[n] = 0.0
                for cat in cat_sz:
                    sums[cat + "." + n] = 0.0
        if sorted(found) != sorted(names):
            raise ValueError(f"{obj}/metrics.txt has the metrics {found}, the objects before it {names}")
        if multicat:
            cat = obj.split("_")[0]
            if cat not in cat_sz:
                raise ValueError(f"{obj}: category {cat!r} is not in {metadata}")
            cat_sz[cat] += 1
            for metric, val in rows:
                sums[cat + "." + metric] += float(val)
        for metric, val in rows:
            sums[metric] += float(val)
    for n in names:
        for cat in cat_sz:
            if cat_sz[cat] > 0:
                sums[cat + "." + n] /= cat_sz[cat]
        sums[n] /= len(objs)
    lines = []
    if multicat:
        for cat in cats:
            if cat_sz[cat] > 0:
                txt = "{:12s}".format(cat_description[cat])
                for n in names:
                    txt += " {}: {:.6f}".format(n, sums[cat + "." + n])
                lines.append(txt + " n_inst: {}".format(cat_sz[cat]))
        total = "---\n{:12s}".format("total")
    else:
        total = ""
    for n in names:
        total += " {}: {:.6f}".format(n, sums[n])
    lines.append(total)
    text = "\n".join(lines)
    out_path = os.path.join(output, "all_metrics.txt")
    with open(out_path, "w") as f:
        f.write(text)
    if verbose:
        print("WROTE", out_path)
        print(text)
    return MetricTotals(sums, text)


class MetricTotals(dict):
    """What metrics_reduce returns: the means by name; .text: the contents of all_metrics.txt."""

    def __init__(self, values, text):
        super().__init__(values)
        self.text = text


def calc_metrics(datadir, output, *, dataset_format="dvr", list_name="softras_test", multicat=False, viewlist="",
                 eval_view_list=None, primary="", exclude_dtu_bad=False, overwrite=False, reduce_only=False,
                 metadata="metadata.yaml", dtu_sort=False, lpips=None, lpips_batch_size=32, metrics="host", device=None,
                 frames_per_call=256, verbose=True):
    """The reference's eval/calc_metrics.py, the step after eval.py: metrics_map (unless reduce_only), then metrics_reduce; the
    keyword arguments are the script's flags (see the two functions) plus this package's metrics / device / frames_per_call /
    verbose.  -> the MetricTotals of metrics_reduce.

    evaluate() already puts PSNR / SSIM into finish.txt, but of the unquantised frames: the published tables, and the
    per-category table of the NMR experiment, are the metrics of the PNGs, which this recomputes from the files alone.

    Under an initialised process group object i of the list belongs to rank i % world; every object has its own metrics.txt,
    so there is nothing to merge: a barrier, rank 0 reduces, and one broadcast gives every rank rank 0's totals."""
    sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    rank, world = (dist.get_rank(), dist.get_world_size()) if sharded else (0, 1)
    if not reduce_only:
        if verbose and rank == 0:
            print(">>> Compute")
        metrics_map(datadir, output, dataset_format=dataset_format, list_name=list_name, multicat=multicat, viewlist=viewlist,
                    eval_view_list=eval_view_list, primary=primary, exclude_dtu_bad=exclude_dtu_bad, overwrite=overwrite,
                    lpips=lpips, lpips_batch_size=lpips_batch_size, metrics=metrics, device=device,
                    frames_per_call=frames_per_call, verbose=verbose, rank=rank, world=world)
    elif metrics not in ("host", "device"):
        raise ValueError(f"metrics must be 'host' or 'device', got {metrics!r}")
    if sharded:
        dist.barrier()                  # every rank's metrics.txt files are written
    totals = None
    if rank == 0:
        if verbose:
            print(">>> Reduce")
        totals = metrics_reduce(datadir, output, multicat=multicat, metadata=metadata, dtu_sort=dtu_sort, verbose=verbose)
    if sharded:
        box = [None if totals is None else (dict(totals), totals.text)]
        dist.broadcast_object_list(box, src=0)
        totals = MetricTotals(*box[0])
    return totals
