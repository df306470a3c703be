"""Shared by the tests that drive evalio.evaluate and train's device-side steps, and by tools/bench_eval.py: the synthetic
dataset, a decoder for the PNGs evalio.write_png writes, and the probe for torch's sync debug mode."""
import struct
import zlib

import numpy as np
import torch


class Objects(list):
    """A dataset as evaluate() takes it: per-object dicts plus the depth range as attributes."""
    z_near, z_far, lindisp = 1.25, 2.75, False


def make_dataset(net32, rend, n_obj, NV, W, H, focal, seed=777, angle_step=40.0):
    """Ground truth = this package's fp32-path render of every target view with the jitter evaluate(seed=seed) will draw for
    that (object, view): evalio keys the per-view seed by frame_seed(frame_seed(seed, object), view)."""
    import golden_util as gu
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    data = Objects()
    for o in range(n_obj):
        poses = torch.from_numpy(np.stack([gu.pose_spherical(angle_step * v + 13.0 * o, -20.0 - 3.0 * o, 2.0) for v in range(NV)]))
        g = torch.Generator().manual_seed(100 + o)
        src_img = torch.rand(1, 3, H, W, generator=g) * 2 - 1                 # the source view is a random image: only the
        images = torch.zeros(NV, 3, H, W)                                       # trunk sees it
        images[0] = src_img[0]
        net32.encode(src_img.cuda()[None], poses[:1].cuda()[None], torch.tensor(focal)[None].cuda())
        for v in range(1, NV):
            rend.forced_seed = frame_seed(frame_seed(seed, o), v)               # the same jitter in ground truth and evaluation
            rgb, _ = rend.render_image(net32, poses[v], W, H, focal, data.z_near, data.z_far)
            images[v] = (rgb.clamp(0, 1).permute(2, 0, 1) * 2 - 1).cpu()
        data.append(dict(path=f"/data/cat{o % 2}/obj{o:03d}", images=images, poses=poses, focal=focal))
    rend.forced_seed = None
    return data


def read_png(path):
    """(H, W, 3) uint8 of an 8-bit RGB PNG with one IDAT chunk and filter-0 scanlines, which is what evalio.write_png writes."""
    raw = open(path, "rb").read()
    w, h = struct.unpack(">II", raw[16:24])
    at = raw.index(b"IDAT")
    n = struct.unpack(">I", raw[at - 4:at])[0]
    return np.frombuffer(zlib.decompress(raw[at + 4:at + 4 + n]), np.uint8).reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)


def sync_debug_mode_works():
    """Whether torch.cuda.set_sync_debug_mode("error") turns a host read of the device into an error under this build."""
    x = torch.ones(1, device="cuda")
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            x.item()
        except RuntimeError:
            return True
        return False
    except Exception:
        return False
    finally:
        torch.cuda.set_sync_debug_mode("default")
