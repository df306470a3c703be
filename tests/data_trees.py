"""Shared by tests/test_data_cpu.py and tests/test_gpu_data.py: SRN and DVR dataset folders written with PIL / numpy, from
values the tests state themselves."""
import os

import numpy as np
from PIL import Image


def boxed_views(NV, H, W, boxes, seed):
    """uint8 (NV, H, W, 3): white (255) background, and inside box v = (cmin, rmin, cmax, rmax), corners included, random
    colours in [0, 254] — so the foreground of view v is exactly its box."""
    rng = np.random.default_rng(seed)
    images = np.full((NV, H, W, 3), 255, np.uint8)
    for v, (cmin, rmin, cmax, rmax) in enumerate(boxes):
        images[v, rmin:rmax + 1, cmin:cmax + 1] = rng.integers(0, 255, (rmax - rmin + 1, cmax - cmin + 1, 3), dtype=np.uint8)
    return images


def random_poses(NV, seed):
    """float32 (NV, 4, 4): a dense 3 x 4 block of values that float32 holds and a text file round-trips, bottom row 0 0 0 1."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((NV, 4, 4), np.float32)
    poses[:, :3] = rng.integers(-2000, 2000, (NV, 3, 4)).astype(np.float32) / 1024.0
    poses[:, 3, 3] = 1.0
    return poses


def write_srn_object(obj_dir, images, poses, focal, cx, cy, stems, rgba=()):
    """One SRN object: intrinsics.txt ("focal cx cy 0." first, "H W" last), rgb/<stem>.png and pose/<stem>.txt per view.
    Views listed in rgba are saved with an alpha channel."""
    NV, H, W, _ = images.shape
    os.makedirs(os.path.join(obj_dir, "rgb"))
    os.makedirs(os.path.join(obj_dir, "pose"))
    with open(os.path.join(obj_dir, "intrinsics.txt"), "w") as f:
        f.write(f"{focal!r} {cx!r} {cy!r} 0.\n0. 0. 0.\n1.\n{H} {W}\n")
    for v in range(NV):
        img = images[v]
        if v in rgba:
            img = np.concatenate([img, np.full((H, W, 1), 7, np.uint8)], axis=-1)
        Image.fromarray(img).save(os.path.join(obj_dir, "rgb", stems[v] + ".png"))
        with open(os.path.join(obj_dir, "pose", stems[v] + ".txt"), "w") as f:
            f.write(" ".join(repr(float(x)) for x in poses[v].reshape(-1)) + "\n")


def write_dvr_object(obj_dir, images, masks, cameras, mask_channels=1):
    """One DVR object: image/<v:04>.png, mask/<v:04>.png (mode L, or RGB with mask_channels = 3), cameras.npz."""
    os.makedirs(os.path.join(obj_dir, "image"))
    os.makedirs(os.path.join(obj_dir, "mask"))
    for v in range(images.shape[0]):
        Image.fromarray(images[v]).save(os.path.join(obj_dir, "image", f"{v:04}.png"))
        m = masks[v] if mask_channels == 1 else np.repeat(masks[v][..., None], 3, axis=-1)
        Image.fromarray(m).save(os.path.join(obj_dir, "mask", f"{v:04}.png"))
    np.savez(os.path.join(obj_dir, "cameras.npz"), **cameras)
