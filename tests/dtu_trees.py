"""Shared by tests/test_dtu_cpu.py and tests/test_gpu_color_jitter.py: DTU scan folders written with PIL / numpy from cameras
the tests choose — P = lambda K [R | -R C] — and the poses the layout's formulas give for them, evaluated in float64."""
import os

import numpy as np
from PIL import Image

import data_trees as dt

FLIP = np.diag([1.0, -1.0, -1.0, 1.0])


def rotation(seed):
    """A rotation matrix (3, 3) float64, det +1."""
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    return Q * np.sign(np.linalg.det(Q))


def intrinsics(fx, fy, cx, cy, skew=0.0):
    return np.array([[fx, skew, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def world_mat(K, R, C, lam=1.0):
    """(4, 4) float64: lam K [R | -R C] over the row 0 0 0 1."""
    P = np.eye(4)
    P[:3] = lam * (K @ np.concatenate([R, -(R @ C)[:, None]], axis=1))
    return P


def scale_mat(scale, offset):
    S = np.eye(4)
    S[:3, :3] = np.diag(scale)
    S[:3, 3] = offset
    return S


def expected_pose(R, C, S=None):
    """The item's pose for a camera (R, C) by the layout's formula, float64: [[R^T, C], [0, 1]], the scale matrix's offset and
    diagonal taken out of the centre, then D @ pose @ D."""
    pose = np.eye(4)
    pose[:3, :3] = R.T
    pose[:3, 3] = C if S is None else (C - S[:3, 3]) / np.diagonal(S)[:3]
    return FLIP @ pose @ FLIP


def camera_of_pose(pose):
    """(R, C) whose expected_pose (without a scale matrix) is `pose` (4, 4)."""
    raw = FLIP @ np.asarray(pose, dtype=np.float64) @ FLIP
    return raw[:3, :3].T.copy(), raw[:3, 3].copy()


def write_scan(scan_dir, images, cameras, masks=None):
    """One scan: image/<v:06>.png, mask/<v:03>.png when masks (NV, H, W) uint8 are given, cameras.npz."""
    os.makedirs(os.path.join(scan_dir, "image"))
    for v in range(images.shape[0]):
        Image.fromarray(images[v]).save(os.path.join(scan_dir, "image", f"{v:06}.png"))
    if masks is not None:
        os.makedirs(os.path.join(scan_dir, "mask"))
        for v in range(masks.shape[0]):
            Image.fromarray(masks[v]).save(os.path.join(scan_dir, "mask", f"{v:03}.png"))
    np.savez(os.path.join(scan_dir, "cameras.npz"), **cameras)


def write_lists(cat_dir, stages, prefix="new_"):
    """stages: {"train": [scan names], ...} -> <cat_dir>/<prefix><stage>.lst"""
    os.makedirs(cat_dir, exist_ok=True)
    for stage, names in stages.items():
        with open(os.path.join(cat_dir, prefix + stage + ".lst"), "w") as f:
            f.write("\n".join(names) + "\n")


def boxed_scan_images(NV, H, W, seed, margin=1):
    """(images (NV, H, W, 3), masks (NV, H, W) uint8 0 / 255, boxes): data_trees.boxed_views with one box per view."""
    boxes = [(margin + v % 2, margin, W - 1 - margin, H - 1 - margin - v % 2) for v in range(NV)]
    images = dt.boxed_views(NV, H, W, boxes, seed)
    masks = np.zeros((NV, H, W), np.uint8)
    for v, (cmin, rmin, cmax, rmax) in enumerate(boxes):
        masks[v, rmin:rmax + 1, cmin:cmax + 1] = 255
    return images, masks, boxes
