"""The DTU sub-format of DVR (Niemeyer et al.): scans with full projection matrices, what upstream pixelNeRF trains its
real-image model on (DVRDataset(sub_format="dtu")), and ColorJitter, the record of the augmentation it trains DTU with."""
import glob
import os

import numpy as np
import torch

from . import _items


class ColorJitter:
    """The four ranges of the colour-jitter augmentation (upstream's ColorJitterDataset defaults as remembered): one
    brightness / contrast / saturation factor in [1 - range, 1 + range] and one hue shift in [-hue, hue] per object and step.
    A plain record: train.make_batch(jitter=...) hands it to util.color_jitter_plan, which draws on the device."""

    def __init__(self, brightness=0.15, contrast=0.15, saturation=0.15, hue=0.15):
        self.brightness, self.contrast, self.saturation, self.hue = float(brightness), float(contrast), float(saturation), float(hue)

    @property
    def ranges(self):
        return (self.brightness, self.contrast, self.saturation, self.hue)

    def __repr__(self):
        return "ColorJitter(brightness={}, contrast={}, saturation={}, hue={})".format(*self.ranges)


def rq3(M):
    """M (3, 3) float64, det > 0 -> (K, R): M = K R, K upper triangular with a positive diagonal, R a rotation.  numpy's QR on
    the flipped transpose, the signs fixed afterwards."""
    flip = np.eye(3)[::-1]
    Q, U = np.linalg.qr((flip @ M).T)
    K, R = flip @ U.T @ flip, flip @ Q.T
    sign = np.diag(np.where(np.diag(K) < 0.0, -1.0, 1.0))
    return K @ sign, sign @ R


def decompose_projection(P):
    """P (3, 4) float64 -> (K, pose): K = intrinsics with K[2, 2] = 1, pose = [[R^T, C], [0, 1]] (camera to world, the
    camera's axes as the matrix has them).  P and -P are the same camera: the sign that makes det(P[:, :3]) positive is taken.
    ValueError for a singular P[:, :3] (a camera at infinity)."""
    P = np.asarray(P, dtype=np.float64)
    M = P[:, :3]
    det = np.linalg.det(M)
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("the projection matrix's left 3 x 3 block is singular: it has no camera centre")
    if det < 0.0:
        P, M = -P, -M
    K, R = rq3(M)
    pose = np.eye(4)
    pose[:3, :3] = R.T
    pose[:3, 3] = -np.linalg.solve(M, P[:, 3])
    return K / K[2, 2], pose


class DTUDataset(torch.utils.data.Dataset):
    """<path>/<category>/{<list_prefix><stage>.lst, <scan>/{image/*, [mask/*], cameras.npz}}, list_prefix "new_".

    PARITY UNPINNED.  The recipe follows upstream's DVRDataset(sub_format="dtu") as remembered; neither upstream's data package
    nor cv2 (whose decomposeProjectionMatrix upstream calls) is available where this package is developed, so the layout and
    the formulas below are the specification.

    Categories, lists and all_objs as in DVRDataset.  Views are the sorted image/*.  With as many mask/* as image/*, masks and
    bbox are made as DVRDataset makes them; with mask/ absent or empty the item has neither key; any other count raises
    RuntimeError.

    Cameras, all in float64 and stored as float32: P = world_mat_i[:3], or -P if det(P[:, :3]) < 0 (ValueError if it is 0);
    P[:, :3] = K R with K upper triangular, positive diagonal, and R a rotation (an RQ decomposition); K /= K[2, 2]; the camera
    centre C = -P[:, :3]^-1 P[:, 3]; pose = [[R^T, C], [0, 1]]; with scale_mat_i present pose[:3, 3] = (pose[:3, 3] -
    scale_mat_i[:3, 3]) / diag(scale_mat_i[:3, :3]); then pose = D @ pose @ D, D = diag(1, -1, -1, 1).  focal = the means over
    the item's views of (K[0, 0], K[1, 1]), c of (K[0, 2], K[1, 2]).  An object with more than max_imgs views yields a random
    subset of them (numpy's global generator), each with its own camera.

    Item: {"path", "img_id", "focal" (2,), "c" (2,), "images", "poses"[, "masks", "bbox"]}.  Attributes: z_near, z_far,
    lindisp = False, balanced."""

    def __init__(self, path, stage="train", list_prefix="new_", max_imgs=100000, z_near=0.1, z_far=5.0, balanced=True,
                 as_bytes=False, image_size=None):
        super().__init__()
        self.base_path = path
        if not os.path.isdir(self.base_path):
            raise FileNotFoundError(f"DTU dataset folder {self.base_path} does not exist")
        self.stage = stage
        all_objs = []
        for cat_dir in sorted(d for d in glob.glob(os.path.join(path, "*")) if os.path.isdir(d)):
            list_path = os.path.join(cat_dir, list_prefix + stage + ".lst")
            if not os.path.exists(list_path):
                continue
            cat = os.path.basename(cat_dir)
            with open(list_path, "r") as f:
                all_objs.extend((cat, os.path.join(cat_dir, line.strip())) for line in f if line.strip())
        self.all_objs = all_objs
        self.image_size = image_size
        self.max_imgs = int(max_imgs)
        self.balanced = bool(balanced)
        self.as_bytes = bool(as_bytes)
        self.z_near, self.z_far = z_near, z_far
        self.lindisp = False

    def __len__(self):
        return len(self.all_objs)

    def __getitem__(self, index):
        cat, root_dir = self.all_objs[index]
        rgb_paths = sorted(glob.glob(os.path.join(root_dir, "image", "*")))
        mask_paths = sorted(glob.glob(os.path.join(root_dir, "mask", "*")))
        if mask_paths and len(mask_paths) != len(rgb_paths):
            raise RuntimeError(f"{root_dir}: {len(rgb_paths)} images but {len(mask_paths)} masks")
        if len(rgb_paths) <= self.max_imgs:
            sel_indices = np.arange(len(rgb_paths))
        else:
            sel_indices = np.random.choice(len(rgb_paths), self.max_imgs, replace=False)
            rgb_paths = [rgb_paths[i] for i in sel_indices]
            mask_paths = [mask_paths[i] for i in sel_indices] if mask_paths else []
        cams = np.load(os.path.join(root_dir, "cameras.npz"))
        flip = np.diag([1.0, -1.0, -1.0, 1.0])

        images, masks, bboxes, poses, Ks = [], [], [], [], []
        for n, (i, rgb_path) in enumerate(zip(sel_indices, rgb_paths)):
            img = _items.read_rgb(rgb_path)
            H, W = img.shape[:2]
            _items.check_image_size(self.image_size, H, W, rgb_path)
            if mask_paths:
                mask = _items.read_u8(mask_paths[n])
                if mask.ndim == 3:
                    mask = mask[..., 0]
                mask = mask != 0
                if mask.shape != (H, W):
                    raise RuntimeError(f"{mask_paths[n]}: {mask.shape} pixels, the image has {(H, W)}")
                bboxes.append(_items.mask_bbox(mask, mask_paths[n]))
                masks.append(mask)
            try:
                K, pose = decompose_projection(np.asarray(cams["world_mat_" + str(i)], dtype=np.float64)[:3])
            except ValueError as e:
                raise ValueError(f"{root_dir}: world_mat_{i}: {e}") from None
            scale_key = "scale_mat_" + str(i)
            if scale_key in cams:
                scale = np.asarray(cams[scale_key], dtype=np.float64)
                pose[:3, 3] = (pose[:3, 3] - scale[:3, 3]) / np.diagonal(scale)[:3]
            poses.append(torch.tensor(flip @ pose @ flip, dtype=torch.float32))
            Ks.append(K)
            images.append(img)

        K = np.mean(np.stack(Ks), axis=0)
        item = {"path": root_dir, "img_id": index, "focal": torch.tensor([K[0, 0], K[1, 1]], dtype=torch.float32),
                "c": torch.tensor([K[0, 2], K[1, 2]], dtype=torch.float32), "poses": torch.stack(poses)}
        if mask_paths:
            item["images"], item["masks"] = _items.pack_views(images, masks, self.as_bytes, self.balanced)
            item["bbox"] = torch.from_numpy(np.stack(bboxes))
        else:
            images = torch.from_numpy(np.stack(images))
            item["images"] = images if self.as_bytes else _items.images_to_float(images, self.balanced)
        return item
