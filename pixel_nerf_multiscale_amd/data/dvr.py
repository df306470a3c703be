"""The ShapeNet sub-format of DVR (Niemeyer et al.) / NMR renders, the layout upstream pixelNeRF's DVRDataset reads."""
import glob
import os

import numpy as np
import torch

from . import _items


class DVRDataset(torch.utils.data.Dataset):
    """<path>/<category>/{<list_prefix><stage>.lst, <object>/{image/*, mask/*, cameras.npz}}.

    Categories are the sub-folders of `path` (sorted); a category's objects are the lines of its list file, and a category
    without that list is skipped.  all_objs holds (category, object folder) pairs in that order.  Views are the sorted image/*;
    masks the sorted mask/*, first channel, non-zero = foreground.  cameras.npz: the pose of view i is world_mat_inv_i when
    present, else the inverse of world_mat_i (a 3 x 4 matrix is extended by the row 0 0 0 1); camera_mat_i[0, 0] must equal
    [1, 1]; fx = camera_mat_i[0, 0] * W / 2 with scale_focal and must be one value over the object; pose = Tw @ pose @ Tc with
    Tw = [[1,0,0,0],[0,0,-1,0],[0,1,0,0],[0,0,0,1]] and Tc = diag(1, -1, -1, 1).  An object with more than max_imgs views
    yields a random subset of them (numpy's global generator).  The DTU sub-format is DTUDataset's (data/dtu.py).

    Item: {"path", "img_id", "focal": 0-dim float32 tensor, "images", "masks", "bbox", "poses"}; there is no "c" (the
    principal point is the image centre).  Attributes: z_near, z_far, lindisp = False, balanced."""

    def __init__(self, path, stage="train", list_prefix="softras_", max_imgs=100000, z_near=1.2, z_far=4.0, scale_focal=True,
                 balanced=True, as_bytes=False, image_size=None):
        super().__init__()
        self.base_path = path
        if not os.path.isdir(self.base_path):
            raise FileNotFoundError(f"DVR dataset folder {self.base_path} does not exist")
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
        self.scale_focal = bool(scale_focal)
        self.balanced = bool(balanced)
        self.as_bytes = bool(as_bytes)
        self._coord_trans_world = torch.tensor([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], dtype=torch.float32)
        self._coord_trans_cam = torch.tensor([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], dtype=torch.float32)
        self.z_near, self.z_far = z_near, z_far
        self.lindisp = False

    def __len__(self):
        return len(self.all_objs)

    def __getitem__(self, index):
        cat, root_dir = self.all_objs[index]
        rgb_paths = sorted(glob.glob(os.path.join(root_dir, "image", "*")))
        mask_paths = sorted(glob.glob(os.path.join(root_dir, "mask", "*")))
        if len(mask_paths) != len(rgb_paths):
            raise RuntimeError(f"{root_dir}: {len(rgb_paths)} images but {len(mask_paths)} masks")
        if len(rgb_paths) <= self.max_imgs:
            sel_indices = np.arange(len(rgb_paths))
        else:
            sel_indices = np.random.choice(len(rgb_paths), self.max_imgs, replace=False)
            rgb_paths = [rgb_paths[i] for i in sel_indices]
            mask_paths = [mask_paths[i] for i in sel_indices]
        cams = np.load(os.path.join(root_dir, "cameras.npz"))

        images, masks, bboxes, poses, focal = [], [], [], [], None
        for i, rgb_path, mask_path in zip(sel_indices, rgb_paths, mask_paths):
            img = _items.read_rgb(rgb_path)
            H, W = img.shape[:2]
            _items.check_image_size(self.image_size, H, W, rgb_path)
            mask = _items.read_u8(mask_path)
            if mask.ndim == 3:
                mask = mask[..., 0]
            mask = mask != 0
            if mask.shape != (H, W):
                raise RuntimeError(f"{mask_path}: {mask.shape} pixels, the image has {(H, W)}")
            bboxes.append(_items.mask_bbox(mask, mask_path))

            inv_key = "world_mat_inv_" + str(i)
            if inv_key in cams:
                pose = cams[inv_key]
            else:
                wmat = cams["world_mat_" + str(i)]
                if wmat.shape[0] == 3:
                    wmat = np.vstack((wmat, np.array([0, 0, 0, 1], dtype=wmat.dtype)))
                pose = np.linalg.inv(wmat)
            K = cams["camera_mat_" + str(i)]
            if K[0, 0] != K[1, 1]:
                raise ValueError(f"{root_dir}: camera_mat_{i} has fx {K[0, 0]} != fy {K[1, 1]}; one focal length per object")
            fx = torch.tensor(K[0, 0] * (W / 2.0) if self.scale_focal else K[0, 0], dtype=torch.float32)
            if focal is None:
                focal = fx
            elif float(focal) != float(fx):
                raise ValueError(f"{root_dir}: view {i} has focal length {float(fx)}, the views before it {float(focal)}")
            pose = self._coord_trans_world @ torch.tensor(pose, dtype=torch.float32) @ self._coord_trans_cam
            poses.append(pose)
            images.append(img)
            masks.append(mask)

        images, masks = _items.pack_views(images, masks, self.as_bytes, self.balanced)
        return {"path": root_dir, "img_id": index, "focal": focal, "images": images, "masks": masks,
                "bbox": torch.from_numpy(np.stack(bboxes)), "poses": torch.stack(poses)}
