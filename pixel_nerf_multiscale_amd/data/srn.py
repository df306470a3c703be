"""SRN cars / chairs (Sitzmann et al.'s ShapeNet renders), the layout upstream pixelNeRF's SRNDataset reads."""
import glob
import os

import numpy as np
import torch

from . import _items


class SRNDataset(torch.utils.data.Dataset):
    """<path>_<stage>/<object>/{intrinsics.txt, rgb/*, pose/*}.

    The root is path + "_" + stage; with "chair" in the basename of `path`, stage "train" and an existing sub-folder
    "chairs_2.0_train" of it, that sub-folder.  Objects are the sorted */intrinsics.txt.  intrinsics.txt: first line
    "focal cx cy _", last line "height width".  Views are the sorted rgb/* paired with the sorted pose/*; a pose file holds 16
    numbers, the row-major 4 x 4 camera-to-world matrix in the OpenCV convention, which is multiplied from the right by
    diag(1, -1, -1, 1).  world_scale != 1 scales the focal length and the translations.  A pixel is background when ANY of its
    channels is 255: mask = (img != 255).all(-1).

    Item: {"path": object folder, "img_id": index, "focal": float, "c": float32 (cx, cy), "images", "masks",
    "bbox" (NV, 4) float32 = cmin, rmin, cmax, rmax, "poses" (NV, 4, 4) float32}; images / masks as the package docstring says
    for as_bytes.  Attributes: z_near, z_far = 1.25, 2.75 for chairs, else 0.8, 1.8; lindisp = False; balanced."""

    def __init__(self, path, stage="train", image_size=None, world_scale=1.0, balanced=True, as_bytes=False):
        super().__init__()
        self.base_path = path + "_" + stage
        self.dataset_name = os.path.basename(path)
        if not os.path.isdir(self.base_path):
            raise FileNotFoundError(f"SRN dataset folder {self.base_path} does not exist")
        is_chair = "chair" in self.dataset_name
        if is_chair and stage == "train":
            tmp = os.path.join(self.base_path, "chairs_2.0_train")
            if os.path.isdir(tmp):
                self.base_path = tmp
        self.stage = stage
        self.intrins = sorted(glob.glob(os.path.join(self.base_path, "*", "intrinsics.txt")))
        self.image_size = image_size
        self.world_scale = float(world_scale)
        self.balanced = bool(balanced)
        self.as_bytes = bool(as_bytes)
        self._coord_trans = np.diag(np.array([1, -1, -1, 1], dtype=np.float32))
        self.z_near, self.z_far = (1.25, 2.75) if is_chair else (0.8, 1.8)
        self.lindisp = False

    def __len__(self):
        return len(self.intrins)

    def __getitem__(self, index):
        intrin_path = self.intrins[index]
        dir_path = os.path.dirname(intrin_path)
        rgb_paths = sorted(glob.glob(os.path.join(dir_path, "rgb", "*")))
        pose_paths = sorted(glob.glob(os.path.join(dir_path, "pose", "*")))
        if len(rgb_paths) != len(pose_paths):
            raise RuntimeError(f"{dir_path}: {len(rgb_paths)} images but {len(pose_paths)} poses")
        with open(intrin_path, "r") as f:
            lines = f.readlines()
        focal, cx, cy, _ = map(float, lines[0].split())
        height, width = map(int, lines[-1].split())

        images, masks, bboxes, poses = [], [], [], []
        for rgb_path, pose_path in zip(rgb_paths, pose_paths):
            img = _items.read_rgb(rgb_path)
            if img.shape[:2] != (height, width):
                raise RuntimeError(f"{rgb_path}: {img.shape[:2]} pixels, intrinsics.txt says {(height, width)}")
            _items.check_image_size(self.image_size, height, width, rgb_path)
            mask = (img != 255).all(axis=-1)
            bboxes.append(_items.mask_bbox(mask, rgb_path))
            pose = np.loadtxt(pose_path, dtype=np.float32).reshape(4, 4)
            poses.append(pose @ self._coord_trans)
            images.append(img)
            masks.append(mask)

        poses = torch.from_numpy(np.stack(poses))
        if self.world_scale != 1.0:
            focal *= self.world_scale
            poses[:, :3, 3] *= self.world_scale
        images, masks = _items.pack_views(images, masks, self.as_bytes, self.balanced)
        return {"path": dir_path, "img_id": index, "focal": focal, "c": torch.tensor([cx, cy], dtype=torch.float32),
                "images": images, "masks": masks, "bbox": torch.from_numpy(np.stack(bboxes)), "poses": poses}
