"""A data source that needs no files: objects made of a few ellipsoids and boxes, ray-cast on the device (util.synth_render,
pnr_synth_render) into items of SRNDataset's form — images, masks, boxes, poses, and the ground-truth depth on request.

The scene records are data (include/pnr.h lays them out); random_scenes draws them, and a hand-written table is equally valid
input of util.synth_render.  The reference's own data step runs Blender over ShapeNet meshes; nothing of it is restated here."""
import os

import numpy as np
import torch

from .. import util
from . import _items

MAX_PRIMS = 8                 # PNR_SYNTH_MAX_PRIMS
REC = 20                      # PNR_SYNTH_REC: kind, centre (3), world -> local rotation (9), half-extents (3), albedo (3), pad
KIND_NONE, KIND_ELLIPSOID, KIND_BOX = 0, 1, 2
STAGE_CODES = {"train": 0, "val": 1, "test": 2}
H_MIN, H_MAX = 0.08, 0.22     # half-extents: sqrt(3) * H_MAX < 0.5, and H_MIN stays wider than a sub-sample at 16 x 16
Z_NEAR, Z_FAR = 0.8, 1.8      # the SRN cars numbers, which pair with cameras at radius 1.3 around the ball of radius 0.5


def _stage_code(stage):
    if stage not in STAGE_CODES:
        raise ValueError(f"stage must be one of {sorted(STAGE_CODES)}, got {stage!r}")
    return STAGE_CODES[stage]


def _seed(seed):
    seed = int(seed)
    if seed < 0:
        raise ValueError(f"seed must not be negative, got {seed}")
    return seed


def _rotation(rng):
    """A rotation matrix uniform over SO(3), float64: that of a normalised 4-d normal draw read as a quaternion."""
    q = rng.standard_normal(4)
    r, i, j, k = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r)],
                     [2 * (i * j + k * r), 1 - 2 * (i * i + k * k), 2 * (j * k - i * r)],
                     [2 * (i * k - j * r), 2 * (j * k + i * r), 1 - 2 * (i * i + j * j)]])


def random_scenes(n, seed, stage="train", max_prims=4):
    """float32 (n, max_prims, REC): object i of a stage, drawn by np.random.default_rng([seed, stage code, i]) alone, so it does
    not depend on n and the stages share no object.  An object has 1 .. max_prims primitives (the remaining records are kind 0),
    each an ellipsoid or a box with half-extents in [0.08, 0.22], a uniform rotation, a centre such that |centre| +
    |half-extents| <= 0.5 (the whole primitive inside the ball of radius 0.5) and albedo components in [0.1, 0.9]."""
    n, P, seed, code = int(n), int(max_prims), _seed(seed), _stage_code(stage)
    if n < 0 or not 1 <= P <= MAX_PRIMS:
        raise ValueError(f"n must not be negative and max_prims must lie in 1..{MAX_PRIMS}, got n = {n}, max_prims = {P}")
    out = np.zeros((n, P, REC), dtype=np.float32)
    for i in range(n):
        rng = np.random.default_rng([seed, code, i])
        for p in range(int(rng.integers(1, P + 1))):
            rec = out[i, p]
            rec[0] = rng.integers(KIND_ELLIPSOID, KIND_BOX + 1)
            h = rng.uniform(H_MIN, H_MAX, 3)
            direction = rng.standard_normal(3)
            radius = rng.uniform() ** (1.0 / 3.0) * 0.999 * (0.5 - np.linalg.norm(h))     # uniform over the ball it may lie in
            rec[1:4] = direction / np.linalg.norm(direction) * radius
            rec[4:13] = _rotation(rng).reshape(9)
            rec[13:16] = h
            rec[16:19] = np.clip(rng.uniform(0.1, 0.9, 3).astype(np.float32), np.float32(0.1), np.float32(0.9))
    return out


def _look_at_origin(position):
    """float64 (4, 4) camera-to-world of a camera at `position` that looks at the origin, in util.gen_rays' convention: x right,
    y up, the camera looks down -z; the world's z is up (the world's y for a camera on the z axis)."""
    back = position / np.linalg.norm(position)
    up = np.array([0.0, 0.0, 1.0]) if abs(back[2]) < 0.999 else np.array([0.0, 1.0, 0.0])
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(back, right), back, position
    return pose


def view_poses(n_views, seed, stage, i, radius=1.3):
    """float32 (n_views, 4, 4) camera-to-world matrices of object i's views, in the convention util.gen_rays takes: cameras on
    the sphere of `radius` that look at the origin.  train / val: uniform on the sphere, drawn by
    np.random.default_rng([seed, stage code, i, 1]); test: a deterministic spiral of three turns that climbs from 10 to 60
    degrees of elevation, the same for every object and seed."""
    n_views, seed, code, i = int(n_views), _seed(seed), _stage_code(stage), int(i)
    if stage == "test":
        t = (np.arange(n_views) + 0.5) / max(n_views, 1)
        elev, azim = np.radians(10.0 + 50.0 * t), 2.0 * np.pi * 3.0 * t
        pos = np.stack((np.cos(elev) * np.cos(azim), np.cos(elev) * np.sin(azim), np.sin(elev)), axis=-1)
    else:
        pos = np.random.default_rng([seed, code, i, 1]).standard_normal((n_views, 3))
        pos /= np.linalg.norm(pos, axis=-1, keepdims=True)
    poses = np.stack([_look_at_origin(p * float(radius)) for p in pos]) if n_views else np.zeros((0, 4, 4))
    return poses.astype(np.float32)


class SyntheticShapes(torch.utils.data.Dataset):
    """n_objects procedural objects of one stage, n_views views each, rendered when an item is asked for.

    Item: SRNDataset's — {"path": "synthetic/<stage>/<index, six digits>", "img_id", "focal" (a float, 131.25 * image_size / 128:
    the ball of radius 0.5 projects inside the frame), "c" float32 (image_size / 2 twice), "images", "masks", "bbox" (NV, 4)
    float32, "poses" (NV, 4, 4) float32}, all on the host; as_bytes=True: images uint8 (NV, H, W, 3) and masks uint8
    (NV, H, W) exactly as the kernel wrote them; else _items.images_to_float of those bytes and float masks (NV, 1, H, W).
    want_depth adds "depth" (NV, H, W) float32, the ray parameter at each pixel's first sub-sample, +inf on the background.
    Attributes: z_near, z_far = 0.8, 1.8; lindisp = False; balanced; as_bytes.

    __getitem__ launches on `device` and copies back, so it touches the device: use it with num_workers=0 (which is what
    Trainer's loaders use), never in forked workers.  The same arguments give the same items, bit for bit."""

    def __init__(self, n_objects, n_views=50, image_size=128, seed=0, stage="train", as_bytes=False, balanced=True, device="cuda",
                 ss=2, max_prims=4, want_depth=False):
        super().__init__()
        self.n_views, self.image_size, self.seed, self.stage = int(n_views), int(image_size), _seed(seed), stage
        if self.n_views < 1 or self.image_size < 1:
            raise ValueError(f"n_views and image_size must be positive, got {n_views}, {image_size}")
        if ss not in (1, 2, 4):
            raise ValueError(f"ss must be 1, 2 or 4, got {ss}")
        self.scenes = torch.from_numpy(random_scenes(n_objects, seed, stage, max_prims))
        self.device = torch.device(device)
        self.as_bytes, self.balanced, self.ss, self.want_depth = bool(as_bytes), bool(balanced), int(ss), bool(want_depth)
        self.focal = 131.25 * self.image_size / 128.0
        self.z_near, self.z_far = Z_NEAR, Z_FAR
        self.lindisp = False
        self._scenes_dev = None

    def __len__(self):
        return int(self.scenes.shape[0])

    def __getitem__(self, index):
        index = int(index)
        if not 0 <= index < len(self):
            raise IndexError(f"object index {index} outside [0, {len(self)})")
        if self._scenes_dev is None:
            self._scenes_dev = util.upload(self.scenes, self.device)
        S, NV = self.image_size, self.n_views
        poses = torch.from_numpy(view_poses(NV, self.seed, self.stage, index))
        ids = torch.full((NV,), index, dtype=torch.int32)
        rgb, mask, depth = util.synth_render(self._scenes_dev, util.upload(ids, self.device), util.upload(poses, self.device), S, S,
                                             self.focal, ss=self.ss, mask_out=True, depth_out=True if self.want_depth else None)
        images, masks = rgb.cpu(), mask.cpu()
        path = f"synthetic/{self.stage}/{index:06d}"
        bbox = np.stack([_items.mask_bbox(m, f"{path} view {v}") for v, m in enumerate(masks.numpy() != 0)])
        if not self.as_bytes:
            images, masks = _items.images_to_float(images, self.balanced), (masks != 0)[:, None].float()
        item = {"path": path, "img_id": index, "focal": self.focal, "c": torch.tensor([S * 0.5, S * 0.5], dtype=torch.float32),
                "images": images, "masks": masks, "bbox": torch.from_numpy(bbox), "poses": poses}
        if self.want_depth:
            item["depth"] = depth.cpu()
        return item


def split(want_split="all", n_objects=None, n_val=None, n_test=None, **kwargs):
    """get_split_dataset's "synthetic": one stage or the (train, val, test) triple.  n_objects counts the train stage; val and
    test default to max(1, n_objects // 8) objects.  kwargs go to SyntheticShapes."""
    if n_objects is None:
        raise ValueError("dataset type 'synthetic' needs n_objects")
    small = max(1, int(n_objects) // 8)
    counts = {"train": int(n_objects), "val": small if n_val is None else int(n_val), "test": small if n_test is None else int(n_test)}
    kwargs.pop("stage", None)
    if want_split in counts:
        return SyntheticShapes(counts[want_split], stage=want_split, **kwargs)
    return tuple(SyntheticShapes(counts[stage], stage=stage, **kwargs) for stage in ("train", "val", "test"))


def write_srn_tree(items, path, stage):
    """Writes byte items (a dataset built with as_bytes=True, or any iterable of such items) as the SRN layout SRNDataset reads:
    <path>_<stage>/<object>/{intrinsics.txt, rgb/%06d.png, pose/%06d.txt}, <object> the last component of the item's "path".
    intrinsics.txt: "focal cx cy 0." first and "height width" last; a pose file: the 16 numbers of pose @ diag(1, -1, -1, 1)
    with %.9g, which SRNDataset multiplies back, so it reads the same floats, bytes, masks and boxes.  -> the stage's folder."""
    from PIL import Image
    root = path + "_" + stage
    flip = np.array([1.0, -1.0, -1.0, 1.0], dtype=np.float32)
    for item in items:            # a dataset without __iter__ is walked by index until its IndexError
        images = item["images"]
        if not torch.is_tensor(images) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError("write_srn_tree needs byte items: images uint8 (NV, H, W, 3), a dataset built with as_bytes=True")
        NV, H, W, _ = (int(s) for s in images.shape)
        obj = os.path.join(root, os.path.basename(str(item["path"])))
        os.makedirs(os.path.join(obj, "rgb"), exist_ok=True)
        os.makedirs(os.path.join(obj, "pose"), exist_ok=True)
        cx, cy = (float(v) for v in item["c"])
        with open(os.path.join(obj, "intrinsics.txt"), "w") as f:
            f.write(f"{float(item['focal']):.17g} {cx:.17g} {cy:.17g} 0.\n0. 0. 0.\n1.\n{H} {W}\n")
        for v in range(NV):
            Image.fromarray(images[v].numpy()).save(os.path.join(obj, "rgb", f"{v:06d}.png"))
            pose = item["poses"][v].numpy().astype(np.float32) * flip[None, :]
            with open(os.path.join(obj, "pose", f"{v:06d}.txt"), "w") as f:
                f.write(" ".join(f"{x:.9g}" for x in pose.reshape(-1)) + "\n")
    return root
