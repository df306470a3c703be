"""A whole split on the card: the images as the bytes their files hold, so a training step uploads only its indices."""
import torch

from .. import util


class ResidentSplit:
    """Loads every object of an as_bytes dataset ONCE and keeps one device pool of bytes (N, NV, H, W, 3), one of poses
    (N, NV, 4, 4), and the boxes and intrinsics on the host (they steer host-side draws).  A whole SRN or NMR training split is
    under 10 GB this way.  Refuses a dataset whose objects differ in NV, H or W, and a pool above max_bytes (checked before
    anything is allocated).

    batch(ids) returns the loader's dict for train.calc_losses — device bytes and poses gathered by pool[ids], host bbox /
    focal / c — and batches() iterates an epoch of them.  Neither reads anything back from the device.  z_near, z_far, lindisp
    and balanced are the dataset's.

    device_boxes=True also keeps the boxes on the card, float32 (N, NV, 4), and batch() adds "bbox_dev", their rows gathered
    on the device: what train.make_batch(draws="device") draws inside without an upload.  With the default the dict is
    unchanged.

    A dataset whose items carry no "bbox" (DTUDataset on scans without masks) is taken too: self.bbox is None and batch() has
    no "bbox" key, so the draws cover the whole image; device_boxes=True on such a dataset raises ValueError.

    image_size=(Ht, Wt) (or an int) other than the items' own size builds the pool at that size, (N, NV, Ht, Wt, 3): each
    object's bytes are uploaded to ONE reused staging buffer and util.resize_area_u8 (area resampling, the exact window mean
    rounded to the nearest byte) writes them into the object's slot; max_bytes is judged on the resized pool; the boxes come
    through util.resize_bbox and focal / c through util.resize_intrinsics (both differ from upstream's float scaling on
    purpose: see there).  batch() and batches() keep their form.  With None or the items' own size nothing changes, not a
    bit.  data.ResizedDataset gives evaluation and validation the same resolution.

    device_masks=True also keeps each object's mask on the card as the bit table of util.mask_table, built while the pool is
    filled: mask_bits (N, NV * H, ceil(W / 32)) and mask_rows (N, NV * H + 1), int32, and batch() adds "mask_bits" and
    "mask_rows", their rows gathered on the device: what train.make_batch(draws="device", prop_inside=...) draws from without an
    upload.  The items' "masks" are uint8 (NV, H, W), inside at >= 128; with image_size they go through util.resize_area_u8
    first, so a target pixel is inside iff its window's mean is >= 127.5 (the resize rounds a tie up).  A dataset without
    "masks" raises ValueError; max_bytes is judged on pool + tables.  With the default nothing changes."""

    def __init__(self, dataset, device, max_bytes=None, device_boxes=False, image_size=None, device_masks=False):
        if not getattr(dataset, "as_bytes", False):
            raise ValueError("ResidentSplit needs a dataset built with as_bytes=True")
        N = len(dataset)
        if N == 0:
            raise ValueError("ResidentSplit needs at least one object")
        self.device = torch.device(device)
        self.balanced = bool(getattr(dataset, "balanced", True))
        for name in ("z_near", "z_far", "lindisp"):
            setattr(self, name, getattr(dataset, name, None))
        self.paths, bbox, focal, c = [], [], [], []
        for i in range(N):
            item = dataset[i]
            images = item["images"]
            if i == 0:
                NV, H, W, C = (int(s) for s in images.shape)
                Ht, Wt = (H, W) if image_size is None else util._target_size(image_size)
                if min(Ht, Wt) < 1:
                    raise ValueError(f"image_size must be positive, got {(Ht, Wt)}")
                resized = (Ht, Wt) != (H, W)
                nbytes = N * NV * Ht * Wt * C
                if device_masks:
                    R, Wd = NV * Ht, (Wt + 31) // 32
                    nbytes += 4 * N * (R * Wd + R + 1)
                if max_bytes is not None and nbytes > max_bytes:
                    raise ValueError(f"the split needs a pool of {nbytes} bytes, above max_bytes = {max_bytes}")
                self.images = torch.empty(N, NV, Ht, Wt, C, dtype=torch.uint8, device=self.device)
                self.poses = torch.empty(N, NV, 4, 4, dtype=torch.float32, device=self.device)
                staging = torch.empty(NV, H, W, C, dtype=torch.uint8, device=self.device) if resized else None
                if device_masks:
                    self.mask_bits = torch.empty(N, R, Wd, dtype=torch.int32, device=self.device)
                    self.mask_rows = torch.empty(N, R + 1, dtype=torch.int32, device=self.device)
                    mask_staging = torch.empty(NV, H, W, 1, dtype=torch.uint8, device=self.device)
            elif tuple(images.shape) != (NV, H, W, C):
                raise ValueError(f"{item['path']}: images {tuple(images.shape)}, the objects before it {(NV, H, W, C)}; "
                                 "a resident pool needs one shape")
            if resized:
                staging.copy_(images)       # stream order: the resize of the object before it has read the buffer by then
                util.resize_area_u8(staging, (Ht, Wt), out=self.images[i])
            else:
                self.images[i].copy_(images)
            if device_masks:
                masks = item.get("masks")
                if masks is None or masks.dtype != torch.uint8 or tuple(masks.shape) != (NV, H, W):
                    raise ValueError(f"{item['path']}: device_masks=True needs 'masks' as uint8 {(NV, H, W)}, got "
                                     f"{None if masks is None else (masks.dtype, tuple(masks.shape))}")
                mask_staging.copy_(masks[..., None])
                small = util.resize_area_u8(mask_staging, (Ht, Wt)) if resized else mask_staging
                util.mask_table(small[..., 0], out=(self.mask_bits[i:i + 1], self.mask_rows[i:i + 1]))
            self.poses[i].copy_(item["poses"])
            self.paths.append(item["path"])
            if i > 0 and ("bbox" in item) != bool(bbox):
                raise ValueError(f"{item['path']}: {'' if 'bbox' in item else 'no '}boxes, unlike the objects before it")
            item_focal, item_c = torch.as_tensor(item["focal"], dtype=torch.float32), item.get("c")
            if resized:
                item_focal, item_c = util.resize_intrinsics(item_focal, item_c, (H, W), (Ht, Wt))
            if "bbox" in item:
                bbox.append(util.resize_bbox(item["bbox"], (H, W), (Ht, Wt)) if resized else item["bbox"])
            focal.append(item_focal)
            c.append(item_c)
        if device_boxes and not bbox:
            raise ValueError("device_boxes=True needs a dataset whose items have a 'bbox'")
        self.bbox = torch.stack(bbox) if bbox else None
        self.focal = torch.stack(focal)
        self.c = None if c[0] is None else torch.stack(c)
        self.bbox_dev = util.upload(self.bbox.to(torch.float32).contiguous(), self.device) if device_boxes else None
        self.image_size = (Ht, Wt)
        if not device_masks:
            self.mask_bits = self.mask_rows = None

    def __len__(self):
        return len(self.paths)

    @property
    def nbytes(self):
        tables = 0 if self.mask_bits is None else 4 * (self.mask_bits.numel() + self.mask_rows.numel())
        return self.images.numel() + tables

    def batch(self, ids):
        """ids: object indices (a sequence or a host int tensor) -> {"path", "img_id", "images" (SB, NV, H, W, 3) uint8 and
        "poses" on the device, "bbox" and "c" (when the dataset has them) and "focal" on the host}."""
        ids = torch.as_tensor(ids, dtype=torch.long).reshape(-1)
        if ids.is_cuda:
            raise ValueError("ids must be host indices: they also select the host-side boxes and intrinsics")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= len(self)):
            raise IndexError(f"object index outside [0, {len(self)})")
        on_dev = util.upload(ids, self.device)
        data = {"path": [self.paths[i] for i in ids.tolist()], "img_id": ids, "images": self.images[on_dev],
                "poses": self.poses[on_dev]}
        if self.bbox is not None:
            data["bbox"] = self.bbox[ids]
        data["focal"] = self.focal[ids]
        if self.c is not None:
            data["c"] = self.c[ids]
        if self.bbox_dev is not None:
            data["bbox_dev"] = self.bbox_dev[on_dev]
        if self.mask_bits is not None:
            data["mask_bits"], data["mask_rows"] = self.mask_bits[on_dev], self.mask_rows[on_dev]
        return data

    def batches(self, batch_size, shuffle=True, generator=None, drop_last=True):
        """One epoch: batch() over a permutation (torch.randperm under `generator`) or over the objects in order."""
        N = len(self)
        order = torch.randperm(N, generator=generator) if shuffle else torch.arange(N)
        stop = N - N % batch_size if drop_last else N
        for first in range(0, stop, batch_size):
            yield self.batch(order[first:first + batch_size])
