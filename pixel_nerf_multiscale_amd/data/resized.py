"""A dataset at another image_size: every item resampled on the device when it is asked for."""
import torch

from .. import util


class ResizedDataset(torch.utils.data.Dataset):
    """dataset[i] at image_size = (Ht, Wt) (or an int): the same keys, dtypes and host placement, with
      images  uint8 (NV, H, W, 3)   -> util.resize_area_u8: the exact window mean, rounded to the nearest byte
              float32 (NV, 3, H, W) -> util.resize_area: the window mean in fp64, rounded to fp32 once
      masks   uint8 (NV, H, W): the one-channel case of the bytes; float32 (NV, 1, H, W): the float path, so a float mask
              becomes fractional where a window holds both kinds of pixel, as upstream pixelNeRF's does
      bbox    util.resize_bbox (integer arithmetic; the box of "any source pixel under the window is foreground")
      focal, c  util.resize_intrinsics (sx = Wt / W, sy = Ht / H)
    and everything else as the wrapped dataset gives it.  The boxes and the intrinsics differ from upstream's float scaling by
    the row scale on purpose (see the two functions).  z_near, z_far, lindisp, balanced and as_bytes are the wrapped dataset's.

    It gives evaluate, evaluate_approx, gen_video, vis_step and a DataLoader-fed Trainer the resolution that a
    ResidentSplit(image_size=...) run trained at.  An item whose size is image_size already is passed through untouched.
    __getitem__ uploads to `device`, runs the kernels and copies back, so it touches the device: use it with num_workers=0
    (which is what Trainer's loaders use), never in forked workers."""

    def __init__(self, dataset, image_size, device="cuda"):
        super().__init__()
        self.dataset = dataset
        self.image_size = util._target_size(image_size)
        if min(self.image_size) < 1:
            raise ValueError(f"image_size must be positive, got {self.image_size}")
        self.device = torch.device(device)
        self.as_bytes = bool(getattr(dataset, "as_bytes", False))
        self.balanced = bool(getattr(dataset, "balanced", True))
        for name in ("z_near", "z_far", "lindisp"):
            setattr(self, name, getattr(dataset, name, None))

    def __len__(self):
        return len(self.dataset)

    def _resample(self, t, channels_last):
        """A host image stack at the new size, back on the host.  channels_last: (NV, H, W[, C]) bytes; else (..., H, W)."""
        on_dev = util.upload(t.contiguous(), self.device)
        if t.dtype == torch.uint8:
            if not channels_last:
                raise ValueError(f"uint8 images must be (NV, H, W, C), got {tuple(t.shape)}")
            out = util.resize_area_u8(on_dev if t.dim() == 4 else on_dev.unsqueeze(-1), self.image_size)
            return (out if t.dim() == 4 else out.squeeze(-1)).cpu()
        return util.resize_area(on_dev, self.image_size).cpu()

    def __getitem__(self, index):
        item = dict(self.dataset[index])
        images = item["images"]
        as_bytes = images.dtype == torch.uint8
        H, W = (int(s) for s in (images.shape[1:3] if as_bytes else images.shape[-2:]))
        if (H, W) == self.image_size:
            return item
        item["images"] = self._resample(images, as_bytes)
        if "masks" in item:
            item["masks"] = self._resample(item["masks"], as_bytes)
        if "bbox" in item:
            item["bbox"] = util.resize_bbox(item["bbox"], (H, W), self.image_size)
        item["focal"], c = util.resize_intrinsics(item["focal"], item.get("c"), (H, W), self.image_size)
        if c is not None:
            item["c"] = c
        return item
