"""What both dataset classes share: reading 8-bit files, the bounding box of a mask, and the two item modes."""
import numpy as np
import torch
from PIL import Image


def read_u8(path):
    """An image file as a uint8 array (H, W) or (H, W, channels), as PIL decodes it."""
    with Image.open(path) as im:
        return np.asarray(im)


def read_rgb(path):
    """The first three channels of an RGB or RGBA file: uint8 (H, W, 3)."""
    with Image.open(path) as im:
        if im.mode not in ("RGB", "RGBA"):
            im = im.convert("RGB")
        return np.ascontiguousarray(np.asarray(im)[..., :3])


def mask_bbox(mask, path):
    """(cmin, rmin, cmax, rmax) float32 of a boolean (H, W) mask: its first and last non-empty column and row."""
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    if rows.size == 0:
        raise RuntimeError(f"{path}: the view has no foreground pixel, so it has no bounding box")
    return np.array([cols[0], rows[0], cols[-1], rows[-1]], dtype=np.float32)


def check_image_size(image_size, H, W, path):
    """image_size None or the files' own (H, W): a dataset reads what the files hold.  Area resampling to another size is done
    on the device, by ResidentSplit(image_size=...) and ResizedDataset."""
    if image_size is None:
        return
    want = (int(image_size), int(image_size)) if np.isscalar(image_size) else tuple(int(s) for s in image_size)
    if want != (H, W):
        raise NotImplementedError(f"image_size {want} differs from the files' {(H, W)} ({path}): resampling is not implemented "
                                  "in the dataset classes; use data.ResidentSplit(image_size=...) or data.ResizedDataset")


def images_to_float(images_u8, balanced):
    """uint8 (NV, H, W, 3) -> float32 (NV, 3, H, W) in torch's own arithmetic: b / 255, balanced: then (. - 0.5) / 0.5 — the
    values pnr_image_to_tensor pins on the device."""
    t = torch.as_tensor(images_u8).permute(0, 3, 1, 2).float().div(255.0)
    if balanced:
        t = t.sub(0.5).div(0.5)
    return t.contiguous()


def pack_views(images, masks, as_bytes, balanced):
    """images: list of uint8 (H, W, 3); masks: list of bool (H, W) -> the item's ("images", "masks") in the asked mode."""
    images = torch.from_numpy(np.stack(images))
    masks = torch.from_numpy(np.stack(masks))
    if as_bytes:
        return images, masks.to(torch.uint8) * 255
    return images_to_float(images, balanced), masks[:, None].float()
