#!/usr/bin/env python3
"""
Golden vectors for the training front end (train/train.py:280-311).  Dev container only, like gen_golden.py: imports the
reference's own util.bbox_sample / gen_rays / pose_spherical (src/util/util.py:225-281,314-328) UNMODIFIED (third-party
stand-ins from tools/_shims) and records, per case, the inputs of one training batch and what the reference makes of them
into tests/golden/train_batch.npz: the pixels bbox_sample draws under a torch seed, the flat indices train.py:298 derives,
the rows of gen_rays over all views at those indices, and the [0, 1] colours of those pixels.  Arrays and numbers only.

    python tools/gen_golden_batch.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402


def _boxes_case1(W, H):
    # (SB, NV, 4) = cmin, rmin, cmax, rmax: one box a single pixel, one the whole image, the rest ordinary
    return torch.tensor([[[5.0, 7.0, 5.0, 7.0], [0.0, 0.0, W - 1.0, H - 1.0], [2.0, 1.0, 9.0, 6.0]],
                         [[3.0, 2.0, 14.0, 11.0], [W - 1.0, H - 1.0, W - 1.0, H - 1.0], [0.0, 4.0, 6.0, 4.0]]])


CASES = [
    # name, seed, SB, NV, W, H, B, focal, c, z_near, z_far, boxes
    ("boxes_fxfy_c", 1234, 2, 3, 16, 12, 67, torch.tensor([[21.5, 19.25], [30.0, 33.75]]),
     torch.tensor([[7.25, 6.5], [9.0, 4.75]]), 0.8, 1.8, _boxes_case1),
    ("uniform_scalar_f", 4321, 2, 3, 16, 12, 67, torch.tensor([25.0, 31.5]), None, 1.2, 4.0, None),
]


def main():
    import util  # the reference's src/util
    out = {"names": np.array(",".join(c[0] for c in CASES))}
    for name, seed, SB, NV, W, H, B, focal, c, zn, zf, boxes in CASES:
        rng = np.random.default_rng(seed)
        images = torch.from_numpy(rng.uniform(-1.0, 1.0, (SB, NV, 3, H, W)).astype(np.float32))
        poses = torch.stack([torch.stack([util.pose_spherical(40.0 * v + 17.0 * o, -20.0 - 5.0 * o, 1.3 + 0.2 * v)
                                          for v in range(NV)]) for o in range(SB)])
        bboxes = None if boxes is None else boxes(W, H)
        torch.manual_seed(seed)
        pix_all, inds_all, rays_all, rgb_all = [], [], [], []
        for o in range(SB):
            if bboxes is not None:
                pix = util.bbox_sample(bboxes[o], B)
                pix_inds = pix[..., 0] * H * W + pix[..., 1] * W + pix[..., 2]
                pix_all.append(pix)
            else:
                pix_inds = torch.randint(0, NV * H * W, (B,))
            cam_rays = util.gen_rays(poses[o], W, H, focal[o], zn, zf, c=None if c is None else c[o])
            assert cam_rays.shape == (NV, H, W, 8)
            rgb = (images[o] * 0.5 + 0.5).permute(0, 2, 3, 1).contiguous().reshape(-1, 3)
            inds_all.append(pix_inds)
            rays_all.append(cam_rays.view(-1, 8)[pix_inds])
            rgb_all.append(rgb[pix_inds])
        out[f"{name}__seed"] = np.array(seed)
        out[f"{name}__images"] = images.numpy()
        out[f"{name}__poses"] = poses.numpy()
        out[f"{name}__bboxes"] = np.zeros(0, np.float32) if bboxes is None else bboxes.numpy()
        out[f"{name}__focal"] = focal.numpy()
        out[f"{name}__c"] = np.zeros(0, np.float32) if c is None else c.numpy()
        out[f"{name}__z"] = np.array([zn, zf], np.float64)
        out[f"{name}__pix"] = np.zeros(0, np.int64) if bboxes is None else torch.stack(pix_all).numpy()
        out[f"{name}__pix_inds"] = torch.stack(inds_all).numpy()
        out[f"{name}__rays"] = torch.stack(rays_all).numpy()
        out[f"{name}__rgb_gt"] = torch.stack(rgb_all).numpy()
    path = os.path.join(gu.GOLDEN_DIR, "train_batch.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
