#!/usr/bin/env python3
"""
Golden vectors for the mask-weighted pixel sampler (src/util/util.py:210-222).  Dev container only, like gen_golden.py: imports
the reference's own util.masked_sample UNMODIFIED (third-party stand-ins from tools/_shims) and records, per case, the float
mask it was given, the pixels it draws under a torch seed and the state the global generator ends in, into
tests/golden/masked_sample.npz.  Arrays and numbers only.

    python tools/gen_golden_masked_sample.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402

CASES = [
    # name, seed, NV, H, W, num_pix, prop_inside, thresh, density
    ("disc_07", 1234, 3, 12, 16, 10, 0.7, 0.5, None),
    ("half_odd", 4321, 2, 5, 33, 5, 0.5, 0.5, 0.3),             # int(2.5 + 0.5) = 3 inside
    ("soft_thresh", 99, 4, 7, 9, 64, 0.25, 0.35, "soft"),
    ("all_outside_slots", 7, 1, 6, 6, 9, 0.0, 0.5, 0.5),
    ("all_inside_slots", 8, 2, 6, 6, 9, 1.0, 0.5, 0.5),
]


def make_mask(NV, H, W, density, seed):
    """float32 (NV, H, W): a disc per view, 0 / 1 noise at a density, or soft values in [0, 1] ("soft")."""
    rng = np.random.default_rng(seed)
    if density is None:
        r, c = np.mgrid[0:H, 0:W]
        return np.stack([((r - H / 2 + v) ** 2 + (c - W / 2 - v) ** 2 <= (min(H, W) / 3) ** 2) for v in range(NV)]).astype(np.float32)
    if density == "soft":
        return rng.random((NV, H, W)).astype(np.float32)
    return (rng.random((NV, H, W)) < density).astype(np.float32)


def main():
    import util  # the reference's src/util
    out = {"names": np.array(",".join(c[0] for c in CASES))}
    for name, seed, NV, H, W, num_pix, prop, thresh, density in CASES:
        masks = make_mask(NV, H, W, density, seed)
        torch.manual_seed(seed)
        pix = util.masked_sample(torch.from_numpy(masks), num_pix, prop, thresh)
        assert tuple(pix.shape) == (num_pix, 3)
        out[f"{name}__seed"] = np.array(seed)
        out[f"{name}__masks"] = masks
        out[f"{name}__args"] = np.array([num_pix, prop, thresh], np.float64)
        out[f"{name}__pix"] = pix.numpy()
        out[f"{name}__rng_end"] = torch.get_rng_state().numpy()
        inside = int((masks[pix[:, 0], pix[:, 1], pix[:, 2]] >= thresh).sum())
        print(f"{name}: {inside} of {num_pix} pixels inside at prop_inside {prop}")
    path = os.path.join(gu.GOLDEN_DIR, "masked_sample.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
