#!/usr/bin/env python3
"""
Golden vectors for the colour map's quantisation.  Dev container only, like gen_golden_rays.py: imports the reference's
own util.image_float_to_uint8 (src/util/util.py:13-23) UNMODIFIED (third-party stand-ins from tools/_shims) and records its
bytes for a handful of seeded float32 maps into tests/golden/vis_quantize.npz: a 19 x 13 uniform map, a ramp with exact ties
at bin edges, a constant 0.7, all zeros, a range of 1e-12 around 1, negative values.  Arrays only.

    python tools/gen_golden_vis.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402

H, W = 13, 19


def maps():
    rng = np.random.default_rng(2024)
    ramp = (np.arange(H * W, dtype=np.float32) % 52).reshape(H, W) * np.float32(5.0)      # 0, 5, .., 255: q * 255 hits integers
    ramp[0, :3] = [0.0, 255.0, 127.5]
    near_one = (1.0 + rng.uniform(-0.5e-12, 0.5e-12, (H, W))).astype(np.float32)           # collapses to 1.0f: range 0
    return [
        ("uniform", rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)),
        ("ramp_ties", ramp),
        ("constant", np.full((H, W), 0.7, np.float32)),
        ("zeros", np.zeros((H, W), np.float32)),
        ("range_1e-12", near_one),
        ("negative", rng.uniform(-3.0, -0.25, (H, W)).astype(np.float32)),
        ("depth_like", rng.uniform(1.25, 2.75, (H, W)).astype(np.float32)),
    ]


def main():
    import util  # the reference's src/util
    out = {"names": np.array(",".join(n for n, _ in maps()))}
    with np.errstate(all="ignore"):
        for name, m in maps():
            q = util.image_float_to_uint8(m.copy())
            assert q.dtype == np.uint8 and q.shape == m.shape
            out[f"{name}__map"] = m
            out[f"{name}__u8"] = q
    path = os.path.join(gu.GOLDEN_DIR, "vis_quantize.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
