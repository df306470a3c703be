"""Shared by tests/test_video_cpu.py, tests/test_gpu_video.py and tools/bench_video.py: the numpy model of the video
back end's quantisation (include/pnr.h, "novel-view video"), the value set its tests run on, the view-strip model and the
fixtures."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F255 = np.float32(255.0)


def quantize_product(p):
    """byte(p) of the header for fp32 products p -> (bytes uint8, out_of_range bool): truncation toward zero for
    -1 < p < 256; elsewhere 0 for p <= -1 and NaN, 255 for p >= 256, and counted."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        inside = (p > np.float32(-1.0)) & (p < np.float32(256.0))
        high = p >= np.float32(256.0)
    out = np.zeros(p.shape, np.uint8)
    out[inside] = np.trunc(p[inside]).astype(np.int32).astype(np.uint8)
    out[~inside & high] = 255
    return out, ~inside


def quantize_model(x):
    """pnr_video_frames for float32 x of any shape -> (bytes of the same shape, the number of out-of-range components)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        out, bad = quantize_product(x * F255)
    return out, int(bad.sum())


def view_strip_model(images, scale, lo):
    """pnr_view_strip for images (NS, 3, H, W) float32 -> (H, NS W, 3) uint8, filled by address (not by np.hstack: the layout
    test compares the two)."""
    images = np.asarray(images, dtype=np.float32)
    NS, _, H, W = images.shape
    with np.errstate(invalid="ignore", over="ignore"):
        p = (images * np.float32(scale) + np.float32(lo)) * F255       # three fp32 operations, each rounded on its own
    q, _ = quantize_product(p)
    out = np.zeros((H, NS * W, 3), np.uint8)
    for v in range(NS):
        for c in range(3):
            out[:, v * W:(v + 1) * W, c] = q[v, c]
    return out


def value_set():
    """-> (in_range float32 values, out_of_range float32 values): all 256 k / 255 in fp32 with both fp32 neighbours of each,
    +-0, a denormal, 1, nextafter(1, 2), -0.5 / 255, 255.9 / 255; outside numpy's range -1 / 255, 256 / 255, 1e30, +-Inf, NaN."""
    k = np.arange(256, dtype=np.float32) / F255
    up, down = np.nextafter(k, np.float32(2.0)), np.nextafter(k, np.float32(-2.0))
    extra = np.array([0.0, -0.0, 1e-41, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.float32(-0.5) / F255,
                      np.float32(255.9) / F255], np.float32)
    outside = np.array([np.float32(-1.0) / F255, np.float32(256.0) / F255, 1e30, np.inf, -np.inf, np.nan], np.float32)
    return np.concatenate((k, up, down, extra)), outside


def fill(n, seed, with_outside=True):
    """n float32 values drawn from the value set in a seeded order, every member present once when n allows."""
    inside, outside = value_set()
    pool = np.concatenate((inside, outside)) if with_outside else inside
    rng = np.random.default_rng(seed)
    idx = rng.permutation(len(pool))
    reps = -(-n // len(pool))
    return pool[np.concatenate([idx] + [rng.permutation(len(pool)) for _ in range(reps - 1)])[:n]].astype(np.float32)


def all_bytes_image(H, W):
    """(H, W, 3) uint8: channel c of pixel i holds (i + 85 c) mod 256, so H * W >= 256 pixels hold every byte value in every
    channel position, and a smaller image does once it is shifted by 0, H * W, 2 H * W, .. (the caller adds the shift)."""
    n = H * W
    img = np.zeros((n, 3), np.uint8)
    for c in range(3):
        img[:, c] = (np.arange(n) + 85 * c) % 256
    return img.reshape(H, W, 3)


def load_paths_fixture():
    return np.load(os.path.join(GOLDEN, "video_paths.npz"))


def load_dtu_keys():
    z = np.load(os.path.join(GOLDEN, "video_dtu_keys.npz"))
    return z["t_in"], z["quats"], z["scales"]
