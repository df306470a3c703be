"""What area resampling costs on a resident SRN-like split: N objects x 50 views of 128 x 128 x 3 bytes brought to 64 x 64.

  pool_plain     data.ResidentSplit(dataset, device) timed to a synchronise: the pool at the items' own size, the base
  pool_resized   the same with image_size=64: every object through ONE staging buffer and util.resize_area_u8 into its slot
  resize_u8      util.resize_area_u8 alone on the whole plain pool (N x 50 frames, one launch), to a synchronise
  torch_area     torch's own recipe on the device for the same frames: float().div(255), F.interpolate(mode="area") — what
                 upstream pixelNeRF does to its float images, without the conversion back to bytes

The dataset is held in host memory (random bytes), so the pool builds time the uploads and the kernel, not a disk.  Alternating
rounds, medians and spread (max - min) over the rounds.  Prints one JSON line.
    python tools/bench_resize.py"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402


class _Objects(list):
    as_bytes, balanced, z_near, z_far, lindisp = True, True, 0.8, 1.8, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=32)
    ap.add_argument("--nv", type=int, default=50)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--target", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()

    from pixel_nerf_multiscale_amd import util
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    dev = torch.device("cuda")
    S, T = a.size, a.target
    rng = np.random.default_rng(9)
    poses = torch.from_numpy(np.stack([gu.pose_spherical(360.0 * v / a.nv, -20.0, 1.3) for v in range(a.nv)])).float()
    objects = _Objects()
    for o in range(a.objects):
        objects.append({"path": f"obj{o}", "img_id": o, "focal": 131.25, "c": torch.tensor([S / 2.0, S / 2.0]),
                        "images": torch.from_numpy(rng.integers(0, 256, (a.nv, S, S, 3), dtype=np.uint8)),
                        "bbox": torch.tensor([[8.0, 8.0, S - 9.0, S - 9.0]] * a.nv), "poses": poses})
    pool = ResidentSplit(objects, dev).images
    frames = pool.view(-1, S, S, 3)
    out = torch.empty(frames.shape[0], T, T, 3, dtype=torch.uint8, device=dev)

    def torch_area():
        x = frames.permute(0, 3, 1, 2).float().div(255.0)
        return torch.nn.functional.interpolate(x, size=(T, T), mode="area")

    variants = {"pool_plain": (lambda: ResidentSplit(objects, dev), 1),
                "pool_resized": (lambda: ResidentSplit(objects, dev, image_size=T), 1),
                "resize_u8": (lambda: util.resize_area_u8(frames, T, out=out), a.steps),
                "torch_area": (torch_area, a.steps)}
    for fn, _ in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (fn, steps) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
                torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / steps * 1e3)

    moved = frames.numel() + out.numel()
    res = {"what": "resize_area", "objects": a.objects, "nv": a.nv, "image": f"{S}x{S}", "target": f"{T}x{T}", "steps": a.steps,
           "rounds": a.rounds, "bytes_pool_plain": frames.numel(), "bytes_pool_resized": out.numel()}
    res.update({"ms_" + k: round(statistics.median(v), 3) for k, v in ms.items()})
    res.update({"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()})
    res["gb_per_s_resize_u8"] = round(moved / (statistics.median(ms["resize_u8"]) * 1e-3) / 1e9, 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
