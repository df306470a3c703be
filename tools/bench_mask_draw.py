"""Mask-weighted draws beside the box draws they replace, on synthetic disc objects held in memory (a disc
covers pi / 4 of its box): each figure timed to a synchronise, the median over --rounds with the spread (max - min).

  ms_table_build       util.mask_table (pnr_mask_table_build) for 32 objects x 50 views of 128 x 128 mask bytes
  ms_make_batch_box    ONE train.make_batch(draws="device") on a data.ResidentSplit(device_boxes=True) batch: pnr_train_draw
  ms_make_batch_mask   the same batch of data.ResidentSplit(device_masks=True) under prop_inside: pnr_train_draw_masked
  fg_share_box/_mask   the share of a step's rays that falls on the foreground under each kind of draw

Prints one JSON line.
    python tools/bench_mask_draw.py --rounds 20 --prop-inside 0.75"""
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


class Discs(list):
    as_bytes, z_near, z_far, lindisp, balanced = True, 0.8, 1.8, False, True


def disc_objects(n_obj, nv, size):
    """Items of an as_bytes dataset: a coloured disc of radius size / 4 on white, its mask and its box, per view."""
    r, c = np.mgrid[0:size, 0:size]
    items = Discs()
    for o in range(n_obj):
        rng = np.random.default_rng(o)
        centres = rng.integers(size // 4 + 1, size - size // 4 - 1, (nv, 2))
        masks = np.stack([(r - cr) ** 2 + (c - cc) ** 2 <= (size // 4) ** 2 for cr, cc in centres])
        images = np.full((nv, size, size, 3), 255, np.uint8)
        images[masks] = rng.integers(0, 255, (int(masks.sum()), 3), dtype=np.uint8)
        bbox = np.array([[cc - size // 4, cr - size // 4, cc + size // 4, cr + size // 4] for cr, cc in centres], np.float32)
        poses = np.stack([gu.pose_spherical(360.0 * v / nv + 11.0 * o, -20.0, 1.3) for v in range(nv)]).astype(np.float32)
        items.append({"path": "obj%03d" % o, "img_id": o, "focal": torch.tensor(131.25), "images": torch.from_numpy(images),
                      "masks": torch.from_numpy(masks.astype(np.uint8) * 255), "bbox": torch.from_numpy(bbox),
                      "poses": torch.from_numpy(poses)})
    return items


def timed(fn, rounds):
    """fn() to a synchronise, `rounds` times after two warm-up calls -> (median ms, spread ms)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4), round(max(ms) - min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--objects", type=int, default=16)
    ap.add_argument("--nv", type=int, default=50)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--prop-inside", type=float, default=0.75)
    a = ap.parse_args()
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    dev = torch.device("cuda")
    out = {"what": "mask_draw", "objects": a.objects, "nv": a.nv, "image": f"{a.size}x{a.size}", "sb": a.sb, "rays_per_obj": a.rays,
           "prop_inside": a.prop_inside, "rounds": a.rounds}

    big = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (32, 50, 128, 128), dtype=np.uint8)).to(dev)
    tables = (torch.empty(32, 50 * 128, 4, dtype=torch.int32, device=dev), torch.empty(32, 50 * 128 + 1, dtype=torch.int32, device=dev))
    out["ms_table_build"], out["spread_ms_table_build"] = timed(lambda: util.mask_table(big, out=tables), a.rounds)
    out["table_build_mask_mb"] = round(big.numel() / 1e6, 1)
    del big, tables

    items = disc_objects(a.objects, a.nv, a.size)
    ids = list(range(a.sb))
    kw = dict(ray_batch_size=a.rays, nviews=[1, 2], z_near=items.z_near, z_far=items.z_far, balanced=True, draws="device", seed=12345)
    boxed = ResidentSplit(items, dev, device_boxes=True).batch(ids)
    masked = ResidentSplit(items, dev, device_masks=True).batch(ids)
    out["ms_make_batch_box"], out["spread_ms_make_batch_box"] = timed(lambda: train.make_batch(boxed, dev, **kw), a.rounds)
    out["ms_make_batch_mask"], out["spread_ms_make_batch_mask"] = timed(
        lambda: train.make_batch(masked, dev, prop_inside=a.prop_inside, **kw), a.rounds)

    # the share of foreground rays: the same draws made by hand, their pixels looked up in the masks (one read each, untimed)
    flat = torch.stack([items[i]["masks"] for i in ids]).to(dev).reshape(a.sb, -1) >= 128
    B = 64 * a.rays
    pix_box, _ = util.train_draw(boxed["bbox_dev"], a.sb, a.nv, a.size, a.size, B, 0, 12345)
    pix_mask, _ = util.train_draw_masked(masked["mask_bits"], masked["mask_rows"], a.sb, a.nv, a.size, a.size, B, 0, 12345, a.prop_inside)
    out["fg_share_box"] = round(float(torch.gather(flat, 1, pix_box).float().mean()), 4)
    out["fg_share_mask"] = round(float(torch.gather(flat, 1, pix_mask).float().mean()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
