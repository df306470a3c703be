"""What the colour-jitter augmentation costs per training step at the DTU shape: SB 4 objects x 49 views of 300 x 400 bytes,
resident on the card (data.ResidentSplit, no boxes).

  make_batch          ONE train.make_batch(draws="device") timed to a synchronise: the parent path, the comparison base
  make_batch_jitter   the same with jitter=ColorJitter(): one plan launch (the draws and the grey mean over all 49 views of
                      every object: every byte of the batch is read once) and the two jitter gathers
  plan                util.color_jitter_plan alone
  host_torch          upstream's recipe restated in torch on the CPU: all 49 float views of ONE object through the four
                      operations (brightness, contrast, saturation, hue in that order, one draw), x SB for a batch

Alternating rounds (every device variant once per round), medians and spread over the rounds; the host recipe is timed
--host-reps times.  Prints one JSON line.
    python tools/bench_jitter.py"""
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
    as_bytes, balanced, z_near, z_far, lindisp = True, True, 0.1, 5.0, False


def _gray(x):
    return (0.2989 * x[:, 0:1] + 0.587 * x[:, 1:2] + 0.114 * x[:, 2:3])


def _hue(x, h):
    """torchvision's tensor adjust_hue restated: x (N, 3, H, W) in [0, 1]."""
    r, g, b = x.unbind(1)
    maxc, minc = x.max(1).values, x.min(1).values
    eq = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eq, ones, maxc)
    d = torch.where(eq, ones, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    hh = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    hh = (hh + h) % 1.0
    i = torch.floor(hh * 6.0)
    f = hh * 6.0 - i
    i = i.to(torch.int32) % 6
    v = maxc
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * f)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    mask = i.unsqueeze(1) == torch.arange(6).view(1, -1, 1, 1)
    a1, a2, a3 = torch.stack((v, q, p, p, t, v), 1), torch.stack((t, v, v, q, p, p), 1), torch.stack((p, p, t, v, v, q), 1)
    a4 = torch.stack((a1, a2, a3), 1)
    return torch.einsum("nijhw,njhw->nihw", a4, mask.to(x.dtype))


def host_recipe(images_u8, fb, fc, fs, fh):
    """One object's 49 views, uint8 (NV, H, W, 3) -> float (NV, 3, H, W) in [-1, 1], jittered with one draw."""
    x = images_u8.permute(0, 3, 1, 2).float().div(255.0)
    x = (x * fb).clamp(0, 1)
    x = (fc * x + (1.0 - fc) * _gray(x).mean()).clamp(0, 1)
    x = (fs * x + (1.0 - fs) * _gray(x)).clamp(0, 1)
    x = _hue(x, fh)
    return x.sub(0.5).div(0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--nv", type=int, default=49)
    ap.add_argument("--width", type=int, default=400)
    ap.add_argument("--height", type=int, default=300)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()

    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.data import ColorJitter, ResidentSplit
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    dev = torch.device("cuda")
    H, W = a.height, a.width
    rng = np.random.default_rng(9)
    objects = _Objects()
    for o in range(a.sb):
        objects.append({"path": f"scan{o}", "img_id": o, "focal": torch.tensor([361.5, 360.0]), "c": torch.tensor([200.3, 150.6]),
                        "images": torch.from_numpy(rng.integers(0, 256, (a.nv, H, W, 3), dtype=np.uint8)),
                        "poses": torch.from_numpy(np.stack([gu.pose_spherical(360.0 * v / a.nv + 11.0 * o, -20.0, 1.3)
                                                            for v in range(a.nv)])).float()})
    split = ResidentSplit(objects, dev)
    data = split.batch(list(range(a.sb)))
    jit = ColorJitter()
    kw = dict(ray_batch_size=a.rays, nviews=[a.views], z_near=0.1, z_far=5.0, draws="device")
    step = [0]

    def key():
        step[0] += 1
        return frame_seed(5, step[0])

    variants = {"make_batch": lambda: train.make_batch(data, dev, seed=key(), **kw),
                "make_batch_jitter": lambda: train.make_batch(data, dev, seed=key(), jitter=jit, **kw),
                "plan": lambda: util.color_jitter_plan(data["images"], jit, key())}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
                torch.cuda.synchronize()                    # one call to a synchronise: what a step waits for at worst
            ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)

    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        host_recipe(objects[0]["images"], 1.1, 0.9, 1.05, 0.1)
        host.append((time.perf_counter() - t0) * 1e3)

    res = {"what": "color_jitter", "sb": a.sb, "nv": a.nv, "image": f"{W}x{H}", "rays_per_obj": a.rays, "views": a.views,
           "steps": a.steps, "rounds": a.rounds, "bytes_resident_pool": split.nbytes, "host_threads": torch.get_num_threads()}
    res.update({"ms_" + k: round(statistics.median(v), 3) for k, v in ms.items()})
    res.update({"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()})
    res["ms_host_torch_one_object"] = round(statistics.median(host), 1)
    res["ms_host_torch_batch"] = round(statistics.median(host) * a.sb, 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
