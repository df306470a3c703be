#!/usr/bin/env python3
"""Timing of upstream pixelNeRF's latent map (encoder.latent_mode = "upstream"): every encoder level resized to level 0's size
and concatenated, plus the channels-last 16-bit image the render kernels gather from.  Timed in the same run, in alternating
rounds, medians reported, ms:
  fwd_torch      3 x F.interpolate(bilinear, align_corners=True) + cat + a channels-last fp16 copy
  fwd_kernel     util.upsample_concat(levels, torch.float16): pnr_upsample_concat, two launches, nothing in between
  fwdbwd_torch   the torch recipe under autograd and its backward (torch's upsample backward scatters with fp32 atomics)
  fwdbwd_kernel  util.upsample_concat under autograd and pnr_upsample_concat_bwd (gather, fp64 sums, one launch per level)
The cotangent of the backward is a fixed tensor, so both variants time the map and its adjoint alone.  One JSON line per shape:
SRN-like levels 64@64x64, 64@32x32, 128@16x16, 256@8x8 with N = 1, 2, 8 and DTU-like 64@150x200, 64@75x100, 128@38x50,
256@19x25 with N = 3.  The bytes are what the kernels must move: the levels read once, fp32 and 16-bit maps written once
(forward); the fp32 cotangent read once, the level gradients written once (backward).
    python tools/bench_upsample.py [--iters 2000] [--warmup 50] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRN = [(64, 64, 64), (64, 32, 32), (128, 16, 16), (256, 8, 8)]
DTU = [(64, 150, 200), (64, 75, 100), (128, 38, 50), (256, 19, 25)]
SHAPES = [("srn", 1, SRN), ("srn", 2, SRN), ("srn", 8, SRN), ("dtu", 3, DTU)]


def torch_map(levels):
    size = tuple(levels[0].shape[2:])
    return torch.cat([levels[0]] + [F.interpolate(l, size=size, mode="bilinear", align_corners=True) for l in levels[1:]], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_upsample.py measures on the GPU; there is none here")
    from pixel_nerf_multiscale_amd import util

    for name, n, shapes in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(3)
        levels = [torch.relu(torch.randn(n, c, h, w, device="cuda", generator=gen)) for c, h, w in shapes]
        leaves = [l.clone().requires_grad_(True) for l in levels]
        sum_c, (h0, w0) = sum(c for c, _, _ in shapes), shapes[0][1:]
        cot = torch.randn(n, sum_c, h0, w0, device="cuda", generator=gen)

        def fwd_torch():
            m = torch_map(levels)
            return m, m.to(torch.float16).contiguous(memory_format=torch.channels_last)

        def fwd_kernel():
            return util.upsample_concat(levels, torch.float16)

        def fwdbwd_torch():
            m = torch_map(leaves)
            m16 = m.detach().to(torch.float16).contiguous(memory_format=torch.channels_last)
            return torch.autograd.grad(m, leaves, cot), m16

        def fwdbwd_kernel():
            m, m16 = util.upsample_concat(leaves, torch.float16)
            return torch.autograd.grad(m, leaves, cot), m16

        variants = dict(fwd_torch=fwd_torch, fwd_kernel=fwd_kernel, fwdbwd_torch=fwdbwd_torch, fwdbwd_kernel=fwdbwd_kernel)

        def run(fn, iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / iters * 1e3

        for fn in variants.values():
            run(fn, a.warmup)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(run(fn, a.iters))
        med = {k: statistics.median(v) for k, v in ms.items()}
        # the two recipes compute the same map (torch's fp32 position arithmetic is a few 1e-7 of the maximum off)
        mk, mt = fwd_kernel()[0], fwd_torch()[0]
        gk, gt = fwdbwd_kernel()[0], fwdbwd_torch()[0]
        level_bytes = 4 * sum(l.numel() for l in levels)
        map_elems = n * sum_c * h0 * w0
        res = {"what": "upsample_concat", "shape": name, "n": n, "levels": ["%d@%dx%d" % s for s in shapes], "iters": a.iters,
               "rounds": a.rounds}
        res.update({"ms_" + k: round(v, 4) for k, v in med.items()})
        res.update({"spread_ms_" + k: round(max(v) - min(v), 4) for k, v in ms.items()})
        res["fwd_bytes"] = level_bytes + 6 * map_elems
        res["bwd_bytes"] = level_bytes + 4 * map_elems
        res["fwd_kernel_gb_per_s"] = round(res["fwd_bytes"] / (med["fwd_kernel"] * 1e-3) / 1e9, 1)
        res["kernel_faster_fwd"] = med["fwd_kernel"] < med["fwd_torch"]
        res["kernel_faster_fwdbwd"] = med["fwdbwd_kernel"] < med["fwdbwd_torch"]
        res["map_maxdiff_over_max"] = float((mk - mt).abs().max() / mt.abs().max())
        res["grad_maxdiff_over_max"] = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(gk, gt))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
