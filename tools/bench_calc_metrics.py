#!/usr/bin/env python3
"""Wall-clock time of evalio.metrics_map for one object with its two back ends, split into decode and
metrics: an SRN-like object (250 pairs of 128 x 128) and a DTU-like one (49 pairs of 400 x 300), seeded noise written as PNGs
into a temporary folder.  Per object and round:
    decode   PIL reads of every pair into uint8 arrays, which both back ends pay
    host     the reference's recipe on the decoded arrays: / 255 in fp32, evalio.psnr / evalio.ssim one pair at a time
    device   the decoded arrays into two pinned buffers, one upload and one util.eval_frames_u8 call per 256 frames, one read
    map_host / map_device   the whole evalio.metrics_map(metrics=.., overwrite=True) call, decode included
A device synchronisation ends every device measurement.
    python tools/bench_calc_metrics.py [--rounds 5]
The measuring runs in a child process under `timeout` (--timeout seconds); the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OBJECTS = [("srn_like", 250, 128, 128), ("dtu_like", 49, 300, 400)]          # name, pairs, H, W


def worker(a):
    import numpy as np
    import torch

    from pixel_nerf_multiscale_amd import evalio, util
    dev = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as tmp:
        for name, n, H, W in OBJECTS:
            datadir, output = os.path.join(tmp, name, "data"), os.path.join(tmp, name, "render")
            os.makedirs(os.path.join(datadir, "obj", "rgb"))
            os.makedirs(os.path.join(output, "obj"))
            rng = np.random.default_rng(n)
            pairs = []
            for v in range(n):
                gt = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
                pred = np.clip(gt.astype(np.int64) + rng.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
                pairs.append((os.path.join(datadir, "obj", "rgb", f"{v:06}.png"), os.path.join(output, "obj", f"{v:06}.png")))
                evalio.write_png(pairs[-1][0], gt)
                evalio.write_png(pairs[-1][1], pred)
            decoded = {}

            def decode():
                t0 = time.perf_counter()
                decoded["gt"] = [evalio._read_u8(g, ("RGB", "RGBA")) for g, _ in pairs]
                decoded["pred"] = [evalio._read_u8(p, ("RGB",)) for _, p in pairs]
                return (time.perf_counter() - t0) * 1e3

            def host():
                t0 = time.perf_counter()
                for g, p in zip(decoded["gt"], decoded["pred"]):
                    g, p = g.astype(np.float32)[..., :3] / 255.0, p.astype(np.float32) / 255.0
                    evalio.psnr(p, g)
                    evalio.ssim(p, g)
                return (time.perf_counter() - t0) * 1e3

            pin = [torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            rows_h = torch.empty((n, 2), dtype=torch.float64, pin_memory=True)

            def device():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for buf, arrays in zip(pin, (decoded["pred"], decoded["gt"])):
                    for i, arr in enumerate(arrays):
                        buf[i].numpy()[...] = arr
                rows = torch.empty(n, 2, dtype=torch.float64, device=dev)
                for s in range(0, n, 256):
                    util.eval_frames_u8(pin[0][s:s + 256].to(dev, non_blocking=True), pin[1][s:s + 256].to(dev, non_blocking=True),
                                        metrics_out=rows[s:s + 256])
                rows_h.copy_(rows, non_blocking=True)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            def whole(metrics):
                def run():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    evalio.metrics_map(datadir, output, dataset_format="srn", overwrite=True, metrics=metrics, verbose=False)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3
                return run

            variants = {"decode": decode, "host": host, "device": device, "map_host": whole("host"), "map_device": whole("device")}
            for fn in variants.values():                                 # warm-up: imports, allocators, code objects
                fn()
            ms = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    ms[k].append(fn())
            med = {k: statistics.median(v) for k, v in ms.items()}
            print(f"{name}: {n} pairs of {W} x {H}; ms per object, median of {a.rounds} alternating rounds (min .. max)")
            for k in variants:
                print(f"  {k:<12}{med[k]:>10.3f}{min(ms[k]):>10.3f}{max(ms[k]):>10.3f}")
            print(json.dumps({"what": "calc_metrics", "object": name, "pairs": n, "image": f"{W}x{H}", "rounds": a.rounds,
                              **{"ms_" + k: round(v, 3) for k, v in med.items()},
                              **{"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--rounds", str(a.rounds)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
