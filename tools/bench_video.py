#!/usr/bin/env python3
"""Wall-clock time of the tail of a novel-view video: --frames frames of --size x --size (40 of 128 x 128 by
default), fp16 kernel, one source view, the camera path video.orbit_poses.  Three variants in one process, in alternating
rounds, device synchronisation at the two ends of each only:
  render_only  the frames rendered into the packed record, nothing quantised, nothing leaves the device
  host_tail    the reference's tail (gen_video.py:236): the same render, the fp32 frames copied to the host (12 bytes per
               pixel), * 255 and astype(np.uint8) in numpy
  device_tail  video.render_video (one pnr_video_frames launch over the stack) and ONE copy of 3 bytes per pixel to the host
A tail's own time is its variant minus render_only.
    python tools/bench_video.py [--frames 40] [--size 128] [--rounds 7]
The measuring runs in a child process under `timeout` (--timeout seconds); the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def worker(a):
    import numpy as np
    import torch

    import golden_util as gu
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, util, video
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    W = H = a.size
    F, HW = a.frames, a.size * a.size
    focal, z_near, z_far, seed = 131.25 * a.size / 128.0, 1.25, 2.75, 777
    spec = dict(gu.CASES["full_ns1"])
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    net.precision = "fp16"
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).cuda().eval()
    src = torch.rand(1, 1, 3, H, W, generator=torch.Generator().manual_seed(1)) * 2 - 1
    pose = torch.from_numpy(np.stack([gu.pose_spherical(0.0, -20.0, 2.0)]))[None]
    with torch.no_grad():
        net.encode(src.cuda(), pose.cuda(), torch.tensor(focal)[None].cuda())
    poses = video.orbit_poses(F, -10.0, 2.0)
    record = torch.empty(F * HW, 4, device="cuda")
    rgb_h = torch.empty(F, H, W, 3, dtype=torch.float32, pin_memory=True)
    u8_h = torch.empty(F, H, W, 3, dtype=torch.uint8, pin_memory=True)
    kept = {}

    def render_into_record():
        with torch.no_grad():
            for i in range(F):
                cam = util.camera(poses[i], W, H, focal, z_near, z_far)
                with rend.keyed(frame_seed(seed, i)):
                    rend._forward_fused(net, None, False, camera=cam, packed=(record[i * HW:(i + 1) * HW].view(1, HW, 4), ("fine",)))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host_tail():
        render_into_record()
        rgb_h.copy_(record[:, :3].reshape(F, H, W, 3), non_blocking=True)
        torch.cuda.synchronize()
        with np.errstate(invalid="ignore"):
            kept["host"] = (rgb_h.numpy() * 255).astype(np.uint8)

    def device_tail():
        frames, _count = video.render_video(net, rend, poses, W, H, focal, z_near, z_far, seed=seed)
        u8_h.copy_(frames, non_blocking=True)
        torch.cuda.synchronize()
        kept["device"] = u8_h.numpy().copy()

    variants = {"render_only": render_into_record, "host_tail": host_tail, "device_tail": device_tail}
    for fn in variants.values():                                     # warm-up: code objects, the allocators, the workspace
        timed(fn)
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    same = bool(np.array_equal(kept["host"], kept["device"]))        # in range the two tails are the same bytes
    print(f"video tail, {F} frames of {W} x {H}, fp16, 64 + 32 samples, 1 source view; ms per video, median of {a.rounds} "
          f"alternating rounds (min .. max); the two tails' bytes are equal: {same}")
    print(f"  {'variant':<14}{'ms':>10}{'min':>10}{'max':>10}{'tail ms':>10}")
    for k in variants:
        tail = "" if k == "render_only" else f"{med[k] - med['render_only']:>10.3f}"
        print(f"  {k:<14}{med[k]:>10.3f}{min(ms[k]):>10.3f}{max(ms[k]):>10.3f}{tail}")
    print(json.dumps({"what": "video_tail", "frames": F, "image": f"{W}x{H}", "precision": "fp16", "rounds": a.rounds,
                      **{"ms_" + k: round(v, 3) for k, v in med.items()},
                      **{"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()}, "bytes_equal": same}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--frames", str(a.frames),
           "--size", str(a.size), "--rounds", str(a.rounds)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
