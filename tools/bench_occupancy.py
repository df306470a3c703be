#!/usr/bin/env python3
"""Wall-clock time of a novel-view video with and without empty-space culling: --frames orbit poses of
--size x --size (40 of 128 x 128 by default, an SRN-like camera), fp16 kernel, 64 + 32 + 16 samples, one source view, and a
synthetic occupancy grid: OccupancyGrid.from_cells of a sphere of --radius in the box [-1, 1]^3 at --cells cells per axis.
The network's weights are synthetic, so the pictures mean nothing: what is measured is the cost of the frames.
  unbounded   render_image per pose
  bounded     NeRFRenderer.render_frames_bounded, and its steps one by one with a device synchronisation after each:
              rays + ray_bounds, the read of the counts, the render launches, the gather
  from_net    OccupancyGrid.from_net at 64^3 (one forward call of the coarse MLP and one pnr_occ_build)
In alternating rounds, device synchronisation at the two ends of each variant only.  Also printed: the share of pixels the
sphere covers (rays that hit / rays).
    python tools/bench_occupancy.py [--frames 40] [--size 128] [--rounds 5]
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
    from pixel_nerf_multiscale_amd.render import occupancy as occ
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
    x = (torch.arange(a.cells) + 0.5) / a.cells * 2 - 1
    i, j, k = torch.meshgrid(x, x, x, indexing="ij")
    grid = occ.OccupancyGrid.from_cells((i * i + j * j + k * k).sqrt() < a.radius, (-1,) * 3, (1,) * 3, device="cuda")
    steps = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def unbounded():
        with torch.no_grad():
            for f in range(F):
                with rend.keyed(frame_seed(seed, f)):
                    rend.render_image(net, poses[f], W, H, focal, z_near, z_far)

    def bounded():
        return rend.render_frames_bounded(net, poses, W, H, focal, z_near, z_far, grid, seed=seed)

    def bounded_steps():
        """render_frames_bounded's own steps, a synchronisation after each."""
        with torch.no_grad():
            def bounds():
                rays = torch.empty(F * HW, 8, device="cuda")
                for f in range(F):
                    util.gen_rays_device(poses[f], W, H, focal, z_near, z_far, out=rays[f * HW:(f + 1) * HW])
                return occ.ray_bounds(grid, rays, HW)
            ms_b, (rays_out, slot, counts) = timed(bounds)
            ms_r, cnt = timed(lambda: occ.read_counts(counts))
            record = torch.empty(F * HW, 4, device="cuda")

            def renders():
                for f, c in enumerate(cnt):
                    if c > 0:
                        with rend.keyed(frame_seed(seed, f)):
                            rend._forward_fused(net, rays_out[f * HW:f * HW + c][None], False,
                                                packed=(record[f * HW:f * HW + c].view(1, c, 4), ("fine",)))
            ms_l, _ = timed(renders)
            ms_g, _ = timed(lambda: occ.frame_from_hits(record, slot, HW, 1.0))
        for name, v in (("bounds", ms_b), ("read", ms_r), ("renders", ms_l), ("gather", ms_g)):
            steps.setdefault(name, []).append(v)
        return cnt

    def from_net():
        return occ.OccupancyGrid.from_net(net, sigma_thresh=0.0, reso=64)

    variants = {"unbounded": unbounded, "bounded": bounded, "bounded_steps": bounded_steps, "from_net": from_net}
    for fn in variants.values():                                     # warm-up: code objects, the allocators, the workspace
        timed(fn)
    steps.clear()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            t, out = timed(fn)
            ms[name].append(t)
            if name == "bounded_steps":
                hits = sum(out)
    med = {k: statistics.median(v) for k, v in ms.items()}
    share = hits / float(F * HW)
    print(f"empty-space culling, {F} frames of {W} x {H}, fp16, 64 + 32 + 16 samples, 1 source view, sphere of radius {a.radius} "
          f"in {a.cells}^3 cells ({grid.occupied_fraction():.4f} of the cells), pad = one cell diagonal")
    print(f"  rays that hit: {hits} of {F * HW} = {share:.4f} of the pixels")
    print(f"  ms per video, median of {a.rounds} alternating rounds (min .. max)")
    for name in variants:
        print(f"  {name:<16}{med[name]:>10.3f}{min(ms[name]):>10.3f}{max(ms[name]):>10.3f}")
    for name, v in steps.items():
        print(f"    {name:<14}{statistics.median(v):>10.3f}{min(v):>10.3f}{max(v):>10.3f}")
    print(json.dumps({"what": "occupancy", "frames": F, "image": f"{W}x{H}", "precision": "fp16", "rounds": a.rounds,
                      "hit_share": round(share, 4), **{"ms_" + k: round(v, 3) for k, v in med.items()},
                      **{"ms_step_" + k: round(statistics.median(v), 3) for k, v in steps.items()},
                      **{"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--frames", str(a.frames),
           "--size", str(a.size), "--rounds", str(a.rounds), "--cells", str(a.cells), "--radius", str(a.radius)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
