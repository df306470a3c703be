#!/usr/bin/env python3
"""Wall-clock time of one train.vis_step at 128 x 128, with 1 and 3 source views and 64 + 32 samples, fp16
kernel, and of the two tails that can follow the same render:
  render_only   the draws, the uploads, the target view's rays, encode and render_par(want_weights=True); nothing leaves the device
  host_tail     the reference's recipe (train/train.py:455-531) restated on top of the same render: seven copies to the host,
                util.cmap on the host (two per pass), np.hstack / np.vstack, a numpy PSNR
  device        train.vis_step: one pnr_vis_panel call; the panel and the PSNR stay on the device
All three in one process, under the same seeds, in alternating rounds of --iters steps; a device synchronise at the two ends
of a round only.  Then both tails once on ONE render, and how far their panels and PSNRs are apart.
    python tools/bench_vis.py [--iters 20] [--rounds 5]
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

Z_NEAR, Z_FAR = 1.25, 2.75


def worker(a):
    import numpy as np
    import torch

    import golden_util as gu
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, train, util
    W = H = a.size
    SB, NV = 2, 5
    spec = dict(gu.CASES["full_ns1"])
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp16")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).cuda().eval()
    render_par = rend.bind_parallel(net, None)
    rng = np.random.default_rng(1)
    data = {
        "images": torch.from_numpy(rng.uniform(-1, 1, (SB, NV, 3, H, W)).astype(np.float32)),
        "poses": torch.from_numpy(np.stack([np.stack([gu.pose_spherical(72.0 * v + 13.0 * o, -20.0 - 3.0 * o, 2.0)
                                                      for v in range(NV)]) for o in range(SB)])),
        "focal": torch.full((SB,), 131.25 * a.size / 128.0),
    }

    def front(nviews):
        """vis_step up to and including the render; -> what the tails need."""
        b = int(np.random.randint(0, SB))
        views_src, view_dest = train.draw_vis_views(NV, nviews)
        images = util.upload(data["images"][b].contiguous(), "cuda")
        poses = data["poses"][b].float()
        rays = util.gen_rays_device(poses[view_dest], W, H, data["focal"][b], Z_NEAR, Z_FAR)
        src = torch.from_numpy(views_src)
        with torch.no_grad():
            net.encode(images.index_select(0, util.upload(src, "cuda")).unsqueeze(0), util.upload(poses[src].contiguous(), "cuda").unsqueeze(0),
                       util.upload(data["focal"][b:b + 1], "cuda"))
            rd = render_par(rays[None], want_weights=True)
        return images, views_src, view_dest, rd

    def host_tail(nviews, fr=None):
        images, views_src, view_dest, rd = front(nviews) if fr is None else fr
        images_0to1 = images * 0.5 + 0.5
        source_views = images_0to1[torch.from_numpy(views_src).cuda()].permute(0, 2, 3, 1).cpu().numpy().reshape(-1, H, W, 3)
        gt = images_0to1[view_dest].permute(1, 2, 0).cpu().numpy().reshape(H, W, 3)
        rows = []
        for lv in ("coarse", "fine"):
            p = rd[lv]
            alpha = p["weights"][0].sum(dim=-1).cpu().numpy().reshape(H, W)
            rgb = p["rgb"][0].cpu().numpy().reshape(H, W, 3)
            depth = p["depth"][0].cpu().numpy().reshape(H, W)
            rows.append(np.hstack([*source_views, gt, util.cmap(depth) / 255, rgb, util.cmap(alpha) / 255]))
        vis = np.vstack(rows)
        return vis, util.psnr(rgb, gt)

    def device(nviews):
        return train.vis_step(net, rend, render_par, data, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR)

    variants = {"render_only": front, "host_tail": host_tail, "device": device}

    def timed(fn, nviews):
        torch.manual_seed(5); np.random.seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn(nviews)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e3

    print(f"train.vis_step, {SB} objects x {NV} views of {W} x {H}, fp16, 64 + 32 samples; ms per step, median of {a.rounds} "
          f"alternating rounds of {a.iters} steps (min .. max)")
    line = {"what": "vis_step", "image": f"{W}x{H}", "precision": "fp16", "iters": a.iters, "rounds": a.rounds}
    for ns in (1, 3):
        nviews = [ns]
        for fn in variants.values():                                     # warm-up: MIOpen's choices, the allocators, the table
            timed(fn, nviews)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(timed(fn, nviews))
        med = {k: statistics.median(v) for k, v in ms.items()}
        base = med["render_only"]
        print(f"  {ns} source view(s), panel {2 * H} x {(ns + 4) * W}")
        print(f"    {'variant':<14}{'ms/step':>9}{'min':>9}{'max':>9}{'tail ms':>10}{'share of a step':>17}")
        for k in variants:
            tail = med[k] - base
            print(f"    {k:<14}{med[k]:>9.3f}{min(ms[k]):>9.3f}{max(ms[k]):>9.3f}" + ("" if k == "render_only" else f"{tail:>10.3f}{tail / med[k]:>16.1%}"))
        # both tails on ONE render: two steps of this set-up under the same seeds were seen 1e-5 dB apart, so their panels
        # say nothing about the tails
        torch.manual_seed(5); np.random.seed(5)
        fr = front(nviews)
        vis_h, psnr_h = host_tail(nviews, fr)
        res = util.vis_panel(fr[0], fr[1], fr[2], [(fr[3][lv]["rgb"][0], fr[3][lv]["depth"][0], fr[3][lv]["weights"][0])
                                                   for lv in ("coarse", "fine")])
        diff = np.abs(res.panel.cpu().numpy().astype(np.float64) - vis_h)
        d_alpha = float(diff[:, (ns + 3) * W:].max())                    # the opacity tiles: fp64 sum here, torch's fp32 sum there
        d_rest = float(diff[:, :(ns + 3) * W].max())
        psnr_d = float(res.psnr)
        print(f"    both tails on one render: psnr host {psnr_h:.6f} device {psnr_d:.6f}; max |panel difference| outside the "
              f"opacity tiles {d_rest:.3e}, on them {d_alpha:.3e} (the colour map stretches the last bits of a nearly constant map "
              "over the whole table)")
        line.update({f"ns{ns}_ms_{k}": round(v, 3) for k, v in med.items()})
        line.update({f"ns{ns}_spread_ms_{k}": round(max(v) - min(v), 3) for k, v in ms.items()})
        line.update({f"ns{ns}_psnr_host": round(psnr_h, 6), f"ns{ns}_psnr_device": round(psnr_d, 6),
                     f"ns{ns}_panel_diff_outside_opacity": d_rest, f"ns{ns}_panel_diff_opacity": d_alpha})
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--size", str(a.size),
           "--iters", str(a.iters), "--rounds", str(a.rounds)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
