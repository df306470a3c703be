#!/usr/bin/env python3
"""Training-step timing of the differentiable path: renderer forward with the tape + loss +
backward, at the reference's training shape (conf/default_mv.conf + train/train.py: SB objects x ray_batch_size
rays, 64 coarse + 32 fine samples, 1-3 source views).  Prints one JSON line per configuration.
    python tools/bench_train.py [--sb 4] [--rays 128] [--views 1 2] [--steps 10]
--front-end: the step starts from a loader-style batch (NV views of 128 x 128 per object on the device, boxes on the host)
and goes through train.calc_losses; timed in the same run, in alternating rounds: the step above (rays and targets made
outside the loop), the calc_losses step, and a step whose front end is the reference's recipe in torch (gen_rays over
every view + indexing, torch criteria, three .item()); and the two front ends alone.
    python tools/bench_train.py --precision bf16 --front-end
--cam-grad: the same step with camera gradients off (the step above: today's backward call) and on (the rays, the c2w source
poses handed to set_cameras, focal and c require grad: pnr_point_mlp_bwd_cam), in alternating rounds of one run; medians and
the spread of the rounds.
    python tools/bench_train.py --precision bf16 --cam-grad"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
import hip_util as hu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "bf16x3"])
    ap.add_argument("--front-end", action="store_true")
    ap.add_argument("--nv", type=int, default=50, help="--front-end: views per object in the batch")
    ap.add_argument("--rounds", type=int, default=5, help="--front-end / --cam-grad: alternating rounds of --steps steps; medians reported")
    ap.add_argument("--cam-grad", action="store_true")
    a = ap.parse_args()
    if a.front_end:
        return front_end(a)
    if a.cam_grad:
        return cam_grad(a)
    for ns in a.views:
        spec = gu._case(seed=5, d_hidden=512, lat=[(256, 8, 8)], image=(128, 128), focal=131.25, NS=ns, SB=a.sb,
                        N=a.rays, Kc=64, Kf=32, Kfd=16)
        rays_np, poses_np = gu.make_inputs(spec)
        net = hu.build_net(spec, poses_np).train()
        net.train_precision = a.precision
        maps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gu.make_latents(spec)]
        net.encoder.set_latents(maps)
        rend = hu.build_renderer(spec)
        rays = torch.from_numpy(rays_np).cuda()
        tgt = torch.rand(a.sb, a.rays, 3, device="cuda")
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            out = rend(net, rays, want_weights=True)
            loss = ((out.coarse.rgb - tgt) ** 2).mean() + ((out.fine.rgb - tgt) ** 2).mean()
            loss.backward()
            opt.step()

        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.steps * 1e3
        n_rays = a.sb * a.rays
        pts = n_rays * (64 + 96)
        flop_fwd = pts * 2 * (ns * 1987584 + 1050624)
        print(json.dumps({"what": "train_step", "sb": a.sb, "rays_per_obj": a.rays, "views": ns, "samples": "64+32",
                          "ms_per_step": round(ms, 2), "rays_per_s": round(n_rays / ms * 1e3),
                          "tflops_fwd_bwd": round(3 * flop_fwd / ms / 1e9, 1), "dtype": {"fp32": "f32", "bf16": "bf16 products, f32 accumulate", "bf16x3": "bf16x3 split products (fp32-class), f32 accumulate"}[a.precision]}))


def cam_grad(a):
    import statistics
    W = H = 128
    for ns in a.views:
        spec = gu._case(seed=5, d_hidden=512, lat=[(256, 8, 8)], image=(W, H), focal=131.25, NS=ns, SB=a.sb,
                        N=a.rays, Kc=64, Kf=32, Kfd=16)
        rays_np, poses_np = gu.make_inputs(spec)
        net = hu.build_net(spec, poses_np).train()
        net.train_precision = a.precision
        maps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gu.make_latents(spec)]
        net.encoder.set_latents(maps)
        rend = hu.build_renderer(spec)
        rays = torch.from_numpy(rays_np).cuda()
        tgt = torch.rand(a.sb, a.rays, 3, device="cuda")
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
        c2w = torch.from_numpy(poses_np).reshape(-1, 4, 4).cuda()
        leaves = [t.requires_grad_(True) for t in (rays.clone(), c2w.clone(), torch.full((a.sb, 2), 131.25, device="cuda"),
                                                   torch.full((a.sb, 2), 64.0, device="cuda"))]

        def step(on):
            opt.zero_grad(set_to_none=True)
            if on:
                for t in leaves:
                    t.grad = None
                net.set_cameras(*leaves[1:], W, H)          # the graph from the c2w / focal / c leaves, rebuilt every step
            out = rend(net, leaves[0] if on else rays, want_weights=True)
            loss = ((out.coarse.rgb - tgt) ** 2).mean() + ((out.fine.rgb - tgt) ** 2).mean()
            loss.backward()
            opt.step()

        def cameras_off():
            net.set_cameras(c2w, *hu.camera_tensors(spec), W, H)

        ms = {"off": [], "on": []}
        for r in range(-1, a.rounds):                       # round -1: warm-up
            for k in ms:
                if k == "off":
                    cameras_off()
                for _ in range(a.warmup if r < 0 else 0):
                    step(k == "on")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step(k == "on")
                torch.cuda.synchronize()
                if r >= 0:
                    ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"what": "train_step_cam_grad", "sb": a.sb, "rays_per_obj": a.rays, "views": ns, "precision": a.precision,
                          "steps": a.steps, "rounds": a.rounds, "ms_off": round(med["off"], 3), "ms_on": round(med["on"], 3),
                          "spread_ms_off": round(max(ms["off"]) - min(ms["off"]), 3),
                          "spread_ms_on": round(max(ms["on"]) - min(ms["on"]), 3),
                          "on_over_off": round(med["on"] / med["off"], 4)}))


def _torch_front_end(data, dev, ray_batch_size, nviews, z_near, z_far):
    """The reference's recipe (train/train.py:243-317) with this package's torch helpers: every view's rays, every image
    to [0, 1], then ray_batch_size rows of each."""
    import numpy as np
    from pixel_nerf_multiscale_amd import util
    all_images, all_poses = data["images"].to(dev), data["poses"].to(dev)
    SB, NV, _, H, W = all_images.shape
    curr = nviews[int(torch.randint(0, len(nviews), ()))]
    image_ord = torch.randint(0, NV, (SB, 1)) if curr == 1 else torch.empty((SB, curr), dtype=torch.long)
    all_rays, all_gt = [], []
    for o in range(SB):
        if curr > 1:
            image_ord[o] = torch.from_numpy(np.random.choice(NV, curr, replace=False))
        images_0to1 = all_images[o] * 0.5 + 0.5
        cam_rays = util.gen_rays(all_poses[o], W, H, data["focal"][o], z_near, z_far, c=None)
        gt_all = images_0to1.permute(0, 2, 3, 1).contiguous().reshape(-1, 3)
        pix = util.bbox_sample(data["bbox"][o], ray_batch_size)
        pix_inds = pix[..., 0] * H * W + pix[..., 1] * W + pix[..., 2]
        all_gt.append(gt_all[pix_inds])
        all_rays.append(cam_rays.view(-1, 8)[pix_inds])
    image_ord = image_ord.to(dev)
    return (torch.stack(all_rays), torch.stack(all_gt), util.batched_index_select_nd(all_images, image_ord),
            util.batched_index_select_nd(all_poses, image_ord))


def front_end(a):
    import statistics

    import numpy as np
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    dev = torch.device("cuda")
    H = W = 128
    lam_c, lam_f = 1.0, 1.0
    for ns in a.views:
        spec = gu._case(seed=5, d_hidden=512, lat=[(256, 8, 8)], image=(W, H), focal=131.25, NS=ns, SB=a.sb,
                        N=a.rays, Kc=64, Kf=32, Kfd=16)
        rays_np, poses_np = gu.make_inputs(spec)
        net = hu.build_net(spec, poses_np).train()
        net.train_precision = a.precision
        maps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gu.make_latents(spec)]
        # the trunk is not what this measures: every variant gets the same fixed latent maps, as the plain step does
        net.encoder.forward = lambda images: net.encoder.set_latents(maps)
        net.encoder.set_latents(maps)
        rend = hu.build_renderer(spec)
        render_par = rend.bind_parallel(net, None)
        rays = torch.from_numpy(rays_np).cuda()
        tgt = torch.rand(a.sb, a.rays, 3, device="cuda")
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
        rng = np.random.default_rng(9)
        lo = rng.integers(0, 48, (a.sb, a.nv, 2))
        data = {
            "images": torch.from_numpy(rng.uniform(-1, 1, (a.sb, a.nv, 3, H, W)).astype(np.float32)).cuda(),
            "poses": torch.from_numpy(np.stack([np.stack([gu.pose_spherical(360.0 * v / a.nv + 11.0 * o, -20.0, spec["radius"])
                                                          for v in range(a.nv)]) for o in range(a.sb)])).cuda(),
            "focal": torch.full((a.sb,), 131.25),
            "bbox": torch.from_numpy(np.concatenate([lo, lo + 64], -1).astype(np.float32)),
        }
        kw = dict(ray_batch_size=a.rays, nviews=[ns], z_near=spec["z_near"], z_far=spec["z_far"])
        crit = RenderLoss(lam_c, lam_f)
        mse = torch.nn.MSELoss()

        def plain_cameras():                    # the other variants' encode() leaves their own source cameras behind
            net.set_cameras(torch.from_numpy(poses_np).reshape(-1, 4, 4), *hu.camera_tensors(spec), W, H)

        def step_plain():                       # the step this tool times without --front-end
            opt.zero_grad(set_to_none=True)
            out = rend(net, rays, want_weights=True)
            loss = ((out.coarse.rgb - tgt) ** 2).mean() + ((out.fine.rgb - tgt) ** 2).mean()
            loss.backward()
            opt.step()

        def step_device():
            opt.zero_grad(set_to_none=True)
            loss, _ = train.calc_losses(net, render_par, data, loss=crit, **kw)
            loss.backward()
            opt.step()

        def step_torch():
            opt.zero_grad(set_to_none=True)
            r, gt, src_images, src_poses = _torch_front_end(data, dev, **kw)
            net.encode(src_images, src_poses, data["focal"].to(dev))
            out = render_par(r, want_weights=True)
            rgb_loss = mse(out["coarse"]["rgb"], gt)
            d = {"rc": rgb_loss.item() * lam_c}
            fine_loss = mse(out["fine"]["rgb"], gt)
            rgb_loss = rgb_loss * lam_c + fine_loss * lam_f
            d["rf"] = fine_loss.item() * lam_f
            d["t"] = rgb_loss.item()
            rgb_loss.backward()
            opt.step()

        variants = {"step_plain": step_plain, "step_calc_losses": step_device, "step_torch_front_end": step_torch,
                    "front_end_device": lambda: train.make_batch(data, dev, **kw),
                    "front_end_torch": lambda: _torch_front_end(data, dev, **kw)}
        for k, fn in variants.items():
            if k == "step_plain":
                plain_cameras()
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                if k == "step_plain":
                    plain_cameras()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"what": "train_step_front_end", "sb": a.sb, "rays_per_obj": a.rays, "views": ns, "nv": a.nv, "image": f"{W}x{H}",
               "precision": a.precision, "steps": a.steps, "rounds": a.rounds}
        res.update({"ms_" + k: round(v, 3) for k, v in med.items()})
        res.update({"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()})
        res["front_end_share_of_step"] = round(med["front_end_device"] / med["step_calc_losses"], 4)
        res["device_front_end_faster_than_torch"] = med["front_end_device"] < med["front_end_torch"]
        res["step_within_plain_plus_front_end_3pct"] = med["step_calc_losses"] <= 1.03 * (med["step_plain"] + med["front_end_device"])
        print(json.dumps(res))


if __name__ == "__main__":
    main()
