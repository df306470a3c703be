"""The opacity losses inside the training step they join: the bf16 step of SB 4 x 128 = 512 rays on a
data.ResidentSplit(device_masks=True) batch of synthetic disc objects (tools/bench_mask_draw.py's), four ways, each timed to a
synchronise — the median over --rounds steps with the spread (max - min):

  ms_step_plain        train.train_step as it is without the losses: the step of the parent commit
  ms_step_mask         + model.loss.MaskLoss (pnr_mask_gather, pnr_alpha_loss, pnr_alpha_loss_bwd)
  ms_step_mask_alpha   + model.loss.AlphaLossNV2 on the fine pass as well
  ms_step_torch        the same two losses written in torch: weights.sum(-1), clamp, F.binary_cross_entropy and the reference's
                       log expression under autograd, the mask uploaded as floats and gathered at the step's pixels

and the losses alone, forward and backward on (512, 64) + (512, 96) weights: ms_losses_hip, ms_losses_torch.
Prints one JSON line.
    python tools/bench_opacity_loss.py --rounds 30"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu  # noqa: E402
from bench_mask_draw import disc_objects  # noqa: E402
from hip_util import model_conf  # noqa: E402

LAM_MASK, LAM_ALPHA, CLAMP_ALPHA = 0.1, 1e-3, 100.0


def timed(fn, rounds):
    """fn(i) to a synchronise, `rounds` times after three warm-up calls -> (median ms, spread ms)."""
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(rounds):
        t0 = time.perf_counter()
        fn(3 + i)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 4), round(max(ms) - min(ms), 4)


def torch_mask_loss(weights, mask_gt, lam):
    a = weights.sum(-1).clamp(0.01, 0.99)
    return lam * F.binary_cross_entropy(a, mask_gt)


def torch_alpha_loss(weights, lam, clamp_alpha):
    a = weights.sum(-1).clamp(0.01, 0.99)
    return lam * torch.clamp_min(torch.log(a) + torch.log(1.0 - a), -clamp_alpha).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--nv", type=int, default=50)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16x3"])
    a = ap.parse_args()
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, train, util
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.model.loss import AlphaLossNV2, MaskLoss, RenderLoss
    from pixel_nerf_multiscale_amd.optim import DeviceAdam
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    dev = torch.device("cuda")
    out = {"what": "opacity_loss", "objects": a.objects, "nv": a.nv, "image": f"{a.size}x{a.size}", "sb": a.sb, "rays_per_obj": a.rays,
           "precision": a.precision, "rounds": a.rounds, "lambda_mask": LAM_MASK, "lambda_alpha": LAM_ALPHA}

    items = disc_objects(a.objects, a.nv, a.size)
    ids = list(range(a.sb))
    data = ResidentSplit(items, dev, device_masks=True, device_boxes=True).batch(ids)
    masks_host = torch.stack([items[i]["masks"] for i in ids]).reshape(a.sb, -1).float().div_(255.0)     # the torch route's upload
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(dict(gu.CASES["full_ns1"]), "fp32")).cuda()
    net.train()
    net.train_precision = a.precision
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).cuda()
    rend.train()
    render_par = rend.bind_parallel(net, None)
    optim = DeviceAdam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    kw = dict(ray_batch_size=a.rays, nviews=[1], z_near=items.z_near, z_far=items.z_far, loss=RenderLoss(1.0, 1.0), balanced=True,
              draws="device")
    mask_loss, alpha_loss = MaskLoss(LAM_MASK, LAM_MASK), AlphaLossNV2(LAM_ALPHA, CLAMP_ALPHA, 0)

    def step(**more):
        def run(i):
            key = frame_seed(3, i)
            with rend.keyed(key):
                train.train_step(net, render_par, data, optim, seed=key, **kw, **more)
        return run

    def torch_step(i):
        key = frame_seed(3, i)
        seen = {}
        real = util.train_draw

        def spy(*args, **kwargs):                           # the step's pixels, where make_batch draws them
            res = real(*args, **kwargs)
            seen["pix"] = res[0]
            return res

        util.train_draw = spy
        try:
            optim.zero_grad()
            with rend.keyed(key):
                rays, rgb_gt, src_images, src_poses, focal, c = train.make_batch(data, dev, seed=key, **{k: v for k, v in kw.items() if k != "loss"})
                net.encode(src_images, src_poses, focal, c=c)
                render_dict = render_par(rays, want_weights=True)
        finally:
            util.train_draw = real
        total, _ = kw["loss"](render_dict, rgb_gt)
        mask_gt = util.upload(masks_host, dev).gather(1, seen["pix"])
        total = total + torch_mask_loss(render_dict["coarse"]["weights"], mask_gt, LAM_MASK) \
            + torch_mask_loss(render_dict["fine"]["weights"], mask_gt, LAM_MASK) \
            + torch_alpha_loss(render_dict["fine"]["weights"], LAM_ALPHA, CLAMP_ALPHA)
        optim.scale(total).backward()
        optim.step()

    for name, fn in (("plain", step()), ("mask", step(mask_loss=mask_loss)), ("mask_alpha", step(mask_loss=mask_loss, alpha_loss=alpha_loss)),
                     ("torch", torch_step), ("plain_again", step())):
        out[f"ms_step_{name}"], out[f"spread_ms_step_{name}"] = timed(fn, a.rounds)

    # the losses alone: value and gradient of mask BCE on both passes + the alpha loss on the fine pass
    n = a.sb * a.rays
    wc = (torch.rand(a.sb, a.rays, 64, device=dev) / 64).requires_grad_(True)
    wf = (torch.rand(a.sb, a.rays, 96, device=dev) / 96).requires_grad_(True)
    mask_gt = (torch.rand(a.sb, a.rays, device=dev) < 0.5).float()
    rd = {"coarse": {"weights": wc}, "fine": {"weights": wf}}

    def hip(i):
        wc.grad = wf.grad = None
        (mask_loss(rd, mask_gt)[0] + alpha_loss(wf)).backward()

    def eager(i):
        wc.grad = wf.grad = None
        (torch_mask_loss(wc, mask_gt, LAM_MASK) + torch_mask_loss(wf, mask_gt, LAM_MASK) + torch_alpha_loss(wf, LAM_ALPHA, CLAMP_ALPHA)).backward()

    out["loss_rays"] = n
    out["ms_losses_hip"], out["spread_ms_losses_hip"] = timed(hip, a.rounds)
    out["ms_losses_torch"], out["spread_ms_losses_torch"] = timed(eager, a.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
