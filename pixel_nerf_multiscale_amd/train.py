"""
The training step's front end on the device: Trainer.calc_losses of the reference (train/train.py:237-373) for this
package's classes.  The reference builds gen_rays for every view of every object, converts every image to [0, 1], keeps
ray_batch_size rows of each, and reads three loss values back; here the sampled pixel indices are uploaded once, one HIP
launch gathers their rays and colours (pnr_train_batch), and the loss leaves its three numbers on the device (pnr_rgb_loss).
"""
import numpy as np
import torch

from . import util


def make_batch(data, device, *, ray_batch_size, nviews, z_near, z_far, use_bbox=True, is_train=True):
    """The front end of calc_losses (train/train.py:243-317): host draws, ONE upload of the (SB, ray_batch_size) pixel
    indices (the source-view choice rides in the same buffer) and one of the intrinsics, both from pinned memory, one launch
    for the rays and colours, and the source views picked on the device.
    -> rays (SB, B, 8), rgb_gt (SB, B, 3), src_images (SB, NS, 3, H, W), src_poses (SB, NS, 4, 4), focal (SB, 2),
    c (SB, 2) or None — the last two on the device, for net.encode.  Never waits for the device.  See calc_losses for `data`
    and the order of the random draws."""
    all_images = util.upload(data["images"], device)
    all_poses = util.upload(data["poses"], device)
    SB, NV, _, H, W = all_images.shape
    all_bboxes = data.get("bbox") if (is_train and use_bbox) else None
    if all_bboxes is not None and all_bboxes.is_cuda:
        raise ValueError("data['bbox'] must be a host tensor: it steers host-side draws and is never read from the device")

    curr_nviews = nviews[int(torch.randint(0, len(nviews), ()))]
    B = int(ray_batch_size)
    host = torch.empty(SB * (B + curr_nviews), dtype=torch.long, pin_memory=True)
    pix_inds, image_ord = host[:SB * B].view(SB, B), host[SB * B:].view(SB, curr_nviews)
    if curr_nviews == 1:
        image_ord.copy_(torch.randint(0, NV, (SB, 1)))
    for obj in range(SB):
        if curr_nviews > 1:
            image_ord[obj] = torch.from_numpy(np.random.choice(NV, curr_nviews, replace=False))
        if all_bboxes is not None:
            pix = util.bbox_sample(all_bboxes[obj], B)
            pix_inds[obj] = pix[:, 0] * (H * W) + pix[:, 1] * W + pix[:, 2]
        else:
            pix_inds[obj] = torch.randint(0, NV * H * W, (B,))
    on_dev = host.to(device, non_blocking=True)
    pix_inds, image_ord = on_dev[:SB * B].view(SB, B), on_dev[SB * B:].view(SB, curr_nviews)

    # the loader's focal (SB,) or (SB, 2) and c (SB, 2): one (SB, 4) block, uploaded once
    focal = torch.as_tensor(data["focal"], dtype=torch.float32)
    c = data.get("c")
    focal = focal.reshape(-1, 2) if focal.dim() == 2 else focal.reshape(-1, 1)        # broadcasts to (SB, 2) below
    if focal.is_cuda or (c is not None and torch.as_tensor(c).is_cuda):
        focal = focal.to(device).expand(SB, 2)
        c = None if c is None else torch.as_tensor(c, dtype=torch.float32).to(device).reshape(-1, 2).expand(SB, 2)
    else:
        block = torch.empty(SB, 4, pin_memory=True)
        block[:, :2] = focal
        block[:, 2:] = 0.0 if c is None else torch.as_tensor(c, dtype=torch.float32).reshape(-1, 2)
        block = block.to(device, non_blocking=True)
        focal, c = block[:, :2], (None if c is None else block[:, 2:])
    focal = focal.contiguous()
    c = None if c is None else c.contiguous()

    rays, rgb_gt = util.train_batch(all_images, all_poses, focal, c, pix_inds, z_near, z_far)
    return (rays, rgb_gt, util.batched_index_select_nd(all_images, image_ord),
            util.batched_index_select_nd(all_poses, image_ord), focal, c)


def calc_losses(net, render_par, data, *, ray_batch_size, nviews, z_near, z_far, loss, use_bbox=True, is_train=True):
    """One batch of the data loader -> (loss, loss_dict), ready for loss.backward().

    net          PixelNeRFNet (on the device)
    render_par   renderer.bind_parallel(net, ...): (rays, want_weights=True) -> nested dict
    data         the loader's dict: images (SB, NV, 3, H, W) in [-1, 1], poses (SB, NV, 4, 4), focal (SB,) or (SB, 2),
                 optional c (SB, 2) and bbox (SB, NV, 4) = cmin, rmin, cmax, rmax.  bbox is read on the host (it steers
                 host-side draws), so it must be a host tensor, as the loader gives it.
    nviews       the source-view counts to draw from (the reference's --nviews list)
    loss         model.loss.RenderLoss
    use_bbox     the reference's self.use_bbox (its switch-off at args.no_bbox_step is the caller's schedule)

    loss_dict has "rc", "rf" (only with a fine pass) and "t".  Unlike the reference, which returns Python floats (three
    .item() calls, i.e. three host synchronisations per step), each value is a 0-dim view of ONE 3-float device buffer:
    the caller decides when to pay for .item() — e.g. only on the steps it prints.  Nothing in here waits for the device.

    Random draws follow the reference's order: curr_nviews and (for one view) image_ord from torch's global CPU
    generator, then per object the source views (numpy's global generator) and the pixels (util.bbox_sample, or a uniform
    randint without boxes / in evaluation).  Parity unpinned for that order: the reference's train.py cannot be imported
    (its data package is absent), so the order is followed by reading it.  Pinned by fixtures: bbox_sample's pixels, the index
    arithmetic, the gathered rays and colours (tests/golden/train_batch.npz)."""
    if "images" not in data:
        return {}
    dev = net.poses.device
    all_rays, all_rgb_gt, src_images, src_poses, focal, c = make_batch(
        data, dev, ray_batch_size=ray_batch_size, nviews=nviews, z_near=z_near, z_far=z_far, use_bbox=use_bbox, is_train=is_train)
    net.encode(src_images, src_poses, focal, c=c)

    render_dict = render_par(all_rays, want_weights=True)
    total, stats = loss(render_dict, all_rgb_gt)
    loss_dict = {"rc": stats[0]}
    fine = render_dict.get("fine")
    if fine is not None and len(fine) > 0:
        loss_dict["rf"] = stats[1]
    loss_dict["t"] = stats[2]
    return total, loss_dict


def train_step(net, render_par, data, optim, *, grad_hook=None, **calc_losses_kw):
    """Trainer.train_step of the reference (train/train.py:375-412) with both ends on the device: zero_grad, calc_losses,
    optim.scale(loss).backward(), grad_hook, optim.step().

    optim        optim.DeviceAdam: unscale, clip_grad_norm_, the found-inf skip, Adam and the scaler's update are its step()
    grad_hook    called with no arguments between backward and the step — the place for
                 parallel.allreduce_gradients(params); a gradient it replaces is re-adopted by optim.step()
    the rest     calc_losses' keywords (ray_batch_size, nviews, z_near, z_far, loss, use_bbox, is_train)

    -> calc_losses' loss_dict with "grad_norm" added (the fp64 norm of the unscaled gradients before clipping, what
    clip_grad_norm_ returns): 0-dim device views, like the others.  Nothing in here waits for the device; whether the step
    was applied is optim.found_inf, also on the device."""
    optim.zero_grad()
    out = calc_losses(net, render_par, data, **calc_losses_kw)
    if not out:
        return {}
    loss, loss_dict = out
    optim.scale(loss).backward()
    if grad_hook is not None:
        grad_hook()
    optim.step()
    loss_dict["grad_norm"] = optim.grad_norm
    return loss_dict
