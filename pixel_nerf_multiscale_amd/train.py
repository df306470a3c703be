"""
The training step's front end on the device: Trainer.calc_losses of the reference (train/train.py:237-373) for this
package's classes.  The reference builds gen_rays for every view of every object, converts every image to [0, 1], keeps
ray_batch_size rows of each, and reads three loss values back; here the sampled pixel indices are uploaded once, one HIP
launch gathers their rays and colours (pnr_train_batch), and the loss leaves its three numbers on the device (pnr_rgb_loss).
"""
import numpy as np
import torch

from . import util


def curr_nviews_for(nviews, seed):
    """The source-view count of the step keyed `seed` under device draws: nviews[seed % len(nviews)].  Computed on the host,
    because it fixes the shapes of the step."""
    return int(nviews[int(seed) % len(nviews)])


def make_batch(data, device, *, ray_batch_size, nviews, z_near, z_far, use_bbox=True, is_train=True, balanced=True,
               draws="host", seed=None, jitter=None, obj_base=0, prop_inside=None, want_mask=False):
    """The front end of calc_losses (train/train.py:243-317): host draws, ONE upload of the (SB, ray_batch_size) pixel
    indices (the source-view choice rides in the same buffer) and one of the intrinsics, both from pinned memory, one launch
    for the rays and colours, and the source views picked on the device.
    -> rays (SB, B, 8), rgb_gt (SB, B, 3), src_images (SB, NS, 3, H, W), src_poses (SB, NS, 4, 4), focal (SB, 2),
    c (SB, 2) or None — the last two on the device, for net.encode.  Never waits for the device.  See calc_losses for `data`
    and the order of the random draws.

    An 8-bit batch — data["images"] uint8 (SB, NV, H, W, 3 | 4), on the host or already on the device (data.ResidentSplit) —
    moves and keeps a quarter of the bytes: the same draws, then util.train_batch_u8 and util.views_to_tensor_u8 convert only
    the sampled pixels and the chosen source views, to the bits the float batch gives.  `balanced` names the float image such
    a batch stands for (the dataset's .balanced); a float batch ignores it.

    draws="device" with seed, the per-step key (parallel.frame_seed(base_seed, global_step)): no host draw and no index
    upload — curr_nviews = nviews[seed % len(nviews)], then ONE util.train_draw launch makes the pixel indices and the source
    views on the device from the key alone (include/pnr.h, pnr_train_draw), and the same gather calls follow.  The boxes are
    data["bbox_dev"] (data.ResidentSplit(device_boxes=True)) or data["bbox"] uploaded.  The batch of a step then depends on
    (seed) only, not on torch's and numpy's global generators, so a run resumed from a checkpoint sees the batches the
    uninterrupted run would have seen.  The stream is not the reference's, the distribution is (see pnr.h).

    jitter, a data.ColorJitter, with an 8-bit batch, draws="device" and is_train: upstream's colour augmentation where the
    bytes lie.  ONE util.color_jitter_plan launch keyed by the same seed draws a record per object (four factors, the order of
    the operations, the object's grey mean over all its views), and the two gathers apply it to the sampled pixels and the
    chosen source views only: no host read and no further upload.  The record depends on (seed) and the bytes alone, so
    checkpoints need nothing new.  A float batch or draws="host" with jitter raises ValueError; is_train=False ignores it;
    None makes the calls made without it.

    obj_base (draws="device" only; ValueError with host draws): `data` holds objects obj_base .. obj_base + SB - 1 of the
    step's batch — a rank's share of a data-parallel step.  The pixel draw, the view draw and the jitter record of its object
    o are keyed as object obj_base + o (pnr_train_draw_at, pnr_color_jitter_plan_at), so the six outputs are rows
    obj_base .. obj_base + SB - 1 of the whole batch's outputs, bit for bit.

    prop_inside, a number in [0, 1], with is_train and use_bbox: the object's MASK takes the place of its boxes — of an object's
    ray_batch_size pixels util.num_inside(ray_batch_size, prop_inside) are uniform over its foreground and the rest over its
    background, all views pooled (the reference's util.masked_sample).  draws="device": the bit table comes from
    data["mask_bits"] / data["mask_rows"] (data.ResidentSplit(device_masks=True)), else it is built from data["masks"]
    (uploaded when on the host) by one util.mask_table call, and ONE util.train_draw_masked launch keyed by the seed takes the
    place of util.train_draw; an object without foreground (or without background) draws every pixel from what it has.
    draws="host": util.masked_sample per object where util.bbox_sample stood, and such an object raises ValueError.  uint8
    masks are inside at >= 128, float masks at >= 0.5.  A batch with neither table nor masks raises ValueError; is_train=False
    or use_bbox=False ignore prop_inside; None (the default) makes the calls made without it.

    want_mask=True: a seventh value, mask_gt (SB, B) float32 — 1.0 where the ray's pixel lies on the object's mask, else 0.0 (the
    ground truth of model.loss.MaskLoss), read by ONE util.mask_gather launch from the bit table: data["mask_bits"] when present,
    else the table built from data["masks"] (uploaded when on the host) — the one prop_inside draws from; it is built at most
    once per step.  Training or not, host or device draws.  A batch with neither raises ValueError.  False (the default)
    returns exactly the six values above."""
    if draws not in ("host", "device"):
        raise ValueError(f"draws must be 'host' or 'device', got {draws!r}")
    obj_base = int(obj_base)
    if obj_base != 0 and draws != "device":
        raise ValueError("obj_base needs draws='device': only the keyed draws can place a slice inside its step's batch")
    if obj_base < 0:
        raise ValueError(f"obj_base must be >= 0, got {obj_base}")
    if draws == "device" and seed is None:
        raise ValueError("draws='device' needs seed, the per-step key: parallel.frame_seed(base_seed, global_step)")
    as_bytes = data["images"].dtype == torch.uint8
    if not is_train:
        jitter = None
    if jitter is not None and not (as_bytes and draws == "device"):
        raise ValueError("jitter needs an 8-bit batch (uint8 images) and draws='device': the augmentation runs on the device, "
                         "keyed by the step's seed")
    if as_bytes and (data["images"].dim() != 5 or data["images"].shape[-1] not in (3, 4)):
        raise ValueError(f"a uint8 batch must be (SB, NV, H, W, 3 | 4), got {tuple(data['images'].shape)}")
    B = int(ray_batch_size)
    by_mask = prop_inside is not None and is_train and use_bbox
    if by_mask:
        util.num_inside(B, prop_inside)                 # ValueError outside [0, 1], before anything is moved or drawn
        if data.get("masks") is None and not (draws == "device" and data.get("mask_bits") is not None
                                              and data.get("mask_rows") is not None):
            raise ValueError("prop_inside needs the batch's masks: data['masks'], or data['mask_bits'] and data['mask_rows'] "
                             "(data.ResidentSplit(device_masks=True)) under draws='device'")
    if want_mask and data.get("masks") is None and data.get("mask_bits") is None:
        raise ValueError("want_mask needs the batch's masks: data['masks'], or data['mask_bits'] "
                         "(data.ResidentSplit(device_masks=True))")
    all_images = util.upload(data["images"], device)
    all_poses = util.upload(data["poses"], device)
    table = []

    def mask_tables():
        """(bits, rows) of the step's objects: the batch's own, or built from its masks — once, whoever asks first."""
        if not table:
            bits, rows = data.get("mask_bits"), data.get("mask_rows")
            if data.get("masks") is not None and (bits is None or rows is None):
                bits, rows = util.mask_table(util.mask_bytes(util.upload(data["masks"], device)))
            table.append((bits, rows))
        return table[0]

    def with_mask(out, pix_inds):
        return out + (util.mask_gather(mask_tables()[0], pix_inds, NV, H, W),) if want_mask else out
    if as_bytes:
        SB, NV, H, W, _ = all_images.shape
    else:
        SB, NV, _, H, W = all_images.shape
    if draws == "device":
        boxes = None
        if is_train and use_bbox and not by_mask:
            boxes = data.get("bbox_dev")
            if boxes is None and data.get("bbox") is not None:
                boxes = util.upload(torch.as_tensor(data["bbox"], dtype=torch.float32), device)
        if boxes is not None:
            boxes = boxes.to(device=device, dtype=torch.float32)
        out_pix = torch.empty(SB, B, dtype=torch.long, device=device)
        if by_mask:
            bits, rows = mask_tables()
            pix_inds, image_ord = util.train_draw_masked(bits, rows, SB, NV, W, H, B, curr_nviews_for(nviews, seed), seed,
                                                         prop_inside, out_pix=out_pix, obj_base=obj_base)
        else:
            pix_inds, image_ord = util.train_draw(boxes, SB, NV, W, H, B, curr_nviews_for(nviews, seed), seed,
                                                  out_pix=out_pix, obj_base=obj_base)
        record = None if jitter is None else util.color_jitter_plan(all_images, jitter, seed, obj_base=obj_base)
        return with_mask(_gather_batch(data, device, all_images, all_poses, pix_inds, image_ord, z_near, z_far, balanced, record),
                         pix_inds)

    all_bboxes = data.get("bbox") if (is_train and use_bbox) else None
    if all_bboxes is not None and all_bboxes.is_cuda:
        raise ValueError("data['bbox'] must be a host tensor: it steers host-side draws and is never read from the device")
    if by_mask:
        all_masks = data["masks"]
        if all_masks.is_cuda:
            raise ValueError("data['masks'] must be a host tensor under draws='host': it steers host-side draws")
        mask_thresh = 128 if all_masks.dtype == torch.uint8 else 0.5

    curr_nviews = nviews[int(torch.randint(0, len(nviews), ()))]
    host = torch.empty(SB * (B + curr_nviews), dtype=torch.long, pin_memory=True)
    pix_inds, image_ord = host[:SB * B].view(SB, B), host[SB * B:].view(SB, curr_nviews)
    if curr_nviews == 1:
        image_ord.copy_(torch.randint(0, NV, (SB, 1)))
    for obj in range(SB):
        if curr_nviews > 1:
            image_ord[obj] = torch.from_numpy(np.random.choice(NV, curr_nviews, replace=False))
        if by_mask:
            pix = util.masked_sample(all_masks[obj], B, prop_inside, thresh=mask_thresh)
            pix_inds[obj] = pix[:, 0] * (H * W) + pix[:, 1] * W + pix[:, 2]
        elif all_bboxes is not None:
            pix = util.bbox_sample(all_bboxes[obj], B)
            pix_inds[obj] = pix[:, 0] * (H * W) + pix[:, 1] * W + pix[:, 2]
        else:
            pix_inds[obj] = torch.randint(0, NV * H * W, (B,))
    on_dev = host.to(device, non_blocking=True)
    pix_inds, image_ord = on_dev[:SB * B].view(SB, B), on_dev[SB * B:].view(SB, curr_nviews)
    return with_mask(_gather_batch(data, device, all_images, all_poses, pix_inds, image_ord, z_near, z_far, balanced), pix_inds)


def _gather_batch(data, device, all_images, all_poses, pix_inds, image_ord, z_near, z_far, balanced, jitter=None):
    """make_batch behind its draws: the intrinsics' upload, the rays and colours of pix_inds (SB, B), the source views and
    poses of image_ord (SB, NS).  jitter: the colour-jitter record (SB, 8) of an 8-bit batch, or None."""
    as_bytes = all_images.dtype == torch.uint8
    SB = all_images.shape[0]
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

    if as_bytes:
        kw = {} if jitter is None else {"jitter": jitter}
        rays, rgb_gt = util.train_batch_u8(all_images, all_poses, focal, c, pix_inds, z_near, z_far, balanced=balanced, **kw)
        src_images = util.views_to_tensor_u8(all_images, image_ord, balanced=balanced, **kw)
    else:
        rays, rgb_gt = util.train_batch(all_images, all_poses, focal, c, pix_inds, z_near, z_far)
        src_images = util.batched_index_select_nd(all_images, image_ord)
    return rays, rgb_gt, src_images, util.batched_index_select_nd(all_poses, image_ord), focal, c


def calc_losses(net, render_par, data, *, ray_batch_size, nviews, z_near, z_far, loss, use_bbox=True, is_train=True,
                balanced=True, draws="host", seed=None, jitter=None, obj_base=0, prop_inside=None, alpha_loss=None, mask_loss=None):
    """One batch of the data loader -> (loss, loss_dict), ready for loss.backward().

    net          PixelNeRFNet (on the device)
    render_par   renderer.bind_parallel(net, ...): (rays, want_weights=True) -> nested dict
    data         the loader's dict: images (SB, NV, 3, H, W) in [-1, 1], poses (SB, NV, 4, 4), focal (SB,) or (SB, 2),
                 optional c (SB, 2) and bbox (SB, NV, 4) = cmin, rmin, cmax, rmax.  bbox is read on the host (it steers
                 host-side draws), so it must be a host tensor, as the loader gives it.  images may instead be the files'
                 bytes, uint8 (SB, NV, H, W, 3 | 4) on the host or the device (an as_bytes dataset of the data package, or
                 data.ResidentSplit.batch): see make_batch.
    balanced     for an 8-bit batch, the dataset's .balanced: whether its float images would lie in [-1, 1] (True) or
                 [0, 1]; ignored for a float batch
    nviews       the source-view counts to draw from (the reference's --nviews list)
    loss         model.loss.RenderLoss
    use_bbox     the reference's self.use_bbox (its switch-off at args.no_bbox_step is the caller's schedule)
    draws, seed  "host" (the default): the draws below; "device" with seed = the per-step key: make_batch's keyed draws on
                 the device, which consume neither global generator
    jitter       None, or a data.ColorJitter: the colour augmentation of make_batch (8-bit batch, draws="device", training
                 only — is_train=False ignores it)
    obj_base     draws="device" only: `data` is the slice [obj_base, obj_base + SB) of the step's batch (make_batch), and the
                 render runs with the renderer's ray_index_base = obj_base * ray_batch_size, so its keyed noise is that of
                 those rays of the whole batch's render.  The loss is the mean over the slice's own rays.
    prop_inside  None, or the share of an object's rays that falls on its mask's foreground: make_batch's mask-weighted draws
                 in place of the boxes (needs data["masks"], or the tables of data.ResidentSplit(device_masks=True); training
                 only, and only while use_bbox is on)
    alpha_loss   None, or a model.loss.AlphaLossNV2: applied to the fine pass's weights when there is one, else to the coarse
                 pass's (the reference's alpha_fine); its own epoch gate decides whether anything is launched
    mask_loss    None, or a model.loss.MaskLoss: make_batch(want_mask=True) gathers the mask at the step's pixels (the batch
                 needs "masks", or the tables of data.ResidentSplit(device_masks=True)), and the loss supervises both passes.
                 Both losses are added to the total on the device, in validation (is_train=False) too; loss_dict gains "a" / "m"
                 (0-dim device views) only for the losses given, and "t" is then the sum.  With both None every call made
                 without them is made unchanged.

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
    batch = make_batch(
        data, dev, ray_batch_size=ray_batch_size, nviews=nviews, z_near=z_near, z_far=z_far, use_bbox=use_bbox, is_train=is_train,
        balanced=balanced, draws=draws, seed=seed, jitter=jitter, obj_base=obj_base,
        **({} if prop_inside is None else {"prop_inside": prop_inside}), **({} if mask_loss is None else {"want_mask": True}))
    all_rays, all_rgb_gt, src_images, src_poses, focal, c = batch[:6]
    net.encode(src_images, src_poses, focal, c=c)

    if obj_base:
        rend = render_par.renderer
        with rend.keyed(rend.forced_seed, base=int(obj_base) * int(ray_batch_size)):
            render_dict = render_par(all_rays, want_weights=True)
    else:
        render_dict = render_par(all_rays, want_weights=True)
    total, stats = loss(render_dict, all_rgb_gt)
    loss_dict = {"rc": stats[0]}
    fine = render_dict.get("fine")
    if fine is not None and len(fine) > 0:
        loss_dict["rf"] = stats[1]
    loss_dict["t"] = stats[2]
    if mask_loss is not None:
        m_total, m_stats = mask_loss(render_dict, batch[6])
        total = total + m_total
        loss_dict["m"] = m_stats[2]
    if alpha_loss is not None:
        has_fine = fine is not None and len(fine) > 0
        a_total = alpha_loss((fine if has_fine else render_dict["coarse"])["weights"])
        if getattr(alpha_loss, "active", True):          # an inactive loss is a cached zero: nothing to add, nothing launched
            total = total + a_total
        loss_dict["a"] = a_total.detach()
    if mask_loss is not None or alpha_loss is not None:
        loss_dict["t"] = total.detach()
    return total, loss_dict


def train_step(net, render_par, data, optim, *, grad_hook=None, **calc_losses_kw):
    """Trainer.train_step of the reference (train/train.py:375-412) with both ends on the device: zero_grad, calc_losses,
    optim.scale(loss).backward(), grad_hook, optim.step().

    optim        optim.DeviceAdam: unscale, clip_grad_norm_, the found-inf skip, Adam and the scaler's update are its step()
    grad_hook    called with no arguments between backward and the step — the place for
                 parallel.allreduce_gradients(params); a gradient it replaces is re-adopted by optim.step()
                 — and for optim.allreduce, DeviceAdam's own all-reduce of its flat gradient buffer (one collective; the
                 mean's divide is folded into the step)
    the rest     calc_losses' keywords (ray_batch_size, nviews, z_near, z_far, loss, use_bbox, is_train, jitter, obj_base,
                 prop_inside, alpha_loss, mask_loss)

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


def eval_step(net, renderer, render_par, data, **calc_losses_kw):
    """Trainer.eval_step of the reference (train/train.py:414-421): calc_losses(..., is_train=False) under torch.no_grad()
    with the renderer in eval mode -> the loss_dict ("rc", "rf" with a fine pass, "t"; "a" / "m" with alpha_loss / mask_loss), the part Trainer.validate consumes,
    its values still on the device; {} for a batch without images.  The reference ends with an unconditional
    renderer.train(); this RESTORES the mode the renderer was in instead.  Nothing in here waits for the device."""
    calc_losses_kw.pop("is_train", None)
    was_training = renderer.training
    renderer.eval()
    try:
        with torch.no_grad():
            out = calc_losses(net, render_par, data, is_train=False, **calc_losses_kw)
    finally:
        renderer.train(was_training)
    return out[1] if out else {}


def validate(net, renderer, render_par, loader, **calc_losses_kw):
    """Trainer.validate of the reference (train/trainlib/trainer.py:404-460): the mean of loss_dict["t"] over the loader's
    batches with the net in eval mode, skipping None batches (a failed collate) and batches without "images"; float("inf")
    when no batch counts.  The reference reads three values per batch back; here "t" is accumulated where eval_step left it
    (on the device) and the mean is read ONCE at the end.  The net's mode is restored, where the reference calls net.train().
    Its progress bar, its TensorBoard scalar and its skipping of batches that raise RuntimeError are the caller's."""
    was_training = net.training
    net.eval()
    total, count = None, 0
    try:
        for data in loader:
            if data is None or not data or "images" not in data:
                continue
            loss_dict = eval_step(net, renderer, render_par, data, **calc_losses_kw)
            if "t" not in loss_dict:
                continue
            t = torch.as_tensor(loss_dict["t"]).detach().double()
            total = t if total is None else total + t
            count += 1
    finally:
        net.train(was_training)
    if count == 0:
        return float("inf")
    return float(total) / count


def draw_vis_views(NV, nviews):
    """The view draws of vis_step in the reference's order (train/train.py:446-450): curr_nviews from torch's global CPU
    generator, the sorted source views and the target view from numpy's; the target is drawn among the NV - curr_nviews views
    that are left and pushed past the sources.  -> (views_src sorted int64 array, view_dest).  ValueError for more sources
    than a panel holds or for no view left over."""
    from ._native import PNR_VIS_MAX_SRC
    curr_nviews = int(nviews[torch.randint(0, len(nviews), (1,)).item()])
    if curr_nviews > PNR_VIS_MAX_SRC:
        raise ValueError(f"vis_step draws at most {PNR_VIS_MAX_SRC} source views, got nviews entry {curr_nviews}")
    if curr_nviews >= NV:
        raise ValueError(f"vis_step needs a target view besides the {curr_nviews} source views, the object has {NV}")
    views_src = np.sort(np.random.choice(NV, curr_nviews, replace=False))
    view_dest = int(np.random.randint(0, NV - curr_nviews))
    for vs in range(curr_nviews):
        view_dest += int(view_dest >= views_src[vs])
    return views_src, view_dest


def vis_step(net, renderer, render_par, data, *, nviews, z_near, z_far, idx=None, lut=None, out="float", verbose=False):
    """Trainer.vis_step of the reference (train/train.py:423-537): one object of the batch, curr_nviews of its views as
    sources, one other view rendered, and the picture a run is judged by — per pass [source views | ground truth | depth map
    | rendered colours | opacity map], coarse row over fine row — plus the view's PSNR.

    The reference generates rays for all NV views to use one, copies seven arrays to the host and colour-maps, stacks and
    measures there.  Here only the target view's rays are made (util.gen_rays_device), the render runs under torch.no_grad()
    with the renderer in eval mode, and ONE util.vis_panel call (pnr_vis_panel) builds panel and PSNR on the device.

    data       the loader's dict (host tensors): images (SB, NV, 3, H, W) in [-1, 1], poses, focal, optional c
    nviews     the source-view counts to draw from; idx: the object, else drawn
    lut        (256, 3) uint8 colour table; None = util.hot_lut() (parity unpinned, see there)
    out        "float": the float32 panel (n_pass H, (NS + 4) W, 3); "uint8": the same as bytes
    -> (vis, {"psnr": 0-dim float64 device tensor}); {} for a batch without images.

    Draws in the reference's order: batch_idx from np.random.randint unless idx is given, then draw_vis_views.  Parity for
    that order is unpinned, as calc_losses says for its own draws.  The renderer's mode is RESTORED afterwards (the reference
    calls renderer.train()).  verbose=True prints the reference's min / max lines and the PSNR, at the cost of one host read;
    with verbose=False the call waits for the device only if data["poses"] is a device tensor (the camera is read on the host)."""
    if "images" not in data:
        return {}
    if out not in ("float", "uint8"):
        raise ValueError(f"out must be 'float' or 'uint8', got {out!r}")
    batch_idx = int(np.random.randint(0, data["images"].shape[0])) if idx is None else int(idx)
    dev = net.poses.device
    NV, _, H, W = data["images"][batch_idx].shape
    views_src, view_dest = draw_vis_views(NV, nviews)
    images = util.upload(data["images"][batch_idx].float().contiguous(), dev)        # (NV, 3, H, W)
    poses = data["poses"][batch_idx].float()
    focal = torch.as_tensor(data["focal"], dtype=torch.float32)[batch_idx:batch_idx + 1]
    c = data.get("c")
    if c is not None:
        c = torch.as_tensor(c, dtype=torch.float32)[batch_idx:batch_idx + 1]
    src_idx = torch.from_numpy(views_src)
    rays = util.gen_rays_device(poses[view_dest], W, H, focal[0], z_near, z_far, c=None if c is None else c[0], device=dev)
    src_images = images.index_select(0, util.upload(src_idx, dev))                    # (NS, 3, H, W)
    was_training = renderer.training
    renderer.eval()
    try:
        with torch.no_grad():
            net.encode(src_images.unsqueeze(0), util.upload(poses[src_idx].contiguous(), dev).unsqueeze(0),
                       util.upload(focal, dev), c=None if c is None else util.upload(c, dev))
            render_dict = render_par(rays[None], want_weights=True)
            passes = [render_dict["coarse"]]
            fine = render_dict.get("fine")
            if fine is not None and len(fine) > 0:
                passes.append(fine)
            res = util.vis_panel(images, views_src, view_dest,
                                 [(p["rgb"][0], p["depth"][0], p["weights"][0]) for p in passes],
                                 lut=lut, want_f32=out == "float", want_u8=out == "uint8")
    finally:
        renderer.train(was_training)
    if verbose:
        stats = res.stats.cpu().tolist()
        for tag, s in zip("cf", stats):
            print("{} rgb min {} max {}".format(tag, s[0], s[1]))
            print("{} alpha min {}, max {}".format(tag, s[2], s[3]))
        print("psnr", float(res.psnr))
    return (res.panel if out == "float" else res.panel_u8), {"psnr": res.psnr}


def __getattr__(name):
    """train.Trainer is trainer.Trainer, the epoch loop over the functions above (looked up on first use: trainer imports
    this module)."""
    if name == "Trainer":
        from .trainer import Trainer
        return Trainer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
