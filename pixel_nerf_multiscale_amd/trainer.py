"""
The training loop: trainlib.Trainer (train/trainlib/trainer.py) and its PixelNeRFTrainer subclass (train/train.py:178-235) of
the reference, restated over this package's pieces — train.train_step / validate / vis_step, optim.DeviceAdam, the data layer —
with plain keywords in place of argparse and HOCON.

What differs from the reference, on purpose:
  * every random choice of a step is keyed by (seed, global_step): the epoch's permutation by (seed, epoch), the batch draws
    (draws="device": pnr_train_draw) and the render noise (renderer.keyed) by parallel.frame_seed(seed, global_step).  A run
    resumed from a checkpoint therefore continues bit for bit as the uninterrupted run would have.  draws="host" keeps the
    reference's draws from torch's and numpy's global generators, and the render noise from torch's, unkeyed;
  * the loop reads the device only every print_interval steps and at the end of an epoch (one host read each time); the
    reference reads three values at every step;
  * with freeze_enc the encoder is put back into eval() after every net.train() (the reference's train_epoch switches its
    frozen encoder's BatchNorm back to training);
  * a resumed run steps the LR scheduler up to the epoch it resumes at (the reference saves latest.pth before the epoch's
    scheduler step, so its resumed run trains one epoch at the previous rate);
  * no TensorBoard and no tqdm: `writer` is any object with add_scalar / add_image, the log goes through print;
  * data_parallel: ONE global batch per step, cut over the ranks of a process group.  Every draw of a step is keyed by the
    object's place in the GLOBAL batch (train.make_batch's obj_base), the render noise by the global ray index, the gradients
    are summed with one collective over DeviceAdam's flat buffer and divided inside the step's kernels: hyper-parameters,
    step count, schedules and checkpoints do not depend on the number of ranks.  See Trainer's docstring for what does.
"""
import os
import re
import time

import torch

from . import train, util
from .optim import DeviceAdam
from .parallel import frame_seed

LR_POLICIES = ("none", "step", "multistep")
SAVE_STRATEGIES = ("keep_last", "keep_all", "milestone")
_EPOCH_FILE = re.compile(r"^epoch_(\d+)\.pth$")


def checkpoints_to_remove(names, strategy, keep_last, current_epoch):
    """The rotation of trainer.py:493-551 as a pure function: which of the file names `names` of a checkpoint folder go.
    Only epoch_<digits>.pth files are candidates — latest.pth, best.pth, _renderer and anything else stay.
      keep_last   keeps the lexicographically last keep_last epoch files
      milestone   keeps epochs <= 10, multiples of 5 up to 100, multiples of 20 beyond, and current_epoch
      keep_all    keeps everything"""
    if strategy not in SAVE_STRATEGIES:
        raise ValueError(f"save_strategy must be one of {SAVE_STRATEGIES}, got {strategy!r}")
    files = sorted(n for n in names if _EPOCH_FILE.match(n))
    if strategy == "keep_all":
        return []
    if strategy == "keep_last":
        keep_last = int(keep_last)
        return files[:len(files) - keep_last] if len(files) > keep_last else []
    out = []
    for n in files:
        e = int(_EPOCH_FILE.match(n).group(1))
        if not (e <= 10 or (e <= 100 and e % 5 == 0) or (e > 100 and e % 20 == 0) or e == current_epoch):
            out.append(n)
    return out


def epoch_permutation(n, seed, epoch):
    """The order of epoch `epoch`: torch.randperm under a generator of its own seeded with frame_seed(seed, epoch), so it
    depends on (seed, epoch) alone — not on what ran before, and not on torch's global generator."""
    return torch.randperm(int(n), generator=torch.Generator().manual_seed(frame_seed(seed, epoch)))


def rank_slice(batch_size, world, rank):
    """Rank `rank` of `world` takes objects [first, first + m) of every global batch of batch_size objects: -> (first, m) with
    m = batch_size / world, first = rank * m.  ValueError when the batch does not divide."""
    batch_size, world, rank = int(batch_size), int(world), int(rank)
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"rank {rank} of {world} ranks")
    if batch_size < 1 or batch_size % world != 0:
        raise ValueError(f"batch_size {batch_size} does not divide over {world} ranks: a data-parallel step cuts ONE global "
                         "batch into equal shares")
    m = batch_size // world
    return rank * m, m


def rank_epoch_order(order, batch_size, world, rank):
    """The objects rank `rank` loads in an epoch whose global order is `order` (epoch_permutation(...).tolist()): of every whole
    global batch order[b * batch_size : (b + 1) * batch_size] its slice rank_slice(...), batch after batch (drop_last).  The
    ranks' lists, interleaved m at a time in rank order, give back the global order's whole batches."""
    first, m = rank_slice(batch_size, world, rank)
    order = list(order)
    out = []
    for b in range(len(order) // int(batch_size)):
        at = b * int(batch_size) + first
        out.extend(order[at:at + m])
    return out


def rank_val_batches(n, batch_size, world, rank):
    """Validation under `world` ranks: the n objects in order, in batches of batch_size (the last one shorter); batch i belongs to
    rank i % world.  -> the rank's batches as lists of object indices."""
    batches = [list(range(i, min(i + int(batch_size), int(n)))) for i in range(0, int(n), int(batch_size))]
    return batches[int(rank)::int(world)]


class _EpochOrder(torch.utils.data.Sampler):
    """The DataLoader's sampler: the permutation the Trainer sets before every epoch."""

    def __init__(self, n):
        self.order = list(range(n))

    def __iter__(self):
        return iter(self.order)

    def __len__(self):
        return len(self.order)


def _is_resident(data):
    return hasattr(data, "batches") and hasattr(data, "batch")


class Trainer:
    """Trainer(net, renderer, train_data, val_data, name=..., checkpoints_path=..., logs_path=..., batch_size=...,
    ray_batch_size=..., nviews=[...], loss=RenderLoss(...)).start()

    net, renderer      PixelNeRFNet and NeRFRenderer on the device
    train_data, val_data   a dataset (wrapped in a DataLoader: the epoch's permutation, drop_last=True, num_workers=0; the
                       validation loader in order, batch size min(batch_size, 4), as the reference's) or a data.ResidentSplit
    num_epochs 100, lr 1e-4, lr_policy "none" | "step" | "multistep" with gamma 0.1, step_size 10000, milestones — torch's
                       StepLR / MultiStepLR on DeviceAdam's one param group, stepped once per epoch as the reference does
    grad_clip, scaler  DeviceAdam's max_norm and scaler dict
    no_bbox_step       steps with global_step >= no_bbox_step draw their pixels from the whole image
    freeze_enc         the encoder's parameters are left out of the optimiser, its latents detached, the encoder in eval()
    seed, draws        the base of every key; "device" (pnr_train_draw) or "host" — see the module text
    jitter             None or a data.ColorJitter: training steps augment their 8-bit batch's colours on the device, keyed like
                       the draws (train.make_batch); needs draws="device"; validation and the picture never see it
    prop_inside        None or a number in [0, 1]: training steps draw that share of an object's rays on its mask's foreground and
                       the rest on its background (train.make_batch) where they would draw inside its boxes — so no_bbox_step
                       ends it too; the batches need "masks", or a data.ResidentSplit(device_masks=True); keyed like every
                       draw under draws="device", so a checkpoint needs nothing new; validation never sees it
    alpha_loss         None or a model.loss.AlphaLossNV2: added to every step's and every validation batch's loss (train.calc_losses);
                       its epoch gate is set from the Trainer's own counter at every epoch's start (set_epoch), so a checkpoint
                       needs nothing new; logged as "a"
    mask_loss          None or a model.loss.MaskLoss: the silhouette loss against the batches' masks ("masks", or a
                       data.ResidentSplit(device_masks=True)), training and validation; logged as "m".  Under data_parallel both
                       are the mean over the rank's own rays, as the rgb loss is.  With both None every call is made unchanged.
    print_interval (steps), save_interval / eval_interval / vis_interval (epochs), keep_last_checkpoints, save_strategy
    resume             False, True (latest.pth of this run if it exists) or a path (FileNotFoundError if missing)
    writer             None or an object with add_scalar(tag, value, step) / add_image(tag, hwc_uint8, step, dataformats="HWC")
    z_near, z_far      default: the training data's
    data_parallel      False: one process on one device — under a process group of several ranks the constructor refuses.
                       True: the default process group; a ProcessGroup: that group.  No initialised group, or a group of one
                       rank, is the loop of one process.  With W ranks, rank r takes objects [r m, (r + 1) m), m = batch_size / W,
                       of every global batch (obj_base = r m; a DataLoader rank decodes only its own objects, a ResidentSplit
                       rank gathers only its own), steps with optimizer.allreduce(group) in train_step's grad_hook slot, and
                       renderer.sched_step(batch_size), no_bbox_step, the LR schedule and global_step are those of one process.
                       ValueError on every rank, before anything is allocated, for batch_size % W != 0 and for draws="host".
                       Parameters and buffers are broadcast from rank 0 at construction (a resumed run: every rank reads the
                       file).  Rank 0 alone prints, feeds `writer`, draws the picture and writes checkpoints (a barrier follows
                       every save); printed values are the ranks' mean (one collective per print step, one for the epoch's
                       average); validation batch i belongs to rank i % W and ONE collective carries the fp64 sum and the
                       count, so every rank takes the same best.pth decision.  The checkpoint notes world_size for the reader
                       only: one written under W ranks resumes under any other W.
                       BatchNorm: an encoder that trains normalises over the rank's OWN images (torch's DDP default; there is
                       no SyncBatchNorm here), and at the end of every epoch, before saving, the net's buffers are broadcast
                       from rank 0 in one collective.  So the run is independent of W — up to the rounding of the gradient
                       sum — only with freeze_enc=True or an encoder without batch statistics.

    Checkpoints (<checkpoints_path>/<name>/): epoch_%04d.pth, latest.pth (holding epoch + 1), best.pth — torch.save dicts with
    epoch, iter, global_step, net_state_dict, optimizer_state_dict (DeviceAdam's, which carries the loss scale), best_val_loss,
    seed and scheduler_state_dict when there is a scheduler — and _renderer, the renderer's state_dict, written at every save.
    The training render runs under renderer.keyed(key): its noise is the in-kernel generator's under that seed."""

    def __init__(self, net, renderer, train_data, val_data, *, name, checkpoints_path, logs_path, batch_size, ray_batch_size,
                 nviews, loss, num_epochs=100, lr=1e-4, lr_policy="none", gamma=0.1, step_size=10000, milestones=(10000, 20000),
                 grad_clip=None, scaler=None, no_bbox_step=100000, freeze_enc=False, seed=0, draws="device", print_interval=10,
                 save_interval=1, eval_interval=10, vis_interval=10, keep_last_checkpoints=20, save_strategy="keep_last",
                 resume=False, writer=None, z_near=None, z_far=None, jitter=None, data_parallel=False, prop_inside=None,
                 alpha_loss=None, mask_loss=None):
        import torch.distributed as dist
        self.group, self.world, self.rank = None, 1, 0
        if data_parallel is not False and data_parallel is not None and dist.is_available() and dist.is_initialized():
            self.group = None if data_parallel is True else data_parallel
            self.world, self.rank = dist.get_world_size(self.group), dist.get_rank(self.group)
        elif dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError(
                "Trainer runs one process on one device; under a process group of "
                f"{dist.get_world_size()} ranks write the loop by hand around train.train_step with "
                "grad_hook=lambda: parallel.allreduce_gradients(params)")
        if lr_policy not in LR_POLICIES:
            raise ValueError(f"lr_policy must be one of {LR_POLICIES}, got {lr_policy!r}")
        if save_strategy not in SAVE_STRATEGIES:
            raise ValueError(f"save_strategy must be one of {SAVE_STRATEGIES}, got {save_strategy!r}")
        if draws not in ("host", "device"):
            raise ValueError(f"draws must be 'host' or 'device', got {draws!r}")
        if jitter is not None and draws != "device":
            raise ValueError("jitter needs draws='device': the augmentation is keyed by the step's seed on the device")
        self.obj_base, self.rank_batch = rank_slice(batch_size, self.world, self.rank)
        if self.world > 1 and draws != "device":
            raise ValueError("data_parallel needs draws='device': a rank's share of the batch is placed by the keyed draws")
        if isinstance(resume, (str, os.PathLike)) and not os.path.exists(resume):
            raise FileNotFoundError(f"checkpoint not found: {os.fspath(resume)}")
        self.net, self.renderer, self.name = net, renderer, name
        self.train_data, self.val_data = train_data, val_data
        self.batch_size, self.ray_batch_size, self.nviews, self.loss = int(batch_size), int(ray_batch_size), list(nviews), loss
        self.num_epochs, self.lr, self.lr_policy = int(num_epochs), float(lr), lr_policy
        self.no_bbox_step, self.freeze_enc, self.seed, self.draws = int(no_bbox_step), bool(freeze_enc), int(seed), draws
        self.print_interval, self.save_interval = max(int(print_interval), 1), max(int(save_interval), 1)
        self.eval_interval, self.vis_interval = max(int(eval_interval), 1), max(int(vis_interval), 1)
        self.keep_last_checkpoints, self.save_strategy, self.writer = int(keep_last_checkpoints), save_strategy, writer
        self.z_near = float(train_data.z_near if z_near is None else z_near)
        self.z_far = float(train_data.z_far if z_far is None else z_far)
        self.balanced = bool(getattr(train_data, "balanced", True))
        self.jitter = jitter
        if prop_inside is not None:
            util.num_inside(self.ray_batch_size, prop_inside)       # ValueError outside [0, 1]
        self.prop_inside = None if prop_inside is None else float(prop_inside)
        self.alpha_loss, self.mask_loss = alpha_loss, mask_loss
        self.device = next(net.parameters()).device

        self.log_dir = os.path.join(logs_path, name)
        self.checkpoint_dir = os.path.join(checkpoints_path, name)
        self.renderer_state_path = os.path.join(self.checkpoint_dir, "_renderer")
        if self.rank == 0:
            os.makedirs(self.log_dir, exist_ok=True)
            os.makedirs(self.checkpoint_dir, exist_ok=True)
        if self.world > 1:
            self._broadcast(list(net.parameters()) + self._state_buffers())

        frozen = set()
        if self.freeze_enc:
            net.stop_encoder_grad = True
            net.encoder.eval()
            frozen = {id(p) for p in net.encoder.parameters()}
        self.params = [p for p in net.parameters() if p.requires_grad and id(p) not in frozen]
        self.optimizer = DeviceAdam(self.params, lr=self.lr, max_norm=grad_clip, scaler=scaler)
        if lr_policy == "step":
            self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=int(step_size), gamma=float(gamma))
        elif lr_policy == "multistep":
            self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=[int(m) for m in milestones],
                                                                  gamma=float(gamma))
        else:
            self.scheduler = None
        self.render_par = renderer.bind_parallel(net, None)

        self._order = None
        if _is_resident(train_data):
            self.train_loader = None
            self.batches_per_epoch = len(train_data) // self.batch_size
        else:                                                       # under W ranks: the rank's own objects, rank_batch at a time
            self.batches_per_epoch = len(train_data) // self.batch_size
            self._order = _EpochOrder(len(train_data) if self.world == 1 else self.batches_per_epoch * self.rank_batch)
            self.train_loader = torch.utils.data.DataLoader(train_data, batch_size=self.rank_batch, sampler=self._order,
                                                            num_workers=0, pin_memory=False, drop_last=True)
        self.val_loader = None
        if val_data is not None and not _is_resident(val_data):
            if self.world == 1:
                self.val_loader = torch.utils.data.DataLoader(val_data, batch_size=min(self.batch_size, 4), shuffle=False,
                                                              num_workers=0, pin_memory=False)
            else:
                mine = rank_val_batches(len(val_data), min(self.batch_size, 4), self.world, self.rank)
                self.val_loader = torch.utils.data.DataLoader(val_data, batch_sampler=mine, num_workers=0, pin_memory=False)

        self.epoch, self.iter, self.global_step, self.best_val_loss = 0, 0, 0, float("inf")
        if resume is True:
            latest = os.path.join(self.checkpoint_dir, "latest.pth")
            if os.path.exists(latest):
                self.load_checkpoint(latest)
            else:
                self._log(f"no checkpoint at {latest}, starting from scratch")
        elif resume:
            self.load_checkpoint(os.fspath(resume))

    # ------------------------------------------------------------------------------------------------ the ranks
    def _log(self, text):
        if self.rank == 0:
            print(text)

    def _src(self):
        """Rank 0 of the group, as the collectives name it (a rank of the default group)."""
        import torch.distributed as dist
        return 0 if self.group is None else dist.get_global_rank(self.group, 0)

    def _state_buffers(self):
        """The net's persistent buffers, what a checkpoint holds of them (BatchNorm's statistics, the code's frequencies).  The
        cameras the last encode() left are per-call data, not state: their shapes may differ from rank to rank."""
        keys = set(self.net.state_dict().keys())
        return [b for name, b in self.net.named_buffers() if name in keys]

    def _broadcast(self, tensors):
        """Rank 0's values of `tensors` (any dtypes, one device) into every rank's, with ONE collective over their bytes."""
        import torch.distributed as dist
        tensors = [t.detach() for t in tensors if t.numel() > 0]
        if self.world == 1 or not tensors:
            return
        tensors.sort(key=lambda t: -t.element_size())       # widest elements first: every tensor starts on a multiple of its own
        flat = torch.cat([t.contiguous().reshape(-1).view(torch.uint8) for t in tensors])
        dist.broadcast(flat, src=self._src(), group=self.group)
        at = 0
        for t in tensors:
            nb = t.numel() * t.element_size()
            if self.rank != 0:
                t.copy_(flat[at:at + nb].view(t.dtype).view(t.shape))
            at += nb

    def _mean_over_ranks(self, values):
        """A device tensor of per-rank values -> their mean over the ranks, fp64; ONE collective that every rank joins."""
        import torch.distributed as dist
        values = values.detach().double()
        if self.world > 1:
            values = values.clone()
            dist.all_reduce(values, op=dist.ReduceOp.SUM, group=self.group)
            values /= self.world
        return values

    def _barrier(self):
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier(group=self.group)

    # ------------------------------------------------------------------------------------------------ batches
    def _train_batches(self, epoch):
        if self.train_loader is None:
            if self.world > 1:
                return self._resident_rank_batches(epoch)
            gen = torch.Generator().manual_seed(frame_seed(self.seed, epoch))       # batches() draws epoch_permutation with it
            return self.train_data.batches(self.batch_size, shuffle=True, generator=gen, drop_last=True)
        order = epoch_permutation(len(self.train_data), self.seed, epoch).tolist()
        self._order.order = order if self.world == 1 else rank_epoch_order(order, self.batch_size, self.world, self.rank)
        return iter(self.train_loader)

    def _resident_rank_batches(self, epoch):
        """The rank's slice of every global batch of the epoch's order: only its own objects are gathered."""
        order = epoch_permutation(len(self.train_data), self.seed, epoch).tolist()
        mine = rank_epoch_order(order, self.batch_size, self.world, self.rank)
        for k in range(0, len(mine), self.rank_batch):
            yield self.train_data.batch(mine[k:k + self.rank_batch])

    def _val_batches(self):
        if self.val_data is None:
            return iter(())
        if self.val_loader is None:
            if self.world > 1:
                mine = rank_val_batches(len(self.val_data), min(self.batch_size, 4), self.world, self.rank)
                return (self.val_data.batch(ids) for ids in mine)
            return self.val_data.batches(min(self.batch_size, 4), shuffle=False, drop_last=False)
        return iter(self.val_loader)

    def _losses_kw(self, key, **more):
        kw = dict(ray_batch_size=self.ray_batch_size, nviews=self.nviews, z_near=self.z_near, z_far=self.z_far, loss=self.loss,
                  balanced=self.balanced, **more)
        if self.alpha_loss is not None:
            kw.update(alpha_loss=self.alpha_loss)
        if self.mask_loss is not None:
            kw.update(mask_loss=self.mask_loss)
        if self.draws == "device":
            kw.update(draws="device", seed=key)
        return kw

    def _keyed(self, key):
        """The scope a render of the step keyed `key` runs in: keyed noise under device draws, the renderer as it is else."""
        import contextlib
        return self.renderer.keyed(key) if self.draws == "device" else contextlib.nullcontext()

    # ------------------------------------------------------------------------------------------------ one epoch
    def train_step(self, data, global_step):
        key = frame_seed(self.seed, global_step)
        more = dict(use_bbox=global_step < self.no_bbox_step, jitter=self.jitter)
        if self.prop_inside is not None:
            more.update(prop_inside=self.prop_inside)
        if self.world > 1:
            more.update(obj_base=self.obj_base, grad_hook=self._allreduce)
        with self._keyed(key):
            return train.train_step(self.net, self.render_par, data, self.optimizer, **self._losses_kw(key, **more))

    def _allreduce(self):
        self.optimizer.allreduce(self.group)

    def _net_train(self):
        self.net.train()
        if self.freeze_enc:
            self.net.encoder.eval()

    def _read(self, loss_dict):
        """ONE host read: the step's values, stacked on the device first — under several ranks their mean over the ranks (one
        collective that every rank joins; grad_norm is the same on all of them already)."""
        keys = [k for k in loss_dict if k != "loss"]
        vals = self._mean_over_ranks(torch.stack([torch.as_tensor(loss_dict[k]).detach().double() for k in keys])).tolist()
        return dict(zip(keys, vals))

    def train_epoch(self, epoch):
        if self.alpha_loss is not None:
            self.alpha_loss.set_epoch(epoch)
        self._net_train()
        self.renderer.train()
        total, count = None, 0
        t0 = time.time()
        for batch_idx, data in enumerate(self._train_batches(epoch)):
            if data is None:
                continue
            loss_dict = self.train_step(data, self.global_step)
            if "t" in loss_dict:
                t = loss_dict["t"].detach()
                total = t.clone() if total is None else total.add_(t)
            count += 1
            if batch_idx % self.print_interval == 0 and loss_dict:
                vals = self._read(loss_dict)
                lr = self.optimizer.param_groups[0]["lr"]
                self._log(f"[{time.time() - t0:.2f}s/it] E {epoch} B {batch_idx}" + "".join(f" {k}:{v:.4f}" for k, v in vals.items())
                          + f" lr {lr:.6f}")
                if self.writer is not None and self.rank == 0:
                    for k, v in vals.items():
                        self.writer.add_scalar(f"train/{k}", v, self.global_step)
                    self.writer.add_scalar("train/lr", lr, self.global_step)
                t0 = time.time()
            self.renderer.sched_step(self.batch_size)
            self.global_step += 1
        if self.world > 1 and total is not None:
            total = self._mean_over_ranks(total)
        avg_loss = float(total) / count if total is not None and count else 0.0
        self._log(f"Epoch {epoch} finished: avg_loss={avg_loss:.4f}")

        if self.world > 1:                                          # a training BatchNorm's statistics are the rank's own
            self._broadcast(self._state_buffers())
        if (epoch + 1) % self.save_interval == 0:
            self.save_checkpoint_with_epoch(epoch)
        if (epoch + 1) % self.eval_interval == 0:
            self._validate_and_keep_best()
        if (epoch + 1) % self.vis_interval == 0 and self.val_data is not None and len(self.val_data) > 0 and self.rank == 0:
            try:
                self.visualise()
            except Exception as e:                                   # as the reference: a failed picture does not end a run
                self._log(f"visualisation failed: {e!r}")
        if self.scheduler is not None:
            self.scheduler.step()
        return avg_loss

    # ------------------------------------------------------------------------------------------------ validation, picture
    def validate(self):
        key = frame_seed(self.seed, self.global_step)
        with self._keyed(key):
            if self.world == 1:
                val_loss = train.validate(self.net, self.renderer, self.render_par, self._val_batches(), **self._losses_kw(key))
            else:
                val_loss = self._validate_ranks(key)
        self._log(f"Validation: avg_loss={val_loss:.4f}")
        if self.writer is not None and self.rank == 0:
            self.writer.add_scalar("val/loss", val_loss, self.global_step)
        self._net_train()
        return val_loss

    def _validate_ranks(self, key):
        """train.validate over the rank's batches (batch i belongs to rank i % W), then ONE collective over (fp64 sum of t,
        count): every rank leaves with the same mean over all batches, inf when none counted."""
        import torch.distributed as dist
        acc = torch.zeros(2, dtype=torch.float64, device=self.device)
        count = 0
        self.net.eval()
        for data in self._val_batches():
            if data is None or not data or "images" not in data:
                continue
            loss_dict = train.eval_step(self.net, self.renderer, self.render_par, data, **self._losses_kw(key))
            if "t" not in loss_dict:
                continue
            acc[0] += torch.as_tensor(loss_dict["t"]).detach().double()
            count += 1
        acc[1] = count
        dist.all_reduce(acc, op=dist.ReduceOp.SUM, group=self.group)
        total, n = acc.tolist()
        return total / n if n > 0 else float("inf")

    def _validate_and_keep_best(self):
        val_loss = self.validate()
        if val_loss < self.best_val_loss:
            self.best_val_loss = val_loss
            self.save_checkpoint("best.pth")
            self._log(f"best checkpoint saved (loss: {val_loss:.4f})")

    def visualise(self):
        """vis_step on the first validation batch -> <logs_path>/<name>/vis_%04d.png (the epoch) and writer.add_image."""
        from PIL import Image
        data = next(self._val_batches(), None)
        if data is None or "images" not in data:
            return None
        if data["images"].dtype == torch.uint8:                      # a byte batch: vis_step takes the float images of one object
            imgs = data["images"]
            if imgs.is_cuda:
                order = torch.arange(imgs.shape[1], device=imgs.device).expand(imgs.shape[0], -1).contiguous()
                imgs = util.views_to_tensor_u8(imgs, order, balanced=self.balanced)
            else:
                from .data._items import images_to_float
                imgs = torch.stack([images_to_float(x[..., :3], self.balanced) for x in imgs])
            data = dict(data, images=imgs)
        key = frame_seed(self.seed, self.global_step)
        with self._keyed(key):
            vis, vals = train.vis_step(self.net, self.renderer, self.render_par, data, nviews=self.nviews, z_near=self.z_near,
                                       z_far=self.z_far, out="uint8")
        panel = vis.cpu().numpy()
        path = os.path.join(self.log_dir, "vis_%04d.png" % self.epoch)
        Image.fromarray(panel).save(path)
        if self.writer is not None:
            self.writer.add_image("vis", panel, self.global_step, dataformats="HWC")
            for k, v in vals.items():
                self.writer.add_scalar(f"vis/{k}", float(v), self.global_step)
        self._net_train()
        return path

    # ------------------------------------------------------------------------------------------------ checkpoints
    def save_checkpoint_with_epoch(self, epoch):
        self.save_checkpoint("epoch_%04d.pth" % epoch, save_epoch=epoch)
        self.save_checkpoint("latest.pth", save_epoch=epoch + 1)                 # what a resumed run starts with
        if self.rank != 0:
            return
        for n in checkpoints_to_remove(os.listdir(self.checkpoint_dir), self.save_strategy, self.keep_last_checkpoints, epoch):
            try:
                os.remove(os.path.join(self.checkpoint_dir, n))
                print(f"removed old checkpoint: {n}")
            except OSError as e:
                print(f"failed to remove {n}: {e}")

    def save_checkpoint(self, filename, save_epoch=None):
        """Rank 0 writes; under several ranks a barrier follows, so no rank runs ahead of a file it may read."""
        if self.rank == 0:
            self._write_checkpoint(filename, save_epoch)
        self._barrier()

    def _write_checkpoint(self, filename, save_epoch):
        ckpt = {"epoch": self.epoch if save_epoch is None else int(save_epoch), "iter": self.iter, "global_step": self.global_step,
                "net_state_dict": self.net.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(),
                "best_val_loss": self.best_val_loss, "seed": self.seed}
        if self.scheduler is not None:
            ckpt["scheduler_state_dict"] = self.scheduler.state_dict()
        if self.world > 1:
            ckpt["world_size"] = self.world                          # for the reader: nothing depends on it
        torch.save(ckpt, os.path.join(self.checkpoint_dir, filename))
        torch.save(self.renderer.state_dict(), self.renderer_state_path)
        if filename != "latest.pth":
            print(f"checkpoint saved: {filename}")

    def load_checkpoint(self, path):
        ckpt = torch.load(path, map_location=self.device, weights_only=False)
        self.epoch, self.iter = int(ckpt.get("epoch", 0)), int(ckpt.get("iter", 0))
        self.global_step = int(ckpt.get("global_step", 0))
        self.best_val_loss = ckpt.get("best_val_loss", float("inf"))
        if "seed" in ckpt and int(ckpt["seed"]) != self.seed:
            self._log(f"the checkpoint was written under seed {ckpt['seed']}: continuing with it instead of {self.seed}")
            self.seed = int(ckpt["seed"])
        self.net.load_state_dict(ckpt["net_state_dict"])
        self.optimizer.load_state_dict(ckpt["optimizer_state_dict"])
        if self.scheduler is not None and "scheduler_state_dict" in ckpt:
            self.scheduler.load_state_dict(ckpt["scheduler_state_dict"])
        rpath = os.path.join(os.path.dirname(path), "_renderer")
        if os.path.exists(rpath):
            self.renderer.load_state_dict(torch.load(rpath, map_location=self.device, weights_only=False))
            self.renderer._apply_sched()
        # the reference's correction (trainer.py:648-665): latest.pth whose epoch disagrees with its global_step
        if self.batches_per_epoch > 0:
            expected = self.global_step // self.batches_per_epoch
            if expected != self.epoch:
                self._log(f"checkpoint inconsistency: saved epoch {self.epoch}, global_step {self.global_step} = epoch {expected} "
                          f"at {self.batches_per_epoch} batches per epoch")
                if os.path.basename(path) == "latest.pth":
                    self._log(f"  correcting to epoch {expected}")
                    self.epoch = expected
        # The reference saves before it steps the scheduler, so latest.pth (which names the NEXT epoch) holds the lr of the
        # epoch that just ended.  The schedule is a function of the epoch: step it up to the epoch the run resumes at.
        if self.scheduler is not None:
            while self.scheduler.last_epoch < self.epoch:
                self.scheduler.step()
        self._log(f"checkpoint loaded: {path}; resuming from epoch {self.epoch}, global_step {self.global_step}")

    # ------------------------------------------------------------------------------------------------ the run
    def start(self):
        self._log(f"training {self.name}: device {self.device}, batch size {self.batch_size}, lr {self.lr}, {self.num_epochs} epochs, "
                  f"draws {self.draws}, seed {self.seed}, checkpoints {self.checkpoint_dir} ({self.save_strategy}), logs {self.log_dir}"
                  + (f", {self.world} ranks of {self.rank_batch} objects" if self.world > 1 else ""))
        if self.alpha_loss is not None:
            self.alpha_loss.set_epoch(self.epoch)
        if self.epoch > 0 and self.epoch % self.eval_interval == 0:        # a resumed epoch on an evaluation node
            self._validate_and_keep_best()
        for epoch in range(self.epoch, self.num_epochs):
            self.epoch = epoch
            self.train_epoch(epoch)
        self._log("training finished")
        if self.writer is not None and self.rank == 0 and hasattr(self.writer, "close"):
            self.writer.close()
