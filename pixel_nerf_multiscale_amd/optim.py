"""
The training step's back end on the device: everything the reference does between loss.backward() and the next zero_grad
(train/train.py:375-412 — GradScaler.unscale_, clip_grad_norm_, scaler.step, scaler.update — with trainlib/trainer.py:169's
Adam) as ONE native call of three launches over every trainable tensor (pnr_adam_step, csrc/optim.hip; the arithmetic is
fixed in include/pnr.h).  Nothing waits for the device: the norm, the found-inf decision, the scale and the step count live
in one small device record, and a step whose gradients are not finite is skipped on the device.
"""
import ctypes as C
import math

import numpy as np
import torch

_SEG = np.dtype([("param", "<u8"), ("offset", "<i8"), ("n", "<i8")])           # pnr_optim_segment
_CHUNK_BYTES = 16                                                               # pnr_optim_chunk
# pnr_optim_state: field -> (byte offset, dtype)
_STATE_BYTES = 56
_STATE = {"grad_norm": (0, torch.float64), "clip_coef": (8, torch.float32), "scale": (12, torch.float32),
          "inv_scale": (16, torch.float32), "found_inf": (20, torch.int32), "growth_tracker": (24, torch.int32),
          "step": (32, torch.int64), "skipped": (40, torch.int64), "step_size": (48, torch.float32),
          "rsqrt_bc2": (52, torch.float32)}
_SCALER_KEYS = ("init_scale", "growth_factor", "backoff_factor", "growth_interval")


def _round_up4(n):
    return (n + 3) & ~3


class DeviceAdam(torch.optim.Optimizer):
    """torch.optim.Adam (weight_decay = 0, amsgrad = False) with gradient clipping and, optionally, GradScaler's dynamic loss
    scale folded in — the whole tail of the reference's train_step in one call that never reads the device.

        optim = DeviceAdam(net.parameters(), lr=1e-4, max_norm=grad_clip, scaler=dict(init_scale=65536.0, growth_factor=2.0,
                                                                                     backoff_factor=0.5, growth_interval=2000))
        optim.zero_grad(); optim.scale(loss).backward(); optim.step()

    params    fp32, contiguous, all on one HIP device; ONE param group (torch's LR schedulers attach to it and `lr` is read
              at every step).
    max_norm  clip_grad_norm_'s max_norm; None or <= 0: no clipping (the norm is still computed).
    scaler    None, or a dict with any of init_scale, growth_factor, backoff_factor, growth_interval (GradScaler's
              defaults otherwise).

    The optimizer owns three flat fp32 buffers (gradients, exp_avg, exp_avg_sq) and points every p.grad at its slice, so
    backward accumulates where step() reads.  zero_grad() is one memset of the gradient buffer; `set_to_none` is accepted and
    IGNORED (the gradients must stay where they are).  step() compares each p.grad's address with its table — no device
    read: a gradient that was replaced (p.grad = other) is copied into its slice and p.grad pointed back; a parameter whose
    .grad is None gets a segment of length 0 for that step, i.e. is left alone, as torch does; the device tables are
    uploaded again, from one of two pinned blocks allocated at the first step, only when something changed.  The no-wait
    property is that of the steady state, where every .grad stays attached: the first step allocates pinned memory (which
    may wait for the device), and a caller that drops gradients every step (zero_grad(set_to_none=True) of another
    optimizer, p.grad = None) pays a copy per re-adopted gradient and a table upload at every step.

    Deviations from torch, both documented in include/pnr.h: a non-finite gradient skips the step with OR without a scaler
    (parameters, moments and step count keep their bits, `skipped` goes up) where torch without a scaler writes NaN into
    every parameter; and .grad is never written, so after step() it still holds the scaled, unclipped values.  There is ONE
    step count for all parameters (torch keeps one per parameter, which differ only when a gradient was None for some steps).

    grad_norm (fp64), found_inf, scale_value, step_count, skipped are 0-dim device views of the state record: reading one
    (.item()) is the only wait, and the caller chooses when.

    Data-parallel steps: allreduce(group), in train_step's grad_hook slot, sums the flat gradient buffer over the ranks with
    ONE collective and arms the next step() to divide by the world size inside its kernels (pnr_adam_step_div)."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=None, scaler=None):
        params = list(params)
        if not params:
            raise ValueError("DeviceAdam got an empty parameter list")
        if isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError("DeviceAdam takes ONE param group (one lr, one clip over all gradients)")
            group_in = dict(params[0])
            plist = list(group_in.pop("params"))
        else:
            group_in, plist = {}, params
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid hyper-parameters lr={lr} betas={betas} eps={eps}")
        for i, p in enumerate(plist):
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"parameter {i} is not a tensor")
            if p.dtype != torch.float32:
                raise TypeError(f"DeviceAdam updates fp32 parameters in place; parameter {i} is {p.dtype}")
            if not p.is_contiguous():
                raise ValueError(f"parameter {i} is not contiguous")
        devs = {p.device for p in plist}
        if len(devs) != 1:
            raise ValueError(f"parameters must share one device, got {sorted(str(d) for d in devs)}")
        if scaler is not None:
            unknown = set(scaler) - set(_SCALER_KEYS)
            if unknown:
                raise ValueError(f"unknown scaler keys {sorted(unknown)}; known: {_SCALER_KEYS}")
            scaler = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000) | dict(scaler)
            if int(scaler["growth_interval"]) < 1 or not scaler["init_scale"] > 0.0:
                raise ValueError("scaler needs growth_interval >= 1 and init_scale > 0")
        dev = devs.pop()
        if dev.type != "cuda":
            raise RuntimeError("DeviceAdam needs parameters on a HIP device (cuda:N): there is no host path")

        self._frozen = False
        # Adam's own keys ride along so that a state_dict loads into torch.optim.Adam as it is
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, max_norm=max_norm)
        group_in["params"] = plist
        super().__init__([group_in], defaults)
        self._frozen = True
        self._check_group(self.param_groups[0])

        from . import _native as N
        self._N = N
        self._dev = dev
        self._params = list(self.param_groups[0]["params"])
        self._numel = [p.numel() for p in self._params]
        self._offset, off = [], 0
        for n in self._numel:
            self._offset.append(off)
            off = _round_up4(off + n)
        self._n_flat = max(off, 4)
        self._grad = torch.zeros(self._n_flat, device=dev)
        self._exp_avg = torch.zeros(self._n_flat, device=dev)
        self._exp_avg_sq = torch.zeros(self._n_flat, device=dev)
        self._slices = [self._grad[o:o + n].view_as(p) for p, o, n in zip(self._params, self._offset, self._numel)]
        self._slice_ptr = [s.data_ptr() for s in self._slices]
        for p, s in zip(self._params, self._slices):
            p.grad = s

        n_seg = len(self._params)
        full = np.asarray(self._numel, dtype=np.int64)
        self._max_chunks = self._plan(full, None, 0)
        self._seg_bytes = (n_seg * _SEG.itemsize + 15) & ~15
        self._tables = torch.zeros(self._seg_bytes + max(self._max_chunks, 1) * _CHUNK_BYTES, dtype=torch.uint8, device=dev)
        self._workspace = torch.zeros(max(int(N.lib.pnr_optim_workspace_bytes(self._max_chunks)), 16), dtype=torch.uint8, device=dev)
        self._staging = []                      # pinned blocks the tables are written into: [tensor, event of its last upload]
        self._seg_n = None                      # what the device tables hold: lengths and parameter addresses
        self._seg_param = None
        self._n_chunks = 0
        self._grad_div = 1                      # armed by allreduce() for ONE step()

        self._scaler_conf = scaler
        self._scaler_arg = None
        if scaler is not None:
            self._scaler_arg = N.pnr_optim_scaler(float(scaler["growth_factor"]), float(scaler["backoff_factor"]),
                                                  int(scaler["growth_interval"]), 0)
        self._state_buf = torch.zeros(_STATE_BYTES, dtype=torch.uint8, device=dev)
        self._write_state(scale=float(scaler["init_scale"]) if scaler else 1.0, growth_tracker=0, step=0, skipped=0)

    # ------------------------------------------------------------------------------------------------ the state record
    def _view(self, name):
        o, dt = _STATE[name]
        return self._state_buf[o:o + torch.empty((), dtype=dt).element_size()].view(dt).reshape(())

    def _write_state(self, scale, growth_tracker, step, skipped):
        """(Re)initialises the record: construction and load_state_dict, never the training loop."""
        rec = self._N.pnr_optim_state()
        rec.clip_coef, rec.scale, rec.inv_scale = 1.0, scale, 1.0 / scale
        rec.growth_tracker, rec.step, rec.skipped = int(growth_tracker), int(step), int(skipped)
        host = torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8)
        self._state_buf.copy_(host)

    grad_norm = property(lambda self: self._view("grad_norm"), doc="fp64 norm of the last step's unscaled gradients")
    clip_coef = property(lambda self: self._view("clip_coef"))
    found_inf = property(lambda self: self._view("found_inf"), doc="1 when the last step was skipped")
    scale_value = property(lambda self: self._view("scale"), doc="the loss scale (1 without a scaler)")
    step_count = property(lambda self: self._view("step"), doc="applied steps t")
    skipped = property(lambda self: self._view("skipped"), doc="skipped steps")
    growth_tracker = property(lambda self: self._view("growth_tracker"))
    step_size = property(lambda self: self._view("step_size"), doc="lr / (1 - beta1^t) of the last applied step, fp32")

    def moments(self, i):
        """(exp_avg, exp_avg_sq) of parameter i: views of the flat buffers, shaped like the parameter."""
        o, n, p = self._offset[i], self._numel[i], self._params[i]
        return self._exp_avg[o:o + n].view_as(p), self._exp_avg_sq[o:o + n].view_as(p)

    def scale(self, loss):
        """loss * the device-resident scale (GradScaler.scale); the loss itself without a scaler."""
        if self._scaler_conf is None:
            return loss
        return loss * self.scale_value

    # ------------------------------------------------------------------------------------------------ torch.optim plumbing
    @staticmethod
    def _check_group(g):
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("DeviceAdam implements Adam with weight_decay = 0, amsgrad = False, maximize = False")

    def add_param_group(self, param_group):
        if getattr(self, "_frozen", False):
            raise ValueError("DeviceAdam takes ONE param group, fixed at construction (it owns the flat buffers)")
        super().add_param_group(param_group)

    def attach_grads(self):
        """Points every p.grad at its slice of the flat buffer again, without copying — after something else (another
        optimizer's zero_grad(set_to_none=True)) dropped them.  step() does this by itself for a gradient it finds replaced."""
        for p, s in zip(self._params, self._slices):
            p.grad = s

    def zero_grad(self, set_to_none=False):
        """One memset.  set_to_none is ignored: every p.grad stays a view of the flat gradient buffer."""
        self._grad.zero_()

    def _plan(self, seg_n, host_ptr, max_chunks):
        n = int(self._N.lib.pnr_optim_plan(seg_n.ctypes.data_as(C.POINTER(C.c_int64)), len(seg_n), host_ptr, max_chunks))
        if n < 0:
            self._N.check(n, "pnr_optim_plan")
        return n

    def _pinned_block(self):
        """One of two alternating pinned staging blocks whose last upload has finished (an event query, no wait); a third,
        fresh one when both are still in flight — tables that change step after step faster than the device drains them."""
        for slot in self._staging:
            if slot[1] is None or slot[1].query():
                self._staging.remove(slot)
                self._staging.append(slot)              # least recently used first
                return slot
        return [torch.empty(self._tables.numel(), dtype=torch.uint8, pin_memory=True), None]

    def _upload_tables(self, seg_n, seg_param):
        if not self._staging:
            self._staging = [[torch.zeros(self._tables.numel(), dtype=torch.uint8, pin_memory=True), None] for _ in range(2)]
        slot = self._pinned_block()
        host = slot[0]
        arr = host.numpy()
        seg = arr[:len(seg_n) * _SEG.itemsize].view(_SEG)
        seg["param"] = seg_param
        seg["offset"] = self._offset
        seg["n"] = seg_n
        self._n_chunks = self._plan(seg_n, host.data_ptr() + self._seg_bytes, self._max_chunks)
        assert self._n_chunks <= self._max_chunks
        self._tables.copy_(host, non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self._dev))
        self._seg_n, self._seg_param = seg_n, seg_param

    @torch.no_grad()
    def allreduce(self, group=None):
        """The gradient exchange of a data-parallel step, for train_step's grad_hook slot: every rank holds the gradient of
        its share of the batch (each a mean over its own rays) and leaves with their sum; the step that follows divides by the
        world size inside its kernels, so the mean costs no pass of its own.
          * a gradient that was replaced (p.grad = other) is copied into its slice and p.grad pointed back, as step() does;
          * a parameter whose .grad is None gets its slice, zeroed: every rank then steps the same segments, whichever of them
            reached the parameter in its backward;
          * ONE dist.all_reduce(SUM) over the whole flat gradient buffer (SUM, not AVG: every backend has it);
          * the next step() — that one only — runs with grad_div = the group's size.  Norm, clip, found_inf and the scaler read
            the same reduced buffer on every rank, so they agree with no further collective.
        group: a ProcessGroup, or None for the default group.  With no initialised group, or a group of one rank, no collective
        is issued and the divisor stays 1: the step's bits are those of a plain step."""
        import torch.distributed as dist
        world = 1
        if dist.is_available() and dist.is_initialized():
            world = dist.get_world_size(group)
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                if world > 1:
                    self._slices[i].zero_()
                    p.grad = self._slices[i]
            elif g.data_ptr() != self._slice_ptr[i] or g.dtype != torch.float32 or not g.is_contiguous():
                if g.shape != p.shape or g.device != self._dev:
                    raise ValueError(f"parameter {i}: replaced .grad has shape {tuple(g.shape)} on {g.device}")
                self._slices[i].copy_(g)
                p.grad = self._slices[i]
        if world > 1:
            dist.all_reduce(self._grad, op=dist.ReduceOp.SUM, group=group)
        self._grad_div = world

    @torch.no_grad()
    def step(self, closure=None, grad_div=None):
        """grad_div: the gradient buffer holds a sum over that many ranks (pnr_adam_step_div); None: what allreduce() armed
        for this step, 1 otherwise."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        armed, self._grad_div = self._grad_div, 1
        grad_div = armed if grad_div is None else int(grad_div)
        if grad_div < 1:
            raise ValueError(f"grad_div must be >= 1, got {grad_div}")
        seg_n = np.empty(len(self._params), dtype=np.int64)
        seg_param = np.empty(len(self._params), dtype=np.uint64)
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                seg_n[i] = 0
            else:
                if g.data_ptr() != self._slice_ptr[i] or g.dtype != torch.float32 or not g.is_contiguous():
                    if g.shape != p.shape or g.device != self._dev:
                        raise ValueError(f"parameter {i}: replaced .grad has shape {tuple(g.shape)} on {g.device}")
                    self._slices[i].copy_(g)                   # re-adopt: into the slice, and point .grad back
                    p.grad = self._slices[i]
                seg_n[i] = self._numel[i]
            if not p.is_contiguous() or p.dtype != torch.float32:
                raise ValueError(f"parameter {i} is no longer fp32 and contiguous")
            seg_param[i] = p.data_ptr()
        if self._seg_n is None or not (np.array_equal(seg_n, self._seg_n) and np.array_equal(seg_param, self._seg_param)):
            self._upload_tables(seg_n, seg_param)

        g = self.param_groups[0]
        N = self._N
        max_norm = g.get("max_norm")
        rc = N.lib.pnr_adam_step_div(self._tables.data_ptr(), len(self._params), self._tables.data_ptr() + self._seg_bytes,
                                     self._n_chunks, self._grad.data_ptr(), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(),
                                     self._n_flat, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                                     0.0 if max_norm is None else float(max_norm),
                                     None if self._scaler_arg is None else C.byref(self._scaler_arg), int(grad_div),
                                     self._state_buf.data_ptr(), self._workspace.data_ptr(), self._workspace.numel(),
                                     N.current_stream(self._dev))
        N.check(rc, "pnr_adam_step_div")
        return loss

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch.optim.Adam's format — state[i] = {step, exp_avg, exp_avg_sq} per parameter index, param_groups — plus a
        "scaler" entry, so a checkpoint written here resumes under torch.optim.Adam and the other way round.  Reads the
        device (a wait is fine at checkpoint time).  Before the first applied step `state` is empty, as Adam's is."""
        rec = self._N.pnr_optim_state.from_buffer_copy(bytes(self._state_buf.cpu().numpy()))
        state = {}
        if rec.step > 0:
            for i, (p, o, n) in enumerate(zip(self._params, self._offset, self._numel)):
                state[i] = {"step": torch.tensor(float(rec.step), dtype=torch.float32),
                            "exp_avg": self._exp_avg[o:o + n].view_as(p).clone(),
                            "exp_avg_sq": self._exp_avg_sq[o:o + n].view_as(p).clone()}
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._params)))
        scaler = None
        if self._scaler_conf is not None:
            scaler = dict(self._scaler_conf, scale=float(rec.scale), growth_tracker=int(rec.growth_tracker))
        return {"state": state, "param_groups": [group], "scaler": scaler, "skipped": int(rec.skipped)}

    def load_state_dict(self, state_dict):
        """Accepts state_dict() of this class or of torch.optim.Adam over the same parameter list.  Adam's per-parameter step
        counts must agree (this optimizer keeps one); parameters Adam holds no state for start from zero moments."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("the checkpoint's param_groups do not match: DeviceAdam has one group of "
                             f"{len(self._params)} parameters")
        self._check_group(groups[0])
        ids = list(groups[0]["params"])
        state = state_dict.get("state", {})
        steps = set()
        for idx in ids:
            st = state.get(idx)
            if st:
                steps.add(int(round(float(st["step"]))))
        if len(steps) > 1:
            raise ValueError(f"the checkpoint's parameters have different step counts {sorted(steps)}; DeviceAdam keeps one")
        self._exp_avg.zero_()
        self._exp_avg_sq.zero_()
        for i, idx in enumerate(ids):
            st = state.get(idx)
            if not st:
                continue
            o, n = self._offset[i], self._numel[i]
            for buf, key in ((self._exp_avg, "exp_avg"), (self._exp_avg_sq, "exp_avg_sq")):
                src = st[key]
                if src.numel() != n:
                    raise ValueError(f"parameter {i}: {key} has {src.numel()} elements, expected {n}")
                buf[o:o + n].copy_(src.detach().reshape(-1).to(device=self._dev, dtype=torch.float32))
        keep = self.param_groups[0]["params"]
        self.param_groups[0].update({k: v for k, v in groups[0].items() if k != "params"})
        self.param_groups[0].setdefault("max_norm", None)
        self.param_groups[0]["params"] = keep
        sc = state_dict.get("scaler")
        scale, tracker = 1.0, 0
        if self._scaler_conf is not None:
            scale = float(sc["scale"]) if sc else float(self._scaler_conf["init_scale"])
            tracker = int(sc["growth_tracker"]) if sc else 0
            if not (scale > 0.0 and math.isfinite(scale)):
                raise ValueError(f"the checkpoint's scale is {scale}")
        self._write_state(scale=scale, growth_tracker=tracker, step=steps.pop() if steps else 0,
                          skipped=int(state_dict.get("skipped", 0)))
