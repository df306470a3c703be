"""
The trainer's losses (reference src/model/loss.py as train/train.py uses it).  get_rgb_loss keeps the reference's name
and return value so its scripts' imports resolve; RenderLoss is what train.calc_losses calls: the coarse and the fine
criterion, their weighted sum and its gradient as two HIP launches (render.autograd.RGBLoss) with nothing read back.

The opacity losses work on the renderer's compositing weights (render_par(rays, want_weights=True)): AlphaLossNV2 /
get_alpha_loss are the reference's, MaskLoss is a binary cross entropy of the weights' sum against the object's mask at the
step's pixels (train.make_batch(want_mask=True)).  Both are render.autograd.AlphaLoss: two launches forward, one backward.
"""
import torch

from ..util import as_conf


def get_rgb_loss(conf, coarse=True, using_bg=False, reduction="mean"):
    """torch's L1Loss / MSELoss by conf.use_l1 (reference loss.py:91-103, the vanilla case).  The uncertainty-weighted loss
    of a fine pass (use_uncertainty) is not part of this package."""
    conf = as_conf(conf)
    if conf.get_bool("use_uncertainty", False) and not coarse:
        raise NotImplementedError("use_uncertainty (RGBWithUncertainty) is not implemented")
    return torch.nn.L1Loss(reduction=reduction) if conf.get_bool("use_l1", False) else torch.nn.MSELoss(reduction=reduction)


class RenderLoss(torch.nn.Module):
    """forward(render_dict, rgb_gt) -> (total, stats): rgb_coarse_crit / rgb_fine_crit of the renderer's nested output
    (render_par(rays, want_weights=True)) combined as train/train.py:338-346 does — total = lambda_coarse * Lc +
    lambda_fine * Lf, or Lc alone (no lambda) when the renderer has no fine pass.  total is a differentiable 0-dim device
    tensor; stats the 3-float device buffer [lambda_coarse * Lc, lambda_fine * Lf, total]."""

    def __init__(self, lambda_coarse, lambda_fine, use_l1=False):
        super().__init__()
        self.lambda_coarse, self.lambda_fine, self.use_l1 = float(lambda_coarse), float(lambda_fine), bool(use_l1)

    @classmethod
    def from_conf(cls, conf, lambda_coarse=1.0, lambda_fine=1.0):
        return cls(lambda_coarse, lambda_fine, as_conf(conf).get_bool("use_l1", False))

    def forward(self, render_dict, rgb_gt):
        from ..render.autograd import RGBLoss
        coarse = render_dict["coarse"]
        fine = render_dict.get("fine")
        fine_rgb = fine["rgb"] if fine is not None and len(fine) > 0 else None
        return RGBLoss.apply(coarse["rgb"], fine_rgb, rgb_gt, self.use_l1, self.lambda_coarse, self.lambda_fine)


class AlphaLossNV2(torch.nn.Module):
    """The reference's Neural Volumes alpha loss 2 (loss.py:4-37): lambda_alpha * mean(max(log a + log(1 - a), -clamp_alpha)), or with
    force_opaque lambda_alpha * BCELoss(a, 1), a = clamp(alpha, 0.01, 0.99) — the reference's constants — from init_epoch on; the
    constructor, the persistent `epoch` buffer and sched_step(num=1) are the reference's.

    Differences, on purpose: forward(weights) takes the (..., K) compositing WEIGHTS, not their sum (the sum is taken in fp64 by
    pnr_alpha_loss, and the gradient is written to the weights directly); the result is a 0-dim tensor, also when the loss is
    inactive (lambda_alpha <= 0 or before init_epoch: a cached device zero, no launch), where the reference returns shape (1,);
    and the gate never reads the device: a host mirror of `epoch` is kept by sched_step and set_epoch(e) and refreshed once when a
    state dict is loaded."""
    CLAMP_LO, CLAMP_HI = 0.01, 0.99

    def __init__(self, lambda_alpha, clamp_alpha, init_epoch, force_opaque=False):
        super().__init__()
        self.lambda_alpha = lambda_alpha
        self.clamp_alpha = clamp_alpha
        self.init_epoch = init_epoch
        self.force_opaque = force_opaque
        self.register_buffer("epoch", torch.tensor(0, dtype=torch.long), persistent=True)
        self._epoch_host = 0
        self._zeros = {}

    def sched_step(self, num=1):
        self.epoch += num
        self._epoch_host += int(num)

    def set_epoch(self, e):
        """The epoch counter, set from the caller's own (a Trainer's, at every epoch's start): no device read."""
        self.epoch.fill_(int(e))
        self._epoch_host = int(e)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._epoch_host = int(self.epoch)              # the one host read of a loaded counter

    @property
    def active(self):
        return self.lambda_alpha > 0.0 and self._epoch_host >= self.init_epoch

    def forward(self, weights):
        if not self.active:
            zero = self._zeros.get(weights.device)
            if zero is None:
                zero = self._zeros[weights.device] = torch.zeros((), device=weights.device)
            return zero
        from .. import _native as N
        from ..render.autograd import AlphaLoss
        mode = N.PNR_ALPHA_OPAQUE if self.force_opaque else N.PNR_ALPHA_NV2
        return AlphaLoss.apply(weights, None, None, mode, self.lambda_alpha, 0.0, self.CLAMP_LO, self.CLAMP_HI, self.clamp_alpha)[0]


def get_alpha_loss(conf):
    """AlphaLossNV2 from the reference's loss.alpha block: lambda_alpha, clamp_alpha, init_epoch, force_opaque (loss.py:40-48)."""
    conf = as_conf(conf)
    return AlphaLossNV2(conf.get_float("lambda_alpha"), conf.get_float("clamp_alpha"), conf.get_int("init_epoch"),
                        force_opaque=conf.get_bool("force_opaque", False))


class MaskLoss(torch.nn.Module):
    """forward(render_dict, mask_gt) -> (total, stats): the binary cross entropy of each pass's opacity — the sum of its compositing
    weights, clamped to [eps, 1 - eps] — against mask_gt (SB, B) in [0, 1], the object's mask at the rays' pixels
    (train.make_batch(want_mask=True)): total = lambda_coarse * BCE(coarse) + lambda_fine * BCE(fine), the fine term only when
    the renderer has a fine pass.  total is a differentiable 0-dim device tensor; stats the 3-float device buffer
    [lambda_coarse * Lc, lambda_fine * Lf, total].  The lambdas have no default: no effect on PSNR or floaters has been measured."""

    def __init__(self, lambda_coarse, lambda_fine, eps=0.01):
        super().__init__()
        self.lambda_coarse, self.lambda_fine, self.eps = float(lambda_coarse), float(lambda_fine), float(eps)
        if not 0.0 < self.eps < 0.5:
            raise ValueError(f"eps must lie in (0, 0.5), got {eps}")

    def forward(self, render_dict, mask_gt):
        from .. import _native as N
        from ..render.autograd import AlphaLoss
        coarse = render_dict["coarse"]
        fine = render_dict.get("fine")
        fine_w = fine["weights"] if fine is not None and len(fine) > 0 else None
        return AlphaLoss.apply(coarse["weights"], fine_w, mask_gt, N.PNR_ALPHA_MASK, self.lambda_coarse, self.lambda_fine,
                               self.eps, 1.0 - self.eps, 0.0)
