"""
The trainer's rgb losses (reference src/model/loss.py as train/train.py uses it).  get_rgb_loss keeps the reference's name
and return value so its scripts' imports resolve; RenderLoss is what train.calc_losses calls: the coarse and the fine
criterion, their weighted sum and its gradient as two HIP launches (render.autograd.RGBLoss) with nothing read back.
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
