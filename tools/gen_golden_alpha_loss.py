#!/usr/bin/env python3
"""
Golden vectors for the alpha loss (src/model/loss.py:4-37).  Dev container only, like gen_golden.py: imports the reference's own
AlphaLossNV2 UNMODIFIED and records, per case, the loss it returns for the fp32 alphas of tests/opacity_loss_util.fixture_alphas()
and torch's autograd gradient with respect to them, into tests/golden/alpha_loss.npz.  Arrays and numbers only.

Cases: both modes (log a + log(1 - a), and force_opaque), each before and after init_epoch, and one with clamp_alpha = 3 so that
clamp_min cuts some terms; no term of that case may lie within 1e-3 of -clamp_alpha (checked here and again by the CPU test).

    python tools/gen_golden_alpha_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402
import opacity_loss_util as ou  # noqa: E402

CASES = [
    # name, lambda_alpha, clamp_alpha, init_epoch, force_opaque, epochs stepped before the call
    ("nv2_before", 0.5, 100.0, 2, False, 1),
    ("nv2_after", 0.5, 100.0, 2, False, 2),
    ("opaque_before", 0.25, 100.0, 1, True, 0),
    ("opaque_after", 0.25, 100.0, 1, True, 1),
    ("nv2_clamp3", 2.0, 3.0, 0, False, 0),
]
MARGIN = 1e-3


def main():
    from model.loss import AlphaLossNV2  # the reference's src/model/loss.py
    alphas = ou.fixture_alphas()
    out = {"names": np.array(",".join(c[0] for c in CASES)), "alpha": alphas}
    for name, lam, clamp_alpha, init_epoch, opaque, steps in CASES:
        crit = AlphaLossNV2(lam, clamp_alpha, init_epoch, force_opaque=opaque)
        if steps:
            crit.sched_step(steps)
        a = torch.from_numpy(alphas.copy()).requires_grad_(True)
        value = crit(a)
        if value.requires_grad:
            value.sum().backward()
            grad = a.grad.numpy().copy()
        else:
            grad = np.zeros_like(alphas)                    # before init_epoch: a constant zero
        if not opaque:
            raw, _ = ou.terms(alphas.astype(np.float64), ou.NV2, ou.REF_LO, ou.REF_HI, 1e30)
            assert (np.abs(raw + clamp_alpha) > MARGIN).all(), f"{name}: a term within {MARGIN} of -clamp_alpha"
        out[f"{name}__cfg"] = np.array([lam, clamp_alpha, init_epoch, float(opaque), steps], np.float64)
        out[f"{name}__value"] = value.detach().numpy().reshape(-1).astype(np.float32)
        out[f"{name}__grad"] = grad.astype(np.float32)
        print(f"{name}: value {float(value.detach().reshape(-1)[0]):.9g}, {int((grad != 0).sum())} of {grad.size} gradients non-zero")
    path = os.path.join(gu.GOLDEN_DIR, "alpha_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
