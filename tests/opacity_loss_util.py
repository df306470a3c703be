"""A numpy fp64 model of the opacity losses as include/pnr.h states them (pnr_alpha_loss / pnr_alpha_loss_bwd / pnr_mask_gather):
the weights' sum in the kernel's own order, the clamp, the three per-ray terms, their gates and gradients, and the bit a gathered
pixel reads.  A Variant plants one mistake at a time; the tests show that their checks catch each.

Nothing here touches the device or the library."""
from dataclasses import dataclass

import numpy as np

NV2, OPAQUE, MASK = 0, 1, 2
EPS32 = 2.0 ** -23
REF_LO, REF_HI = np.float32(0.01), np.float32(0.99)        # the reference's clamp constants, as fp32 holds them


@dataclass(frozen=True)
class Variant:
    no_clamp_gate: bool = False          # the clamp's gradient not gated
    inverted_min_gate: bool = False      # clamp_min's gate the wrong way round
    mean_over_nk: bool = False           # the mean taken over n * K instead of n
    lambda_twice: bool = False           # lambda applied to the per-ray term and again to the mean
    flip_one_minus_m: bool = False       # the sign of the (1 - m) term
    col_shift6: bool = False             # the gathered word indexed by col >> 6


RIGHT = Variant()


def alpha_sum(w):
    """(n, K) float32 -> (n,) float64 in the order the header fixes: lane l adds w[:, l], w[:, l + 64], .. ascending from +0, then
    the 64 lane sums fold by an xor butterfly over distances 32 .. 1.  Bit for bit what the device writes to alpha_out."""
    w = np.asarray(w, np.float32)
    n, K = w.shape
    chunks = (K + 63) // 64
    padded = np.zeros((n, chunks * 64), np.float64)
    padded[:, :K] = w.astype(np.float64)
    lanes = np.zeros((n, 64), np.float64)
    for c in range(chunks):
        lanes = lanes + padded[:, 64 * c:64 * c + 64]
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ d]
    return lanes[:, 0]


def clamp(alpha, lo, hi):
    """torch.clamp: both bounds pass at equality, a NaN stays a NaN."""
    return np.where(alpha < lo, lo, np.where(alpha > hi, hi, alpha))


def terms(alpha, mode, lo, hi, clamp_alpha=0.0, m=None, v=RIGHT):
    """alpha (n,) float64 -> (t (n,), dt/dalpha (n,)), float64, gates applied."""
    alpha = np.asarray(alpha, np.float64)
    lo, hi, ca = float(lo), float(hi), float(clamp_alpha)
    with np.errstate(all="ignore"):
        a = clamp(alpha, lo, hi)
        if mode == OPAQUE:
            t, g = -np.log(a), -1.0 / a
        elif mode == MASK:
            m = np.asarray(m, np.float64)
            s = -1.0 if v.flip_one_minus_m else 1.0
            t = -(m * np.log(a) + s * (1.0 - m) * np.log(1.0 - a))
            g = -(m / a - s * (1.0 - m) / (1.0 - a))
        else:
            raw = np.log(a) + np.log(1.0 - a)
            cut = raw < -ca
            t = np.where(cut, -ca, raw)
            g = 1.0 / a - 1.0 / (1.0 - a)
            g = np.where(~cut if v.inverted_min_gate else cut, 0.0, g)
            g = np.where(np.isnan(raw), raw, g)
        if not v.no_clamp_gate:
            g = np.where((alpha < lo) | (alpha > hi), 0.0, g)
    return t, g


def fold(t):
    """(n,) float64 -> the sum in the device's order: ray r in thread r % 1024 ascending, butterfly per wave, waves ascending."""
    n = t.shape[0]
    rounds = (n + 1023) // 1024
    padded = np.zeros(rounds * 1024, np.float64)
    padded[:n] = t
    acc = np.zeros(1024, np.float64)
    for r in range(rounds):
        acc = acc + padded[1024 * r:1024 * r + 1024]
    lanes = acc.reshape(16, 64)
    idx = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ d]
    total = lanes[0, 0]
    for w in range(1, 16):
        total = total + lanes[w, 0]
    return total


def one_pass(w, mode, lam, lo, hi, clamp_alpha=0.0, m=None, d_total=1.0, v=RIGHT):
    """One pass: w (n, K) float32 -> dict(alpha (n,), loss = lambda * L (float64), grad (n,) float64: d total / d w[r, k], the
    same for every k)."""
    w = np.asarray(w, np.float32)
    n, K = w.shape
    alpha = alpha_sum(w)
    t, g = terms(alpha, mode, lo, hi, clamp_alpha, m, v)
    lam = float(lam)
    count = float(n * K if v.mean_over_nk else n)
    if v.lambda_twice:
        t, g = lam * t, lam * g
    with np.errstate(all="ignore"):
        loss = lam * (fold(t) / count) if n else 0.0
        grad = float(d_total) * (lam / count * g) if n else g
    return dict(alpha=alpha, loss=loss, grad=grad)


def model(coarse_w, fine_w, mask, mode, lam_c, lam_f, lo, hi, clamp_alpha=0.0, d_total=1.0, v=RIGHT):
    """pnr_alpha_loss and its backward -> dict(stats64 (2,) float64 [lambda_c Lc, lambda_f Lf] (0 for a None pass), stats32 (3,)
    float32 as the device rounds them, alpha (2, n) float64 (NaN rows for a None pass), grad_c / grad_f (n,) float64 or None)."""
    n = (coarse_w if coarse_w is not None else fine_w).shape[0]
    out = dict(stats64=np.zeros(2), alpha=np.full((2, n), np.nan), grad_c=None, grad_f=None)
    for k, (w, lam, name) in enumerate(((coarse_w, lam_c, "grad_c"), (fine_w, lam_f, "grad_f"))):
        if w is None:
            continue
        p = one_pass(w, mode, lam, lo, hi, clamp_alpha, mask, d_total, v)
        out["stats64"][k], out["alpha"][k], out[name] = p["loss"], p["alpha"], p["grad"]
    with np.errstate(all="ignore"):
        s32 = out["stats64"].astype(np.float32)
        out["stats32"] = np.array([s32[0], s32[1], np.float32(s32[0] + s32[1])], np.float32)
    return out


def within_one_rounding(got, want64):
    """got (float32 values) within 2^-23 relative of the fp64 model — one rounding, doubled; NaNs and infinities must coincide."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    finite = np.isfinite(want64)
    same_special = np.array_equal(np.isnan(got), np.isnan(want64)) and np.array_equal(got[~finite & ~np.isnan(want64)],
                                                                                       want64[~finite & ~np.isnan(want64)])
    return bool(same_special and (np.abs(got[finite] - want64[finite]) <= EPS32 * np.abs(want64[finite])).all())


def fixture_criterion(got, v_ref, v64):
    """|got - v_ref| <= |v_ref - v64| + 2^-23 |v64|: the reference's own fp32 error plus one fp32 rounding, elementwise."""
    got, v_ref, v64 = (np.asarray(x, np.float64) for x in (got, v_ref, v64))
    return bool((np.abs(got - v_ref) <= np.abs(v_ref - v64) + EPS32 * np.abs(v64)).all())


# ------------------------------------------------------------------------------------------------------------ the gather
def gather(bits, pix, NV, H, W, v=RIGHT):
    """bits (SB, NV * H, ceil(W / 32)) uint32, pix (SB, B) int64 -> (SB, B) float32: the pixel's bit as 1 / 0, NaN for an index
    outside [0, NV * H * W).  Indexes numpy arrays, so a read outside bits[o] would raise."""
    bits, pix = np.asarray(bits), np.asarray(pix)
    SB, B = pix.shape
    out = np.full((SB, B), np.nan, np.float32)
    for o in range(SB):
        for j in range(B):
            p = int(pix[o, j])
            if 0 <= p < NV * H * W:
                row, col = divmod(p, W)
                word = int(bits[o, row, (col >> 6) if v.col_shift6 else (col >> 5)])
                out[o, j] = float((word >> (col & 31)) & 1)
    return out


def fixture_alphas():
    """The fp32 alphas tools/gen_golden_alpha_loss.py feeds the reference: values below 0.01, above 0.99, exactly 0.01f and 0.99f,
    their fp32 neighbours, and random ones in between — 64 in all."""
    lo, hi = REF_LO, REF_HI
    edge = [0.0, 0.005, np.nextafter(lo, np.float32(0)), lo, np.nextafter(lo, np.float32(1)), 0.5,
            np.nextafter(hi, np.float32(0)), hi, np.nextafter(hi, np.float32(1)), 0.995, 1.0, 1.25]
    rng = np.random.default_rng(2024)
    rest = rng.uniform(0.02, 0.98, 64 - len(edge))
    return np.concatenate([np.array(edge, np.float32), rest.astype(np.float32)]).astype(np.float32)
