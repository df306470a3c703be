"""Host model of the colour-jitter augmentation, written from include/pnr.h ("colour jitter"): the Philox draws of a record, the
Lehmer order, the chain on float32 pixels in [0, 1] — numpy's float32 arithmetic rounds every operation on its own, which is
what the header asks for — the fp64 grey mean, and the two gathers' outputs.  Shared by tests/test_color_jitter_cpu.py and
tests/test_gpu_color_jitter.py.

The chain takes `variant`, a planted mistake the pixel set must tell from the model, and `counts`, a dict it fills with how
often each branch ran (hue sectors, maxc branches, the grey case, low and high clamps per operation)."""
import itertools

import numpy as np

from sampler_util import philox4x32_10, u01

DRAW_JITTER = 10
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
F = np.float32
GRAY_W = (F(0.2989), F(0.587), F(0.114))
# "no_fixup" drops hue's 1.0 -> 0.0 fix-up together with the `i mod 6` behind it (sector 6 matches no row: zeros, as a chain
# without either would give); "no_fixup_mod" drops the fix-up alone, which `i mod 6` makes invisible (6 H' = 6 gives i = 0, f = 0,
# the bits of H' = 0)
VARIANTS = ("no_clamp", "reversed", "hue_sign", "gray_perm", "balanced_first", "no_fixup")


# ------------------------------------------------------------------------------------------------------------ draws
def jitter_counter(seed, o, block):
    """(key0, key1, c0, c1, c2, c3) of object o's block: the samplers' layout with draw id 10."""
    return (seed & 0xFFFFFFFF, seed >> 32, o & 0xFFFFFFFF, (o >> 32) & 0xFFFFFFFF, DRAW_JITTER, block)


def order_of(code):
    """The Lehmer code q in [0, 24) over [brightness, contrast, saturation, hue] -> the four operations in order."""
    left = [BRIGHTNESS, CONTRAST, SATURATION, HUE]
    out = [left.pop(code // 6), left.pop((code % 6) // 2), left.pop(code % 2)]
    return out + left


def code_of(order):
    """The inverse of order_of."""
    for q in range(24):
        if order_of(q) == list(order):
            return q
    raise ValueError(order)


def draw_records(seed, SB, ranges):
    """-> (SB, 8) float32 records with mean 0: [brightness, contrast, saturation, hue, 0, code, 0, 0]."""
    o = np.arange(SB, dtype=np.uint64)
    lo32, hi32 = o & np.uint64(0xFFFFFFFF), o >> np.uint64(32)
    a = philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, lo32, hi32, DRAW_JITTER, 0)
    b = philox4x32_10(seed & 0xFFFFFFFF, seed >> 32, lo32, hi32, DRAW_JITTER, 1)
    rec = np.zeros((SB, 8), F)
    for k in range(4):
        centre, rng = F(0.0 if k == HUE else 1.0), F(ranges[k])
        lo, hi = F(centre - rng), F(centre + rng)
        rec[:, k] = lo + (F(hi - lo) * u01(a[k])).astype(F)
    rec[:, 5] = ((b[0] * np.uint64(24)) >> np.uint64(32)).astype(F)
    return rec


# ------------------------------------------------------------------------------------------------------------ the chain
def _clamp(v, name, counts, variant):
    if counts is not None:
        counts[name + "_low"] = counts.get(name + "_low", 0) + int((v < 0).sum())
        counts[name + "_high"] = counts.get(name + "_high", 0) + int((v > 1).sum())
    if variant == "no_clamp":
        return v
    return np.where(v < 0, F(0), np.where(v > 1, F(1), v)).astype(F)


def gray(x, variant=None):
    w = (GRAY_W[1], GRAY_W[0], GRAY_W[2]) if variant == "gray_perm" else GRAY_W
    return ((w[0] * x[:, 0] + w[1] * x[:, 1]) + w[2] * x[:, 2]).astype(F)


def hue_op(x, h, counts=None, variant=None):
    h = F(-h) if variant == "hue_sign" else F(h)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    eq = maxc == minc
    cr = maxc - minc
    one = np.ones_like(maxc)
    s = cr / np.where(eq, one, maxc)
    d = np.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
    is_r, is_g = maxc == r, (maxc == g) & (maxc != r)
    is_b = (maxc != g) & (maxc != r)
    zero = np.zeros_like(maxc)
    hr, hg, hb = np.where(is_r, bc - gc, zero), np.where(is_g, (F(2) + rc) - bc, zero), np.where(is_b, (F(4) + gc) - rc, zero)
    H = ((hr + hg) + hb) / F(6) + F(1)
    H = np.fmod(H, F(1)).astype(F)
    t = H + h
    H = (t - np.floor(t)).astype(F)
    if counts is not None:
        counts["fixup"] = counts.get("fixup", 0) + int((H == 1).sum())
        counts["eq"] = counts.get("eq", 0) + int(eq.sum())
        for name, m in (("max_r", is_r), ("max_g", is_g), ("max_b", is_b)):
            counts[name] = counts.get(name, 0) + int((m & ~eq).sum())
    if variant not in ("no_fixup", "no_fixup_mod"):
        H = np.where(H == 1, F(0), H)
    h6 = H * F(6)
    fi = np.floor(h6)
    f = h6 - fi
    i = fi.astype(np.int64) if variant == "no_fixup" else fi.astype(np.int64) % 6
    v = maxc
    p = _clamp(v * (F(1) - s), "hue", None, None)
    q = _clamp(v * (F(1) - s * f), "hue", None, None)
    u = _clamp(v * (F(1) - s * (F(1) - f)), "hue", None, None)
    if counts is not None:
        for k in range(6):
            counts[f"sector{k}"] = counts.get(f"sector{k}", 0) + int(((i == k) & ~eq).sum())
    rows = ((v, u, p), (q, v, p), (p, v, u), (p, q, v), (u, p, v), (v, p, q))
    out = np.empty_like(x)
    for ch in range(3):
        out[:, ch] = np.select([i == k for k in range(6)], [rows[k][ch] for k in range(6)], default=F(0)).astype(F)
    assert out.dtype == np.float32
    return out


def chain(x, rec, until_contrast=False, counts=None, variant=None):
    """x (N, 3) float32 in [0, 1] through the record's operations in its order; identities are skipped."""
    x = np.array(x, dtype=F)
    fb, fc, fs, fh, mean = (F(v) for v in rec[:5])
    order = order_of(int(rec[5]))
    if variant == "reversed":
        order = order[::-1]
    for op in order:
        if op == BRIGHTNESS:
            if fb != 1:
                x = _clamp(fb * x, "brightness", counts, variant)
        elif op == CONTRAST:
            if until_contrast:
                return x
            if fc != 1:
                x = _clamp(fc * x + F(F(1) - fc) * mean, "contrast", counts, variant)
        elif op == SATURATION:
            if fs != 1:
                x = _clamp(fs * x + (F(F(1) - fs) * gray(x, variant))[:, None], "saturation", counts, variant)
        elif fh != 0:
            x = hue_op(x, fh, counts, variant)
        assert x.dtype == np.float32
    return x


def unit(b):
    """float(b) / 255.0f, one correctly rounded division."""
    return (np.asarray(b).astype(F) / F(255)).astype(F)


def balance(y, balanced):
    return ((y - F(0.5)) / F(0.5)).astype(F) if balanced else y


def mean64(images_u8, rec):
    """The object's grey mean as the header defines it, in fp64: images_u8 (NV, H, W, C) -> float64."""
    x = unit(images_u8[..., :3].reshape(-1, 3))
    g = gray(chain(x, rec, until_contrast=True))
    return float(g.astype(np.float64).sum() / g.size)


def with_mean(rec, images_u8, per_view=None):
    """A copy of the record whose mean is the model's (0 for a contrast factor of exactly 1).  per_view: the planted variant
    that takes the mean over that view only."""
    rec = np.array(rec, dtype=F)
    rec[4] = 0.0 if rec[1] == 1 else F(mean64(images_u8 if per_view is None else images_u8[per_view:per_view + 1], rec))
    return rec


def model_rgb_gt(bytes3, rec, balanced, variant=None, counts=None):
    """bytes (N, 3) uint8 of one object -> rgb_gt (N, 3): 0.5 T + 0.5 of the chained pixel."""
    if variant == "balanced_first":
        y = chain(balance(unit(bytes3), balanced), rec, counts=counts)
    else:
        y = balance(chain(unit(bytes3), rec, counts=counts, variant=variant), balanced)
    return (F(0.5) * y + F(0.5)).astype(F)


def model_views(view_u8, rec, balanced, variant=None):
    """One view (H, W, C) uint8 -> planes (3, H, W) float32."""
    Hh, Ww = view_u8.shape[:2]
    y = balance(chain(unit(view_u8[..., :3].reshape(-1, 3)), rec, variant=variant), balanced)
    return np.ascontiguousarray(y.reshape(Hh, Ww, 3).transpose(2, 0, 1))


# ------------------------------------------------------------------------------------------------------------ the pixel set
def pixel_set():
    """The GPU cases' pixels, (97, 3) uint8: the 8 corner colours, six named ones and 83 random byte triples."""
    corners = [[a, b, c] for a, b, c in itertools.product((0, 255), repeat=3)]
    named = [[200, 200, 10], [10, 200, 200], [200, 10, 200], [7, 7, 7], [128, 128, 128], [254, 255, 255]]
    rnd = np.random.default_rng(20241020).integers(0, 256, (83, 3)).tolist()
    return np.array(corners + named + rnd, dtype=np.uint8)


def written_records(identity=True):
    """Records the tests write themselves: all 24 orders with factors cycling through 0.85 / 1.15 and hue -+0.15 (mean set by
    the caller), plus one identity record."""
    recs = []
    for q in range(24):
        f = [F(0.85) if (q >> k) & 1 else F(1.15) for k in range(3)]
        recs.append([f[0], f[1], f[2], F(0.15) if q % 3 else F(-0.15), 0.0, float(q), 0.0, 0.0])
    if identity:
        recs.append([1.0, 1.0, 1.0, 0.0, 0.0, 7.0, 0.0, 0.0])
    return np.array(recs, dtype=F)


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))
