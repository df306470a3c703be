"""The numpy model of include/pnr.h's visualisation arithmetic (quantize, cmap, opacity, panel, mse, stats), written from the
header's text and independently of pixel_nerf_multiscale_amd.util.cmap, plus the helpers the vis tests share."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_quantize.npz")
F32 = np.float32


def load_quantize_fixture():
    z = np.load(GOLDEN, allow_pickle=False)
    return {n: (z[n + "__map"], z[n + "__u8"]) for n in str(z["names"]).split(",")}


def model_lut():
    """The default table from its definition, entry by entry in Python floats (fp64)."""
    clamp = lambda v: min(1.0, max(0.0, v))
    rows = []
    for i in range(256):
        x = i / 255
        rows.append([int(255 * v + 0.5) for v in (min(1.0, x / 0.375), clamp((x - 0.375) / 0.375), clamp((x - 0.75) / 0.25))])
    return np.array(rows, dtype=np.uint8)


def minmax(m):
    """fp32 (min, max); a NaN anywhere makes both NaN."""
    m = np.asarray(m, F32)
    if np.isnan(m).any():
        return F32(np.nan), F32(np.nan)
    return F32(m.min()), F32(m.max())


def quantize(m):
    m = np.asarray(m, F32)
    vmin, vmax = minmax(m)
    with np.errstate(all="ignore"):
        if float(F32(vmax - vmin)) < 1e-10:
            vmax = F32(float(vmax) + 1e-10)
        den = F32(vmax - vmin)
        q = np.divide(np.subtract(m, vmin, dtype=F32), den, dtype=F32)
        p = np.multiply(q, F32(255.0), dtype=F32)
    out = np.zeros(m.shape, np.uint8)
    fin = np.isfinite(p)
    out[fin] = np.trunc(p[fin]).astype(np.int64).astype(np.uint8)
    return out


def cmap(m, lut):
    return lut[quantize(m)]


def alpha_of(weights):
    """Sequential ascending fp64 sum over k (the last column of a cumsum), rounded once to fp32."""
    return np.cumsum(np.asarray(weights, F32).astype(np.float64), axis=-1)[..., -1].astype(F32)


def image_tile(img):
    """(3, H, W) in [-1, 1] -> (H, W, 3) = img * 0.5 + 0.5 in fp32 (x * 0.5 is exact, so one rounding either way)."""
    return (np.asarray(img, F32) * F32(0.5) + F32(0.5)).transpose(1, 2, 0)


def to_u8(x):
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        c = np.where(x < 0, F32(0), np.where(x > 1, F32(1), x)).astype(F32)
        p = np.multiply(c, F32(255.0), dtype=F32)
    out = np.zeros(x.shape, np.uint8)
    ok = ~np.isnan(p)
    out[ok] = np.trunc(p[ok]).astype(np.int64).astype(np.uint8)
    return out


def pieces(images, src_views, gt_view, passes, lut, W, H):
    """Per pass the list of (H, W, 3) float32 tiles in panel order, and the alpha maps."""
    rows, alphas = [], []
    for rgb, depth, weights in passes:
        a = alpha_of(weights).reshape(H, W)
        alphas.append(a)
        tiles = [image_tile(images[v]) for v in src_views] + [image_tile(images[gt_view])]
        tiles.append(cmap(np.asarray(depth, F32).reshape(H, W), lut).astype(F32) / F32(255.0))
        tiles.append(np.asarray(rgb, F32).reshape(H, W, 3))
        tiles.append(cmap(a, lut).astype(F32) / F32(255.0))
        rows.append(tiles)
    return rows, alphas


def panel_model(images, src_views, gt_view, passes, lut):
    """-> dict(panel (n_pass H, (NS + 4) W, 3) fp32, panel_u8, alpha (n_pass, H, W), stats (n_pass, 6), mse fp64).  The
    panel is filled tile by tile at its address; test_vis_cpu proves that equal to hstack / vstack of the pieces."""
    images = np.asarray(images, F32)
    _, _, H, W = images.shape
    NS, n_pass = len(src_views), len(passes)
    rows, alphas = pieces(images, src_views, gt_view, passes, lut, W, H)
    panel = np.zeros((n_pass * H, (NS + 4) * W, 3), F32)
    for p, tiles in enumerate(rows):
        for j, t in enumerate(tiles):
            panel[p * H:(p + 1) * H, j * W:(j + 1) * W] = t
    stats = np.zeros((n_pass, 6), F32)
    for p, (rgb, depth, _) in enumerate(passes):
        stats[p] = [*minmax(rgb), *minmax(alphas[p]), *minmax(depth)]
    x = np.asarray(passes[-1][0], F32).reshape(H, W, 3).astype(np.float64)
    g = image_tile(images[gt_view]).astype(np.float64)
    sq = ((x - g) ** 2).reshape(-1)
    mse = float(np.cumsum(sq)[-1] / (3.0 * H * W)) if not np.isnan(sq).any() else float("nan")
    return dict(panel=panel, panel_u8=to_u8(panel), alpha=np.stack(alphas), stats=stats, mse=mse)
