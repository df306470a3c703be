"""numpy restatement of include/pnr.h's pnr_upsample_concat / pnr_upsample_concat_bwd (upstream pixelNeRF's latent map: every
level resized to level 0's size, bilinear with align_corners=True, and concatenated along the channels).

model32        the specification itself: fp32, one rounding per operation (numpy rounds every float32 operation on its own)
model64        the same formulas in fp64 — the exact operator up to 1e-16
adjoint64      the fp64 adjoint of model64, per level
adjoint_abs64  the adjoint applied to |g| with |w|: the scale an elementwise error bound of the backward is relative to
adjoint32w     the backward kernel's arithmetic: tap weights w = fl32(wy wx) from model32's lam / mu, products and sums in fp64
               (before its single final rounding)
Levels are (N, C, H, W) arrays; shapes are the tuples of their shapes."""
import numpy as np

# the level lists of the tests, (C, H, W) per level
CASES = {
    "A": (2, [(3, 7, 5), (2, 4, 3), (5, 2, 2), (1, 1, 1)]),        # non-integer ratios, a one-texel level, odd channels
    "B": (1, [(8, 6, 9), (8, 6, 9), (16, 3, 5), (32, 2, 3)]),      # an identity level, sumC = 64 for out16
    "C": (1, [(2, 1, 4), (3, 5, 2)]),                              # H_0 = 1 and a level larger than level 0
    "D": (3, [(4, 3, 300), (4, 2, 70)]),                           # rows longer than a workgroup
}
CPU_CASES = dict(CASES)
CPU_CASES["srn"] = (1, [(2, 64, 64), (2, 8, 8), (2, 16, 16), (2, 32, 32)])
CPU_CASES["dtu"] = (1, [(2, 150, 200), (2, 19, 25)])


def make_levels(name, seed=0, cases=CPU_CASES):
    """relu(N(0, 1)) maps, like post-ReLU ResNet features."""
    n, shapes = cases[name]
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    return [np.maximum(rng.standard_normal((n, c, h, w)), 0).astype(np.float32) for c, h, w in shapes]


def make_cotangent(name, seed=0, cases=CPU_CASES):
    n, shapes = cases[name]
    rng = np.random.default_rng(2000 + seed + sum(map(ord, name)))
    return rng.standard_normal((n, sum(c for c, _, _ in shapes), shapes[0][1], shapes[0][2])).astype(np.float32)


def axis_pos(n_in, n_out, dt):
    """Taps and weights of every fine index of one axis: i0, i1 (int), lam, mu (dt)."""
    D = np.arange(n_out, dtype=np.int64)
    if n_in == 1 or n_out == 1:
        i0 = np.zeros(n_out, np.int64)
        lam = np.zeros(n_out, dt)
    else:
        num = D * (n_in - 1)
        i0 = num // (n_out - 1)
        lam = (num % (n_out - 1)).astype(dt) / dt(n_out - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    mu = dt(1.0) - lam
    assert lam.dtype == dt and mu.dtype == dt
    return i0, i1, lam, mu


def _resize(x, H0, W0, dt):
    x = x.astype(dt)
    h, w = x.shape[2:]
    if (h, w) == (H0, W0):
        return x.copy()
    y0, y1, ly, my = axis_pos(h, H0, dt)
    x0, x1, lx, mx = axis_pos(w, W0, dt)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = mx * r0[..., x0] + lx * r0[..., x1]          # each product and each sum is rounded to dt
    bot = mx * r1[..., x0] + lx * r1[..., x1]
    out = my[:, None] * top + ly[:, None] * bot
    assert out.dtype == dt
    return out


def model32(levels):
    H0, W0 = levels[0].shape[2:]
    return np.concatenate([_resize(l, H0, W0, np.float32) for l in levels], axis=1)


def model64(levels):
    H0, W0 = levels[0].shape[2:]
    return np.concatenate([_resize(l, H0, W0, np.float64) for l in levels], axis=1)


def _adjoint(g, shapes, wdt, absolute):
    g = np.abs(g.astype(np.float64)) if absolute else g.astype(np.float64)
    H0, W0 = shapes[0][2:]
    out, c = [], 0
    for n, C, h, w in shapes:
        gl = g[:, c:c + C]
        c += C
        if (h, w) == (H0, W0):
            out.append(gl.copy())
            continue
        y0, y1, ly, my = axis_pos(h, H0, wdt)
        x0, x1, lx, mx = axis_pos(w, W0, wdt)
        d = np.zeros((n, C, h, w), np.float64)
        for iy, wy in ((y0, my), (y1, ly)):
            for ix, wx in ((x0, mx), (x1, lx)):
                wgt = wy[:, None] * wx[None, :]                     # rounded to wdt: the kernel's w for wdt = float32
                assert wgt.dtype == wdt
                np.add.at(d, (slice(None), slice(None), iy[:, None], ix[None, :]), wgt.astype(np.float64) * gl)
        out.append(d)
    return out


def adjoint64(g, shapes):
    return _adjoint(g, shapes, np.float64, False)


def adjoint_abs64(g, shapes):
    return _adjoint(g, shapes, np.float64, True)


def adjoint32w(g, shapes):
    return _adjoint(g, shapes, np.float32, False)


def torch_reference(levels, dtype):
    """torch's own F.interpolate(mode="bilinear", align_corners=True) + cat on the CPU, and the leaf tensors it was built from."""
    import torch
    import torch.nn.functional as F
    leaves = [torch.from_numpy(l).to(dtype).requires_grad_(True) for l in levels]
    size = tuple(leaves[0].shape[2:])
    out = torch.cat([F.interpolate(l, size=size, mode="bilinear", align_corners=True) for l in leaves], dim=1)
    return out, leaves
