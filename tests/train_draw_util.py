"""Host model of pnr_train_draw, written from the text of include/pnr.h with sampler_util's Philox4x32-10 and Python ints.

Layout: key = (seed lo32, seed hi32).  Pixel (o, j): counter (lo32(r), hi32(r), 8, 0) with r = o B + j; words x, y, z give
the view, the column and the row through mulhi(x, n) = (x * n) >> 32.  Views of object o: draw s is word s & 3 of the block
with counter (lo32(o), hi32(o), 9, s >> 2)."""
import math

import numpy as np

from sampler_util import philox4x32_10

DRAW_PIX, DRAW_VIEWS = 8, 9
M32 = 0xFFFFFFFF


def mulhi(x, n):
    return (int(x) * int(n)) >> 32


def pixel_counter(seed, o, j, B):
    """(key0, key1, c0, c1, c2, c3) of pixel (o, j), plain ints."""
    r = o * B + j
    return (seed & M32, seed >> 32, r & M32, (r >> 32) & M32, DRAW_PIX, 0)


def view_counter(seed, o, s):
    """(key0, key1, c0, c1, c2, c3, word) of view draw s of object o, plain ints."""
    return (seed & M32, seed >> 32, o & M32, (o >> 32) & M32, DRAW_VIEWS, s >> 2, s & 3)


def box_of(b):
    """The four floats of a box -> (cmin, rmin, cmax, rmax) ints, or None when one of them is not finite."""
    if not all(math.isfinite(float(v)) for v in b):
        return None
    return tuple(int(float(v)) for v in b)           # int() truncates towards zero


def pixel_from_words(x, y, z, box, NV, W, H, boxed):
    """(view, index) of one pixel from its three words; box = the four floats of bbox[o, view] (looked up by the caller)."""
    view = mulhi(x, NV)
    if boxed:
        ib = box_of(box(view))
        if ib is None:
            return view, -1
        cmin, rmin, cmax, rmax = ib
        if not (0 <= cmin <= cmax < W and 0 <= rmin <= rmax < H):
            return view, -1
        col = cmin + mulhi(y, cmax + 1 - cmin)
        row = rmin + mulhi(z, rmax + 1 - rmin)
    else:
        col, row = mulhi(y, W), mulhi(z, H)
    return view, view * H * W + row * W + col


def views_from_words(words, NV):
    """The ordered subset from word_0 .. word_{NS-1}: t = mulhi(word_s, NV - s), pushed past every chosen view c <= t walking
    the chosen ones in ascending order."""
    chosen, out = [], []
    for s, w in enumerate(words):
        t = mulhi(w, NV - s)
        for c in sorted(chosen):
            if t >= c:
                t += 1
        chosen.append(t)
        out.append(t)
    return out


def model_draw(bbox, SB, NV, W, H, B, NS, seed):
    """-> (pix_inds (SB, B) int64, view_ord (SB, NS) int64, views (SB, B) int64: the view each pixel drew)."""
    seed = int(seed)
    k0, k1 = seed & M32, seed >> 32
    pix = np.empty((SB, B), np.int64)
    pview = np.empty((SB, B), np.int64)
    if B:
        r = np.arange(SB * B, dtype=np.uint64)
        x, y, z, _ = philox4x32_10(k0, k1, r & np.uint64(M32), r >> np.uint64(32), DRAW_PIX, 0)
        for i in range(SB * B):
            o = i // B
            v, idx = pixel_from_words(int(x[i]), int(y[i]), int(z[i]), (lambda view: bbox[o][view]) if bbox is not None else None,
                                      NV, W, H, bbox is not None)
            pview[o, i % B], pix[o, i % B] = v, idx
    order = np.empty((SB, NS), np.int64)
    if NS:
        o = np.arange(SB, dtype=np.uint64)[:, None]
        blk = np.arange((NS + 3) // 4, dtype=np.uint64)[None, :]
        w = philox4x32_10(k0, k1, o & np.uint64(M32), o >> np.uint64(32), DRAW_VIEWS, blk)
        words = np.stack(w, axis=-1).reshape(SB, -1)[:, :NS]              # (SB, blocks, 4) -> draw s = block s >> 2, word s & 3
        for i in range(SB):
            order[i] = views_from_words([int(v) for v in words[i]], NV)
    return pix, order, pview
