"""Host model of pnr_train_draw_at, written from the text of include/pnr.h on top of train_draw_util's pieces: the call's object o
is object obj_base + o of the step, and only the counters see it —

    pixel (o, j)        counter (lo32(r), hi32(r), 8, 0) with r = (obj_base + o) * B + j, a 64-bit index
    views of object o   counter (lo32(obj_base + o), hi32(obj_base + o), 9, s >> 2)

The boxes and the outputs are the call's own SB rows.  Python ints and uint64 arrays, so the high counter word is exact."""
import numpy as np

import train_draw_util as du
from sampler_util import philox4x32_10

M32 = du.M32


def model_draw_at(bbox, SB, NV, W, H, B, NS, seed, obj_base):
    """-> (pix_inds (SB, B) int64, view_ord (SB, NS) int64)."""
    seed, obj_base = int(seed), int(obj_base)
    assert 0 <= obj_base and (obj_base + SB) * max(B, 1) < 1 << 63
    k0, k1 = seed & M32, seed >> 32
    pix = np.empty((SB, B), np.int64)
    if B:
        r = np.uint64(obj_base * B) + np.arange(SB * B, dtype=np.uint64)
        x, y, z, _ = philox4x32_10(k0, k1, r & np.uint64(M32), r >> np.uint64(32), du.DRAW_PIX, 0)
        for i in range(SB * B):
            o = i // B
            _, idx = du.pixel_from_words(int(x[i]), int(y[i]), int(z[i]), (lambda view: bbox[o][view]) if bbox is not None else None,
                                         NV, W, H, bbox is not None)
            pix[o, i % B] = idx
    order = np.empty((SB, NS), np.int64)
    if NS:
        o = (np.uint64(obj_base) + np.arange(SB, dtype=np.uint64))[:, None]
        blk = np.arange((NS + 3) // 4, dtype=np.uint64)[None, :]
        w = philox4x32_10(k0, k1, o & np.uint64(M32), o >> np.uint64(32), du.DRAW_VIEWS, blk)
        words = np.stack(w, axis=-1).reshape(SB, -1)[:, :NS]
        for i in range(SB):
            order[i] = du.views_from_words([int(v) for v in words[i]], NV)
    return pix, order
