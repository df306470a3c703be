"""Host model of pnr_mask_table_build and pnr_train_draw_masked, written from the text of include/pnr.h with numpy, Python ints
and sampler_util's Philox4x32-10.

Table: pixel p = (view * H + row) * W + col is inside iff byte >= thresh; bit col & 31 of word col >> 5 of row view * H + row,
LSB first, tail bits zero; rows = the prefix of the rows' popcounts, R + 1 entries.
Draw: pixel (o, j), r = (obj_base + o) * B + j, x = word 0 of philox(seed; lo32(r), hi32(r), 11, 0); slot j < B_inside takes the
k-th inside pixel, k = mulhi(x, n_in), the others the k-th outside pixel, k = mulhi(x, n_out); an empty population hands its
slots to the other one.  The selection is the two-step one of the header: an upper-bound search over the prefix, then a walk of
the row's words.  The views are train_draw_util's.

`Variant` switches single decisions of the model to a plausible wrong one: the tests plant each and ask that it is caught."""
import dataclasses

import numpy as np

import train_draw_util as du
from sampler_util import philox4x32_10

DRAW_MASK_PIX = 11
M32 = 0xFFFFFFFF

# (N, NV, H, W): one pixel; 31 / 32 / 33 around a word; 63 / 64 / 65 around a ballot; 130 = three ballots, the last of 2 lanes;
# rows of 65 words; R = 1200 and 5000 rows, past one scan chunk of 256
TABLE_SHAPES = [(1, 1, 1, 1), (2, 2, 3, 31), (2, 2, 3, 32), (1, 3, 2, 33), (1, 1, 4, 63), (1, 1, 4, 64), (1, 1, 4, 65), (1, 2, 1, 130),
                (3, 1, 5, 2049), (1, 3, 400, 5), (2, 5, 1000, 1)]


@dataclasses.dataclass(frozen=True)
class Variant:
    msb_first: bool = False          # bit 31 - (col & 31) instead of col & 31
    tail_outside: bool = False       # n_out counts the tail bits: R * Wd * 32 - n_in
    lower_bound: bool = False        # the row before the first prefix >= k instead of the last row with cum[r] <= k
    floor_inside: bool = False       # B_inside = floor(B * prop) instead of int(B * prop + 0.5)
    per_view: bool = False           # a uniform view first, then its own population, instead of all views pooled
    no_tail_mask: bool = False       # the complemented last word keeps its tail bits


RIGHT = Variant()


def n_inside(B, prop, v=RIGHT):
    return int(B * prop) if v.floor_inside else int(B * prop + 0.5)


def inside_of(masks_u8, thresh=128):
    """(N, NV, H, W) uint8 -> bool, the header's `byte >= thresh`."""
    return np.asarray(masks_u8) >= thresh


def model_table(inside, v=RIGHT):
    """inside (N, NV, H, W) bool -> (bits (N, R, Wd) uint32, rows (N, R + 1) uint32)."""
    N, NV, H, W = inside.shape
    R, Wd = NV * H, (W + 31) // 32
    flat = inside.reshape(N, R, W)
    bits = np.zeros((N, R, Wd), np.uint32)
    for col in range(W):
        sh = 31 - (col & 31) if v.msb_first else col & 31
        bits[:, :, col >> 5] |= flat[:, :, col].astype(np.uint32) << np.uint32(sh)
    rows = np.zeros((N, R + 1), np.uint32)
    rows[:, 1:] = np.cumsum(flat.sum(axis=2), axis=1)
    return bits, rows


def brute_table(inside):
    """The same table one pixel at a time, in Python ints."""
    N, NV, H, W = inside.shape
    R, Wd = NV * H, (W + 31) // 32
    bits = np.zeros((N, R, Wd), np.uint32)
    rows = np.zeros((N, R + 1), np.uint32)
    for n in range(N):
        count = 0
        for r in range(R):
            words = [0] * Wd
            for col in range(W):
                if inside[n, r // H, r % H, col]:
                    words[col >> 5] |= 1 << (col & 31)
                    count += 1
            bits[n, r] = words
            rows[n, r + 1] = count
    return bits, rows


def popcount(x):
    return bin(int(x)).count("1")


def select(bits, rows, W, k, want_inside, v=RIGHT):
    """The k-th pixel of one object's population, from its table alone: bits (R, Wd), rows (R + 1,).  -> linear index or -1."""
    R, Wd = bits.shape
    cum = (lambda r: int(rows[r])) if want_inside else (lambda r: r * W - int(rows[r]))
    if v.lower_bound:
        first = 0
        while first < R and cum(first) < k:         # std::lower_bound: the first entry >= k
            first += 1
        lo = max(first - 1, 0)
    else:
        lo, hi = 0, R
        while hi - lo > 1:
            mid = lo + ((hi - lo) >> 1)
            if cum(mid) <= k:
                lo = mid
            else:
                hi = mid
    rem = k - cum(lo)
    if rem < 0:
        return -1
    for q in range(Wd):
        word = int(bits[lo, q]) if want_inside else ~int(bits[lo, q]) & M32
        if q == Wd - 1 and W & 31 and not v.no_tail_mask:
            word &= (1 << (W & 31)) - 1
        c = popcount(word)
        if rem < c:
            for _ in range(rem):
                word &= word - 1
            low = (word & -word).bit_length() - 1
            col = q * 32 + (31 - low if v.msb_first else low)
            return lo * W + col
        rem -= c
    return -1


def pixel_words(seed, SB, B, obj_base=0):
    """Word 0 of every pixel's block: (SB, B) Python-int-valued uint64."""
    seed = int(seed)
    r = (np.arange(SB * B, dtype=np.uint64) + np.uint64(obj_base * B)) if SB * B else np.zeros(0, np.uint64)
    x = philox4x32_10(seed & M32, seed >> 32, r & np.uint64(M32), r >> np.uint64(32), DRAW_MASK_PIX, 0)[0]
    return np.asarray(x, np.uint64).reshape(SB, B)


def model_draw(bits, rows, SB, NV, W, H, B, B_inside, NS, seed, obj_base=0, v=RIGHT):
    """-> (pix_inds (SB, B) int64, view_ord (SB, NS) int64, from_inside (SB, B) bool: the population each slot drew from)."""
    R, Wd = NV * H, (W + 31) // 32
    assert bits.shape == (SB, R, Wd) and rows.shape == (SB, R + 1)
    x = pixel_words(seed, SB, B, obj_base)
    pix = np.empty((SB, B), np.int64)
    src = np.empty((SB, B), bool)
    for o in range(SB):
        n_in = int(rows[o, R])
        n_out = (R * Wd * 32 if v.tail_outside else R * W) - n_in
        for j in range(B):
            want = j < B_inside
            if (n_in if want else n_out) == 0:
                want = not want
            if v.per_view:
                view = du.mulhi(int(x[o, j]), NV)
                b, r = bits[o, view * H:(view + 1) * H], rows[o, view * H:(view + 1) * H + 1].astype(np.int64) - int(rows[o, view * H])
                n = int(r[H]) if want else H * W - int(r[H])
                idx = -1 if n == 0 else select(b, r, W, du.mulhi(int(x[o, j]) * 2654435761 & M32, n), want, v)
                pix[o, j] = idx if idx < 0 else view * H * W + idx
            else:
                pix[o, j] = select(bits[o], rows[o], W, du.mulhi(int(x[o, j]), n_in if want else n_out), want, v)
            src[o, j] = want
    order = np.empty((SB, NS), np.int64)
    if NS:
        _, order, _ = du.model_draw(None, SB, NV, 1, 1, 0, NS, seed) if obj_base == 0 else _views_at(SB, NV, NS, seed, obj_base)
    return pix, order, src


def brute_draw(inside, B, B_inside, seed, obj_base=0):
    """The pixels by the header's DEFINITION, no table: np.flatnonzero of the population, entry mulhi(x, n).  inside
    (SB, NV, H, W) bool -> (SB, B) int64."""
    SB = inside.shape[0]
    x = pixel_words(seed, SB, B, obj_base)
    pix = np.empty((SB, B), np.int64)
    for o in range(SB):
        pops = {True: np.flatnonzero(inside[o].ravel()), False: np.flatnonzero(~inside[o].ravel())}
        for j in range(B):
            want = j < B_inside
            if len(pops[want]) == 0:
                want = not want
            pix[o, j] = pops[want][du.mulhi(int(x[o, j]), len(pops[want]))]
    return pix


def _views_at(SB, NV, NS, seed, obj_base):
    """train_draw_util's views of objects obj_base .. obj_base + SB - 1 (its model has no object base: draw the head too)."""
    _, order, _ = du.model_draw(None, obj_base + SB, NV, 1, 1, 0, NS, seed)
    return None, order[obj_base:], None


def random_masks(N, NV, H, W, density, seed):
    """uint8 (N, NV, H, W): 255 with probability `density`, else 0."""
    rng = np.random.default_rng(seed)
    return (rng.random((N, NV, H, W)) < density).astype(np.uint8) * 255
