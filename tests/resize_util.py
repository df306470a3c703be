"""Shared by tests/test_resize_cpu.py and tests/test_gpu_resize.py: the numpy restatement of include/pnr.h's area resampling
(written from the header, not from the kernel), torch's own fp64 F.interpolate(mode="area") as the outside reference, the brute
force behind util.resize_bbox, and the byte and float inputs of the cases."""
import numpy as np
import torch

# (H, W) -> (Ht, Wt), each named for what it can break (tests/test_gpu_resize.py)
GPU_SHAPES = {
    "integer_ratio": ((8, 8), (4, 4)),
    "overlapping_windows": ((7, 5), (3, 2)),
    "identity_is_a_copy": ((5, 7), (5, 7)),
    "one_window_is_the_image": ((3, 3), (1, 1)),
    "odd_both_ways": ((13, 11), (5, 3)),
    "upsampling": ((5, 5), (7, 8)),
    "row_past_a_workgroup": ((2, 700), (1, 300)),
}
# the CPU comparison with torch: the seven above and three more (a 1 x 1 target of a wide image, a long thin one, a square
# non-integer ratio)
CPU_SHAPES = dict(GPU_SHAPES, wide_to_one=((4, 9), (1, 1)), thin=((31, 2), (4, 3)), square_ratio=((16, 16), (6, 6)))
BBOX_SHAPES = [((8, 8), (4, 4)), ((7, 5), (3, 2)), ((9, 6), (4, 5)), ((13, 11), (5, 3)), ((4, 4), (3, 3)), ((5, 5), (7, 8)),
               ((16, 12), (5, 9))]


# ---------------------------------------------------------------------------------------------------- the windows
def windows(n_in, n_out):
    """[(lo(i), hi(i))] for i < n_out, by integer arithmetic: floor(i n_in / n_out), ceil((i + 1) n_in / n_out)."""
    return [((i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def windows_by_round(n_in, n_out):
    """A planted mistake: the edges rounded to nearest instead of floor and ceil."""
    return [(int(round(i * n_in / n_out)), max(int(round((i + 1) * n_in / n_out)), int(round(i * n_in / n_out)) + 1))
            for i in range(n_out)]


# ---------------------------------------------------------------------------------------------------- bytes
def window_sums_u8(a, Ht, Wt, window=windows):
    """a uint8 (..., H, W, C) -> (S int64 (..., Ht, Wt, C): the exact window sums, n int64 (Ht, Wt): the pixel counts)."""
    a = np.asarray(a)
    H, W = a.shape[-3], a.shape[-2]
    rows, cols = window(H, Ht), window(W, Wt)
    S = np.zeros(a.shape[:-3] + (Ht, Wt, a.shape[-1]), np.int64)
    n = np.zeros((Ht, Wt), np.int64)
    for y, (r0, r1) in enumerate(rows):
        for x, (c0, c1) in enumerate(cols):
            S[..., y, x, :] = a[..., r0:r1, c0:c1, :].astype(np.int64).sum(axis=(-3, -2))
            n[y, x] = (r1 - r0) * (c1 - c0)
    return S, n


def round_half_up(S, n):
    n = n[..., None]
    return ((2 * S + n) // (2 * n)).astype(np.uint8)


def truncate(S, n):
    """A planted mistake: the mean cut off instead of rounded."""
    return (S // n[..., None]).astype(np.uint8)


def model_u8(a, Ht, Wt):
    """pnr_resize_area_u8 on a (..., H, W, C) uint8: (2 S + n) // (2 n)."""
    return round_half_up(*window_sums_u8(a, Ht, Wt))


def ties(S, n):
    """Where the window mean lies exactly half way between two bytes."""
    n = n[..., None]
    return (2 * S) % (2 * n) == n


# ---------------------------------------------------------------------------------------------------- floats
def model_f32(a, Ht, Wt):
    """pnr_resize_area_f32 on a (..., H, W) float32: the window summed in fp64 row-major, one term after the other, divided by n
    in fp64, rounded to fp32 once."""
    a = np.asarray(a)
    assert a.dtype == np.float32
    H, W = a.shape[-2], a.shape[-1]
    out = np.zeros(a.shape[:-2] + (Ht, Wt), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for y, (r0, r1) in enumerate(windows(H, Ht)):
            for x, (c0, c1) in enumerate(windows(W, Wt)):
                acc = np.zeros(a.shape[:-2], np.float64)
                for r in range(r0, r1):
                    for c in range(c0, c1):
                        acc = acc + a[..., r, c].astype(np.float64)
                out[..., y, x] = (acc / np.float64((r1 - r0) * (c1 - c0))).astype(np.float32)
    return out


def torch_area64(planes, Ht, Wt):
    """torch's own F.interpolate(mode="area") in fp64 on planes (..., H, W) -> float64 (..., Ht, Wt)."""
    t = torch.as_tensor(np.asarray(planes, dtype=np.float64))
    lead = t.shape[:-2]
    r = torch.nn.functional.interpolate(t.reshape(1, -1, *t.shape[-2:]), size=(Ht, Wt), mode="area")
    return r.reshape(*lead, Ht, Wt).numpy()


def ulp_distance(a, b):
    """Elementwise distance of two float32 arrays in units in the last place (the number of floats between them)."""
    def ordered(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


# ---------------------------------------------------------------------------------------------------- boxes
def target_mask(mask, Ht, Wt, window=windows):
    """A target pixel is foreground when ANY source pixel under its window is."""
    H, W = mask.shape
    out = np.zeros((Ht, Wt), bool)
    for y, (r0, r1) in enumerate(window(H, Ht)):
        for x, (c0, c1) in enumerate(window(W, Wt)):
            out[y, x] = mask[r0:r1, c0:c1].any()
    return out


def mask_box(mask):
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    return np.array([cols[0], rows[0], cols[-1], rows[-1]], dtype=np.float32)


def brute_force_bbox(box, src, dst):
    """The box (cmin, rmin, cmax, rmax) of a filled source box's mask after the resampling, by building both masks."""
    (H, W), (Ht, Wt) = src, dst
    cmin, rmin, cmax, rmax = (int(v) for v in box)
    mask = np.zeros((H, W), bool)
    mask[rmin:rmax + 1, cmin:cmax + 1] = True
    return mask_box(target_mask(mask, Ht, Wt))


def bbox_cases(src, seed):
    """Boxes of an (H, W) image: the whole image, one touching each edge alone, every corner and the centre as one-pixel
    boxes, and 40 random ones."""
    H, W = src
    boxes = [(0, 0, W - 1, H - 1), (0, 1, W - 2, H - 2), (1, 0, W - 2, H - 2), (1, 1, W - 1, H - 2), (1, 1, W - 2, H - 1)]
    boxes += [(c, r, c, r) for c in (0, W // 2, W - 1) for r in (0, H // 2, H - 1)]
    rng = np.random.default_rng(seed)
    for _ in range(40):
        c = np.sort(rng.integers(0, W, 2))
        r = np.sort(rng.integers(0, H, 2))
        boxes.append((int(c[0]), int(r[0]), int(c[1]), int(r[1])))
    return np.array(boxes, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------- inputs
def bytes_case(F, H, W, C, Ht, Wt):
    """uint8 (F, H, W, C): a stream that runs through all 256 values where the case is large enough, with planted windows —
    per frame, in turn, the first target window all 255, the last all 0, and a window whose mean is exactly k + 1/2 (half of
    its bytes 1, half 0, where its pixel count is even).  A plant may overwrite part of an earlier one where windows overlap;
    the tests count what the model sees."""
    j = np.arange(F * H * W * C, dtype=np.int64)
    a = ((j * 7 + 3 + j // 256) % 256).astype(np.uint8).reshape(F, H, W, C)
    rows, cols = windows(H, Ht), windows(W, Wt)
    cells = [(y, x) for y in range(Ht) for x in range(Wt)]
    for f in range(F):
        picks = {"ones": cells[0], "zeros": cells[-1], "tie": cells[len(cells) // 2]}
        if len(cells) < 3:
            picks = {("ones", "zeros", "tie")[f % 3]: cells[0]}
        for kind, (y, x) in picks.items():
            (r0, r1), (c0, c1) = rows[y], cols[x]
            block = a[f, r0:r1, c0:c1]
            if kind == "ones":
                block[...] = 255
            elif kind == "zeros":
                block[...] = 0
            else:
                n = (r1 - r0) * (c1 - c0)
                flat = np.zeros((n, C), np.uint8)
                flat[: n // 2] = 1
                block[...] = flat.reshape(r1 - r0, c1 - c0, C)
    return a


def floats_case(F, H, W, kind):
    """float32 (F, H, W): "quotients" b / 255 as torch divides them; "balanced" values in [-1, 1] with uneven magnitudes."""
    j = np.arange(F * H * W, dtype=np.int64)
    if kind == "quotients":
        b = torch.from_numpy(((j * 11 + 5 + j // 256) % 256).astype(np.uint8))
        return b.float().div(255.0).numpy().reshape(F, H, W)
    rng = np.random.default_rng(F * 1000 + H * 10 + W)
    v = rng.uniform(-1.0, 1.0, (F, H, W)) * rng.choice([1.0, 1e-3, 1e-6], (F, H, W))
    return v.astype(np.float32)
