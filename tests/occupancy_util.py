"""numpy models of pnr_occ_build, pnr_ray_bounds and pnr_frame_from_hits, written from include/pnr.h ("empty-space culling")
alone, an independent fp64 brute force for the traversal, and the grids and rays the CPU and GPU tests share.  The models
take `mistake=`: a planted error that the tests' checks must reject."""
import numpy as np

F32 = np.float32
BRUTE_SAMPLES = 8192
EXCLUDE = 1e-4                       # of a cell edge: a brute-force sample this close to a face of its cell is not counted


# ------------------------------------------------------------------------------------------------------------ the bit grid
def pack_cells(cells, mistake=None):
    """(cx, cy, cz) bool -> uint32 words, cell (i, j, k) = bit k & 31 of word (i cy + j) wz + (k >> 5)."""
    cx, cy, cz = cells.shape
    wz = (cz + 31) // 32
    words = np.zeros((cx, cy, wz), dtype=np.uint32)
    for k in range(cz):
        bit = 31 - (k & 31) if mistake == "bit_reversed" else k & 31
        words[:, :, k >> 5] |= cells[:, :, k].astype(np.uint32) << np.uint32(bit)
    return words.reshape(-1)


def unpack_words(words, cell_counts):
    cx, cy, cz = cell_counts
    wz = (cz + 31) // 32
    w = np.asarray(words).astype(np.uint32).reshape(cx, cy, wz)
    out = np.zeros((cx, cy, cz), dtype=bool)
    for k in range(cz):
        out[:, :, k] = (w[:, :, k >> 5] >> np.uint32(k & 31)) & np.uint32(1)
    return out


def hot_samples(sigma, thresh):
    with np.errstate(invalid="ignore"):
        return ~(sigma.astype(np.float64) < thresh)


def raw_cells(sigma, thresh):
    hot = hot_samples(sigma, thresh)
    nx, ny, nz = hot.shape
    raw = np.zeros((nx - 1, ny - 1, nz - 1), dtype=bool)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                raw |= hot[a:nx - 1 + a, b:ny - 1 + b, c:nz - 1 + c]
    return raw


def dilate_cells(raw, dilate, mistake=None):
    """Occupied iff a raw-occupied cell lies within `dilate` cells (Chebyshev): one axis after the other, a running OR of the
    shifted array."""
    occ = raw.copy()
    for axis in range(3):
        if mistake == "dilate_skips_axis" and axis == 2:
            continue
        src = occ.copy()
        n = src.shape[axis]
        for s in range(1, dilate + 1):
            if s >= n:
                break
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - s), slice(s, n)
            occ[tuple(hi)] |= src[tuple(lo)]
            occ[tuple(lo)] |= src[tuple(hi)]
    return occ


def build_model(sigma, thresh, dilate, prev=None, mistake=None):
    """pnr_occ_build -> uint32 words; prev: the words to accumulate into."""
    words = pack_cells(dilate_cells(raw_cells(sigma, thresh), dilate, mistake), mistake)
    return words if prev is None else words | np.asarray(prev).astype(np.uint32)


def build_brute(sigma, thresh, dilate):
    """The definition cell by cell: a shifted maximum over every offset of the (2 dilate + 1)^3 neighbourhood."""
    raw = raw_cells(sigma, thresh)
    cx, cy, cz = raw.shape
    d = dilate
    padded = np.zeros((cx + 2 * d, cy + 2 * d, cz + 2 * d), dtype=bool)
    padded[d:d + cx, d:d + cy, d:d + cz] = raw
    occ = np.zeros_like(raw)
    for a in range(2 * d + 1):
        for b in range(2 * d + 1):
            for c in range(2 * d + 1):
                occ = np.maximum(occ, padded[a:a + cx, b:b + cy, c:c + cz])
    return occ


# ------------------------------------------------------------------------------------------------------------ the traversal
def min_s(a, b):
    return np.where(b < a, b, a)


def max_s(a, b):
    return np.where(b > a, b, a)


def grid_consts(c1, c2, cell_counts):
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    n = np.asarray(cell_counts, np.float64)
    return c1.astype(F32), c2.astype(F32), ((c2 - c1) / n).astype(F32), (n / (c2 - c1)).astype(F32)


def trace_model(rays, c1, c2, cells, pad, mistake=None):
    """pnr_ray_bounds' steps 1-5 for rays (n, 8) float32 and cells (cx, cy, cz) bool -> (hit (n) bool, near' (n), far' (n)
    float32; unspecified where hit is False)."""
    rays = np.ascontiguousarray(rays, dtype=F32)
    n = rays.shape[0]
    cnt = np.asarray(cells.shape, dtype=np.int64)
    lo, hi, h, inv_h = grid_consts(c1, c2, cnt)
    pad32 = F32(pad)
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    with np.errstate(all="ignore"):
        alive = np.isfinite(rays).all(axis=1) & ~(d == 0).all(axis=1) & ~(near > far)
        t0, t1 = near.copy(), far.copy()
        for a in range(3):
            zero = d[:, a] == 0
            alive &= ~(zero & ((o[:, a] < lo[a]) | (o[:, a] > hi[a])))
            ta, tb = (lo[a] - o[:, a]) / d[:, a], (hi[a] - o[:, a]) / d[:, a]
            t0 = np.where(zero, t0, max_s(t0, min_s(ta, tb)))
            t1 = np.where(zero, t1, min_s(t1, max_s(ta, tb)))
        alive &= ~(t0 > t1)
        # rays that are out keep harmless values so that the arithmetic below stays defined
        t0 = np.where(alive, t0, F32(0)).astype(F32)
        t1 = np.where(alive, t1, F32(0)).astype(F32)
        c = np.zeros((n, 3), dtype=np.int64)
        step = np.zeros((n, 3), dtype=np.int64)
        tmax = np.full((n, 3), np.inf, dtype=F32)

        def boundary_t(a, rows):
            b = c[rows, a] + (step[rows, a] > 0)
            B = np.where(b == cnt[a], hi[a], lo[a] + b.astype(F32) * h[a]).astype(F32)
            return ((B - o[rows, a]) / d[rows, a]).astype(F32)

        for a in range(3):
            p = o[:, a] + t0 * d[:, a]
            f = np.floor((p - lo[a]) * inv_h[a])
            f = min_s(F32(cnt[a] - 1), max_s(F32(0), f))
            c[:, a] = np.where(alive, f, 0).astype(np.int64)
            step[:, a] = np.where(d[:, a] > 0, 1, np.where(d[:, a] < 0, -1, 0))
            if mistake == "negative_as_positive":
                step[:, a] = np.where(d[:, a] != 0, 1, 0)
            rows = np.nonzero(alive & (step[:, a] != 0))[0]
            tmax[rows, a] = boundary_t(a, rows)
        hit = np.zeros(n, dtype=bool)
        t_in, t_out, t_cur = np.zeros(n, F32), np.zeros(n, F32), t0.copy()
        walking = alive.copy()
        for _ in range(int(cnt.sum()) + 3):
            if not walking.any():
                break
            tm = min_s(min_s(tmax[:, 0], tmax[:, 1]), tmax[:, 2])
            te = max_s(min_s(tm, t1), t_cur)
            stop = ~(tm < t1)
            occ = walking & cells[c[:, 0], c[:, 1], c[:, 2]]
            if mistake == "last_cell_dropped":
                occ &= ~stop
            first = occ & ~hit
            t_in = np.where(first, t_cur, t_in)
            hit |= occ
            t_out = np.where(occ, te, t_out)
            walking &= ~stop
            axis = np.where((tmax[:, 0] <= tmax[:, 1]) & (tmax[:, 0] <= tmax[:, 2]), 0, np.where(tmax[:, 1] <= tmax[:, 2], 1, 2))
            for a in range(3):
                rows = np.nonzero(walking & (axis == a))[0]
                c[rows, a] += step[rows, a]
                left = (step[rows, a] == 0) | (c[rows, a] < 0) | (c[rows, a] >= cnt[a])
                walking[rows[left]] = False
                c[rows[left], a] = 0
                rows = rows[~left]
                tmax[rows, a] = boundary_t(a, rows)
            t_cur = np.where(walking, te, t_cur)
        near2 = max_s(near, (t_in - pad32).astype(F32)).astype(F32)
        far2 = min_s(far, (t_out + pad32).astype(F32)).astype(F32)
        if mistake == "pad_one_end":
            far2 = min_s(far, t_out).astype(F32)
    return hit, near2, far2


def bounds_model(rays, rays_per_frame, c1, c2, cells, pad, mistake=None):
    """pnr_ray_bounds -> (rows: list over frames of the (count_f, 8) compact rows, slot (n) int32, counts (F) int64), by the
    sequential walk the header names."""
    rays = np.ascontiguousarray(rays, dtype=F32)
    n, R = rays.shape[0], int(rays_per_frame)
    hit, near2, far2 = trace_model(rays, c1, c2, cells, pad, mistake)
    slot = np.full(n, -1, dtype=np.int32)
    counts = np.zeros(n // R, dtype=np.int64)
    rows = []
    for f in range(n // R):
        mine = []
        for i in range(f * R, (f + 1) * R):
            if hit[i]:
                slot[i] = len(mine)
                row = rays[i].copy()
                row[6], row[7] = near2[i], far2[i]
                mine.append(row)
        counts[f] = len(mine)
        rows.append(np.stack(mine) if mine else np.zeros((0, 8), F32))
    return rows, slot, counts


def frame_model(rec, slot, rays_per_frame, bg):
    """pnr_frame_from_hits: rec (n, >= 4) -> (n, 4)."""
    n, R = slot.shape[0], int(rays_per_frame)
    out = np.empty((n, 4), dtype=F32)
    for i in range(n):
        s = int(slot[i])
        out[i] = (bg, bg, bg, 0.0) if s < 0 else rec[(i // R) * R + s, :4]
    return out


def brute_force(rays, c1, c2, cells):
    """Independent of the stepping: BRUTE_SAMPLES values of t per ray in fp64 -> per ray (t of the counted samples, number of
    in-cell samples).  In-cell: the point lies in an occupied cell; counted: also at least EXCLUDE of a cell edge away from
    every face of that cell."""
    r = np.asarray(rays, dtype=np.float64)
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    cnt = np.asarray(cells.shape)
    frac_t = (np.arange(BRUTE_SAMPLES) + 0.5) / BRUTE_SAMPLES
    out = []
    for ray in r:
        if not np.isfinite(ray).all() or ray[6] > ray[7] or not ray[3:6].any():        # the misses by convention
            out.append((np.zeros(0), 0))
            continue
        t = ray[6] + (ray[7] - ray[6]) * frac_t
        u = (ray[None, 0:3] + t[:, None] * ray[None, 3:6] - c1) / (c2 - c1) * cnt
        idx = np.floor(u)
        inside = ((idx >= 0) & (idx < cnt)).all(axis=1)
        ii = np.clip(idx, 0, cnt - 1).astype(np.int64)
        in_cell = inside & cells[ii[:, 0], ii[:, 1], ii[:, 2]]
        fr = u - idx
        counted = in_cell & ((fr >= EXCLUDE) & (fr <= 1.0 - EXCLUDE)).all(axis=1)
        out.append((t[counted], int(in_cell.sum())))
    return out


def distance_to_occupied(points, c1, c2, cells):
    """Chebyshev distance, in cell edges, from each point (m, 3) to the nearest occupied cell (a closed box); inf for an empty
    grid."""
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    u = (np.asarray(points, np.float64) - c1) / (c2 - c1) * np.asarray(cells.shape)
    occ = np.argwhere(cells)
    if len(occ) == 0:
        return np.full(len(u), np.inf)
    best = np.full(len(u), np.inf)
    for k in range(0, len(occ), 4096):
        part = occ[k:k + 4096][None]                                   # (1, m, 3)
        dist = np.maximum(np.maximum(part - u[:, None], u[:, None] - (part + 1)), 0.0).max(axis=2)
        best = np.minimum(best, dist.min(axis=1))
    return best


# ------------------------------------------------------------------------------------------------------------ shared cases
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def case_grids():
    """name -> (cx, cy, cz) bool.  Odd sizes, more than one word along z."""
    shape = (9, 11, 35)
    i, j, k = np.meshgrid(*(np.arange(s) + 0.5 for s in shape), indexing="ij")
    r = np.sqrt(((i / shape[0] - 0.5) ** 2 + (j / shape[1] - 0.5) ** 2 + (k / shape[2] - 0.5) ** 2))
    single = np.zeros(shape, dtype=bool)
    single[4, 6, 33] = True
    return {"shell": (r > 0.28) & (r < 0.4), "single": single, "full": np.ones(shape, dtype=bool), "empty": np.zeros(shape, dtype=bool)}


def case_rays(seed=0, n_random=96):
    """Rays (n, 8) float32 around BOX: random ones from outside and inside, directions with one and two zero components,
    grazes of a face and an edge, starts inside cells, near / far cutting through the box, and the misses the header names."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n_random):                                         # from outside, aimed at a point inside
        o = rng.normal(size=3)
        o = o / np.linalg.norm(o) * rng.uniform(2.0, 3.0)
        d = rng.uniform(-0.8, 0.8, 3) - o
        d /= np.linalg.norm(d)
        rows.append([*o, *d, 0.5, 4.5])
    for _ in range(n_random // 2):                                    # from inside the box, near / far cutting through cells
        o = rng.uniform(-0.9, 0.9, 3)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        rows.append([*o, *d, rng.uniform(0.0, 0.3), rng.uniform(0.4, 1.2)])
    for a in range(3):                                                # one and two zero components, both signs
        for sgn in (1.0, -1.0):
            d = np.zeros(3); d[a] = sgn
            o = rng.uniform(-0.7, 0.7, 3); o[a] = -2.0 * sgn
            rows.append([*o, *d, 0.25, 3.5])
            d2 = np.full(3, sgn * 0.6); d2[a] = 0.0
            o2 = rng.uniform(-0.5, 0.5, 3) - 2.0 * d2
            rows.append([*o2, *d2, 0.0, 4.0])
    eps = 1e-3 * 2.0 / 9.0
    rows.append([-2.0, 1.0, 0.1, 1.0, 0.0, 0.0, 0.0, 4.0])            # in the plane of the face y = hi
    rows.append([-2.0, 1.0 - eps, 0.1, 1.0, 0.0, 0.0, 0.0, 4.0])      # just inside it
    rows.append([-2.0, 1.0 + eps, 0.1, 1.0, 0.0, 0.0, 0.0, 4.0])      # just outside: a miss
    s = np.sqrt(0.5)
    rows.append([0.0, 2.0, 0.3, s, -s, 0.0, 0.0, 4.0])                # through the edge x = hi, y = hi: touches the box in a point
    rows.append([-0.5, 2.5, 0.3, s, -s, 0.0, 0.0, 4.0])               # the same direction, through the box
    rows.append([0.1, 0.2, 0.3, 0.0, 0.0, 0.0, 0.0, 4.0])             # no direction
    rows.append([0.1, 0.2, 0.3, 0.0, 0.0, 1.0, 2.0, 1.0])             # near > far
    rows.append([np.nan, 0.2, 0.3, 0.0, 0.0, 1.0, 0.0, 4.0])
    rows.append([0.1, 0.2, 0.3, 0.0, np.inf, 1.0, 0.0, 4.0])
    rows.append([0.1, 0.2, -3.0, 0.0, 0.0, 1.0, 0.0, 1.5])            # far in front of the box
    return np.asarray(rows, dtype=F32)
