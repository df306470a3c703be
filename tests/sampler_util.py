"""Host model of the samplers, written from definitions (include/pnr.h and the published Philox4x32-10), in numpy and
Python ints: the counter-based generator and its draw layout, the fp64 resampling with the interval of bins an fp32 cdf
may legitimately pick, and the accounting that takes a merged, sorted row apart again.

Generator (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11): a round maps the counter (c0..c3) to
(hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is bumped by (W0, W1) between rounds; ten rounds.

Draw layout: key = (seed lo32, seed hi32), counter = (ray lo32, ray hi32, draw id, block); draw ids coarse 0, u 1, r 2, g 3.
Uniform draw idx = word idx & 3 of block idx >> 2 as (x >> 8) * 2^-24; normal draw idx = block idx, a = 1 - u01(word 0),
b = u01(word 1), sqrt(-2 ln a) cos(fp32(2 pi) b).
"""
import bisect
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
DRAW_ID = {"noise_c": 0, "u": 1, "r": 2, "g": 3}
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
F32_TWO_PI = np.float32(6.28318530717958647692)


def philox4x32_10(key0, key1, c0, c1, c2, c3):
    """Vectorised over broadcastable integer arrays (values below 2^32); returns four uint64 arrays holding 32-bit words."""
    k0, k1, c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (key0, key1, c0, c1, c2, c3)])
    for rnd in range(10):
        p0 = np.uint64(M0) * c0          # both factors below 2^32: the product fits 64 bits
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c0, c1, c2, c3


def u01(x):
    """(x >> 8) * 2^-24: 24 bits, exact in fp32, in [0, 1)."""
    return ((np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def global_ray(base, n_rays, rays_per_obj=1, stride=0):
    """Global index of the call's local rays 0 .. n_rays - 1 (pnr_noise.ray_index_obj_stride)."""
    r = np.arange(n_rays, dtype=np.int64)
    if stride != 0:
        return np.int64(base) + r + (r // rays_per_obj) * np.int64(stride - rays_per_obj)
    return np.int64(base) + r


def counter_of(seed, ray, kind, idx):
    """(key0, key1, c0, c1, c2, c3, word) of draw `idx` of `kind` for one ray — the layout, as plain Python ints."""
    ray &= (1 << 64) - 1
    blk, word = (idx, 0) if kind == "g" else (idx >> 2, idx & 3)
    return (seed & 0xFFFFFFFF, seed >> 32, ray & 0xFFFFFFFF, ray >> 32, DRAW_ID[kind], blk, word)


def _blocks(seed, rays, kind, blk):
    rays = np.asarray(rays, dtype=np.int64).astype(np.uint64)[:, None]
    return philox4x32_10(int(seed) & 0xFFFFFFFF, int(seed) >> 32, rays & MASK, rays >> S32, DRAW_ID[kind],
                         np.asarray(blk, dtype=np.uint64)[None, :])


def normal_parts(seed, rays, n):
    """(a, arg, R) of the n normal draws of every ray: a and arg = fp32(fp32(2 pi) * b) as fp32, R = sqrt(-2 ln a) in fp64."""
    w = _blocks(seed, rays, "g", np.arange(n))
    a = np.float32(1.0) - u01(w[0])
    arg = F32_TWO_PI * u01(w[1])
    assert a.dtype == np.float32 and arg.dtype == np.float32
    return a, arg, np.sqrt(-2.0 * np.log(a.astype(np.float64)))


def draws(seed, rays, kind, n):
    """(N, n) draws of `kind` in noise_c, u, r (fp32, exact) or g (fp64) for the global ray indices `rays`."""
    if kind == "g":
        a, arg, R = normal_parts(seed, rays, n)
        return R * np.cos(arg.astype(np.float64))
    idx = np.arange(n)
    w = _blocks(seed, rays, kind, idx >> 2)
    out = np.where((idx & 3)[None] == 0, w[0], np.where((idx & 3)[None] == 1, w[1], np.where((idx & 3)[None] == 2, w[2], w[3])))
    return u01(out)


# ------------------------------------------------------------------------------------------- resampling in fp64
def margin_of(Kc):
    """Bound on |fp32 cdf - cdf64| in absolute terms (entries are at most 1, half an ulp there is 2^-25): every entry takes
    one rounding of w + 1e-5 and one of the division, the shared sum s its own summation error, a 6-level scan inside a
    64-entry segment, Kc / 64 carries across segments, and a cushion of about two: (16 + Kc / 32) * 2^-24."""
    return (16.0 + Kc / 32.0) * 2.0 ** -24


def cdf64(weights):
    w = np.asarray(weights, dtype=np.float32).astype(np.float64) + 1e-5
    c = np.cumsum(w / w.sum(-1, keepdims=True), -1)
    return np.concatenate([np.zeros_like(c[:, :1]), c], -1)


def fine_bins_fp64(weights, u, Kc, margin=None):
    """(lo, hi) per draw: the bins #(cdf64 <= u -+ margin) - 1, clamped at 0 below and NOT above (hi == Kc is legal)."""
    margin = margin_of(Kc) if margin is None else margin
    c = cdf64(weights)
    assert c.shape[1] == Kc + 1
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    lo, hi = np.empty(u.shape, np.int64), np.empty(u.shape, np.int64)
    for i in range(u.shape[0]):
        lo[i] = np.maximum(np.searchsorted(c[i], u[i] - margin, side="right") - 1, 0)
        hi[i] = np.maximum(np.searchsorted(c[i], u[i] + margin, side="right") - 1, 0)
    return lo, hi


def t_to_z(t, near, far, lindisp):
    near, far = np.float64(near), np.float64(far)
    if not lindisp:
        return near * (1.0 - t) + far * t
    return 1.0 / ((1.0 - t) / near + t / far)


def z_to_t(z, near, far, lindisp):
    near, far, z = np.float64(near), np.float64(far), np.asarray(z, dtype=np.float64)
    if not lindisp:
        return (z - near) / (far - near)
    return (1.0 / z - 1.0 / near) / (1.0 / far - 1.0 / near)


def z_of_bin(ind, r, Kc, near, far, lindisp):
    return t_to_z((np.asarray(ind, dtype=np.float64) + np.asarray(r, dtype=np.float32).astype(np.float64)) / Kc, near, far, lindisp)


def z_tolerance(near, far, lindisp):
    """8 * 2^-24 * max(|near|, |far|); with lindisp 8 * 2^-24 * far^2 / near (the error of y = 1 / z amplified by z^2)."""
    near, far = float(near), float(far)
    return 8 * 2.0 ** -24 * (far * far / near if lindisp else max(abs(near), abs(far)))


def depth_samples(depth, g, std, near, far):
    """clamp(fp32(depth + g * std), near, far) per ray, (B, n_dep) fp32."""
    z = (np.asarray(depth, np.float32).astype(np.float64)[:, None]
         + np.asarray(g, np.float32).astype(np.float64) * np.float64(np.float32(std))).astype(np.float32)
    return np.maximum(np.minimum(z, np.float32(far)), np.float32(near))


def tags(n_imp):
    """r[j] = (j + 0.5) / n_imp: the fractional part of t * Kc names the draw."""
    return ((np.arange(n_imp) + 0.5) / max(n_imp, 1)).astype(np.float32)


class Accounting(AssertionError):
    pass


def ulp32(x):
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def remove_coarse(z_sorted, zc):
    """One row: the row without its coarse values, each removed once by exact equality (the sort is a permutation)."""
    z_sorted = np.asarray(z_sorted, np.float32)
    if not (np.diff(z_sorted) >= 0).all():
        raise Accounting("row not ascending")
    rest = z_sorted.tolist()
    for v in np.sort(np.asarray(zc, np.float32))[::-1].tolist():
        i = bisect.bisect_left(rest, v)
        if i >= len(rest) or rest[i] != v:
            raise Accounting(f"coarse value {v!r} missing from the merged row")
        rest.pop(i)
    return np.asarray(rest, np.float32)


def split_depth(rest, zd_expected, ulps=1):
    """Takes the depth samples out of `rest` (ascending): each expected value claims its nearest remaining entry, which
    must lie within `ulps` fp32 ulps.  Returns the importance samples (ascending)."""
    rest = np.asarray(rest, np.float32).tolist()
    for v in np.sort(np.asarray(zd_expected, np.float32)).tolist():
        i = bisect.bisect_left(rest, v)
        cand = [k for k in (i - 1, i) if 0 <= k < len(rest)]
        if not cand:
            raise Accounting("no entry left for a depth sample")
        k = min(cand, key=lambda q: abs(rest[q] - v))
        if abs(rest[k] - v) > ulps * float(ulp32(v)):
            raise Accounting(f"depth sample {v!r}: nearest entry {rest[k]!r} is more than {ulps} ulp away")
        rest.pop(k)
    return np.asarray(rest, np.float32)


def attribute(z_sorted, zc, Kc, n_imp, near, far, lindisp, zd_expected=(), tagged=True):
    """Undoes the merge of one ray.  Returns (ind, z): bin and position of importance draw j, j = 0 .. n_imp - 1, found from
    the tags planted in r (tagged), or just the ascending importance positions (ind None)."""
    z_sorted = np.asarray(z_sorted, np.float32)
    if z_sorted.shape != (Kc + n_imp + len(zd_expected),):
        raise Accounting(f"row has {z_sorted.shape} entries")
    imp = split_depth(remove_coarse(z_sorted, zc), zd_expected)
    assert imp.shape == (n_imp,)
    if not tagged or n_imp == 0:
        return None, imp
    x = z_to_t(imp, near, far, lindisp) * Kc
    j = np.clip(np.rint((x - np.floor(x)) * n_imp - 0.5).astype(np.int64), 0, n_imp - 1)
    if len(np.unique(j)) != n_imp:
        raise Accounting(f"tags found {np.sort(j).tolist()}: not every draw exactly once")
    r = tags(n_imp).astype(np.float64)
    ind = np.rint(x - r[j]).astype(np.int64)
    out_i, out_z = np.empty(n_imp, np.int64), np.empty(n_imp, np.float32)
    out_i[j], out_z[j] = ind, imp
    return out_i, out_z


def some_assignment(imp, lo, hi, r, Kc, near, far, lindisp, tol):
    """True if the ascending importance positions `imp` are within tol of z_of_bin(i_j, r_j) for SOME choice lo_j <= i_j <=
    hi_j: a perfect matching draws <-> entries (augmenting paths)."""
    n = len(imp)
    adj = []
    for j in range(n):
        cand = z_of_bin(np.arange(lo[j], hi[j] + 1), r[j], Kc, near, far, lindisp)
        adj.append(np.nonzero((np.abs(imp.astype(np.float64)[:, None] - cand[None]) <= tol).any(1))[0].tolist())
    owner = [-1] * n

    def grow(j, seen):
        for e in adj[j]:
            if e not in seen:
                seen.add(e)
                if owner[e] < 0 or grow(owner[e], seen):
                    owner[e] = j
                    return True
        return False

    return all(grow(j, set()) for j in range(n))


# ------------------------------------------------------------------------------------------- the edge families
BOUNDS = [(1.25, 2.75), (0.8, 1.8)]
SHAPES = [(1, 1, 0), (63, 64, 0), (64, 64, 0), (64, 65, 0), (65, 40, 23), (128, 64, 32), (129, 200, 0), (300, 112, 100),
          (2048, 1, 0), (4000, 64, 32)]
FAMILIES = ["random", "zero", "one@0", "one@63", "one@64", "one@last", "ends", "tiny", "opaque"]


def n_rays_of(Kc):
    return 5 if Kc >= 2048 else 24


@functools.lru_cache(maxsize=None)
def make_case(Kc, n_imp, n_dep, near, far, lindisp, seed=0):
    """Inputs of one resampling case: rays, coarse positions, weights by family (ray i -> FAMILIES[i % 9]), u planted per
    ray (0, 1 - 2^-24, fp32(cdf64[k]) and both neighbours at several k incl. the ends of a flat run; the rest random),
    random u of a second run, tags and random r, g, and depths on both sides of the bounds with std 0 and 0.3."""
    import torch
    from oracle import pixelnerf_oracle as orc
    B = n_rays_of(Kc)
    rng = np.random.default_rng([Kc, n_imp, n_dep, int(round(near * 100)), int(lindisp), seed])
    near32, far32 = np.float32(near), np.float32(far)
    rays = np.zeros((B, 8), np.float32)
    rays[:, 5], rays[:, 6], rays[:, 7] = 1.0, near32, far32
    zc = orc.sample_coarse(torch.from_numpy(rays), Kc, lindisp, torch.from_numpy(rng.random((B, Kc), dtype=np.float32))).numpy()
    fam = [FAMILIES[i % len(FAMILIES)] for i in range(B)]
    w = np.zeros((B, Kc), np.float32)
    for i, f in enumerate(fam):
        if f == "random":
            w[i] = rng.random(Kc, dtype=np.float32) * (rng.random(Kc) < 0.7)
            w[i] /= max(w[i].sum(), 1e-3) * 1.1
        elif f.startswith("one@"):
            p = Kc - 1 if f == "one@last" else int(f[4:])
            w[i, min(p, Kc - 1)] = 1.0
        elif f == "ends":
            w[i, 0] = w[i, -1] = 0.5
        elif f == "tiny":
            w[i] = 1e-9
        elif f == "opaque":       # a real profile: a dense slab behind empty space, composited by the oracle
            sig = np.where((np.arange(Kc) >= Kc // 3) & (np.arange(Kc) < Kc // 3 + max(Kc // 8, 1)), 40.0 * Kc, 0.0)
            out = torch.from_numpy(np.concatenate([np.full((1, Kc, 3), 0.5), sig[None, :, None]], -1).astype(np.float32))
            w[i] = orc.composite(torch.from_numpy(rays[i:i + 1]), torch.from_numpy(zc[i:i + 1]), out, False)[0][0].numpy()
    c64 = cdf64(w)
    u_rand = rng.random((B, n_imp), dtype=np.float32)
    u = u_rand.copy()
    for i in range(B):
        # entries of the cdf to sit on: first, second, a segment boundary of the scan, the ends of the flat run in front
        # of the one-hot bin / of the last bin, and (Kc > 1) the last entry itself: from there upwards ind == Kc
        # (with Kc == 1 the top bin's t = 1 + r reaches 2, where the lindisp 1 / z crosses zero: no bound on z holds there)
        ks = [k for k in (0, 1, min(64, Kc), min(65, Kc), Kc // 2, Kc - 1, Kc) if k < Kc or Kc > 1]
        plant = [np.float32(0.0), np.float32(1.0 - 2.0 ** -24)]
        for k in ks:
            v = np.float32(c64[i, k])
            plant += [v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2))]
        plant = [p for p in plant if p >= 0]
        order = rng.permutation(len(plant))[:n_imp]
        u[i, :len(order)] = np.asarray(plant, np.float32)[order]
    depth = np.resize(np.array([near - 0.5, near + 0.3, 0.5 * (near + far), far - 1e-3, far + 0.4, near], np.float32), B)
    std = 0.3
    g = rng.standard_normal((B, n_dep)).astype(np.float32)
    return dict(B=B, Kc=Kc, n_imp=n_imp, n_dep=n_dep, near=near32, far=far32, lindisp=lindisp, rays=rays, zc=zc, w=w,
                fam=fam, u=u, u_rand=u_rand, r_tag=np.tile(tags(n_imp), (B, 1)), r_rand=rng.random((B, n_imp), dtype=np.float32),
                g=g, depth=depth, stds=(0.0, std))


def check_rows(case, z_got, u, r, std, tagged):
    """The asserts of the resampling test on a (B, Kt) result; returns (draws, draws with lo < hi, rays, rays with every
    draw lo == hi, worst |dz| / tol), per family 'random' and overall, for the docstrings."""
    Kc, n_imp, n_dep = case["Kc"], case["n_imp"], case["n_dep"]
    near, far, lindisp = case["near"], case["far"], case["lindisp"]
    tol = z_tolerance(near, far, lindisp)
    lo, hi = fine_bins_fp64(case["w"], u, Kc)
    zd = depth_samples(case["depth"], case["g"], std, near, far)
    stats = dict(draws=0, ambiguous=0, rays=0, clean_rays=0, worst=0.0, rand_draws=0, rand_ambiguous=0, rand_rays=0,
                 rand_clean=0, top_bin=0)
    z_got = np.asarray(z_got, np.float32)
    assert z_got.shape == (case["B"], Kc + n_imp + n_dep)
    for i in range(case["B"]):
        what = (case["fam"][i], i, Kc, n_imp, n_dep, float(near), float(far), lindisp, std)
        ind, imp = attribute(z_got[i], case["zc"][i], Kc, n_imp, near, far, lindisp, zd[i], tagged)
        amb = int((lo[i] < hi[i]).sum())
        rnd = case["fam"][i] == "random"
        stats["draws"] += n_imp; stats["ambiguous"] += amb; stats["rays"] += 1; stats["clean_rays"] += amb == 0
        if rnd:
            stats["rand_draws"] += n_imp; stats["rand_ambiguous"] += amb; stats["rand_rays"] += 1; stats["rand_clean"] += amb == 0
        if n_imp == 0:
            continue
        if tagged:
            assert ((lo[i] <= ind) & (ind <= hi[i])).all(), (what, "bin outside [lo, hi]", ind.tolist(), lo[i].tolist(), hi[i].tolist())
            err = np.abs(imp.astype(np.float64) - z_of_bin(ind, r[i], Kc, near, far, lindisp)).max()
            stats["top_bin"] += int((ind == Kc).sum())
        elif amb == 0:
            want = np.sort(z_of_bin(lo[i], r[i], Kc, near, far, lindisp))
            err = np.abs(imp.astype(np.float64) - want).max()
        else:
            assert some_assignment(imp, lo[i], hi[i], r[i], Kc, near, far, lindisp, tol), (what, "no assignment within [lo, hi]")
            err = 0.0
        stats["worst"] = max(stats["worst"], err / tol)
        assert err <= tol, (what, "z error / tol", err / tol)
    return stats
