"""The colour-jitter augmentation without a GPU: the host model of include/pnr.h's section (tests/color_jitter_util.py) — the
distribution of its draws, that the pixel set the GPU cases run on reaches every branch of the chain, that it tells the model
from a list of planted mistakes — and the argument checks of every new entry point and wrapper.

Statistical bounds (5 sigma, 4096 objects): a factor is uniform over a width w = 2 range, so its sample mean has standard
deviation w / sqrt(12 n) and its sample variance sqrt(w^4 / (180 n)) (the uniform law's fourth central moment is w^4 / 80); an
order's count has sqrt(n p (1 - p)) with p = 1 / 24."""
import ctypes
import math

import numpy as np
import pytest
import torch

import color_jitter_util as cj
from sampler_util import philox4x32_10

F = np.float32
RANGES = (0.15, 0.15, 0.15, 0.15)
N_OBJ = 4096


# ------------------------------------------------------------------------------------------------------------ draws
def test_counter_layout_and_order_code():
    seed = (0x89ABCDEF << 32) | 0x01234567
    assert cj.jitter_counter(seed, 5, 1) == (0x01234567, 0x89ABCDEF, 5, 0, 10, 1)
    assert cj.jitter_counter(seed, (1 << 32) + 6, 0) == (0x01234567, 0x89ABCDEF, 6, 1, 10, 0)
    assert cj.order_of(0) == [0, 1, 2, 3] and cj.order_of(23) == [3, 2, 1, 0]
    assert cj.order_of(7) == [1, 0, 3, 2]                   # 7 = 1 * 6 + 0 * 2 + 1: contrast, brightness, hue, saturation
    assert sorted(tuple(cj.order_of(q)) for q in range(24)) == sorted({tuple(cj.order_of(q)) for q in range(24)})
    assert all(cj.code_of(cj.order_of(q)) == q for q in range(24))
    # one record taken one counter at a time
    rec = cj.draw_records(seed, 3, RANGES)[2]
    a = [int(w) for w in philox4x32_10(*cj.jitter_counter(seed, 2, 0))]
    b = [int(w) for w in philox4x32_10(*cj.jitter_counter(seed, 2, 1))]
    for k in range(4):
        u = F((a[k] >> 8) * 2.0 ** -24)
        lo, hi = (F(-0.15), F(0.15)) if k == 3 else (F(F(1) - F(0.15)), F(F(1) + F(0.15)))
        assert rec[k] == F(lo + F(F(hi - lo) * u))
    assert rec[5] == (b[0] * 24) >> 32 and rec[4] == 0 and rec[6] == 0 and rec[7] == 0


@pytest.mark.parametrize("seed", [20241020, (77 << 40) + 3])
def test_draws_follow_the_uniform_law(seed):
    rec = cj.draw_records(seed, N_OBJ, RANGES)
    for k, name in enumerate(("brightness", "contrast", "saturation", "hue")):
        w, centre = 2.0 * RANGES[k], (0.0 if k == 3 else 1.0)
        f = rec[:, k].astype(np.float64)
        assert (np.abs(f - centre) <= RANGES[k] + 1e-7).all()
        d_mean = abs(f.mean() - centre) / (w / math.sqrt(12.0 * N_OBJ))
        d_var = abs(f.var() - w * w / 12.0) / math.sqrt(w ** 4 / (180.0 * N_OBJ))
        print(f"{name}: mean off by {d_mean:.2f} sigma, variance by {d_var:.2f} sigma")
        assert d_mean <= 5.0 and d_var <= 5.0, (name, d_mean, d_var)
    counts = np.bincount(rec[:, 5].astype(np.int64), minlength=24)
    p = 1.0 / 24.0
    dev = np.abs(counts - N_OBJ * p).max() / math.sqrt(N_OBJ * p * (1.0 - p))
    print(f"orders: worst deviation {dev:.2f} sigma")
    assert len(counts) == 24 and (counts > 0).all() and dev <= 5.0


def test_a_record_depends_on_seed_and_object_only():
    a = cj.draw_records(11, 8, RANGES)
    assert np.array_equal(a[:3], cj.draw_records(11, 3, RANGES))
    assert not np.array_equal(a, cj.draw_records(12, 8, RANGES))
    assert len({tuple(r) for r in a}) == 8
    zero = cj.draw_records(11, 4, (0.0, 0.0, 0.0, 0.0))
    assert (zero[:, :3] == 1).all() and (zero[:, 3] == 0).all() and not np.signbit(zero[:, 3]).any()


# ------------------------------------------------------------------------------------------------------------ the chain
def test_identity_record_leaves_the_bits_alone():
    px = cj.pixel_set()
    rec = cj.written_records()[-1]
    assert np.array_equal(cj.chain(cj.unit(px), rec).view(np.uint32), cj.unit(px).view(np.uint32))
    for balanced in (0, 1):
        want = (F(0.5) * cj.balance(cj.unit(px), balanced) + F(0.5)).astype(F)
        assert np.array_equal(cj.model_rgb_gt(px, rec, balanced).view(np.uint32), want.view(np.uint32))


def test_hue_pair_agrees_with_colorsys():
    """The RGB -> HSV -> RGB pair of the header against Python's colorsys in fp64, a hue shift of 0.15 in between.  Bound: H is
    rounded where it lies in [1, 2) (H / 6 + 1: half an ulp there is 2^-24), again by the shift (2^-25) and carries about 2^-26
    from the three quotients; f = 6 H' - i multiplies that by 6, and p, q, t add three roundings of values below 1 (2^-25
    each): 6 (2^-24 + 2^-25 + 2^-26) + 3 * 2^-25 < 16 * 2^-24."""
    import colorsys
    px = cj.pixel_set()
    x = cj.unit(px)
    got = cj.hue_op(x, 0.15)
    worst = 0.0
    for row, out in zip(x.astype(np.float64), got):
        h, s, v = colorsys.rgb_to_hsv(*row)
        want = colorsys.hsv_to_rgb((h + float(F(0.15))) % 1.0, s, v)
        worst = max(worst, float(np.abs(np.array(want) - out).max()))
    print(f"hue pair vs colorsys: max |d| = {worst:.3e}")
    assert worst <= 16 * 2.0 ** -24


def test_the_pixel_set_reaches_every_branch():
    """Factors 1.15 / 1.15 / 1.15 and hue -+0.15 over all 24 orders: every hue sector, all three maxc branches, the grey case,
    the low clamp of contrast and saturation, the high clamp of brightness, contrast and saturation."""
    px = cj.pixel_set()
    assert px.shape == (97, 3) and px[:8].tolist() == [[a, b, c] for a in (0, 255) for b in (0, 255) for c in (0, 255)]
    assert px[8:14].tolist() == [[200, 200, 10], [10, 200, 200], [200, 10, 200], [7, 7, 7], [128, 128, 128], [254, 255, 255]]
    for order_free in (True, False):
        counts = {}
        for q in (range(24) if order_free else (0,)):
            for h in (0.15, -0.15):
                rec = cj.with_mean(np.array([1.15, 1.15, 1.15, h, 0, q, 0, 0], F), px[None, None])
                cj.chain(cj.unit(px), rec, counts=counts)
        print({k: counts[k] for k in sorted(counts)})
        for k in [f"sector{i}" for i in range(6)] + ["max_r", "max_g", "max_b", "eq", "contrast_low", "saturation_low",
                                                      "brightness_high", "contrast_high", "saturation_high"]:
            assert counts.get(k, 0) > 0, (k, order_free)


def _object():
    """Two views of 1 x 97 pixels: the pixel set, and the pixel set darkened — so a per-view mean is not the object's."""
    px = cj.pixel_set()
    return np.stack([px[None], (px // 3)[None]])            # (2, 1, 97, 3)


@pytest.mark.parametrize("variant", cj.VARIANTS[:-1])
def test_the_pixel_set_separates_planted_variants(variant):
    obj = _object()
    px = obj[0, 0]
    differs = 0
    for rec in cj.written_records(identity=False):
        rec = cj.with_mean(rec, obj)
        good = cj.model_rgb_gt(px, rec, 1)
        bad = cj.model_rgb_gt(px, rec, 1, variant=variant)
        differs += int(not np.array_equal(good.view(np.uint32), bad.view(np.uint32)))
    print(f"{variant}: differs under {differs} of 24 records")
    assert differs > 0


def test_the_pixel_set_separates_a_per_view_mean():
    obj = _object()
    px = obj[0, 0]
    differs = 0
    for rec in cj.written_records(identity=False):
        good, bad = cj.with_mean(rec, obj), cj.with_mean(rec, obj, per_view=0)
        assert good[4] != bad[4]
        differs += int(not np.array_equal(cj.model_rgb_gt(px, good, 1).view(np.uint32), cj.model_rgb_gt(px, bad, 1).view(np.uint32)))
    assert differs > 0


def test_the_hue_fix_up_on_an_input_that_reaches_it():
    """Pure red has H = 0; a hue shift of -1e-9 gives t = -1e-9 and t - floor(t) = 1.0f, the case the fix-up is for.  A chain
    without the fix-up looks up sector 6, which matches no row.  With the header's `i mod 6` behind it the fix-up is not
    observable — 6 H' = 6 gives i = 0, f = 0, exactly the bits of H' = 0 — which the last assertion records."""
    px = np.array([[255, 0, 0], [255, 0, 0]], np.uint8)
    rec = np.array([1, 1, 1, -1e-9, 0, 0, 0, 0], F)
    counts = {}
    good = cj.model_rgb_gt(px, rec, 0, counts=counts)
    assert counts["fixup"] == 2
    assert np.array_equal(good, np.array([[1.0, 0.5, 0.5]] * 2, F))
    assert not np.array_equal(good, cj.model_rgb_gt(px, rec, 0, variant="no_fixup"))
    assert np.array_equal(good.view(np.uint32), cj.model_rgb_gt(px, rec, 0, variant="no_fixup_mod").view(np.uint32))


def test_the_mean_is_taken_in_front_of_contrast_only():
    obj = _object()
    base = np.array([1.15, 0.85, 1.15, 0.15, 0, 0, 0, 0], F)
    means = {}
    for pos in range(4):                                    # contrast at each position of the order
        order = [o for o in (cj.BRIGHTNESS, cj.SATURATION, cj.HUE)]
        order.insert(pos, cj.CONTRAST)
        rec = base.copy()
        rec[5] = cj.code_of(order)
        means[pos] = cj.mean64(obj, rec)
    plain = float(cj.gray(cj.unit(obj.reshape(-1, 3))).astype(np.float64).mean())
    assert means[0] == plain and len(set(means.values())) == 4
    rec = base.copy(); rec[1] = 1.0
    assert cj.with_mean(rec, obj)[4] == 0


# ------------------------------------------------------------------------------------------------------------ arguments
E_NULL, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -4, -5


def _ranges(*v):
    return (ctypes.c_float * 4)(*v)


def test_plan_refusals_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    assert N.PNR_JITTER_BLOCK == 4096
    wb = N.lib.pnr_color_jitter_workspace_bytes
    assert wb(1, 1, 1, 1) == 8 and wb(3, 1, 4097, 1) == 48 and wb(2, 3, 64, 64) == 2 * 3 * 8
    assert wb(0, 1, 1, 1) == 0 and wb(1, 0, 1, 1) == 0 and wb(1, 2, 32768, 32768) == 0
    p = 64

    def plan(images=p, SB=2, NV=3, W=8, H=6, C=3, ranges=_ranges(*RANGES), rec=p, ws=p, ws_bytes=1 << 20):
        return N.lib.pnr_color_jitter_plan(images, SB, NV, W, H, C, ranges, 7, rec, ws, ws_bytes, None)

    assert plan(ranges=None) == E_NULL and plan(rec=None) == E_NULL and plan(images=None) == E_NULL and plan(ws=None) == E_NULL
    for bad in ((-0.1, 0, 0, 0), (1.5, 0, 0, 0), (0, 1.01, 0, 0), (0, 0, -1, 0), (0, 0, 2, 0), (0, 0, 0, 0.51), (0, 0, 0, -0.1),
                (float("nan"), 0, 0, 0), (0, 0, 0, float("nan"))):
        assert plan(ranges=_ranges(*bad)) == E_SHAPE, bad
    assert plan(C=2) == E_SHAPE and plan(C=5) == E_SHAPE and plan(C=0) == E_SHAPE
    assert plan(SB=0) == E_SHAPE and plan(NV=0) == E_SHAPE and plan(W=0) == E_SHAPE and plan(H=-1) == E_SHAPE
    assert plan(NV=2, W=32768, H=32768) == E_SHAPE
    assert plan(ws=p + 4) == E_ALIGN
    assert plan(ws_bytes=2 * 8 - 1) == E_WORKSPACE and plan(ws_bytes=0) == E_WORKSPACE
    assert plan(ranges=_ranges(1.0, 1.0, 1.0, 0.5), ws_bytes=0) == E_WORKSPACE       # the largest ranges are accepted


def test_gather_refusals_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    p = 64

    def tb(images=p, poses=p, focal=p, SB=1, NV=2, W=4, H=4, pix=p, B=8, rays=p, rgb=p, C=3, balanced=1, jitter=p):
        return N.lib.pnr_train_batch_u8_jitter(images, poses, focal, None, SB, NV, W, H, 0.1, 1.0, pix, B, rays, rgb, C, balanced,
                                               jitter, None)

    assert tb(jitter=None) == E_NULL and tb(poses=None) == E_NULL and tb(focal=None) == E_NULL and tb(pix=None) == E_NULL
    assert tb(rays=None) == E_NULL and tb(images=None) == E_NULL
    assert tb(C=2) == E_SHAPE and tb(C=5) == E_SHAPE and tb(balanced=2) == E_SHAPE
    assert tb(SB=0) == E_SHAPE and tb(NV=0) == E_SHAPE and tb(B=-1) == E_SHAPE and tb(NV=2, W=32768, H=32768) == E_SHAPE
    assert tb(B=0) == 0                                     # nothing to do: no launch

    def vt(images=p, order=p, SB=1, NV=2, NS=1, W=4, H=4, C=3, balanced=1, out=p, jitter=p):
        return N.lib.pnr_views_to_tensor_u8_jitter(images, order, SB, NV, NS, W, H, C, balanced, out, jitter, None)

    assert vt(jitter=None) == E_NULL and vt(images=None) == E_NULL and vt(order=None) == E_NULL and vt(out=None) == E_NULL
    assert vt(C=1) == E_SHAPE and vt(balanced=-1) == E_SHAPE and vt(NS=0) == E_SHAPE and vt(SB=0) == E_SHAPE
    assert vt(NV=2, W=32768, H=32768) == E_SHAPE
    assert vt(out=p + 2) == E_ALIGN


def test_wrappers_check_their_arguments():
    from pixel_nerf_multiscale_amd import data, train, util
    jit = data.ColorJitter()
    assert jit.ranges == (0.15, 0.15, 0.15, 0.15) and data.ColorJitter(0.1, 0.2, 0.3, 0.4).ranges == (0.1, 0.2, 0.3, 0.4)
    img = torch.zeros(1, 2, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        util.color_jitter_plan(img.float(), jit, 1)
    with pytest.raises(ValueError):
        util.color_jitter_plan(img, (0.1, 0.1, 0.1), 1)
    with pytest.raises(ValueError):
        util.color_jitter_plan(img, jit, -1)
    with pytest.raises(ValueError):
        util.color_jitter_plan(img, jit, 1 << 64)
    with pytest.raises(RuntimeError):                       # host tensors pass the shape checks and are refused as such
        util.color_jitter_plan(img, jit, 1)
    # make_batch: a float batch, or host draws, with jitter
    kw = dict(ray_batch_size=4, nviews=[1], z_near=0.1, z_far=1.0)
    floats = {"images": torch.zeros(1, 2, 3, 4, 4), "poses": torch.zeros(1, 2, 4, 4), "focal": torch.ones(1)}
    with pytest.raises(ValueError, match="jitter"):
        train.make_batch(floats, "cpu", draws="device", seed=1, jitter=jit, **kw)
    with pytest.raises(ValueError, match="jitter"):
        train.make_batch(dict(floats, images=img), "cpu", draws="host", jitter=jit, **kw)
