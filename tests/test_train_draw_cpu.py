"""The training draws without a GPU: the host model of pnr_train_draw (tests/train_draw_util.py) — its counter layout as
plain ints, the distribution it promises (a uniform view, then a uniform cell of its box; a uniformly random ordered subset of
the views), permutations and invalid boxes — then the argument checks of util.train_draw and make_batch, and that
draws="host" consumes torch's and numpy's global generators exactly as before.

Statistical bounds: a count over n draws with cell probability p has standard deviation sqrt(n p (1 - p)); the tests allow
5 of them (seed 20240917; the model's worst deviations are 2.93 and 2.46) and ask that every cell and every triple occurs."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import train_draw_util as du
from sampler_util import philox4x32_10

SEED = 20240917


# ------------------------------------------------------------------------------------------------------------ layout
def test_counter_layout_as_plain_ints():
    seed = (0x89ABCDEF << 32) | 0x01234567
    assert du.pixel_counter(seed, 0, 0, 7) == (0x01234567, 0x89ABCDEF, 0, 0, 8, 0)
    assert du.pixel_counter(seed, 3, 5, 1000) == (0x01234567, 0x89ABCDEF, 3005, 0, 8, 0)
    # o B + j past 2^32: only the counter's high word tells the two pixels apart
    B = 1 << 31
    assert du.pixel_counter(seed, 2, 9, B) == (0x01234567, 0x89ABCDEF, 9, 1, 8, 0)
    assert du.pixel_counter(seed, 0, 9, B) == (0x01234567, 0x89ABCDEF, 9, 0, 8, 0)
    assert du.view_counter(seed, 0, 0) == (0x01234567, 0x89ABCDEF, 0, 0, 9, 0, 0)
    assert du.view_counter(seed, 6, 7) == (0x01234567, 0x89ABCDEF, 6, 0, 9, 1, 3)
    assert du.view_counter(seed, (1 << 32) + 6, 4) == (0x01234567, 0x89ABCDEF, 6, 1, 9, 1, 0)


def test_the_high_counter_word_changes_the_block():
    seed = 5
    lo = [int(w) for w in philox4x32_10(*du.pixel_counter(seed, 0, 9, 1 << 31))]
    hi = [int(w) for w in philox4x32_10(*du.pixel_counter(seed, 2, 9, 1 << 31))]
    assert lo != hi and all(0 <= w < 1 << 32 for w in lo + hi)


def test_model_follows_the_layout():
    """model_draw's vectorised blocks against the same draws taken one counter at a time."""
    SB, NV, W, H, B, NS = 3, 5, 7, 6, 4, 5
    bbox = np.tile(np.array([1.0, 2.0, 4.0, 3.0], np.float32), (SB, NV, 1))
    pix, order, pview = du.model_draw(bbox, SB, NV, W, H, B, NS, SEED)
    for o, j in ((0, 0), (2, 3)):
        x, y, z, _ = (int(w) for w in philox4x32_10(*du.pixel_counter(SEED, o, j, B)))
        view = (x * NV) >> 32
        col, row = 1 + ((y * 4) >> 32), 2 + ((z * 2) >> 32)
        assert pview[o, j] == view and pix[o, j] == view * H * W + row * W + col
    for o, s in ((0, 0), (2, 4)):
        c = du.view_counter(SEED, o, s)
        words = [int(philox4x32_10(*du.view_counter(SEED, o, q)[:6])[du.view_counter(SEED, o, q)[6]]) for q in range(s + 1)]
        assert c[5] == s >> 2 and c[6] == s & 3
        assert du.views_from_words(words, NV) == order[o, :s + 1].tolist()


def test_known_answers():
    """Words of the published generator at this layout, and the draws they give (values worked out once, by hand from the
    words: the arithmetic is three multiplications and shifts)."""
    x, y, z, w = (int(v) for v in philox4x32_10(*du.pixel_counter(SEED, 1, 2, 10)))
    view, idx = du.pixel_from_words(x, y, z, None, 3, 16, 12, False)
    assert view == (x * 3) >> 32 and idx == view * 192 + ((z * 12) >> 32) * 16 + ((y * 16) >> 32)
    # the walk: words that ask for "the first view left" three times give 0, 1, 2; "the last view left" gives 4, 3, 2
    assert du.views_from_words([0, 0, 0], 5) == [0, 1, 2]
    assert du.views_from_words([0xFFFFFFFF] * 3, 5) == [4, 3, 2]
    # t = 1 of 4 left after {1} was taken -> pushed to 2; then t = 1 of 3 left after {1, 2} -> pushed twice to 3
    assert du.views_from_words([(1 << 32) // 5 + 1, (1 << 32) // 4 + 1, (1 << 32) // 3 + 1], 5) == [1, 2, 3]
    # Philox4x32-10 itself: the published known-answer vectors (Random123 kat_vectors)
    assert [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert [int(v) for v in philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)] == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


# ------------------------------------------------------------------------------------------------------------ statistics
BOXES = np.array([[[2, 1, 6, 3], [0, 0, 15, 11], [5, 5, 5, 5]],
                  [[15, 11, 15, 11], [3, 2, 4, 9], [0, 4, 15, 4]]], np.float32)


def test_boxed_pixels_are_uniform_over_view_and_box():
    SB, NV, W, H, B = 2, 3, 16, 12, 32768
    pix, _, pview = du.model_draw(BOXES, SB, NV, W, H, B, 0, SEED)
    assert (pix >= 0).all() and (pix // (H * W) == pview).all()
    worst = 0.0
    for o in range(SB):
        counts = np.bincount(pix[o], minlength=NV * H * W).reshape(NV, H, W)
        inside = np.zeros((NV, H, W), bool)
        for v in range(NV):
            cmin, rmin, cmax, rmax = (int(t) for t in BOXES[o, v])
            inside[v, rmin:rmax + 1, cmin:cmax + 1] = True
            p = 1.0 / (NV * (cmax + 1 - cmin) * (rmax + 1 - rmin))
            sigma = math.sqrt(B * p * (1.0 - p))
            cell = counts[v][inside[v]]
            dev = np.abs(cell - B * p).max() / sigma
            worst = max(worst, dev)
            assert (cell > 0).all(), (o, v, "a cell of the box is never drawn")
            assert dev <= 5.0, (o, v, dev)
        assert counts[~inside].sum() == 0, (o, "a pixel outside its box")
    print(f"boxed pixels: worst deviation {worst:.2f} sigma")


def test_unboxed_pixels_cover_the_image():
    SB, NV, W, H, B = 1, 2, 5, 3, 6000
    pix, _, _ = du.model_draw(None, SB, NV, W, H, B, 0, SEED)
    counts = np.bincount(pix[0], minlength=NV * H * W)
    p = 1.0 / (NV * H * W)
    assert len(counts) == NV * H * W and (np.abs(counts - B * p) <= 5.0 * math.sqrt(B * p * (1 - p))).all()


def test_ordered_view_subsets_are_uniform():
    N, NV, NS = 61440, 5, 3
    _, order, _ = du.model_draw(None, N, NV, 1, 1, 0, NS, SEED)
    keys = order[:, 0] * 25 + order[:, 1] * 5 + order[:, 2]
    triples = [a * 25 + b * 5 + c for a, b, c in itertools.permutations(range(NV), NS)]
    counts = np.bincount(keys, minlength=125)
    assert len(triples) == 60 and counts.sum() == counts[triples].sum() == N        # distinct views only
    p = 1.0 / 60
    dev = np.abs(counts[triples] - N * p) / math.sqrt(N * p * (1 - p))
    print(f"ordered triples: worst deviation {dev.max():.2f} sigma")
    assert (counts[triples] > 0).all() and dev.max() <= 5.0


def test_all_views_give_a_permutation():
    for NV in (1, 2, 5, 64):
        _, order, _ = du.model_draw(None, 7, NV, 1, 1, 0, NV, SEED + NV)
        for row in order:
            assert sorted(row.tolist()) == list(range(NV))
    assert len({tuple(r) for r in du.model_draw(None, 50, 5, 1, 1, 0, 5, SEED)[1].tolist()}) > 25


@pytest.mark.parametrize("bad", [[np.nan, 1, 3, 3], [1, 1, np.inf, 3], [4, 1, 3, 3], [1, 5, 3, 4], [-1, 0, 3, 3], [0, 0, 16, 3],
                                 [0, 0, 3, 12], [0, -1.5, 3, 3], [3e9, 0, 3e9, 3]])
def test_invalid_box_gives_minus_one_for_its_view_only(bad):
    SB, NV, W, H, B = 2, 3, 16, 12, 300
    boxes = BOXES.copy()
    boxes[1, 1] = bad
    pix, _, pview = du.model_draw(boxes, SB, NV, W, H, B, 0, SEED)
    hit = np.zeros((SB, B), bool)
    hit[1] = pview[1] == 1
    assert hit.any() and (pix[hit] == -1).all() and (pix[~hit] >= 0).all()
    good, _, _ = du.model_draw(BOXES, SB, NV, W, H, B, 0, SEED)
    assert np.array_equal(pix[~hit], good[~hit])


def test_a_fraction_truncates_towards_zero():
    """-0.5 truncates to 0 and 3.9 to 3: a valid box, the cells 0..3."""
    boxes = np.array([[[-0.5, 0.25, 3.9, 0.75]]], np.float32)
    pix, _, _ = du.model_draw(boxes, 1, 1, 8, 8, 400, 0, SEED)
    assert sorted(set(pix[0].tolist())) == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------------------------ arguments
def test_train_draw_checks_its_arguments():
    from pixel_nerf_multiscale_amd import util
    ok = dict(bbox=None, SB=2, NV=3, W=16, H=12, B=8, NS=2, seed=1)
    call = lambda **kw: util.train_draw(**{**ok, **kw})
    for kw in (dict(SB=0), dict(NV=0), dict(W=0), dict(H=-1), dict(B=-1), dict(NS=-1), dict(NS=4), dict(NV=100, NS=65),
               dict(seed=-1), dict(seed=1 << 64), dict(bbox=torch.zeros(2, 3, 3)), dict(bbox=torch.zeros(2, 3, 4, dtype=torch.float64)),
               dict(bbox=np.zeros((2, 3, 4), np.float32)), dict(out_pix=torch.zeros(2, 7, dtype=torch.long)),
               dict(out_pix=torch.zeros(2, 8, dtype=torch.int32)), dict(out_views=torch.zeros(2, 3, dtype=torch.long)),
               dict(out_pix=torch.zeros(8, 2, dtype=torch.long).t())):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(RuntimeError):                     # host tensors pass the shape checks and are refused as such
        call(bbox=torch.zeros(2, 3, 4))


def test_entry_point_refusals_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    E_NULL, E_SHAPE, p = -1, -2, 64
    td = lambda bbox=None, SB=1, NV=2, W=4, H=4, B=8, NS=1, pix=p, views=p: \
        N.lib.pnr_train_draw(bbox, SB, NV, W, H, B, NS, 7, pix, views, None)
    assert td(pix=None) == E_NULL and td(views=None) == E_NULL
    assert td(NS=3) == E_SHAPE and td(NV=100, NS=65) == E_SHAPE and td(NS=-1) == E_SHAPE
    assert td(SB=0) == E_SHAPE and td(NV=0) == E_SHAPE and td(W=0) == E_SHAPE and td(H=0) == E_SHAPE and td(B=-1) == E_SHAPE
    assert td(NV=2, W=32768, H=32768) == E_SHAPE
    assert td(B=0, NS=0, pix=None, views=None) == 0       # nothing to do: no launch


def test_make_batch_checks_draws_and_seed():
    from pixel_nerf_multiscale_amd import train
    data = {"images": torch.zeros(1, 2, 3, 4, 4), "poses": torch.zeros(1, 2, 4, 4), "focal": torch.ones(1)}
    kw = dict(ray_batch_size=4, nviews=[1], z_near=0.1, z_far=1.0)
    with pytest.raises(ValueError, match="seed"):
        train.make_batch(data, "cpu", draws="device", **kw)
    with pytest.raises(ValueError, match="draws"):
        train.make_batch(data, "cpu", draws="gpu", seed=1, **kw)


def test_curr_nviews_rule():
    from pixel_nerf_multiscale_amd import train
    assert [train.curr_nviews_for([1, 2, 5], s) for s in (0, 1, 2, 3, 7, (1 << 63) - 1)] == [1, 2, 5, 1, 2, [1, 2, 5][((1 << 63) - 1) % 3]]


# ------------------------------------------------------------------------------------------------------------ host draws
def _fixture(name):
    d = np.load(os.path.join(gu.GOLDEN_DIR, "train_batch.npz"))
    return {k[len(name) + 2:]: d[k] for k in d.files if k.startswith(name + "__")}


def _host_make_batch(monkeypatch, data, nviews, use_bbox, free_curr_nviews):
    """make_batch(draws="host") on the CPU: the pinned allocation, the uploads and the native gathers are replaced (there is
    no CPU seam), the draws are not.  free_curr_nviews: the 0-dim randint that picks curr_nviews leaves the generator where
    it found it, so the pixel draws start where the fixture's did.  -> (pix_inds, image_ord) as the gathers received them."""
    from pixel_nerf_multiscale_amd import train, util
    seen = {}
    real_empty, real_randint = torch.empty, torch.randint

    def empty(*a, pin_memory=False, **kw):
        return real_empty(*a, **kw)

    def randint(*a, **kw):
        if free_curr_nviews and len(a) == 3 and a[2] == ():
            state = torch.get_rng_state()
            out = real_randint(*a, **kw)
            torch.set_rng_state(state)
            return out
        return real_randint(*a, **kw)

    def train_batch(images, poses, focal, c, pix_inds, z_near, z_far):
        seen["pix_inds"] = pix_inds.clone()
        return torch.zeros(*pix_inds.shape, 8), torch.zeros(*pix_inds.shape, 3)

    def select(t, inds):
        seen.setdefault("image_ord", inds.clone())
        return t[torch.arange(t.shape[0])[:, None].expand_as(inds), inds]

    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(torch, "randint", randint)
    monkeypatch.setattr(util, "upload", lambda t, device: t)
    monkeypatch.setattr(util, "train_batch", train_batch)
    monkeypatch.setattr(util, "batched_index_select_nd", select)
    train.make_batch(data, "cpu", ray_batch_size=67, nviews=nviews, z_near=0.8, z_far=1.8, use_bbox=use_bbox)
    monkeypatch.undo()
    return seen["pix_inds"], seen["image_ord"]


@pytest.mark.parametrize("name", ["boxes_fxfy_c", "uniform_scalar_f"])
def test_host_draws_consume_the_generators_as_before(monkeypatch, name):
    """The pixels make_batch(draws="host") hands the gather are the fixture's (recorded from the reference under the same
    torch seed), and both global generators end where the draws of the previous make_batch, repeated by hand, leave them."""
    from pixel_nerf_multiscale_amd import util
    fx = _fixture(name)
    boxed = fx["bboxes"].size > 0
    data = {"images": torch.from_numpy(fx["images"]), "poses": torch.from_numpy(fx["poses"]), "focal": torch.from_numpy(fx["focal"])}
    if boxed:
        data["bbox"] = torch.from_numpy(fx["bboxes"])
        data["c"] = torch.from_numpy(fx["c"])
    SB, NV, _, H, W = fx["images"].shape
    seed = int(fx["seed"])

    torch.manual_seed(seed); np.random.seed(seed)
    pix, _ = _host_make_batch(monkeypatch, data, [2], boxed, free_curr_nviews=True)
    assert np.array_equal(pix.numpy(), fx["pix_inds"])

    for nviews in ([2], [1], [1, 2, 3]):
        torch.manual_seed(seed); np.random.seed(seed)
        pix, order = _host_make_batch(monkeypatch, data, nviews, boxed, free_curr_nviews=False)
        t_state, n_state = torch.get_rng_state(), np.random.get_state()[1].copy()

        torch.manual_seed(seed); np.random.seed(seed)
        curr = nviews[int(torch.randint(0, len(nviews), ()))]
        want_ord = torch.randint(0, NV, (SB, 1)) if curr == 1 else torch.empty(SB, curr, dtype=torch.long)
        want_pix = torch.empty(SB, 67, dtype=torch.long)
        for o in range(SB):
            if curr > 1:
                want_ord[o] = torch.from_numpy(np.random.choice(NV, curr, replace=False))
            if boxed:
                p = util.bbox_sample(data["bbox"][o], 67)
                want_pix[o] = p[:, 0] * (H * W) + p[:, 1] * W + p[:, 2]
            else:
                want_pix[o] = torch.randint(0, NV * H * W, (67,))
        assert torch.equal(pix, want_pix) and torch.equal(order, want_ord)
        assert torch.equal(t_state, torch.get_rng_state()) and np.array_equal(n_state, np.random.get_state()[1])


def test_device_draws_leave_the_generators_alone():
    """draws="device" never touches torch's or numpy's generator: the source of make_batch's device branch has no draw."""
    import ast
    import inspect
    import textwrap
    from pixel_nerf_multiscale_amd import train
    tree = ast.parse(textwrap.dedent(inspect.getsource(train.make_batch)))
    branch = [n for n in ast.walk(tree) if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
              and getattr(n.test.left, "id", None) == "draws" and getattr(n.test.comparators[0], "value", None) == "device"
              and any(isinstance(b, ast.Return) for b in n.body)]
    assert len(branch) == 1
    called = {c.func.attr for c in ast.walk(branch[0]) if isinstance(c, ast.Call) and isinstance(c.func, ast.Attribute)}
    assert "train_draw" in called and not called & {"randint", "rand", "choice", "bbox_sample", "randperm", "pin_memory"}
