"""Mask-weighted training draws without a GPU: the host model of pnr_mask_table_build / pnr_train_draw_masked
(tests/mask_draw_util.py) against brute force and against np.flatnonzero for every k, the distribution it promises, planted
mistakes that each check must catch, util.masked_sample against the reference's own function (tests/golden/masked_sample.npz),
the entry points' refusals (all returned before any launch), and make_batch's keyword: its refusals, its host path in the
generator order of the existing one, and that None makes the calls made before.

Statistical bound: a count over n draws with cell probability p has standard deviation sqrt(n p (1 - p)); 5 of them are allowed,
seed 0."""
import math
import os
import re

import numpy as np
import pytest
import torch

import golden_util as gu
import mask_draw_util as mu
import train_draw_util as du

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5
M32_ALL = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------------------ the library
def test_exports_argtypes_and_version():
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    i32, i64, u64, p = C.c_int32, C.c_int64, C.c_uint64, C.c_void_p
    assert N.PROTOTYPES["pnr_mask_table_build"] == (i32, [p, i32, i32, i32, i32, i64, i32, p, p, p])
    assert N.PROTOTYPES["pnr_train_draw_masked"] == (i32, [p, p, i32, i32, i32, i32, i64, i64, i32, u64, p, p, p])
    assert N.PROTOTYPES["pnr_train_draw_masked_at"] == (i32, [p, p, i32, i32, i32, i32, i64, i64, i32, u64, i64, p, p, p])
    for name in ("pnr_mask_table_build", "pnr_train_draw_masked", "pnr_train_draw_masked_at"):
        assert callable(getattr(N.lib, name)) and hasattr(N.lib._cdll, name)
    assert N.lib.pnr_version() == 102
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pnr.h")).read()
    comment = header[header.index("#define PNR_VERSION 102"):header.index("#define PNR_MAX_LEVELS")]
    for name in ("pnr_mask_table_build", "pnr_train_draw_masked", "pnr_train_draw_masked_at"):
        assert name in comment and re.search(rf"int32_t {name}\(", header)
    assert "draw id 11" in header and mu.DRAW_MASK_PIX == 11 and mu.DRAW_MASK_PIX not in (0, 1, 2, 3, du.DRAW_PIX, du.DRAW_VIEWS, 10)


def test_table_build_refusals_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    p = 64
    tb = lambda masks=p, N_=1, NV=2, H=3, W=5, stride=1, thresh=128, bits=p, rows=p: \
        N.lib.pnr_mask_table_build(masks, N_, NV, H, W, stride, thresh, bits, rows, None)
    assert tb(masks=None) == E_NULL and tb(bits=None) == E_NULL and tb(rows=None) == E_NULL
    assert tb(N_=0) == E_SHAPE and tb(NV=0) == E_SHAPE and tb(H=0) == E_SHAPE and tb(W=-1) == E_SHAPE
    assert tb(NV=2, H=32768, W=32768) == E_SHAPE and tb(stride=0) == E_SHAPE and tb(stride=-4) == E_SHAPE
    assert tb(thresh=0) == E_SHAPE and tb(thresh=256) == E_SHAPE and tb(thresh=-1) == E_SHAPE
    assert tb(bits=p + 2) == E_ALIGN and tb(rows=p + 1) == E_ALIGN
    assert tb(masks=None, bits=p + 2, N_=0) == E_NULL           # a refusal, whichever comes first, and no launch


def test_masked_draw_refusals_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    p = 64

    def td(bits=p, rows=p, SB=1, NV=2, W=4, H=4, B=8, B_in=4, NS=1, base=0, pix=p, views=p, at=True):
        if at:
            return N.lib.pnr_train_draw_masked_at(bits, rows, SB, NV, W, H, B, B_in, NS, 7, base, pix, views, None)
        return N.lib.pnr_train_draw_masked(bits, rows, SB, NV, W, H, B, B_in, NS, 7, pix, views, None)

    for at in (True, False):
        assert td(pix=None, at=at) == E_NULL and td(views=None, at=at) == E_NULL
        assert td(bits=None, at=at) == E_NULL and td(rows=None, at=at) == E_NULL
        assert td(NS=3, at=at) == E_SHAPE and td(NV=100, NS=65, at=at) == E_SHAPE and td(NS=-1, at=at) == E_SHAPE
        assert td(SB=0, at=at) == E_SHAPE and td(NV=0, at=at) == E_SHAPE and td(W=0, at=at) == E_SHAPE
        assert td(H=0, at=at) == E_SHAPE and td(B=-1, B_in=0, at=at) == E_SHAPE and td(NV=2, W=32768, H=32768, at=at) == E_SHAPE
        assert td(B_in=-1, at=at) == E_SHAPE and td(B_in=9, at=at) == E_SHAPE
        assert td(B=0, B_in=0, NS=0, bits=None, rows=None, pix=None, views=None, at=at) == 0    # nothing to do: no launch
    assert td(base=-1) == E_SHAPE and td(base=(1 << 63) - 1) == E_SHAPE and td(base=1 << 61, B=8) == E_SHAPE


def test_python_wrappers_check_their_arguments():
    from pixel_nerf_multiscale_amd import util
    m = torch.zeros(2, 3, 4, 5, dtype=torch.uint8)
    for kw in (dict(thresh=0), dict(thresh=256), dict(pix_stride=0)):
        with pytest.raises(ValueError):
            util.mask_table(m, **kw)
    with pytest.raises(ValueError):
        util.mask_table(torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(RuntimeError):                     # host tensors pass the shape checks and are refused as such
        util.mask_table(m)
    bits, rows = torch.zeros(2, 12, 1, dtype=torch.int32), torch.zeros(2, 13, dtype=torch.int32)
    ok = dict(bits=bits, rows=rows, SB=2, NV=3, W=5, H=4, B=8, NS=2, seed=1, prop_inside=0.5)
    call = lambda **kw: util.train_draw_masked(**{**ok, **kw})
    for kw in (dict(SB=0), dict(B=-1), dict(NS=4), dict(seed=-1), dict(seed=1 << 64), dict(prop_inside=-0.1), dict(prop_inside=1.5),
               dict(prop_inside=float("nan")), dict(bits=bits.long()), dict(rows=rows[:, :12]), dict(bits=bits[:1]), dict(obj_base=-1),
               dict(out_pix=torch.zeros(2, 7, dtype=torch.long)), dict(out_views=torch.zeros(2, 3, dtype=torch.long))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(RuntimeError):
        call()
    assert [util.num_inside(B, q) for B, q in ((5, 0.5), (10, 0.7), (8, 0.0), (8, 1.0), (3, 0.5), (128, 0.75))] == [3, 7, 0, 8, 2, 96]
    soft, hard = torch.tensor([[0.2, 0.5], [1.0, 0.49]]), torch.tensor([[0, 255], [255, 0]], dtype=torch.uint8)
    assert torch.equal(util.mask_bytes(soft[None, None, None]), hard[None, None])          # (SB, NV, 1, H, W) loses its channel axis
    assert torch.equal(util.mask_bytes(soft[None, None]), hard[None, None]) and torch.equal(util.mask_bytes(soft[None]), hard[None])
    assert torch.equal(util.mask_bytes(torch.tensor([[[True, False]]])), torch.tensor([[[255, 0]]], dtype=torch.uint8))
    assert util.mask_bytes(m) is m


# ------------------------------------------------------------------------------------------------------------ the model
def _masks(shape, density, seed=1):
    return mu.random_masks(*shape, density, seed + sum(shape))


@pytest.mark.parametrize("shape", mu.TABLE_SHAPES)
def test_model_table_is_the_brute_force_table(shape):
    for density, thresh in ((0.5, 128), (0.0, 1), (1.0, 255)):
        inside = mu.inside_of(_masks(shape, density), thresh)
        bits, rows = mu.model_table(inside)
        want_bits, want_rows = mu.brute_table(inside)
        assert np.array_equal(bits, want_bits) and np.array_equal(rows, want_rows)
        N, NV, H, W = shape
        assert rows[:, -1].tolist() == inside.reshape(N, -1).sum(axis=1).tolist()
        if W & 31:
            assert not (bits[:, :, -1] >> np.uint32(W & 31)).any()      # tail bits zero


def test_thresholds_on_random_bytes():
    rng = np.random.default_rng(3)
    b = rng.integers(0, 256, (1, 2, 3, 40), dtype=np.uint8)
    b[0, 0, 0, :6] = (0, 1, 127, 128, 254, 255)
    for thresh in (1, 128, 255):
        inside = mu.inside_of(b, thresh)
        assert inside[0, 0, 0, :6].tolist() == [v >= thresh for v in (0, 1, 127, 128, 254, 255)]
        assert np.array_equal(mu.model_table(inside)[0], mu.brute_table(inside)[0])


@pytest.mark.parametrize("shape", mu.TABLE_SHAPES)
def test_selection_is_flatnonzero_for_every_k(shape):
    N, NV, H, W = shape
    for density in (0.0, 0.3, 1.0):
        inside = mu.inside_of(_masks(shape, density))[:1]              # one object: the selection sees one object's table
        bits, rows = mu.model_table(inside)
        for want in (True, False):
            pop = np.flatnonzero(inside[0].ravel() == want)
            got = [mu.select(bits[0], rows[0], W, k, want) for k in range(len(pop))]
            assert got == pop.tolist(), (shape, density, want)


def test_an_inconsistent_table_gives_minus_one_and_stays_inside():
    """A prefix that claims more pixels than the words hold: the bit is not found.  The model indexes numpy arrays, so a read
    outside bits / rows would raise."""
    inside = mu.inside_of(_masks((1, 2, 3, 33), 0.5))
    bits, rows = mu.model_table(inside)
    first = int(rows[0, 1])                              # row 0 holds bits 0 .. first - 1 and is told to hold 40 more
    rows = rows.copy()
    rows[0, 1:] += 40
    assert mu.select(bits[0], rows[0], 33, first - 1, True) >= 0 and mu.select(bits[0], rows[0], 33, first, True) == -1
    assert mu.select(bits[0], rows[0], 33, first + 39, True) == -1
    zeros = np.zeros_like(bits)
    assert mu.select(zeros[0], rows[0], 33, 0, True) == -1


# ------------------------------------------------------------------------------------------------------------ the draws
def test_draws_are_the_definition():
    """model_draw (table + two-step selection) against brute_draw (flatnonzero), with views and an object base."""
    for shape, B, prop in (((2, 2, 3, 33), 37, 0.7), ((3, 1, 4, 65), 5, 0.5), ((2, 3, 2, 31), 8, 0.0), ((2, 3, 2, 32), 8, 1.0)):
        SB, NV, H, W = shape
        inside = mu.inside_of(_masks(shape, 0.4))
        bits, rows = mu.model_table(inside)
        B_in = mu.n_inside(B, prop)
        pix, order, src = mu.model_draw(bits, rows, SB, NV, W, H, B, B_in, min(NV, 2), 77)
        assert np.array_equal(pix, mu.brute_draw(inside, B, B_in, 77))
        assert src[:, :B_in].all() and not src[:, B_in:].any()
        flat = inside.reshape(SB, -1)
        for o in range(SB):
            assert flat[o][pix[o, :B_in]].all() and not flat[o][pix[o, B_in:]].any()
        assert np.array_equal(order, du.model_draw(None, SB, NV, W, H, 0, min(NV, 2), 77)[1])
        # a slice under an object base is the whole call's rows
        part, part_order, _ = mu.model_draw(bits[1:], rows[1:], SB - 1, NV, W, H, B, B_in, min(NV, 2), 77, obj_base=1)
        assert np.array_equal(part, pix[1:]) and np.array_equal(part_order, order[1:])
    assert mu.n_inside(5, 0.5) == 3 and mu.n_inside(10, 0.7) == 7


def test_an_empty_population_hands_its_slots_to_the_other():
    for density, kind in ((0.0, False), (1.0, True)):
        inside = mu.inside_of(_masks((1, 2, 3, 33), density))
        bits, rows = mu.model_table(inside)
        pix, _, src = mu.model_draw(bits, rows, 1, 2, 33, 3, 40, 20, 0, 5)
        assert (src == kind).all() and (pix >= 0).all() and pix.max() < 2 * 3 * 33
        assert np.array_equal(pix, mu.brute_draw(inside, 40, 20, 5))
        assert len(set(pix[0, :20].tolist())) > 10 and len(set(pix[0, 20:].tolist())) > 10


def test_distribution_is_uniform_over_each_population():
    NV, H, W, B, prop = 2, 5, 9, 36000, 0.75
    inside = mu.inside_of(mu.random_masks(1, NV, H, W, 0.4, 0))
    bits, rows = mu.model_table(inside)
    B_in = mu.n_inside(B, prop)
    pix, _, src = mu.model_draw(bits, rows, 1, NV, W, H, B, B_in, 0, 0)
    assert B_in == 27000 and int(src.sum()) == B_in and src[0, :B_in].all()
    flat = inside.ravel()
    worst = 0.0
    for want, draws in ((True, pix[0, :B_in]), (False, pix[0, B_in:])):
        cells = np.flatnonzero(flat == want)
        counts = np.bincount(draws, minlength=flat.size)
        assert counts[flat != want].sum() == 0, "a pixel of the other population"
        p = 1.0 / len(cells)
        dev = np.abs(counts[cells] - len(draws) * p) / math.sqrt(len(draws) * p * (1.0 - p))
        worst = max(worst, dev.max())
        assert (counts[cells] > 0).all() and dev.max() <= 5.0, (want, dev.max())
    print(f"mask draws: worst deviation {worst:.2f} sigma")


# ------------------------------------------------------------------------------------------------------------ planted mistakes
def _checks(v):
    """Every check above in small, run on the model under variant v -> the names of the checks that fail."""
    failed = []
    for shape in ((2, 2, 3, 33), (1, 3, 4, 40)):
        SB, NV, H, W = shape
        inside = mu.inside_of(_masks(shape, 0.45))
        right_bits, right_rows = mu.brute_table(inside)
        bits, rows = mu.model_table(inside, v)
        if not (np.array_equal(bits, right_bits) and np.array_equal(rows, right_rows)):
            failed.append("table")
        for want in (True, False):
            pop = np.flatnonzero(inside[0].ravel() == want)
            if [mu.select(right_bits[0], right_rows[0], W, k, want, v) for k in range(len(pop))] != pop.tolist():
                failed.append("selection")
        B = 41
        B_in = mu.n_inside(B, 0.5, v)
        if B_in != 21:
            failed.append("slot split")
        if not np.array_equal(mu.model_draw(right_bits, right_rows, SB, NV, W, H, B, 21, 0, 0, v=v)[0], mu.brute_draw(inside, B, 21, 0)):
            failed.append("draws")
    # an inconsistent table — every pixel of a 33-wide row inside, a prefix that says none is: the outside bit asked for does
    # not exist and must come back as -1, not as one of the last word's 31 tail bits
    full = np.array([[M32_ALL, 1]], np.uint32)
    if mu.select(full, np.array([0, 0], np.uint32), 33, 0, False, v) != -1:
        failed.append("not found")
    return set(failed)


def test_the_model_passes_its_own_checks():
    assert _checks(mu.RIGHT) == set()


@pytest.mark.parametrize("field,caught_by", [("msb_first", "table"), ("tail_outside", "draws"), ("lower_bound", "selection"),
                                             ("floor_inside", "slot split"), ("per_view", "draws"), ("no_tail_mask", "not found")])
def test_planted_mistakes_are_caught(field, caught_by):
    failed = _checks(mu.Variant(**{field: True}))
    assert caught_by in failed, (field, failed)


# ------------------------------------------------------------------------------------------------------------ the host sampler
def test_masked_sample_is_the_reference_function():
    from pixel_nerf_multiscale_amd import util
    d = np.load(os.path.join(gu.GOLDEN_DIR, "masked_sample.npz"))
    names = str(d["names"]).split(",")
    assert len(names) == 5
    for name in names:
        masks = torch.from_numpy(d[f"{name}__masks"])
        num_pix, prop, thresh = d[f"{name}__args"].tolist()
        for m in (masks, masks[:, None]):                                  # (NV, H, W) and the loader's (NV, 1, H, W)
            torch.manual_seed(int(d[f"{name}__seed"]))
            pix = util.masked_sample(m, int(num_pix), prop, thresh)
            assert pix.dtype == torch.long and np.array_equal(pix.numpy(), d[f"{name}__pix"]), name
            assert np.array_equal(torch.get_rng_state().numpy(), d[f"{name}__rng_end"]), name
        n_in = int(num_pix * prop + 0.5)
        vals = masks[pix[:, 0], pix[:, 1], pix[:, 2]]
        assert bool((vals[:n_in] >= thresh).all()) and bool((vals[n_in:] < thresh).all())
    disc = torch.from_numpy(d["disc_07__masks"])
    for empty in (torch.zeros_like(disc), torch.ones_like(disc)):
        with pytest.raises(ValueError):
            util.masked_sample(empty, 10, 0.7)
    with pytest.raises(ValueError):
        util.masked_sample(disc[0], 10, 0.7)


# ------------------------------------------------------------------------------------------------------------ make_batch
def _data(masks=True, as_bytes=False):
    SB, NV, H, W = 2, 3, 6, 7
    rng = np.random.default_rng(11)
    m = torch.from_numpy(rng.random((SB, NV, H, W)) < 0.4)
    data = {"images": torch.zeros(SB, NV, H, W, 3, dtype=torch.uint8) if as_bytes else torch.zeros(SB, NV, 3, H, W),
            "poses": torch.zeros(SB, NV, 4, 4), "focal": torch.ones(SB),
            "bbox": torch.tensor([0.0, 0.0, W - 1.0, H - 1.0]).expand(SB, NV, 4).contiguous()}
    if masks:
        data["masks"] = m.to(torch.uint8) * 255 if as_bytes else m[:, :, None].float()
    return data


KW = dict(ray_batch_size=10, nviews=[2], z_near=0.1, z_far=1.0)


def test_make_batch_refusals():
    from pixel_nerf_multiscale_amd import train
    for draws in (dict(), dict(draws="device", seed=3)):
        with pytest.raises(ValueError, match="masks"):
            train.make_batch(_data(masks=False), "cpu", prop_inside=0.5, **draws, **KW)
        for bad in (-0.25, 1.01, float("nan")):
            with pytest.raises(ValueError, match="prop_inside"):
                train.make_batch(_data(), "cpu", prop_inside=bad, **draws, **KW)
    # the tables alone do not serve host draws
    tables = dict(_data(masks=False), mask_bits=torch.zeros(2, 18, 1, dtype=torch.int32), mask_rows=torch.zeros(2, 19, dtype=torch.int32))
    with pytest.raises(ValueError, match="masks"):
        train.make_batch(tables, "cpu", prop_inside=0.5, **KW)


def _spied(monkeypatch, data, **kw):
    """make_batch on the CPU with every native call and the gather replaced by recorders -> the calls' names, in order, with
    what the draw received."""
    from pixel_nerf_multiscale_amd import train, util
    calls = []
    real_empty = torch.empty
    SB, B = data["poses"].shape[0], KW["ray_batch_size"]

    def rec(name, result):
        def f(*a, **k):
            calls.append((name, a, k))
            return result(*a, **k) if callable(result) else result
        return f

    draw = (torch.zeros(SB, B, dtype=torch.long), torch.zeros(SB, 2, dtype=torch.long))
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: real_empty(*a, **k))
    monkeypatch.setattr(util, "upload", lambda t, device: t)
    monkeypatch.setattr(util, "train_draw", rec("train_draw", draw))
    monkeypatch.setattr(util, "train_draw_masked", rec("train_draw_masked", draw))
    monkeypatch.setattr(util, "mask_table", rec("mask_table", ("BITS", "ROWS")))
    monkeypatch.setattr(util, "bbox_sample", rec("bbox_sample", util.bbox_sample))
    monkeypatch.setattr(util, "masked_sample", rec("masked_sample", util.masked_sample))
    monkeypatch.setattr(train, "_gather_batch", rec("gather", None))
    train.make_batch(data, "cpu", **kw, **KW)
    monkeypatch.undo()
    return calls


def test_none_makes_the_calls_made_before(monkeypatch):
    dev = dict(draws="device", seed=9)
    for data in (_data(), _data(as_bytes=True), _data(masks=False)):
        for kw in (dev, dict(dev, use_bbox=False), dict(dev, is_train=False), dict(dev, obj_base=4)):
            a, b = _spied(monkeypatch, data, **kw), _spied(monkeypatch, data, prop_inside=None, **kw)
            assert [c[0] for c in a] == [c[0] for c in b] == ["train_draw", "gather"]
            (_, args_a, kw_a), (_, args_b, kw_b) = a[0], b[0]
            assert args_a[1:] == args_b[1:] and kw_a["obj_base"] == kw_b["obj_base"] and sorted(kw_a) == sorted(kw_b) == ["obj_base", "out_pix"]
            assert (args_a[0] is None) == (args_b[0] is None) == (not (kw.get("use_bbox", True) and kw.get("is_train", True)))
        torch.manual_seed(4); np.random.seed(4)
        host = _spied(monkeypatch, data, prop_inside=None)
        assert [c[0] for c in host] == ["bbox_sample", "bbox_sample", "gather"]


def test_prop_inside_takes_the_place_of_the_boxes(monkeypatch):
    dev = dict(draws="device", seed=9, prop_inside=0.3)
    for data in (_data(), _data(as_bytes=True)):
        calls = _spied(monkeypatch, data, obj_base=2, **dev)
        assert [c[0] for c in calls] == ["mask_table", "train_draw_masked", "gather"]
        table_in = calls[0][1][0]
        assert table_in.dtype == torch.uint8 and tuple(table_in.shape) == (2, 3, 6, 7)
        want = data["masks"] if data["masks"].dtype == torch.uint8 else (data["masks"][:, :, 0] >= 0.5).to(torch.uint8) * 255
        assert torch.equal(table_in, want)
        _, a, k = calls[1]
        assert a[:2] == ("BITS", "ROWS") and a[2:] == (2, 3, 7, 6, 10, 2, 9, 0.3) and k["obj_base"] == 2 and tuple(k["out_pix"].shape) == (2, 10)
        # a resident batch brings its tables: nothing is built
        calls = _spied(monkeypatch, dict(data, mask_bits="B", mask_rows="R"), **dev)
        assert [c[0] for c in calls] == ["train_draw_masked", "gather"] and calls[0][1][:2] == ("B", "R")
        # evaluation and the steps past no_bbox_step never see it
        for off in (dict(is_train=False), dict(use_bbox=False)):
            calls = _spied(monkeypatch, data, **dev, **off)
            assert [c[0] for c in calls] == ["train_draw", "gather"] and calls[0][1][0] is None
            assert [c[0] for c in _spied(monkeypatch, _data(masks=False), **dev, **off)] == ["train_draw", "gather"]


@pytest.mark.parametrize("as_bytes", [False, True])
def test_host_draws_use_masked_sample_in_the_generator_order(monkeypatch, as_bytes):
    from pixel_nerf_multiscale_amd import util
    data = _data(as_bytes=as_bytes)
    torch.manual_seed(21); np.random.seed(21)
    calls = _spied(monkeypatch, data, prop_inside=0.7)
    end = (torch.get_rng_state(), np.random.get_state()[1].copy())
    assert [c[0] for c in calls] == ["masked_sample", "masked_sample", "gather"]
    pix_inds, image_ord = calls[-1][1][4], calls[-1][1][5]

    torch.manual_seed(21); np.random.seed(21)
    assert int(torch.randint(0, 1, ())) == 0                                # curr_nviews
    inside = data["masks"] >= 128 if as_bytes else data["masks"][:, :, 0] >= 0.5
    for o in range(2):
        want_ord = torch.from_numpy(np.random.choice(3, 2, replace=False))
        p = util.masked_sample(inside[o].float(), 10, 0.7)
        assert torch.equal(image_ord[o], want_ord) and torch.equal(pix_inds[o], p[:, 0] * 42 + p[:, 1] * 7 + p[:, 2])
        assert bool(inside[o].reshape(-1)[pix_inds[o, :7]].all()) and not bool(inside[o].reshape(-1)[pix_inds[o, 7:]].any())
    assert torch.equal(end[0], torch.get_rng_state()) and np.array_equal(end[1], np.random.get_state()[1])


def test_trainer_and_step_carry_the_keyword():
    import inspect
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.trainer import Trainer
    for fn in (train.make_batch, train.calc_losses, Trainer.__init__):
        assert inspect.signature(fn).parameters["prop_inside"].default is None
    assert inspect.signature(ResidentSplit.__init__).parameters["device_masks"].default is False
