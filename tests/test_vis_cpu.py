"""Visualisation, host side: the four entry points are declared, bound and exported; every argument check of pnr_cmap and
pnr_vis_panel (all made before any launch, so they run without a GPU); the workspace sizes; util.cmap's quantisation against
the reference's own function (tests/golden/vis_quantize.npz, written by tools/gen_golden_vis.py) and against the numpy model
of tests/vis_util.py; the default table; the panel layout; vis_step's draws and refusals; validate."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vis_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -4
NAMES = ("pnr_cmap_workspace_bytes", "pnr_cmap", "pnr_vis_panel_workspace_bytes", "pnr_vis_panel")


def test_the_four_prototypes_are_declared_bound_and_exported():
    from pixel_nerf_multiscale_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    assert "vis.hip" in __import__("pixel_nerf_multiscale_amd.build_native", fromlist=["SOURCES"]).SOURCES
    assert int(re.search(r"#define PNR_VIS_MAX_SRC (\d+)", hdr).group(1)) == N.PNR_VIS_MAX_SRC == 8
    assert "parity unpinned" in hdr.lower()


def test_cmap_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p, big = 64, 1 << 20          # a non-NULL value: the checks return before anything dereferences or launches

    def cm(map=p, stride=0, W=16, H=16, lut=p, out=p, mm=None, ws=p, ws_bytes=big):
        return L.pnr_cmap(map, stride, W, H, lut, out, mm, ws, ws_bytes, None)

    assert cm(map=None) == E_NULL and cm(out=None) == E_NULL and cm(lut=None) == E_NULL and cm(ws=None) == E_NULL
    assert cm(W=0) == E_SHAPE and cm(H=0) == E_SHAPE and cm(W=-3) == E_SHAPE
    assert cm(W=65536, H=32768) == E_SHAPE and cm(W=46341, H=46341) == E_SHAPE          # W * H >= 2^31
    assert cm(stride=-1) == E_SHAPE
    need = L.pnr_cmap_workspace_bytes(16, 16)
    assert cm(ws_bytes=need - 1) == E_WORKSPACE and cm(ws_bytes=0, W=300, H=400) == E_WORKSPACE
    with pytest.raises(ValueError):
        N.check(cm(ws_bytes=0), "pnr_cmap")


def test_vis_panel_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p, big = 64, 1 << 24

    def vp(images=p, NV=5, src=(0, 2), NS=None, gt=1, passes="dense", n_pass=None, W=16, H=16, lut=p, f32=None, u8=None,
           alpha=None, stats=None, mse=None, ws=p, ws_bytes=big, K=4, strides=(0, 0, 0), missing=None, no_src=False):
        arr = None
        if passes is not None:
            n = 2 if passes == "two" else 1
            arr = (N.pnr_vis_pass * 2)()
            for i in range(2):
                arr[i].rgb, arr[i].depth, arr[i].weights = p, p, p
                arr[i].rgb_stride, arr[i].depth_stride, arr[i].weights_stride = strides
                arr[i].K = K
            if missing is not None:
                setattr(arr[n - 1], missing, None)
            n_pass = n if n_pass is None else n_pass
        srcs = None if no_src else (C.c_int32 * max(len(src), 1))(*src)
        return L.pnr_vis_panel(images, NV, srcs, len(src) if NS is None else NS, gt, arr, 1 if n_pass is None else n_pass, W, H,
                               lut, f32, u8, alpha, stats, mse, ws, ws_bytes, None)

    assert vp(images=None, f32=p) == E_NULL and vp(no_src=True, f32=p) == E_NULL
    assert vp(passes=None, f32=p) == E_NULL and vp(lut=None, f32=p) == E_NULL
    for field in ("rgb", "depth", "weights"):
        assert vp(missing=field, f32=p) == E_NULL and vp(passes="two", missing=field, f32=p) == E_NULL
    assert vp(mse=p, ws=None) == E_NULL                                     # mse without a workspace
    assert vp(f32=p, W=0) == E_SHAPE and vp(f32=p, H=0) == E_SHAPE and vp(f32=p, W=-3) == E_SHAPE
    assert vp(f32=p, W=65536, H=32768) == E_SHAPE and vp(f32=p, W=46341, H=46341) == E_SHAPE
    assert vp(f32=p, n_pass=0) == E_SHAPE and vp(f32=p, n_pass=3) == E_SHAPE
    assert vp(f32=p, src=(), NS=0) == E_SHAPE and vp(f32=p, src=tuple(range(9)), NV=12, gt=10) == E_SHAPE
    assert vp(f32=p, src=tuple(range(8)), NV=12, gt=10, ws_bytes=0) == E_WORKSPACE      # 8 sources pass the shape checks
    assert vp(f32=p, NV=0) == E_SHAPE
    assert vp(f32=p, gt=-1) == E_SHAPE and vp(f32=p, gt=5) == E_SHAPE
    assert vp(f32=p, src=(0, 5)) == E_SHAPE and vp(f32=p, src=(-1,)) == E_SHAPE
    assert vp(f32=p, K=0) == E_SHAPE
    assert vp(f32=p, strides=(2, 0, 0)) == E_SHAPE and vp(f32=p, strides=(0, -1, 0)) == E_SHAPE
    assert vp(f32=p, strides=(0, 0, 3)) == E_SHAPE and vp(f32=p, strides=(0, 0, 3), passes="two") == E_SHAPE
    for n, which in ((1, "dense"), (2, "two")):
        need = L.pnr_vis_panel_workspace_bytes(16, 16, n)
        for out in ("f32", "u8", "alpha", "stats", "mse"):
            assert vp(passes=which, ws_bytes=need - 1, **{out: p}) == E_WORKSPACE, (n, out)
    assert vp(f32=p, ws_bytes=0, W=300, H=400) == E_WORKSPACE
    assert vp() == 0 and vp(passes="two", ws=None, ws_bytes=0) == 0          # every output NULL: no launch
    with pytest.raises(ValueError):
        N.check(vp(f32=p, ws_bytes=0), "pnr_vis_panel")


def test_workspace_bytes_grow_with_the_tile_count():
    from pixel_nerf_multiscale_amd import _native as N
    cw, pw = N.lib.pnr_cmap_workspace_bytes, N.lib.pnr_vis_panel_workspace_bytes
    assert cw(1, 1) > 0 and cw(1, 1) == cw(16, 16) < cw(17, 16) == cw(16, 17)
    sizes = [cw(n, n) for n in (1, 16, 17, 32, 33, 64, 128, 129, 400)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[2] < sizes[4] < sizes[-1]
    assert cw(400, 300) == cw(300, 400) >= 8 * 25 * 19
    assert cw(0, 16) == 0 and cw(16, -1) == 0 and cw(65536, 32768) == 0
    for n in (1, 2):
        sizes = [pw(s, s, n) for s in (1, 16, 17, 32, 33, 64, 128, 129, 400)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
        assert pw(400, 300, n) == pw(300, 400, n) >= 4 * n * 400 * 300 + (8 + 24 * n) * 25 * 19
    assert pw(33, 17, 2) > pw(33, 17, 1)
    assert pw(0, 16, 1) == 0 and pw(16, -1, 2) == 0 and pw(65536, 32768, 1) == 0 and pw(16, 16, 0) == 0 and pw(16, 16, 3) == 0


# ------------------------------------------------------------------------------------------------------- the arithmetic
def test_quantisation_equals_the_reference_fixture_and_the_model():
    from pixel_nerf_multiscale_amd import util
    fx = vu.load_quantize_fixture()
    assert {"uniform", "ramp_ties", "constant", "zeros", "range_1e-12", "negative"} <= set(fx)
    ident = np.arange(256, dtype=np.uint8)[:, None].repeat(3, axis=1)        # a table that shows the byte itself
    for name, (m, want) in fx.items():
        assert m.dtype == np.float32 and want.dtype == np.uint8
        got = util.cmap(m, ident)
        assert got.shape == m.shape + (3,) and got.dtype == np.uint8
        assert np.array_equal(got[..., 0], want) and np.array_equal(got[..., 2], want), name
        assert np.array_equal(vu.quantize(m), want), name
        assert np.array_equal(util.cmap(m), vu.cmap(m, vu.model_lut())), name
    assert fx["uniform"][0].shape == (13, 19)
    assert len(np.unique(fx["ramp_ties"][1])) > 40 and fx["uniform"][1].max() == 255 and fx["negative"][1].max() == 255
    for name in ("constant", "zeros", "range_1e-12"):
        assert not fx[name][1].any(), name


def test_reference_maps_with_the_default_table():
    from pixel_nerf_multiscale_amd import util
    lut = util.hot_lut()
    rng = np.random.default_rng(5)
    nan_map = rng.uniform(0, 1, (7, 9)).astype(np.float32)
    nan_map[3, 4] = np.nan
    for m in (np.full((7, 9), 0.7, np.float32), np.full((7, 9), -2.5, np.float32), nan_map, np.zeros((7, 9), np.float32)):
        out = util.cmap(m)
        assert out.shape == (7, 9, 3) and (out == lut[0]).all()
        assert np.array_equal(out, vu.cmap(m, vu.model_lut()))
    inf_map = rng.uniform(0, 1, (7, 9)).astype(np.float32)
    inf_map[2, 2] = np.inf
    assert np.array_equal(util.cmap(inf_map), vu.cmap(inf_map, vu.model_lut()))
    for m in (rng.uniform(0, 1, (13, 19)), rng.uniform(-5, -1, (4, 4)), rng.normal(0, 100, (33, 17)),
              np.array([[0.0, 1e-7]]), np.array([[1.25, 2.75]])):
        m = m.astype(np.float32)
        out = util.cmap(m)
        at = np.unravel_index(np.argmax(m), m.shape)
        assert (out[at] == lut[255]).all() and (out[np.unravel_index(np.argmin(m), m.shape)] == lut[0]).all()
        assert np.array_equal(out, vu.cmap(m, vu.model_lut()))
    with pytest.raises(ValueError):
        util.cmap(np.zeros((4, 4), np.float32), np.zeros((256, 4), np.uint8))


def test_hot_lut():
    from pixel_nerf_multiscale_amd import util
    lut = util.hot_lut()
    assert isinstance(lut, np.ndarray) and lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [0, 0, 0] and lut[255].tolist() == [255, 255, 255]
    assert (np.diff(lut.astype(np.int32), axis=0) >= 0).all()
    assert np.array_equal(lut, vu.model_lut())
    assert "parity unpinned" in util.hot_lut.__doc__.lower()
    # red saturates first, blue starts last: RGB order
    assert lut[96].tolist()[0] == 255 and lut[95, 1] == 0 and lut[191, 2] == 0 and lut[192, 2] > 0


def test_byte_over_255_is_the_float64_quotient_rounded():
    b = np.arange(256)
    f = b.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(f, (b / 255).astype(np.float32))
    assert np.array_equal(vu.to_u8(f), b.astype(np.uint8))                   # panel_u8 of a colour-map tile is the LUT byte


def _panel_case(W, H, NS, n_pass, K, seed):
    rng = np.random.default_rng(seed)
    NV = NS + 2
    images = rng.uniform(-1, 1, (NV, 3, H, W)).astype(np.float32)
    passes = []
    for _ in range(n_pass):
        w = rng.uniform(0, 1, (H * W, K)).astype(np.float32)
        w /= np.float32(1.3) * w.sum(-1, keepdims=True)
        passes.append((rng.uniform(-0.1, 1.1, (H * W, 3)).astype(np.float32), rng.uniform(1.25, 2.75, H * W).astype(np.float32), w))
    src = sorted(rng.choice(NV, NS, replace=False).tolist())
    gt = [v for v in range(NV) if v not in src][-1]
    return images, src, gt, passes


@pytest.mark.parametrize("W,H,NS,n_pass", [(19, 13, 1, 2), (5, 4, 3, 1), (16, 16, 2, 2)])
def test_panel_reassembly(W, H, NS, n_pass):
    """The reference's own assembly (np.hstack of the tiles, np.vstack of the rows, train.py:497-526) equals the model's
    panel, which is filled by address: the layout is right before any kernel runs."""
    images, src, gt, passes = _panel_case(W, H, NS, n_pass, 7, seed=W * H + NS)
    lut = vu.model_lut()
    m = vu.panel_model(images, src, gt, passes, lut)
    rows, alphas = vu.pieces(images, src, gt, passes, lut, W, H)
    vis = np.hstack(rows[0])
    if n_pass == 2:
        vis = np.vstack((vis, np.hstack(rows[1])))
    assert m["panel"].shape == (n_pass * H, (NS + 4) * W, 3) and m["panel"].dtype == np.float32
    assert np.array_equal(vis.view(np.int32), m["panel"].view(np.int32))
    assert m["panel_u8"].shape == m["panel"].shape and m["alpha"].shape == (n_pass, H, W) and m["stats"].shape == (n_pass, 6)
    for p in range(n_pass):
        for col, src_map in ((NS + 1, passes[p][1].reshape(H, W)), (NS + 3, alphas[p])):
            assert np.array_equal(m["panel_u8"][p * H:(p + 1) * H, col * W:(col + 1) * W], vu.cmap(src_map, lut))
        assert np.array_equal(m["panel"][p * H:(p + 1) * H, (NS + 2) * W:(NS + 3) * W], passes[p][0].reshape(H, W, 3))
    x = passes[-1][0].reshape(H, W, 3).astype(np.float64)
    g = vu.image_tile(images[gt]).astype(np.float64)                       # the fp32 tile, as the header says
    assert abs(m["mse"] - ((x - g) ** 2).mean()) <= 3 * H * W * 2.0 ** -52 * m["mse"]


# ------------------------------------------------------------------------------------------------------- train.py, host side
@pytest.mark.parametrize("NV", [2, 3, 5])
def test_vis_step_draws(NV):
    from pixel_nerf_multiscale_amd import train
    for k in range(1, NV):
        torch.manual_seed(100 + k); np.random.seed(100 * NV + k)
        targets, sources = set(), set()
        for _ in range(200):
            src, dest = train.draw_vis_views(NV, [k])
            src = [int(v) for v in src]
            assert len(src) == k and src == sorted(set(src)) and all(0 <= v < NV for v in src)
            assert 0 <= dest < NV and dest not in src
            targets.add(dest)
            sources.add(tuple(src))
        assert targets == set(range(NV)), (NV, k, targets)
        assert len(sources) > 1 or NV == 2 or k == NV        # the draw moves
    torch.manual_seed(1); np.random.seed(1)
    ks = {len(train.draw_vis_views(5, [1, 3])[0]) for _ in range(50)}
    assert ks == {1, 3}                                       # curr_nviews comes from the list


def test_vis_step_draws_follow_the_reference_order():
    from pixel_nerf_multiscale_amd import train
    torch.manual_seed(9); np.random.seed(9)
    src, dest = train.draw_vis_views(5, [2, 3])
    torch.manual_seed(9); np.random.seed(9)
    k = [2, 3][torch.randint(0, 2, (1,)).item()]
    want_src = np.sort(np.random.choice(5, k, replace=False))
    want_dest = np.random.randint(0, 5 - k)
    for vs in range(k):
        want_dest += want_dest >= want_src[vs]
    assert np.array_equal(src, want_src) and dest == int(want_dest)


def test_vis_step_refusals():
    from pixel_nerf_multiscale_amd import train

    class Net:
        poses = torch.zeros(1)

    data = {"images": torch.zeros(2, 10, 3, 4, 4), "poses": torch.eye(4).expand(2, 10, 4, 4), "focal": torch.tensor([5.0, 5.0])}
    with pytest.raises(ValueError, match="source views"):
        train.vis_step(Net(), None, None, data, nviews=[9], z_near=1.0, z_far=2.0, idx=0)          # more than the panel holds
    for k in (3, 4):
        small = {k_: (v[:, :3] if k_ != "focal" else v) for k_, v in data.items()}
        with pytest.raises(ValueError, match="target view"):
            train.vis_step(Net(), None, None, small, nviews=[k], z_near=1.0, z_far=2.0, idx=1)     # curr_nviews >= NV
    with pytest.raises(ValueError, match="out"):
        train.vis_step(Net(), None, None, data, nviews=[1], z_near=1.0, z_far=2.0, out="png")
    assert train.vis_step(Net(), None, None, {"poses": data["poses"]}, nviews=[1], z_near=1.0, z_far=2.0) == {}


class _ModeStub(torch.nn.Module):
    pass


def test_validate_with_a_stub_eval_step(monkeypatch):
    from pixel_nerf_multiscale_amd import train
    seen = []

    def stub(net, renderer, render_par, data, **kw):
        assert not net.training and kw == {"nviews": [1]}
        seen.append(data["id"])
        return {"rc": torch.tensor(9.0), "t": torch.tensor(data["t"], dtype=torch.float32)}

    monkeypatch.setattr(train, "eval_step", stub)
    net, rend = _ModeStub(), _ModeStub()
    loader = [{"images": 0, "id": 0, "t": 0.25}, None, {"id": 1, "t": 100.0}, {}, {"images": 0, "id": 2, "t": 1.0},
              {"images": 0, "id": 3, "t": 0.5}]
    for mode in (True, False):
        seen.clear()
        net.train(mode)
        got = train.validate(net, rend, None, loader, nviews=[1])
        assert isinstance(got, float) and got == (0.25 + 1.0 + 0.5) / 3 and seen == [0, 2, 3]
        assert net.training is mode
    assert train.validate(net, rend, None, [None, {}, {"id": 5, "t": 1.0}], nviews=[1]) == float("inf")
    assert train.validate(net, rend, None, [], nviews=[1]) == float("inf")


def test_eval_step_restores_the_renderer_mode_and_records_no_graph(monkeypatch):
    from pixel_nerf_multiscale_amd import train
    calls = []

    def fake_calc_losses(net, render_par, data, **kw):
        calls.append((kw, torch.is_grad_enabled(), render_par.training))
        return (torch.tensor(1.0), {"t": torch.tensor(0.5)}) if "images" in data else {}

    monkeypatch.setattr(train, "calc_losses", fake_calc_losses)
    rend = _ModeStub()
    for mode in (True, False):
        rend.train(mode)
        d = train.eval_step(None, rend, rend, {"images": 0}, nviews=[2], ray_batch_size=8)
        assert sorted(d) == ["t"] and rend.training is mode
        kw, grad, training = calls[-1]
        assert kw == {"is_train": False, "nviews": [2], "ray_batch_size": 8} and grad is False and training is False
    assert train.eval_step(None, rend, rend, {}, nviews=[2]) == {}


def test_wrappers_check_shapes_on_the_host():
    from pixel_nerf_multiscale_amd import util
    with pytest.raises(ValueError):
        util.cmap_device(torch.zeros(4, 4, 3))                               # not (H, W)
    with pytest.raises(ValueError):
        util.cmap_device(torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        util.vis_panel(torch.zeros(3, 4, 8, 8), [0], 1, [(None, None, None)])     # not (NV, 3, H, W)
    with pytest.raises(ValueError):
        util.vis_panel(torch.zeros(12, 3, 8, 8), list(range(9)), 10, [(None, None, None)])
    with pytest.raises(ValueError):
        util.vis_panel(torch.zeros(3, 3, 8, 8), [0], 1, [])
