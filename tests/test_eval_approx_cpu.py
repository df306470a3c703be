"""Approximate evaluation, host side: the two entry points are declared and exported, every argument check of pnr_eval_frames
(all made before any launch, so they run without a GPU), the workspace size, the view draws of evalio.draw_approx_views against
the reference's own statements (tests/golden/eval_approx_views.npz, tools/gen_golden_eval_approx.py), and what
evalio.evaluate_approx refuses before it looks at the network."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -4


def test_both_prototypes_are_declared_bound_and_exported():
    from pixel_nerf_multiscale_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("pnr_eval_frames", "pnr_eval_frames_workspace_bytes"):
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    version = hdr[hdr.index("#define PNR_VERSION"):hdr.index("#define PNR_MAX_LEVELS")]
    assert "PNR_VERSION 102" in version and "pnr_eval_frames" in version and N.lib.pnr_version() == 102


def test_eval_frames_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p = 64          # a non-NULL value: the checks below return before anything dereferences or launches
    big = 1 << 40

    def ef(rgb=p, rs=0, fs=0, gt=p, F=2, W=16, H=16, clamp=0, m=p, ws=p, ws_bytes=big):
        return L.pnr_eval_frames(rgb, rs, fs, gt, F, W, H, clamp, m, ws, ws_bytes, None)

    for name in ("rgb", "gt", "m", "ws"):
        assert ef(**{name: None}) == E_NULL, name
    assert ef(F=0) == E_SHAPE and ef(F=-1) == E_SHAPE
    for W, H in ((6, 16), (16, 6), (6, 6), (0, 16), (16, -1)):     # below the 7 x 7 window
        assert ef(W=W, H=H) == E_SHAPE
    assert ef(F=1, W=65536, H=32768) == E_SHAPE                     # W * H = 2^31
    assert ef(F=1, W=46341, H=46341) == E_SHAPE                     # just above 2^31
    assert ef(F=(1 << 23) + 1) == E_SHAPE                           # F x tiles above 2^23 workgroups
    assert ef(F=(1 << 15) + 1, W=256, H=256) == E_SHAPE             # 256 tiles per frame
    assert ef(F=3, W=32768, H=32768) == E_SHAPE                     # 2^22 tiles per frame: two frames are the limit
    assert ef(rs=1) == E_SHAPE and ef(rs=2) == E_SHAPE and ef(rs=-4) == E_SHAPE
    assert ef(fs=16 * 16 * 3 - 1) == E_SHAPE and ef(rs=4, fs=16 * 16 * 4 - 1) == E_SHAPE and ef(fs=-1) == E_SHAPE
    need = L.pnr_eval_frames_workspace_bytes(2, 16, 16)
    assert ef(ws_bytes=need - 1) == E_WORKSPACE and ef(ws_bytes=0) == E_WORKSPACE
    assert ef(F=3, W=300, H=400, ws_bytes=L.pnr_eval_frames_workspace_bytes(2, 300, 400)) == E_WORKSPACE
    with pytest.raises(ValueError):
        N.check(ef(ws_bytes=0), "pnr_eval_frames")


def test_workspace_is_one_pair_per_frame_and_tile():
    from pixel_nerf_multiscale_amd import _native as N
    wb = N.lib.pnr_eval_frames_workspace_bytes
    for F, W, H in ((1, 7, 7), (3, 16, 16), (3, 17, 16), (2, 23, 37), (4, 128, 128), (5, 400, 300), (1 << 15, 256, 256)):
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        assert wb(F, W, H) == F * tiles * 16, (F, W, H)
        assert F > 1 or wb(F, W, H) == N.lib.pnr_eval_frame_workspace_bytes(W, H)
    for F, W, H in ((0, 16, 16), (-2, 16, 16), (1, 6, 16), (1, 16, 6), (1, 0, 16), (1, 65536, 32768), ((1 << 15) + 1, 256, 256),
                    ((1 << 23) + 1, 7, 7)):
        assert wb(F, W, H) == 0, (F, W, H)


def test_view_draws_are_the_references():
    from pixel_nerf_multiscale_amd import evalio
    g = np.load(os.path.join(ROOT, "tests", "golden", "eval_approx_views.npz"))
    cases = g["cases"]
    assert len(cases) >= 4
    kinds = set()
    for i, (SB, NV, seed, n_batches) in enumerate(cases.tolist()):
        source = g[f"case{i}__source"]
        arg = " ".join(str(v) for v in source.tolist())                    # as --source gives it
        kinds.add("random" if source.tolist() == [-1] else "one" if len(source) == 1 else "many")
        if NV - len(source) == 1:
            kinds.add("one_left")
        for form in (arg, source.tolist(), torch.from_numpy(source)):
            torch.random.manual_seed(seed)
            for b in range(n_batches):                                     # consecutive batches after ONE manual_seed
                src_view, dest_view = evalio.draw_approx_views(SB, NV, form)
                assert src_view.dtype == torch.int64 and dest_view.dtype == torch.int64
                assert tuple(src_view.shape) == (SB, len(source)) and tuple(dest_view.shape) == (SB, 1)
                assert np.array_equal(src_view.numpy(), g[f"case{i}__src_view"][b]), (i, b)
                assert np.array_equal(dest_view.numpy(), g[f"case{i}__dest_view"][b]), (i, b)
                assert not (dest_view == src_view).any() and 0 <= int(dest_view.min()) and int(dest_view.max()) < NV
    assert kinds == {"random", "one", "many", "one_left"}
    assert g["case0__dest_view"].reshape(2, 4).tolist() == [[1, 1, 1, 4], [4, 3, 1, 1]]     # seed 1234, SB 4, NV 6, "0 2 5"


@pytest.mark.parametrize("SB,NV,source", [(2, 6, "2 0 5"), (2, 6, "0 2 2"),      # not strictly increasing
                                           (2, 6, "0 6"), (2, 6, "64"),          # a source index >= NV
                                           (2, 3, "0 1 2"), (2, 1, "-1")])       # NV - NS < 1
def test_view_draws_refuse_what_the_reference_leaves_undefined(SB, NV, source):
    from pixel_nerf_multiscale_amd import evalio
    torch.random.manual_seed(3)
    state = torch.random.get_rng_state()
    with pytest.raises(ValueError):
        evalio.draw_approx_views(SB, NV, source)
    assert torch.equal(torch.random.get_rng_state(), state)                  # refused before anything is drawn


class _Loader(list):
    class dataset:
        z_near, z_far = 1.25, 2.75


def test_evaluate_approx_refuses_before_touching_the_network():
    from pixel_nerf_multiscale_amd import evalio
    batch = dict(images=torch.zeros(2, 4, 3, 6, 16), poses=torch.eye(4).expand(2, 4, 4, 4), focal=torch.tensor([20.0, 20.0]))
    for metrics in ("host", "device"):
        with pytest.raises(ValueError, match="7 x 7"):
            evalio.evaluate_approx(None, None, _Loader([batch]), source="0", metrics=metrics, verbose=False)
    with pytest.raises(ValueError, match="metrics"):
        evalio.evaluate_approx(None, None, _Loader([batch]), source="0", metrics="gpu")
    assert evalio.evaluate_approx(None, None, _Loader([]), source="0", verbose=False) == (0.0, 0.0, 0)


def test_eval_frames_wrapper_checks_shapes_on_the_host():
    from pixel_nerf_multiscale_amd import util
    with pytest.raises(ValueError):
        util.eval_frames(torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 3))      # gt is not (F, 3, H, W)
    with pytest.raises(ValueError):
        util.eval_frames(torch.zeros(3, 8, 8, 3), torch.zeros(2, 3, 8, 8))      # another number of frames
    with pytest.raises(ValueError):
        util.eval_frames(torch.zeros(8, 8, 3), torch.zeros(1, 3, 8, 8)[0:0])    # no frame
