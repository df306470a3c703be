"""Evaluation back end, host side: the two entry points are declared and exported, every argument check of pnr_eval_frame
(all made before any launch, so they run without a GPU), the workspace size, and evaluate()'s `metrics` switch."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -4


def test_both_prototypes_are_declared_bound_and_exported():
    from pixel_nerf_multiscale_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("pnr_eval_frame", "pnr_eval_frame_workspace_bytes"):
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    assert "eval.hip" in __import__("pixel_nerf_multiscale_amd.build_native", fromlist=["SOURCES"]).SOURCES


def test_eval_frame_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p = 64          # a non-NULL value: the checks below return before anything dereferences or launches
    big = 1 << 20

    def ef(rgb=p, rs=0, depth=None, ds=0, gt=None, W=16, H=16, zn=0.5, zf=2.0, u8=None, cmp=None, dn=None, m=None, ws=None,
           ws_bytes=0):
        return L.pnr_eval_frame(rgb, rs, depth, ds, gt, W, H, zn, zf, u8, cmp, dn, m, ws, ws_bytes, None)

    assert ef(rgb=None, u8=p) == E_NULL
    assert ef(cmp=p) == E_NULL                                      # compare strip without ground truth
    assert ef(m=p, ws=p, ws_bytes=big) == E_NULL                    # metrics without ground truth
    assert ef(dn=p) == E_NULL                                       # normalised depth without depth
    assert ef(gt=p, m=p, ws=None, ws_bytes=big) == E_NULL           # metrics without a workspace
    assert ef(u8=p, W=0) == E_SHAPE and ef(u8=p, H=0) == E_SHAPE and ef(u8=p, W=-3) == E_SHAPE
    assert ef(u8=p, W=65536, H=32768) == E_SHAPE                    # W * H = 2^31
    assert ef(u8=p, W=46341, H=46341) == E_SHAPE                    # just above 2^31
    for W, H in ((6, 16), (16, 6), (6, 6)):                         # below the 7 x 7 window
        assert ef(gt=p, m=p, ws=p, ws_bytes=big, W=W, H=H) == E_SHAPE
    assert ef(depth=p, dn=p, zn=1.25, zf=1.25) == E_SHAPE           # z_far == z_near
    assert ef(u8=p, rs=2) == E_SHAPE and ef(depth=p, dn=p, ds=-1) == E_SHAPE     # a stride below the record's own width
    need = L.pnr_eval_frame_workspace_bytes(16, 16)
    assert ef(gt=p, m=p, ws=p, ws_bytes=need - 1) == E_WORKSPACE
    assert ef(gt=p, m=p, ws=p, ws_bytes=0, W=300, H=400) == E_WORKSPACE
    assert ef() == 0                                                # nothing asked for: no launch
    with pytest.raises(ValueError):
        N.check(ef(gt=p, m=p, ws=p, ws_bytes=0), "pnr_eval_frame")


def test_workspace_bytes_grow_with_the_tile_count():
    from pixel_nerf_multiscale_amd import _native as N
    wb = N.lib.pnr_eval_frame_workspace_bytes
    assert wb(7, 7) > 0
    assert wb(7, 7) == wb(16, 16)                                   # one tile either way
    sizes = [wb(n, n) for n in (7, 16, 17, 32, 33, 64, 128, 129, 400)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] < sizes[2] < sizes[4] < sizes[-1]
    assert wb(17, 16) == wb(16, 17) == 2 * wb(16, 16) and wb(400, 300) == wb(300, 400)
    assert wb(400, 300) >= 2 * 8 * 25 * 19                          # one (squared error, SSIM) pair of doubles per 16 x 16 tile
    assert wb(0, 16) == 0 and wb(16, -1) == 0 and wb(65536, 32768) == 0


def test_evaluate_rejects_an_unknown_back_end():
    from pixel_nerf_multiscale_amd import evalio
    with pytest.raises(ValueError, match="metrics"):
        evalio.evaluate(None, None, [], "", metrics="gpu")           # refused before the network is looked at


def test_eval_frame_wrapper_checks_shapes_on_the_host():
    import torch
    from pixel_nerf_multiscale_amd import util
    with pytest.raises(ValueError):
        util.eval_frame(torch.zeros(8, 8, 4))                        # not (H, W, 3)
    with pytest.raises(ValueError):
        util.eval_frame(torch.zeros(8, 8, 3), want_metrics=True)     # metrics without ground truth
    with pytest.raises(ValueError):
        util.eval_frame(torch.zeros(8, 8, 3), want_metrics=False, want_depth=True)   # depth output without depth
