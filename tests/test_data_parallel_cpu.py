"""The data-parallel training step without a GPU: the three entry points it adds (pnr_train_draw_at, pnr_color_jitter_plan_at,
pnr_adam_step_div) are declared, bound and built and refuse bad arguments before any launch; the pure helpers that cut a global
batch, an epoch and the validation set over the ranks; the ValueErrors of obj_base under host draws."""
import ctypes
import os
import re
import types

import pytest
import torch

from pixel_nerf_multiscale_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -4
I64_MAX = (1 << 63) - 1


def test_the_new_entry_points_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("pnr_train_draw_at", "pnr_color_jitter_plan_at", "pnr_adam_step_div"):
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    assert N.lib.pnr_version() == 102                     # added without a bump, and named in the version comment
    comment = hdr[hdr.index("#define PNR_VERSION"):hdr.index("#define PNR_MAX_LEVELS")]
    for name in ("pnr_train_draw_at", "pnr_color_jitter_plan_at", "pnr_adam_step_div"):
        assert name in comment, name


def test_train_draw_at_refuses_a_bad_object_base():
    p = 64          # a non-NULL value: every call below returns before anything is dereferenced or launched

    def td(obj_base, SB=2, NV=2, W=4, H=4, B=8, NS=1, pix=p, views=p):
        return N.lib.pnr_train_draw_at(None, SB, NV, W, H, B, NS, 7, obj_base, pix, views, None)

    assert td(-1) == E_SHAPE and td(-(1 << 63)) == E_SHAPE
    assert td(I64_MAX) == E_SHAPE and td(I64_MAX - 1) == E_SHAPE             # obj_base + SB leaves int64
    assert td(I64_MAX // 8) == E_SHAPE                                        # (obj_base + SB) * B leaves int64
    assert td(I64_MAX // 8 - 1, B=0, NS=0, pix=None, views=None) == 0         # no pixel counter to overflow; nothing to launch
    assert td(0, B=0, NS=0, pix=None, views=None) == 0 and td(5, B=0, NS=0, pix=None, views=None) == 0
    # the checks of pnr_train_draw come with it
    assert td(0, pix=None) == E_NULL and td(3, views=None) == E_NULL and td(3, SB=0) == E_SHAPE and td(3, NS=3) == E_SHAPE


def test_color_jitter_plan_at_refuses_a_bad_object_base():
    p = 64
    ranges = (ctypes.c_float * 4)(0.4, 0.4, 0.4, 0.1)

    def plan(obj_base, SB=2, ws_bytes=0):
        return N.lib.pnr_color_jitter_plan_at(p, SB, 3, 8, 6, 3, ranges, 7, obj_base, p, p, ws_bytes, None)

    assert plan(-1) == E_SHAPE and plan(I64_MAX) == E_SHAPE and plan(I64_MAX - 1) == E_SHAPE
    # a good base passes that check and reaches the next one (no workspace bytes), still before any launch
    assert plan(0) == E_WORKSPACE and plan(7) == E_WORKSPACE and plan(I64_MAX - 2) == E_WORKSPACE
    assert plan(7, SB=0) == E_SHAPE


def test_adam_step_div_refuses_a_bad_divisor():
    L = N.lib
    p = 4096
    need = L.pnr_optim_workspace_bytes(3)

    def st(grad_div, ws_bytes=need, state=p):
        return L.pnr_adam_step_div(p, 2, p, 3, p, p, p, 64, 1e-4, 0.9, 0.999, 1e-8, 1.0, None, grad_div, state, p, ws_bytes, None)

    assert st(0) == E_SHAPE and st(-1) == E_SHAPE and st(-(1 << 31)) == E_SHAPE
    assert st(0, state=None) == E_SHAPE                                       # the divisor is looked at first
    for div in (1, 2, 3, 8):                                                  # a good divisor reaches pnr_adam_step's checks
        assert st(div, ws_bytes=need - 1) == E_WORKSPACE and st(div, state=None) == E_NULL


# ------------------------------------------------------------------------------------------------------------ the helpers
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_rank_slices_tile_the_global_batch(world):
    from pixel_nerf_multiscale_amd.trainer import rank_slice
    for batch_size in (world, 2 * world, 12):
        seen = []
        for rank in range(world):
            first, m = rank_slice(batch_size, world, rank)
            assert m == batch_size // world and first == rank * m
            seen.extend(range(first, first + m))
        assert seen == list(range(batch_size))                                # disjoint, and the union in rank order is the batch
    if world > 1:
        with pytest.raises(ValueError, match="does not divide"):
            rank_slice(world + 1, world, 0)
    for bad_rank in (-1, world):
        with pytest.raises(ValueError):
            rank_slice(12, world, bad_rank)


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_rank_samplers_union_is_the_epoch_permutation(world):
    from pixel_nerf_multiscale_amd.trainer import epoch_permutation, rank_epoch_order, rank_slice
    for n, batch_size in ((24, 12), (25, 12), (12, 12), (11, 12)):
        order = epoch_permutation(n, seed=5, epoch=3).tolist()
        per_rank = [rank_epoch_order(order, batch_size, world, r) for r in range(world)]
        m = rank_slice(batch_size, world, 0)[1]
        n_batches = n // batch_size
        assert all(len(p) == n_batches * m for p in per_rank)
        rebuilt = []
        for b in range(n_batches):                                            # global batch b: the ranks' b-th shares, in rank order
            for p in per_rank:
                rebuilt.extend(p[b * m:(b + 1) * m])
        assert rebuilt == order[:n_batches * batch_size]                      # drop_last, as one process does
        flat = [i for p in per_rank for i in p]
        assert len(set(flat)) == len(flat)                                    # no object twice
        if n % batch_size == 0:
            assert sorted(flat) == list(range(n))
    assert rank_epoch_order(list(range(12)), 12, 1, 0) == list(range(12))     # one rank: the order itself


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_validation_batches_go_round_the_ranks(world):
    from pixel_nerf_multiscale_amd.trainer import rank_val_batches
    for n, bs in ((0, 4), (1, 4), (7, 4), (8, 4), (9, 2)):
        whole = [list(range(i, min(i + bs, n))) for i in range(0, n, bs)]
        per_rank = [rank_val_batches(n, bs, world, r) for r in range(world)]
        for i, b in enumerate(whole):
            assert per_rank[i % world][i // world] == b
        assert sum(len(p) for p in per_rank) == len(whole)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_obj_base_needs_device_draws():
    from pixel_nerf_multiscale_amd import train
    data = {"images": torch.zeros(1, 2, 3, 4, 4), "poses": torch.zeros(1, 2, 4, 4), "focal": torch.ones(1)}
    kw = dict(ray_batch_size=4, nviews=[1], z_near=0.1, z_far=1.0)
    with pytest.raises(ValueError, match="obj_base"):
        train.make_batch(data, "cpu", obj_base=1, **kw)                       # host draws are the default
    with pytest.raises(ValueError, match="obj_base"):
        train.make_batch(data, "cpu", draws="host", obj_base=2, **kw)
    with pytest.raises(ValueError, match="obj_base"):
        train.make_batch(data, "cpu", draws="device", seed=1, obj_base=-1, **kw)
    net = types.SimpleNamespace(poses=torch.zeros(1))
    with pytest.raises(ValueError, match="obj_base"):
        train.calc_losses(net, None, data, loss=None, obj_base=1, **kw)
    with pytest.raises(ValueError, match="obj_base"):
        train.train_step(net, None, data, _NoOptim(), loss=None, obj_base=1, **kw)


class _NoOptim:
    def zero_grad(self):
        pass


def test_util_refuses_a_negative_obj_base():
    from pixel_nerf_multiscale_amd import util
    for bad in (-1, 1 << 63):
        with pytest.raises(ValueError, match="obj_base"):
            util.train_draw(None, 1, 2, 4, 4, 8, 1, 7, obj_base=bad)
        with pytest.raises(ValueError, match="obj_base"):
            util.color_jitter_plan(torch.zeros(1, 2, 4, 4, 3, dtype=torch.uint8), (0.4, 0.4, 0.4, 0.1), 7, obj_base=bad)


class _Data:
    z_near, z_far = 0.8, 1.8

    def __len__(self):
        return 4


def test_trainer_keeps_its_refusals_and_adds_the_data_parallel_ones(tmp_path):
    """No process group here: data_parallel=True is the loop of one process, so only what is independent of the group shows —
    the keyword exists, and a solo Trainer is rank 0 of 1 with the whole batch."""
    from pixel_nerf_multiscale_amd.trainer import Trainer
    kw = dict(name="run", checkpoints_path=str(tmp_path / "ckpt"), logs_path=str(tmp_path / "logs"), batch_size=2, ray_batch_size=8,
              nviews=[1], loss=None)
    with pytest.raises(ValueError, match="draws"):
        Trainer(torch.nn.Linear(2, 2), None, _Data(), None, data_parallel=True, draws="gpu", **kw)
    with pytest.raises(RuntimeError, match="HIP device"):                    # past every refusal: DeviceAdam has no host path
        Trainer(torch.nn.Linear(2, 2), None, _Data(), None, data_parallel=True, **kw)


# ------------------------------------------------------------------------------------------------------------ the host model
def test_the_model_with_a_base_slices_the_model_without():
    """data_parallel_util.model_draw_at against train_draw_util.model_draw: base 0 is the same draw, a slice under its base is the
    whole draw's rows, and the high counter word changes the draw."""
    import numpy as np

    import data_parallel_util as dpu
    import train_draw_util as du
    boxes = np.tile(np.array([1, 2, 9, 5], np.float32), (4, 3, 1))
    for bx in (None, boxes):
        whole = du.model_draw(bx, 4, 3, 11, 7, 5, 2, 77 + (3 << 35))
        for k, m in ((0, 4), (1, 2), (3, 1)):
            pix, order = dpu.model_draw_at(None if bx is None else bx[k:k + m], m, 3, 11, 7, 5, 2, 77 + (3 << 35), k)
            assert np.array_equal(pix, whole[0][k:k + m]) and np.array_equal(order, whole[1][k:k + m])
    a = dpu.model_draw_at(None, 1, 3, 11, 7, 64, 2, 77, 5)
    b = dpu.model_draw_at(None, 1, 3, 11, 7, 64, 2, 77, 5 + (1 << 32))
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
