"""Training back end, host side: the fp64 model of its arithmetic (optim_util, written from include/pnr.h) against torch's own
Adam and clip_grad_norm_ on the CPU, with mutations that show the comparison can tell; pnr_optim_plan (pure host code); the
argument checks of pnr_adam_step (all made before any launch); the exports; DeviceAdam's refusals.

Bounds of the model-vs-torch comparison, from the fp32 format (u = 2^-24, one rounding's relative error) — torch's Adam is a
correctly rounded fp32 sequence, so after k steps
  p   k * (u * max|p| + lr * 1e-5)        the last rounding of p each step, plus the update lr * m^ / (sqrt(v^) + eps), |.| <~ lr,
                                          whose ~10 roundings and the fp32 norm behind clip_coef stay below 1e-5 relative
  m   30 * 2u * gmax                      three roundings per step and torch's fp32 norm (a few u more) on terms <= gmax, the
                                          largest clipped |g| so far; the errors decay with beta1: sum 0.9^j < 10
  v   120 * 2u * gmax^2                   the same on g^2, decaying with beta2: 40 steps, no decay to speak of
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import optim_util as ou
from pixel_nerf_multiscale_amd import _native as N            # the whole file needs the feature: it fails to import without it
from pixel_nerf_multiscale_amd.optim import DeviceAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -4, -5
U = 2.0 ** -24
LR, BETAS, EPS, MAX_NORM, STEPS = ou.LR, ou.BETAS, ou.EPS, ou.MAX_NORM, ou.STEPS
SKIP_AT = 5            # the step (0-based) whose gradient carries an Inf in the runs that test the skip


# ------------------------------------------------------------------------------------------------- model vs torch
@pytest.fixture(scope="module")
def torch_run():
    return ou.torch_reference()


def test_model_matches_torch_adam_and_clip(torch_run):
    params, grads, err, snaps = torch_run
    for s in snaps:
        assert abs(s["torch_norm"] - s["norm"]) <= 1e-5 * s["norm"]
    for k in (1, 2, 10, STEPS):
        e, s = err[k - 1], snaps[k - 1]
        bound = {"p": k * (U * s["pmax"] + LR * 1e-5), "m": 30 * 2 * U * s["gmax"], "v": 120 * 2 * U * s["gmax"] ** 2}
        print(f"step {k}: max |torch fp32 - model|  p {e['p']:.3e} (bound {bound['p']:.3e})  m {e['m']:.3e} ({bound['m']:.3e})"
              f"  v {e['v']:.3e} ({bound['v']:.3e})")
    for k in range(1, STEPS + 1):
        e, s = err[k - 1], snaps[k - 1]
        assert e["p"] <= k * (U * s["pmax"] + LR * 1e-5), k
        assert e["m"] <= 30 * 2 * U * s["gmax"], k
        assert e["v"] <= 120 * 2 * U * s["gmax"] ** 2, k


@pytest.mark.parametrize("mutation", ou.MUTATIONS)
def test_a_mutated_model_lands_outside_torchs_error(torch_run, mutation):
    """Each rule of the arithmetic, broken alone, moves p, m or v at least 10x further from the model than torch's fp32 run
    is at the same step — so a kernel held to 2x torch's error cannot carry that mutation.  The skip rule needs a skipped
    step: both models get an Inf in step SKIP_AT's gradient (torch's run, which has no such step, is the reference for the
    error of the steps around it)."""
    params, grads, err, snaps = torch_run
    grads = [list(G) for G in grads]
    skip = mutation == "step_counts_skips"
    if skip:
        bad = grads[SKIP_AT][-1].copy()
        bad.reshape(-1)[-1] = np.inf
        grads[SKIP_AT][-1] = bad
    good = ou.AdamModel(params, LR, BETAS, EPS, MAX_NORM)
    mut = ou.AdamModel(params, LR, BETAS, EPS, MAX_NORM, mutation=mutation)
    best, ti = 0.0, 0
    for k, G in enumerate(grads):
        good.step(G)
        mut.step(G)
        if skip and k == SKIP_AT:
            assert good.t == SKIP_AT and mut.t == SKIP_AT + 1 and good.skipped == mut.skipped == 1
            continue
        e = err[ti]          # torch's error after as many APPLIED steps
        ti += 1
        for q, a, b in (("p", mut.p, good.p), ("m", mut.m, good.m), ("v", mut.v, good.v)):
            best = max(best, ou.worst(a, b) / e[q])
    print(f"{mutation}: the mutated model is up to {best:.3g} x torch's own error away from the model")
    assert best >= 10.0


def test_model_skip_and_scaler_rules():
    params, grads = ou.trajectory_inputs(8, seed=3)
    sc = dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    a = ou.AdamModel(params, LR, BETAS, EPS, 1.0, scaler=sc)
    scaled = lambda G, s: [(g * np.float32(s)).astype(np.float32) for g in G]
    for k in range(3):
        assert float(a.scale) == 1024.0 and a.tracker == k
        a.step(scaled(grads[k], a.scale))
    assert float(a.scale) == 2048.0 and a.tracker == 0 and a.t == 3
    before = [x.copy() for x in a.p + a.m + a.v]
    bad = scaled(grads[3], a.scale)
    bad[0].reshape(-1)[0] = np.nan
    a.step(bad)
    assert a.found_inf == 1 and a.t == 3 and a.skipped == 1 and float(a.scale) == 1024.0 and a.tracker == 0
    assert all(np.array_equal(x, y) for x, y in zip(before, a.p + a.m + a.v))
    # unscaling by a power of two is exact: the scaled run equals the plain one
    b = ou.AdamModel(params, LR, BETAS, EPS, 1.0)
    for k in range(3):
        b.step(grads[k])
    assert all(np.array_equal(x, y) for x, y in zip(b.p + b.m + b.v, a.p + a.m + a.v))
    # a None gradient leaves its tensor alone and out of the norm
    c = ou.AdamModel(params, LR, BETAS, EPS, 1.0)
    G = list(grads[0])
    G[4] = None
    c.step(G)
    assert np.array_equal(c.p[4], np.asarray(params[4], dtype=np.float64)) and not c.m[4].any()
    want = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for i, g in enumerate(grads[0]) if i != 4))
    assert abs(c.grad_norm - want) <= 1e-12 * want


# ------------------------------------------------------------------------------------------------- pnr_optim_plan
def _plan(seg_n, max_chunks=None):
    seg = np.asarray(seg_n, dtype=np.int64)
    sp = seg.ctypes.data_as(C.POINTER(C.c_int64))
    n = N.lib.pnr_optim_plan(sp, len(seg), None, 0)
    assert n >= 0
    cap = n if max_chunks is None else max_chunks
    out = (N.pnr_optim_chunk * max(cap, 1))()
    assert N.lib.pnr_optim_plan(sp, len(seg), C.addressof(out), cap) == n
    return n, [(out[i].segment, out[i].first) for i in range(min(n, cap))]


def _check_plan(seg_n):
    CH = N.lib.pnr_optim_chunk_elems()
    n, chunks = _plan(seg_n)
    assert n == sum((s + CH - 1) // CH for s in seg_n)
    seen = [np.zeros(s, dtype=np.int32) for s in seg_n]
    for seg, first in chunks:
        assert 0 <= seg < len(seg_n) and 0 <= first < seg_n[seg] and first % CH == 0
        seen[seg][first:min(first + CH, seg_n[seg])] += 1        # the slice cannot leave the segment: the kernel's min()
    assert all(bool((s == 1).all()) for s in seen)                # each element in exactly one chunk
    assert chunks == sorted(chunks) and len(set(chunks)) == len(chunks)      # ascending (segment, first)


def test_plan_covers_every_element_once():
    CH = N.lib.pnr_optim_chunk_elems()
    assert CH >= 256 and CH % 256 == 0
    _check_plan(ou.SIZES)
    _check_plan(ou.SIZES[:5] + [0] + ou.SIZES[5:])                # a length-0 segment (a tensor without a gradient)
    _check_plan([0, 0, 7, 0])
    _check_plan([3 * CH + 1])                                     # a single segment of 3 chunks + 1 element
    _check_plan([CH - 1, CH, CH + 1, 2 * CH + 1])
    assert _plan([])[0] == 0 and _plan([0])[0] == 0


def test_plan_counts_past_the_capacity_and_checks_arguments():
    CH = N.lib.pnr_optim_chunk_elems()
    n, chunks = _plan([2 * CH + 1, 5], max_chunks=2)             # counted, not written
    assert n == 4 and chunks == [(0, 0), (0, CH)]
    seg = np.asarray([4, -1], dtype=np.int64)
    sp = seg.ctypes.data_as(C.POINTER(C.c_int64))
    assert N.lib.pnr_optim_plan(sp, 2, None, 0) == E_SHAPE        # a negative length
    assert N.lib.pnr_optim_plan(sp, -1, None, 0) == E_SHAPE
    assert N.lib.pnr_optim_plan(sp, 1, None, -1) == E_SHAPE
    assert N.lib.pnr_optim_plan(None, 2, None, 0) == E_NULL


# ------------------------------------------------------------------------------------------------- pnr_adam_step
def test_adam_step_checks_arguments_without_gpu():
    L = N.lib
    p = 4096        # a non-NULL, 16-byte aligned value: every call below returns before anything is dereferenced or launched
    need = L.pnr_optim_workspace_bytes(3)

    def st(seg=p, n_seg=2, ch=p, n_ch=3, g=p, m=p, v=p, n_flat=64, scaler=None, state=p, ws=p, ws_bytes=None):
        return L.pnr_adam_step(seg, n_seg, ch, n_ch, g, m, v, n_flat, 1e-4, 0.9, 0.999, 1e-8, 1.0, scaler, state, ws,
                               need if ws_bytes is None else ws_bytes, None)

    for k in ("seg", "ch", "g", "m", "v", "state", "ws"):
        assert st(**{k: None}) == E_NULL, k
    assert st(n_seg=-1) == E_SHAPE and st(n_ch=-1) == E_SHAPE and st(n_flat=-1) == E_SHAPE
    assert st(n_ch=1 << 31) == E_SHAPE
    assert st(n_seg=0) == E_SHAPE and st(n_flat=0) == E_SHAPE    # chunks with nothing to point into
    assert st(ws_bytes=need - 1) == E_WORKSPACE and st(ws_bytes=0) == E_WORKSPACE
    for k in ("g", "m", "v", "ws"):
        assert st(**{k: p + 4}) == E_ALIGN and st(**{k: p + 8}) == E_ALIGN, k
    for k in ("seg", "ch", "state"):
        assert st(**{k: p + 4}) == E_ALIGN, k
    bad = N.pnr_optim_scaler(2.0, 0.5, 0, 0)
    assert st(scaler=C.byref(bad)) == E_SHAPE                     # growth_interval < 1
    assert st(n_ch=0, seg=None, ch=None, g=None, m=None, v=None, ws=None, ws_bytes=0) == 0      # no gradient anywhere: no launch
    assert st(n_ch=0, state=None) == E_NULL
    with pytest.raises(ValueError):
        N.check(st(ws_bytes=0), "pnr_adam_step")


def test_workspace_bytes():
    wb = N.lib.pnr_optim_workspace_bytes
    assert wb(0) == 0 and wb(-1) == 0 and wb(1 << 31) == 0
    for n in (1, 2, 3, 4, 5, 255, 256, 257, 3700):
        assert wb(n) >= 12 * n and wb(n) % 16 == 0 and wb(n) <= 12 * n + 32     # one double and one flag per chunk
    sizes = [wb(n) for n in range(1, 40)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


def test_exports_are_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("pnr_optim_chunk_elems", "pnr_optim_plan", "pnr_optim_workspace_bytes", "pnr_adam_step"):
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    assert "optim.hip" in __import__("pixel_nerf_multiscale_amd.build_native", fromlist=["SOURCES"]).SOURCES
    assert N.lib.pnr_version() == 102
    # the record the header defines, field for field
    S = N.pnr_optim_state
    assert C.sizeof(S) == 56 and C.sizeof(N.pnr_optim_segment) == 24 and C.sizeof(N.pnr_optim_chunk) == 16
    offs = {f: getattr(S, f).offset for f, _ in S._fields_}
    assert offs == {"grad_norm": 0, "clip_coef": 8, "scale": 12, "inv_scale": 16, "found_inf": 20, "growth_tracker": 24,
                    "reserved0": 28, "step": 32, "skipped": 40, "step_size": 48, "rsqrt_bc2": 52}
    from pixel_nerf_multiscale_amd import optim
    assert {k: v[0] for k, v in optim._STATE.items()} == {k: v for k, v in offs.items() if k != "reserved0"}
    for f in ("grad_norm", "clip_coef", "scale", "inv_scale", "found_inf", "growth_tracker", "step", "skipped"):
        assert re.search(r"\b" + f + r"\b", hdr), f


# ------------------------------------------------------------------------------------------------- DeviceAdam, host side
def test_device_adam_refuses_what_it_cannot_update():
    from pixel_nerf_multiscale_amd import train
    assert callable(train.train_step)
    ok = lambda *s: torch.nn.Parameter(torch.zeros(*s))
    with pytest.raises(TypeError, match="fp32"):
        DeviceAdam([ok(4), torch.nn.Parameter(torch.zeros(4, dtype=torch.float16))])
    with pytest.raises(ValueError, match="contiguous"):
        DeviceAdam([ok(4), torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError, match="one device"):
        DeviceAdam([ok(4), torch.nn.Parameter(torch.zeros(4, device="meta"))])
    with pytest.raises(ValueError, match="ONE param group"):
        DeviceAdam([{"params": [ok(4)]}, {"params": [ok(3)], "lr": 1e-3}])
    with pytest.raises(ValueError):
        DeviceAdam([])
    with pytest.raises(ValueError, match="scaler"):
        DeviceAdam([ok(4)], scaler=dict(init_scale=2.0, growth=2.0))
    with pytest.raises(ValueError):
        DeviceAdam([ok(4)], betas=(1.0, 0.999))
    with pytest.raises(RuntimeError, match="HIP device"):        # everything else in order: there is no host path
        DeviceAdam([ok(4), ok(3, 5)])
