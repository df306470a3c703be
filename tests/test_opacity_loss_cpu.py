"""The opacity losses without a GPU: the fp64 model of tests/opacity_loss_util.py against torch's float64 autograd on the plain
expressions (F.binary_cross_entropy on the clamped sum, and the reference's two lines), the reference's own AlphaLossNV2 as
recorded in tests/golden/alpha_loss.npz against the model, six planted mistakes that those checks must each catch, the three
entry points' refusals (all returned before any launch), and the Python layers that need no device: AlphaLossNV2's gate and
state dict, get_alpha_loss, MaskLoss's constructor, make_batch's want_mask and the keywords of calc_losses and the Trainer.

Bounds.  Model against torch fp64: 1e-12 relative — both are fp64 and differ by the association of the sums only.
Fixture: a value g passes when |g - v_ref| <= |v_ref - v64| + 2^-23 |v64| (the reference's own fp32 error plus one fp32
rounding).  For g = fp32(v64) that holds by the triangle inequality, so the fixture test also bounds the reference's own error
|v_ref - v64|, which is what makes the fixture a witness for the model: the reference adds 64 fp32 terms of one sign, each the sum
of two fp32 logs (torch's CPU log is within 1 ulp), so its value is within (2 + 2 + 6) 2^-24 relative — 16 x 2^-24 allowed; a
gradient entry is lambda / n (1 / a - 1 / (1 - a)) from two fp32 quotients and a sum, each within 2^-24 of its own size, so its
error is within 4 x 2^-24 x lambda / n (1 / a + 1 / (1 - a)) — 8 x allowed."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import mask_draw_util as mu
import opacity_loss_util as ou

E_NULL, E_SHAPE, E_ALIGN = -1, -2, -5
NAMES = ("pnr_mask_gather", "pnr_alpha_loss", "pnr_alpha_loss_bwd")


# ------------------------------------------------------------------------------------------------------------ the library
def test_exports_argtypes_and_header():
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    i32, i64, f, p = C.c_int32, C.c_int64, C.c_float, C.c_void_p
    assert N.PROTOTYPES["pnr_mask_gather"] == (i32, [p, i32, i32, i32, i32, p, i64, p, p])
    assert N.PROTOTYPES["pnr_alpha_loss"] == (i32, [p, i32, p, i32, p, i64, i32, f, f, f, f, f, p, p, p])
    assert N.PROTOTYPES["pnr_alpha_loss_bwd"] == (i32, [p, p, i64, i32, i32, i32, f, f, f, f, f, p, p, p, p])
    for name in NAMES:
        assert callable(getattr(N.lib, name)) and hasattr(N.lib._cdll, name)
    assert (N.PNR_ALPHA_NV2, N.PNR_ALPHA_OPAQUE, N.PNR_ALPHA_MASK) == (ou.NV2, ou.OPAQUE, ou.MASK) == (0, 1, 2)
    assert N.lib.pnr_version() == 102
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pnr.h")).read()
    comment = header[header.index("#define PNR_VERSION 102"):header.index("#define PNR_MAX_LEVELS")]
    for name in NAMES:
        assert name in comment and re.search(rf"int32_t {name}\(", header)
    assert "PNR_ALPHA_NV2 = 0, PNR_ALPHA_OPAQUE = 1, PNR_ALPHA_MASK = 2" in header
    assert "ALWAYS apply" in header and "unlike pnr_rgb_loss" in header        # the lambda rule is written down


def test_mask_gather_refusals_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    p = 64
    mg = lambda bits=p, SB=1, NV=2, H=3, W=5, pix=p, B=8, out=p: N.lib.pnr_mask_gather(bits, SB, NV, H, W, pix, B, out, None)
    assert mg(bits=None) == E_NULL and mg(pix=None) == E_NULL and mg(out=None) == E_NULL
    assert mg(SB=0) == E_SHAPE and mg(NV=0) == E_SHAPE and mg(H=0) == E_SHAPE and mg(W=-1) == E_SHAPE and mg(B=-1) == E_SHAPE
    assert mg(NV=2, H=32768, W=32768) == E_SHAPE and mg(SB=1 << 20, B=1 << 40) == E_SHAPE
    assert mg(bits=p + 2) == E_ALIGN and mg(out=p + 1) == E_ALIGN and mg(pix=p + 4) == E_ALIGN
    assert mg(B=0, bits=None, pix=None, out=None) == 0                       # nothing to do: no launch


def test_alpha_loss_refusals_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    p = 64

    def fwd(c=p, Kc=4, f=p, Kf=6, mask=p, n=10, mode=0, lo=0.01, hi=0.99, ca=100.0, alpha=p, losses=p):
        return N.lib.pnr_alpha_loss(c, Kc, f, Kf, mask, n, mode, 1.0, 1.0, lo, hi, ca, alpha, losses, None)

    def bwd(alpha=p, mask=p, n=10, Kc=4, Kf=6, mode=0, lo=0.01, hi=0.99, ca=100.0, d=p, dc=p, df=p):
        return N.lib.pnr_alpha_loss_bwd(alpha, mask, n, Kc, Kf, mode, 1.0, 1.0, lo, hi, ca, d, dc, df, None)

    assert fwd(c=None, f=None) == E_NULL and fwd(mode=2, mask=None) == E_NULL
    assert fwd(alpha=None) == E_NULL and fwd(losses=None) == E_NULL
    assert bwd(dc=None, df=None) == E_NULL and bwd(mode=2, mask=None) == E_NULL and bwd(alpha=None) == E_NULL
    for call in (fwd, bwd):
        assert call(Kc=0) == E_SHAPE and call(Kf=-1) == E_SHAPE and call(n=-1) == E_SHAPE and call(n=(1 << 32) + 1) == E_SHAPE
        assert call(mode=3) == E_SHAPE and call(mode=-1) == E_SHAPE
        for lo, hi in ((0.0, 0.99), (-0.1, 0.5), (0.5, 0.5), (0.6, 0.4), (0.01, 1.0), (0.01, 1.5), (float("nan"), 0.99), (0.01, float("nan"))):
            assert call(lo=lo, hi=hi) == E_SHAPE, (lo, hi)
        assert call(alpha=p + 4) == E_ALIGN and call(alpha=p + 1) == E_ALIGN
    # K of a NULL pass is not looked at; a mask is not asked for outside MASK mode
    assert fwd(c=None, Kc=0, n=-1) == E_SHAPE and fwd(f=None, Kf=0, n=-1) == E_SHAPE
    assert fwd(mode=0, mask=None, n=-1) == E_SHAPE and fwd(mode=1, mask=None, n=-1) == E_SHAPE
    assert bwd(dc=None, Kc=0, n=0) == 0 and bwd(df=None, Kf=0, n=0, d=None) == 0          # no rays: nothing to do, no launch


# ------------------------------------------------------------------------------------------------------------ model vs torch fp64
def _weights(n, K, seed):
    """(n, K) fp32 weights whose row sums cover the clamp's three regimes: below lo, inside, above hi — none near a bound."""
    rng = np.random.default_rng(seed)
    w = rng.random((n, K)).astype(np.float32)
    target = np.concatenate([rng.uniform(0.0, 0.008, n // 5), rng.uniform(0.995, 1.3, n // 5), rng.uniform(0.02, 0.98, n - 2 * (n // 5))])
    return (w / w.sum(axis=1, keepdims=True) * target[:, None]).astype(np.float32)


def _torch_loss(w, mode, lam, lo, hi, clamp_alpha, m):
    """The plain expression in float64 under autograd -> (loss, d loss / d w (n, K))."""
    w64 = torch.from_numpy(w).double().requires_grad_(True)
    a = torch.clamp(w64.sum(-1), float(lo), float(hi))
    if mode == ou.NV2:
        loss = lam * torch.clamp_min(torch.log(a) + torch.log(1.0 - a), -clamp_alpha).mean()      # reference loss.py:32-34
    elif mode == ou.OPAQUE:
        loss = lam * F.binary_cross_entropy(a, torch.ones_like(a))                               # loss.py:28-30
    else:
        loss = lam * F.binary_cross_entropy(a, torch.from_numpy(m).double())
    loss.backward()
    return float(loss.detach()), w64.grad.numpy()


def _close(got, want, rel):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= rel * np.abs(want)).all())


def _torch_check(v):
    """The model under variant v against torch fp64 for the three modes at K = 1, 3, 65, soft masks among them."""
    lo, hi = np.float32(0.01), np.float32(0.99)
    for K in (1, 3, 65):
        n = 41
        w = _weights(n, K, 10 + K)
        m = np.random.default_rng(K).choice(np.array([0.0, 0.25, 1.0], np.float32), n)
        for mode, ca in ((ou.NV2, 100.0), (ou.NV2, 3.0), (ou.OPAQUE, 0.0), (ou.MASK, 0.0)):
            want_loss, want_grad = _torch_loss(w, mode, 0.75, lo, hi, ca, m)
            got = ou.one_pass(w, mode, 0.75, lo, hi, ca, m, v=v)
            if not (_close(got["loss"], want_loss, 1e-12) and _close(np.repeat(got["grad"][:, None], K, 1), want_grad, 1e-12)):
                return False
    return True


def test_model_is_torch_fp64_autograd():
    assert _torch_check(ou.RIGHT)
    # the clamp3 rows exercise both sides of clamp_min, and none sits on it
    w = _weights(41, 3, 13)
    raw, _ = ou.terms(ou.alpha_sum(w), ou.NV2, 0.01, 0.99, 1e30)
    assert (raw < -3.0).any() and (raw > -3.0).any() and (np.abs(raw + 3.0) > 1e-3).all()


def test_alpha_sum_is_the_fp64_sum_and_the_fold_is_the_sum():
    for K in (1, 63, 64, 65, 257):
        w = np.random.default_rng(K).random((9, K)).astype(np.float32)
        a = ou.alpha_sum(w)
        assert _close(a, w.astype(np.float64).sum(axis=1), 1e-14)
        if K == 1:
            assert np.array_equal(a, w[:, 0].astype(np.float64))          # exact: the gates at the bounds rest on it
    for n in (1, 63, 1025, 4097):
        t = np.random.default_rng(n).random(n)
        assert _close(ou.fold(t), t.sum(), 1e-13)


# ------------------------------------------------------------------------------------------------------------ the fixture
def _fixture():
    d = np.load(os.path.join(gu.GOLDEN_DIR, "alpha_loss.npz"))
    names = str(d["names"]).split(",")
    cases = {}
    for name in names:
        lam, ca, init_epoch, opaque, steps = d[f"{name}__cfg"].tolist()
        cases[name] = dict(lam=lam, clamp_alpha=ca, init_epoch=int(init_epoch), opaque=bool(opaque), steps=int(steps),
                           value=d[f"{name}__value"], grad=d[f"{name}__grad"])
    return d["alpha"], cases


def _model_of_case(alpha, case, v=ou.RIGHT):
    """(value float64, grad (n,) float64) of the model for a fixture case: zeros before init_epoch."""
    if not (case["lam"] > 0.0 and case["steps"] >= case["init_epoch"]):
        return 0.0, np.zeros(alpha.shape[0])
    p = ou.one_pass(alpha[:, None], ou.OPAQUE if case["opaque"] else ou.NV2, case["lam"], ou.REF_LO, ou.REF_HI, case["clamp_alpha"], v=v)
    return p["loss"], p["grad"]


def _fixture_check(v):
    """The issue's criterion for the model under variant v, rounded to fp32, against the recorded reference and the RIGHT model."""
    alpha, cases = _fixture()
    for case in cases.values():
        v64, g64 = _model_of_case(alpha, case)
        got_v, got_g = _model_of_case(alpha, case, v)
        if not ou.fixture_criterion(np.float32(got_v), case["value"][0], v64):
            return False
        if not ou.fixture_criterion(got_g.astype(np.float32), case["grad"], g64):
            return False
    return True


def test_fixture_is_the_reference_and_the_model_agrees():
    alpha, cases = _fixture()
    assert np.array_equal(alpha, ou.fixture_alphas()) and alpha.dtype == np.float32 and alpha.shape == (64,)
    assert sorted(cases) == ["nv2_after", "nv2_before", "nv2_clamp3", "opaque_after", "opaque_before"]
    assert (alpha < ou.REF_LO).sum() >= 3 and (alpha > ou.REF_HI).sum() >= 3
    at_lo, at_hi = int(np.flatnonzero(alpha == ou.REF_LO)[0]), int(np.flatnonzero(alpha == ou.REF_HI)[0])
    a64 = np.clip(alpha.astype(np.float64), float(ou.REF_LO), float(ou.REF_HI))
    for name, case in cases.items():
        v64, g64 = _model_of_case(alpha, case)
        v_ref, g_ref = float(case["value"][0]), case["grad"].astype(np.float64)
        if name.endswith("before"):
            assert v_ref == 0.0 and not g_ref.any() and v64 == 0.0
            continue
        # the reference's own fp32 error, bounded as the module text derives
        assert abs(v_ref - v64) <= 16 * 2.0 ** -24 * abs(v64), (name, v_ref, v64)
        scale = case["lam"] / 64.0 * (1.0 / a64 + (0.0 if case["opaque"] else 1.0 / (1.0 - a64)))
        assert (np.abs(g_ref - g64) <= 8 * 2.0 ** -24 * scale).all(), name
        print(f"{name}: reference value off the model by {abs(v_ref - v64) / abs(v64):.2e} relative, "
              f"gradients by at most {np.max(np.abs(g_ref - g64) / scale):.2e} of scale")
        # the gates: zero outside the bounds, NOT zero exactly at them
        outside = (alpha < ou.REF_LO) | (alpha > ou.REF_HI)
        assert not g_ref[outside].any() and not g64[outside].any()
        if name != "nv2_clamp3":
            assert g_ref[at_lo] != 0.0 and g_ref[at_hi] != 0.0 and g64[at_lo] != 0.0 and g64[at_hi] != 0.0
    assert _fixture_check(ou.RIGHT)
    # clamp_alpha = 3: clamp_min cuts some terms, passes others, and none lies within 1e-3 of the cut
    raw, _ = ou.terms(alpha.astype(np.float64), ou.NV2, ou.REF_LO, ou.REF_HI, 1e30)
    assert (np.abs(raw + 3.0) > 1e-3).all() and (raw < -3.0).any() and (raw > -3.0).any()
    c3 = cases["nv2_clamp3"]
    inside = ~((alpha < ou.REF_LO) | (alpha > ou.REF_HI))
    assert not c3["grad"][raw < -3.0].any() and c3["grad"][(raw > -3.0) & inside & (alpha != 0.5)].all()
    assert c3["grad"][at_lo] == 0.0 and c3["grad"][at_hi] == 0.0        # log 0.01 + log 0.99 = -4.6: cut by clamp_min there


# ------------------------------------------------------------------------------------------------------------ the gather's model
def _gather_check(v):
    rng = np.random.default_rng(5)
    for shape in ((2, 2, 3, 33), (1, 3, 4, 65), (2, 1, 5, 31)):
        SB, NV, H, W = shape
        inside = mu.inside_of(mu.random_masks(*shape, 0.5, 3 + W))
        bits, _ = mu.model_table(inside)
        pix = rng.integers(0, NV * H * W, (SB, 200))
        pix[:, 0], pix[:, 1], pix[:, 2], pix[:, 3] = -1, NV * H * W, 0, NV * H * W - 1
        got = ou.gather(bits, pix, NV, H, W, v)
        want = np.stack([inside[o].reshape(-1)[np.clip(pix[o], 0, NV * H * W - 1)] for o in range(SB)]).astype(np.float32)
        want[:, :2] = np.nan
        if not np.array_equal(got, want, equal_nan=True):
            return False
    return True


# ------------------------------------------------------------------------------------------------------------ planted mistakes
def _checks(v):
    """Every criterion above, on the model under variant v -> the names of those that fail."""
    failed = set()
    if not _torch_check(v):
        failed.add("torch fp64")
    if not _fixture_check(v):
        failed.add("fixture")
    if not _gather_check(v):
        failed.add("gather")
    return failed


def test_the_model_passes_its_own_checks():
    assert _checks(ou.RIGHT) == set()


@pytest.mark.parametrize("field,caught_by", [("no_clamp_gate", "fixture"), ("inverted_min_gate", "fixture"), ("mean_over_nk", "torch fp64"),
                                             ("lambda_twice", "fixture"), ("flip_one_minus_m", "torch fp64"), ("col_shift6", "gather")])
def test_planted_mistakes_are_caught(field, caught_by):
    failed = _checks(ou.Variant(**{field: True}))
    assert caught_by in failed, (field, failed)


# ------------------------------------------------------------------------------------------------------------ model/loss.py
def _no_reads(monkeypatch):
    log = []

    def spy(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            log.append(name)
            return real(self, *a, **k)
        return f

    for name in ("item", "tolist", "numpy", "cpu", "__bool__", "__int__", "__float__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, spy(name))
    return log


def test_alpha_loss_nv2_gate_state_dict_and_conf(monkeypatch):
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.model import loss as L
    from pixel_nerf_multiscale_amd.render import autograd as A
    ref_params = ["lambda_alpha", "clamp_alpha", "init_epoch", "force_opaque"]
    assert list(inspect.signature(L.AlphaLossNV2.__init__).parameters)[1:] == ref_params
    assert inspect.signature(L.AlphaLossNV2.__init__).parameters["force_opaque"].default is False
    crit = L.AlphaLossNV2(0.5, 100.0, 2)
    assert list(crit.state_dict()) == ["epoch"] and crit.epoch.dtype == torch.long and int(crit.epoch) == 0
    calls = []
    monkeypatch.setattr(A.AlphaLoss, "apply", staticmethod(lambda *a: (calls.append(a), ("TOTAL", "STATS"))[1]))
    w = torch.rand(2, 5, 7)
    log = _no_reads(monkeypatch)
    assert not crit.active
    z = crit(w)
    assert z.shape == () and z.device == w.device and crit(w) is z and not calls           # a cached 0-dim zero, nothing launched
    crit.sched_step()
    assert not crit.active and crit(w) is z
    crit.sched_step(1)
    assert crit.active and crit(w) == "TOTAL"
    crit.set_epoch(1)
    assert not crit.active
    crit.set_epoch(7)
    assert crit.active
    assert log == [], log                                                                   # the gate never read a tensor
    monkeypatch.undo()
    assert float(z) == 0.0 and int(crit.epoch) == 7
    assert calls == [(w, None, None, N.PNR_ALPHA_NV2, 0.5, 0.0, 0.01, 0.99, 100.0)]
    # the state dict carries the counter; loading refreshes the host mirror
    other = L.AlphaLossNV2(0.5, 100.0, 2)
    other.load_state_dict(crit.state_dict())
    assert int(other.epoch) == 7 and other.active and other._epoch_host == 7
    assert not L.AlphaLossNV2(0.0, 100.0, 0).active and not L.AlphaLossNV2(-1.0, 100.0, 0).active and L.AlphaLossNV2(1e-4, 100.0, 0).active
    # force_opaque picks the BCE mode
    calls.clear()
    monkeypatch.setattr(A.AlphaLoss, "apply", staticmethod(lambda *a: (calls.append(a), ("TOTAL", "STATS"))[1]))
    L.AlphaLossNV2(0.25, 3.0, 0, force_opaque=True)(w)
    assert calls[0][3:] == (N.PNR_ALPHA_OPAQUE, 0.25, 0.0, 0.01, 0.99, 3.0)
    # the reference's conf block
    got = L.get_alpha_loss({"lambda_alpha": 0.001, "clamp_alpha": 100, "init_epoch": 5})
    assert (got.lambda_alpha, got.clamp_alpha, got.init_epoch, got.force_opaque) == (0.001, 100.0, 5, False)
    assert L.get_alpha_loss({"lambda_alpha": 1.0, "clamp_alpha": 1.0, "init_epoch": 0, "force_opaque": True}).force_opaque is True


def test_mask_loss_has_no_default_lambdas_and_passes_both_passes(monkeypatch):
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.model import loss as L
    from pixel_nerf_multiscale_amd.render import autograd as A
    with pytest.raises(TypeError):
        L.MaskLoss()
    with pytest.raises(TypeError):
        L.MaskLoss(1.0)
    for bad in (0.0, 0.5, -0.1):
        with pytest.raises(ValueError):
            L.MaskLoss(1.0, 1.0, eps=bad)
    calls = []
    monkeypatch.setattr(A.AlphaLoss, "apply", staticmethod(lambda *a: (calls.append(a), ("TOTAL", "STATS"))[1]))
    crit = L.MaskLoss(0.5, 2.0)
    wc, wf, m = torch.rand(2, 3, 4), torch.rand(2, 3, 6), torch.rand(2, 3)
    assert crit({"coarse": {"weights": wc}, "fine": {"weights": wf}}, m) == ("TOTAL", "STATS")
    assert crit({"coarse": {"weights": wc}, "fine": {}}, m) == ("TOTAL", "STATS") and crit({"coarse": {"weights": wc}}, m)
    assert calls[0] == (wc, wf, m, N.PNR_ALPHA_MASK, 0.5, 2.0, 0.01, 0.99, 0.0)
    assert calls[1][:3] == (wc, None, m) and calls[2][:3] == (wc, None, m)


# ------------------------------------------------------------------------------------------------------------ make_batch
def _data(masks=True, as_bytes=False):
    SB, NV, H, W = 2, 3, 6, 7
    m = torch.from_numpy(np.random.default_rng(11).random((SB, NV, H, W)) < 0.4)
    data = {"images": torch.zeros(SB, NV, H, W, 3, dtype=torch.uint8) if as_bytes else torch.zeros(SB, NV, 3, H, W),
            "poses": torch.zeros(SB, NV, 4, 4), "focal": torch.ones(SB),
            "bbox": torch.tensor([0.0, 0.0, W - 1.0, H - 1.0]).expand(SB, NV, 4).contiguous()}
    if masks:
        data["masks"] = m.to(torch.uint8) * 255 if as_bytes else m[:, :, None].float()
    return data


KW = dict(ray_batch_size=10, nviews=[2], z_near=0.1, z_far=1.0)
SIX = ("RAYS", "RGB", "SRC", "POSES", "FOCAL", "C")


def _spied(monkeypatch, data, **kw):
    """make_batch on the CPU with every native call and the gather replaced by recorders -> (its result, the calls in order)."""
    from pixel_nerf_multiscale_amd import train, util
    calls = []
    real_empty = torch.empty
    SB, B = data["poses"].shape[0], KW["ray_batch_size"]

    def rec(name, result):
        def f(*a, **k):
            calls.append((name, a, k))
            return result(*a, **k) if callable(result) else result
        return f

    draw = (torch.arange(SB * B).view(SB, B), torch.zeros(SB, 2, dtype=torch.long))
    monkeypatch.setattr(torch, "empty", lambda *a, pin_memory=False, **k: real_empty(*a, **k))
    monkeypatch.setattr(util, "upload", lambda t, device: t)
    for name, result in (("train_draw", draw), ("train_draw_masked", draw), ("mask_table", ("BITS", "ROWS")), ("mask_gather", "MASK"),
                         ("bbox_sample", util.bbox_sample), ("masked_sample", util.masked_sample)):
        monkeypatch.setattr(util, name, rec(name, result))
    monkeypatch.setattr(train, "_gather_batch", rec("gather", SIX))
    out = train.make_batch(data, "cpu", **kw, **KW)
    monkeypatch.undo()
    return out, calls


def test_want_mask_false_makes_the_calls_made_before(monkeypatch):
    from pixel_nerf_multiscale_amd import train
    assert inspect.signature(train.make_batch).parameters["want_mask"].default is False
    dev = dict(draws="device", seed=9)
    for data in (_data(), _data(as_bytes=True), _data(masks=False)):
        for kw in (dev, dict(dev, use_bbox=False), dict(dev, is_train=False), dict(dev, obj_base=4)):
            (out_a, a), (out_b, b) = _spied(monkeypatch, data, **kw), _spied(monkeypatch, data, want_mask=False, **kw)
            assert out_a == out_b == SIX
            assert [c[0] for c in a] == [c[0] for c in b] == ["train_draw", "gather"]
            assert a[0][1][1:] == b[0][1][1:] and sorted(a[0][2]) == sorted(b[0][2]) == ["obj_base", "out_pix"]
        if "masks" in data:
            out, calls = _spied(monkeypatch, data, prop_inside=0.3, **dev)
            assert out == SIX and [c[0] for c in calls] == ["mask_table", "train_draw_masked", "gather"]
        torch.manual_seed(4); np.random.seed(4)
        out, host = _spied(monkeypatch, data)
        assert out == SIX and [c[0] for c in host] == ["bbox_sample", "bbox_sample", "gather"]


def test_want_mask_gathers_from_one_table(monkeypatch):
    from pixel_nerf_multiscale_amd import train
    dev = dict(draws="device", seed=9, want_mask=True)
    for data in (_data(), _data(as_bytes=True)):
        out, calls = _spied(monkeypatch, data, **dev)
        assert out == SIX + ("MASK",) and [c[0] for c in calls] == ["train_draw", "gather", "mask_table", "mask_gather"]
        table_in = calls[2][1][0]
        want = data["masks"] if data["masks"].dtype == torch.uint8 else (data["masks"][:, :, 0] >= 0.5).to(torch.uint8) * 255
        assert table_in.dtype == torch.uint8 and torch.equal(table_in, want)
        g = calls[3][1]
        assert g[0] == "BITS" and torch.equal(g[1], torch.arange(20).view(2, 10)) and g[2:] == (3, 6, 7)
        # with prop_inside the draw and the gather share ONE table
        out, calls = _spied(monkeypatch, data, prop_inside=0.3, **dev)
        assert out == SIX + ("MASK",) and [c[0] for c in calls] == ["mask_table", "train_draw_masked", "gather", "mask_gather"]
        assert calls[1][1][:2] == ("BITS", "ROWS") and calls[3][1][0] == "BITS"
        # a resident batch brings its tables: nothing is built; the bits alone serve the gather
        for extra in (dict(mask_bits="B", mask_rows="R"), dict(mask_bits="B")):
            res = {k: v for k, v in data.items() if k != "masks"}
            out, calls = _spied(monkeypatch, dict(res, **extra), **dev)
            assert [c[0] for c in calls] == ["train_draw", "gather", "mask_gather"] and calls[2][1][0] == "B"
        out, calls = _spied(monkeypatch, dict(data, mask_bits="B", mask_rows="R"), prop_inside=0.3, **dev)
        assert [c[0] for c in calls] == ["train_draw_masked", "gather", "mask_gather"] and calls[2][1][0] == "B"
        # evaluation and host draws gather too
        out, calls = _spied(monkeypatch, data, is_train=False, **dev)
        assert out[6] == "MASK" and [c[0] for c in calls] == ["train_draw", "gather", "mask_table", "mask_gather"]
        torch.manual_seed(4); np.random.seed(4)
        out, calls = _spied(monkeypatch, data, want_mask=True)
        assert out[6] == "MASK" and [c[0] for c in calls] == ["bbox_sample", "bbox_sample", "gather", "mask_table", "mask_gather"]
    for draws in (dict(), dict(draws="device", seed=3)):
        with pytest.raises(ValueError, match="want_mask needs the batch's masks"):
            train.make_batch(_data(masks=False), "cpu", want_mask=True, **draws, **KW)


def test_python_wrapper_checks_its_arguments():
    from pixel_nerf_multiscale_amd import util
    bits, pix = torch.zeros(2, 12, 1, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.long)
    ok = dict(bits=bits, pix_inds=pix, NV=3, H=4, W=5)
    call = lambda **kw: util.mask_gather(**{**ok, **kw})
    for kw in (dict(NV=0), dict(W=33), dict(bits=bits.long()), dict(bits=bits[:1]), dict(pix_inds=pix.int()), dict(pix_inds=pix[0]),
               dict(out=torch.zeros(2, 7)), dict(out=torch.zeros(2, 8, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(RuntimeError):                     # host tensors pass the shape checks and are refused as such
        call()


def test_steps_and_trainer_carry_the_keywords():
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.trainer import Trainer
    for fn in (train.calc_losses, Trainer.__init__):
        for name in ("alpha_loss", "mask_loss"):
            assert inspect.signature(fn).parameters[name].default is None
