"""pnr_mask_gather, pnr_alpha_loss and pnr_alpha_loss_bwd on the device against the fp64 model of tests/opacity_loss_util.py, and
the layers on top: render.autograd.AlphaLoss, model.loss.AlphaLossNV2 / MaskLoss, train.make_batch(want_mask=True),
train.calc_losses(alpha_loss=, mask_loss=) and a Trainer resumed from a checkpoint.

Bounds.  The gather is integer: torch.equal.  alpha_out is the model's sum bit for bit (the order is the header's).  Every loss
value and every gradient entry lies within 2^-23 relative of the fp64 model: the device evaluates in fp64 and rounds once
(2^-24); its log and its sum's order may differ from numpy's in the last fp64 bits, far below the doubled allowance.  The
gates (which entries are exactly zero) must be the model's.  The reference's recorded values pass under the CPU test's
criterion, |got - v_ref| <= |v_ref - v64| + 2^-23 |v64|.  Through the composite the project's backward bound applies:
5e-4 of the gradient's scale against float64 autograd through the oracle."""
import os

import numpy as np
import pytest
import torch

import data_trees as dt
import golden_util as gu
import mask_draw_util as mu
import opacity_loss_util as ou

pytestmark = pytest.mark.gpu

LO, HI = ou.REF_LO, ou.REF_HI
SENT_F, SENT_D = -777.25, -555.5


# ------------------------------------------------------------------------------------------------------------ the gather
@pytest.mark.parametrize("W", [1, 31, 32, 33, 65])
def test_mask_gather_matches_the_model(W):
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd import util
    SB, NV, H, PAD = 2, 2, 3, 37
    n_pix = NV * H * W
    masks = mu.random_masks(SB, NV, H, W, 0.5, 7 + W)
    bits = util.mask_table(torch.from_numpy(masks).cuda())[0]
    mbits, _ = mu.model_table(mu.inside_of(masks))
    assert torch.equal(bits.cpu(), torch.from_numpy(mbits.view(np.int32)))
    rng = np.random.default_rng(W)
    for B in (1, 255, 256, 257):
        pix = rng.integers(0, n_pix, (SB, B))
        pix[0, 0] = n_pix - 1
        if B > 1:
            pix[0, 1], pix[1, 0], pix[1, B - 1], pix[1, 1] = -1, n_pix, 0, np.iinfo(np.int64).min
        want = torch.from_numpy(ou.gather(mbits, pix, NV, H, W))
        dev_pix = torch.from_numpy(pix).cuda()
        got = util.mask_gather(bits, dev_pix, NV, H, W)
        assert got.dtype == torch.float32 and tuple(got.shape) == (SB, B)
        assert torch.equal(torch.isnan(got.cpu()), torch.isnan(want)) and torch.equal(got.cpu().nan_to_num(-1.0), want.nan_to_num(-1.0))
        inside = torch.from_numpy(mu.inside_of(masks).reshape(SB, -1))
        ok = (dev_pix.cpu() >= 0) & (dev_pix.cpu() < n_pix)
        assert torch.equal(got.cpu()[ok], torch.gather(inside, 1, dev_pix.cpu().clamp(0, n_pix - 1))[ok].float())
        if B > 1:
            assert int(torch.isnan(got).sum()) == 3
        # sentinel margins around mask_out, which sits at an odd 4-byte offset of a larger buffer
        buf = torch.full((PAD + SB * B + PAD,), SENT_F, device="cuda")
        rc = N.lib.pnr_mask_gather(bits.data_ptr(), SB, NV, H, W, dev_pix.data_ptr(), B, buf.data_ptr() + 4 * PAD, N.current_stream(buf.device))
        torch.cuda.synchronize()
        assert rc == 0 and bool((buf[:PAD] == SENT_F).all()) and bool((buf[PAD + SB * B:] == SENT_F).all())
        assert torch.equal(buf[PAD:PAD + SB * B].view(SB, B).nan_to_num(-1.0), got.nan_to_num(-1.0))
        out = torch.empty(SB, B, device="cuda")
        assert util.mask_gather(bits, dev_pix, NV, H, W, out=out).data_ptr() == out.data_ptr() and torch.equal(out.nan_to_num(-1.0), got.nan_to_num(-1.0))


# ------------------------------------------------------------------------------------------------------------ the loss, raw calls
def _weights(n, K, seed):
    """(n, K) fp32 weights whose row sums cover the clamp's three regimes (below lo, inside, above hi), none near a bound."""
    rng = np.random.default_rng(seed)
    w = rng.random((n, K)).astype(np.float32) + np.float32(0.05)
    kinds = rng.integers(0, 5, n)
    target = np.where(kinds == 0, rng.uniform(0.0, 0.008, n), np.where(kinds == 1, rng.uniform(0.995, 1.3, n), rng.uniform(0.02, 0.98, n)))
    return (w / w.sum(axis=1, keepdims=True) * target[:, None]).astype(np.float32)


def _call(c, f, m, mode, lam_c, lam_f, lo=LO, hi=HI, ca=100.0, d_total=None, pad=0):
    """pnr_alpha_loss then pnr_alpha_loss_bwd on numpy inputs -> dict(stats (3,), alpha (2, n), d_c, d_f) of numpy arrays; with pad,
    every output sits inside a sentinel-filled buffer whose margins are checked."""
    from pixel_nerf_multiscale_amd import _native as N
    dev = torch.device("cuda")
    n = (c if c is not None else f).shape[0]
    tc, tf, tm = (None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda() for x in (c, f, m))
    Kc, Kf = (0 if c is None else c.shape[1]), (0 if f is None else f.shape[1])
    alpha = torch.full((pad + 2 * n + pad,), SENT_D, dtype=torch.float64, device=dev)
    stats = torch.full((pad + 3 + pad,), SENT_F, device=dev)
    d_c = None if c is None else torch.full((pad + n * Kc + pad,), SENT_F, device=dev)
    d_f = None if f is None else torch.full((pad + n * Kf + pad,), SENT_F, device=dev)
    dt_ = None if d_total is None else torch.tensor([d_total], dtype=torch.float32, device=dev)
    s = N.current_stream(dev)
    p = lambda t, size: None if t is None else t.data_ptr() + size * pad
    cfg = (mode, float(lam_c), float(lam_f), float(lo), float(hi), float(ca))
    rc = N.lib.pnr_alpha_loss(N.ptr(tc), Kc, N.ptr(tf), Kf, N.ptr(tm), n, *cfg, p(alpha, 8), p(stats, 4), s)
    assert rc == 0
    rc = N.lib.pnr_alpha_loss_bwd(p(alpha, 8), N.ptr(tm), n, Kc, Kf, *cfg, N.ptr(dt_), p(d_c, 4), p(d_f, 4), s)
    torch.cuda.synchronize()
    assert rc == 0
    out = {}
    for name, t, count, sent in (("alpha", alpha, 2 * n, SENT_D), ("stats", stats, 3, SENT_F), ("d_c", d_c, n * Kc, SENT_F), ("d_f", d_f, n * Kf, SENT_F)):
        if t is None:
            out[name] = None
            continue
        assert bool((t[:pad] == sent).all()) and bool((t[pad + count:] == sent).all()), name
        out[name] = t[pad:pad + count].cpu().numpy()
    out["alpha"] = out["alpha"].reshape(2, n)
    out["d_c"] = None if c is None else out["d_c"].reshape(n, Kc)
    out["d_f"] = None if f is None else out["d_f"].reshape(n, Kf)
    return out


def _compare(got, want, c, f, tag):
    """Every value and gradient of one call against the model; -> the worst relative errors seen (value, gradient)."""
    assert ou.within_one_rounding(got["stats"][:2], want["stats64"]), (tag, got["stats"], want["stats64"])
    assert got["stats"][2] == np.float32(got["stats"][0] + got["stats"][1]), tag
    worst_v = max(abs(float(g) - w) / abs(w) for g, w in zip(got["stats"][:2], want["stats64"]) if w != 0.0)
    worst_g = 0.0
    for k, (w, d, g64) in enumerate(((c, got["d_c"], want["grad_c"]), (f, got["d_f"], want["grad_f"]))):
        if w is None:
            assert got["stats"][k] == 0.0
            continue
        assert np.array_equal(got["alpha"][k], want["alpha"][k]), tag                 # the header's order, bit for bit
        assert (d == d[:, :1]).all(), tag                                                # one value per ray
        assert ou.within_one_rounding(d[:, 0], g64), tag
        assert np.array_equal(d[:, 0] == 0.0, g64 == 0.0), tag                           # the gates
        nz = g64 != 0.0
        if nz.any():
            worst_g = max(worst_g, float(np.max(np.abs(d[nz, 0] - g64[nz]) / np.abs(g64[nz]))))
    return worst_v, worst_g


N_RAYS = (1, 63, 64, 65, 1023, 1025, 4097)
KS = ((1, 1), (63, 65), (64, 112), (257, 0))
MODES = ((ou.NV2, 100.0), (ou.NV2, 3.0), (ou.OPAQUE, 0.0), (ou.MASK, 0.0))


@pytest.mark.parametrize("Kc,Kf", KS)
def test_values_and_gradients_match_the_model(Kc, Kf):
    worst = [0.0, 0.0]
    for n in N_RAYS:
        c = _weights(n, Kc, 1000 * Kc + n)
        f = _weights(n, Kf, 2000 * Kf + n + 1) if Kf else None
        m = np.random.default_rng(n).choice(np.array([0.0, 0.25, 1.0], np.float32), n)
        for mode, ca in MODES:
            got = _call(c, f, m if mode == ou.MASK else None, mode, 0.75, 1.5, ca=ca, pad=19 if n in (1, 65, 1025) else 0)
            want = ou.model(c, f, m, mode, 0.75, 1.5, LO, HI, ca)
            v, g = _compare(got, want, c, f, (n, Kc, Kf, mode, ca))
            worst = [max(worst[0], v), max(worst[1], g)]
    # the fine pass alone: the coarse row of alpha_out and its statistic stay out of it
    if Kf:
        got = _call(None, f, None, ou.NV2, 0.75, 1.5)
        want = ou.model(None, f, None, ou.NV2, 0.75, 1.5, LO, HI, 100.0)
        _compare(got, want, None, f, "fine alone")
        assert (got["alpha"][0] == SENT_D).all()
    print(f"K = ({Kc}, {Kf}): worst relative error of a value {worst[0]:.2e}, of a gradient entry {worst[1]:.2e} (allowed {ou.EPS32:.2e})")


def test_gates_are_exact_at_the_clamp_bounds():
    """K = 1: alpha is the weight itself.  Exactly 0.01f and 0.99f pass the clamp's gate, their fp32 neighbours outside do not."""
    alpha = ou.fixture_alphas()
    at_lo, at_hi = int(np.flatnonzero(alpha == LO)[0]), int(np.flatnonzero(alpha == HI)[0])
    m = np.resize(np.array([0.0, 0.25, 1.0], np.float32), alpha.shape[0])
    m[at_lo], m[at_hi] = 0.25, 0.25
    for mode, ca in MODES:
        got = _call(alpha[:, None], alpha[:, None], m if mode == ou.MASK else None, mode, 0.5, 0.25, ca=ca)
        want = ou.model(alpha[:, None], alpha[:, None], m, mode, 0.5, 0.25, LO, HI, ca)
        _compare(got, want, alpha[:, None], alpha[:, None], (mode, ca))
        outside = (alpha < LO) | (alpha > HI)
        assert not got["d_c"][outside].any() and not got["d_f"][outside].any()
        if ca != 3.0:                                     # under clamp_alpha = 3 clamp_min cuts the term at both bounds
            assert got["d_c"][at_lo, 0] != 0.0 and got["d_c"][at_hi, 0] != 0.0
        else:
            assert got["d_c"][at_lo, 0] == 0.0 and got["d_c"][at_hi, 0] == 0.0
        for k in (at_lo - 1, at_hi + 1):
            assert got["d_c"][k, 0] == 0.0 and outside[k]


def test_a_nan_weight_gives_a_nan_loss_and_a_nan_row():
    n, K = 70, 65
    c, f = _weights(n, K, 3), _weights(n, 7, 4)
    c[5, 64] = np.nan
    m = np.full(n, 0.25, np.float32)
    for mode, ca in MODES:
        got = _call(c, f, m if mode == ou.MASK else None, mode, 1.0, 1.0, ca=ca)
        assert np.isnan(got["stats"][0]) and np.isfinite(got["stats"][1]) and np.isnan(got["stats"][2])
        assert np.isnan(got["d_c"][5]).all() and np.isfinite(np.delete(got["d_c"], 5, axis=0)).all() and np.isfinite(got["d_f"]).all()
        assert np.isnan(got["alpha"][0, 5]) and np.isfinite(np.delete(got["alpha"][0], 5)).all()


def test_d_total_scales_exactly_and_runs_repeat():
    n = 1025
    c, f = _weights(n, 64, 8), _weights(n, 112, 9)
    m = np.random.default_rng(1).choice(np.array([0.0, 0.25, 1.0], np.float32), n)
    for mode, ca in MODES:
        mm = m if mode == ou.MASK else None
        base = _call(c, f, mm, mode, 0.75, 1.5, ca=ca)
        again = _call(c, f, mm, mode, 0.75, 1.5, ca=ca, d_total=1.0)
        for k in ("stats", "alpha", "d_c", "d_f"):
            assert np.array_equal(base[k].view(np.uint8), again[k].view(np.uint8)), k            # the same bits, NULL d_total = 1
        for e in (-3, 10, 16):
            scaled = _call(c, f, mm, mode, 0.75, 1.5, ca=ca, d_total=2.0 ** e)
            assert np.array_equal(scaled["d_c"], base["d_c"] * np.float32(2.0 ** e)) and np.array_equal(scaled["d_f"], base["d_f"] * np.float32(2.0 ** e))


def test_no_rays_give_three_zeros():
    from pixel_nerf_multiscale_amd import _native as N
    stats = torch.full((3,), SENT_F, device="cuda")
    alpha = torch.full((4,), SENT_D, dtype=torch.float64, device="cuda")
    w = torch.zeros(4, device="cuda")
    s = N.current_stream(w.device)
    assert N.lib.pnr_alpha_loss(N.ptr(w), 4, N.ptr(w), 2, None, 0, ou.NV2, 1.0, 1.0, 0.01, 0.99, 100.0, alpha.data_ptr(), N.ptr(stats), s) == 0
    assert N.lib.pnr_alpha_loss_bwd(alpha.data_ptr(), None, 0, 4, 2, ou.NV2, 1.0, 1.0, 0.01, 0.99, 100.0, None, N.ptr(w), N.ptr(w), s) == 0
    torch.cuda.synchronize()
    assert stats.tolist() == [0.0, 0.0, 0.0] and bool((alpha == SENT_D).all()) and not bool(w.any())


# ------------------------------------------------------------------------------------------------------------ under autograd
def test_alpha_loss_function_under_autograd():
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.render.autograd import AlphaLoss
    SB, B, Kc, Kf = 2, 33, 8, 14
    c, f = _weights(SB * B, Kc, 5), _weights(SB * B, Kf, 6)
    m = np.random.default_rng(2).choice(np.array([0.0, 0.25, 1.0], np.float32), SB * B)
    tc = torch.from_numpy(c).cuda().view(SB, B, Kc).requires_grad_(True)
    tf = torch.from_numpy(f).cuda().view(SB, B, Kf).requires_grad_(True)
    tm = torch.from_numpy(m).cuda().view(SB, B).requires_grad_(True)
    total, stats = AlphaLoss.apply(tc, tf, tm, N.PNR_ALPHA_MASK, 0.75, 1.5, 0.01, 0.99, 0.0)
    assert total.dim() == 0 and total.requires_grad and not stats.requires_grad and tuple(stats.shape) == (3,)
    assert total.data_ptr() == stats[2].data_ptr()
    (total * 4.0).backward()
    want = ou.model(c, f, m, ou.MASK, 0.75, 1.5, LO, HI, 0.0, d_total=4.0)
    assert ou.within_one_rounding(stats.cpu().numpy()[:2], want["stats64"])
    assert tuple(tc.grad.shape) == (SB, B, Kc) and tuple(tf.grad.shape) == (SB, B, Kf) and tm.grad is None
    assert ou.within_one_rounding(tc.grad.cpu().numpy().reshape(-1, Kc)[:, 0], want["grad_c"])
    assert ou.within_one_rounding(tf.grad.cpu().numpy().reshape(-1, Kf)[:, 3], want["grad_f"])
    # one pass alone, and only the weights that ask get a gradient
    tc2 = tc.detach().clone().requires_grad_(True)
    t2, s2 = AlphaLoss.apply(tc2, tf.detach(), None, N.PNR_ALPHA_NV2, 0.5, 0.25, 0.01, 0.99, 100.0)
    t2.backward()
    want2 = ou.model(c, f, None, ou.NV2, 0.5, 0.25, LO, HI, 100.0)
    assert ou.within_one_rounding(tc2.grad.cpu().numpy().reshape(-1, Kc)[:, 0], want2["grad_c"])
    with pytest.raises(ValueError):
        AlphaLoss.apply(None, None, None, N.PNR_ALPHA_NV2, 1.0, 1.0, 0.01, 0.99, 100.0)
    with pytest.raises(ValueError):
        AlphaLoss.apply(tc, tf[:, :5], None, N.PNR_ALPHA_NV2, 1.0, 1.0, 0.01, 0.99, 100.0)
    with pytest.raises(ValueError):
        AlphaLoss.apply(tc, None, tm[:, :5], N.PNR_ALPHA_MASK, 1.0, 1.0, 0.01, 0.99, 100.0)
    with pytest.raises(ValueError):
        AlphaLoss.apply(tc, None, None, N.PNR_ALPHA_MASK, 1.0, 1.0, 0.01, 0.99, 100.0)           # PNR_E_NULL: MASK without a mask


def test_the_reference_fixture_through_alpha_loss_nv2():
    from pixel_nerf_multiscale_amd.model.loss import AlphaLossNV2
    d = np.load(os.path.join(gu.GOLDEN_DIR, "alpha_loss.npz"))
    alpha = d["alpha"]
    for name in str(d["names"]).split(","):
        lam, ca, init_epoch, opaque, steps = d[f"{name}__cfg"].tolist()
        crit = AlphaLossNV2(lam, ca, int(init_epoch), force_opaque=bool(opaque)).cuda()
        if steps:
            crit.sched_step(int(steps))
        w = torch.from_numpy(alpha.copy()).cuda()[:, None].requires_grad_(True)
        value = crit(w)
        assert value.dim() == 0
        active = steps >= init_epoch
        assert crit.active == active and int(crit.epoch) == int(steps)
        if not active:
            assert float(value) == 0.0 and not value.requires_grad and float(d[f"{name}__value"][0]) == 0.0
            continue
        value.backward()
        p = ou.one_pass(alpha[:, None], ou.OPAQUE if opaque else ou.NV2, lam, LO, HI, ca)
        got_v, got_g = value.detach().cpu().numpy(), w.grad.cpu().numpy()[:, 0]
        print(f"{name}: device {float(got_v):.9g}, reference {float(d[f'{name}__value'][0]):.9g}, fp64 model {p['loss']:.12g}")
        assert ou.fixture_criterion(got_v, d[f"{name}__value"][0], p["loss"]), name
        assert ou.fixture_criterion(got_g, d[f"{name}__grad"], p["grad"]), name
        assert np.array_equal(got_g == 0.0, d[f"{name}__grad"] == 0.0), name                       # the reference's gates, entry by entry


def test_mask_loss_gradient_through_the_composite():
    """B = 8 rays of K = 8 samples, total = the mask loss alone: d(rgb sigma) against float64 autograd through the oracle's
    composite, within the project's backward bound of 5e-4 of the gradient's scale."""
    from oracle import pixelnerf_oracle as orc
    from pixel_nerf_multiscale_amd.model.loss import MaskLoss
    from pixel_nerf_multiscale_amd.render.autograd import Composite
    B, K = 8, 8
    rng = np.random.default_rng(12)
    rays = np.zeros((B, 8), np.float32)
    rays[:, 3:6], rays[:, 6], rays[:, 7] = rng.normal(size=(B, 3)), 1.0, 3.0
    z = np.sort(rng.uniform(1.0, 3.0, (B, K)), axis=1).astype(np.float32)
    out = np.concatenate([rng.random((B, K, 3)), rng.uniform(-1.0, 6.0, (B, K, 1))], axis=2).astype(np.float32)
    m = np.array([0.0, 1.0, 0.25, 1.0, 0.0, 1.0, 0.0, 1.0], np.float32)
    crit = MaskLoss(0.75, 1.5)
    t_out = torch.from_numpy(out).cuda().requires_grad_(True)
    w, _, _ = Composite.apply(torch.from_numpy(rays).cuda(), torch.from_numpy(z).cuda(), t_out, True)
    total, stats = crit({"coarse": {"weights": w.view(1, B, K)}}, torch.from_numpy(m).cuda().view(1, B))
    total.backward()
    o64 = torch.from_numpy(out).double().requires_grad_(True)
    w64, _, _ = orc.composite(torch.from_numpy(rays).double(), torch.from_numpy(z).double(), o64, True)
    a = torch.clamp(w64.sum(-1), float(LO), float(HI))
    want = 0.75 * torch.nn.functional.binary_cross_entropy(a, torch.from_numpy(m).double())
    want.backward()
    got, ref = t_out.grad.cpu().double(), o64.grad
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    print(f"mask loss through the composite: value {float(total):.7g} vs {float(want):.10g}, gradient off by {err / scale:.2e} of scale")
    assert scale > 0.0 and err <= 5e-4 * scale
    # the value: the fp32 weights are within K 2^-24 relative, alpha within 8 x 6e-8 = 5e-7, and |dt / dalpha| <= 1 / 0.01 inside the
    # clamp: 5e-5 of a term of order one at worst — 1e-4 relative allowed
    assert abs(float(total) - float(want)) <= 1e-4 * abs(float(want)) and float(stats[1]) == 0.0
    assert not bool(got[..., :3].any())                       # the colours do not reach the weights


# ------------------------------------------------------------------------------------------------------------ calc_losses
CAT, SIZE = "02691156", 8


@pytest.fixture(scope="module")
def dvr_tree(tmp_path_factory):
    """Three objects of three 8 x 8 views with L-shaped masks (test_gpu_mask_draw's tree)."""
    root = tmp_path_factory.mktemp("nmr8")
    rng = np.random.default_rng(4)
    for o, name in enumerate(("a", "b", "c")):
        images = rng.integers(0, 256, (3, SIZE, SIZE, 3), dtype=np.uint8)
        masks = np.zeros((3, SIZE, SIZE), np.uint8)
        for v in range(3):
            masks[v, 1 + o % 2:6, 2:3 + v] = 255
            masks[v, 5:6 + v % 2, 2:7 - o % 2] = 255
        cams = {}
        for v in range(3):
            mat = np.eye(4)
            mat[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            mat[:3, 3] = rng.normal(size=3)
            cams[f"world_mat_{v}"], cams[f"camera_mat_{v}"] = mat, np.diag([2.1875, 2.1875, 1.0, 1.0])
        dt.write_dvr_object(str(root / CAT / name), images, masks, cams)
    with open(str(root / CAT / "softras_train.lst"), "w") as fh:
        fh.write("a\nb\nc\n")
    return str(root)


def _stack(dset, ids):
    keys = [k for k in ("images", "masks", "poses", "bbox", "focal", "c") if k in dset[0]]
    return {k: torch.stack([torch.as_tensor(dset[i][k]) for i in ids]) for k in keys}


def test_calc_losses_three_ways(dvr_tree, monkeypatch):
    from test_gpu_train_front import _front_end_setup
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.data import ResidentSplit, get_split_dataset
    from pixel_nerf_multiscale_amd.model.loss import AlphaLossNV2, MaskLoss, RenderLoss
    as_float = get_split_dataset("dvr", dvr_tree, want_split="train", as_bytes=False)
    as_bytes = get_split_dataset("dvr", dvr_tree, want_split="train", as_bytes=True)
    ids, B, dev = [2, 0], 24, torch.device("cuda")
    split = ResidentSplit(as_bytes, "cuda", device_masks=True, device_boxes=True)
    batches = (_stack(as_float, ids), _stack(as_bytes, ids), split.batch(ids))
    net, rend, _, _ = _front_end_setup()
    render_par = rend.bind_parallel(net, None)
    kw = dict(ray_batch_size=B, nviews=[2], z_near=as_bytes.z_near, z_far=as_bytes.z_far, loss=RenderLoss(1.0, 1.0), balanced=as_bytes.balanced,
              draws="device", seed=77)
    mask_loss, alpha_loss = MaskLoss(0.5, 0.25), AlphaLossNV2(1e-2, 100.0, 1)
    alpha_loss.set_epoch(1)
    masks = torch.from_numpy(mu.inside_of(batches[1]["masks"].numpy()).reshape(2, -1)).float()
    results = []
    for data in batches:
        for prop in (None, 0.75):
            more = {} if prop is None else {"prop_inside": prop}
            out = train.make_batch(data, dev, want_mask=True, **{k: v for k, v in kw.items() if k != "loss"}, **more)
            six = train.make_batch(data, dev, **{k: v for k, v in kw.items() if k != "loss"}, **more)
            assert len(out) == 7 and len(six) == 6
            for x, y in zip(out, six):
                assert (x is None and y is None) or torch.equal(x, y)
            rays, mask_gt = out[0], out[6]
            # the masks gathered in torch at the same pix_inds: the draw is keyed, so it can be made again
            if prop is None:
                pix, _ = util.train_draw(data.get("bbox_dev") if "bbox_dev" in data else data["bbox"].float().cuda(), 2, 3, SIZE, SIZE, B, 2, 77)
            else:
                bits, rows = (data["mask_bits"], data["mask_rows"]) if "mask_bits" in data else util.mask_table(util.mask_bytes(data["masks"].cuda()))
                pix, _ = util.train_draw_masked(bits, rows, 2, 3, SIZE, SIZE, B, 2, 77, prop)
            assert mask_gt.dtype == torch.float32 and tuple(mask_gt.shape) == (2, B)
            assert torch.equal(mask_gt.cpu(), torch.gather(masks, 1, pix.cpu()))
            if prop is not None:
                assert bool((mask_gt[:, :18] == 1.0).all()) and bool((mask_gt[:, 18:] == 0.0).all())
        for p in net.parameters():
            p.grad = None
        with rend.keyed(5):                                 # one key: every render of this batch draws the same samples
            total, d = train.calc_losses(net, render_par, data, alpha_loss=alpha_loss, mask_loss=mask_loss, **kw)
            plain_total, plain = train.calc_losses(net, render_par, data, **kw)
            none_total, none = train.calc_losses(net, render_par, data, alpha_loss=None, mask_loss=None, **kw)
            ev = train.eval_step(net, rend, render_par, data, alpha_loss=alpha_loss, mask_loss=mask_loss, **kw)
            early = AlphaLossNV2(1e-2, 100.0, 5)
            e_total, e = train.calc_losses(net, render_par, data, alpha_loss=early, **kw)
        total.backward()
        assert list(d) == ["rc", "rf", "t", "m", "a"] and all(v.dim() == 0 and v.is_cuda and not v.requires_grad for v in d.values())
        assert float(d["m"]) > 0.0 and float(d["a"]) < 0.0 and float(d["t"]) == float(total.detach())
        assert float(d["rc"]) == float(plain["rc"]) and float(d["rf"]) == float(plain["rf"])
        assert float(total.detach()) == float((plain_total.detach() + d["m"]) + d["a"])
        grads = [p.grad.detach().clone() for p in net.mlp_coarse.parameters()]
        assert all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0.0 for g in grads)
        # both at None: the same calls, the same bits as without the keywords
        assert list(none) == list(plain) == ["rc", "rf", "t"] and torch.equal(none_total, plain_total)
        assert all(torch.equal(none[k], plain[k]) for k in plain)
        # validation computes them too; before init_epoch "a" is a zero and nothing is added
        assert list(ev) == ["rc", "rf", "t", "m", "a"] and float(ev["m"]) > 0.0 and float(ev["a"]) < 0.0
        assert float(e["a"]) == 0.0 and torch.equal(e_total, plain_total) and list(e) == ["rc", "rf", "t", "a"]
        results.append((float(total.detach()), float(d["m"]), float(d["a"]), grads))
    for r in results[1:]:                                   # float batch, byte batch and resident tables: one step
        assert r[:3] == results[0][:3]

    # the step on a resident batch: the losses add no host read and no transfer to what the step made without them, and the
    # front end and the two losses on their own read nothing at all
    data = batches[2]
    log = []
    real_to = torch.Tensor.to

    def to(self, *a, **k):
        out = real_to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            log.append(("read", "to"))
        return out

    def read(name):
        real = getattr(torch.Tensor, name)

        def f(self, *a, **k):
            if self.is_cuda:
                log.append(("read", name))
            return real(self, *a, **k)
        return f

    monkeypatch.setattr(torch.Tensor, "to", to)
    for name in ("cpu", "item", "tolist", "numpy", "__bool__", "__int__", "__float__"):
        monkeypatch.setattr(torch.Tensor, name, read(name))
    with rend.keyed(5):
        total, d = train.calc_losses(net, render_par, data, prop_inside=0.75, **kw)
        total.backward()
        without, log[:] = list(log), []
        total, d = train.calc_losses(net, render_par, data, alpha_loss=alpha_loss, mask_loss=mask_loss, prop_inside=0.75, **kw)
        total.backward()
        with_losses, log[:] = list(log), []
    batch = train.make_batch(data, dev, want_mask=True, prop_inside=0.75, **{k: v for k, v in kw.items() if k != "loss"})
    wc = torch.rand(2, B, 8, device="cuda", requires_grad=True)
    wf = torch.rand(2, B, 14, device="cuda", requires_grad=True)
    m_total, _ = mask_loss({"coarse": {"weights": wc}, "fine": {"weights": wf}}, batch[6])
    (m_total + alpha_loss(wf) + early(wf)).backward()
    alone = list(log)
    monkeypatch.undo()
    assert with_losses == without and alone == [], (without, with_losses, alone)
    assert wc.grad is not None and wf.grad is not None
    with pytest.raises(ValueError, match="want_mask needs the batch's masks"):
        train.calc_losses(net, render_par, {k: v for k, v in batches[0].items() if k != "masks"}, mask_loss=mask_loss, **kw)


# ------------------------------------------------------------------------------------------------------------ the Trainer
def test_a_resumed_run_with_opacity_losses_continues_bit_for_bit(tmp_path, monkeypatch):
    """test_gpu_trainer's resumed-run test with MaskLoss and AlphaLossNV2(1e-4, 100, 1) on a ResidentSplit with mask tables: run A
    two epochs, run B one epoch and a resumed second; every parameter and both Adam moments agree exactly.  The alpha loss is
    off in epoch 0 and on in epoch 1 — in the resumed run too, whose AlphaLossNV2 is a fresh one: the Trainer sets its epoch."""
    import test_gpu_trainer as tg
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.model.loss import AlphaLossNV2, MaskLoss
    from pixel_nerf_multiscale_amd.render.autograd import AlphaLoss
    root = tmp_path / "srn"
    for stage, n_obj in (("train", 4), ("val", 2)):
        for o in range(n_obj):
            images = dt.boxed_views(tg.NV, tg.H, tg.W, [(2 + v, 3, 12, 13 - v - o % 2) for v in range(tg.NV)], seed=10 * o + (stage == "val"))
            poses = np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(tg.NV)]).astype(np.float32)
            poses[:, :, 1:3] *= -1.0
            dt.write_srn_object(str(root / f"cars_{stage}" / f"obj{o}"), images, poses, 16.5, 8.0, 8.0, ["000000", "000001", "000002"])
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    modes, real = [], AlphaLoss.apply

    def spy(*a):
        modes.append(a[3])
        return real(*a)

    monkeypatch.setattr(AlphaLoss, "apply", staticmethod(spy))
    losses = lambda: dict(mask_loss=MaskLoss(0.5, 0.5), alpha_loss=AlphaLossNV2(1e-4, 100, 1))
    try:
        train_set, _ = tg._datasets(str(root / "cars"), as_bytes=True)
        split = ResidentSplit(train_set, "cuda", device_masks=True)
        writer = tg.Writer()
        a = tg._trainer(str(tmp_path / "a"), split, None, writer=writer, **losses())
        a.start()
        assert modes == [2, 2, 2, 0, 2, 0]                  # four steps of the mask loss; the alpha loss joins in epoch 1
        tags = {t for t, _, _ in writer.scalars}
        assert {"train/m", "train/a", "train/t"} <= tags
        b1 = tg._trainer(str(tmp_path / "b"), split, None, num_epochs=1, **losses())
        b1.start()
        half = tg._state(b1)
        del modes[:]
        b2 = tg._trainer(str(tmp_path / "b"), split, None, resume=True, **losses())
        assert (b2.epoch, b2.global_step) == (1, 2)
        b2.start()
        assert modes == [2, 0, 2, 0] and b2.alpha_loss.active and int(b2.alpha_loss.epoch) == 1
        sa, sb = tg._state(a), tg._state(b2)
        assert sa[3] == 4 and sa[4] == 4
        tg._assert_same(sa, sb)
        assert not torch.equal(half[1], sa[1])
        # and the losses change the run: the same two epochs without them end elsewhere
        plain = tg._trainer(str(tmp_path / "p"), split, None)
        plain.start()
        assert not torch.equal(tg._state(plain)[1], sa[1])
    finally:
        torch.backends.cudnn.deterministic = was
