"""CPU self-checks of tests/train_fp64_util.py, the fp64 truth test_gpu_train_fp64.py holds the training backward to: the
exact-geometry lattice lands where it is planned, the oracle's lookup follows ATen's grid_sampler_2d at the borders, the ray
mask catches what it is for, and the comparison rules at the bounds used reject planted kernel defects."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import train_fp64_util as tu
from oracle import pixelnerf_oracle as orc

LATTICES = [((9, 5), tu.LATTICE_IMAGE, (1.0, 1.0)), ((5, 3), tu.LATTICE_IMAGE, (1.0, 1.0)), ((9, 5), (18, 10), (0.5, 0.5))]


@pytest.mark.parametrize("WH,image,scale", LATTICES)
def test_lattice_plan_lands_exactly(WH, image, scale):
    """float32 numpy in the kernels' order (rot3, project, the uv scale, bilinear_taps' normalisation): every planned point
    lands on its planned texel coordinate bit for bit, and the planned-behind points are behind the camera."""
    W, H = WH
    xyz, plan = tu.lattice_points(W, H, image=image, scale=scale)
    got = tu.kernel_texel_coords(xyz, tu.lattice_c2w(), tu.LATTICE_FOCAL, image, W, H, scale)
    front = ~np.isnan(plan[:, 0])
    assert front.sum() > 100 and (~front).sum() == 3
    assert (got[front, 2] == -2.0).all() and (got[~front, 2] > 0).all()
    assert np.array_equal(got[front, :2], plan[front])
    # every configuration the GPU test names is present: texel lines, borders and corners, outside
    ix, iy = plan[front, 0], plan[front, 1]
    for x in (0.0, W - 1.0):
        for y in (0.0, H - 1.0):
            assert ((ix == x) & (iy == y)).any()
    assert (ix < 0).any() and (ix > W - 1).any() and (iy < 0).any() and (iy > H - 1).any()
    assert ((ix == np.floor(ix)) & (ix > 0) & (ix < W - 1)).any()


def test_oracle_lookup_follows_grid_sample_at_the_borders():
    """The oracle's index_latent against fp64 F.grid_sample(align_corners=True, padding_mode="border") on the whole lattice:
    values and gradients (uv and map), borders included, where ATen drops the clip's gradient."""
    W, H = 9, 5
    _, plan = tu.lattice_points(W, H)
    plan = plan[~np.isnan(plan[:, 0])]
    rng = np.random.default_rng(0)
    lat = torch.from_numpy(rng.standard_normal((1, 6, H, W)))
    cot = torch.from_numpy(rng.standard_normal((1, 6, plan.shape[0])))
    uv_a = torch.from_numpy(plan)[None].clone().requires_grad_(True)
    lat_a = lat.clone().requires_grad_(True)
    a = orc.index_latent(uv_a, [lat_a])
    (a * cot).sum().backward()
    uv_b = torch.from_numpy(plan)[None].clone().requires_grad_(True)
    lat_b = lat.clone().requires_grad_(True)
    grid = torch.stack([uv_b[..., 0] / (W - 1) * 2 - 1, uv_b[..., 1] / (H - 1) * 2 - 1], -1)[:, None]      # (1,1,P,2)
    b = F.grid_sample(lat_b, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, :, 0]
    (b * cot).sum().backward()
    assert torch.allclose(a, b, rtol=0, atol=1e-12)
    assert torch.allclose(uv_a.grad, uv_b.grad, rtol=0, atol=1e-12)
    assert torch.allclose(lat_a.grad, lat_b.grad, rtol=0, atol=1e-12)
    on_border = torch.from_numpy((plan[:, 0] == 0) | (plan[:, 0] == W - 1))
    assert bool((uv_a.grad[0, on_border, 0] == 0).all())


def test_ray_mask_catches_a_bin_flip_and_a_depth_near_tie():
    rng = np.random.default_rng(1)
    n, Kc, Kimp, Kfd = 6, 16, 8, 4
    near, far = np.full(n, 1.0), np.full(n, 3.0)
    zc = np.sort(rng.random((n, Kc)) * 2 + 1, -1)
    zi = np.sort(rng.random((n, Kimp)) * 2 + 1, -1)
    d64 = rng.random(n) * 1.5 + 1.25
    dh = d64 + 1e-6
    raw = d64[:, None] + rng.standard_normal((n, Kfd)) * 0.2
    raw[2, 1] = zc[2, 5] + 2e-6                          # a depth sample 2e-6 from a coarse sample, |d depth| = 1e-6
    raw[4, 0] = far[4] + 1e-6                            # where the clamp starts
    zd = np.clip(raw, 1.0, 3.0)
    z64 = np.sort(np.concatenate([zc, zi, zd], -1), -1)
    zh = z64.copy()
    zh[3, 7] += 0.05                                     # an importance sample in another bin
    zh = np.sort(zh, -1)
    keep = tu.ray_mask(zh, z64, dh, d64, raw, np.concatenate([zc, zi], -1), near, far, False)
    assert not keep[2] and not keep[3] and not keep[4]
    assert keep[[0, 1, 5]].all()
    keep_l = tu.ray_mask(zh, z64, d64, d64, None, None, near, far, True)     # lindisp compares 1/z
    assert not keep_l[3] and keep_l[[0, 1, 2, 4, 5]].all()


# ----------------------------------------------------------------------------- planted defects
def _small_points(NS=1, P=600, lat=(8, 5, 7), combine="average", seed=3):
    spec = gu._case(seed=seed, d_hidden=32, lat=[lat], NS=NS, SB=1, combine_type=combine, image=(40, 30), focal=45.0)
    rays, poses = gu.make_inputs(dict(spec, N=P))
    rng = np.random.default_rng(seed)
    t = 1.25 + 1.5 * rng.random((P, 1))
    xyz = (rays[0, :, :3] + t * rays[0, :, 3:6])[None].astype(np.float32)
    dirs = rays[0, :, 3:6][None].copy()
    cot = rng.standard_normal((1, P, 4)).astype(np.float32)
    return spec, poses, gu.make_latents(spec), xyz, dirs, cot


def test_full_compare_rejects_a_dropped_lds_block():
    spec, poses, maps, xyz, dirs, cot = _small_points()
    _, truth = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, cot)
    assert tu.full_compare(truth, truth, 5e-4)["latent.0"] == 0
    c2 = cot.copy()
    c2[:, 256:512] = 0                                    # the second 256-point block's partial map lost in the reduction
    _, dropped = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, c2)
    with pytest.raises(AssertionError, match="latent.0"):
        tu.full_compare({**truth, "latent.0": dropped["latent.0"]}, truth, 5e-4)


def test_l2_rule_with_the_fp32_restatement_rejects_planted_defects(monkeypatch):
    """l2_compare as the whole-step and route tests use it (5e-4, or 4x the fp32 restatement's distance from fp64): the fp32
    restatement itself passes; a dropped 256-point block and view-max ties sent to the last view do not."""
    spec, poses, maps, xyz, dirs, cot = _small_points(NS=3, P=600, combine="max")
    poses[:, 2] = poses[:, 0]
    maps[0][2] = maps[0][0]
    _, truth = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, cot)
    _, ref32 = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, cot, dtype=torch.float32)
    tu.l2_compare(ref32, truth, 5e-4, ref32=ref32)
    c2 = cot.copy()
    c2[:, 256:512] = 0
    _, dropped = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, c2)
    with pytest.raises(AssertionError, match="latent.0"):
        tu.l2_compare({**truth, "latent.0": dropped["latent.0"]}, truth, 5e-4, ref32=ref32)
    monkeypatch.setattr(orc, "resnetfc", _resnetfc_last_tie)
    _, wrong = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, cot)
    with pytest.raises(AssertionError, match="latent.0"):
        tu.l2_compare(wrong, truth, 5e-4, ref32=ref32)


def _resnetfc_last_tie(sd, zx, d_latent, NS, P, n_blocks=5, combine_layer=3, combine_type="average"):
    """orc.resnetfc with the view-max tie sent to the LAST view (the defect)."""
    lin = lambda x, k: torch.addmm(sd[k + ".bias"], x, sd[k + ".weight"].t())
    z, x = zx[:, :d_latent], zx[:, d_latent:]
    x = lin(x, "lin_in")
    for b in range(n_blocks):
        if b == combine_layer and NS > 1:
            x = x.reshape(-1, NS, P, x.shape[-1]).flip(1).max(dim=1)[0].reshape(-1, x.shape[-1])
        if b < combine_layer:
            x = x + lin(z, f"lin_z.{b}")
        x = x + lin(torch.relu(lin(torch.relu(x), f"blocks.{b}.fc_0")), f"blocks.{b}.fc_1")
    return lin(torch.relu(x), "lin_out")


def test_full_compare_rejects_max_ties_sent_to_the_last_view(monkeypatch):
    spec, poses, maps, xyz, dirs, cot = _small_points(NS=3, P=200, combine="max")
    poses[:, 2] = poses[:, 0]
    maps[0][2] = maps[0][0]
    _, truth = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, cot)
    assert not truth["latent.0"][2].any() and truth["latent.0"][0].any()
    monkeypatch.setattr(orc, "resnetfc", _resnetfc_last_tie)
    _, wrong = tu.point_grads_fp64(spec, poses, maps, xyz, dirs, cot)
    with pytest.raises(AssertionError, match="latent.0"):
        tu.full_compare(wrong, truth, 5e-4)


def test_full_compare_rejects_the_clamp_gradient_at_a_border(monkeypatch):
    spec = gu._case(seed=5, d_hidden=32, lat=[(8, 5, 9)], NS=1, SB=1, image=tu.LATTICE_IMAGE, focal=tu.LATTICE_FOCAL)
    xyz, plan = tu.lattice_points(9, 5)
    P = xyz.shape[0]
    dirs = np.tile(np.array([[0.0, 0.6, -0.8]], np.float32), (1, P, 1))
    cot = np.random.default_rng(2).standard_normal((1, P, 4)).astype(np.float32)
    poses = tu.lattice_c2w()[None, None]
    maps = gu.make_latents(spec)
    _, truth = tu.point_grads_fp64(spec, poses, maps, xyz[None], dirs, cot)
    def clamp_rule(uv, latents):        # the oracle's lookup before the border fix: torch.clamp, gradient 1 at a bound
        outs = []
        for lat in latents:
            B, C, H, W = lat.shape
            ix, iy = torch.clamp(uv[:, :, 0], 0, W - 1), torch.clamp(uv[:, :, 1], 0, H - 1)
            x0, y0 = torch.floor(ix), torch.floor(iy)
            flat, acc = lat.reshape(B, C, H * W), 0.0
            for xx, yy, ww in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                               (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
                inb = (xx <= W - 1) & (yy <= H - 1)
                i = (torch.where(inb, yy, 0 * yy) * W + torch.where(inb, xx, 0 * xx)).long()[:, None, :].expand(-1, C, -1)
                acc = acc + torch.gather(flat, 2, i) * (ww * inb)[:, None, :]
            outs.append(acc)
        return torch.cat(outs, 1)

    monkeypatch.setattr(orc, "index_latent", clamp_rule)
    _, wrong = tu.point_grads_fp64(spec, poses, maps, xyz[None], dirs, cot)
    monkeypatch.undo()
    border = (plan[:, 0] == 0) | (plan[:, 0] == 8) | (plan[:, 1] == 0) | (plan[:, 1] == 4)
    assert np.abs(wrong["xyz"][0, border] - truth["xyz"][0, border]).max() > 0
    with pytest.raises(AssertionError, match="xyz"):
        tu.full_compare(wrong, truth, 5e-4)


# ----------------------------------------------------------------------------- the ReLU-margin mask
@pytest.mark.parametrize("name", list(tu.MARGIN_CASES))
def test_relu_margin_mask_stays_under_the_cap_and_removes_the_events(name):
    """Every case of test_several_views_match_fp64_at_every_entry, oracle in fp64 and fp32 only: at most 5 % of the points
    masked, and the masked fp32 restatement within 1e-5 of fp64 at every entry of every gradient (with 5e-4 to spend, a
    kernel's own error is what is left to see)."""
    for P in tu.MARGIN_POINTS:
        c = tu.margin_case(name, P)
        args = (c["spec"], c["poses"], c["maps"], c["xyz"], c["dirs"])
        keep = tu.relu_margin_mask(*args, uv_scale=c["uvs"])
        assert keep.shape == c["cot"].shape[:2]
        assert int((~keep).sum()) <= tu.MASK_MAX_FRACTION * keep.size, (name, P, int((~keep).sum()))
        cot = tu.mask_points(c["cot"], keep)
        _, truth = tu.point_grads_fp64(*args, cot, uv_scale=c["uvs"])
        _, ref32 = tu.point_grads_fp64(*args, cot, uv_scale=c["uvs"], dtype=torch.float32)
        tu.full_compare(ref32, truth, 1e-5, f"{name} P {P}")


@functools.lru_cache(maxsize=None)
def _four_views():
    """(256, 8, 9), four views, 1001 points per object: (case, args, keep, masked cotangent, fp64 (out, grads, d(zx))); shared,
    so read-only."""
    c = tu.margin_case("fix_ns4", 1001)
    args = (c["spec"], c["poses"], c["maps"], c["xyz"], c["dirs"])
    keep = tu.relu_margin_mask(*args)
    cot = tu.mask_points(c["cot"], keep)
    return c, args, keep, cot, tu.point_grads_fp64(*args, cot, stages=True)


def test_without_the_mask_the_fp32_restatement_is_not_within_1e_5():
    """The mask is what removes the events: the same four-view run with every cotangent row fails the 1e-5 rule."""
    c = tu.margin_case("fix_ns4", 1001)
    args = (c["spec"], c["poses"], c["maps"], c["xyz"], c["dirs"])
    _, truth = tu.point_grads_fp64(*args, c["cot"])
    _, ref32 = tu.point_grads_fp64(*args, c["cot"], dtype=torch.float32)
    with pytest.raises(AssertionError):
        tu.full_compare(ref32, truth, 1e-5)


def test_argmax_rule_masks_a_near_tie_of_the_view_maximum():
    """combine_type "max" with views 0 and 2 sharing pose and map: every unit of the parked stream ties, so every point is
    masked by the argmax rule; the same inputs under "average" keep nearly all."""
    spec, poses, maps, xyz, dirs, _ = _small_points(NS=3, P=50, combine="max")
    poses[:, 2] = poses[:, 0]
    maps[0][2] = maps[0][0]
    info = {}
    keep = tu.relu_margin_mask(spec, poses, maps, xyz, dirs, info=info)
    assert not keep.any() and info["argmax"] > 0
    assert tu.relu_margin_mask(dict(spec, combine_type="average"), poses, maps, xyz, dirs).sum() > 40


def test_latent_scatter_is_the_lookups_adjoint_on_absolute_values():
    """latent_scatter's sum |g w| against autograd through the oracle's lookup with |g| as cotangent, and its counts
    where it is zero; three levels with uv_scale, points on and beyond the borders."""
    rng = np.random.default_rng(6)
    lat, B, P = [(3, 16, 16), (2, 8, 8), (4, 5, 9)], 2, 200
    uv = rng.random((B, P, 2)) * 40 - 4
    uvs = [(0.5, 0.5), (0.25, 0.25), (0.25, 0.125)]
    g = rng.standard_normal((B * P, 9 + 5))
    got = tu.latent_scatter(g, uv, lat, uvs)
    c0 = 0
    for (C, H, W), s, (tot, cnt) in zip(lat, uvs, got):
        m = torch.zeros(B, C, H, W, dtype=tu.F64, requires_grad=True)
        o = orc.index_latent(torch.from_numpy(uv) * torch.tensor(s, dtype=tu.F64), [m])              # (B, C, P)
        (o * torch.from_numpy(np.abs(g[:, c0:c0 + C])).reshape(B, P, C).transpose(1, 2)).sum().backward()
        assert np.allclose(tot, m.grad.numpy(), rtol=0, atol=1e-12)
        assert cnt.sum() <= 4 * B * P and cnt.min() >= 0 and ((cnt[:, 0] > 0) == (tot.max(axis=1) > 0)).all()
        c0 += C


def _view_mean_scaled(rows, NS_scale):
    """orc.resnetfc with the view mean's backward multiplied by NS_scale on the given rows of the reduced stream (the
    forward unchanged): k_combine_bwd leaving out 1 / NS there."""
    def net(sd, zx, d_latent, NS, P, n_blocks=5, combine_layer=3, combine_type="average"):
        lin = lambda x, k: torch.addmm(sd[k + ".bias"], x, sd[k + ".weight"].t())
        z, x = zx[:, :d_latent], zx[:, d_latent:]
        x = lin(x, "lin_in")
        for b in range(n_blocks):
            if b == combine_layer and NS > 1:
                x = x.reshape(-1, NS, P, x.shape[-1]).mean(dim=1).reshape(-1, x.shape[-1])
                extra = torch.zeros(x.shape[0], 1, dtype=x.dtype)
                extra[rows] = NS_scale - 1.0
                x = x + (x - x.detach()) * extra         # + 0 exactly; the gradient times 1 + extra
            if b < combine_layer:
                x = x + lin(z, f"lin_z.{b}")
            x = x + lin(torch.relu(lin(torch.relu(x), f"blocks.{b}.fc_0")), f"blocks.{b}.fc_1")
        return lin(torch.relu(x), "lin_out")
    return net


def test_every_entry_rule_under_the_mask_rejects_view_and_block_mutants(monkeypatch):
    """full_compare at 5e-4 on the masked four-view case, truth against truth with one planted defect each (applied to the
    fp64 gradients on the CPU): one view's scatter landing in the next view's map; one view's contributions dropped; the view
    mean's 1 / NS missing on one 256-thread block of k_combine_bwd (4 points at d_hidden 64); the last 4 points of an object
    (the last block of k_features_bwd's (P + 3) / 4 grid) dropped."""
    c, args, keep, cot, (_, truth, dzx) = _four_views()
    SB, NS, P = c["spec"]["SB"], c["spec"]["NS"], 1001
    assert tu.full_compare(truth, truth, 5e-4)["latent.0"] == 0
    g = truth["latent.0"].reshape(SB, NS, *truth["latent.0"].shape[1:])
    moved = g.copy()
    moved[1, 3] += moved[1, 2]
    moved[1, 2] = 0
    dropped = g.copy()
    dropped[2, 1] = 0
    for what, bad in (("moved", moved), ("dropped", dropped)):
        with pytest.raises(AssertionError, match="latent.0"):
            tu.full_compare({**truth, "latent.0": bad.reshape(truth["latent.0"].shape)}, truth, 5e-4, what)
    # the last 4 points of object 1 that carry a cotangent: every gradient that sums over points notices, d(xyz) has the rows themselves
    live = np.flatnonzero(keep[1])[-4:]
    c2 = cot.copy()
    c2[1, live] = 0
    _, short = tu.point_grads_fp64(*args, c2)
    with pytest.raises(AssertionError) as e:
        tu.full_compare(short, truth, 5e-4)
    assert "latent.0" in str(e.value) and "xyz" in str(e.value) and "lin_z.0.weight" in str(e.value)
    # 1 / NS missing on the block of points 1001 + 4 .. 1001 + 7 of the reduced stream (kept ones)
    rows = P + np.flatnonzero(keep[1])[4:8]
    monkeypatch.setattr(orc, "resnetfc", _view_mean_scaled(torch.from_numpy(rows), float(NS)))
    _, unscaled = tu.point_grads_fp64(*args, cot)
    monkeypatch.undo()
    for k in ("coarse.blocks.3.fc_0.weight", "coarse.lin_out.weight"):        # behind the reduction: untouched
        assert np.array_equal(unscaled[k], truth[k])
    with pytest.raises(AssertionError) as e:
        tu.full_compare(unscaled, truth, 5e-4)
    assert "latent.0" in str(e.value) and "lin_z.0.weight" in str(e.value)


def test_every_entry_rule_rejects_a_fixed_point_sum_that_wraps():
    """The four-view case's own contributions g w (fp32 d(zx) rows times the fp64 taps' weights) through fixed_point_sum.
    k_latq_scale's s = 61 - ex - ceil(log2 n_terms) keeps two bits of headroom, so with at most n_terms contributions of
    |g w| < 2^ex per entry a scale two bits larger is the last that cannot wrap: it must still pass.  What n_terms guards is
    the case of every contribution to an entry having one sign and the largest magnitude; with that entry planted (n_terms
    contributions of max |g|), a scale two bits beyond what n_terms allows (s + 4) wraps the entry and is rejected, and so
    is n_terms understated 16-fold (MV / 4 for 4 MV)."""
    c, args, keep, cot, (_, truth, dzx) = _four_views()
    spec = c["spec"]
    C, H, W = spec["lat"][0]
    with torch.no_grad():
        uv = tu.point_forward_oracle(*args)[1]["uv"].numpy()
    B, P = uv.shape[:2]
    ix, iy = np.clip(uv[..., 0], 0, W - 1), np.clip(uv[..., 1], 0, H - 1)
    x0, y0 = np.floor(ix), np.floor(iy)
    g32 = dzx[:, :C].astype(np.float32).reshape(B, P, C)
    contrib, index = [], []
    for xx, yy, ww in ((x0, y0, (x0 + 1 - ix) * (y0 + 1 - iy)), (x0 + 1, y0, (ix - x0) * (y0 + 1 - iy)),
                       (x0, y0 + 1, (x0 + 1 - ix) * (iy - y0)), (x0 + 1, y0 + 1, (ix - x0) * (iy - y0))):
        live = (xx <= W - 1) & (yy <= H - 1) & (ww != 0)
        b, p = np.nonzero(live)
        tex = (yy[b, p] * W + xx[b, p]).astype(np.int64)
        contrib.append((g32[b, p] * ww[b, p].astype(np.float32)[:, None]).reshape(-1))
        index.append(((b[:, None] * C + np.arange(C)[None]) * (H * W) + tex[:, None]).reshape(-1))
    contrib, index = np.concatenate(contrib), np.concatenate(index)
    n_terms = 4 * B * P
    gmax = float(np.abs(g32).max())
    s = tu.latq_scale_bits(gmax, n_terms)
    t = truth["latent.0"].reshape(-1)
    for bits in (0, 2):
        got = tu.fixed_point_sum(contrib, index, t.size, s + bits)
        assert tu.full_compare({"m": got}, {"m": t}, 5e-4)["m"] < 1e-5
    # the guarded case: entry 0 receives n_terms contributions of + max |g|
    free = index != 0
    contrib = np.concatenate([contrib[free], np.full(n_terms, gmax, np.float32)])
    index = np.concatenate([index[free], np.zeros(n_terms, np.int64)])
    t = np.zeros_like(t)
    np.add.at(t, index, contrib.astype(np.float64))
    rest = np.arange(t.size) != 0
    for bits, n in ((0, n_terms), (2, n_terms)):
        got = tu.fixed_point_sum(contrib, index, t.size, tu.latq_scale_bits(gmax, n) + bits)
        assert abs(got[0] - t[0]) <= 1e-6 * t[0]
        assert tu.full_compare({"m": got[rest]}, {"m": t[rest]}, 5e-4)["m"] < 1e-5
    for bits, n in ((4, n_terms), (0, n_terms // 16)):
        got = tu.fixed_point_sum(contrib, index, t.size, tu.latq_scale_bits(gmax, n) + bits)
        with pytest.raises(AssertionError):
            tu.full_compare({"m": got}, {"m": t}, 5e-4)


def test_depth_bound_rejects_the_neighbouring_slot_of_a_tie():
    """depth_std 0: every depth sample of a ray ties; d(depth) = the sum of d(z_sorted) over the tied slots, in any order.
    Reading one tied sample's gradient from the slot next to the run fails the 1e-6 sum|terms| bound."""
    rng = np.random.default_rng(4)
    B, Kc, Kfd = 8, 16, 5
    zc = np.sort(rng.random((B, Kc)) * 2 + 1, -1)
    depth = torch.from_numpy(rng.random(B) * 1.5 + 1.25).requires_grad_(True)
    zd = depth[:, None].expand(B, Kfd)
    z, idx = torch.sort(torch.cat([torch.from_numpy(zc), zd], -1), -1)
    dz = torch.from_numpy(rng.standard_normal((B, Kc + Kfd)))
    (z * dz).sum().backward()
    slots = torch.argsort(idx, -1)[:, Kc:]                   # the tied run
    terms = torch.gather(dz, 1, slots).abs().sum(-1)
    right = torch.gather(dz, 1, slots).sum(-1)
    assert tu.depth_grad_ok(right, depth.grad, terms)
    wrong_slots = slots.clone()
    wrong_slots[:, -1] = (slots.max(-1).values + 1).clamp_max(Kc + Kfd - 1)
    wrong_slots[slots.max(-1).values == Kc + Kfd - 1, -1] = slots.min(-1).values[slots.max(-1).values == Kc + Kfd - 1] - 1
    wrong = torch.gather(dz, 1, wrong_slots).sum(-1)
    assert not tu.depth_grad_ok(wrong, depth.grad, terms)


def test_resolution_bound_rejects_a_scale_off_by_one_bit():
    """The fixed-point route in numpy (k_latq_scale's s, 64-bit sums): within n_terms 2^-s of the fp64 sum, with one
    contribution 2^20 times the rest; the same sums finalised with 2^-(s+1) or 2^-(s-1) are rejected."""
    rng = np.random.default_rng(5)
    n_out, m = 300, 4000
    c = rng.standard_normal(m).astype(np.float32)
    c[7] *= np.float32(2.0 ** 20)
    idx = rng.integers(0, n_out, m)
    idx[7] = 0
    truth = np.zeros(n_out)
    np.add.at(truth, idx, c.astype(np.float64))
    s = tu.latq_scale_bits(float(np.abs(c).max()), m)
    got = tu.fixed_point_sum(c, idx, n_out, s)
    small = np.ones(n_out, bool)
    small[0] = False
    assert np.abs(got - truth).max() <= m * 2.0 ** -s
    assert tu.full_compare({"m": got[small]}, {"m": truth[small]}, 5e-4)["m"] < 1e-6
    for off in (1, -1):
        bad = got * 2.0 ** -off
        with pytest.raises(AssertionError):
            tu.full_compare({"m": bad[small]}, {"m": truth[small]}, 5e-4)
