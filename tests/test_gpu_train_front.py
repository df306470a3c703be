"""Training front end on the device: pnr_train_batch (rays and colours of sampled pixels), pnr_rgb_loss / pnr_rgb_loss_bwd
(the trainer's loss) and train.calc_losses on top of them.

Bounds, none of them taken from what the kernels give:
  rays vs the reference fixture   2e-6, the bound test_gen_rays_kernel_matches_reference_fixture holds pnr_gen_rays to
  rays vs pnr_gen_rays, colours   bit-identical (same device functions; x * 0.5 is exact, so fmaf(x, 0.5, 0.5) = x * 0.5 + 0.5)
  loss value vs fp64              relative 1e-5: every term is non-negative, so the relative error is at most
                                  (additions on a term's path + 3) * 2^-24; 1e-5 allows ~160 additions, the kernel's path has
                                  n / 4096 + 23 (27 at 5000 rays).  A dropped tail row, n in place of 3n or a missing lambda
                                  moves the value by 1e-3 or more at these sizes.
  gradient vs fp64                1e-6 * max|d|: four roundings (2/n, the weight, x - gt, the product), 2.4e-7 relative
  calc_losses vs today's route    1e-5 * the tensor's max |gradient| (see test_calc_losses_end_to_end)
"""
import numpy as np
import pytest
import torch

import golden_util as gu
import hip_util as hu
from test_train_front_cpu import load_batch_fixture

pytestmark = pytest.mark.gpu

LOSS_SIZES = [1, 21, 64, 341, 342, 1025, 5000]     # both sides of a wave (192 elements), of a 1024-thread pass (1023 / 1026), of 4 | 3n
LAM_C, LAM_F = 0.7, 1.3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case1():
    fx = load_batch_fixture()["boxes_fxfy_c"]
    t = {k: torch.from_numpy(fx[k]) for k in ("images", "poses", "focal", "c")}
    return fx, t


# --------------------------------------------------------------------------------------------- pnr_train_batch
@pytest.mark.parametrize("name", ["boxes_fxfy_c", "uniform_scalar_f"])
def test_batch_kernel_matches_reference_fixture(name):
    from pixel_nerf_multiscale_amd import util
    fx = load_batch_fixture()[name]
    c = torch.from_numpy(fx["c"]) if fx["c"].size else None
    rays, rgb = util.train_batch(torch.from_numpy(fx["images"]).cuda(), torch.from_numpy(fx["poses"]).cuda(),
                                 torch.from_numpy(fx["focal"]), c, torch.from_numpy(fx["pix_inds"]).cuda(),
                                 float(fx["z"][0]), float(fx["z"][1]))
    assert tuple(rays.shape) == fx["rays"].shape and tuple(rgb.shape) == fx["rgb_gt"].shape
    assert np.array_equal(rgb.cpu().numpy(), fx["rgb_gt"])
    d = float(np.abs(rays.cpu().numpy() - fx["rays"]).max())
    print(f"{name}: max |rays - reference| = {d:.3e}")
    assert d <= 2e-6


@pytest.fixture(scope="module")
def camera_rays():
    """pnr_gen_rays for every camera of case 1: [o][v] -> (H*W, 8), computed once."""
    from pixel_nerf_multiscale_amd import util
    fx, t = _case1()
    SB, NV, _, H, W = fx["images"].shape
    zn, zf = float(fx["z"][0]), float(fx["z"][1])
    return [[util.gen_rays_device(t["poses"][o, v], W, H, t["focal"][o], zn, zf, c=t["c"][o]) for v in range(NV)]
            for o in range(SB)]


def _edge_indices(SB, NV, HW, B, seed):
    """First the pixels that sit on the edges of the index range: pixel 0 and HW-1 of every view, i.e. of the first and the
    last view and both sides of every view boundary; then seeded random ones.  Cut to B."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for o in range(SB):
        edge = [v * HW + p for v in range(NV) for p in (0, HW - 1)]
        rnd = torch.randint(0, NV * HW, (max(B, len(edge)),), generator=g).tolist()
        rows.append((edge + rnd)[:B] if o % 2 == 0 else (edge[::-1] + rnd)[:B])
    return torch.tensor(rows, dtype=torch.long)


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_batch_kernel_bit_identical_to_gen_rays(B, camera_rays):
    from pixel_nerf_multiscale_amd import util
    fx, t = _case1()
    SB, NV, _, H, W = fx["images"].shape
    HW = H * W
    inds = _edge_indices(SB, NV, HW, B, seed=B)
    if B >= 2 * NV:
        for o in range(SB):
            assert {v * HW + p for v in range(NV) for p in (0, HW - 1)} <= set(inds[o].tolist())
    rays, rgb = util.train_batch(t["images"].cuda(), t["poses"].cuda(), t["focal"], t["c"], inds.cuda(),
                                 float(fx["z"][0]), float(fx["z"][1]))
    rgb_all = (t["images"] * 0.5 + 0.5).permute(0, 1, 3, 4, 2).reshape(SB, NV * HW, 3)
    for o in range(SB):
        assert torch.equal(rgb[o].cpu(), rgb_all[o][inds[o]])
        for v in range(NV):
            sel = (inds[o] // HW) == v
            if sel.any():
                want = camera_rays[o][v][(inds[o][sel] % HW).cuda()]
                assert torch.equal(_bits(rays[o][sel.cuda()]), _bits(want)), (o, v)


def test_batch_kernel_guards_out_of_range_indices():
    """Indices outside [0, NV*H*W) — just outside and at the ends of int64 — read nothing and leave NaN rows; every other
    row is what a clean call gives, and the floats around both outputs stay untouched."""
    from pixel_nerf_multiscale_amd import _native as N
    fx, t = _case1()
    SB, NV, _, H, W = fx["images"].shape
    HW, B, PAD, CANARY = H * W, 65, 64, 12345.0
    good = _edge_indices(SB, NV, HW, B, seed=99)
    bad = good.clone()
    bad_at = {(0, 0): -1, (0, 7): NV * HW, (0, B - 1): 2 ** 63 - 1, (1, 3): -2 ** 63, (1, 64): NV * HW + 5, (1, 0): 2 ** 31}
    for (o, i), v in bad_at.items():
        bad[o, i] = v
    images, poses = t["images"].cuda(), t["poses"].cuda()
    focal, c = t["focal"].cuda().contiguous(), t["c"].cuda().contiguous()

    def run(inds):
        inds = inds.cuda()
        rbuf = torch.full((PAD + SB * B * 8 + PAD,), CANARY, device="cuda")
        gbuf = torch.full((PAD + SB * B * 3 + PAD,), CANARY, device="cuda")
        rc = N.lib.pnr_train_batch(N.ptr(images), N.ptr(poses), N.ptr(focal), N.ptr(c), SB, NV, W, H, float(fx["z"][0]),
                                   float(fx["z"][1]), inds.data_ptr(), B, rbuf.data_ptr() + 4 * PAD, gbuf.data_ptr() + 4 * PAD,
                                   N.current_stream(images.device))
        assert rc == 0
        torch.cuda.synchronize()
        for buf in (rbuf, gbuf):
            assert bool((buf[:PAD] == CANARY).all()) and bool((buf[-PAD:] == CANARY).all())
        return rbuf[PAD:-PAD].reshape(SB, B, 8).cpu(), gbuf[PAD:-PAD].reshape(SB, B, 3).cpu()

    rays0, rgb0 = run(good)
    rays1, rgb1 = run(bad)
    assert not torch.isnan(rays0).any() and not torch.isnan(rgb0).any()
    keep = torch.ones(SB, B, dtype=torch.bool)
    for (o, i) in bad_at:
        keep[o, i] = False
        assert torch.isnan(rays1[o, i]).all() and torch.isnan(rgb1[o, i]).all(), (o, i)
    assert torch.equal(_bits(rays1[keep]), _bits(rays0[keep])) and torch.equal(_bits(rgb1[keep]), _bits(rgb0[keep]))


# --------------------------------------------------------------------------------------------- pnr_rgb_loss
def _loss_inputs(n, seed=0):
    g = torch.Generator().manual_seed(1000 + n + seed)
    return tuple(torch.rand(n, 3, generator=g) for _ in range(3))       # coarse, fine, gt


def _loss_call(c, f, g, use_l1, d_total="skip", want=("c", "f")):
    """-> losses (3,), d_coarse, d_fine (device tensors; the gradients only when d_total != 'skip')."""
    from pixel_nerf_multiscale_amd import _native as N
    n = c.shape[0]
    s = N.current_stream(c.device)
    losses = torch.full((3,), -1.0, device="cuda")
    assert N.lib.pnr_rgb_loss(N.ptr(c), N.ptr(f), N.ptr(g), n, int(use_l1), LAM_C, LAM_F, N.ptr(losses), s) == 0
    if isinstance(d_total, str):
        return losses, None, None
    d_c = torch.full_like(c, 777.0) if "c" in want else None
    d_f = torch.full_like(f, 777.0) if (f is not None and "f" in want) else None
    assert N.lib.pnr_rgb_loss_bwd(N.ptr(c), N.ptr(f), N.ptr(g), n, int(use_l1), LAM_C, LAM_F, N.ptr(d_total), N.ptr(d_c),
                                  N.ptr(d_f), s) == 0
    return losses, d_c, d_f


def _loss_fp64(c, f, g, use_l1):
    lc, lf = float(np.float32(LAM_C)), float(np.float32(LAM_F))
    term = (lambda x: np.abs(x - g.double().numpy()).mean()) if use_l1 else (lambda x: ((x - g.double().numpy()) ** 2).mean())
    Lc = term(c.double().numpy())
    if f is None:
        return lc * Lc, 0.0, Lc
    Lf = term(f.double().numpy())
    return lc * Lc, lf * Lf, lc * Lc + lf * Lf


@pytest.mark.parametrize("n", LOSS_SIZES)
def test_loss_value_against_fp64(n):
    c, f, g = _loss_inputs(n)
    for use_l1 in (False, True):
        for fine in (True, False):
            got = _loss_call(c.cuda(), f.cuda() if fine else None, g.cuda(), use_l1)[0].cpu().double().numpy()
            want = _loss_fp64(c, f if fine else None, g, use_l1)
            rel = [abs(a - b) / b if b else abs(a) for a, b in zip(got, want)]
            print(f"n_rays={n} l1={use_l1} fine={fine}: rel err rc/rf/t = {rel[0]:.2e} {rel[1]:.2e} {rel[2]:.2e}")
            assert max(rel) <= 1e-5, (n, use_l1, fine, got, want)
            if fine:
                assert abs(got[2] - (got[0] + got[1])) <= 2.0 ** -23 * got[2]          # t = rc + rf, one rounding
            else:
                assert got[1] == 0.0
                assert abs(got[0] - float(np.float32(LAM_C)) * got[2]) <= 2.0 ** -23 * got[0]   # no lambda in total; rc = lambda_c * total


def test_loss_of_nothing_is_three_zeros():
    from pixel_nerf_multiscale_amd import _native as N
    x = torch.ones(4, 3, device="cuda")           # an empty tensor has no address to pass: any valid one, with n_rays = 0
    losses = torch.full((3,), -1.0, device="cuda")
    assert N.lib.pnr_rgb_loss(N.ptr(x), None, N.ptr(x), 0, 0, LAM_C, LAM_F, N.ptr(losses), N.current_stream(x.device)) == 0
    assert losses.cpu().tolist() == [0.0, 0.0, 0.0]


@pytest.mark.parametrize("n", LOSS_SIZES)
def test_loss_gradient_against_fp64(n):
    c, f, g = _loss_inputs(n)
    hit = torch.arange(0, 3 * n, 5)                       # elements exactly equal to the target: sign(0) = 0
    c.view(-1)[hit] = g.view(-1)[hit]
    one, k1024 = torch.ones(1, device="cuda"), torch.full((1,), 1024.0, device="cuda")
    lc, lf = float(np.float32(LAM_C)), float(np.float32(LAM_F))
    for use_l1 in (False, True):
        for fine in (True, False):
            cd, fd, gd = c.cuda(), (f.cuda() if fine else None), g.cuda()
            _, d_c, d_f = _loss_call(cd, fd, gd, use_l1, one)
            for x, d, w in ((c, d_c, lc if fine else 1.0), (f, d_f, lf)):
                if d is None:
                    continue
                r = x.double().numpy() - g.double().numpy()
                want = w * (np.sign(r) if use_l1 else 2.0 * r) / (3 * n)
                err = float(np.abs(d.cpu().double().numpy() - want).max())
                print(f"n_rays={n} l1={use_l1} fine={fine}: max |d - fp64| / max|d| = {err / np.abs(want).max():.2e}")
                assert err <= 1e-6 * np.abs(want).max(), (n, use_l1, fine)
            if use_l1:
                assert bool((d_c.view(-1)[hit.cuda()] == 0).all())
            _, s_c, s_f = _loss_call(cd, fd, gd, use_l1, k1024)           # a GradScaler scale: exact
            assert torch.equal(s_c, d_c * 1024) and (not fine or torch.equal(s_f, d_f * 1024))
            _, u_c, u_f = _loss_call(cd, fd, gd, use_l1, None)            # NULL d_total = 1
            assert torch.equal(_bits(u_c), _bits(d_c)) and (not fine or torch.equal(_bits(u_f), _bits(d_f)))
            _, o_c, o_f = _loss_call(cd, fd, gd, use_l1, one, want=("c",))   # NULL d_fine_rgb
            assert o_f is None and torch.equal(_bits(o_c), _bits(d_c))
            if fine:
                _, p_c, p_f = _loss_call(cd, fd, gd, use_l1, one, want=("f",))   # NULL d_coarse_rgb
                assert p_c is None and torch.equal(_bits(p_f), _bits(d_f))


def test_loss_is_bit_reproducible():
    c, f, g = (t.cuda() for t in _loss_inputs(5000))
    one = torch.ones(1, device="cuda")
    for use_l1 in (False, True):
        a = _loss_call(c, f, g, use_l1, one)
        b = _loss_call(c.clone(), f.clone(), g.clone(), use_l1, one)
        for x, y in zip(a, b):
            assert torch.equal(_bits(x), _bits(y))


def test_rgb_loss_function_under_autograd():
    """RGBLoss through autograd against torch's own criteria: 0-dim differentiable total, a stats buffer that is not, and a
    scaled backward (what GradScaler does) reaching the kernel through the gradient's device pointer."""
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    c, f, g = (t.reshape(2, -1, 3) for t in _loss_inputs(342))
    for use_l1 in (False, True):
        crit = torch.nn.L1Loss() if use_l1 else torch.nn.MSELoss()
        for fine in (True, False):
            cr, fr = c.clone().requires_grad_(True), f.clone().requires_grad_(True)
            ref = LAM_C * crit(cr, g) + LAM_F * crit(fr, g) if fine else crit(cr, g)
            (ref * 1024).backward()
            cd, fd = c.cuda().requires_grad_(True), f.cuda().requires_grad_(True)
            rd = {"coarse": {"rgb": cd}, "fine": {"rgb": fd} if fine else {}}
            total, stats = RenderLoss(LAM_C, LAM_F, use_l1)(rd, g.cuda())
            assert total.dim() == 0 and total.is_cuda and total.requires_grad
            assert tuple(stats.shape) == (3,) and stats.is_cuda and not stats.requires_grad
            (total * 1024).backward()
            assert abs(float(total.detach()) - float(ref.detach())) <= 1e-5 * float(ref.detach()) and float(stats[2]) == float(total.detach())
            for a, b in ((cd.grad, cr.grad), (fd.grad, fr.grad)) if fine else ((cd.grad, cr.grad),):
                assert float((a.cpu() - b).abs().max()) <= 1e-6 * float(b.abs().max())
            if not fine:
                assert fd.grad is None


# --------------------------------------------------------------------------------------------- train.calc_losses
Z_NEAR, Z_FAR, RAY_BATCH = 1.25, 2.75, 32


def _front_end_setup():
    """tiny_ns2_codeview's network in train mode (fp32 products), an encoder stand-in whose latent maps are a fixed function
    of the source images (so the choice of source views matters) and leaves of the graph (so their gradient can be read),
    and a loader-style batch: SB = 2 objects, NV = 4 views of 12 x 16 pixels, host tensors as a DataLoader gives them."""
    fx, spec, net, rend = hu.setup("tiny_ns2_codeview")
    net.train()
    net.train_precision = "fp32"
    rend.fixed_noise = None                 # the fixture's draws are sized for its own 16 rays: in-kernel generator here
    C_lat, Hl, Wl = spec["lat"][0]
    kept = []

    def encoder(images):
        pooled = torch.nn.functional.adaptive_avg_pool2d(images, (Hl, Wl))                 # (SB*NS, 3, Hl, Wl)
        maps = torch.relu(pooled.repeat(1, (C_lat + 2) // 3, 1, 1)[:, :C_lat] * 2.0 + 0.5).detach().requires_grad_(True)
        kept.append(maps)
        net.encoder.set_latents([maps])

    net.encoder.forward = encoder
    SB, NV, H, W = 2, 4, 12, 16
    rng = np.random.default_rng(77)
    data = {
        "images": torch.from_numpy(rng.uniform(-1, 1, (SB, NV, 3, H, W)).astype(np.float32)),
        "poses": torch.from_numpy(np.stack([np.stack([gu.pose_spherical(25.0 * v + 40.0 * o, -20.0 - 4.0 * v, spec["radius"])
                                                      for v in range(NV)]) for o in range(SB)])),
        "focal": torch.tensor([18.0, 19.5]),
        "c": torch.tensor([[8.25, 5.5], [7.5, 6.25]]),
        "bbox": torch.tensor([[[2.0, 1.0, 13.0, 10.0]] * NV, [[4.0, 3.0, 4.0, 3.0]] * NV]),      # object 1: one pixel per view
    }
    return net, rend, data, kept


def _grads(net, maps):
    out = {}
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        for k, p in mlp.named_parameters():
            out[f"{which}.{k}"] = p.grad.detach().clone()
            p.grad = None
    out["latent"] = maps.grad.detach().clone()
    return out


def _todays_route(net, rend, data, nviews):
    """calc_losses as the project could be driven before: the same host draws, rays from util.gen_rays over every view +
    indexing, colours by torch, rend(...), torch's criteria."""
    from pixel_nerf_multiscale_amd import util
    images, poses = data["images"].cuda(), data["poses"].cuda()
    SB, NV, _, H, W = images.shape
    curr = nviews[int(torch.randint(0, len(nviews), ()))]
    image_ord = torch.randint(0, NV, (SB, 1)) if curr == 1 else torch.empty((SB, curr), dtype=torch.long)
    rays, gts = [], []
    for o in range(SB):
        if curr > 1:
            image_ord[o] = torch.from_numpy(np.random.choice(NV, curr, replace=False))
        pix = util.bbox_sample(data["bbox"][o], RAY_BATCH)
        inds = (pix[:, 0] * H * W + pix[:, 1] * W + pix[:, 2]).cuda()
        cam = util.gen_rays(poses[o], W, H, data["focal"][o], Z_NEAR, Z_FAR, c=data["c"][o])
        rays.append(cam.reshape(-1, 8)[inds])
        gts.append((images[o] * 0.5 + 0.5).permute(0, 2, 3, 1).reshape(-1, 3)[inds])
    rays, gt = torch.stack(rays), torch.stack(gts)
    image_ord = image_ord.cuda()
    net.encode(util.batched_index_select_nd(images, image_ord), util.batched_index_select_nd(poses, image_ord),
               data["focal"].cuda(), c=data["c"].cuda())
    out = rend(net, rays, want_weights=True)
    mse = torch.nn.MSELoss()
    return LAM_C * mse(out.coarse.rgb, gt) + LAM_F * mse(out.fine.rgb, gt), rays, gt


@pytest.mark.parametrize("nviews", [[2], [1]])
def test_calc_losses_end_to_end(nviews):
    """Parameter and latent gradients of calc_losses(...)[0].backward() against today's route under the same seeds.
    Bound 1e-5 * the tensor's max |gradient|: the two d_rgb differ by at most 4 ulp and everything after them is the same
    deterministic kernels."""
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend, data, kept = _front_end_setup()
    render_par = rend.bind_parallel(net, None)

    torch.manual_seed(7); np.random.seed(7)
    loss, d = train.calc_losses(net, render_par, data, ray_batch_size=RAY_BATCH, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR,
                                loss=RenderLoss(LAM_C, LAM_F))
    assert loss.dim() == 0 and loss.is_cuda and net.num_views_per_obj == nviews[0] and net.num_objs == 2
    assert sorted(d) == ["rc", "rf", "t"] and all(v.is_cuda and v.dim() == 0 for v in d.values())
    assert len({v.untyped_storage().data_ptr() for v in d.values()}) == 1            # views of the one stats buffer
    loss.backward()
    got = _grads(net, kept[-1])
    rc, rf, t = (float(d[k]) for k in ("rc", "rf", "t"))
    assert abs(t - (rc + rf)) <= 2.0 ** -23 * t and t == float(loss.detach())

    torch.manual_seed(7); np.random.seed(7)
    ref_loss, _, _ = _todays_route(net, rend, data, nviews)
    ref_loss.backward()
    ref_loss = ref_loss.detach()
    want = _grads(net, kept[-1])
    print(f"nviews={nviews}: loss {t:.8g} vs today's route {float(ref_loss):.8g}")
    worst = 0.0
    for k in want:
        scale = float(want[k].abs().max())
        ratio = float((got[k] - want[k]).abs().max()) / scale
        worst = max(worst, ratio)
        print(f"  {k}: max |d grad| / max |grad| = {ratio:.3e}")
    print(f"nviews={nviews}: worst ratio {worst:.3e}")
    assert abs(t - float(ref_loss)) <= 1e-5 * float(ref_loss)
    for k in want:
        assert float((got[k] - want[k]).abs().max()) <= 1e-5 * float(want[k].abs().max()), k


def test_calc_losses_batches(monkeypatch):
    """What calc_losses hands the kernel and gets back: with boxes every pixel of object 1 is its one-pixel box; with
    is_train=False no box is consulted and the pixels are the uniform draws; either way each object's colours come from
    its OWN images (the object stride)."""
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend, data, kept = _front_end_setup()
    render_par = rend.bind_parallel(net, None)
    SB, NV, _, H, W = data["images"].shape
    seen, boxes_used = [], []
    real_batch, real_sample = util.train_batch, util.bbox_sample

    def spy_batch(images, poses, focal, c, pix_inds, z_near, z_far):
        out = real_batch(images, poses, focal, c, pix_inds, z_near, z_far)
        seen.append((pix_inds, *out))
        return out

    def spy_sample(bboxes, num_pix):
        boxes_used.append(1)
        return real_sample(bboxes, num_pix)

    monkeypatch.setattr(util, "train_batch", spy_batch)
    monkeypatch.setattr(util, "bbox_sample", spy_sample)
    kw = dict(ray_batch_size=RAY_BATCH, nviews=[2], z_near=Z_NEAR, z_far=Z_FAR, loss=RenderLoss(LAM_C, LAM_F))
    rgb_all = (data["images"] * 0.5 + 0.5).permute(0, 1, 3, 4, 2).reshape(SB, NV * H * W, 3)

    torch.manual_seed(11); np.random.seed(11)
    with torch.no_grad():
        train.calc_losses(net, render_par, data, **kw)
    inds, rays, gt = (x.cpu() for x in seen[-1])
    assert len(boxes_used) == SB and tuple(inds.shape) == (SB, RAY_BATCH)
    assert bool(((inds[1] % (H * W)) == 3 * W + 4).all()) and len(set((inds[0] % (H * W)).tolist())) > 8
    for o in range(SB):
        assert torch.equal(gt[o], rgb_all[o][inds[o]])
    assert not torch.equal(gt[0], gt[1])

    boxes_used.clear()
    torch.manual_seed(11); np.random.seed(11)
    with torch.no_grad():
        _, d = train.calc_losses(net, render_par, data, is_train=False, **kw)
    inds, rays, gt = (x.cpu() for x in seen[-1])
    assert not boxes_used
    torch.manual_seed(11)
    torch.randint(0, 1, ())                                 # curr_nviews
    for o in range(SB):
        assert torch.equal(inds[o], torch.randint(0, NV * H * W, (RAY_BATCH,)))
        assert torch.equal(gt[o], rgb_all[o][inds[o]])
    assert not bool(((inds[1] % (H * W)) == 3 * W + 4).all())
    # the same pixels asked of both objects: different images, different colours
    same = inds[:1].expand(SB, -1).contiguous().cuda()
    _, gt2 = real_batch(data["images"].cuda(), data["poses"].cuda(), data["focal"], data["c"], same, Z_NEAR, Z_FAR)
    assert torch.equal(gt2[1].cpu(), rgb_all[1][inds[0]]) and not torch.equal(gt2[0], gt2[1])


@pytest.mark.parametrize("nviews", [[2], [1]])
def test_calc_losses_forward_matches_the_oracle(nviews):
    """The route above compares calc_losses with the HIP path driven by hand.  Here the batch calc_losses drew — its rays, its
    source poses and its per-object focal (SB, 2) and c (SB, 2), as it handed them to net.encode — goes through orc.render
    with the same explicit noise (rend.fixed_noise): out.coarse.rgb within 1e-4, the bound test_gradients_match_reference
    holds the taped forward to."""
    import train_fp64_util as tu
    from oracle import pixelnerf_oracle as orc
    from oracle_util import maxdiff
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend, data, kept = _front_end_setup()
    spec = gu.CASES["tiny_ns2_codeview"]
    SB, NV, _, H, W = data["images"].shape
    noise = tu.make_noise(dict(spec, SB=SB, N=RAY_BATCH), 31)
    rend.fixed_noise = {k: v.cuda() for k, v in noise.items()}
    render_par = rend.bind_parallel(net, None)
    seen = {}
    real_encode = net.encode

    def spy_encode(images, poses, focal, z_bounds=None, c=None):
        seen.update(poses=poses.detach().cpu(), focal=focal.detach().cpu(), c=c.detach().cpu())
        return real_encode(images, poses, focal, z_bounds, c=c)

    def spy_render(rays, want_weights=True):
        out = render_par(rays, want_weights=want_weights)
        seen.update(rays=rays.detach().cpu(), out=out)
        return out

    net.encode = spy_encode
    torch.manual_seed(13); np.random.seed(13)
    train.calc_losses(net, spy_render, data, ray_batch_size=RAY_BATCH, nviews=nviews, z_near=Z_NEAR, z_far=Z_FAR,
                      loss=RenderLoss(LAM_C, LAM_F))
    NS = nviews[0]
    assert tuple(seen["poses"].shape) == (SB, NS, 4, 4) and tuple(seen["focal"].shape) == tuple(seen["c"].shape) == (SB, 2)
    assert torch.equal(seen["focal"], data["focal"][:, None].expand(SB, 2)) and torch.equal(seen["c"], data["c"])
    assert not torch.equal(seen["focal"][0], seen["focal"][1]) and not torch.equal(seen["c"][0], seen["c"][1])
    cam = orc.encode_cameras(seen["poses"], seen["focal"], seen["c"], W, H)
    sd = lambda mlp: {k: v.detach().cpu() for k, v in mlp.state_dict().items()}
    res = orc.render(sd(net.mlp_coarse), sd(net.mlp_fine), cam, [kept[-1].detach().cpu()], seen["rays"], NS, spec["Kc"], spec["Kf"],
                     spec["Kfd"], spec["depth_std"], spec["white_bkgd"], spec["lindisp"], noise,
                     use_code_viewdirs=spec["use_code_viewdirs"], n_blocks=spec["n_blocks"], combine_layer=spec["combine_layer"],
                     combine_type=spec["combine_type"])
    got = seen["out"]["coarse"]["rgb"].detach().cpu()
    d = maxdiff(got, res["coarse"]["rgb"])
    print(f"nviews={nviews}: max |coarse rgb - oracle| = {d:.3e}")
    assert tuple(got.shape) == (SB, RAY_BATCH, 3) and d <= 1e-4
