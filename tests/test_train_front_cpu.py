"""Training front end, host side: the pixel draws and index arithmetic against what the reference recorded
(tests/golden/train_batch.npz, written by tools/gen_golden_batch.py), the tensor helper, the argument checks of the three
entry points (made before any HIP call, so they run without a GPU) and the loss factory."""
import ast
import inspect
import os
import textwrap

import numpy as np
import pytest
import torch

import golden_util as gu


def load_batch_fixture():
    d = np.load(os.path.join(gu.GOLDEN_DIR, "train_batch.npz"))
    out = {}
    for name in str(d["names"]).split(","):
        out[name] = {k[len(name) + 2:]: d[k] for k in d.files if k.startswith(name + "__")}
    return out


def test_bbox_sample_draws_the_reference_pixels():
    from pixel_nerf_multiscale_amd import util
    fx = load_batch_fixture()["boxes_fxfy_c"]
    SB, NV, _, H, W = fx["images"].shape
    B = fx["pix"].shape[1]
    bboxes = torch.from_numpy(fx["bboxes"])
    torch.manual_seed(int(fx["seed"]))
    for o in range(SB):
        pix = util.bbox_sample(bboxes[o], B)
        assert pix.dtype == torch.long and tuple(pix.shape) == (B, 3)
        assert np.array_equal(pix.numpy(), fx["pix"][o])
        inds = pix[:, 0] * (H * W) + pix[:, 1] * W + pix[:, 2]
        assert np.array_equal(inds.numpy(), fx["pix_inds"][o])
    # the fixture holds what its description says: a single-pixel box is hit, every pixel lies in its view's box
    pix, box = fx["pix"], fx["bboxes"]
    for o in range(SB):
        b = box[o][pix[o][:, 0]]
        assert np.all((pix[o][:, 2] >= b[:, 0]) & (pix[o][:, 2] <= b[:, 2]) & (pix[o][:, 1] >= b[:, 1]) & (pix[o][:, 1] <= b[:, 3]))
    assert np.any((pix[0][:, 0] == 0) & (pix[0][:, 1] == 7) & (pix[0][:, 2] == 5))


def test_uniform_pixels_follow_the_seed():
    fx = load_batch_fixture()["uniform_scalar_f"]
    SB, NV, _, H, W = fx["images"].shape
    torch.manual_seed(int(fx["seed"]))
    for o in range(SB):
        assert np.array_equal(torch.randint(0, NV * H * W, (fx["pix_inds"].shape[1],)).numpy(), fx["pix_inds"][o])


def test_batched_index_select_nd_is_plain_indexing():
    from pixel_nerf_multiscale_amd import util
    g = torch.Generator().manual_seed(3)
    t = torch.randn(2, 5, 3, 4, 4, generator=g)
    inds = torch.tensor([[4, 0, 2], [1, 1, 3]])
    out = util.batched_index_select_nd(t, inds)
    assert tuple(out.shape) == (2, 3, 3, 4, 4)
    for b in range(2):
        for j in range(3):
            assert torch.equal(out[b, j], t[b, inds[b, j]])
    p = torch.randn(2, 5, 4, 4, generator=g)
    assert torch.equal(util.batched_index_select_nd(p, inds[:, :1]), torch.stack([p[0, 4:5], p[1, 1:2]]))


def test_entry_points_check_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    E_NULL, E_SHAPE = -1, -2
    p = 64          # a non-NULL value: the checks below return before anything dereferences or launches
    tb = lambda images=p, poses=p, focal=p, c=None, SB=1, NV=1, W=4, H=4, inds=p, B=8, rays=p, rgb=p: \
        L.pnr_train_batch(images, poses, focal, c, SB, NV, W, H, 0.1, 1.0, inds, B, rays, rgb, None)
    assert tb(poses=None) == E_NULL and tb(focal=None) == E_NULL and tb(inds=None) == E_NULL and tb(rays=None) == E_NULL
    assert tb(images=None) == E_NULL                      # colours wanted, no images
    assert tb(SB=0) == E_SHAPE and tb(NV=0) == E_SHAPE and tb(W=0) == E_SHAPE and tb(H=-1) == E_SHAPE and tb(B=-1) == E_SHAPE
    assert tb(NV=2, W=32768, H=32768) == E_SHAPE          # NV*H*W = 2^31
    assert tb(B=0) == 0                                   # nothing to do: no launch
    assert tb(images=None, rgb=None, B=0) == 0            # images may be NULL when no colours are asked for
    assert L.pnr_rgb_loss(None, None, p, 4, 0, 1.0, 1.0, p, None) == E_NULL
    assert L.pnr_rgb_loss(p, None, None, 4, 0, 1.0, 1.0, p, None) == E_NULL
    assert L.pnr_rgb_loss(p, None, p, 4, 0, 1.0, 1.0, None, None) == E_NULL
    assert L.pnr_rgb_loss(p, None, p, -1, 0, 1.0, 1.0, p, None) == E_SHAPE
    assert L.pnr_rgb_loss_bwd(None, None, p, 4, 0, 1.0, 1.0, None, p, None, None) == E_NULL
    assert L.pnr_rgb_loss_bwd(p, None, None, 4, 0, 1.0, 1.0, None, p, None, None) == E_NULL
    assert L.pnr_rgb_loss_bwd(p, None, p, 4, 0, 1.0, 1.0, None, p, p, None) == E_NULL      # d_fine without fine
    assert L.pnr_rgb_loss_bwd(p, None, p, -1, 0, 1.0, 1.0, None, p, None, None) == E_SHAPE
    assert L.pnr_rgb_loss_bwd(p, None, p, 0, 0, 1.0, 1.0, None, p, None, None) == 0


def test_get_rgb_loss_and_render_loss_surface():
    from pixel_nerf_multiscale_amd.model import loss
    assert isinstance(loss.get_rgb_loss({"use_l1": True}), torch.nn.L1Loss)
    assert isinstance(loss.get_rgb_loss({"use_l1": False}, coarse=False), torch.nn.MSELoss)
    assert isinstance(loss.get_rgb_loss({}), torch.nn.MSELoss)
    assert loss.get_rgb_loss({"use_l1": True}, reduction="none").reduction == "none"
    assert isinstance(loss.get_rgb_loss({"use_uncertainty": True}, coarse=True), torch.nn.MSELoss)
    with pytest.raises(NotImplementedError):
        loss.get_rgb_loss({"use_uncertainty": True}, coarse=False)
    r = loss.RenderLoss(0.7, 1.3, use_l1=True)
    assert (r.lambda_coarse, r.lambda_fine, r.use_l1) == (0.7, 1.3, True)


def test_calc_losses_never_waits_for_the_device():
    """No .item() / .cpu() / .tolist() / .numpy() / synchronize call in calc_losses, and none in what it runs per step
    on device data (make_batch, train_batch, RGBLoss, RenderLoss)."""
    from pixel_nerf_multiscale_amd import train, util
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    from pixel_nerf_multiscale_amd.render.autograd import RGBLoss
    banned = {"item", "cpu", "tolist", "numpy", "synchronize"}
    for fn in (train.calc_losses, train.make_batch, util.train_batch, RenderLoss.forward, RGBLoss.forward, RGBLoss.backward):
        tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
        called = {n.func.attr for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)}
        assert not (called & banned), (fn.__qualname__, called & banned)
