"""Approximate evaluation on the device (pnr_eval_frames / util.eval_frames / evalio.evaluate_approx): the batched metrics
against the one-frame entry (bit for bit when clamped) and against the host functions that define the project's numbers on the
UNclamped arrays (evalio.psnr, evalio.ssim; SSIM is this project's restatement of skimage, parity unpinned), the isolation of
the frames of a call, and the loop end to end with both back ends.  Run with -s for the measured differences.

Bounds, those of tests/test_gpu_eval_back.py (fixed by the formats, none by what the kernel gives): SSIM |d| <= 1e-6,
PSNR |d| <= 2e-5 dB."""
import functools
import math

import numpy as np
import pytest
import torch

from eval_util import make_dataset, sync_debug_mode_works
from test_gpu_eval_back import PSNR_TOL, SSIM_TOL, _frame, _g01

pytestmark = pytest.mark.gpu

SIZES = [(7, 7), (8, 23), (37, 23)]          # (H, W): one window, one ragged tile, ragged tiles in both directions
CONTENTS = ["noise", "white", "disc"]        # frame f of a call has content f: the frames differ


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


def _frames(H, W, F):
    """-> rgb (F, H, W, 3) UNclamped, gt (F, 3, H, W), frame f of content CONTENTS[f]."""
    pairs = [_frame(H, W, CONTENTS[f]) for f in range(F)]
    return torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()


def _noise_frames(H, W, F=3):
    """F frames of the "noise" recipe of tests/test_gpu_eval_back.py — g uniform in [0, 1], render = g + 0.05 N(0, 1), which
    leaves [0, 1] here and there — from seeds of this file's own: that file's 7 x 7 noise frame happens to stay inside [0, 1],
    where clamping changes nothing (the test below asserts on the host numbers that every frame used here is not of that kind)."""
    xs, gts = [], []
    for k in range(F):
        rng = np.random.default_rng(1000 * H + W + 100003 + 7919 * (k + 1))
        g01 = rng.random((H, W, 3))
        x = g01 + 0.05 * rng.standard_normal((H, W, 3))
        xs.append(torch.from_numpy(x.astype(np.float32)))
        gts.append(torch.from_numpy((g01.transpose(2, 0, 1) * 2.0 - 1.0).astype(np.float32)))
    return torch.stack(xs).contiguous(), torch.stack(gts).contiguous()


@functools.lru_cache(maxsize=None)
def _host_numbers(H, W):
    """Per noise frame ((psnr, ssim) on the raw arrays, (psnr, ssim) on the clamped ones), by the host functions, once."""
    from pixel_nerf_multiscale_amd import evalio
    x, gt = _noise_frames(H, W)
    out = []
    for f in range(x.shape[0]):
        raw, g = x[f].numpy(), _g01(gt[f])
        clamped = np.clip(raw, 0.0, 1.0)
        out.append(((float(evalio.psnr(raw, g)), float(evalio.ssim(raw, g))),
                    (float(evalio.psnr(clamped, g)), float(evalio.ssim(clamped, g)))))
    return out


def _psnr(mse):
    return float("inf") if mse == 0.0 else 10.0 * math.log10(1.0 / mse)


@pytest.mark.parametrize("layout", ["dense", "record", "gap"])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_clamped_frames_are_bit_identical_to_the_one_frame_entry(H, W, F, layout):
    from pixel_nerf_multiscale_amd import util
    x, gt = _frames(H, W, F)
    gt_d = gt.cuda()
    want = torch.stack([util.eval_frame(x[f].cuda(), gt=gt_d[f], want_u8=False)[3] for f in range(F)])
    if layout == "dense":
        rgb = x.cuda()
        assert torch.equal(_bits(util.eval_frames(rgb.reshape(F, H * W, 3), gt_d, clamp=True)), _bits(want))     # the (F, H*W, 3) form
    elif layout == "record":                                         # a stride-4 view of the packed (N, 4) per-ray record
        rec = torch.full((F * H * W, 4), float("nan"))
        rec[:, :3] = x.reshape(-1, 3)
        rgb = rec.cuda().view(F, H, W, 4)[..., :3]
        assert rgb.stride() == (4 * H * W, 4 * W, 4, 1) and not rgb.is_contiguous()
    else:                                                            # frames apart by more than a frame, NaN in between
        n = H * W * 3
        buf = torch.full((F, n + 5), float("nan"))
        buf[:, :n] = x.reshape(F, n)
        rgb = buf.cuda()[:, :n].unflatten(1, (H, W, 3))
        assert rgb.stride()[1:] == (3 * W, 3, 1) and (F == 1 or rgb.stride(0) == n + 5)      # torch normalises the stride of a size-1 dim
    got = util.eval_frames(rgb, gt_d, clamp=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (F, 2) and got.is_cuda
    assert not torch.isnan(got).any()
    assert torch.equal(_bits(got), _bits(want)), (got.cpu(), want.cpu())
    out = torch.full((F + 1, 2), -1.0, dtype=torch.float64, device="cuda")
    assert util.eval_frames(rgb, gt_d, clamp=True, metrics_out=out[:F]) is not None
    assert torch.equal(_bits(out[:F]), _bits(want)) and (out[F] == -1.0).all()      # metrics_out: those rows and no other


@pytest.mark.parametrize("H,W", SIZES)
def test_unclamped_frames_match_the_host_functions_on_the_raw_arrays(H, W):
    from pixel_nerf_multiscale_amd import util
    host = _host_numbers(H, W)
    for f, ((p_raw, s_raw), (p_cl, s_cl)) in enumerate(host):        # the case has teeth: the two modes are far apart
        print(f"eval_approx {H}x{W} noise frame {f}: host raw {p_raw:.4f} dB {s_raw:.8f}, clamped {p_cl:.4f} dB {s_cl:.8f}")
        assert abs(p_raw - p_cl) > 100 * PSNR_TOL and abs(s_raw - s_cl) > 100 * SSIM_TOL, (f, host[f])
    x, gt = _noise_frames(H, W)
    got = util.eval_frames(x.cuda(), gt.cuda(), clamp=False).cpu().tolist()
    got_cl = util.eval_frames(x.cuda(), gt.cuda(), clamp=True).cpu().tolist()
    for f, ((p_raw, s_raw), (p_cl, s_cl)) in enumerate(host):
        d_psnr, d_ssim = abs(_psnr(got[f][0]) - p_raw), abs(got[f][1] - s_raw)
        print(f"eval_approx {H}x{W} noise frame {f} unclamped: |dPSNR| = {d_psnr:.3e} dB  |dSSIM| = {d_ssim:.3e}")
        assert d_psnr <= PSNR_TOL and d_ssim <= SSIM_TOL, (f, got[f], host[f])
        assert abs(_psnr(got_cl[f][0]) - p_cl) <= PSNR_TOL and abs(got_cl[f][1] - s_cl) <= SSIM_TOL


@pytest.mark.parametrize("clamp", [False, True])
def test_frames_do_not_mix_and_a_repeat_gives_the_same_bits(clamp):
    from pixel_nerf_multiscale_amd import util
    H, W = 37, 23
    x, gt = _frames(H, W, 3)
    gt_d = gt.cuda()
    clean = util.eval_frames(x.cuda(), gt_d, clamp=clamp)
    xn = x.clone()
    xn[1, 20, 17, 1] = float("nan")
    bad = util.eval_frames(xn.cuda(), gt_d, clamp=clamp)
    again = util.eval_frames(xn.cuda(), gt_d, clamp=clamp)
    assert torch.isnan(bad[1]).all()                                 # not clamped away, in either mode
    assert not torch.isnan(clean).any()
    assert torch.equal(_bits(bad[0]), _bits(clean[0])) and torch.equal(_bits(bad[2]), _bits(clean[2]))
    assert torch.equal(_bits(bad), _bits(again))


def test_eval_frames_does_not_wait_for_the_device():
    from pixel_nerf_multiscale_amd import util
    x, gt = _frames(37, 23, 3)
    rgb, gt_d = x.cuda(), gt.cuda()
    out = torch.empty(3, 2, dtype=torch.float64, device="cuda")
    want = util.eval_frames(rgb, gt_d)                               # warm-up: allocations, code objects
    works = sync_debug_mode_works()
    print(f'torch.cuda.set_sync_debug_mode("error") works under this build: {works}')
    if works:
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = util.eval_frames(rgb, gt_d)
        util.eval_frames(rgb.view(3, 37 * 23, 3), gt_d, clamp=True, metrics_out=out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------------------------------------------------- the loop
class _Batches(list):
    """A loader as evaluate_approx takes it: batched dicts, the depth range on .dataset."""


def _runs(evalio, net, rend, loader, seed, frames, recording):
    """name -> (result, per_object rows, recorded frames on the host) of four evaluate_approx runs with the same seed."""
    runs = {}
    for name, kw in (("device", dict(metrics="device", verbose=False)), ("host", dict(metrics="host", verbose=False)),
                     ("device_again", dict(metrics="device", verbose=True)), ("default_wrapper", dict(metrics="device", verbose=False))):
        frames.clear()
        po = []
        res = evalio.evaluate_approx(net, rend, loader, source="0", seed=seed, per_object=po,
                                     render_par=None if name == "default_wrapper" else recording, **kw)
        runs[name] = (res, po, [f.cpu() for f in frames])
    return runs


def test_evaluate_approx_end_to_end():
    import golden_util as gu
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio
    from pixel_nerf_multiscale_amd.render.nerf import _RenderWrapper
    spec = dict(gu.CASES["full_ns1"])
    W = H = 32
    focal, NV, SB, seed = 33.0, 4, 2, 7                                 # target views [1, 2] then [2, 3]
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    rend = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).cuda().eval()
    data = make_dataset(net, rend, 2 * SB, NV, W, H, focal)
    net.precision = "fp16"
    loader = _Batches(dict(images=torch.stack([d["images"] for d in data[b * SB:(b + 1) * SB]]),
                           poses=torch.stack([d["poses"] for d in data[b * SB:(b + 1) * SB]]),
                           masks=None, focal=torch.full((SB,), focal)) for b in range(2))
    loader.dataset = data                                            # z_near, z_far

    torch.random.manual_seed(seed)                                   # the views of this seed, with no render in between
    want_views = [evalio.draw_approx_views(SB, NV, "0") for _ in range(2)]
    assert [v[1].flatten().tolist() for v in want_views] == [[1, 2], [2, 3]]

    inner, frames = _RenderWrapper(net, rend, simple_output=True).eval(), []

    def recording(rays):
        rgb, depth = inner(rays)
        frames.append(rgb.detach().clone())
        return rgb, depth

    # The encoder is torch's resnet34: the convolution library's default choices for its deeper layers differ in the last bit
    # from run to run, which a random-weight network amplifies.  Runs that are compared with each other need torch's switch
    # for deterministic convolutions; it is restored below.
    was_deterministic = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        runs = _runs(evalio, net, rend, loader, seed, frames, recording)
    finally:
        torch.backends.cudnn.deterministic = was_deterministic
    assert rend.forced_seed is None and net.training is False

    (res_d, po_d, fr_d), (res_h, po_h, fr_h) = runs["device"], runs["host"]
    assert res_d[2] == 4 and res_h[2] == 4 and len(po_d) == 4 and len(po_h) == 4 and len(fr_d) == 2
    assert all(torch.equal(a, b) for a, b in zip(fr_d, fr_h))                    # the same seed renders the same frames
    assert not torch.equal(fr_d[0][0], fr_d[0][1])
    for k, (d, h) in enumerate(zip(po_d, po_h)):
        b, sb = divmod(k, SB)
        src_view, dest_view = want_views[b]
        for got in (d, h):                                           # rendering did not consume the generator of the view draws
            assert got[:4] == (b, sb, src_view[sb].tolist(), int(dest_view[sb, 0])), (got, want_views)
        assert d[2] == [0] and d[3] != 0
        raw = fr_d[b][sb].reshape(H, W, 3).numpy()                   # UNclamped
        g = (data[k]["images"][d[3]] * 0.5 + 0.5).permute(1, 2, 0).contiguous().numpy()
        want_psnr, want_ssim = float(evalio.psnr(raw, g)), float(evalio.ssim(raw, g))
        print(f"eval_approx loop batch {b} object {sb} view {d[3]}: psnr {want_psnr:.4f} dB ssim {want_ssim:.8f}  device |dPSNR| = "
              f"{abs(d[4] - want_psnr):.3e} dB |dSSIM| = {abs(d[5] - want_ssim):.3e}  host |dPSNR| = {abs(h[4] - want_psnr):.3e} dB "
              f"|dSSIM| = {abs(h[5] - want_ssim):.3e}")
        assert abs(d[4] - h[4]) <= PSNR_TOL and abs(d[5] - h[5]) <= SSIM_TOL
        for got in (d, h):
            assert abs(got[4] - want_psnr) <= PSNR_TOL and abs(got[5] - want_ssim) <= SSIM_TOL
    for res, po in ((res_d, po_d), (res_h, po_h)):
        assert abs(res[0] - sum(p[4] for p in po) / 4) < 1e-9 and abs(res[1] - sum(p[5] for p in po) / 4) < 1e-9
    assert runs["device_again"][0] == res_d and runs["device_again"][1] == po_d   # a second run, read batch by batch
    assert runs["default_wrapper"][0] == res_d and runs["default_wrapper"][1] == po_d
