"""calc_metrics on the device (pnr_eval_frames_u8 / util.eval_frames_u8 / evalio.calc_metrics(metrics="device")): the metrics of
8-bit interleaved pairs against the host functions that define the project's numbers on the np.float32(p) / np.float32(255)
arrays (evalio.psnr, evalio.ssim; SSIM is this project's restatement of skimage, parity unpinned), the planar outputs bit for
bit, what a result must not depend on (alpha bytes, the other frames of a call, the chunk size), and the driver end to end
with both back ends and after evaluate(write_images=True).  Run with -s for the measured differences.

Bounds, those of tests/test_gpu_eval_back.py (fixed by the formats, none by what the kernel gives): SSIM |d| <= 1e-6,
PSNR |d| <= 2e-5 dB."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from eval_util import make_dataset, read_png, sync_debug_mode_works
from test_calc_metrics_cpu import _expected, _metrics_txt, _srn_tree
from test_gpu_eval_back import PSNR_TOL, SSIM_TOL

pytestmark = pytest.mark.gpu

SIZES = [(7, 7), (8, 23), (37, 23)]          # (H, W): one window, one ragged tile, ragged tiles in both directions


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


def _psnr(mse):
    return float("inf") if mse == 0.0 else 10.0 * math.log10(1.0 / mse)


@functools.lru_cache(maxsize=None)
def _pairs(H, W, F):
    """Seeded random bytes -> (pred (F, H, W, 3), gt (F, H, W, 4)) uint8 on the host; gt[..., :3] is the RGB ground truth."""
    rng = np.random.default_rng(100000 * F + 1000 * H + W)
    pred = torch.from_numpy(rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8))
    gt = torch.from_numpy(rng.integers(0, 256, (F, H, W, 4), dtype=np.uint8))
    return pred, gt


@functools.lru_cache(maxsize=None)
def _host_numbers(H, W, F):
    """[(psnr, ssim)] per pair by the host functions on the fp32 quotients, once."""
    from pixel_nerf_multiscale_amd import evalio
    pred, gt = _pairs(H, W, F)
    out = []
    for f in range(F):
        x = np.float32(pred[f].numpy()) / np.float32(255)
        g = np.float32(gt[f].numpy()[..., :3]) / np.float32(255)
        out.append((float(evalio.psnr(x, g)), float(evalio.ssim(x, g))))
    return out


@pytest.mark.parametrize("gt_channels", [3, 4])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_bytes_match_the_host_functions(H, W, F, gt_channels):
    from pixel_nerf_multiscale_amd import util
    pred, gt = _pairs(H, W, F)
    gt = gt[..., :gt_channels].contiguous()
    assert pred.numel() // F % 2 == 1 or (H, W) != (7, 7)           # 7 x 7 x 3 = 147: frame 1 starts at an odd address
    got = util.eval_frames_u8(pred.cuda(), gt.cuda())
    assert got.dtype == torch.float64 and tuple(got.shape) == (F, 2) and got.is_cuda
    worst_p = worst_s = 0.0
    for f, ((p, s), (mse, ss)) in enumerate(zip(_host_numbers(H, W, F), got.cpu().tolist())):
        assert math.isfinite(p) and mse > 0.0
        worst_p, worst_s = max(worst_p, abs(_psnr(mse) - p)), max(worst_s, abs(ss - s))
    print(f"calc_metrics u8 {H}x{W} F={F} gt channels {gt_channels}: worst |dPSNR| = {worst_p:.3e} dB  |dSSIM| = {worst_s:.3e}")
    assert worst_p <= PSNR_TOL and worst_s <= SSIM_TOL
    out = torch.full((F + 1, 2), -1.0, dtype=torch.float64, device="cuda")
    assert util.eval_frames_u8(pred.cuda(), gt.cuda(), metrics_out=out[:F]) is not None
    assert torch.equal(_bits(out[:F]), _bits(got)) and (out[F] == -1.0).all()       # metrics_out: those rows and no other


def test_planar_outputs_are_the_numpy_expression_bit_for_bit():
    from pixel_nerf_multiscale_amd import util
    rng = np.random.default_rng(5)
    every = np.arange(256, dtype=np.uint8)
    pred = np.stack([every, every[::-1], rng.permutation(every)], -1).reshape(1, 16, 16, 3)        # all 256 values, per channel
    gt = np.stack([rng.permutation(every), every, every[::-1], rng.permutation(every)], -1).reshape(1, 16, 16, 4)
    pred = np.concatenate([pred, rng.integers(0, 256, pred.shape, dtype=np.uint8)])                  # F = 2
    gt = np.concatenate([gt, rng.integers(0, 256, gt.shape, dtype=np.uint8)])
    m, pp, gp = util.eval_frames_u8(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), want_planar=True)
    planar = lambda p: ((np.float32(p) / np.float32(255)) * np.float32(2) - np.float32(1)).transpose(0, 3, 1, 2)
    for got, want in ((pp, planar(pred)), (gp, planar(gt[..., :3]))):
        assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 16, 16)
        assert np.array_equal(got.cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32))
    assert len(set(pp[0, 0].cpu().flatten().tolist())) == 256
    assert torch.equal(_bits(m), _bits(util.eval_frames_u8(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda())))


def test_alpha_identical_pairs_other_frames_and_a_repeat():
    from pixel_nerf_multiscale_amd import util
    H, W = 37, 23
    pred, gt = _pairs(H, W, 3)
    rgb = gt[..., :3].contiguous()
    base = util.eval_frames_u8(pred.cuda(), rgb.cuda())
    for alpha in (0, 255, None):                                    # whatever the alpha bytes
        g4 = gt.clone()
        if alpha is not None:
            g4[..., 3] = alpha
        assert torch.equal(_bits(util.eval_frames_u8(pred.cuda(), g4.cuda())), _bits(base)), alpha
    p4 = torch.cat([pred, gt[..., 3:]], -1).contiguous()            # and an RGBA render at the C level of the wrapper
    assert torch.equal(_bits(util.eval_frames_u8(p4.cuda(), rgb.cuda())), _bits(base))

    same = util.eval_frames_u8(pred.cuda(), torch.cat([pred, gt[..., 3:]], -1).cuda()).cpu()
    assert (same[:, 0] == 0.0).all() and ((same[:, 1] - 1.0).abs() <= SSIM_TOL).all(), same

    changed = pred.clone()
    changed[1] = 255 - changed[1]
    other = util.eval_frames_u8(changed.cuda(), rgb.cuda())
    assert torch.equal(_bits(other[0]), _bits(base[0])) and torch.equal(_bits(other[2]), _bits(base[2]))
    assert not torch.equal(_bits(other[1]), _bits(base[1]))
    assert torch.equal(_bits(util.eval_frames_u8(changed.cuda(), rgb.cuda())), _bits(other))
    for f in range(3):                                              # a frame alone: the bits of its row in the call of three
        assert torch.equal(_bits(util.eval_frames_u8(pred[f:f + 1].cuda(), rgb[f:f + 1].cuda())[0]), _bits(base[f]))


def test_eval_frames_u8_does_not_wait_for_the_device():
    from pixel_nerf_multiscale_amd import util
    pred, gt = _pairs(37, 23, 3)
    pred_d, gt_d = pred.cuda(), gt.cuda()
    out = torch.empty(3, 2, dtype=torch.float64, device="cuda")
    want = util.eval_frames_u8(pred_d, gt_d, want_planar=True)      # warm-up: allocations, code objects
    works = sync_debug_mode_works()
    print(f'torch.cuda.set_sync_debug_mode("error") works under this build: {works}')
    if works:
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = util.eval_frames_u8(pred_d, gt_d, want_planar=True)
        util.eval_frames_u8(pred_d, gt_d[..., :3], metrics_out=out)         # a view that is made dense on the way
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(out), _bits(want[0]))
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


# -------------------------------------------------------------------------------------------------------------- the driver
def _numbers(text):
    return [float(line.split()[1]) for line in text.split("\n")]


def test_both_back_ends_and_the_chunk_size(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    datadir, output, files = _srn_tree(evalio, str(tmp_path), objs=("o1", "o2"), n_views=5, gt_kind={1: "rgba", 3: "jpg"})
    calls = []

    def stub(pred, gt):
        assert pred.is_cuda and gt.is_cuda and pred.dtype == torch.float32 and tuple(pred.shape[1:]) == (3, 9, 11)
        assert float(pred.min()) >= -1.0 and float(pred.max()) <= 1.0
        calls.append(pred.shape[0])
        return (pred - gt).abs().mean(dim=(1, 2, 3))

    runs = {}
    for name, kw in (("host", dict(metrics="host", device="cuda")), ("device", dict(metrics="device")),
                     ("device_1", dict(metrics="device", frames_per_call=1)), ("device_2", dict(metrics="device", frames_per_call=2))):
        calls.clear()
        totals = evalio.calc_metrics(datadir, output, dataset_format="srn", overwrite=True, verbose=False, lpips=stub,
                                     lpips_batch_size=2, **kw)
        assert calls == [2, 2, 1, 2, 2, 1], (name, calls)
        runs[name] = (totals, [_metrics_txt(output, o) for o in ("o1", "o2")], open(os.path.join(output, "all_metrics.txt")).read())
    assert runs["device"][1] == runs["device_1"][1] == runs["device_2"][1]      # chunking does not change a bit
    assert runs["device"][2] == runs["device_1"][2] == runs["device_2"][2] == runs["host"][2]      # to the 6 printed decimals
    for k, obj in enumerate(("o1", "o2")):
        want_psnr, want_ssim, _ = _expected(evalio, files[obj], range(5))
        (hp, hs, hl), (dp, ds, dl) = _numbers(runs["host"][1][k]), _numbers(runs["device"][1][k])
        print(f"calc_metrics {obj}: psnr {want_psnr:.4f} dB ssim {want_ssim:.8f}  device - host |dPSNR| = {abs(dp - hp):.3e} dB "
              f"|dSSIM| = {abs(ds - hs):.3e} |dLPIPS stub| = {abs(dl - hl):.3e}")
        assert hp == want_psnr and hs == want_ssim
        assert abs(dp - hp) <= PSNR_TOL and abs(ds - hs) <= SSIM_TOL and abs(dl - hl) <= 1e-6
    with pytest.raises(ValueError, match="frames_per_call"):
        evalio.metrics_map(datadir, output, dataset_format="srn", overwrite=True, verbose=False, metrics="device", frames_per_call=0)


def test_round_trip_with_the_renderer(tmp_path):
    import golden_util as gu
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio
    spec = dict(gu.CASES["full_ns1"])
    W = H = 32
    focal, NV = 33.0, 4
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    rend = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=True).cuda().eval()
    data = make_dataset(net, rend, 2, NV, W, H, focal)
    net.precision = "fp16"
    out, datadir = str(tmp_path / "eval_out"), str(tmp_path / "data")
    evalio.evaluate(net, rend, data, out, source="0", verbose=False, seed=777, metrics="device", write_images=True)
    gt_u8 = []
    for o in range(2):                                              # the dataset's images as 8-bit files, srn layout
        folder = os.path.join(datadir, f"obj{o:03d}", "rgb")
        os.makedirs(folder)
        g = evalio.quantize_uint8((data[o]["images"] * 0.5 + 0.5).permute(0, 2, 3, 1).contiguous().numpy())
        for v in range(NV):
            evalio.write_png(os.path.join(folder, f"{v:06}.png"), g[v])
        gt_u8.append(g)
    totals = evalio.calc_metrics(datadir, out, dataset_format="srn", metrics="device", verbose=False)
    rows = []
    for o in range(2):
        obj = os.path.join(out, f"obj{o:03d}")
        psnr = ssim = 0.0
        for v in range(1, NV):                                      # view 0 is the source: never rendered, not counted
            x = np.float32(read_png(os.path.join(obj, f"{v:06}.png"))) / np.float32(255)
            g = np.float32(gt_u8[o][v]) / np.float32(255)
            psnr += float(evalio.psnr(x, g)) / (NV - 1)
            ssim += evalio.ssim(x, g) / (NV - 1)
        got_psnr, got_ssim = _numbers(open(os.path.join(obj, "metrics.txt")).read())
        print(f"calc_metrics round trip obj{o:03d}: psnr {psnr:.4f} dB ssim {ssim:.8f}  |dPSNR| = {abs(got_psnr - psnr):.3e} dB  "
              f"|dSSIM| = {abs(got_ssim - ssim):.3e}")
        assert abs(got_psnr - psnr) <= PSNR_TOL and abs(got_ssim - ssim) <= SSIM_TOL
        rows.append((got_psnr, got_ssim))
    means = [(rows[0][k] + rows[1][k]) / 2 for k in (0, 1)]
    assert totals.text == " psnr: {:.6f} ssim: {:.6f}".format(*means) and dict(totals) == {"psnr": means[0], "ssim": means[1]}
