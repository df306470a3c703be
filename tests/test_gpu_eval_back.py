"""Evaluation back end on the device (pnr_eval_frame / util.eval_frame / evaluate(metrics="device")) against the host
functions that define the project's numbers: evalio.quantize_uint8, evalio.psnr, evalio.ssim (SSIM is this project's
restatement of skimage: parity with the reference's own numbers stays unpinned).  Run with -s for the measured errors.

Bounds (all fixed by the formats, none by what the kernel gives):
  bytes        exact.
  SSIM         |d| <= 1e-6: an fp32 emulation of centred window moments stays within 6.4e-8 of evalio.ssim, the uncentred
               form (E[xy] - E[x]E[y]) is off by 1.0e-4 on the 7 x 7 white frame, so that case alone rejects it.
  PSNR         |d| <= 2e-5 dB (an fp32 mean of the squared errors stays within 6e-7 dB).
  depth_norm   <= 2e-7 absolute against the fp64 formula: two fp32 roundings (the difference, the quotient) of values in
               [0, 1]; z_near / z_far are chosen exactly representable with an exact difference, as the entry takes them in fp32.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from eval_util import make_dataset, read_png

pytestmark = pytest.mark.gpu

SSIM_TOL, PSNR_TOL, DEPTH_TOL = 1e-6, 2e-5, 2e-7
SIZES = [(7, 7), (8, 23), (37, 23), (64, 64), (128, 128), (300, 400)]        # (H, W): one window, one tile, ragged tiles in
CONTENTS = ["noise", "white", "disc"]                                         # both directions, SRN and DTU frames


def _frame(H, W, content):
    """-> render (H, W, 3) fp32 UNclamped, gt (3, H, W) fp32 in [-1, 1], from fixed seeds."""
    rng = np.random.default_rng(1000 * H + W + {"noise": 1, "white": 2, "disc": 3}[content] * 100003)
    if content == "noise":
        g01 = rng.random((H, W, 3))
        x = g01 + 0.05 * rng.standard_normal((H, W, 3))                      # leaves [0, 1] here and there: the kernel clamps
    elif content == "white":
        g01 = 1.0 - 1e-3 * rng.random((H, W, 3))
        x = np.clip(g01 + 5e-4 * rng.standard_normal((H, W, 3)), 0.0, 1.0)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        r = np.hypot(yy - (H - 1) / 2.0, xx - (W - 1) / 2.0)
        tex = 0.5 + 0.4 * np.sin(0.9 * xx + 0.3 * np.arange(3)[:, None, None]) * np.cos(0.7 * yy)      # (3, H, W)
        inside = r <= min(H, W) / 3.0
        g01 = np.where(inside[..., None], tex.transpose(1, 2, 0), 1.0)
        x = np.where(inside[..., None], g01 + 0.02 * rng.standard_normal((H, W, 3)), 1.0)
    gt = torch.from_numpy((g01.transpose(2, 0, 1) * 2.0 - 1.0).astype(np.float32)).contiguous()
    return torch.from_numpy(x.astype(np.float32)).contiguous(), gt


def _g01(gt):
    """(3, H, W) in [-1, 1] -> (H, W, 3) in [0, 1] the way evaluate() forms its ground truth: torch's images * 0.5 + 0.5."""
    return (gt * 0.5 + 0.5).permute(1, 2, 0).contiguous().numpy()


@functools.lru_cache(maxsize=None)
def _host_reference(H, W, content):
    """The host functions on the clamped fp32 arrays, once per case."""
    from pixel_nerf_multiscale_amd import evalio
    x, gt = _frame(H, W, content)
    xc, g = np.clip(x.numpy(), 0.0, 1.0), _g01(gt)
    return evalio.quantize_uint8(xc), float(evalio.psnr(xc, g)), float(evalio.ssim(xc, g))


def _psnr(mse):
    return float("inf") if mse == 0.0 else 10.0 * math.log10(1.0 / mse)


def test_bytes_are_the_host_quantisation():
    from pixel_nerf_multiscale_amd import evalio, util
    # frame A, 16 x 16 x 3 = 768 values: every k / 255 with its two fp32 neighbours — k = 0 brings 0.0 and the denormals on
    # both sides of it (one below 0), k = 255 brings 1.0 and its neighbour above 1
    k = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    a = np.stack([np.nextafter(k, np.float32(-1.0)), k, np.nextafter(k, np.float32(2.0))], -1).astype(np.float32).reshape(16, 16, 3)
    # frame B, ragged (9 x 21): the signed zeros, 1.0, values below 0 and above 1, infinities, then noise across [-0.2, 1.2]
    rng = np.random.default_rng(5)
    b = rng.uniform(-0.2, 1.2, 9 * 21 * 3).astype(np.float32)
    b[:12] = [0.0, -0.0, 1.0, -1e-3, -7.5, 1.0 + 1e-3, 300.0, np.inf, -np.inf, 1e-30, 0.999999, 254.5 / 255.0]
    b = b.reshape(9, 21, 3)
    for x in (a, b):
        H, W, _ = x.shape
        gt = torch.from_numpy(np.random.default_rng(6).uniform(-1.0, 1.0, (3, H, W)).astype(np.float32))
        gt.reshape(-1)[:4] = torch.tensor([-1.0, 1.0, 0.0, -0.0])
        gt.reshape(-1)[4:4 + 256] = torch.from_numpy(k) * 2 - 1
        u8, cmp, _, _ = util.eval_frame(torch.from_numpy(x).cuda(), gt=gt.cuda(), want_compare=True, want_metrics=False)
        xc = np.clip(x, 0.0, 1.0)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (H, W, 3) and tuple(cmp.shape) == (H, 2 * W, 3)
        assert np.array_equal(u8.cpu().numpy(), evalio.quantize_uint8(xc))
        assert np.array_equal(cmp.cpu().numpy(), evalio.quantize_uint8(np.hstack((xc, _g01(gt)))))
    want = evalio.quantize_uint8(a)
    assert (want.reshape(-1, 3)[1:, 0] < np.arange(1, 256)).any()
    # ^ the case has teeth: neighbours just below k / 255 truncate to k - 1, where rounding would give k


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("H,W", SIZES)
def test_metrics_match_the_host_functions(H, W, content):
    from pixel_nerf_multiscale_amd import util
    x, gt = _frame(H, W, content)
    want_u8, want_psnr, want_ssim = _host_reference(H, W, content)
    u8, _, _, m = util.eval_frame(x.cuda(), gt=gt.cuda())
    mse, ssim = m.cpu().tolist()
    d_ssim, d_psnr = abs(ssim - want_ssim), abs(_psnr(mse) - want_psnr)
    print(f"eval_back {H}x{W} {content}: psnr {want_psnr:.4f} dB ssim {want_ssim:.8f}  |dSSIM| = {d_ssim:.3e}  |dPSNR| = {d_psnr:.3e} dB")
    assert np.array_equal(u8.cpu().numpy(), want_u8)
    assert d_ssim <= SSIM_TOL, (d_ssim, ssim, want_ssim)
    assert d_psnr <= PSNR_TOL, (d_psnr, mse, want_psnr)


def test_identical_images_and_a_nan_pixel():
    from pixel_nerf_multiscale_amd import util
    H, W = 37, 23
    _, gt = _frame(H, W, "noise")
    x = (gt * 0.5 + 0.5).permute(1, 2, 0).contiguous()               # the bits the kernel forms for the ground truth
    u8, _, _, m = util.eval_frame(x.cuda(), gt=gt.cuda())
    mse, ssim = m.cpu().tolist()
    print(f"eval_back identical {H}x{W}: mse = {mse!r}  |SSIM - 1| = {abs(ssim - 1.0):.3e}")
    assert mse == 0.0 and abs(ssim - 1.0) <= SSIM_TOL
    xn = x.clone()
    xn[20, 17, :] = float("nan")
    u8n, cmpn, _, mn = util.eval_frame(xn.cuda(), gt=gt.cuda(), want_compare=True)
    assert torch.isnan(mn).all()                                     # not clamped away: the host path's metrics are NaN too
    u8n, u8 = u8n.cpu(), u8.cpu()
    assert (u8n[20, 17] == 0).all() and (cmpn[20, 17].cpu() == 0).all()
    u8n[20, 17] = u8[20, 17]
    assert torch.equal(u8n, u8)                                      # and nothing else moved


def test_strided_record_and_repeat_are_bit_identical():
    from pixel_nerf_multiscale_amd import util
    H, W = 37, 23
    x, gt = _frame(H, W, "disc")
    zn, zf = 1.25, 2.75
    depth = torch.from_numpy(np.random.default_rng(8).uniform(zn, zf, (H, W)).astype(np.float32))
    rec = torch.cat((x.reshape(-1, 3), depth.reshape(-1, 1)), 1).cuda().contiguous()      # the (N, 4) per-ray record
    r3 = rec.view(H, W, 4)
    kw = dict(z_near=zn, z_far=zf, want_compare=True, want_depth=True)
    dense = util.eval_frame(x.cuda(), depth.cuda(), gt.cuda(), **kw)
    strided = util.eval_frame(r3[..., :3], r3[..., 3], gt.cuda(), **kw)
    again = util.eval_frame(r3[..., :3], r3[..., 3], gt.cuda(), **kw)
    assert r3[..., :3].stride() == (4 * W, 4, 1) and not r3[..., :3].is_contiguous()
    for a, b, c in zip(dense, strided, again):
        assert torch.equal(a, b) and torch.equal(b, c)
    assert torch.equal(dense[3].view(torch.int64), strided[3].view(torch.int64))          # the metrics' bits, not their values
    with pytest.raises(ValueError):
        util.eval_frame(r3.permute(1, 0, 2)[..., :3], gt=gt.cuda())                        # not a row-major record
    with pytest.raises(ValueError):
        util.eval_frame(x.cuda(), gt=gt[:, :-1].cuda())                                    # ground truth of another size


@pytest.mark.parametrize("zn,zf", [(1.25, 2.75), (0.5, 4.0)])
def test_normalised_depth(zn, zf):
    from pixel_nerf_multiscale_amd import util
    H, W = 37, 23
    d = np.random.default_rng(9).uniform(zn, zf, (H, W)).astype(np.float32)
    d.reshape(-1)[:4] = [zn, zf, np.nextafter(np.float32(zn), np.float32(9)), np.nextafter(np.float32(zf), np.float32(0))]
    x, _ = _frame(H, W, "noise")
    _, _, dn, _ = util.eval_frame(x.cuda(), torch.from_numpy(d).cuda(), z_near=zn, z_far=zf, want_u8=False, want_depth=True,
                                  want_metrics=False)
    want = (d.astype(np.float64) - zn) / (zf - zn)
    err = float(np.abs(dn.cpu().numpy().astype(np.float64) - want).max())
    print(f"eval_back depth_norm [{zn}, {zf}]: worst |d| = {err:.3e}")
    assert dn.dtype == torch.float32 and err <= DEPTH_TOL
    assert dn.cpu().numpy().reshape(-1)[0] == 0.0 and dn.cpu().numpy().reshape(-1)[1] == 1.0


# ---------------------------------------------------------------------------------------------------------------- the loop
def test_evaluate_on_the_device_back_end(tmp_path):
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
    out = str(tmp_path / "eval_out")
    net.precision = "fp16"

    orig, frames = rend.render_image, []

    def recording(*a, **k):
        res = orig(*a, **k)
        frames.append((res[0].detach().clone(), res[1].detach().clone()))
        return res
    rend.render_image = recording
    try:
        with pytest.raises(ValueError):          # no resampling on the device: refused before anything is rendered
            evalio.evaluate(net, rend, data, str(tmp_path / "scaled"), source="0", scale=0.5, verbose=False, metrics="device")
        assert not frames and not os.path.exists(str(tmp_path / "scaled" / "obj000"))
        m1 = evalio.evaluate(net, rend, data, out, source="0", verbose=False, seed=777, metrics="device", write_compare=True,
                             write_depth=True)
        assert len(frames) == 2 * (NV - 1)
        rows = [x.split() for x in open(os.path.join(out, "finish.txt")).read().split("\n") if x]
        assert [r[0] for r in rows] == ["obj000", "obj001"] and all(r[3] == "1" for r in rows)
        zn, zf = data.z_near, data.z_far
        for o in range(2):
            obj = os.path.join(out, f"obj{o:03d}")
            assert sorted(os.listdir(obj)) == sorted(f"{v:06}{suffix}" for v in range(1, NV)
                                                     for suffix in (".png", "_compare.png", "_depth.npy"))
            g01 = (data[o]["images"] * 0.5 + 0.5).permute(0, 2, 3, 1).contiguous().numpy()
            psnr = ssim = 0.0
            for i, v in enumerate(range(1, NV)):
                rgb, depth = frames[o * (NV - 1) + i]
                xc = rgb.clamp(0, 1).cpu().numpy()
                assert np.array_equal(read_png(os.path.join(obj, f"{v:06}.png")), evalio.quantize_uint8(xc))
                assert np.array_equal(read_png(os.path.join(obj, f"{v:06}_compare.png")),
                                      evalio.quantize_uint8(np.hstack((xc, g01[v]))))
                dn = np.load(os.path.join(obj, f"{v:06}_depth.npy"))
                assert dn.dtype == np.float32 and dn.shape == (H, W)
                assert np.abs(dn.astype(np.float64) - (depth.cpu().numpy().astype(np.float64) - zn) / (zf - zn)).max() <= DEPTH_TOL
                psnr += evalio.psnr(xc, g01[v]) / (NV - 1)
                ssim += evalio.ssim(xc, g01[v]) / (NV - 1)
            print(f"eval_back loop obj{o:03d}: |dPSNR| = {abs(float(rows[o][1]) - psnr):.3e} dB  |dSSIM| = {abs(float(rows[o][2]) - ssim):.3e}")
            assert abs(float(rows[o][1]) - psnr) <= PSNR_TOL and abs(float(rows[o][2]) - ssim) <= SSIM_TOL
        assert m1[2] == 2 and abs(m1[0] - (float(rows[0][1]) + float(rows[1][1])) / 2) < 1e-9
        assert abs(m1[1] - (float(rows[0][2]) + float(rows[1][2])) / 2) < 1e-9

        # resume: nothing is rendered, by either back end — the file format is unchanged
        frames.clear()
        m2 = evalio.evaluate(net, rend, data, out, source="0", verbose=False, seed=777, metrics="device", write_compare=True,
                             write_depth=True)
        m3 = evalio.evaluate(net, rend, data, out, source="0", verbose=False, seed=777, metrics="host")
        assert not frames and m2 == m1 and m3 == m1

        # write_depth on the host back end: the same file from the frame that path copies anyway, nothing else changes
        out_h = str(tmp_path / "eval_host")
        evalio.evaluate(net, rend, data, out_h, source="0", max_objects=1, verbose=False, seed=777, write_depth=True)
        assert sorted(os.listdir(os.path.join(out_h, "obj000"))) == sorted(f"{v:06}{suffix}" for v in range(1, NV)
                                                                           for suffix in (".png", "_depth.npy"))
        for i, v in enumerate(range(1, NV)):
            rgb, depth = frames[i]
            assert np.array_equal(read_png(os.path.join(out_h, "obj000", f"{v:06}.png")),
                                  evalio.quantize_uint8(rgb.clamp(0, 1).cpu().numpy()))
            dn = np.load(os.path.join(out_h, "obj000", f"{v:06}_depth.npy"))
            assert dn.dtype == np.float32 and dn.shape == (H, W)
            assert np.abs(dn.astype(np.float64) - (depth.cpu().numpy().astype(np.float64) - zn) / (zf - zn)).max() <= DEPTH_TOL
    finally:
        rend.render_image = orig
