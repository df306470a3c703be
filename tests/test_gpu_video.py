"""Novel-view video on the card: pnr_video_frames against the numpy model of tests/video_util.py byte for byte and count for
count (every route: dense with float4 loads, dense from an unaligned base, the stride-4 record; `out` at byte offsets 0..3 of a
larger buffer whose other bytes must stay as they were; run twice), pnr_image_to_tensor against torch's own division on the CPU,
pnr_view_strip against the model, and the drivers end to end on the small network of the evaluation-loop tests: render_video
against three render_image calls, gen_video and eval_real through their files.  Every comparison is an equality.
The rendered frames are 16 x 16; the SOURCE views are 32 x 32, the smallest square the encoder takes (its deepest level must
keep 2 x 2 texels: the render refuses a 1 x 1 latent map, whose texel mapping divides by W - 1), so gen_video at scale=1
writes 32 x 32 frames and eval_real brings its 16 x 16 array to 32 on the host first, as the driver does for a photograph."""
import os

import numpy as np
import pytest
import torch

import video_util as vu
from eval_util import make_dataset, read_png, sync_debug_mode_works

pytestmark = pytest.mark.gpu

GUARD = 0xA5
Z_NEAR, Z_FAR, FOCAL, SIDE = 1.25, 2.75, 16.5, 16            # the rendered frames
SRC, SRC_FOCAL = 32, 33.0                                        # the source views: the same field of view at twice the size


# ------------------------------------------------------------------------------------------------------- pnr_video_frames
@pytest.mark.parametrize("F,H,W", [(1, 1, 1), (3, 3, 5), (2, 4, 8), (3, 20, 20)])
@pytest.mark.parametrize("route", ["dense", "dense_unaligned", "stride4"])
def test_video_frames_equals_the_model(F, H, W, route):
    from pixel_nerf_multiscale_amd import util
    P = F * H * W
    x = vu.fill(3 * P, seed=P)
    want, n_want = vu.quantize_model(x)
    if P >= 1200:
        assert n_want >= 6 and len(np.unique(want)) == 256                   # the whole value set is in the largest case
    if route == "dense":
        rgb = torch.from_numpy(x).cuda().view(P, 3)
        assert rgb.data_ptr() % 16 == 0
    elif route == "dense_unaligned":                                         # one float into an allocation: no float4 loads
        store = torch.zeros(3 * P + 1, device="cuda")
        store[1:] = torch.from_numpy(x).cuda()
        rgb = store[1:].view(P, 3)
        assert rgb.data_ptr() % 16 == 4 and rgb.is_contiguous()
    else:                                                                    # the packed per-ray record; its depth slot is NaN
        rec = torch.full((P, 4), float("nan"), device="cuda")
        rec[:, :3] = torch.from_numpy(x).cuda().view(P, 3)
        rgb = rec[:, :3]
    got = []
    for off in range(4):
        for rep in range(2):
            buf = torch.full((3 * P + 24,), GUARD, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 4 == 0
            out = buf[8 + off:8 + off + 3 * P]
            count = torch.full((1,), -7, dtype=torch.int64, device="cuda")    # set by the call, not added to
            frames, cnt = util.video_frames(rgb, F, H, W, out=out, count=count)
            assert frames.shape == (F, H, W, 3) and frames.data_ptr() == out.data_ptr() and cnt.data_ptr() == count.data_ptr()
            got.append((off, rep, buf, count))
    frames, cnt = util.video_frames(rgb, F, H, W)                            # the wrapper's own buffers
    torch.cuda.synchronize()
    assert np.array_equal(frames.cpu().numpy().reshape(-1), want) and int(cnt) == n_want
    for off, rep, buf, count in got:
        b = buf.cpu().numpy()
        assert np.array_equal(b[8 + off:8 + off + 3 * P], want), (off, rep)
        assert (b[:8 + off] == GUARD).all() and (b[8 + off + 3 * P:] == GUARD).all(), (off, rep)
        assert int(count) == n_want, (off, rep)


def test_video_frames_without_a_counter_and_in_range_count_is_zero():
    from pixel_nerf_multiscale_amd import _native as N, util
    F, H, W = 2, 5, 7
    x = vu.fill(3 * F * H * W, seed=11, with_outside=False)
    want, n = vu.quantize_model(x)
    assert n == 0
    rgb = torch.from_numpy(x).cuda()
    out = torch.zeros(F, H, W, 3, dtype=torch.uint8, device="cuda")
    N.check(N.lib.pnr_video_frames(rgb.data_ptr(), 0, F, W, H, out.data_ptr(), None, N.current_stream(rgb.device)), "pnr_video_frames")
    frames, cnt = util.video_frames(rgb.view(F, H, W, 3), F, H, W)
    assert np.array_equal(out.cpu().numpy().reshape(-1), want) and torch.equal(frames, out) and int(cnt) == 0
    assert np.array_equal(want, (x * np.float32(255)).astype(np.uint8))     # numpy's own cast on its defined range


# ------------------------------------------------------------------------------------------------------- the other two entries
@pytest.mark.parametrize("H,W", [(3, 5), (16, 17)])
def test_image_to_tensor_equals_torch_division(H, W):
    from pixel_nerf_multiscale_amd import util
    seen = [set(), set(), set()]
    for start in range(0, 256, H * W):                                       # every byte value in every channel position
        img = ((vu.all_bytes_image(H, W).astype(np.int32) + start) % 256).astype(np.uint8)
        for c in range(3):
            seen[c] |= set(img[..., c].reshape(-1).tolist())
        t = torch.from_numpy(img)
        want0 = t.float().div(255).permute(2, 0, 1).contiguous()
        want1 = t.float().div(255).sub(0.5).div(0.5).permute(2, 0, 1).contiguous()
        got0 = util.image_to_tensor(img)                                     # numpy in, uploaded
        got1 = util.image_to_tensor(t.cuda(), balanced=True)                 # device tensor in
        assert got0.shape == (3, H, W) and got0.dtype == torch.float32 and got0.is_cuda
        assert torch.equal(got0.cpu().view(torch.int32), want0.view(torch.int32))
        assert torch.equal(got1.cpu().view(torch.int32), want1.view(torch.int32))
    assert all(s == set(range(256)) for s in seen)
    assert float(got1.min()) >= -1.0 and float(got1.max()) <= 1.0


@pytest.mark.parametrize("NS", [1, 3])
def test_view_strip_equals_the_model(NS):
    from pixel_nerf_multiscale_amd import util
    H, W = 3, 5
    x = vu.fill(NS * 3 * H * W, seed=NS, with_outside=False) * np.float32(2.0) - np.float32(1.0)      # the value set in [-1, 1]
    images = x.reshape(NS, 3, H, W)
    images[:, :, 0, 0] = np.arange(NS, dtype=np.float32)[:, None] / np.float32(NS) - np.float32(0.5)  # distinct views
    got = util.view_strip(torch.from_numpy(images).cuda())
    assert got.shape == (H, NS * W, 3) and got.dtype == torch.uint8
    want = vu.view_strip_model(images, 0.5, 0.5)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want, np.hstack((*((images.transpose(0, 2, 3, 1) * np.float32(0.5) + np.float32(0.5)) * 255).astype(np.uint8),)))
    assert len({tuple(want[0, v * W]) for v in range(NS)}) == NS             # the views are where hstack puts them
    unit = (images * np.float32(0.5) + np.float32(0.5))
    got = util.view_strip(torch.from_numpy(unit).cuda(), scale=1.0, lo=0.0)
    assert np.array_equal(got.cpu().numpy(), vu.view_strip_model(unit, 1.0, 0.0))
    wide = np.array([-3.0, 3.0, np.nan, 1.0], np.float32).reshape(1, 1, 1, 4).repeat(3, axis=1)       # saturation, as the frames'
    got = util.view_strip(torch.from_numpy(wide).cuda())
    assert got.cpu().numpy()[0, :, 0].tolist() == [0, 255, 0, 255]
    assert np.array_equal(got.cpu().numpy(), vu.view_strip_model(wide, 0.5, 0.5))


# ------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def scene():
    import golden_util as gu
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet
    spec = dict(gu.CASES["full_ns1"])
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    rend = NeRFRenderer(n_coarse=32, n_fine=16, n_fine_depth=8, white_bkgd=False).cuda().eval()
    data = make_dataset(net, rend, 1, 2, SRC, SRC, SRC_FOCAL)
    return net, rend, data[0]


def _encode_first_view(net, item):
    net.encode(item["images"][:1].cuda()[None], item["poses"][:1].cuda()[None], torch.tensor(SRC_FOCAL)[None].cuda())


def test_render_video_equals_three_render_image_calls(scene):
    from pixel_nerf_multiscale_amd import video
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    net, rend, item = scene
    _encode_first_view(net, item)
    poses = video.orbit_poses(3, -10, 2.0)
    seed = 20240
    video.render_video(net, rend, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, seed=seed)      # warm-up: allocations, code objects
    works = sync_debug_mode_works()
    print(f'torch.cuda.set_sync_debug_mode("error") works under this build: {works}')
    if works:
        torch.cuda.set_sync_debug_mode("error")
    try:
        frames, count = video.render_video(net, rend, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, seed=seed)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert frames.is_cuda and frames.shape == (3, SIDE, SIDE, 3) and frames.dtype == torch.uint8
    assert count.is_cuda and count.dtype == torch.int64 and rend.forced_seed is None
    got = frames.cpu().numpy()
    for f in range(3):
        rend.forced_seed = frame_seed(seed, f)
        try:
            rgb, _ = rend.render_image(net, poses[f], SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR)
        finally:
            rend.forced_seed = None
        want, n = vu.quantize_model(rgb.cpu().numpy())
        assert n == 0 and np.array_equal(got[f], want), f
    assert int(count) == 0                      # fp32 path, black background: convex sums of sigmoids stay far below 256 / 255
    assert len(np.unique(got)) > 8 and not np.array_equal(got[0], got[1])                  # a picture, and the camera moves


def test_gen_video_writes_frames_and_view_strip(scene, tmp_path):
    from pixel_nerf_multiscale_amd import video
    net, rend, item = scene
    seen = []
    orig = rend._forward_fused

    def recording(*a, **k):
        seen.append((rend.n_coarse, rend.n_fine))
        return orig(*a, **k)
    rend._forward_fused = recording
    try:
        res = video.gen_video(net, rend, item, str(tmp_path), [0, 1], num_views=3, elevation=-10.0, radius=2.0, z_near=Z_NEAR,
                              z_far=Z_FAR, seed=9)
    finally:
        del rend._forward_fused
    assert seen == [(64, 128)] * 3 and (rend.n_coarse, rend.n_fine) == (32, 16)            # bumped for the video, then restored
    assert res.frames.shape == (3, SRC, SRC, 3) and res.frames.dtype == np.uint8 and res.n_out_of_range == 0
    stem = os.path.join(str(tmp_path), "video0000_v000_001")
    assert res.frame_paths == [os.path.join(stem + "_frames", f"{i:04}.png") for i in range(3)]
    assert sorted(os.listdir(stem + "_frames")) == ["0000.png", "0001.png", "0002.png"]
    for i, p in enumerate(res.frame_paths):
        assert np.array_equal(read_png(p), res.frames[i]), i
    assert res.view_path == stem + "_view.png" and res.video_path is None
    strip = read_png(res.view_path)
    assert strip.shape == (SRC, 2 * SRC, 3)
    assert np.array_equal(strip, vu.view_strip_model(item["images"][[0, 1]].numpy(), 0.5, 0.5))
    assert len(np.unique(res.frames)) > 8
    # without the bump the renderer's own counts render, and stay
    seen.clear()
    rend._forward_fused = recording
    try:
        res2 = video.gen_video(net, rend, item, str(tmp_path / "b"), [1], num_views=2, radius=0.0, z_near=Z_NEAR, z_far=Z_FAR,
                               ensure_resolution=False, split="test", subset=7, seed=9)
    finally:
        del rend._forward_fused
    assert seen == [(32, 16)] * 2 and (rend.n_coarse, rend.n_fine) == (32, 16)
    assert os.path.basename(res2.view_path) == "videot0007_v001_view.png" and read_png(res2.view_path).shape == (SRC, SRC, 3)


def test_eval_real_from_an_array(scene, tmp_path):
    from pixel_nerf_multiscale_amd import util, video
    net, rend, _ = scene
    img = np.random.default_rng(4).integers(0, 256, (SIDE, SIDE, 3), dtype=np.uint8)
    try:
        import PIL  # noqa: F401
    except ImportError:
        img = np.random.default_rng(4).integers(0, 256, (SRC, SRC, 3), dtype=np.uint8)     # nothing to resize with: the size itself
    sized = video._load_image(img, SRC)                                                    # the host step: 16 -> 32 through PIL
    assert sized.shape == (SRC, SRC, 3) and sized.dtype == np.uint8
    fed = []
    hook = net.encoder.register_forward_hook(lambda mod, args, out: fed.append(args[0].detach().clone()))
    try:
        res = video.eval_real(net, rend, img, str(tmp_path), size=SRC, out_size=SIDE, focal=FOCAL, radius=2.0, elevation=-10.0,
                              num_views=3, z_near=Z_NEAR, z_far=Z_FAR, seed=2)
    finally:
        hook.remove()
    assert len(fed) == 1 and tuple(fed[0].shape) == (1, 3, SRC, SRC)
    assert torch.equal(fed[0][0], util.image_to_tensor(sized))                             # the encoder saw image_to_tensor's output
    assert torch.equal(fed[0][0].cpu(), torch.from_numpy(sized).float().div(255).permute(2, 0, 1))
    assert res.frames.shape == (3, SIDE, SIDE, 3) and res.view_path is None and res.video_path is None
    assert res.frame_paths == [os.path.join(str(tmp_path), "image_frames", f"{i:04}.png") for i in range(3)]
    for i, p in enumerate(res.frame_paths):
        assert np.array_equal(read_png(p), res.frames[i]), i
    assert (net.poses.cpu()[0, :, :3] == torch.eye(3)).all() and float(net.poses[0, 2, 3]) == -2.0     # the dummy camera
