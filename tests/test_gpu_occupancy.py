"""Empty-space culling on the device (csrc/occupancy.hip, render/occupancy.py, NeRFRenderer.render_frames_bounded and the
drivers' occupancy= argument) against the numpy models of tests/occupancy_util.py, bit for bit, and end to end against the
unbounded renderer where the two must agree."""
import os

import numpy as np
import pytest
import torch

import occupancy_util as U
from eval_util import sync_debug_mode_works

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -777.25, -12345
Z_NEAR, Z_FAR, FOCAL, SIDE = 1.25, 2.75, 16.5, 16
SRC, SRC_FOCAL = 32, 33.0


def _words(t):
    return t.cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------- pnr_occ_build
def _sigma(shape, seed):
    rng = np.random.default_rng(seed)
    s = rng.normal(size=shape).astype(np.float32) * 10.0
    flat = s.reshape(-1)
    flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = np.nan
    flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = np.inf
    flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = -np.inf
    return s


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 34), (33, 2, 65), (17, 17, 17)])
@pytest.mark.parametrize("stride", [1, 4])
def test_occ_build_equals_the_model(shape, stride):
    from pixel_nerf_multiscale_amd import _native as N
    nx, ny, nz = shape
    sigma = _sigma(shape, seed=nx * 100 + nz)
    thresh = 14.0                                                     # few hot samples: dilation has room to show
    n_words = (nx - 1) * (ny - 1) * ((nz - 1 + 31) // 32)
    store = torch.full((sigma.size, stride), SENT_F, device="cuda")
    store[:, stride - 1] = torch.from_numpy(sigma.reshape(-1)).cuda()
    field_ptr = store.data_ptr() + 4 * (stride - 1)
    stream = N.current_stream(store.device)
    prev = None
    for dilate in (0, 1, 2):
        want = U.build_model(sigma, thresh, dilate)
        buf = torch.full((n_words + 8,), SENT_I, dtype=torch.int32, device="cuda")
        N.check(N.lib.pnr_occ_build(field_ptr, stride, nx, ny, nz, thresh, dilate, 0, buf[4:].data_ptr(), stream), "pnr_occ_build")
        got = buf.cpu()
        assert bool((got[:4] == SENT_I).all()) and bool((got[-4:] == SENT_I).all()), dilate
        assert torch.equal(got[4:-4], torch.from_numpy(want.view(np.int32))), dilate
        if prev is not None:                                          # accumulate: a lower threshold ORed into the words before
            acc = buf[4:-4].clone()
            N.check(N.lib.pnr_occ_build(field_ptr, stride, nx, ny, nz, -5.0, 0, 1, acc.data_ptr(), stream), "pnr_occ_build")
            assert torch.equal(acc.cpu(), torch.from_numpy(U.build_model(sigma, -5.0, 0, prev=want).view(np.int32)))
        prev = want
    assert U.unpack_words(want, (nx - 1, ny - 1, nz - 1)).any()


# ------------------------------------------------------------------------------------------------------- pnr_ray_bounds
def _bounds_call(rays, R, cells, pad):
    """The entry point on buffers with sentinel margins -> (rays_out (n, 8), slot, counts) numpy, margins checked."""
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.render.occupancy import OccupancyGrid
    grid = OccupancyGrid.from_cells(torch.from_numpy(cells), *U.BOX, device="cuda")
    n = rays.shape[0]
    r = torch.from_numpy(rays).cuda()
    out = torch.full((n + 4, 8), SENT_F, device="cuda")
    slot = torch.full((n + 8,), SENT_I, dtype=torch.int32, device="cuda")
    counts = torch.full((n // R + 4,), SENT_I, dtype=torch.int64, device="cuda")
    nbytes = int(N.lib.pnr_ray_bounds_workspace_bytes(n, R))
    ws = torch.full((nbytes + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    N.check(N.lib.pnr_ray_bounds(r.data_ptr(), n, R, (C.c_double * 3)(*U.BOX[0]), (C.c_double * 3)(*U.BOX[1]),
                                 (C.c_int32 * 3)(*cells.shape), grid.bits.data_ptr(), float(pad), ws.data_ptr(), nbytes,
                                 out[2:].data_ptr(), slot[4:].data_ptr(), counts[2:].data_ptr(), N.current_stream(r.device)),
            "pnr_ray_bounds")
    torch.cuda.synchronize()
    out, slot, counts, ws = out.cpu().numpy(), slot.cpu().numpy(), counts.cpu().numpy(), ws.cpu().numpy()
    assert (out[:2] == SENT_F).all() and (out[-2:] == SENT_F).all()
    assert (slot[:4] == SENT_I).all() and (slot[-4:] == SENT_I).all()
    assert (counts[:2] == SENT_I).all() and (counts[-2:] == SENT_I).all()
    assert (ws[nbytes:] == 0x5A).all()
    return out[2:-2], slot[4:-4], counts[2:-2]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("grid_name", ["shell", "single", "full", "empty"])
def test_ray_bounds_equals_the_model_on_every_ray_kind(grid_name):
    cells = U.case_grids()[grid_name]
    rays = U.case_rays()
    for pad in (0.0, 0.07):
        rows, slot, counts = U.bounds_model(rays, len(rays), *U.BOX, cells, pad)
        got_rows, got_slot, got_counts = _bounds_call(rays, len(rays), cells, pad)
        assert np.array_equal(got_slot, slot) and np.array_equal(got_counts, counts)
        assert _same_bits(got_rows[:counts[0]], rows[0])
        assert (got_rows[counts[0]:] == SENT_F).all()                 # rows past the count are not written
    if grid_name in ("shell", "full"):
        assert 0 < counts[0] < len(rays)


@pytest.mark.parametrize("n,R", [(1, 1), (63, 63), (64, 64), (65, 65), (255, 255), (256, 256), (257, 257), (1000, 250)])
def test_ray_bounds_compaction_at_every_size(n, R):
    cells = U.case_grids()["shell"]
    base = U.case_rays(seed=n)
    rays = np.ascontiguousarray(np.tile(base, (n // len(base) + 1, 1))[np.random.default_rng(n).permutation(n) % len(base)][:n])
    rows, slot, counts = U.bounds_model(rays, R, *U.BOX, cells, 0.03)
    got_rows, got_slot, got_counts = _bounds_call(rays, R, cells, 0.03)
    assert np.array_equal(got_counts, counts) and np.array_equal(got_slot, slot)
    for f in range(n // R):
        assert _same_bits(got_rows[f * R:f * R + counts[f]], rows[f]), f
        assert (got_rows[f * R + counts[f]:(f + 1) * R] == SENT_F).all(), f
    if n >= 63:
        assert 0 < counts.sum() < n


# ------------------------------------------------------------------------------------------------------- pnr_frame_from_hits
@pytest.mark.parametrize("stride", [4, 7])
@pytest.mark.parametrize("bg", [0.0, 1.0])
def test_frame_from_hits_equals_the_model(stride, bg):
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    R, F = 37, 3
    n = R * F
    rng = np.random.default_rng(stride)
    hit = rng.random(n) < 0.6
    hit[R:2 * R] = False                                              # a frame with no hit
    slot = np.full(n, -1, np.int32)
    for f in range(F):
        idx = np.nonzero(hit[f * R:(f + 1) * R])[0] + f * R
        slot[idx] = np.arange(len(idx), dtype=np.int32)
    rec = rng.normal(size=(n, stride)).astype(np.float32)
    rec[~np.isin(np.arange(n), [f * R + s for f in range(F) for s in range(int(hit[f * R:(f + 1) * R].sum()))])] = np.nan
    want = U.frame_model(rec, slot, R, bg)
    store = torch.full((n + 2, 6), SENT_F, device="cuda")
    out = store[1:-1, :4]                                             # rows of 6 floats: the two behind each pixel stay
    got = occ.frame_from_hits(torch.from_numpy(rec).cuda(), torch.from_numpy(slot).cuda(), R, bg, out=out)
    assert got.data_ptr() == out.data_ptr()
    s = store.cpu().numpy()
    assert _same_bits(s[1:-1, :4], want) and not np.isnan(want).any()
    assert (s[0] == SENT_F).all() and (s[-1] == SENT_F).all() and (s[:, 4:] == SENT_F).all()
    assert (want[R:2 * R] == np.array([bg, bg, bg, 0.0], np.float32)).all()


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
    net.precision = "fp16"
    image = torch.rand(1, 3, SRC, SRC, generator=torch.Generator().manual_seed(100)) * 2 - 1
    pose = torch.from_numpy(np.asarray(gu.pose_spherical(13.0, -20.0, 2.0), dtype=np.float32))
    net.encode(image.cuda()[None], pose.cuda()[None, None], torch.tensor(SRC_FOCAL)[None].cuda())
    return net, rend


def _full_grid(half=5.0, cells=4):
    from pixel_nerf_multiscale_amd.render.occupancy import OccupancyGrid
    return OccupancyGrid.from_cells(torch.ones(cells, cells, cells, dtype=torch.bool), (-half,) * 3, (half,) * 3, device="cuda")


def _sphere_grid(radius=0.45, cells=16):
    from pixel_nerf_multiscale_amd.render.occupancy import OccupancyGrid
    x = (torch.arange(cells) + 0.5) / cells * 2 - 1
    i, j, k = torch.meshgrid(x, x, x, indexing="ij")
    return OccupancyGrid.from_cells((i * i + j * j + k * k).sqrt() < radius, (-1,) * 3, (1,) * 3, device="cuda")


def test_identity_with_a_full_grid_around_every_segment(scene):
    """Every ray hits and no bound moves: the bounded frames are render_image's under the frames' seeds, bit for bit."""
    from pixel_nerf_multiscale_amd import util, video
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    net, rend = scene
    assert net.resolved_precision(net.mlp_coarse, net.mlp_fine) == "fp16"
    poses = video.orbit_poses(2, -10, 2.0)
    seed, HW = 4242, SIDE * SIDE
    grid = _full_grid()
    rgb, depth = rend.render_frames_bounded(net, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, grid, pad=0.0, seed=seed)
    assert rgb.shape == (2, SIDE, SIDE, 3) and depth.shape == (2, SIDE, SIDE) and rgb.is_cuda
    rays = torch.cat([util.gen_rays_device(poses[f], SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR) for f in range(2)])
    rays_out, slot, counts = occ.ray_bounds(grid, rays, HW, pad=0.0)
    assert counts.tolist() == [HW, HW] and torch.equal(slot.view(2, HW), torch.arange(HW, dtype=torch.int32, device="cuda").expand(2, HW))
    assert torch.equal(rays_out.view(torch.int32), rays.view(torch.int32))
    for f in range(2):
        with rend.keyed(frame_seed(seed, f)):
            want_rgb, want_depth = rend.render_image(net, poses[f], SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR)
        assert torch.equal(rgb[f].view(torch.int32), want_rgb.view(torch.int32)), f
        assert torch.equal(depth[f].view(torch.int32), want_depth.view(torch.int32)), f
    assert rend.forced_seed is None


def _away(pose):
    """The same camera position, looking the other way (two axes flipped: still a rotation)."""
    p = pose.clone()
    p[:3, 0] *= -1
    p[:3, 2] *= -1
    return p


@pytest.mark.parametrize("white", [False, True])
def test_culling_background_hits_and_no_launch_for_an_empty_frame(scene, white, monkeypatch):
    from pixel_nerf_multiscale_amd import util, video
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    net, rend = scene
    poses = video.orbit_poses(2, -10, 2.0)
    poses = torch.stack([poses[0], _away(poses[1]), poses[1]])
    seed, HW = 99, SIDE * SIDE
    grid = _sphere_grid()
    launches = []
    fused = rend._forward_fused
    monkeypatch.setattr(rend, "white_bkgd", white)
    monkeypatch.setattr(rend, "_forward_fused", lambda *a, **k: (launches.append(a[1].shape[1]), fused(*a, **k))[1])
    rgb, depth = rend.render_frames_bounded(net, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, grid, pad=0.05, seed=seed)
    monkeypatch.setattr(rend, "_forward_fused", fused)
    rays = torch.cat([util.gen_rays_device(poses[f], SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR) for f in range(3)])
    rays_out, slot, counts = occ.ray_bounds(grid, rays, HW, pad=0.05)
    counts = counts.tolist()
    assert counts[1] == 0 and 0 < counts[0] < HW and 0 < counts[2] < HW
    assert launches == [counts[0], counts[2]]                         # the frame without a hit launched nothing
    miss = (slot < 0).view(3, SIDE, SIDE)
    bg = 1.0 if white else 0.0
    assert bool((rgb[miss] == bg).all()) and bool((depth[miss] == 0.0).all()) and bool(miss[1].all())
    for f in (0, 2):
        with rend.keyed(frame_seed(seed, f)):
            out = rend(net, rays_out[f * HW:f * HW + counts[f]][None]).fine
        assert torch.equal(rgb[f][~miss[f]].view(torch.int32), out.rgb[0].view(torch.int32)), f
        assert torch.equal(depth[f][~miss[f]].view(torch.int32), out.depth[0].view(torch.int32)), f
        near_far = rays_out[f * HW:f * HW + counts[f], 6:8]
        assert bool((near_far[:, 0] >= Z_NEAR).all()) and bool((near_far[:, 1] <= Z_FAR).all())
        # no longer than the ball of cells (radius 0.45 + half a cell diagonal of 0.2165) and the pad at both ends: 1.2165
        assert float((near_far[:, 1] - near_far[:, 0]).max()) <= 1.22 < Z_FAR - Z_NEAR


def test_from_net_equals_the_model_on_the_networks_own_sigma(scene):
    from pixel_nerf_multiscale_amd import util
    from pixel_nerf_multiscale_amd.render.occupancy import OccupancyGrid
    net, rend = scene
    reso, c1, c2 = (5, 6, 35), (-0.8, -0.7, -0.9), (0.9, 0.8, 0.7)
    with torch.no_grad():
        xyz, dirs = util.gen_grid_device(c1, c2, reso, fake_viewdirs=True, device="cuda")

        def sigma(coarse, d):
            out = net(xyz[None], coarse=coarse, viewdirs=d[None])
            return out.reshape(-1, out.shape[-1])[:, 3].cpu().numpy().reshape(reso)

        s_c = sigma(True, dirs)
        thresh = float(np.sort(s_c.reshape(-1))[-12])                 # 12 hot samples: some cells occupied, most not
        g = OccupancyGrid.from_net(net, sigma_thresh=thresh, c1=c1, c2=c2, reso=reso, dilate=1)
        want = U.build_model(s_c, thresh, 1)
        assert np.array_equal(_words(g.bits), want) and 0 < U.unpack_words(want, g.cell_counts).mean() < 1
        assert torch.equal(g.cells().cpu(), torch.from_numpy(U.unpack_words(want, g.cell_counts)))
        assert abs(g.occupied_fraction() - U.unpack_words(want, g.cell_counts).mean()) < 1e-6
        both = OccupancyGrid.from_net(net, sigma_thresh=thresh, c1=c1, c2=c2, reso=reso, dilate=0, mlps=("coarse", "fine"))
        assert np.array_equal(_words(both.bits), U.build_model(s_c, thresh, 0) | U.build_model(sigma(False, dirs), thresh, 0))
        vd = torch.tensor([[0.0, 0.0, -1.0], [0.6, 0.0, 0.8], [0.0, 1.0, 0.0]])
        many = OccupancyGrid.from_net(net, sigma_thresh=thresh, c1=c1, c2=c2, reso=reso, dilate=0, viewdirs=vd)
        want = np.zeros_like(want)
        for v in vd:
            want |= U.build_model(sigma(True, v.cuda()[None].expand(xyz.shape[0], 3).contiguous()), thresh, 0)
        assert np.array_equal(_words(many.bits), want)


class _Ball:
    """The reference's model protocol: a solid sphere of constant density and colour."""
    use_viewdirs = False

    def __call__(self, xyz, coarse=True, viewdirs=None):
        inside = (xyz.norm(dim=-1, keepdim=True) < 0.2).float()
        return torch.cat([torch.full_like(xyz, 0.5) * inside, 8.0 * inside], dim=-1)


def test_the_value_of_the_bounds_measured_on_a_solid_sphere():
    """16 coarse samples per ray, over the tightened bounds and over [z_near, z_far], against 1024 samples over [z_near,
    z_far].  Asserted: the bounded mean squared error is no larger than the unbounded one plus the unbounded spread
    (max - min) over the same 5 seeds, measured in this run."""
    from pixel_nerf_multiscale_amd import NeRFRenderer, video
    model = _Ball()
    pose = video.orbit_poses(1, -10, 2.0)
    grid = _sphere_grid(radius=0.2 + 0.055, cells=32)                 # every cell the ball reaches into: half a cell diagonal is 0.0541
    coarse = NeRFRenderer(n_coarse=16, n_fine=0).cuda().eval()
    fine = NeRFRenderer(n_coarse=1024, n_fine=0).cuda().eval()
    ref = fine.render_frames_bounded(model, pose, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, _full_grid(), pad=0.0, seed=1)[0][0]
    mse_b, mse_u = [], []
    for seed in range(5):
        b = coarse.render_frames_bounded(model, pose, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, grid, seed=seed)[0][0]
        u = coarse.render_frames_bounded(model, pose, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, _full_grid(), pad=0.0, seed=seed)[0][0]
        mse_b.append(float(((b - ref) ** 2).mean()))
        mse_u.append(float(((u - ref) ** 2).mean()))
    print(f"solid sphere, 16 samples per ray, mse vs 1024 samples over 5 seeds: bounded mean {np.mean(mse_b):.3e} "
          f"(min {min(mse_b):.3e} max {max(mse_b):.3e}), unbounded mean {np.mean(mse_u):.3e} (min {min(mse_u):.3e} max {max(mse_u):.3e})")
    assert float(ref.max()) > 0.3                                     # the ball is in the picture
    assert np.mean(mse_b) <= np.mean(mse_u) + (max(mse_u) - min(mse_u))


def test_render_video_with_a_grid_is_video_frames_of_the_bounded_frames(scene):
    from pixel_nerf_multiscale_amd import util, video
    net, rend = scene
    poses = video.orbit_poses(2, -10, 2.0)
    grid = _sphere_grid()
    frames, count = video.render_video(net, rend, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, seed=31, occupancy=grid)
    rgb = rend.render_frames_bounded(net, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, grid, seed=31)[0]
    want, want_count = util.video_frames(rgb.contiguous(), 2, SIDE, SIDE)
    assert frames.shape == (2, SIDE, SIDE, 3) and torch.equal(frames, want) and int(count) == int(want_count)
    plain, _ = video.render_video(net, rend, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, seed=31)
    assert not torch.equal(plain, frames)
    by_dict, _ = video.render_video(net, rend, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, seed=31,
                                    occupancy=dict(sigma_thresh=float("-inf"), c1=(-5,) * 3, c2=(5,) * 3, reso=3, pad=0.0))
    assert torch.equal(by_dict, plain)                                # a full grid around every segment: the plain video


def test_one_host_read(scene, monkeypatch):
    from pixel_nerf_multiscale_amd import video
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    net, rend = scene
    poses = video.orbit_poses(3, -10, 2.0)
    grid = _sphere_grid()
    args = (net, poses, SIDE, SIDE, FOCAL, Z_NEAR, Z_FAR, grid)
    want = rend.render_frames_bounded(*args, seed=5)                  # warm-up: allocations, code objects
    reads = []
    read = occ.read_counts

    def exempt(counts):                                               # the one read, let through
        reads.append(counts.numel())
        torch.cuda.set_sync_debug_mode("default")
        try:
            return read(counts)
        finally:
            if works:
                torch.cuda.set_sync_debug_mode("error")

    monkeypatch.setattr(occ, "read_counts", exempt)
    works = sync_debug_mode_works()
    print(f'torch.cuda.set_sync_debug_mode("error") works under this build: {works}')
    if works:
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = rend.render_frames_bounded(*args, seed=5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reads == [3]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])     # and a frame is reproducible under its seed


# ------------------------------------------------------------------------------------------------------- evaluate
def _tree_files(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_evaluate_with_occupancy_on_an_srn_tree(tmp_path):
    import data_trees as dt
    import golden_util as gu
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio
    from pixel_nerf_multiscale_amd.data import ResizedDataset, get_split_dataset
    NV, stems = 3, ["000000", "000001", "000002"]
    for stage in ("train", "val", "test"):
        for o in range(2):
            images = dt.boxed_views(NV, 16, 16, [(2 + v, 3, 12, 13 - v) for v in range(NV)], seed=10 * o + 1)
            poses = np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(NV)]).astype(np.float32)
            poses[:, :, 1:3] *= -1.0
            dt.write_srn_object(str(tmp_path / "srn" / f"cars_{stage}" / f"obj{o}"), images, poses, 16.5, 8.5, 7.25, stems)
    data = ResizedDataset(get_split_dataset("srn", str(tmp_path / "srn" / "cars"), want_split="val", as_bytes=False), (8, 8))
    torch.manual_seed(0)
    conf = model_conf(dict(gu.CASES["tiny_ns2_codeview"]), "fp32")
    conf["encoder"]["num_layers"] = 3
    conf["encoder"]["use_first_pool"] = False
    net = PixelNeRFNet(conf).cuda().eval()
    rend = NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, white_bkgd=True).cuda().eval()
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        kw = dict(source="0", verbose=False, seed=5)
        evalio.evaluate(net, rend, data, str(tmp_path / "plain"), **kw)
        full = dict(sigma_thresh=float("-inf"), c1=(-6,) * 3, c2=(6,) * 3, reso=3, pad=0.0)
        evalio.evaluate(net, rend, data, str(tmp_path / "full"), occupancy=full, **kw)
        plain, bounded = _tree_files(tmp_path / "plain"), _tree_files(tmp_path / "full")
        assert sorted(plain) == sorted(bounded) and "finish.txt" in plain and sum(k.endswith(".png") for k in plain) == 4
        assert plain == bounded                                       # finish.txt and every PNG, byte for byte
        with torch.no_grad():                                         # a finite threshold: the median density of object 0
            item = data[0]
            net.encode(item["images"][:1].cuda()[None], item["poses"][:1].cuda()[None], torch.as_tensor(item["focal"]).float()[None].cuda(),
                       c=torch.as_tensor(item["c"]).float().cuda()[None])
            xyz = (torch.rand(1, 512, 3, device="cuda") - 0.5)
            thresh = float(net(xyz, coarse=True, viewdirs=torch.nn.functional.normalize(-xyz, dim=-1))[..., 3].median())
        finite = dict(sigma_thresh=thresh, c1=(-0.5,) * 3, c2=(0.5,) * 3, reso=9)
        out = str(tmp_path / "finite")
        m1 = evalio.evaluate(net, rend, data, out, occupancy=finite, max_objects=1, **kw)
        first = _tree_files(out)
        m2 = evalio.evaluate(net, rend, data, out, occupancy=finite, **kw)       # resumes: object 0 is skipped, object 1 added
        assert m1[2] == 1 and m2[2] == 2 and all(first[k] == v for k, v in _tree_files(out).items() if k.startswith("obj0"))
        out2 = str(tmp_path / "finite2")
        evalio.evaluate(net, rend, data, out2, occupancy=finite, **kw)
        assert _tree_files(out) == _tree_files(out2)                  # the same files twice
    finally:
        torch.backends.cudnn.deterministic = was
