"""CPU-side tests: the C-ABI library loads and exports every symbol include/pnr.h declares (no compute
without a GPU), the ctypes structs match the header's layout, and the host logic mirrors the reference."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_declarations():
    """(name, return kind, [parameter kinds]) of every function include/pnr.h declares, comments stripped.  Kinds: "pointer",
    "int32_t", "int64_t", "uint64_t", "float", "double" (and "void" for a return)."""
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    hdr = re.sub(r"^\s*#.*$", " ", hdr, flags=re.M)

    def kind(decl):
        decl = decl.strip()
        if "*" in decl or "[" in decl:
            return "pointer"
        words = [w for w in decl.split() if w not in ("const", "unsigned", "signed")]
        base = next((w for w in words if w in ("int32_t", "int64_t", "uint64_t", "float", "double", "void", "int")), None)
        assert base is not None, decl
        return "int32_t" if base == "int" else base

    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(pnr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        params = params.strip()
        out.append((name, kind(ret), [] if params in ("", "void") else [kind(q) for q in params.split(",")]))
    return out


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "contents"):          # POINTER(...) types carry `contents`
        return "pointer"
    return {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t", ctypes.c_float: "float",
            ctypes.c_double: "double"}[t]


def test_library_exports_every_declared_symbol():
    """Every function of include/pnr.h has a prototype in _native.PROTOTYPES and the other way round, with the header's return
    type and the kind of every parameter, and the loaded library's functions carry exactly those."""
    from pixel_nerf_multiscale_amd import _native as N
    decls = _header_declarations()
    declared = [d[0] for d in decls]
    assert declared and len(declared) == len(set(declared)), "no prototypes parsed, or one parsed twice"
    assert set(declared) == set(N.PROTOTYPES), set(declared) ^ set(N.PROTOTYPES)
    wrong = []
    for name, ret, params in decls:
        res, args = N.PROTOTYPES[name]
        if (_ctypes_kind(res), [_ctypes_kind(a) for a in args]) != (ret, params):
            wrong.append((name, ret, params, _ctypes_kind(res), [_ctypes_kind(a) for a in args]))
        assert hasattr(N.lib, name), name
        fn = getattr(N.lib._cdll, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert not wrong, wrong
    assert N.lib.pnr_version() == 102
    assert N.lib.pnr_error_string(-4).decode() == "workspace too small"


def test_struct_layout_matches_header():
    from pixel_nerf_multiscale_amd import _native as N
    src = '#include <stdio.h>\n#include "pnr.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pnr_mlp), sizeof(pnr_views), sizeof(pnr_params), sizeof(pnr_noise), sizeof(pnr_outputs), sizeof(pnr_mlp_grads));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [ctypes.sizeof(s) for s in (N.pnr_mlp, N.pnr_views, N.pnr_params, N.pnr_noise, N.pnr_outputs, N.pnr_mlp_grads)]


def test_null_and_shape_errors_without_gpu():
    """Argument validation happens before any HIP call."""
    from pixel_nerf_multiscale_amd import _native as N
    assert N.lib.pnr_sample_coarse(None, 4, 8, 0, None, 0, 0, None, None) == -1
    assert N.lib.pnr_composite(None, None, None, 4, 8, 0, None, None, None, None) == -1
    assert N.lib.pnr_gen_rays(None, 4, 4, 1.0, 1.0, 2.0, 2.0, 0.1, 1.0, 0, 16, None, None) == -1
    assert N.lib.pnr_resnetfc_forward(None, None, 1, 1, 1, None, None, 0, None) == -1
    assert N.lib.pnr_resnetfc_workspace_bytes(None, 1) == 0
    assert N.lib.pnr_index_latent(None, None, 4, 1, None, None) == -1
    assert N.lib.pnr_render_camera(None, None, None, None, None, 4, 4, 1.0, 1.0, 2.0, 2.0, 0.1, 1.0, 0, 16, None, 0, 0,
                                   None, None, 0, None) == -1
    with pytest.raises(ValueError):
        N.check(-2, "x")
    with pytest.raises(RuntimeError):
        N.ptr(torch.zeros(3))          # CPU tensors never reach the library


def test_state_dict_keys_match_reference_layout():
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import PixelNeRFNet
    spec = gu.CASES["full_ns1"]
    net = PixelNeRFNet(model_conf(spec))
    keys = set(net.state_dict().keys())
    for which in ("mlp_coarse", "mlp_fine"):
        for k, v in gu.make_mlp_state(spec, "coarse").items():
            assert f"{which}.{k}" in keys
            assert tuple(net.state_dict()[f"{which}.{k}"].shape) == v.shape
    assert tuple(net.state_dict()["code._freqs"].shape) == (1, 12, 1)
    assert tuple(net.state_dict()["code._phases"].shape) == (1, 12, 1)
    assert "encoder.model.layer3.5.conv2.weight" in keys and "encoder.layers.0.0.weight" in keys
    assert sum(p.numel() for p in net.mlp_coarse.parameters()) == 3045380
    assert net.d_in == 42 and net.d_latent == 256 and net.latent_size == 256


@pytest.mark.parametrize("name", ["tiny_ns2_lindisp_black", "tiny_sb2_ns2", "full_ns3"])
def test_set_cameras_matches_reference_encode(name):
    from hip_util import build_net
    fx = gu.load_fixture(name)
    net = build_net(fx["spec"], fx["poses"], device="cpu")
    assert np.abs(net.poses.numpy() - fx["enc_w2c"]).max() < 1e-6
    assert np.array_equal(net.focal.numpy(), fx["enc_focal"])
    assert np.array_equal(net.c.numpy(), fx["enc_c"])
    assert np.array_equal(net.image_shape.numpy(), fx["enc_image_shape"])


def test_gen_rays_and_pose_spherical():
    from pixel_nerf_multiscale_amd import util
    c2w = util.pose_spherical(75.0, -25.0, 2.0)
    ref = gu.pose_spherical(75.0, -25.0, 2.0)
    assert np.abs(c2w.numpy() - ref).max() < 1e-6
    W, H, f = 40, 30, 45.0
    rays = util.gen_rays(c2w[None], W, H, torch.tensor(f), 1.25, 2.75)
    assert rays.shape == (1, H, W, 8)
    pix = np.arange(W * H)
    ref_rays = gu.pinhole_rays(ref, W, H, f, 1.25, 2.75, pix)
    assert np.abs(rays.reshape(-1, 8).numpy() - ref_rays).max() < 1e-6


def test_renderer_surface_and_schedule():
    from pixel_nerf_multiscale_amd import NeRFRenderer
    r = NeRFRenderer.from_conf(dict(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True,
                                    sched=[[2, 4], [16, 32], [8, 16]]), lindisp=False)
    assert (r.n_coarse, r.n_fine, r.n_fine_depth, r.using_fine, r.eval_batch_size) == (64, 32, 16, True, 100000)
    assert set(r.state_dict()) == {"iter_idx", "last_sched"} and r.iter_idx.dtype == torch.long
    r.sched_step(1)
    assert (r.n_coarse, r.n_fine) == (64, 32)
    r.sched_step(1)
    assert (r.n_coarse, r.n_fine, int(r.last_sched)) == (16, 8, 1)
    r.sched_step(5)
    assert (r.n_coarse, r.n_fine, int(r.last_sched)) == (32, 16, 2)
    d = NeRFRenderer()
    assert (d.n_coarse, d.n_fine, d.white_bkgd, d.lindisp, d.sched) == (128, 0, False, False, None)
    with pytest.warns(UserWarning):          # several ids, no process group: one device, with a warning (a16)
        w = d.bind_parallel(None, gpus=[0, 1])
    assert type(w).__name__ == "_RenderWrapper"


def test_container_modules_do_not_evaluate_in_pytorch():
    """ResnetFC.forward / SpatialEncoder.index are native stage calls: no CPU tensors, no PyTorch evaluation."""
    from pixel_nerf_multiscale_amd.model import ResnetFC, SpatialEncoder
    with pytest.raises(RuntimeError):
        ResnetFC(42, d_latent=8, d_hidden=32)(torch.zeros(2, 50))
    with pytest.raises(NotImplementedError):
        ResnetFC(42, d_latent=8, d_hidden=32)(torch.zeros(2, 50), combine_index=torch.zeros(2))
    enc = SpatialEncoder(pretrained=False)
    with pytest.raises(RuntimeError):
        enc.index(torch.zeros(1, 2, 2))          # no latent yet
    enc(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError):
        enc.index(torch.zeros(1, 2, 2))          # CPU tensors never reach the library
    # the conv trunk itself is ordinary PyTorch (runs once per object, out of the hot path)
    lat = enc(torch.zeros(1, 3, 64, 64))
    assert lat.shape == (1, 256, 4, 4) and enc.latent_size == 256
    ms = SpatialEncoder(pretrained=False, use_multi_scale=True, use_first_pool=False)
    lats = ms(torch.zeros(2, 3, 64, 64))
    assert [tuple(l.shape[1:]) for l in lats] == [(64, 32, 32), (64, 32, 32), (128, 16, 16), (256, 8, 8)]


def test_training_and_projection_switches_host_logic():
    """Routing and descriptor logic that needs no GPU: which calls take the differentiable path, the parameter order the
    training Functions exchange with the C ABI, argument errors of the training / projected-pack entry points."""
    import hip_util as hu
    from pixel_nerf_multiscale_amd import PixelNeRFNet, _native as N
    from pixel_nerf_multiscale_amd.model.models import mlp_tensors
    from pixel_nerf_multiscale_amd.render import autograd as ag
    spec = gu.CASES["tiny_ns1"]
    net = PixelNeRFNet(hu.model_conf(spec))
    assert net.project_latent and net.train_precision == "fp32" and net.differentiable is None
    x = torch.zeros(1, 4, 3)
    net.eval()
    assert not net.wants_grad(x)                       # eval(): fused kernels
    net.train()
    net.encoder.latent = torch.zeros(1, 512, 2, 2)
    net.encoder._level_maps = [net.encoder.latent]
    assert net.wants_grad(x)                           # training mode + parameters requiring grad
    with torch.no_grad():
        assert not net.wants_grad(x)
    net.differentiable = False
    assert not net.wants_grad(x)
    net.differentiable = None
    for p in net.parameters():
        p.requires_grad_(False)
    assert not net.wants_grad(x) and net.wants_grad(x.clone().requires_grad_(True))
    # parameter order <-> pnr_mlp / pnr_mlp_grads slots
    mlp = net.mlp_coarse
    ts = mlp_tensors(mlp)
    assert ts[0] is mlp.lin_in.weight and ts[3] is mlp.lin_out.bias and ts[4] is mlp.blocks[0].fc_0.weight
    assert ts[-1] is mlp.lin_z[-1].bias and len(ts) == 4 + 4 * mlp.n_blocks + 2 * len(mlp.lin_z)
    hdr = dict(n_blocks=mlp.n_blocks, n_lin_z=len(mlp.lin_z))
    marks = [object() for _ in ts]

    class P:     # stand-in with a data_ptr, so the slot mapping can be checked without device memory
        is_cuda = True
        def __init__(self, i): self.i = i
        def data_ptr(self): return 1000 + self.i
    g = ag._grads_struct_from(hdr, [P(i) for i in range(len(ts))])
    assert g.lin_in_w == 1000 and g.lin_out_b == 1003 and g.fc0_w[0] == 1004 and g.fc1_b[0] == 1007
    assert g.lin_z_b[len(mlp.lin_z) - 1] == 1000 + len(ts) - 1
    # argument validation before any HIP call
    assert N.lib.pnr_train_tape_bytes(None, None, 10) == 0
    assert N.lib.pnr_composite_bwd(None, None, None, 4, 8, 0, None, None, None, None, None, None) == -1
    assert N.lib.pnr_sample_fine_bwd(None, None, 4, 8, 4, 2, 0.01, None, 0, 0, None, None, None, None) == -1
    assert N.lib.pnr_packed_mlp_projected_bytes(None, None) == 0
    assert N.lib.pnr_pack_mlp_projected(None, None, N.PNR_BF16, None, 0, None) == -1


def test_gen_rays_mirror_matches_reference_fixture():
    """N1: util.gen_rays / unproj_map / pose_spherical (host mirrors of reference util.py:118-148,243-281,314-328) against
    the reference's own outputs (tests/golden/gen_rays.npz): both principal-point conventions, (fx, fy) focal,
    non-square and odd sizes, a batch of poses."""
    import numpy as np
    import torch
    import golden_util as gu
    from pixel_nerf_multiscale_amd import util
    for cs in gu.load_rays_fixture():
        poses = torch.stack([util.pose_spherical(*cam) for cam in cs["cams"]])
        assert np.abs(poses.numpy() - cs["poses"]).max() <= 1e-6, cs["name"]
        c = None if cs["c"] is None else torch.from_numpy(cs["c"])
        rays = util.gen_rays(torch.from_numpy(cs["poses"]), cs["W"], cs["H"], torch.from_numpy(cs["focal"]), cs["z_near"],
                             cs["z_far"], c=c)
        assert rays.shape == cs["rays"].shape
        assert np.abs(rays.numpy() - cs["rays"]).max() <= 2e-6, cs["name"]


@pytest.mark.parametrize("M,N,Rn,rows,split", [(49152, 512, 512, 0, 0), (32768, 512, 512, 0, 0), (300, 42, 512, 0, 0), (129, 512, 64, 0, 0),
                                               (512, 512, 40960, 1024, 1), (512, 42, 3000, 1024, 1), (4, 512, 100, 64, 1)])
def test_tile_gemm_grid_is_a_bijection_and_xcd_local(M, N, Rn, rows, split):
    """The 1-D, XCD-aware launch grid of the tile GEMMs (fp32 path + training path; csrc/train_f32.hip mgemm_grid /
    mgemm_tile_of), through its host-side diagnostics: every (m tile, n tile[, split]) is visited exactly once, padding
    workgroups are the rest, and the tiles that share an operand — the n tiles of one m tile, or all tiles of one split —
    sit on ONE XCD (workgroup id mod 8) in consecutive slots."""
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N_
    grid = N_.lib.pnr_debug_gemm_grid(M, N, Rn, rows, split)
    gx, gy = (M + 127) // 128, (N + 127) // 128
    gz = (Rn + rows - 1) // rows if split else 1
    assert grid % 8 == 0 and grid >= gx * gy * gz
    out = (C.c_int32 * 3)()
    seen, by_group = {}, {}
    for b in range(grid):
        if N_.lib.pnr_debug_gemm_tile(b, M, N, Rn, rows, split, out):
            tile = (out[0], out[1], out[2])
            assert tile not in seen and 0 <= tile[0] < gx and 0 <= tile[1] < gy and 0 <= tile[2] < gz
            seen[tile] = b
            by_group.setdefault(tile[2] if split else tile[0], []).append(b)
    assert len(seen) == gx * gy * gz
    for grp, blocks in by_group.items():
        assert len({b % 8 for b in blocks}) == 1                                   # one XCD
        slots = sorted(b // 8 for b in blocks)
        assert slots == list(range(slots[0], slots[0] + len(slots)))              # consecutive slots of that XCD


def test_headline_dtype_is_held_to_survey_8c():
    """a 16-bit render is >= 50 dB from the fp32 path on every synthetic config.  The dtype bench.py quotes its
    headline on must be the dtype the GPU suite holds to that bound (coarse pass, injected fine positions, fine end to end);
    any other 16-bit format is labelled non-conforming there and appears in the bench as a secondary row only."""
    import bench
    import test_gpu_parity as tp
    h = bench.HEADLINE_DTYPE
    assert h == "fp16" and h not in tp.NON_CONFORMING_DTYPES
    assert bench.PSNR_BOUND_8C_DB == tp.SURVEY_8C_DB == 50.0
    assert tp.FLOOR_DB[h] >= tp.SURVEY_8C_DB and tp.FINE_E2E_FLOOR_DB[h] >= tp.SURVEY_8C_DB
    assert bench.SECONDARY[0] == (bench.DEFAULT, "bf16")          # the other 16-bit format stays visible beside the headline
    # every BASELINE shape is benchmarked in the headline dtype
    for wl in bench.WORKLOADS:
        assert wl == bench.DEFAULT or (wl, h) in bench.SECONDARY, wl


# pnr_train_tape_bytes_for (and, after each fp32 entry, pnr_train_tape_bytes) over _tape_configs(), in its order
_TAPE_BYTES = (
    164096, 164096, 167424, 167424, 12484864, 12484864, 256, 4096, 8651008, 164096, 167424, 12484864, 164096, 164096,
    167424, 167424, 12484864, 12484864, 256, 4096, 8651008, 164096, 167424, 12484864, 164096, 164096, 167424, 167424,
    12484864, 12484864, 256, 4096, 8651008, 164096, 167424, 12484864, 164096, 164096, 168704, 168704, 17072384, 17072384,
    256, 6400, 17432832, 164096, 168704, 17072384, 164096, 164096, 171776, 171776, 29655296, 29655296, 256, 7936, 23724288,
    164096, 171776, 29655296, 189696, 189696, 193536, 193536, 14148864, 14148864, 25856, 30208, 10315008, 189696, 193536,
    14148864, 266496, 266496, 270336, 270336, 14225664, 14225664, 25856, 30208, 10315008, 266496, 270336, 14225664, 317696,
    317696, 321536, 321536, 14276864, 14276864, 25856, 30208, 10315008, 317696, 321536, 14276864, 240896, 240896, 246528,
    246528, 22064384, 22064384, 77056, 84224, 22424832, 240896, 246528, 22064384, 317696, 317696, 326400, 326400, 34724096,
    34724096, 77056, 85760, 28716288, 317696, 326400, 34724096, 295168, 295168, 300544, 300544, 21004544, 21004544, 131328,
    137216, 17170688, 295168, 300544, 21004544, 688384, 688384, 693760, 693760, 21397760, 21397760, 131328, 137216,
    17170688, 688384, 693760, 21397760, 950528, 950528, 955904, 955904, 21659904, 21659904, 131328, 137216, 17170688,
    950528, 955904, 21659904, 557312, 557312, 568064, 568064, 42631424, 42631424, 393472, 405760, 42991872, 557312, 568064,
    42631424, 950528, 950528, 964352, 964352, 55607552, 55607552, 393472, 407296, 49283328, 950528, 964352, 55607552, 256,
    256, 6400, 6400, 22413568, 22413568, 256, 6400, 22413568, 256, 6400, 22413568, 256, 256, 6400, 6400, 22413568, 22413568,
    256, 6400, 22413568, 256, 6400, 22413568, 256, 256, 6400, 6400, 22413568, 22413568, 256, 6400, 22413568, 256, 6400,
    22413568, 256, 256, 8448, 8448, 29753600, 29753600, 256, 8448, 29753600, 256, 8448, 29753600, 256, 256, 14592, 14592,
    53346560, 53346560, 256, 14592, 53346560, 256, 14592, 53346560, 25856, 25856, 32512, 32512, 24077568, 24077568, 25856,
    32512, 24077568, 25856, 32512, 24077568, 25856, 25856, 32512, 32512, 24077568, 24077568, 25856, 32512, 24077568, 25856,
    32512, 24077568, 25856, 25856, 32512, 32512, 24077568, 24077568, 25856, 32512, 24077568, 25856, 32512, 24077568, 77056,
    77056, 86272, 86272, 34745600, 34745600, 77056, 86272, 34745600, 77056, 86272, 34745600, 77056, 77056, 92416, 92416,
    58338560, 58338560, 77056, 92416, 58338560, 77056, 92416, 58338560, 131328, 131328, 139520, 139520, 30933248, 30933248,
    131328, 139520, 30933248, 131328, 139520, 30933248, 131328, 131328, 139520, 139520, 30933248, 30933248, 131328, 139520,
    30933248, 131328, 139520, 30933248, 131328, 131328, 139520, 139520, 30933248, 30933248, 131328, 139520, 30933248,
    131328, 139520, 30933248, 393472, 393472, 407808, 407808, 55312640, 55312640, 393472, 407808, 55312640, 393472, 407808,
    55312640, 393472, 393472, 413952, 413952, 78905600, 78905600, 393472, 413952, 78905600, 393472, 413952, 78905600,
    10486016, 10486016, 10509056, 10509056, 103547136, 103547136, 10486016, 10501888, 74187008, 10486016, 10509056,
    103547136, 10486016, 10486016, 10509056, 10509056, 103547136, 103547136, 10486016, 10501888, 74187008, 10486016,
    10509056, 103547136, 10486016, 10486016, 10509056, 10509056, 103547136, 103547136, 10486016, 10501888, 74187008,
    10486016, 10509056, 103547136, 10486016, 10486016, 10515712, 10515712, 130154752, 130154752, 10486016, 10516736,
    134349056, 10486016, 10515712, 130154752, 10486016, 10486016, 10540288, 10540288, 230818048, 230818048, 10486016,
    10529024, 184680704, 10486016, 10540288, 230818048, 10511616, 10511616, 10535168, 10535168, 105211136, 105211136,
    10511616, 10528000, 75851008, 10511616, 10535168, 105211136, 11126016, 11126016, 11149568, 11149568, 105825536,
    105825536, 10511616, 10528000, 75851008, 11126016, 11149568, 105825536, 11535616, 11535616, 11559168, 11559168,
    106235136, 106235136, 10511616, 10528000, 75851008, 11535616, 11559168, 106235136, 10562816, 10562816, 10593536,
    10593536, 135146752, 135146752, 10562816, 10594560, 139341056, 10562816, 10593536, 135146752, 11177216, 11177216,
    11232512, 11232512, 236424448, 236424448, 10562816, 10606848, 189672704, 11177216, 11232512, 236424448, 10617088,
    10617088, 10642176, 10642176, 112066816, 112066816, 10617088, 10636032, 86900992, 10617088, 10642176, 112066816,
    13762816, 13762816, 13787904, 13787904, 115212544, 115212544, 13762816, 13781760, 90046720, 13762816, 13787904,
    115212544, 15859968, 15859968, 15885056, 15885056, 117309696, 117309696, 15859968, 15878912, 92143872, 15859968,
    15885056, 117309696, 10879232, 10879232, 10915072, 10915072, 155713792, 155713792, 10879232, 10919168, 172491008,
    10879232, 10915072, 155713792, 14024960, 14024960, 14085376, 14085376, 259522816, 259522816, 14024960, 14077184,
    225968384, 14024960, 14085376, 259522816,
)


def _tape_configs():
    import itertools
    return itertools.product((64, 120, 512), (0, 100, 512), ((1, 0), (1, 3), (1, 5), (3, 0), (3, 3)),
                             ("fp32", "bf16", "bf16_tape_fp32"), (0, 1, 4096))


def test_train_tape_bytes_are_pinned():
    """The training tape's layout (csrc/train_f32.hip carve_tape), seen through its size: d_hidden that suits no MFMA kernel /
    the bf16 MFMA kernel / the LDS-DMA kernels, d_latent absent / unaligned / suiting the LDS-DMA lin_z, one view and three,
    the view reduction in front of block 0, inside the chain and (one view) behind it, the fp32 tape, the 16-bit tape and the
    fp32 tape under bf16 products, and 0, 1 and 4096 points.  The values are those of the layout the kernels were measured on."""
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    got = []
    for H, L, (NS, cl), prec, P in _tape_configs():
        mlp = N.pnr_mlp(d_in=42, d_latent=L, d_hidden=H, d_out=4, n_blocks=5, combine_layer=cl)
        vw = N.pnr_views(n_objs=1, n_views=NS, n_levels=1 if L else 0)
        vw.lat_c[0], vw.lat_h[0], vw.lat_w[0] = L, 8, 8
        prm = N.pnr_params(precision=N.PNR_F32 if prec == "fp32" else N.PNR_BF16, train_tape_fp32=int(prec == "bf16_tape_fp32"))
        got.append(((H, L, NS, cl, prec, P), N.lib.pnr_train_tape_bytes_for(C.byref(prm), C.byref(mlp), C.byref(vw), P)))
        if prec == "fp32":
            got.append(((H, L, NS, cl, "no params", P), N.lib.pnr_train_tape_bytes(C.byref(mlp), C.byref(vw), P)))
    assert len(got) == len(_TAPE_BYTES) == 540
    wrong = [(cfg, v, want) for (cfg, v), want in zip(got, _TAPE_BYTES) if v != want]
    assert not wrong, wrong[:5]


# ----------------------------------------------------------------------------- the host layer of a render call
_POSE = [[1.0, 0.0, 0.0, 0.5], [0.0, 0.0, -1.0, 2.0], [0.0, 1.0, 0.0, -0.25], [0.0, 0.0, 0.0, 1.0]]
_POSE16 = [1.0, 0.0, 0.0, 0.5, 0.0, 0.0, -1.0, 2.0, 0.0, 1.0, 0.0, -0.25, 0.0, 0.0, 0.0, 1.0]


@pytest.mark.parametrize("pose", [torch.tensor(_POSE), np.array(_POSE), np.array(_POSE, dtype=np.float32), _POSE],
                         ids=["tensor", "float64 array", "float32 array", "nested list"])
def test_camera_record_is_the_tuple_the_call_sites_built(pose):
    """util.camera against the 11 values render_image, render_video and the sampler test spelled out by hand: (fx, fy) and
    scalar focal, a given principal point and the image centre, a pixel range and the whole image."""
    from pixel_nerf_multiscale_amd import util
    cam = util.camera(pose, 24, 17, (30.0, 33.0), 1.25, 2.75, c=(12.0, 8.5), pix0=37, n=131)
    assert cam == (_POSE16, 24, 17, 30.0, 33.0, 12.0, 8.5, 1.25, 2.75, 37, 131)
    whole = (_POSE16, 24, 17, 30.0, 30.0, 12.0, 8.5, 1.25, 2.75, 0, 408)
    assert util.camera(pose, 24, 17, 30.0, 1.25, 2.75) == whole                                 # c=None: (W / 2, H / 2); n=None: W H
    assert util.camera(pose, 24.0, 17.0, torch.tensor([30.0]), np.float32(1.25), 2.75, c=None, n=None) == whole
    assert util.camera(pose, 24, 17, torch.tensor([[30.0, 33.0]]), 1.25, 2.75, c=np.array([[12.0, 8.5]]))[3:7] == (30.0, 33.0, 12.0, 8.5)
    assert (cam.c2w16, cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy, cam.z_near, cam.z_far, cam.pix0, cam.n) == tuple(cam)
    # host values only: nothing in the record is a tensor, so building it cannot touch a device
    assert [type(v) for v in cam] == [list, int, int, float, float, float, float, float, float, int, int]
    assert all(type(x) is float for x in cam.c2w16)
    args = cam.c_args()
    assert list(args[0]) == _POSE16 and args[1:] == tuple(cam)[1:]


@pytest.mark.parametrize("focal,c,want", [((30.0, 33.0), (12.0, 8.5), (30.0, 33.0, 12.0, 8.5)), (30.0, None, (30.0, 30.0, 12.0, 8.5)),
                                          ((30.0, 33.0), (11.25, 9.0), (30.0, 33.0, 11.25, 9.0))])
def test_intrinsics_are_what_unproj_map_uses(focal, c, want):
    """util.intrinsics is the parse, and unproj_map's directions are to the bit those of the parse written out by hand."""
    from pixel_nerf_multiscale_amd import util
    W, H = 24, 17
    assert util.intrinsics(focal, c, W, H) == want
    assert util.intrinsics(torch.tensor(focal), None if c is None else np.array(c), W, H) == want
    fx, fy, cx, cy = want
    ys = (torch.arange(H, dtype=torch.float32) - cy) / fy
    xs = (torch.arange(W, dtype=torch.float32) - cx) / fx
    Y, X = torch.meshgrid(ys, xs, indexing="ij")
    d = torch.stack((X, -Y, -torch.ones_like(X)), dim=-1)
    assert torch.equal(util.unproj_map(W, H, focal, c=c), d / d.norm(dim=-1, keepdim=True))


@pytest.mark.parametrize("d_latent", [8, 0])
def test_mlp_field_table_is_the_one_order(d_latent):
    """The slots of models.mlp_slots: as many as mlp_tensors() gives parameters, each a field of pnr_mlp AND of pnr_mlp_grads,
    and in mlp_tensors' order — lin_in, lin_out, per block fc_0 and fc_1, then lin_z."""
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.model import ResnetFC
    from pixel_nerf_multiscale_amd.model import models as M
    mlp = ResnetFC(42, n_blocks=3, d_latent=d_latent, d_hidden=32, combine_layer=2)
    n_z = 2 if d_latent else 0
    assert M.n_lin_z(mlp) == n_z
    slots = M.mlp_slots(mlp.n_blocks, n_z)
    ts = M.mlp_tensors(mlp)
    want = [mlp.lin_in.weight, mlp.lin_in.bias, mlp.lin_out.weight, mlp.lin_out.bias]
    for blk in mlp.blocks:
        want += [blk.fc_0.weight, blk.fc_0.bias, blk.fc_1.weight, blk.fc_1.bias]
    for b in range(n_z):
        want += [mlp.lin_z[b].weight, mlp.lin_z[b].bias]
    assert len(slots) == len(ts) == len(want) == 4 + 4 * 3 + 2 * n_z and all(a is b for a, b in zip(ts, want))
    for struct_t in (N.pnr_mlp, N.pnr_mlp_grads):
        fields = dict(struct_t._fields_)
        for field, b, _, _ in slots:
            assert field in fields and (b is None) == (fields[field] is ctypes.c_void_p), (struct_t.__name__, field, b)
        st = M.fill_mlp_slots(struct_t(), mlp.n_blocks, n_z, range(1, len(ts) + 1))
        assert [getattr(st, f) if b is None else getattr(st, f)[b] for f, b, _, _ in slots] == list(range(1, len(ts) + 1))
        assert (st.lin_in_w, st.lin_out_b, st.fc0_w[0], st.fc1_b[2]) == (1, 4, 5, 16)
        assert (st.lin_z_w[0], st.lin_z_b[1]) == ((17, 20) if d_latent else (None, None))
        with pytest.raises(ValueError):
            M.fill_mlp_slots(struct_t(), mlp.n_blocks, n_z, range(len(ts) - 1))       # one address short: an error, not a shift


def test_keyed_scope_restores_what_it_found():
    from pixel_nerf_multiscale_amd import NeRFRenderer
    r = NeRFRenderer()
    assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (None, 0, 0)
    with r.keyed(11, 5, 7):
        assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (11, 5, 7)
    assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (None, 0, 0)
    r.forced_seed, r.ray_index_base, r.ray_index_obj_stride = 3, 100, 400                       # prior values that are no defaults
    with r.keyed(12):                                                                           # a seed alone leaves the ray key
        assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (12, 100, 400)
        with r.keyed(None, 0, 0):
            assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (None, 0, 0)
        assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (12, 100, 400)
    assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (3, 100, 400)
    with pytest.raises(KeyError):
        with r.keyed(13, 1, 2):
            r.forced_seed = 99                                                                  # the body may set them too
            raise KeyError("from the body")
    assert (r.forced_seed, r.ray_index_base, r.ray_index_obj_stride) == (3, 100, 400)


def test_apply_sched_leaves_the_counts_of_the_stage():
    """_apply_sched on a renderer whose state says which stage it is in (a loaded checkpoint): the counts that sched_step
    leaves in test_renderer_surface_and_schedule."""
    from pixel_nerf_multiscale_amd import NeRFRenderer
    conf = dict(n_coarse=64, n_fine=32, n_fine_depth=16, sched=[[2, 4], [16, 32], [8, 16]])
    for stage, want in ((0, (64, 32)), (1, (16, 8)), (2, (32, 16))):
        r = NeRFRenderer.from_conf(conf)
        r.last_sched.fill_(stage)
        r._apply_sched()
        assert (r.n_coarse, r.n_fine) == want
    d = NeRFRenderer(n_coarse=48)
    d._apply_sched()                                                                            # no schedule: nothing changes
    assert (d.n_coarse, d.n_fine) == (48, 0)


def test_dptr_takes_any_dtype_on_the_device_only():
    from pixel_nerf_multiscale_amd import _native as N
    assert N.dptr(None) is None and N.ptr(None) is None
    for dt in (torch.float32, torch.int64, torch.uint8, torch.float16):
        with pytest.raises(RuntimeError):
            N.dptr(torch.zeros(3, dtype=dt))          # CPU tensors never reach the library
    with pytest.raises(RuntimeError):
        N.dptr(N.scratch(8, "cpu"))
    assert N.scratch(0, "cpu").numel() == 16 and N.scratch(100, "cpu").numel() == 100 and N.scratch(1, "cpu").dtype == torch.uint8


# ----------------------------------------------------------------------------- the C host layer: layouts, checks, the work split
def _size_mlp(N, L, H=512, cl=3):
    return N.pnr_mlp(d_in=42, d_latent=L, d_hidden=H, d_out=4, n_blocks=5, combine_layer=cl)


def _size_views(N, L, SB=1, NS=1):
    vw = N.pnr_views(n_objs=SB, n_views=NS, n_levels=1)
    vw.lat_c[0], vw.lat_h[0], vw.lat_w[0] = L, 8, 8
    return vw


def _host_sizes():
    """(what, bytes) of every size function whose layout is carved by one function (csrc/pnr_common.h Bump), in a fixed order.
    The training maps are (L, 8, 8) with L = 100 (25 KiB: the latent gradient's LDS route on any device, and without one) and
    L = 512 (128 KiB: the fixed-point route on any device)."""
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    lib, r = N.lib, C.byref
    for prec in (N.PNR_F32, N.PNR_F16):
        prm = N.pnr_params(n_coarse=64, n_fine=32, precision=prec)
        for NS in (1, 3):
            vw = _size_views(N, 512, 1, NS)
            for L in (512, 1024):                       # the coarse MLP, and a fine MLP of larger d_latent
                for n in (0, 1, 4096):
                    yield ("workspace", prec, NS, L, n), lib.pnr_workspace_bytes(r(prm), r(_size_mlp(N, L)), r(vw), n)
    for L in (100, 512):
        for SB in (1, 2):
            for NS in (1, 3):
                mlp, vw = _size_mlp(N, L), _size_views(N, L, SB, NS)
                for P in (0, 1, 4096):
                    yield ("train_bwd", L, SB, NS, P), lib.pnr_train_bwd_workspace_bytes(r(mlp), r(vw), P)
                    for wp, wc in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        yield ("train_bwd_cam", L, SB, NS, P, wp, wc), lib.pnr_train_bwd_cam_workspace_bytes(r(mlp), r(vw), P, wp, wc)
    for L, H in ((0, 64), (512, 512), (100, 120)):
        for NS in (1, 2):
            yield ("resnetfc", L, H, NS), lib.pnr_resnetfc_workspace_bytes(r(_size_mlp(N, L, H)), NS)
    for g in ((1, 1, 1), (16, 16, 16), (17, 16, 15)):
        yield ("mc",) + g, lib.pnr_mc_workspace_bytes(*g)
    for W, H in ((16, 16), (17, 16), (1, 1)):
        yield ("cmap", W, H), lib.pnr_cmap_workspace_bytes(W, H)
        for n_pass in (1, 2):
            yield ("vis_panel", W, H, n_pass), lib.pnr_vis_panel_workspace_bytes(W, H, n_pass)
    for n in (0, 1, 3, 4):
        yield ("optim", n), lib.pnr_optim_workspace_bytes(n)
    for W, H in ((7, 7), (16, 17)):
        yield ("eval_frame", W, H), lib.pnr_eval_frame_workspace_bytes(W, H)
        for F in (1, 3):
            yield ("eval_frames", F, W, H), lib.pnr_eval_frames_workspace_bytes(F, W, H)
            yield ("eval_frames_u8", F, W, H), lib.pnr_eval_frames_u8_workspace_bytes(F, W, H)


# _host_sizes() in its order, recorded from the library before the layouts moved onto one allocator
_HOST_SIZES = (
    311558912, 311562496, 322241280, 412222208, 412225792, 422904576, 933102336, 933105920, 943784704, 1235092224,
    1235095808, 1245774592, 67109376, 67112960, 77791744, 134218240, 134221824, 144900608, 335544832, 335548416,
    346227200, 402653696, 402657280, 413336064, 67240192, 67240192, 67240448, 67240448, 67240448, 67272960, 67272960,
    67273728, 67273472, 67273984, 95240448, 95240448, 95503360, 95339008, 95601664, 67240192, 67240192, 67240448,
    67240448, 67240448, 67337472, 67337472, 67338496, 67337984, 67338752, 151109888, 151109888, 151898112, 151208448,
    151996416, 67240192, 67240192, 67240448, 67240448, 67240448, 67247360, 67247360, 67247872, 67247872, 67248128,
    95240448, 95240448, 95503360, 95339008, 95601664, 67240192, 67240192, 67240448, 67240448, 67240448, 67260672,
    67260672, 67261184, 67261184, 67261440, 151109888, 151109888, 151898112, 151208448, 151996416, 67502592, 67502592,
    67502848, 67502848, 67502848, 67511296, 67511296, 67512064, 67511808, 67512320, 101843456, 101843456, 102106368,
    101942016, 102204672, 68026880, 68026880, 68027136, 68027136, 68027136, 68052480, 68052480, 68053504, 68052992,
    68053760, 170918400, 170918400, 171706624, 171016960, 171804928, 67764736, 67764736, 67764992, 67764992, 67764992,
    67773440, 67773440, 67773952, 67773952, 67774208, 102105600, 102105600, 102368512, 102204160, 102466816, 68813312,
    68813312, 68813568, 68813568, 68813568, 68838912, 68838912, 68839424, 68839424, 68839680, 171704832, 171704832,
    172493056, 171803392, 172591360, 33423616, 66846976, 310247680, 620495104, 75104512, 150208768, 0, 49152, 49152, 72,
    1120, 2168, 80, 1216, 2352, 72, 100, 128, 0, 32, 48, 48, 16, 16, 16, 48, 48, 32, 32, 32, 96, 96,
)


def test_workspace_sizes_are_pinned():
    got = list(_host_sizes())
    assert len(got) == len(_HOST_SIZES)
    wrong = [(what, v, want) for (what, v), want in zip(got, _HOST_SIZES) if v != want]
    assert not wrong, wrong[:8]


def _mlp_check_codes():
    """Return codes of the entry points that check an MLP's pointers, for an MLP with fc1_b[2] NULL, one with lin_z_w[0] NULL, one
    with lin_z_w[0] NULL and d_out = 3, one with lin_in_w NULL and d_out = 3 — and the whole one, which every call here stops
    behind its MLP checks by another argument (a misaligned output, no rows, a blob of no bytes), so that nothing is launched."""
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    lib, r, p = N.lib, C.byref, 0x10000

    def model(broken):
        prm = N.pnr_params(num_freqs=6, freq_factor=1.5, precision=N.PNR_F32)
        m = _size_mlp(N, 256)
        m.lin_in_w = m.lin_in_b = m.lin_out_w = m.lin_out_b = p
        for b in range(5):
            for f in ("fc0_w", "fc0_b", "fc1_w", "fc1_b", "lin_z_w", "lin_z_b"):
                getattr(m, f)[b] = p
        v = _size_views(N, 256)
        v.n_focal = v.n_c = 1
        v.w2c = v.focal = v.c = v.latent[0] = p
        if broken == "fc1_b[2]":
            m.fc1_b[2] = None
        if broken in ("lin_z_w[0]", "lin_z_w[0] + d_out"):
            m.lin_z_w[0] = None
        if broken == "lin_in_w + d_out":
            m.lin_in_w = None
        if broken.endswith("d_out"):
            m.d_out = 3
        return prm, m, v

    for broken in ("fc1_b[2]", "lin_z_w[0]", "lin_z_w[0] + d_out", "lin_in_w + d_out", "whole"):
        prm, m, v = model(broken)
        whole = broken == "whole"
        g = N.pnr_mlp_grads()
        pts = (None, None, 0, p, p, 8, 8)                    # explicit points
        yield (broken, "pnr_point_mlp"), lib.pnr_point_mlp(r(prm), r(m), r(v), *pts, p + 4, p, 1 << 40, None)
        yield (broken, "pnr_resnetfc_forward"), lib.pnr_resnetfc_forward(r(m), p, 0, 1, 8, p, p, 1 << 40, None)
        yield (broken, "pnr_pack_mlp"), lib.pnr_pack_mlp(r(m), N.PNR_BF16, p, 0 if whole else 1 << 40, None)
        yield (broken, "pnr_pack_mlp_projected"), lib.pnr_pack_mlp_projected(r(m), r(v), N.PNR_BF16, p, 0 if whole else 1 << 40, None)
        yield (broken, "pnr_point_mlp_train_fwd"), lib.pnr_point_mlp_train_fwd(r(prm), r(m), r(v), *pts, p + 4, p, 1 << 40, None)
        bwd = (r(prm), r(m), r(v), *pts, p + 4, p, p, 1 << 40, r(g), None, None, None)
        yield (broken, "pnr_point_mlp_bwd"), lib.pnr_point_mlp_bwd(*bwd, p, 1 << 40, None)
        yield (broken, "pnr_point_mlp_bwd_cam"), lib.pnr_point_mlp_bwd_cam(*bwd, None, None, None, p, 1 << 40, None)


# _mlp_check_codes() in its order, recorded from the library before the four checks became one
_MLP_CHECK_CODES = (
    -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -2, -1, -3, -3, -2, -2, -2, -1, -1, -3, -3, -1, -1, -1, -5,
    0, -4, -4, -5, -5, -5,
)


def test_mlp_pointer_checks_keep_their_codes_and_order():
    got = list(_mlp_check_codes())
    assert len(got) == len(_MLP_CHECK_CODES) == 35
    wrong = [(what, v, want) for (what, v), want in zip(got, _MLP_CHECK_CODES) if v != want]
    assert not wrong, wrong


_TILE_PTS, _MAX_GRID, _E_SHAPE, _E_UNSUPPORTED = 128, 512, -2, -3


def _split_reference(grid, n_objs, proj, fused, K, n_points, pts_per_obj):
    """The four branches of the fused launch's work split as point_mfma() spelled them out before point_split: returns
    (grid, tiles_per_wg, rays_per_wg, wgs_per_obj) or an error code."""
    cdiv = lambda a, b: (a + b - 1) // b
    tiles_per_wg = rays_per_wg = wgs_per_obj = 0
    n_rays = n_points // K if fused else 0
    if proj and n_objs > 1:
        wpo = max(grid // n_objs, 1)
        if wpo * n_objs > _MAX_GRID:
            return _E_UNSUPPORTED
        if fused:
            rays_per_obj = pts_per_obj // K
            rpw = max(cdiv(rays_per_obj, wpo), cdiv(_TILE_PTS, K))
            if rpw * K >= 0x7fffffff:
                return _E_SHAPE
            rays_per_wg = rpw
            wpo = cdiv(rays_per_obj, rpw)
        else:
            tiles_obj = cdiv(pts_per_obj, _TILE_PTS)
            tpw = cdiv(tiles_obj, wpo)
            if tpw * _TILE_PTS >= 0x7fffffff:
                return _E_SHAPE
            tiles_per_wg = tpw
            wpo = cdiv(tiles_obj, tpw)
        wgs_per_obj = wpo
        grid = wpo * n_objs
    elif fused:
        rpw = max(cdiv(n_rays, grid), cdiv(_TILE_PTS, K))
        if rpw * K >= 0x7fffffff:
            return _E_SHAPE
        rays_per_wg = rpw
        grid = cdiv(n_rays, rpw)
    else:
        n_tiles = cdiv(n_points, _TILE_PTS)
        tpw = cdiv(n_tiles, grid)
        if tpw * _TILE_PTS >= 0x7fffffff:
            return _E_SHAPE
        tiles_per_wg = tpw
        grid = cdiv(n_tiles, tpw)
    return (grid, tiles_per_wg, rays_per_wg, wgs_per_obj)


def test_point_split_is_the_four_branches_it_replaced():
    """pnr_debug_point_split (csrc/point_mfma.hip point_split) against the branches restated above: every cap, plain launches
    round the tile size and the int32 limit, fused launches round the ray counts at which a workgroup's share changes, and the
    same per object for 2, 3 and 16 objects with projected streams."""
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    out = (C.c_int32 * 4)()

    def split(cap, objs, K, count, per_obj):
        rc = N.lib.pnr_debug_point_split(cap, objs, K, count, per_obj, out)
        return tuple(out) if rc == 0 else rc

    n_checked = n_refused = 0
    for cap in (1, 8, 256, 512):
        for objs in (1, 2, 3, 16):
            proj = objs > 1
            for n in (1, 127, 128, 129, 65536, 65537, 1 << 33):                 # points (per object); 2^33: past int32 on one workgroup
                want = _split_reference(cap, objs, proj, False, 0, n * objs, n)
                assert split(cap, objs, 0, n * objs, n) == want, (cap, objs, n, want)
                n_refused += want == _E_SHAPE
                n_checked += 1
            for K in (1, 16, 96, 128, 129):
                for rays in (1, 511, 512, 513, 16384):                         # rays (per object)
                    want = _split_reference(cap, objs, proj, True, K, rays * objs * K, rays * K)
                    assert split(cap, objs, K, rays * objs, rays) == want, (cap, objs, K, rays, want)
                    n_checked += 1
    assert n_checked == 4 * 4 * (7 + 25) and n_refused > 0
    # without projected streams several objects share the workgroups: the object count does not enter
    assert split(256, 1, 96, 16384, 4096) == _split_reference(256, 4, False, True, 96, 16384 * 96, 4096 * 96)
    assert split(256, 4, 96, 16384, 4096) == _split_reference(256, 4, True, True, 96, 16384 * 96, 4096 * 96) != split(256, 1, 96, 16384, 4096)
    assert N.lib.pnr_debug_point_split(256, 1, 0, 4096, 4096, None) == -1
    assert N.lib.pnr_debug_point_split(0, 1, 0, 4096, 4096, out) == -2 and N.lib.pnr_debug_point_split(256, 1, 0, 0, 0, out) == -2
