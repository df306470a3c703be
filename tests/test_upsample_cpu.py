"""Upstream pixelNeRF's latent map (latent_mode = "upstream"), host side: the two entry points' declarations and every
argument check (all made before any launch, so they run without a GPU), the numpy restatement of the specification
(tests/upsample_util.py) against torch's own fp64 F.interpolate + cat and its autograd, and the encoder's level computation,
sizes, refusals and checkpoint keys."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import upsample_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_UNSUPPORTED, E_ALIGN = -1, -2, -3, -5
EPS = 2.0 ** -24


def test_prototypes_are_declared_bound_and_exported():
    from pixel_nerf_multiscale_amd import _native as N, util
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("pnr_upsample_concat", "pnr_upsample_concat_bwd"):
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name
    assert "upsample.hip" in __import__("pixel_nerf_multiscale_amd.build_native", fromlist=["SOURCES"]).SOURCES
    assert N.lib.pnr_version() == 102
    assert hasattr(util, "upsample_concat")


def _i32(vals):
    return None if vals is None else (C.c_int32 * len(vals))(*vals)


def _ptrs(vals):
    return None if vals is None else (C.c_void_p * len(vals))(*vals)


def test_entry_points_check_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p = 64                        # a non-NULL, 16-byte aligned value: the checks return before anything dereferences it

    def fwd(levels=(p, p), c=(8, 8), h=(6, 3), w=(9, 5), n_levels=2, n_maps=2, out=p, out16=None, dt=N.PNR_BF16):
        return L.pnr_upsample_concat(_ptrs(levels), _i32(c), _i32(h), _i32(w), n_levels, n_maps, out, out16, dt, None)

    def bwd(d_out=p, c=(8, 8), h=(6, 3), w=(9, 5), n_levels=2, n_maps=2, levels=(p, None)):
        return L.pnr_upsample_concat_bwd(d_out, _i32(c), _i32(h), _i32(w), n_levels, n_maps, _ptrs(levels), None)

    for fn in (fwd, bwd):
        assert fn(levels=None) == E_NULL
        assert fn(c=None) == E_NULL and fn(h=None) == E_NULL and fn(w=None) == E_NULL
        assert fn(n_levels=0) == E_SHAPE and fn(n_levels=-1) == E_SHAPE
        six = dict(levels=(p,) * 6, c=(8,) * 6, h=(4,) * 6, w=(4,) * 6, n_levels=N.PNR_MAX_LEVELS + 1)
        assert fn(**six) == E_SHAPE
        assert fn(c=(8, 0)) == E_SHAPE and fn(h=(0, 3)) == E_SHAPE and fn(w=(9, -5)) == E_SHAPE
        assert fn(h=(32769, 3)) == E_SHAPE and fn(w=(9, 32769)) == E_SHAPE
        assert fn(n_maps=-1) == E_SHAPE
        assert fn(c=(8, 8), h=(32768, 4), w=(32768, 4), n_maps=1) == E_SHAPE          # level 0: 2^33 elements
        assert fn(c=(1, 1), h=(32768, 32768), w=(32768, 32768), n_maps=1) == E_SHAPE  # every level 2^30, the output 2^31
        assert fn(c=(1, 2), h=(4, 32768), w=(4, 32768), n_maps=1) == E_SHAPE          # a level 2^31, the output small
        assert fn(n_maps=0) == 0                                                      # nothing to write: no launch
    assert fwd(levels=(p, None)) == E_NULL
    assert fwd(out=None, out16=None) == E_NULL
    assert bwd(d_out=None) == E_NULL
    assert fwd(c=(8, 4), out16=p) == E_SHAPE and fwd(c=(7, 2), out=None, out16=p) == E_SHAPE      # sumC % 8 != 0
    assert fwd(c=(8, 4), n_maps=0) == 0                                               # without out16 any sumC passes the checks
    for dt in (N.PNR_F32, N.PNR_BF16X3, 7, -1):
        assert fwd(out16=p, dt=dt) == E_UNSUPPORTED
    assert fwd(out16=p + 8) == E_ALIGN and fwd(out=None, out16=p + 2, dt=N.PNR_F16) == E_ALIGN
    assert fwd(n_maps=0, out=None, out16=p, dt=N.PNR_F16) == 0
    with pytest.raises(ValueError):
        N.check(fwd(n_levels=0), "pnr_upsample_concat")


@pytest.fixture(scope="module", params=sorted(U.CPU_CASES))
def case(request):
    name = request.param
    levels = U.make_levels(name)
    ref, leaves = U.torch_reference(levels, torch.float64)
    return dict(name=name, levels=levels, shapes=[l.shape for l in levels], ref=ref, leaves=leaves,
                m64=U.model64(levels), m32=U.model32(levels))


def test_model64_equals_torch_fp64_interpolate_and_cat(case):
    ref = case["ref"].detach().numpy()
    err = np.abs(case["m64"] - ref).max() / ref.max()
    print(f"{case['name']}: model64 vs torch fp64 {err:.2e}")
    assert case["m64"].shape == ref.shape and err <= 1e-12


def test_model32_is_within_its_eight_roundings_of_model64(case):
    """At most 8 roundings lie on an output's path — lam and mu of each axis (4), a product and a sum in top / bot (2), a product
    and a sum in out (2) — each at most 2^-24 of a convex combination's operands, so of the map's maximum."""
    m32, m64 = case["m32"], case["m64"]
    assert m32.dtype == np.float32
    err = np.abs(m32.astype(np.float64) - m64).max() / m64.max()
    print(f"{case['name']}: model32 vs model64 {err / EPS:.2f} x 2^-24")
    assert err <= 8 * EPS


def test_an_identity_level_compares_equal(case):
    levels = case["levels"]
    c = 0
    for l in levels:
        if l.shape[2:] == levels[0].shape[2:]:
            assert np.array_equal(case["m32"][:, c:c + l.shape[1]].view(np.uint32), l.view(np.uint32))
            assert np.array_equal(case["m64"][:, c:c + l.shape[1]], l.astype(np.float64))
        c += l.shape[1]


def test_adjoint64_equals_torch_fp64_autograd_and_the_dot_product_identity(case):
    g = U.make_cotangent(case["name"])
    grads = torch.autograd.grad(case["ref"], case["leaves"], torch.from_numpy(g).double(), retain_graph=True)
    adj = U.adjoint64(g, case["shapes"])
    absadj = U.adjoint_abs64(g, case["shapes"])
    for a, b, s in zip(adj, grads, absadj):
        b = b.numpy()
        err = np.abs(a - b).max() / np.abs(b).max()
        print(f"{case['name']}: adjoint64 vs torch fp64 autograd {err:.2e}")
        assert a.shape == b.shape and err <= 1e-12
        assert (s >= np.abs(a) * (1 - 1e-12)).all()
    lhs = float((case["m64"] * g.astype(np.float64)).sum())                    # <U x, g>
    rhs = sum(float((l.astype(np.float64) * a).sum()) for l, a in zip(case["levels"], adj))      # <x, U^T g>
    scale = float((case["m64"] * np.abs(g)).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale


def test_the_backward_kernels_arithmetic_is_inside_its_bound(case):
    """fp32 tap weights (at most 5 roundings in w = fl(wy wx)), fp64 products and sums, one final rounding: within
    8 x 2^-24 of the fp64 adjoint, relative to the adjoint of |g| — the bound tests/test_gpu_upsample.py holds the kernel to."""
    g = U.make_cotangent(case["name"])
    for k, a, s in zip(U.adjoint32w(g, case["shapes"]), U.adjoint64(g, case["shapes"]), U.adjoint_abs64(g, case["shapes"])):
        k = k.astype(np.float32).astype(np.float64)
        worst = (np.abs(k - a) / np.maximum(s, 1e-300)).max()
        print(f"{case['name']}: fp32-weight adjoint vs adjoint64 {worst / EPS:.2f} x 2^-24")
        assert (np.abs(k - a) <= 8 * EPS * s).all()


# ---------------------------------------------------------------------------------------------------- encoder
def _encoder(**kw):
    from pixel_nerf_multiscale_amd.model import SpatialEncoder
    torch.manual_seed(0)
    return SpatialEncoder(backbone="resnet18", pretrained=False, **kw).eval()


def test_level_features_sizes_and_level_zero_before_the_pool():
    enc = _encoder(latent_mode="upstream", use_first_pool=False)
    with torch.no_grad():
        feats = enc.level_features(torch.randn(2, 3, 64, 64))
    assert [tuple(f.shape[2:]) for f in feats] == [(32, 32), (32, 32), (16, 16), (8, 8)]
    enc = _encoder(latent_mode="upstream", use_first_pool=True)
    x = torch.randn(1, 3, 128, 128)
    with torch.no_grad():
        feats = enc.level_features(x)
        direct = torch.relu(enc.model.bn1(enc.model.conv1(x)))
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 64, 64), (64, 32, 32), (128, 16, 16), (256, 8, 8)]
    assert torch.equal(feats[0], direct)                         # taken BEFORE the max-pool
    with torch.no_grad():
        three = _encoder(latent_mode="upstream", num_layers=3).level_features(x)
    assert [tuple(f.shape[1:]) for f in three] == [(64, 64, 64), (64, 32, 32), (128, 16, 16)]


def test_upstream_mode_sizes_defaults_refusals_and_keys():
    from pixel_nerf_multiscale_amd.model import SpatialEncoder
    fork, up = _encoder(), _encoder(latent_mode="upstream")
    assert fork.latent_mode == "fork" and fork.latent_size == 256 and fork.uv_scale == "latent"
    assert up.latent_size == 512 and up.uv_scale == "image"
    assert _encoder(latent_mode="upstream", num_layers=3).latent_size == 256
    with pytest.raises(ValueError):
        _encoder(latent_mode="upstream", use_multi_scale=True)
    with pytest.raises(ValueError):
        _encoder(latent_mode="both")
    assert list(fork.state_dict().keys()) == list(up.state_dict().keys())
    enc = SpatialEncoder.from_conf(dict(backbone="resnet18", pretrained=False, latent_mode="upstream", num_layers=4))
    assert enc.latent_mode == "upstream" and enc.latent_size == 512
    assert SpatialEncoder.from_conf(dict(backbone="resnet18", pretrained=False)).latent_mode == "fork"
    with pytest.raises(RuntimeError):
        up(torch.randn(1, 3, 32, 32))                           # the map is built on the HIP device only: no CPU fall-back


def _net(latent_mode):
    from pixel_nerf_multiscale_amd import PixelNeRFNet
    mlp = dict(type="resnet", n_blocks=2, d_hidden=32, combine_layer=1, combine_type="average")
    conf = dict(use_encoder=True, use_global_encoder=False, use_xyz=True, normalize_z=True, use_code=True,
                code=dict(num_freqs=6, freq_factor=1.5, include_input=True), use_viewdirs=True, use_code_viewdirs=False,
                mlp_coarse=dict(mlp), mlp_fine=dict(mlp),
                encoder=dict(backbone="resnet18", pretrained=False, num_layers=4, latent_mode=latent_mode), precision="fp32")
    return PixelNeRFNet(conf)


def test_a_checkpoint_with_upstream_keys_only_loads(tmp_path):
    """Upstream's SpatialEncoder has `model` alone; `layers` here aliases the same modules.  A state-dict without the
    encoder.layers.* keys loads through evalio.load_checkpoint and load_weights, and the aliases see the values."""
    from types import SimpleNamespace
    from pixel_nerf_multiscale_amd import evalio
    torch.manual_seed(1)
    src = _net("upstream")
    assert src.d_latent == 512 and tuple(src.mlp_coarse.lin_z[0].weight.shape) == (32, 512)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(torch.randn_like(p) * 0.01)
    sd = {k: v.clone() for k, v in src.state_dict().items() if not k.startswith("encoder.layers.")}
    assert any(k.startswith("encoder.model.") for k in sd) and len(sd) < len(src.state_dict())
    path = tmp_path / "ckpt" / "run"
    path.mkdir(parents=True)
    torch.save(sd, str(path / "pixel_nerf_latest"))

    def verify(net, missing=None):
        if missing is not None:
            assert missing and all(k.startswith("encoder.layers.") for k in missing)
        full = net.state_dict()
        for k, v in src.state_dict().items():
            assert torch.equal(full[k], v), k                    # encoder.layers.* included
        assert net.encoder.layers[0][0].weight is net.encoder.model.conv1.weight
        assert torch.equal(net.encoder.layers[1][0].conv1.weight, sd["encoder.model.layer1.0.conv1.weight"])
        assert torch.equal(net.encoder.layers[0][1].running_var, sd["encoder.model.bn1.running_var"])

    torch.manual_seed(2)
    net = _net("upstream")
    missing, unexpected = evalio.load_checkpoint(net, str(path / "pixel_nerf_latest"))
    assert unexpected == []
    verify(net, missing)
    torch.manual_seed(3)
    net = _net("upstream")
    net.load_weights(SimpleNamespace(resume=True, checkpoints_path=str(tmp_path / "ckpt"), name="run"), strict=False)
    verify(net)
    # the single-scale fork net has d_latent = 256: upstream's 512-wide lin_z does not fit it
    with pytest.raises(RuntimeError):
        _net("fork").load_state_dict(sd, strict=False)
