"""The Python layer that prepares a native call, on the device: the MLP descriptors of the inference path and of the training
Functions come from one field table (models.MLP_FIELD_TABLE), so they name the same storage slot for slot."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_inference_and_training_descriptors_share_every_slot():
    from hip_util import setup
    from pixel_nerf_multiscale_amd.model import models as M
    from pixel_nerf_multiscale_amd.render import autograd as ag
    fx, spec, net, rend = setup("tiny_ns2_codeview")
    read = lambda st, slots: [getattr(st, f) if b is None else getattr(st, f)[b] for f, b, _, _ in slots]
    for mlp in (net.mlp_coarse, net.mlp_fine):
        if mlp is None:
            continue
        ts = M.mlp_tensors(mlp)
        slots = M.mlp_slots(mlp.n_blocks, M.n_lin_z(mlp))
        hdr = ag._header(net, mlp, True)
        assert hdr["n_params"] == len(ts) == len(slots)
        m_inf, keep_inf = net.mlp_struct(mlp, "fp32")
        m_trn, keep_trn = ag._mlp_struct_from(hdr, ts)
        want = [t.data_ptr() for t in ts]                      # float32 contiguous parameters: the structs point at them
        assert len(set(want)) == len(want) and 0 not in want
        assert read(m_inf, slots) == read(m_trn, slots) == want
        assert [t.data_ptr() for t in keep_inf] == [t.data_ptr() for t in keep_trn] == want
        for name in ("d_in", "d_latent", "d_hidden", "d_out", "n_blocks", "combine_layer", "combine_type"):
            assert getattr(m_inf, name) == getattr(m_trn, name), name
        # gradients: slot i holds g_i, an absent gradient is NULL
        grads = [torch.zeros_like(t) if i % 5 else None for i, t in enumerate(ts)]
        g = ag._grads_struct_from(hdr, grads)
        assert read(g, slots) == [None if t is None else t.data_ptr() for t in grads]


# ----------------------------------------------------------------------------- every workspace layout stays inside its size
GUARD = 4096


class _Guards:
    """Workspaces of exactly the asked size, cut out of a larger buffer of 0xA5 with GUARD bytes in front and behind."""

    def __init__(self):
        self.held = []

    def alloc(self, nbytes, dev):
        n = int(nbytes)
        big = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ws = big[GUARD:GUARD + n]
        assert ws.data_ptr() % 256 == 0
        self.held.append((big, n))
        return ws

    def check(self):
        torch.cuda.synchronize()
        assert self.held, "the run asked for no workspace"
        pattern = torch.full((GUARD,), 0xA5, dtype=torch.uint8, device=self.held[0][0].device)
        for i, (big, n) in enumerate(self.held):
            assert torch.equal(big[:GUARD], pattern), f"bytes in front of workspace {i} ({n} bytes) were written"
            assert torch.equal(big[GUARD + n:], pattern), f"bytes behind workspace {i} ({n} bytes) were written"


def _run_render(name, precision):
    def run(guards):
        from hip_util import setup
        fx, spec, net, rend = setup(name, precision=precision)
        out = rend(net, torch.from_numpy(fx["rays"]).cuda(), want_weights=True)
        return [out.coarse.rgb, out.coarse.depth, out.coarse.weights, out.fine.rgb, out.fine.depth, out.fine.weights]
    return run


def _run_train_step(guards):
    import golden_util as gu
    from hip_util import setup
    fx, spec, net, rend = setup("tiny_sb2_ns2")
    net.train()
    maps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gu.make_latents(spec)]
    net.encoder.set_latents(maps)
    out = rend(net, torch.from_numpy(fx["rays"]).cuda(), want_weights=True)
    G = {k: torch.from_numpy(v).cuda() for k, v in gu.make_loss_weights(spec).items()}
    loss = sum((out[t].rgb * G[f"{t}_rgb"]).sum() + (out[t].depth * G[f"{t}_depth"]).sum()
               + (out[t].weights * G[f"{t}_weights"]).sum() for t in ("coarse", "fine"))
    loss.backward()
    params = [p for m in (net.mlp_coarse, net.mlp_fine) if m is not None for p in m.parameters()]
    return [out.fine.rgb.detach()] + [p.grad for p in params] + [m.grad for m in maps]


def _run_resnetfc(guards):
    """pnr_resnetfc_forward itself, on two views and one point more than a chunk: the partial second chunk gathers the views' rows
    into the workspace (the modules call it with whole batches only)."""
    import ctypes as C
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.model import ResnetFC
    torch.manual_seed(3)
    mlp = ResnetFC(10, d_out=4, n_blocks=2, d_latent=6, d_hidden=32, combine_layer=1).cuda().eval()
    NS, B = 2, 49152 + 1
    zx = torch.randn(1, NS, B, 16, generator=torch.Generator().manual_seed(4)).cuda()
    m, keep = mlp.native_struct()
    nbytes = int(N.lib.pnr_resnetfc_workspace_bytes(C.byref(m), NS))
    ws = guards.alloc(nbytes, zx.device) if guards else torch.empty(nbytes, dtype=torch.uint8, device=zx.device)
    out = torch.empty(B, 4, device=zx.device)
    N.check(N.lib.pnr_resnetfc_forward(C.byref(m), N.ptr(zx), 1, NS, B, N.ptr(out), ws.data_ptr(), nbytes,
                                       N.current_stream(zx.device)), "pnr_resnetfc_forward")
    return [out]


def _run_mesh(guards):
    from pixel_nerf_multiscale_amd import recon
    g = torch.linspace(-1, 1, 9)
    x, y, z = torch.meshgrid(g, g, g, indexing="ij")
    field = (0.8 - torch.sqrt(x * x + y * y + z * z)).cuda()          # a sphere of radius 0.8 on a 9 x 9 x 9 grid
    v, t = recon.extract_mesh(field, 0.0)
    assert v.shape[0] > 0 and t.shape[0] > 0
    return [v, t]


def _run_adam(guards):
    from pixel_nerf_multiscale_amd import _native as N
    from pixel_nerf_multiscale_amd.optim import DeviceAdam
    gen = torch.Generator().manual_seed(6)
    chunk = int(N.lib.pnr_optim_chunk_elems())
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen).cuda()) for n in (2 * chunk + 5, 37)]       # four chunks
    opt = DeviceAdam(ps, lr=1e-2, max_norm=1.0)
    nbytes = max(int(N.lib.pnr_optim_workspace_bytes(opt._max_chunks)), 16)
    assert opt._workspace.numel() == nbytes and opt._max_chunks == 4
    if guards:
        opt._workspace = guards.alloc(nbytes, ps[0].device)
    for p in ps:
        p.grad.copy_(torch.randn(p.shape, generator=gen).cuda())
    opt.step()
    return [p.detach() for p in ps] + [opt.grad_norm, opt.moments(0)[0], opt.moments(0)[1]]


def _run_frames(guards):
    from pixel_nerf_multiscale_amd import util
    W, H, F = 17, 16, 3
    gen = torch.Generator().manual_seed(7)
    rgb = (torch.rand(F, H, W, 3, generator=gen) * 1.4 - 0.2).cuda()
    gt = (torch.rand(F, 3, H, W, generator=gen) * 2 - 1).cuda()
    depth = (torch.rand(H, W, generator=gen) + 1.0).cuda()
    u8, cmp, dn, met = util.eval_frame(rgb[0], depth, gt[0], z_near=1.0, z_far=2.0, want_compare=True, want_depth=True)
    cm, minmax = util.cmap_device(depth)
    return [u8, cmp, dn, met, util.eval_frames(rgb, gt, clamp=True), cm, minmax]


def _run_panel(guards):
    from pixel_nerf_multiscale_amd import util
    from test_gpu_vis import _device_passes, _panel_inputs
    images, src, gt, passes = _panel_inputs(17, 16, 3, 2, 2, seed=8)
    dev_passes, keep = _device_passes(passes, False)
    res = util.vis_panel(torch.from_numpy(images).cuda(), src, gt, dev_passes, want_f32=True, want_u8=True, want_alpha=True)
    return [res.panel, res.panel_u8, res.alpha, res.stats, res.mse]


_GUARDED_RUNS = {
    "render tiny_ns1 fp32": _run_render("tiny_ns1", "fp32"),
    "render full_ns1 fused": _run_render("full_ns1", "fp16"),
    "render full_ns3 fused": _run_render("full_ns3", "fp16"),
    "train step tiny_sb2_ns2": _run_train_step,
    "pnr_resnetfc_forward": _run_resnetfc,
    "extract_mesh 9^3 sphere": _run_mesh,
    "DeviceAdam.step": _run_adam,
    "eval_frame eval_frames cmap_device 17x16": _run_frames,
    "vis_panel 17x16 two passes": _run_panel,
}


@pytest.mark.parametrize("what", list(_GUARDED_RUNS))
def test_workspace_stays_inside_its_size(what, monkeypatch):
    """The ordinary Python paths with every workspace handed out at exactly the size asked for, between two guards of 4096 bytes
    of 0xA5 (N.scratch, PixelNeRFNet.workspace, and for the two calls that allocate their own, that buffer): both guards keep
    their pattern, and every result has the bits of the same run on ordinary buffers — the workspace itself starts as 0xA5
    too, so nothing in it is read before it is written."""
    from pixel_nerf_multiscale_amd import PixelNeRFNet, _native as N
    run = _GUARDED_RUNS[what]
    plain = [t.clone() for t in run(None)]
    guards = _Guards()
    monkeypatch.setattr(N, "scratch", lambda nbytes, dev: guards.alloc(max(int(nbytes), 16), dev))
    monkeypatch.setattr(PixelNeRFNet, "workspace", lambda self, nbytes, device: guards.alloc(nbytes, device))
    got = run(guards)
    guards.check()
    assert len(plain) == len(got)
    for i, (a, b) in enumerate(zip(plain, got)):
        assert a.dtype == b.dtype and a.shape == b.shape, i
        assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), f"{what}: output {i} differs"
