"""
Training path: the renderer under autograd, as train/train.py:324-346,382-410 uses the
reference (calc_losses -> renderer(net, rays, want_weights=True) -> loss.backward()).

torch.autograd.Functions, each a thin shell over a forward/backward pair of libpnr_hip.so entry
points (csrc/train_f32.hip) — no PyTorch arithmetic on the per-point data:

  PointMLP      pnr_point_mlp_train_fwd / pnr_point_mlp_bwd    PixelNeRFNet.forward (models.py.backup2:155-282)
  Composite     pnr_composite / pnr_composite_bwd              NeRFRenderer.composite (nerf.py:178-182,223-249)
  SampleFine    pnr_sample_fine / pnr_sample_fine_bwd          sample_fine* + cat + sort (nerf.py:120-161,285-295)
  RGBLoss       pnr_rgb_loss / pnr_rgb_loss_bwd                the trainer's rgb loss (train.py:338-346, loss.py:99-103)
  AlphaLoss     pnr_alpha_loss / pnr_alpha_loss_bwd            the opacity losses on the weights (loss.py:24-37, and a mask BCE)

Gradients reach the MLP weights, the encoder's latent maps (and through them the ResNet trunk, which stays
a PyTorch module) and — because nerf.py:287-289 does not detach the depth-guided samples — the coarse depth
through the fine pass's sample positions.  Arithmetic is fp32 (the reference trains in fp32);
`net.train_precision = "bf16"` runs the GEMM products on the bf16 MFMA with fp32 accumulation, a 16-bit tape (the block inputs
and fc_0 outputs kept as the bf16 values those GEMMs stage anyway: gradients bit-identical to an fp32 tape's, which
`net.train_tape = "fp32"` selects) and fp32
results (the counterpart of the reference's AMP switch, train/train.py:385-398).
"""
import ctypes as C

import torch

from .. import _native as N
from ..model.models import fill_mlp_slots, mlp_struct_from, mlp_tensors, n_lin_z, views_from


def _mlp_struct_from(hdr, tensors):
    """pnr_mlp of hdr's module over the ordered parameter list of models.mlp_tensors()."""
    return mlp_struct_from(hdr["mlp"], tensors)


def _grads_struct_from(hdr, grads):
    """pnr_mlp_grads over one gradient tensor (or None) per parameter, in the same order."""
    return fill_mlp_slots(N.pnr_mlp_grads(), hdr["n_blocks"], hdr["n_lin_z"], [N.dptr(t) for t in grads])


def _train_params(net):
    prm = net.params_struct(None, net.train_precision)
    prm.train_tape_fp32 = 1 if getattr(net, "train_tape", "auto") == "fp32" else 0
    return prm


class PointMLP(torch.autograd.Function):
    """out (n_points, 4) = PixelNeRFNet.forward at points named by rays+z (a, b = rays (N,8), z (N,K)) or
    explicitly (a, b = xyz (SB*P,3), viewdirs (SB*P,3)).  Differentiable in a and b, the stored cameras (poses, focal, c:
    pnr_point_mlp_bwd_cam, called only when one of them or the rays / view directions asks), the MLP parameters and the
    latent maps.  Columns 6:8 of d(rays) are exact zeros."""

    @staticmethod
    def forward(ctx, hdr, a, b, poses, focal, c, *tensors):
        n_par = hdr["n_params"]
        params, maps = tensors[:n_par], tensors[n_par:]
        dev = a.device
        a, b = N.f32c(a.detach()), N.f32c(b.detach())
        m, k1 = _mlp_struct_from(hdr, params)
        v, k2 = views_from(poses, focal, c, hdr["n_views"], maps, hdr["uv_scale"])
        rays_mode = hdr["rays_mode"]
        if rays_mode:
            n_rays, K = b.shape
            n_points = n_rays * K
        else:
            n_points, K = a.shape[0], 0
        if n_points % v.n_objs:
            raise ValueError("points do not divide evenly over the encoded objects")
        prm = hdr["prm"]
        tape = N.scratch(N.lib.pnr_train_tape_bytes_for(C.byref(prm), C.byref(m), C.byref(v), n_points), dev)
        out = torch.empty(n_points, 4, device=dev)
        args = (N.ptr(a), N.ptr(b), K, None, None) if rays_mode else (None, None, 0, N.ptr(a), N.ptr(b))
        N.check(N.lib.pnr_point_mlp_train_fwd(C.byref(prm), C.byref(m), C.byref(v), *args, n_points,
                                              n_points // v.n_objs, N.ptr(out), tape.data_ptr(), tape.numel(),
                                              N.current_stream(dev)), "pnr_point_mlp_train_fwd")
        ctx.hdr = hdr
        ctx.save_for_backward(a, b, poses, focal, c, out, tape, *params, *maps)
        return out

    @staticmethod
    def backward(ctx, d_out):
        hdr = ctx.hdr
        a, b, poses, focal, c, out, tape = ctx.saved_tensors[:7]
        rest = ctx.saved_tensors[7:]
        n_par = hdr["n_params"]
        params, maps = rest[:n_par], rest[n_par:]
        dev = a.device
        m, k1 = _mlp_struct_from(hdr, params)
        v, k2 = views_from(poses, focal, c, hdr["n_views"], maps, hdr["uv_scale"])
        need = ctx.needs_input_grad            # (hdr, a, b, poses, focal, c, *params, *maps)
        need_par, need_map = need[6:6 + n_par], need[6 + n_par:]
        # one zero fill for all parameter gradients (the kernels accumulate with atomics)
        flat = torch.zeros(sum(p.numel() for p, nd in zip(params, need_par) if nd), device=dev)
        g_par, off = [], 0
        for p, nd in zip(params, need_par):
            g_par.append(flat[off:off + p.numel()].view(p.shape) if nd else None)
            off += p.numel() if nd else 0
        g_map = [torch.zeros(mp.shape, device=dev) if nd else None for mp, nd in zip(maps, need_map)]
        rays_mode = hdr["rays_mode"]
        n_points = out.shape[0]
        d_pos = None
        if rays_mode and need[2]:
            d_pos = torch.empty_like(b)
        elif not rays_mode and need[1]:
            d_pos = torch.empty_like(a)
        g = _grads_struct_from(hdr, g_par)
        dl = (C.c_void_p * N.PNR_MAX_LEVELS)(*[N.dptr(t) for t in g_map])
        d_out = N.f32c(d_out)
        K = b.shape[1] if rays_mode else 0
        args = (N.ptr(a), N.ptr(b), K, None, None) if rays_mode else (None, None, 0, N.ptr(a), N.ptr(b))
        head = (C.byref(hdr["prm"]), C.byref(m), C.byref(v), *args, n_points, n_points // v.n_objs, N.ptr(out), N.ptr(d_out),
                tape.data_ptr(), tape.numel(), C.byref(g), dl,
                None if rays_mode else N.ptr(d_pos), N.ptr(d_pos) if rays_mode else None)
        # the camera outputs: the other member of (a, b) — the rays, or the view directions — and the stored cameras
        want_other = need[1] if rays_mode else need[2]
        want_cam = need[3] or need[4] or need[5]
        if not (want_other or want_cam):
            ws = N.scratch(N.lib.pnr_train_bwd_workspace_bytes(C.byref(m), C.byref(v), n_points), dev)
            N.check(N.lib.pnr_point_mlp_bwd(*head, ws.data_ptr(), ws.numel(), N.current_stream(dev)), "pnr_point_mlp_bwd")
            return (None, d_pos if not rays_mode else None, d_pos if rays_mode else None, None, None, None, *g_par, *g_map)
        d_other = torch.empty_like(a if rays_mode else b) if want_other else None
        d_cam = torch.empty(v.n_objs * v.n_views, 16, device=dev) if want_cam else None
        ws = N.scratch(N.lib.pnr_train_bwd_cam_workspace_bytes(C.byref(m), C.byref(v), n_points, int(bool(want_other)),
                                                               int(bool(want_cam))), dev)
        N.check(N.lib.pnr_point_mlp_bwd_cam(*head, None if rays_mode else N.ptr(d_other), N.ptr(d_other) if rays_mode else None,
                                            N.ptr(d_cam), ws.data_ptr(), ws.numel(), N.current_stream(dev)),
                "pnr_point_mlp_bwd_cam")
        g_a, g_b = (d_other, d_pos) if rays_mode else (d_pos, d_other)
        g_poses = g_focal = g_c = None
        if want_cam:
            nv = d_cam.shape[0]
            if need[3]:
                g_poses = torch.cat((d_cam[:, :9].reshape(nv, 3, 3), d_cam[:, 9:12].reshape(nv, 3, 1)), dim=2).reshape(poses.shape)
            g_focal = _rows_as_stored(d_cam[:, 12:14], focal, v.n_objs) if need[4] else None
            g_c = _rows_as_stored(d_cam[:, 14:16], c, v.n_objs) if need[5] else None
        return (None, g_a, g_b, g_poses, g_focal, g_c, *g_par, *g_map)


def _rows_as_stored(d_view, stored, n_objs):
    """Per-view intrinsics gradients (n_views_total, 2) summed into the rows the caller stored: one row for all views, one
    per object (views_from repeats those per view) or one per view.  torch sums on the device, in a fixed order."""
    nv, rows = d_view.shape[0], stored.shape[0]
    if rows == nv:
        return d_view.reshape(stored.shape)
    if rows == 1:
        return d_view.sum(0, keepdim=True).reshape(stored.shape)
    if rows == n_objs:
        return d_view.reshape(n_objs, nv // n_objs, 2).sum(1).reshape(stored.shape)
    raise ValueError(f"{rows} intrinsics rows for {nv} views of {n_objs} objects")


class Composite(torch.autograd.Function):
    """(weights, rgb, depth) = composite(rays, z, rgbsigma); differentiable in rgbsigma and z."""

    @staticmethod
    def forward(ctx, rays, z, rgbs, white_bkgd):
        rays, z, rgbs = N.f32c(rays.detach()), N.f32c(z.detach()), N.f32c(rgbs.detach())
        B, K = z.shape
        dev = rays.device
        weights, rgb, depth = torch.empty(B, K, device=dev), torch.empty(B, 3, device=dev), torch.empty(B, device=dev)
        N.check(N.lib.pnr_composite(N.ptr(rays), N.ptr(z), N.ptr(rgbs), B, K, int(bool(white_bkgd)), N.ptr(weights),
                                    N.ptr(rgb), N.ptr(depth), N.current_stream(dev)), "pnr_composite")
        ctx.white = int(bool(white_bkgd))
        ctx.save_for_backward(rays, z, rgbs)
        return weights, rgb, depth

    @staticmethod
    def backward(ctx, d_w, d_rgb, d_depth):
        rays, z, rgbs = ctx.saved_tensors
        B, K = z.shape
        dev = rays.device
        keep = [None if t is None else N.f32c(t) for t in (d_w, d_rgb, d_depth)]
        d_rgbs = torch.empty_like(rgbs)
        d_z = torch.empty_like(z) if ctx.needs_input_grad[1] else None
        N.check(N.lib.pnr_composite_bwd(N.ptr(rays), N.ptr(z), N.ptr(rgbs), B, K, ctx.white,
                                        *[N.ptr(t) for t in keep], N.ptr(d_rgbs), N.ptr(d_z), N.current_stream(dev)),
                "pnr_composite_bwd")
        return None, d_z, d_rgbs, None


class SampleFine(torch.autograd.Function):
    """z_sorted (N, Kc+Kf) = sort(cat(z_coarse, importance samples, depth samples)); differentiable in depth."""

    @staticmethod
    def forward(ctx, rend, rays, z_coarse, weights, depth, seed, noise):
        dev = rays.device
        rays, zc = N.f32c(rays.detach()), N.f32c(z_coarse.detach())
        w, d = N.f32c(weights.detach()), N.f32c(depth.detach())
        B = rays.shape[0]
        z = torch.empty(B, rend.n_coarse + rend.n_fine, device=dev)
        u, r, g = (None if noise is None or noise.get(k) is None else N.f32c(noise[k], dev) for k in ("u", "r", "g"))
        cfg = (int(rend.n_coarse), int(rend.n_fine), int(rend.n_fine_depth), float(rend.depth_std), int(bool(rend.lindisp)),
               int(seed), int(rend.ray_index_base))
        N.check(N.lib.pnr_sample_fine(N.ptr(rays), N.ptr(zc), N.ptr(w), N.ptr(d), B, cfg[0], cfg[1], cfg[2], cfg[3], cfg[4],
                                      N.ptr(u), N.ptr(r), N.ptr(g), cfg[5], cfg[6], N.ptr(z), N.current_stream(dev)),
                "pnr_sample_fine")
        ctx.cfg = cfg
        ctx.g = g
        ctx.save_for_backward(rays, d, z)
        return z

    @staticmethod
    def backward(ctx, d_z):
        rays, d, z = ctx.saved_tensors
        Kc, Kf, Kfd, std, _, seed, base = ctx.cfg
        if Kfd == 0 or not ctx.needs_input_grad[4]:
            return (None,) * 7
        d_depth = torch.empty_like(d)
        d_z = N.f32c(d_z)
        N.check(N.lib.pnr_sample_fine_bwd(N.ptr(rays), N.ptr(d), rays.shape[0], Kc, Kf, Kfd, std,
                                          N.ptr(ctx.g), seed, base, N.ptr(z), N.ptr(d_z), N.ptr(d_depth),
                                          N.current_stream(rays.device)), "pnr_sample_fine_bwd")
        return None, None, None, None, d_depth, None, None


class RGBLoss(torch.autograd.Function):
    """(total, stats) = rgb loss of the coarse and (unless None) the fine colours against rgb_gt, all (..., 3):
    MSELoss / L1Loss(reduction="mean") combined as train/train.py:338-346 does.  total: 0-dim, differentiable in both
    colour tensors.  stats: the 3-float device buffer [lambda_c Lc, lambda_f Lf, total] (loss_dict rc / rf / t), not
    differentiable.  Nothing is read back: the incoming gradient is handed to the backward kernel as a device pointer."""

    @staticmethod
    def forward(ctx, coarse_rgb, fine_rgb, rgb_gt, use_l1, lambda_coarse, lambda_fine):
        dev = N.same_device(coarse_rgb, fine_rgb, rgb_gt)
        if coarse_rgb.shape != rgb_gt.shape or coarse_rgb.shape[-1] != 3 or (fine_rgb is not None and fine_rgb.shape != rgb_gt.shape):
            raise ValueError(f"rgb tensors must share one (..., 3) shape: coarse {tuple(coarse_rgb.shape)}, fine "
                             f"{None if fine_rgb is None else tuple(fine_rgb.shape)}, gt {tuple(rgb_gt.shape)}")
        c, g = N.f32c(coarse_rgb.detach()), N.f32c(rgb_gt.detach())
        f = None if fine_rgb is None else N.f32c(fine_rgb.detach())
        cfg = (c.numel() // 3, int(bool(use_l1)), float(lambda_coarse), float(lambda_fine))
        stats = torch.empty(3, device=dev)
        N.check(N.lib.pnr_rgb_loss(N.ptr(c), N.ptr(f), N.ptr(g), cfg[0], cfg[1], cfg[2], cfg[3], N.ptr(stats),
                                   N.current_stream(dev)), "pnr_rgb_loss")
        ctx.cfg = cfg
        ctx.has_fine = f is not None
        ctx.save_for_backward(c, g, *([f] if f is not None else []))
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)        # no zero tensor for the stats' absent gradient
        return stats[2], stats                  # total: a 0-dim view of the stats buffer, no copy

    @staticmethod
    def backward(ctx, d_total, _d_stats):
        if d_total is None:
            return (None,) * 6
        c, g = ctx.saved_tensors[:2]
        f = ctx.saved_tensors[2] if ctx.has_fine else None
        n, use_l1, lc, lf = ctx.cfg
        d_c = torch.empty_like(c) if ctx.needs_input_grad[0] else None
        d_f = torch.empty_like(f) if (f is not None and ctx.needs_input_grad[1]) else None
        d_total = N.f32c(d_total, c.device)
        N.check(N.lib.pnr_rgb_loss_bwd(N.ptr(c), N.ptr(f), N.ptr(g), n, use_l1, lc, lf, N.ptr(d_total), N.ptr(d_c), N.ptr(d_f),
                                       N.current_stream(c.device)), "pnr_rgb_loss_bwd")
        return d_c, d_f, None, None, None, None


class AlphaLoss(torch.autograd.Function):
    """(total, stats) = an opacity loss of the coarse and / or the fine pass's compositing weights (..., K) — either may be None,
    not both: mode N.PNR_ALPHA_NV2 / PNR_ALPHA_OPAQUE (the reference's AlphaLossNV2, loss.py:24-37) or PNR_ALPHA_MASK, a binary
    cross entropy of the weights' sum against mask (...), any values in [0, 1] (include/pnr.h writes the arithmetic down: fp64
    from the sum to the loss).  total: 0-dim, differentiable in the two weight tensors only.  stats: the 3-float device buffer
    [lambda_c Lc, lambda_f Lf, total], not differentiable.  The fp64 sums are kept for the backward; nothing is read back."""

    @staticmethod
    def forward(ctx, coarse_w, fine_w, mask, mode, lambda_coarse, lambda_fine, clamp_lo, clamp_hi, clamp_alpha):
        dev = N.same_device(coarse_w, fine_w, mask)
        first = coarse_w if coarse_w is not None else fine_w
        if first is None:
            raise ValueError("AlphaLoss needs the weights of at least one pass")
        if first.dim() < 1 or (coarse_w is not None and fine_w is not None and coarse_w.shape[:-1] != fine_w.shape[:-1]):
            raise ValueError("weights must share their ray axes (..., K): coarse "
                             f"{None if coarse_w is None else tuple(coarse_w.shape)}, fine {None if fine_w is None else tuple(fine_w.shape)}")
        n_rays = first.numel() // max(first.shape[-1], 1)
        if mask is not None and mask.numel() != n_rays:
            raise ValueError(f"mask must hold one value per ray ({n_rays}), got {tuple(mask.shape)}")
        c = None if coarse_w is None else N.f32c(coarse_w.detach())
        f = None if fine_w is None else N.f32c(fine_w.detach())
        m = None if mask is None else N.f32c(mask.detach())
        Kc, Kf = (0 if c is None else c.shape[-1]), (0 if f is None else f.shape[-1])
        cfg = (n_rays, Kc, Kf, int(mode), float(lambda_coarse), float(lambda_fine), float(clamp_lo), float(clamp_hi),
               float(clamp_alpha))
        alpha = torch.empty(2, n_rays, dtype=torch.float64, device=dev)
        stats = torch.empty(3, device=dev)
        N.check(N.lib.pnr_alpha_loss(N.ptr(c), Kc, N.ptr(f), Kf, N.ptr(m), n_rays, *cfg[3:], alpha.data_ptr(), N.ptr(stats),
                                     N.current_stream(dev)), "pnr_alpha_loss")
        ctx.cfg = cfg
        ctx.shapes = (None if c is None else c.shape, None if f is None else f.shape)
        ctx.has_mask = m is not None
        ctx.save_for_backward(alpha, *([m] if m is not None else []))
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)        # no zero tensor for the stats' absent gradient
        return stats[2], stats                  # total: a 0-dim view of the stats buffer, no copy

    @staticmethod
    def backward(ctx, d_total, _d_stats):
        if d_total is None:
            return (None,) * 9
        alpha = ctx.saved_tensors[0]
        m = ctx.saved_tensors[1] if ctx.has_mask else None
        n_rays, Kc, Kf = ctx.cfg[:3]
        dev = alpha.device
        d_c = torch.empty(ctx.shapes[0], device=dev) if (ctx.shapes[0] is not None and ctx.needs_input_grad[0]) else None
        d_f = torch.empty(ctx.shapes[1], device=dev) if (ctx.shapes[1] is not None and ctx.needs_input_grad[1]) else None
        if d_c is None and d_f is None:
            return (None,) * 9
        d_total = N.f32c(d_total, dev)
        N.check(N.lib.pnr_alpha_loss_bwd(alpha.data_ptr(), N.ptr(m), n_rays, Kc, Kf, *ctx.cfg[3:], N.ptr(d_total), N.ptr(d_c),
                                         N.ptr(d_f), N.current_stream(dev)), "pnr_alpha_loss_bwd")
        return (d_c, d_f) + (None,) * 7


# ---------------------------------------------------------------------------------------------------------------
def _header(net, mlp, rays_mode):
    return dict(mlp=mlp, n_blocks=mlp.n_blocks, n_lin_z=n_lin_z(mlp), n_params=len(mlp_tensors(mlp)),
                n_views=int(net.num_views_per_obj), rays_mode=rays_mode, prm=_train_params(net),
                uv_scale=net.uv_scales())


def point_mlp_rays(net, mlp, rays, z):
    """(N, K, 4) network outputs at the samples z (N,K) of rays (N,8), under autograd."""
    hdr = _header(net, mlp, True)
    out = PointMLP.apply(hdr, rays, z, net.poses, net.focal, net.c, *mlp_tensors(mlp), *net.latent_maps_for_grad())
    return out.reshape(z.shape[0], z.shape[1], 4)


def point_mlp_points(net, mlp, xyz, viewdirs):
    """(SB, P, 4) network outputs at explicit points, under autograd (PixelNeRFNet.forward in training)."""
    SB, P, _ = xyz.shape
    hdr = _header(net, mlp, False)
    out = PointMLP.apply(hdr, xyz.reshape(-1, 3), viewdirs.reshape(-1, 3), net.poses, net.focal, net.c,
                         *mlp_tensors(mlp), *net.latent_maps_for_grad())
    return out.reshape(SB, P, 4)


def render_train(rend, net, rays, want_weights):
    """NeRFRenderer.forward (nerf.py:251-303) with every stage differentiable where the reference's is."""
    from ..util import AttrDict
    SB, B, _ = rays.shape
    r = N.f32c(rays).reshape(-1, 8)
    if net.poses.shape[0] != SB * int(net.num_views_per_obj):
        raise ValueError(f"rays has {SB} objects but encode() saw {net.poses.shape[0] // int(net.num_views_per_obj)}")
    seed = rend._seed()
    noise = rend.fixed_noise

    def sigma_noise(out):        # nerf.py:225-226, training only
        if rend.training and rend.noise_std > 0.0:
            return torch.cat([out[..., :3], out[..., 3:] + torch.randn_like(out[..., 3:]) * rend.noise_std], dim=-1)
        return out

    z_c = rend.sample_coarse(r, seed)
    out_c = sigma_noise(point_mlp_rays(net, net.mlp_coarse, r, z_c))
    comp_c = Composite.apply(r, z_c, out_c, rend.white_bkgd)
    res = AttrDict(coarse=rend._format_outputs(comp_c, SB, want_weights))
    keep = getattr(rend, "keep_samples", False)          # the sample positions, as the fused path leaves them
    if keep:
        res.coarse.z = z_c.detach().reshape(SB, B, -1)
    if rend.using_fine:
        z_f = SampleFine.apply(rend, r, z_c, comp_c[0], comp_c[2], seed, noise)
        mlp_f = net.mlp_fine if net.mlp_fine is not None else net.mlp_coarse
        out_f = sigma_noise(point_mlp_rays(net, mlp_f, r, z_f))
        res.fine = rend._format_outputs(Composite.apply(r, z_f, out_f, rend.white_bkgd), SB, want_weights)
        if keep:
            res.fine.z = z_f.detach().reshape(SB, B, -1)
    return res
