"""
Cameras under autograd: what a differentiable pixelNeRF is used for besides training.  The renderer's training path gives
gradients at the rays and at the stored source cameras (render.autograd.PointMLP, pnr_point_mlp_bwd_cam); here are the torch
pieces in front of it — an se(3) chart, the rays of selected pixels as a differentiable function of the camera, and a small
photometric pose refinement (iNeRF-style) on top of both.  Everything runs on the device; nothing is read back in a loop.
"""
import torch


def _hat(w):
    """(..., 3) -> (..., 3, 3) cross-product matrices."""
    z = torch.zeros_like(w[..., 0])
    return torch.stack((torch.stack((z, -w[..., 2], w[..., 1]), dim=-1),
                        torch.stack((w[..., 2], z, -w[..., 0]), dim=-1),
                        torch.stack((-w[..., 1], w[..., 0], z), dim=-1)), dim=-2)


def se3_exp(xi):
    """xi (..., 6) = (rotation vector w, translation part u) -> (..., 4, 4) rigid transforms exp([w]x, u):
    R = I + A K + B K^2, t = (I + B K + C K^2) u with K = [w]x, A = sin(th)/th, B = (1 - cos th)/th^2, C = (th - sin th)/th^3.
    Below th^2 = 1e-8 the coefficients are their series (exact to rounding there), so the map and its gradient are smooth at
    xi = 0, where a refinement starts."""
    w, u = xi[..., :3], xi[..., 3:]
    t2 = (w * w).sum(-1)
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)
    th = t2s.sqrt()
    A = torch.where(small, 1.0 - t2 / 6.0, torch.sin(th) / th)
    B = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(th)) / t2s)
    Cc = torch.where(small, 1.0 / 6.0 - t2 / 120.0, (th - torch.sin(th)) / (t2s * th))
    K = _hat(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device).expand(K.shape)
    A, B, Cc = (s[..., None, None] for s in (A, B, Cc))
    R = eye + A * K + B * K2
    t = ((eye + B * K + Cc * K2) @ u[..., None])
    top = torch.cat((R, t), dim=-1)
    bottom = torch.zeros_like(top[..., :1, :])
    bottom[..., 0, 3] = 1.0
    return torch.cat((top, bottom), dim=-2)


def rays_at(pose, pix, W, H, focal, z_near, z_far, c=None):
    """Rays (n, 8) = [origin, direction, near, far] of the pixels pix (n,) (flat indices y * W + x) of ONE pinhole camera
    pose (4, 4) camera-to-world: the statements of util.gen_rays / unproj_map (reference util.py:118-148,243-281) as torch
    ops on pose's device and in pose's dtype, so the result is differentiable in pose, focal (a scalar or (fx, fy)) and c
    ((cx, cy); None = the image centre)."""
    dev, dt = pose.device, pose.dtype
    f = torch.as_tensor(focal, dtype=dt, device=dev).flatten()
    fx, fy = f[0], f[-1]
    if c is None:
        cx, cy = W * 0.5, H * 0.5
    else:
        c = torch.as_tensor(c, dtype=dt, device=dev).flatten()
        cx, cy = c[0], c[1]
    pix = torch.as_tensor(pix, device=dev)
    Y = (torch.div(pix, W, rounding_mode="floor").to(dt) - cy) / fy
    X = ((pix % W).to(dt) - cx) / fx
    d = torch.stack((X, -Y, -torch.ones_like(X)), dim=-1)
    d = d / d.norm(dim=-1, keepdim=True)
    dirs = d @ pose[:3, :3].transpose(0, 1)
    orig = pose[:3, 3].expand(dirs.shape[0], -1)
    near = torch.full((dirs.shape[0], 1), float(z_near), dtype=dt, device=dev)
    far = torch.full((dirs.shape[0], 1), float(z_far), dtype=dt, device=dev)
    return torch.cat((orig, dirs, near, far), dim=-1)


def step_pixels(seed, steps, rays_per_step, n_pix):
    """The pixel set of every step of refine_pose: (steps, rays_per_step) flat indices drawn once from `seed` on the host."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    return torch.randint(0, int(n_pix), (int(steps), int(rays_per_step)), generator=g)


def step_seed(seed, step):
    """The key the renderer's sample noise of one refinement step is drawn under (NeRFRenderer.keyed)."""
    return (int(seed) << 20) + int(step)


def rgb_loss(render, rgb_gt):
    """(total, stats) of model.loss.RenderLoss(1, 1): the coarse plus the fine mean squared colour error of a nested render."""
    from .model.loss import RenderLoss
    return RenderLoss(1.0, 1.0)(render, rgb_gt)


def refine_pose(net, renderer, target_image, pose0, focal, z_near, z_far, c=None, steps=10, rays_per_step=64, lr=1e-2, seed=0):
    """Photometric refinement of one camera against a photograph: pose = se3_exp(xi) @ pose0, Adam on the 6-vector xi from 0.
    net: an encoded single-object PixelNeRFNet; target_image (H, W, 3) colours in [0, 1]; pose0 (4, 4) camera-to-world.
    Every step renders a fixed pixel set drawn from `seed` (step_pixels) under renderer.keyed(step_seed(seed, step)) — the
    sample noise is the keyed Philox draw, not torch's generator — and takes the rgb loss of model.loss.RenderLoss.  Only xi
    receives a gradient (the network's parameters keep their .grad).  Returns (pose (4, 4), losses (steps,)), both on the
    device; nothing is read back inside the loop."""
    dev = net.poses.device
    target = torch.as_tensor(target_image, dtype=torch.float32, device=dev)
    H, W = int(target.shape[0]), int(target.shape[1])
    target = target.reshape(H * W, 3)
    pose0 = torch.as_tensor(pose0, dtype=torch.float32, device=dev)
    pix = step_pixels(seed, steps, rays_per_step, H * W).to(dev)
    xi = torch.zeros(6, device=dev, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=lr)
    losses = torch.empty(int(steps), device=dev)
    was = net.differentiable
    net.differentiable = True
    try:
        for i in range(int(steps)):
            rays = rays_at(se3_exp(xi) @ pose0, pix[i], W, H, focal, z_near, z_far, c=c)
            with renderer.keyed(step_seed(seed, i)):
                render = renderer(net, rays[None], want_weights=True)
            total, _ = rgb_loss(render, target[pix[i]][None])
            xi.grad, = torch.autograd.grad(total, xi)
            opt.step()
            losses[i].copy_(total.detach())
    finally:
        net.differentiable = was
    with torch.no_grad():
        return se3_exp(xi) @ pose0, losses
