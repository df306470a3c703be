#!/usr/bin/env python3
"""
Golden CAMERA gradients.  Dev container only, like gen_golden_grad.py: runs the reference's renderer + PixelNeRFNet under
autograd on the fixture inputs with the rays, the camera-to-world source poses, focal and c as leaves, replaying the noise
draws recorded in the forward fixture, with gen_golden_grad.py's loss, and writes tests/golden/<case>_camgrad.npz:
    rays_od (SB, N, 6), rays_nf (SB, N, 2), poses (SB, NS, 4, 4), focal, c   the reference's own gradients, flat (c absent where
                                                                           the case passes none); rays_od = origin and
                                                                           direction, rays_nf = near and far
    <key>__norm                                                            the l2 norm of each
    loss                                                                   the scalar

    python tools/gen_golden_cam_grad.py [case ...]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (sets up sys.path for the reference + shims + tests)
import gen_golden_grad as ggg  # noqa: E402
import golden_util as gu  # noqa: E402

CASES = ["tiny_sb2_ns2", "tiny_sb2_ns2_intr"]


def run(name, NeRFRenderer, PixelNeRFNet):
    fx = gu.load_fixture(name)
    spec = fx["spec"]
    net, renderer, enc, rays_np, poses_np = gg.build_case(spec, NeRFRenderer, PixelNeRFNet)
    W, H = spec["image"]
    focal_np, c_np = gu.intrinsics(spec)
    leaf = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).clone().requires_grad_(True)
    poses, focal, rays = leaf(poses_np), leaf(focal_np), leaf(rays_np)
    c = None if c_np is None else leaf(c_np)
    net.encode(torch.zeros(spec["SB"], spec["NS"], 3, H, W), poses, focal, c=c)
    G = {k: torch.from_numpy(v) for k, v in gu.make_loss_weights(spec).items()}
    with ggg.NoisePlayer(fx):
        out = renderer(net, rays, want_weights=True)
    loss = 0.0
    for tag in ("coarse", "fine") if renderer.using_fine else ("coarse",):
        lvl = getattr(out, tag)
        loss = loss + (lvl.rgb * G[f"{tag}_rgb"]).sum() + (lvl.depth * G[f"{tag}_depth"]).sum() \
            + (lvl.weights * G[f"{tag}_weights"]).sum()
    assert np.array_equal(out.coarse.rgb.detach().numpy(), fx["coarse_rgb"])       # the forward fixture's forward
    loss.backward()
    res = {"loss": np.float64(loss.item())}
    named = dict(rays_od=rays.grad[..., :6], rays_nf=rays.grad[..., 6:], poses=poses.grad, focal=focal.grad)
    if c is not None:
        named["c"] = c.grad
    for key, g in named.items():
        g = g.detach().numpy().astype(np.float32)
        assert np.isfinite(g).all() and g.size <= gu.GRAD_SAMPLES, key
        res[key] = g.reshape(-1)
        res[key + "__norm"] = np.float64(np.linalg.norm(g.astype(np.float64)))
    path = os.path.join(gu.GOLDEN_DIR, name + "_camgrad.npz")
    np.savez_compressed(path, **res)
    print(f"{name}: loss={loss.item():.6f} " + " ".join(f"{k}{tuple(np.shape(v))}" for k, v in named.items())
          + f" -> {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    NeRFRenderer, PixelNeRFNet = gg.load_reference()
    for n in sys.argv[1:] or CASES:
        run(n, NeRFRenderer, PixelNeRFNet)


if __name__ == "__main__":
    main()
