"""What the data layer costs per training step: ONE train.make_batch timed to a synchronise, for the same batch (SB objects of
NV views of 128 x 128) handed over three ways, and the whole bf16 step around each, as bench_train.py --front-end builds it.

  host_float   the loader's float32 batch on the host: 12 bytes per pixel pinned and uploaded every step (today's route)
  host_bytes   the loader's uint8 batch on the host: 3 bytes per pixel pinned and uploaded
  resident     data.ResidentSplit.batch(ids): the split lies on the card as bytes, the step gathers its objects there

Alternating rounds (every variant once per round, so drift hits all alike), medians and spread over the rounds.  Prints one
JSON line per source-view count; nothing starts loader worker processes.
    python tools/bench_data.py --precision bf16"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
import hip_util as hu  # noqa: E402


class _Objects(list):
    as_bytes, balanced, z_near, z_far, lindisp = True, True, 0.8, 1.8, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--nv", type=int, default=50)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--objects", type=int, default=8, help="objects in the resident split the batches are drawn from")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16x3"])
    a = ap.parse_args()

    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    from pixel_nerf_multiscale_amd.data._items import images_to_float
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    dev = torch.device("cuda")
    H = W = 128
    rng = np.random.default_rng(9)
    objects = _Objects()
    for o in range(a.objects):
        lo = rng.integers(0, 48, (a.nv, 2))
        objects.append({"path": f"obj{o}", "img_id": o, "focal": 131.25,
                        "images": torch.from_numpy(rng.integers(0, 256, (a.nv, H, W, 3), dtype=np.uint8)),
                        "poses": torch.from_numpy(np.stack([gu.pose_spherical(360.0 * v / a.nv + 11.0 * o, -20.0, 1.3)
                                                            for v in range(a.nv)])).float(),
                        "bbox": torch.from_numpy(np.concatenate([lo, lo + 64], -1).astype(np.float32))})
    split = ResidentSplit(objects, dev)
    ids = list(range(a.sb))
    host_bytes = {k: torch.stack([torch.as_tensor(objects[i][k]) for i in ids]) for k in ("images", "poses", "bbox", "focal")}
    host_float = dict(host_bytes, images=torch.stack([images_to_float(objects[i]["images"], True) for i in ids]))
    sources = {"host_float": lambda: host_float, "host_bytes": lambda: host_bytes, "resident": lambda: split.batch(ids)}

    for ns in a.views:
        spec = gu._case(seed=5, d_hidden=512, lat=[(256, 8, 8)], image=(W, H), focal=131.25, NS=ns, SB=a.sb, N=a.rays, Kc=64,
                        Kf=32, Kfd=16)
        _, poses_np = gu.make_inputs(spec)
        net = hu.build_net(spec, poses_np).train()
        net.train_precision = a.precision
        maps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gu.make_latents(spec)]
        # the trunk is not what this measures: every variant gets the same fixed latent maps
        net.encoder.forward = lambda images: net.encoder.set_latents(maps)
        net.encoder.set_latents(maps)
        rend = hu.build_renderer(spec)
        render_par = rend.bind_parallel(net, None)
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
        kw = dict(ray_batch_size=a.rays, nviews=[ns], z_near=spec["z_near"], z_far=spec["z_far"])
        crit = RenderLoss(1.0, 1.0)

        def front_end(source):
            return lambda: train.make_batch(source(), dev, **kw)

        def step(source):
            def run():
                opt.zero_grad(set_to_none=True)
                loss, _ = train.calc_losses(net, render_par, source(), loss=crit, **kw)
                loss.backward()
                opt.step()
            return run

        variants = {"front_end_" + k: front_end(s) for k, s in sources.items()}
        variants.update({"step_" + k: step(s) for k, s in sources.items()})
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    fn()
                    if k.startswith("front_end_"):
                        torch.cuda.synchronize()            # one make_batch to a synchronise: what a step waits for at worst
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        res = {"what": "data_layer", "sb": a.sb, "nv": a.nv, "image": f"{W}x{H}", "rays_per_obj": a.rays, "views": ns,
               "precision": a.precision, "steps": a.steps, "rounds": a.rounds,
               "bytes_float_batch": host_float["images"].numel() * 4, "bytes_byte_batch": host_bytes["images"].numel(),
               "bytes_resident_pool": split.nbytes}
        res.update({"ms_" + k: round(statistics.median(v), 3) for k, v in ms.items()})
        res.update({"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
