"""Steps per second of train.Trainer on a synthetic SRN-like tree (objects of 50 views of 128 x 128, SB 4, bf16 products, the real
encoder), three ways, and train.make_batch alone to a synchronise under both kinds of draws.

  loader_host      host draws, a DataLoader over the as_bytes dataset (PNG decode + collate + upload every step)
  resident_host    host draws, data.ResidentSplit (the split on the card; a step uploads its index buffer)
  resident_device  device draws, data.ResidentSplit(device_boxes=True) (pnr_train_draw; a step uploads its intrinsics only)

The host-draw rows run make_batch as it was before the `draws` keyword, so they are the baseline.  Every configuration trains
the same number of epochs after one warm-up epoch; no checkpoint, validation or picture falls into the timed part.  Prints one
JSON line.
    python tools/bench_trainer.py --epochs 3

--ranks N (at most 8) measures the data-parallel loop instead: the resident_device configuration under
Trainer(data_parallel=True), once with 1 rank and once with N, each in a torch.distributed.run of its own that this script starts
under a time limit of its own (one process per card; the global batch --sb must divide by N).  It needs N cards: on a machine that
shows fewer it prints "not measured: one card" and measures nothing.
    python tools/bench_trainer.py --ranks 8 --sb 8 --objects 32"""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import data_trees as dt  # noqa: E402
import golden_util as gu  # noqa: E402
from hip_util import model_conf  # noqa: E402


def write_tree(root, n_obj, nv, size):
    stems = ["%06d" % v for v in range(nv)]
    for o in range(n_obj):
        lo = np.random.default_rng(o).integers(8, 40, (nv, 2))
        images = dt.boxed_views(nv, size, size, [(int(c), int(r), int(c) + 64, int(r) + 64) for c, r in lo], seed=o)
        poses = np.stack([gu.pose_spherical(360.0 * v / nv + 11.0 * o, -20.0, 1.3) for v in range(nv)]).astype(np.float32)
        poses[:, :, 1:3] *= -1.0
        dt.write_srn_object(os.path.join(root, "cars_train", "obj%03d" % o), images, poses, 131.25, size / 2, size / 2, stems)


MAX_RANKS = 8
RANK_RUN_SECONDS = 600         # the time limit of ONE torch.distributed.run of --ranks


def rank_worker(a):
    """One rank of --ranks (started by torch.distributed.run): resident_device under Trainer(data_parallel=True); rank 0 prints
    the steps per second of the timed epochs as one JSON line."""
    import torch.distributed as dist
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, train
    from pixel_nerf_multiscale_amd.data import ResidentSplit, get_split_dataset
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist.init_process_group("nccl", device_id=dev)
    try:
        dataset = get_split_dataset("srn", os.path.join(a.worker, "cars"), want_split="train", as_bytes=True)
        torch.manual_seed(0)
        net = PixelNeRFNet(model_conf(dict(gu.CASES["full_ns1"]), "fp32")).to(dev)
        net.train_precision = a.precision
        rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).to(dev)
        never = 10 ** 9
        t = train.Trainer(net, rend, ResidentSplit(dataset, dev, device_boxes=True), None, name="ranks",
                          checkpoints_path=os.path.join(a.worker, "ckpt"), logs_path=os.path.join(a.worker, "logs"), batch_size=a.sb,
                          ray_batch_size=a.rays, nviews=a.views, loss=RenderLoss(1.0, 1.0), num_epochs=1 + a.epochs, draws="device",
                          seed=3, print_interval=never, save_interval=never, eval_interval=never, vis_interval=never,
                          data_parallel=True)
        with contextlib.redirect_stdout(io.StringIO()):
            t.train_epoch(0)
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            for epoch in range(1, 1 + a.epochs):
                t.train_epoch(epoch)
            torch.cuda.synchronize()
            dist.barrier()
        if dist.get_rank() == 0:
            print(json.dumps({"ranks": dist.get_world_size(), "steps_per_s": round(a.epochs * t.batches_per_epoch / (time.perf_counter() - t0), 3)}),
                  flush=True)
    finally:
        dist.destroy_process_group()


def measure_ranks(a):
    """--ranks: this process never opens a card; it counts them, writes the tree and starts one torch.distributed.run per world
    size, each under its own time limit."""
    n = min(int(a.ranks), MAX_RANKS)
    cards = torch.cuda.device_count()
    if cards < 2 or n < 2:
        print("not measured: one card", flush=True)
        return
    if cards < n:
        print(f"not measured: {n} ranks asked for, {cards} cards", flush=True)
        return
    if a.sb % n != 0:
        raise SystemExit(f"--sb {a.sb} does not divide over {n} ranks")
    res = {"what": "trainer_ranks", "sb": a.sb, "nv": a.nv, "objects": a.objects, "rays_per_obj": a.rays, "views": a.views,
           "precision": a.precision, "epochs": a.epochs, "steps_per_epoch": a.objects // a.sb}
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp, a.objects, a.nv, 128)
        for world in (1, n):
            cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--nproc_per_node", str(world), os.path.abspath(__file__),
                   "--worker", tmp, "--sb", str(a.sb), "--rays", str(a.rays), "--epochs", str(a.epochs), "--precision", a.precision,
                   "--views", *[str(v) for v in a.views]]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=RANK_RUN_SECONDS)
            if done.returncode != 0:
                raise SystemExit(f"{world} ranks: exit status {done.returncode}\n{done.stderr[-2000:]}")
            line = next(l for l in reversed(done.stdout.splitlines()) if l.startswith("{"))
            res[f"steps_per_s_{world}_ranks"] = json.loads(line)["steps_per_s"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--nv", type=int, default=50)
    ap.add_argument("--objects", type=int, default=16)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs per configuration, after one warm-up epoch")
    ap.add_argument("--rounds", type=int, default=20, help="make_batch calls per kind of draw")
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16x3"])
    ap.add_argument("--ranks", type=int, default=0, help=f"measure the data-parallel loop at 1 and N <= {MAX_RANKS} ranks instead (needs N cards)")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)      # a rank of --ranks: the tree's folder
    a = ap.parse_args()
    if a.worker:
        return rank_worker(a)
    if a.ranks:
        return measure_ranks(a)

    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, train
    from pixel_nerf_multiscale_amd.data import ResidentSplit, get_split_dataset
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    dev = torch.device("cuda")
    size = 128
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp, a.objects, a.nv, size)
        dataset = get_split_dataset("srn", os.path.join(tmp, "cars"), want_split="train", as_bytes=True)
        sources = {"loader_host": (lambda: dataset, "host"), "resident_host": (lambda: ResidentSplit(dataset, dev), "host"),
                   "resident_device": (lambda: ResidentSplit(dataset, dev, device_boxes=True), "device")}
        res = {"what": "trainer", "sb": a.sb, "nv": a.nv, "objects": a.objects, "image": f"{size}x{size}", "rays_per_obj": a.rays,
               "views": a.views, "precision": a.precision, "epochs": a.epochs, "steps_per_epoch": a.objects // a.sb}
        for name, (make, draws) in sources.items():
            torch.manual_seed(0)
            net = PixelNeRFNet(model_conf(dict(gu.CASES["full_ns1"]), "fp32")).cuda()
            net.train_precision = a.precision
            rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).cuda()
            never = 10 ** 9
            t = train.Trainer(net, rend, make(), None, name=name, checkpoints_path=os.path.join(tmp, "ckpt"),
                              logs_path=os.path.join(tmp, "logs"), batch_size=a.sb, ray_batch_size=a.rays, nviews=a.views,
                              loss=RenderLoss(1.0, 1.0), num_epochs=1 + a.epochs, draws=draws, seed=3, print_interval=never,
                              save_interval=never, eval_interval=never, vis_interval=never)
            with contextlib.redirect_stdout(io.StringIO()):
                t.train_epoch(0)                                     # warm-up: allocations, kernel selection, the pinned blocks
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for epoch in range(1, 1 + a.epochs):
                    t.train_epoch(epoch)
                torch.cuda.synchronize()
            steps = a.epochs * t.batches_per_epoch
            res["steps_per_s_" + name] = round(steps / (time.perf_counter() - t0), 3)

        # make_batch alone, to a synchronise: what a step waits for at worst
        split = ResidentSplit(dataset, dev, device_boxes=True)
        data = split.batch(list(range(a.sb)))
        kw = dict(ray_batch_size=a.rays, nviews=a.views, z_near=dataset.z_near, z_far=dataset.z_far, balanced=True)
        for draws in ("host", "device"):
            ms = []
            for i in range(3 + a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                train.make_batch(data, dev, draws=draws, seed=frame_seed(3, i), **kw)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            res[f"ms_make_batch_{draws}"] = round(statistics.median(ms[3:]), 3)
            res[f"spread_ms_make_batch_{draws}"] = round(max(ms[3:]) - min(ms[3:]), 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
