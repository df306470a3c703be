#!/usr/bin/env python3
"""Wall-clock time per batch of evalio.evaluate_approx with its two back ends: a synthetic loader in the style
of tools/bench_eval.py — batches of --sb objects, 128 x 128 frames, fp16 kernel, one source view, ground truth = the fp32
path's render of the views — evaluated with metrics="host" (the reference's tail: the batch's fp32 frames to the host, numpy /
scipy per object) and metrics="device" (util.eval_frames, one read at the end), both with verbose=False, in one process, in
alternating rounds; and the same batches with no tail at all (view draws, rays, encode, one render call, nothing leaves the
device), which is what the tail's share of a batch is measured against.  Device synchronisation at the two ends of a loop only.
    python tools/bench_eval_approx.py [--sb 4] [--batches 3] [--rounds 5]
The measuring runs in a child process under `timeout` (--timeout seconds); the parent never touches the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def worker(a):
    import torch

    import golden_util as gu
    from eval_util import make_dataset
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio, util
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    from pixel_nerf_multiscale_amd.render.nerf import _RenderWrapper
    W = H = a.size
    SB, NV, seed = a.sb, 3, 1234
    focal = 131.25 * a.size / 128.0
    spec = dict(gu.CASES["full_ns1"])
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).cuda().eval()
    data = make_dataset(net, rend, SB * a.batches, NV, W, H, focal, seed=seed, angle_step=360.0 / NV)
    net.precision = "fp16"
    loader = [dict(images=torch.stack([d["images"] for d in data[b * SB:(b + 1) * SB]]),
                   poses=torch.stack([d["poses"] for d in data[b * SB:(b + 1) * SB]]), focal=torch.full((SB,), focal))
              for b in range(a.batches)]
    zn, zf = data.z_near, data.z_far
    render_par = _RenderWrapper(net, rend, simple_output=True).eval()
    dev = net.poses.device
    results = {}

    def run_evaluate(metrics):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results[metrics] = evalio.evaluate_approx(net, rend, loader, source="0", seed=seed, z_near=zn, z_far=zf, metrics=metrics,
                                                  render_par=render_par, verbose=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.batches * 1e3

    def run_render_only():
        """evaluate_approx's batch without its tail: the same draws, uploads, rays, encode and render call."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.random.manual_seed(seed)
        with torch.no_grad():
            for b, d in enumerate(loader):
                f = d["focal"][0]
                src_view, dest_view = evalio.draw_approx_views(SB, NV, "0")
                dest_poses = util.batched_index_select_nd(d["poses"], dest_view).reshape(SB, 4, 4)
                rays = torch.empty(SB, H * W, 8, device=dev)
                for sb in range(SB):
                    util.gen_rays_device(dest_poses[sb], W, H, f, zn, zf, out=rays[sb])
                net.encode(util.upload(util.batched_index_select_nd(d["images"], src_view).contiguous(), dev),
                           util.upload(util.batched_index_select_nd(d["poses"], src_view).contiguous(), dev), util.upload(f, dev))
                with rend.keyed(frame_seed(seed, b)):
                    render_par(rays)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.batches * 1e3

    variants = {"render_only": run_render_only, "host": lambda: run_evaluate("host"), "device": lambda: run_evaluate("device")}
    for fn in variants.values():                                     # warm-up: MIOpen's choices, the allocators, scipy's import
        fn()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(fn())
    med = {k: statistics.median(v) for k, v in ms.items()}
    base = med["render_only"]
    print(f"evalio.evaluate_approx, {a.batches} batches of SB {SB} objects, one target view of {W} x {H} each, fp16, 64 + 32 samples, "
          f"1 source view; ms per batch (the batch's encode included), median of {a.rounds} alternating rounds (min .. max)")
    print(f"  {'variant':<14}{'ms/batch':>9}{'min':>9}{'max':>9}{'tail ms':>13}{'share of a batch':>18}")
    for k in variants:
        tail = med[k] - base
        print(f"  {k:<14}{med[k]:>9.3f}{min(ms[k]):>9.3f}{max(ms[k]):>9.3f}" + ("" if k == "render_only" else f"{tail:>13.3f}{tail / med[k]:>17.1%}"))
    print(json.dumps({"what": "eval_approx", "sb": SB, "batches": a.batches, "image": f"{W}x{H}", "precision": "fp16",
                      "rounds": a.rounds, **{"ms_" + k: round(v, 3) for k, v in med.items()},
                      **{"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      "psnr_ssim_host": [round(x, 6) for x in results["host"][:2]],
                      "psnr_ssim_device": [round(x, 6) for x in results["device"][:2]]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sb", type=int, default=4, help="objects per batch")
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--sb", str(a.sb),
           "--batches", str(a.batches), "--size", str(a.size), "--rounds", str(a.rounds)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
