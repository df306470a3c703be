#!/usr/bin/env python3
"""Wall-clock time per view of evalio.evaluate with its two back ends: a synthetic dataset in the style of
tests/test_gpu_eval_loop.py — 128 x 128 frames, fp16 kernel, one source view, --views target views per object, ground truth =
the fp32 path's render of the same views — evaluated with metrics="host" (the reference's recipe: fp32 rgb + depth to the
host, numpy / scipy) and metrics="device" (util.eval_frame), with write_images off and on, in one process, in alternating
rounds; and the same views rendered with no back end at all (encode + render_image, nothing leaves the device), which is what
the back end's share of a view is measured against.  Device synchronisation at the two ends of a loop only.
    python tools/bench_eval.py [--objects 2] [--views 24] [--rounds 5]
The measuring runs in a child process under `timeout` (--timeout seconds); the parent never touches the GPU."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def worker(a):
    import torch

    import golden_util as gu
    from eval_util import make_dataset
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    W = H = a.size
    focal, NV, seed = 131.25 * a.size / 128.0, a.views + 1, 777
    spec = dict(gu.CASES["full_ns1"])
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).cuda().eval()
    data = make_dataset(net, rend, a.objects, NV, W, H, focal, seed=seed, angle_step=360.0 / NV)
    net.precision = "fp16"
    n_views = a.objects * a.views
    tmp = tempfile.mkdtemp(prefix="bench_eval_")
    results = {}

    def run_evaluate(metrics, write_images):
        out = os.path.join(tmp, "out")
        shutil.rmtree(out, ignore_errors=True)                       # a fresh directory: nothing to resume
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evalio.evaluate(net, rend, data, out, source="0", verbose=False, seed=seed, metrics=metrics,
                              write_images=write_images)
        torch.cuda.synchronize()
        results[metrics] = res
        return (time.perf_counter() - t0) / n_views * 1e3

    def run_render_only():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            for o, d in enumerate(data):
                net.encode(d["images"][:1].cuda()[None], d["poses"][:1].cuda()[None], torch.tensor(focal)[None].cuda())
                for v in range(1, NV):
                    rend.forced_seed = frame_seed(frame_seed(seed, o), v)
                    rend.render_image(net, d["poses"][v], W, H, focal, data.z_near, data.z_far)
        rend.forced_seed = None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n_views * 1e3

    variants = {"render_only": run_render_only,
                "host": lambda: run_evaluate("host", False), "device": lambda: run_evaluate("device", False),
                "host+png": lambda: run_evaluate("host", True), "device+png": lambda: run_evaluate("device", True)}
    try:
        for fn in variants.values():                                 # warm-up: MIOpen's choices, the allocators, scipy's import
            fn()
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                ms[k].append(fn())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    base = med["render_only"]
    print(f"evalio.evaluate, {a.objects} objects x {a.views} target views of {W} x {H}, fp16, 64 + 32 samples, 1 source view; "
          f"ms per view (the object's encode included), median of {a.rounds} alternating rounds (min .. max)")
    print(f"  {'variant':<14}{'ms/view':>9}{'min':>9}{'max':>9}{'back end ms':>13}{'share of a view':>17}")
    for k in variants:
        back = med[k] - base
        print(f"  {k:<14}{med[k]:>9.3f}{min(ms[k]):>9.3f}{max(ms[k]):>9.3f}" + ("" if k == "render_only" else f"{back:>13.3f}{back / med[k]:>16.1%}"))
    print(json.dumps({"what": "eval_back_end", "objects": a.objects, "views": a.views, "image": f"{W}x{H}", "precision": "fp16",
                      "rounds": a.rounds, **{"ms_" + k: round(v, 3) for k, v in med.items()},
                      **{"spread_ms_" + k: round(max(v) - min(v), 3) for k, v in ms.items()},
                      "psnr_ssim_host": [round(x, 6) for x in results["host"][:2]],
                      "psnr_ssim_device": [round(x, 6) for x in results["device"][:2]]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=2)
    ap.add_argument("--views", type=int, default=24, help="target views per object")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--objects", str(a.objects),
           "--views", str(a.views), "--size", str(a.size), "--rounds", str(a.rounds)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
