#!/usr/bin/env python3
"""Wall-clock time of mesh extraction at the reference's default 128^3 grid on the SRN-shaped net in fp16, one
source view, by two routes in one process, in alternating rounds:
  host     the reference's recipe (util/recon.py) with THIS package's net: util.gen_grid and the fake view directions on the
           host, 100 000-point chunks uploaded, one .cpu() per chunk, then the numpy oracle tests/mc_util.py.  The extractor is
           NOT PyMCubes (it is not installed); it is the vectorised numpy restatement the tests compare against.
  device   recon.marching_cubes' route: pnr_grid_points, one net.forward, pnr_mc_count / one read of the counts / pnr_mc_emit on
           the sigma column where it lies, one copy out.
Each route is split into grid, sigma, extraction and copy-out, timed with the host clock and a device synchronise at every
boundary.  The two extraction calls are also timed alone with device events and reported in GB/s against the bytes the
algorithm needs (mc_bytes below).  The level is the 0.7 quantile of sigma (the synthetic weights know no object).
    python tools/bench_mesh.py [--reso 128] [--rounds 5]
The measuring runs in a child process under `timeout` (--timeout seconds); the parent never touches the GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARTS = ("grid", "sigma", "extract", "copy_out")


def mc_bytes(n, n_v, n_t):
    """Bytes the two calls must move for n grid points, n_v vertices, n_t triangles.
    count: the field once (4), the per-point code written and read again by the offsets pass (2 + 2), two offsets written (8).
    emit:  the code once (2); per vertex its two field values, its offset and 3 doubles (8 + 4 + 24); per triangle its offset,
           three owners' code and offset, and 3 indices (4 + 18 + 12)."""
    return n * 16, n * 2 + n_v * 36 + n_t * 34


def worker(a):
    import numpy as np
    import torch

    import golden_util as gu
    import mc_util
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import PixelNeRFNet, recon, util
    from pixel_nerf_multiscale_amd import _native as N
    spec = dict(gu.CASES["full_ns1"])
    torch.manual_seed(0)
    net = PixelNeRFNet(model_conf(spec, "fp32")).cuda().eval()
    for which, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)):
        mlp.load_state_dict({k: torch.from_numpy(v) for k, v in gu.make_mlp_state(spec, which).items()})
    image = torch.rand(1, 1, 3, 128, 128, generator=torch.Generator().manual_seed(1)) * 2 - 1
    pose = torch.from_numpy(np.stack([gu.pose_spherical(30.0, -20.0, 2.0)]))[None]
    net.encode(image.cuda(), pose.cuda(), torch.tensor(131.25)[None].cuda())
    net.precision = "fp16"
    c1, c2, reso, chunk = [-1.0] * 3, [1.0] * 3, [a.reso] * 3, 100000
    n = a.reso ** 3
    sync = torch.cuda.synchronize
    state = {}

    def clock(parts, name, t0):
        sync()
        t1 = time.perf_counter()
        parts[name] = (t1 - t0) * 1e3
        return t1

    def host_route(iso):
        parts = {}
        with torch.no_grad():
            sync()
            t = time.perf_counter()
            grid = util.gen_grid(*zip(c1, c2, reso), ij_indexing=True)
            dirs = -grid / torch.norm(grid, dim=-1).unsqueeze(-1)
            t = clock(parts, "grid", t)
            sig = [net(p.cuda()[None], coarse=True, viewdirs=d.cuda()[None])[0, :, 3].cpu()
                   for p, d in zip(torch.split(grid, chunk), torch.split(dirs, chunk))]
            sigma = torch.cat(sig).view(*reso).numpy()
            t = clock(parts, "sigma", t)
            state["sigma"] = sigma
            if iso is None:
                return parts
            v, tri, _ = mc_util.marching_cubes(sigma, iso)
            v = mc_util.scale_vertices(v, 2.0 / a.reso, c1)
            t = clock(parts, "extract", t)
            parts["copy_out"] = 0.0
            state["host"] = (v, tri)
        return parts

    def device_route(iso):
        parts = {}
        with torch.no_grad():
            sync()
            t = time.perf_counter()
            xyz, dirs = util.gen_grid_device(c1, c2, reso, fake_viewdirs=True)
            t = clock(parts, "grid", t)
            out = net(xyz[None], coarse=True, viewdirs=dirs[None])[0]
            t = clock(parts, "sigma", t)
            v, tri = recon.extract_mesh(out[:, 3].view(*reso), iso, origin=c1, scale=[2.0 / a.reso] * 3)
            t = clock(parts, "extract", t)
            v, tri = v.cpu().numpy(), tri.cpu().numpy()
            t = clock(parts, "copy_out", t)
            state["device"], state["out"] = (v, tri), out
        return parts

    host_route(None)
    iso = float(np.quantile(state["sigma"], 0.7))
    for _ in range(2):                                               # warm-up: code objects, allocators, numpy's pools
        host_route(iso)
        device_route(iso)
    ms = {"host": [], "device": []}
    for _ in range(a.rounds):
        ms["host"].append(host_route(iso))
        ms["device"].append(device_route(iso))
    med = {r: {p: statistics.median(x[p] for x in ms[r]) for p in PARTS} for r in ms}
    tot = {r: [sum(x.values()) for x in ms[r]] for r in ms}
    (vh, th), (vd, td) = state["host"], state["device"]

    # the two extraction calls alone, device events, the counts known
    out = state["out"]
    field = out[:, 3]
    nbytes = int(N.lib.pnr_mc_workspace_bytes(*reso))
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    vbuf = torch.empty(len(vd), 3, dtype=torch.float64, device="cuda")
    tbuf = torch.empty(len(td), 3, dtype=torch.int32, device="cuda")
    d3 = lambda x: (C.c_double * 3)(*x)
    stream = N.current_stream(out.device)
    calls = {
        "count": lambda: N.check(N.lib.pnr_mc_count(field.data_ptr(), 4, *reso, iso, ws.data_ptr(), nbytes, counts.data_ptr(),
                                                    stream), "pnr_mc_count"),
        "emit": lambda: N.check(N.lib.pnr_mc_emit(field.data_ptr(), 4, *reso, iso, d3(c1), d3([2.0 / a.reso] * 3), ws.data_ptr(),
                                                  nbytes, len(vd), len(td), vbuf.data_ptr(), tbuf.data_ptr(), stream), "pnr_mc_emit"),
    }
    us = {k: [] for k in calls}
    for r in range(a.rounds + 1):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            sync()
            if r:
                us[k].append(e0.elapsed_time(e1) / 20 * 1e3)
    assert counts.cpu().tolist() == [len(vd), len(td)]
    bc, be = mc_bytes(n, len(vd), len(td))
    us_med = {k: statistics.median(v) for k, v in us.items()}
    gbs = {"count": bc / us_med["count"] * 1e-3, "emit": be / us_med["emit"] * 1e-3}

    print(f"mesh extraction, {a.reso}^3 = {n} grid points, fp16, 1 source view, level {iso:.4f} (0.7 quantile of sigma): "
          f"{len(vd)} vertices, {len(td)} triangles; ms, median of {a.rounds} alternating rounds")
    print(f"  {'route':<8}" + "".join(f"{p:>11}" for p in PARTS) + f"{'total':>11}{'min':>10}{'max':>10}")
    for r in ("host", "device"):
        print(f"  {r:<8}" + "".join(f"{med[r][p]:>11.3f}" for p in PARTS)
              + f"{statistics.median(tot[r]):>11.3f}{min(tot[r]):>10.3f}{max(tot[r]):>10.3f}")
    print(f"  host route's mesh: {len(vh)} vertices, {len(th)} triangles (its view directions are torch's on the host, the device "
          f"route's are the kernel's: they differ in the last bit, and so may a few fp16 sigmas next to the level)")
    for k, b in (("count", bc), ("emit", be)):
        print(f"  pnr_mc_{k:<6}{us_med[k]:>9.1f} us (min {min(us[k]):.1f}, max {max(us[k]):.1f}; 20 calls per event pair)  "
              f"{b / 1e6:>8.2f} MB algorithmic  {gbs[k]:>8.1f} GB/s")
    print(json.dumps({"what": "mesh_extract", "reso": a.reso, "precision": "fp16", "rounds": a.rounds, "iso": round(iso, 6),
                      "vertices": len(vd), "triangles": len(td), "host_vertices": len(vh), "host_triangles": len(th),
                      **{f"ms_{r}_{p}": round(med[r][p], 3) for r in med for p in PARTS},
                      **{f"ms_{r}_total": round(statistics.median(tot[r]), 3) for r in tot},
                      **{f"us_mc_{k}": round(v, 1) for k, v in us_med.items()}, **{f"gbs_mc_{k}": round(v, 1) for k, v in gbs.items()}}))
    if statistics.median(tot["device"]) > statistics.median(tot["host"]):
        sys.exit("the device route took longer than the host route")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reso", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=400, help="seconds the measuring child process may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--worker", "--reso", str(a.reso),
           "--rounds", str(a.rounds)]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
