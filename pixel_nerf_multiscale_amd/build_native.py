"""Builds libpnr_hip.so in-tree with hipcc for gfx950 (no cmake, no JIT cache).  `python -m
pixel_nerf_multiscale_amd.build_native` or __graft_entry__.build()."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libpnr_hip.so")
SOURCES = ["pnr_api.hip", "stage_kernels.hip", "point_f32.hip", "point_mfma.hip", "train_f32.hip", "cam_grad.hip", "loss.hip", "eval.hip",
           "mesh.hip", "optim.hip", "upsample.hip", "vis.hip", "video.hip", "data.hip", "jitter.hip", "train_draw.hip", "resize.hip",
           "occupancy.hip", "mask_draw.hip", "opacity_loss.hip", "synth.hip"]
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]


def _newer(src_list, out):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in src_list)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(LIBDIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, "pnr_common.h"), os.path.join(HERE, "..", "include", "pnr.h")]
    hdrs += [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    # a library newer than every source and header is current, with or without its object files next to it (a tree copied
    # without *.o must not recompile everything)
    if not force and not _newer([os.path.join(CSRC, s) for s in SOURCES] + hdrs, LIB):
        return LIB
    objs, jobs = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIBDIR, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _newer([src] + hdrs, obj):
            jobs.append([hipcc] + FLAGS + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _newer(objs, LIB):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
