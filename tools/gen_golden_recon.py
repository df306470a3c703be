#!/usr/bin/env python3
"""
Golden vectors for mesh extraction.  Dev container only, like gen_golden.py: imports the reference's own src/util/recon.py
UNMODIFIED, with stand-in modules for what it imports and is not installed —
  mcubes   marching_cubes(volume, level) calls the CPU oracle tests/mc_util.py and records its arguments (PyMCubes' own
           conventions are therefore NOT pinned; everything around it is)
  tqdm     only if it is missing: tqdm(iterable, total=None) -> iterable
— and a stub network (one parameter, use_viewdirs=True) whose forward records its inputs and returns an analytic function
of xyz and viewdirs.  Writes
  tests/golden/recon_wrapper.npz    for a (6, 5, 4) grid with unequal corners: the points and view directions the reference
                                    handed the network chunk by chunk, the sigma volume it handed to mcubes, the index-space
                                    and the final vertices
  tests/golden/save_obj_plain.obj, save_obj_rgb.obj    the reference's save_obj for a six-triangle mesh

    python tools/gen_golden_recon.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402
import mc_util  # noqa: E402

C1, C2, RESO, ISO, CHUNK = [-1.0, -0.5, -0.75], [1.25, 1.0, 0.5], [6, 5, 4], 0.5, 50
RECORD = {}


def _mcubes_marching_cubes(volume, level):
    RECORD["volume"], RECORD["level"] = np.array(volume, copy=True), float(level)
    vertices, triangles, _ = mc_util.marching_cubes(volume, level)
    RECORD["vertices_index"], RECORD["triangles"] = vertices.copy(), triangles.copy()
    return vertices, triangles


class StubNet(torch.nn.Module):
    use_viewdirs = True

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward(self, xyz, coarse=True, viewdirs=None):
        self.calls.append((xyz.clone(), viewdirs.clone(), coarse))
        x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
        sigma = 2.0 - 3.0 * (1.5 * (x - 0.3) ** 2 + (y + 0.1) ** 2 + 0.7 * (z - 0.2) ** 2) + 0.1 * viewdirs[..., 0]
        rgb = torch.sigmoid(xyz + viewdirs)
        return torch.cat((rgb, sigma[..., None]), dim=-1)


def load_reference_recon():
    sys.modules["mcubes"] = types.SimpleNamespace(marching_cubes=_mcubes_marching_cubes)
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.SimpleNamespace(tqdm=lambda it, total=None: it)
    spec = importlib.util.spec_from_file_location("_reference_recon", os.path.join(gen_golden.REF, "util", "recon.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    recon = load_reference_recon()
    net = StubNet().train()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vertices, triangles = recon.marching_cubes(net, c1=C1, c2=C2, reso=RESO, isosurface=ISO, eval_batch_size=CHUNK)
    assert net.training and len(net.calls) == 3 and len(triangles) > 0
    out = dict(c1=np.array(C1), c2=np.array(C2), reso=np.array(RESO), iso=np.array(ISO),
               chunks=np.array([c[0].shape[0] for c in net.calls]),
               xyz=torch.cat([c[0] for c in net.calls]).numpy(), viewdirs=torch.cat([c[1] for c in net.calls]).numpy(),
               volume=RECORD["volume"], vertices_index=RECORD["vertices_index"], triangles=np.asarray(triangles),
               vertices=np.asarray(vertices))
    path = os.path.join(gu.GOLDEN_DIR, "recon_wrapper.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(vertices), "vertices", len(triangles), "triangles")

    rng = np.random.default_rng(5)
    v = np.round(rng.uniform(-2, 2, (8, 3)), 5)
    v[0] = (0.00005, -0.00005, 1.23455)                 # %.4f rounding and a negative zero
    t = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [1, 5, 2], [7, 3, 0]], dtype=np.int32)
    rgb = rng.uniform(0, 1, (8, 3)).astype(np.float32)
    recon.save_obj(v, t, os.path.join(gu.GOLDEN_DIR, "save_obj_plain.obj"))
    recon.save_obj(v, t, os.path.join(gu.GOLDEN_DIR, "save_obj_rgb.obj"), vert_rgb=rgb)
    np.savez_compressed(os.path.join(gu.GOLDEN_DIR, "save_obj_mesh.npz"), vertices=v, triangles=t, rgb=rgb)
    print("wrote save_obj_plain.obj, save_obj_rgb.obj, save_obj_mesh.npz")


if __name__ == "__main__":
    main()
