#!/usr/bin/env python3
"""
Golden vectors for the camera paths of the video drivers.  Dev container only, like gen_golden_rays.py: imports the
reference's own util.pose_spherical, coord_from_blender, coord_to_blender and quat_to_rot (src/util/util.py:151-176,314-328,
489-509) UNMODIFIED (third-party stand-ins from tools/_shims) and records into tests/golden/video_paths.npz what they return:
the orbit of eval/gen_video.py:166-172 (pose_spherical at np.linspace(-180, 180, num_views + 1)[:-1]) for a handful of
(num_views, elevation, radius), the same orbits left-multiplied by coord_from_blender (eval/eval_real.py:100-107), the two
blender matrices, and quat_to_rot of a dozen quaternions, unnormalised ones among them.  It also stores the key table of the
reference's DTU trajectory (eval/gen_video.py:124-137: knots, 5 x 4 quaternions, scales) as data in
tests/golden/video_dtu_keys.npz, the argument video.quat_path takes.  Arrays only.

    python tools/gen_golden_video.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: F401,E402  (puts the reference + shims + tests on sys.path)
import golden_util as gu  # noqa: E402

ORBITS = [(3, -10.0, 2.0), (5, -30.0, 1.3), (8, 0.0, 2.0), (24, 25.0, 0.5 * (1.25 + 2.75)), (40, -10.0, 2.7)]   # num_views, elevation, radius


def quats():
    rng = np.random.default_rng(406)
    q = rng.normal(0.0, 1.0, (12, 4)).astype(np.float32)
    q[:4] /= np.linalg.norm(q[:4], axis=1, keepdims=True)          # four of unit length (to fp32 rounding), eight that are not
    q[4] = [1.0, 0.0, 0.0, 0.0]
    q[5] = [0.0, 0.0, 3.0, 0.0]
    q[6] *= np.float32(1e-3)
    q[7] *= np.float32(250.0)
    return q


def dtu_keys():
    """The key table of the reference's DTU trajectory (eval/gen_video.py:124-137), read out of the script's syntax tree — the
    script cannot be imported (it parses arguments and renders) and the table is nowhere else: the first list literal in the
    value of each of the three assignments."""
    import ast
    src = open(os.path.join(os.path.dirname(gen_golden.REF), "eval", "gen_video.py")).read()
    found = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
            if name in ("t_in", "pose_quat", "scales") and name not in found:
                lists = [n for n in ast.walk(node.value) if isinstance(n, ast.List)]
                found[name] = np.array(ast.literal_eval(lists[0]), np.float32)
    assert found["t_in"].shape == found["scales"].shape and found["pose_quat"].shape == (len(found["t_in"]), 4)
    return found["t_in"], found["pose_quat"], found["scales"]


def main():
    import util  # the reference's src/util
    t_in, quats_in, scales = dtu_keys()
    path = os.path.join(gu.GOLDEN_DIR, "video_dtu_keys.npz")
    np.savez_compressed(path, t_in=t_in, quats=quats_in, scales=scales)
    print("wrote", path, os.path.getsize(path), "bytes")
    out = {"orbits": np.array(ORBITS, np.float64), "from_blender": util.coord_from_blender().numpy(),
           "to_blender": util.coord_to_blender().numpy()}
    for i, (nv, el, radius) in enumerate(ORBITS):
        angles = np.linspace(-180, 180, nv + 1)[:-1]
        poses = torch.stack([util.pose_spherical(angle, el, radius) for angle in angles], 0)
        blender = torch.stack([util.coord_from_blender() @ util.pose_spherical(angle, el, radius) for angle in angles], 0)
        assert poses.shape == (nv, 4, 4) and poses.dtype == torch.float32
        out[f"orbit{i}__poses"] = poses.numpy()
        out[f"orbit{i}__from_blender"] = blender.numpy()
    q = quats()
    out["quats"] = q
    out["quat_rot"] = util.quat_to_rot(torch.from_numpy(q)).numpy()
    path = os.path.join(gu.GOLDEN_DIR, "video_paths.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
