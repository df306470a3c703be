"""Shared by tests/test_synthetic_cpu.py and tests/test_gpu_synthetic.py: the numpy float32 model of pnr_synth_render, written
from the text of include/pnr.h ("procedural datasets") with one rounded operation per line and np.float32 throughout, and an
independent fp64 analytic ray cast with its own code (matrix products, np.minimum / np.maximum slabs, both roots), which shares
no helper with the model.  The model takes planted mistakes by name, so that the tests can show that their checks reject them."""
import numpy as np

F32 = np.float32
REC = 20
INF = F32(np.inf)
MISTAKES = ("far_root", "untransposed_rotation", "normal_sign", "centre_mask", "clamp_255", "round_down")


# ------------------------------------------------------------------------------------------- scenes and cameras of the tests
def record(kind, centre=(0, 0, 0), rot=None, half=(0.1, 0.1, 0.1), albedo=(0.5, 0.5, 0.5)):
    r = np.zeros(REC, dtype=F32)
    r[0] = kind
    r[1:4] = centre
    r[4:13] = (np.eye(3) if rot is None else np.asarray(rot)).reshape(9)
    r[13:16] = half
    r[16:19] = albedo
    return r


def rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])          # world -> local of a body turned by `angle` about z


def rot_x(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, s], [0.0, -s, c]])


def table(*scenes, P=None):
    """Scenes (lists of records) -> float32 (n, P, REC), padded with kind 0."""
    P = max(len(s) for s in scenes) if P is None else P
    out = np.zeros((len(scenes), P, REC), dtype=F32)
    for i, s in enumerate(scenes):
        for p, r in enumerate(s):
            out[i, p] = r
    return out


def named_scenes():
    """The three scenes of the issue, as one table: a sphere of radius 0.5; a box of half-extents (0.3, 0.2, 0.4) turned 0.6 rad
    about z; an ellipsoid and a box that overlap, the box with an albedo above 1 so that lit faces saturate and only the clamp to
    254 keeps them foreground."""
    sphere = [record(1, half=(0.5, 0.5, 0.5), albedo=(0.8, 0.4, 0.2))]
    box = [record(2, rot=rot_z(0.6), half=(0.3, 0.2, 0.4), albedo=(0.3, 0.7, 0.9))]
    two = [record(1, centre=(0.1, 0.0, 0.05), rot=rot_x(0.4) @ rot_z(0.3), half=(0.3, 0.15, 0.2), albedo=(0.9, 0.2, 0.3)),
           record(2, centre=(-0.1, 0.05, -0.05), rot=rot_z(-0.5) @ rot_x(0.2), half=(0.15, 0.25, 0.2), albedo=(1.6, 1.5, 1.7))]
    return table(sphere, box, two)


def orbit_pose(azim_deg, elev_deg, radius=1.3):
    """float32 (4, 4) camera-to-world of a camera on the sphere that looks at the origin (x right, y up, looks down -z; world z
    up), written out with trigonometry, independently of data.synthetic.view_poses."""
    az, el = np.radians(azim_deg), np.radians(elev_deg)
    back = np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    right = np.array([-np.sin(az), np.cos(az), 0.0])
    up = np.cross(back, right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, up, back, radius * back
    return pose.astype(F32)


def issue_poses():
    return np.stack([orbit_pose(a, -20.0) for a in (0.0, 37.0, 123.0)])


def light32(light):
    l = np.asarray(light, dtype=np.float64)
    return (l / np.sqrt((l * l).sum())).astype(F32)


# ------------------------------------------------------------------------------------------- the float32 model of the header
def _dot3(a0, a1, a2, b0, b1, b2):
    p0 = a0 * b0
    p1 = a1 * b1
    p2 = a2 * b2
    s = p0 + p1
    return s + p2


def model_render(scenes, scene_ids, poses, W, H, fx, fy, cx, cy, ss=2, ambient=0.3, light=(0.3, 0.5, 0.8), mistake=None):
    """-> (rgb uint8 (F, H, W, 3), mask uint8 (F, H, W), depth float32 (F, H, W)): include/pnr.h, step by step."""
    assert mistake is None or mistake in MISTAKES
    scenes = np.asarray(scenes, dtype=F32)
    poses = np.asarray(poses, dtype=F32)
    n, P, _ = scenes.shape
    F = len(scene_ids)
    fx, fy, cx, cy, ambient = F32(fx), F32(fy), F32(cx), F32(cy), F32(ambient)
    one_minus = F32(1.0) - ambient
    l = light32(light)
    inv = F32(1.0 / (ss * ss))
    rgb = np.zeros((F, H, W, 3), dtype=np.uint8)
    mask = np.zeros((F, H, W), dtype=np.uint8)
    depth = np.zeros((F, H, W), dtype=F32)
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rows, cols = rows.reshape(-1).astype(F32), cols.reshape(-1).astype(F32)
    N = H * W
    with np.errstate(all="ignore"):
        for f in range(F):
            sid = int(scene_ids[f])
            recs = scenes[sid] if 0 <= sid < n else np.zeros((0, REC), dtype=F32)
            C, o = poses[f, :3, :3], poses[f, :3, 3]
            acc = [np.zeros(N, dtype=F32) for _ in range(3)]
            any_hit = np.zeros(N, dtype=bool)
            for b in range(ss):
                y = rows + F32((b + 0.5) / ss - 0.5)
                v = -((y - cy) / fy)
                for a in range(ss):
                    x = cols + F32((a + 0.5) / ss - 0.5)
                    u = (x - cx) / fx
                    ln = np.sqrt((u * u + v * v) + F32(1.0))
                    dc = (u / ln, v / ln, F32(-1.0) / ln)
                    d = [_dot3(C[i, 0], C[i, 1], C[i, 2], dc[0], dc[1], dc[2]) for i in range(3)]
                    t, col, hit = _model_sample(recs, o, d, l, ambient, one_minus, mistake)
                    if b == 0 and a == 0:
                        depth[f] = t.reshape(H, W)
                        first_hit = hit
                    any_hit |= hit
                    for c in range(3):
                        acc[c] = acc[c] + col[c]
            covered = first_hit if mistake == "centre_mask" else any_hit
            for c in range(3):
                mean = acc[c] * inv
                w = mean * F32(255.0)
                if mistake != "round_down":
                    w = w + F32(0.5)
                byte = np.where(~(w > 0), 0, np.where(w >= 255, 255, np.floor(w))).astype(np.int64)
                if mistake != "clamp_255":
                    byte = np.where(covered, np.minimum(byte, 254), byte)
                rgb[f, :, :, c] = byte.reshape(H, W)
            mask[f] = np.where(covered, 255, 0).reshape(H, W)
    return rgb, mask, depth


def _model_sample(recs, o, d, l, ambient, one_minus, mistake):
    N = d[0].shape[0]
    best = np.full(N, INF, dtype=F32)
    win = np.full(N, -1, dtype=np.int64)
    win_face = np.zeros(N, dtype=np.int64)
    win_tp = np.zeros(N, dtype=F32)
    local = []
    for p, r in enumerate(recs):
        kind = r[0]
        local.append(None)
        if kind != 1 and kind != 2:
            continue
        R = r[4:13].reshape(3, 3)
        Rl = R.T if mistake == "untransposed_rotation" else R
        h = r[13:16]
        q = [o[j] - r[1 + j] for j in range(3)]
        ol = [_dot3(Rl[i, 0], Rl[i, 1], Rl[i, 2], q[0], q[1], q[2]) for i in range(3)]
        dl = [_dot3(Rl[i, 0], Rl[i, 1], Rl[i, 2], d[0], d[1], d[2]) for i in range(3)]
        local[-1] = (Rl, h, ol, dl)
        if kind == 1:
            tc = -_dot3(ol[0], ol[1], ol[2], dl[0], dl[1], dl[2])
            shift = [tc * dl[i] for i in range(3)]
            os_ = [ol[i] + shift[i] for i in range(3)]
            oe = [os_[i] / h[i] for i in range(3)]
            de = [dl[i] / h[i] for i in range(3)]
            A = _dot3(de[0], de[1], de[2], de[0], de[1], de[2])
            B = _dot3(oe[0], oe[1], oe[2], de[0], de[1], de[2])
            Cq = _dot3(oe[0], oe[1], oe[2], oe[0], oe[1], oe[2]) - F32(1.0)
            bb = B * B
            ac = A * Cq
            disc = bb - ac
            sq = np.sqrt(disc)
            num = (-B + sq) if mistake == "far_root" else (-B - sq)
            tp = num / A
            t = tc + tp
            hit = (disc > 0) & (t > 0)
            upd = hit & (t < best)
            best = np.where(upd, t, best).astype(F32)
            win = np.where(upd, p, win)
            win_tp = np.where(upd, tp, win_tp).astype(F32)
        else:
            tn = np.full(N, -INF, dtype=F32)
            tf = np.full(N, INF, dtype=F32)
            face = np.zeros(N, dtype=np.int64)
            miss = np.zeros(N, dtype=bool)
            for a in range(3):
                zero = dl[a] == 0
                miss |= zero & (np.abs(ol[a]) > h[a])
                t1 = (-h[a] - ol[a]) / dl[a]
                t2 = (h[a] - ol[a]) / dl[a]
                lo = np.where(t2 < t1, t2, t1)
                hi = np.where(t2 > t1, t2, t1)
                c1 = ~zero & (lo > tn)
                tn = np.where(c1, lo, tn).astype(F32)
                face = np.where(c1, a, face)
                c2 = ~zero & (hi < tf)
                tf = np.where(c2, hi, tf).astype(F32)
            hit = ~miss & (tn < tf) & (tn > 0)
            upd = hit & (tn < best)
            best = np.where(upd, tn, best).astype(F32)
            win = np.where(upd, p, win)
            win_face = np.where(upd, face, win_face)
    col = [np.ones(N, dtype=F32) for _ in range(3)]
    for p, r in enumerate(recs):
        sel = win == p
        if local[p] is None or not sel.any():
            continue
        Rl, h, ol, dl = local[p]
        if r[0] == 1:
            g = []
            tc = -_dot3(ol[0], ol[1], ol[2], dl[0], dl[1], dl[2])
            for i in range(3):
                shift = tc * dl[i]
                oe = (ol[i] + shift) / h[i]
                de = dl[i] / h[i]
                td = win_tp * de
                g.append((oe + td) / h[i])
            m = [(Rl[0, j] * g[0] + Rl[1, j] * g[1]) + Rl[2, j] * g[2] for j in range(3)]
            ln = np.sqrt(_dot3(m[0], m[1], m[2], m[0], m[1], m[2]))
            nrm = [m[j] / ln for j in range(3)]
        else:
            row = Rl[win_face]                                                # (N, 3)
            dlf = _dot3(row[:, 0], row[:, 1], row[:, 2], d[0], d[1], d[2])
            s = np.where(dlf > 0, F32(-1.0), F32(1.0)).astype(F32)
            nrm = [row[:, j] * s for j in range(3)]
        if mistake == "normal_sign":
            nrm = [-v for v in nrm]
        k = _dot3(nrm[0], nrm[1], nrm[2], l[0], l[1], l[2])
        k = np.where(k > 0, k, F32(0.0)).astype(F32)
        shade = ambient + one_minus * k
        for c in range(3):
            col[c] = np.where(sel, r[16 + c] * shade, col[c]).astype(F32)
    return best, col, win >= 0


# ------------------------------------------------------------------------------------------- the fp64 analytic ray cast
def reference_render(scenes, scene_ids, poses, W, H, fx, fy, cx, cy, ss=1, ambient=0.3, light=(0.3, 0.5, 0.8)):
    """The same pictures from analytic geometry in float64, by other means: rays as one array, the local frames by matrix
    products, the quadratic's two roots, slabs by np.minimum / np.maximum.  -> dict: rgb (F, H, W, 3) uint8 by the byte rule,
    value (F, H, W, 3) the real number w = mean * 255 + 0.5 before the floor, mask (F, H, W) bool (any sub-sample hit), depth
    (F, H, W) of the first sub-sample (inf on a miss), winner (F, H, W) the primitive the first sub-sample hit (-1: none),
    margin (F, H, W): the smallest |discriminant| or |slab gap| over the pixel's sub-samples and primitives."""
    scenes = np.asarray(scenes, dtype=np.float64)
    poses = np.asarray(poses, dtype=np.float64)
    F = len(scene_ids)
    lgt = np.asarray(light, dtype=np.float64)
    lgt = lgt / np.linalg.norm(lgt)
    out = {"rgb": np.zeros((F, H, W, 3), np.uint8), "value": np.zeros((F, H, W, 3)), "mask": np.zeros((F, H, W), bool),
           "depth": np.full((F, H, W), np.inf), "winner": np.full((F, H, W), -1), "margin": np.full((F, H, W), np.inf)}
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))          # (H, W): column, row
    with np.errstate(all="ignore"):
        for f in range(F):
            sid = int(scene_ids[f])
            recs = scenes[sid] if 0 <= sid < scenes.shape[0] else []
            cam, eye = poses[f, :3, :3], poses[f, :3, 3]
            total = np.zeros((H, W, 3))
            for sb in range(ss):
                for sa in range(ss):
                    px = jj + (sa + 0.5) / ss - 0.5
                    py = ii + (sb + 0.5) / ss - 0.5
                    dirs = np.stack(((px - cx) / fx, -(py - cy) / fy, -np.ones_like(px)), axis=-1)
                    dirs = dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)
                    dirs = dirs @ cam.T
                    nearest = np.full((H, W), np.inf)
                    who = np.full((H, W), -1)
                    colour = np.ones((H, W, 3))
                    for p, r in enumerate(recs):
                        kind, centre, rot, half, albedo = int(r[0]), r[1:4], r[4:13].reshape(3, 3), r[13:16], r[16:19]
                        if kind not in (1, 2):
                            continue
                        lo_ = rot @ (eye - centre)
                        ld = dirs @ rot.T
                        if True:
                            if kind == 1:
                                so, sd = lo_ / half, ld / half
                                qa, qb, qc = (sd * sd).sum(-1), 2.0 * (sd * so).sum(-1), (so * so).sum() - 1.0
                                disc = qb * qb - 4.0 * qa * qc
                                root = np.sqrt(np.maximum(disc, 0.0))
                                t = np.minimum((-qb - root) / (2.0 * qa), (-qb + root) / (2.0 * qa))
                                ok = (disc > 0) & (t > 0)
                                margin = np.abs(disc) / 4.0                       # the header's disc = B B - A Cq has b = 2 B
                                grad = (so + t[..., None] * sd) / half
                                normal = grad @ rot
                                normal = normal / np.linalg.norm(normal, axis=-1, keepdims=True)
                            else:
                                ta, tb = (-half - lo_) / ld, (half - lo_) / ld
                                parallel = ld == 0
                                enter = np.where(parallel, -np.inf, np.minimum(ta, tb))
                                leave = np.where(parallel, np.inf, np.maximum(ta, tb))
                                outside = (parallel & (np.abs(lo_) > half)).any(-1)
                                t, t_out = enter.max(-1), leave.min(-1)
                                ok = ~outside & (t < t_out) & (t > 0)
                                margin = np.where(outside, np.inf, np.abs(t_out - t))
                                axis = enter.argmax(-1)
                                sign = -np.sign(np.take_along_axis(ld, axis[..., None], -1)[..., 0])
                                normal = rot[axis] * sign[..., None]
                        out["margin"][f] = np.minimum(out["margin"][f], margin)
                        take = ok & (t < nearest)
                        nearest = np.where(take, t, nearest)
                        who = np.where(take, p, who)
                        lambert = np.maximum((normal * lgt).sum(-1), 0.0)
                        shade = albedo[None, None, :] * (ambient + (1.0 - ambient) * lambert)[..., None]
                        colour = np.where(take[..., None], shade, colour)
                    total += colour
                    out["mask"][f] |= who >= 0
                    if sa == 0 and sb == 0:
                        out["depth"][f], out["winner"][f] = nearest, who
            value = total / (ss * ss) * 255.0 + 0.5
            byte = np.clip(np.floor(value), 0, 255)
            out["value"][f] = value
            out["rgb"][f] = np.where(out["mask"][f][..., None], np.minimum(byte, 254), 255).astype(np.uint8)
    return out


def implicit(scenes, sid, prim, points):
    """The implicit function of primitive `prim` of scene `sid` at world points (..., 3), float64: |R (x - c) / h|^2 - 1 for an
    ellipsoid, max_a(|R (x - c)|_a - h_a) for a box; both are 0 on the surface."""
    r = np.asarray(scenes, dtype=np.float64)[sid, prim]
    local = (np.asarray(points, dtype=np.float64) - r[1:4]) @ r[4:13].reshape(3, 3).T
    if int(r[0]) == 1:
        return ((local / r[13:16]) ** 2).sum(-1) - 1.0
    return (np.abs(local) - r[13:16]).max(-1)
