"""Derives the marching-cubes case table of csrc/mesh.hip and writes pixel_nerf_multiscale_amd/csrc/mc_tables.h.

No table is typed in: every case follows from one rule, so the rule can be read and the result checked (tests/test_mesh_cpu.py
regenerates the header text and verifies the properties below).

  corners   c = 0..7 at offsets (c & 1, (c >> 1) & 1, (c >> 2) & 1) along grid axes 0, 1, 2
  edges     the 12 corner pairs that differ in one bit: e = 4 * axis + slot, slot = the rank of the edge's LOWER corner among
            the four corners whose `axis` bit is clear (EDGE_CORNERS)
  faces     for each of the 6 faces the crossed edges are connected: two crossings give one segment; four crossings (two
            diagonal corners inside) give two segments, each cutting off one INSIDE corner.  Only the face's own four signs
            enter, so the two cells that share a face always agree on it.
  direction every segment runs with its inside corner on the left as seen from outside the cube; the segments then form
            directed closed loops over the crossed edges
  fans      a loop is cut into a fan from the first of its rotations none of whose diagonals joins two edges of a common
            cube face: such a diagonal lies in the face plane, where the neighbouring cell can produce the same mesh edge
            again (a non-manifold edge).  Rotation 0 starts at the loop's smallest edge.
  winding   the fan's triangles are emitted so that their normals point from the inside (field >= iso) to the outside

usage: python tools/gen_mc_tables.py [--check]     (--check: compare with the committed header, write nothing)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "pixel_nerf_multiscale_amd", "csrc", "mc_tables.h")


def corner_offset(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def _edge_corners():
    out = []
    for axis in range(3):
        for lower in (c for c in range(8) if not (c >> axis) & 1):
            out.append((lower, lower | (1 << axis)))
    return out


EDGE_CORNERS = _edge_corners()                       # edge -> (lower corner, upper corner)
EDGE_AXIS = [e >> 2 for e in range(12)]
EDGE_OF = {frozenset(cc): e for e, cc in enumerate(EDGE_CORNERS)}


def edges_share_face(e0, e1):
    """Both edges lie on one of the six cube faces: some coordinate is the same for all four end corners."""
    cs = EDGE_CORNERS[e0] + EDGE_CORNERS[e1]
    return any(len({(c >> a) & 1 for c in cs}) == 1 for a in range(3))


def _face_cycle(axis, side):
    """The face's four corners, counter-clockwise as seen from outside the cube, with their 2-D face coordinates."""
    u, v = (axis + 1) % 3, (axis + 2) % 3            # e_u x e_v = e_axis: right-handed with the outward normal of side 1
    if side == 0:
        u, v = v, u
    cyc = []
    for x, y in ((0, 0), (1, 0), (1, 1), (0, 1)):
        cyc.append(((side << axis) | (x << u) | (y << v), (x, y)))
    return cyc


def _segments(mask):
    """Directed segments (from edge, to edge) of one inside mask over all six faces."""
    segs = []
    for axis in range(3):
        for side in (0, 1):
            cyc = _face_cycle(axis, side)
            inside = [(mask >> c) & 1 for c, _ in cyc]
            crossed = [k for k in range(4) if inside[k] != inside[(k + 1) % 4]]      # face edge k joins corners k, k + 1
            mid = lambda k: tuple((a + b) / 2 for a, b in zip(cyc[k][1], cyc[(k + 1) % 4][1]))
            eid = lambda k: EDGE_OF[frozenset((cyc[k][0], cyc[(k + 1) % 4][0]))]
            if len(crossed) == 2:
                pairs = [(crossed[0], crossed[1], inside.index(1))]
            elif len(crossed) == 4:                  # corner k inside: its two face edges are k - 1 and k
                pairs = [((k - 1) % 4, k, k) for k in range(4) if inside[k]]
            else:
                assert not crossed
                continue
            for ka, kb, kin in pairs:
                p, q, c = mid(ka), mid(kb), cyc[kin][1]
                left = (-(q[1] - p[1]), q[0] - p[0])                                 # (q - p) turned a quarter counter-clockwise
                s = (c[0] - p[0]) * left[0] + (c[1] - p[1]) * left[1]
                assert s != 0
                segs.append((eid(ka), eid(kb)) if s > 0 else (eid(kb), eid(ka)))
    return segs


def loops_of(mask):
    """Directed closed loops over the crossed edges, each starting at its smallest edge, ordered by that edge."""
    segs = _segments(mask)
    nxt = dict(segs)
    assert len(nxt) == len(segs) and sorted(nxt) == sorted(nxt.values()), "segments do not form closed loops"
    crossed = {e for e, (a, b) in enumerate(EDGE_CORNERS) if ((mask >> a) ^ (mask >> b)) & 1}
    assert set(nxt) == crossed
    loops, seen = [], set()
    for e in sorted(nxt):
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def fan_rotation(loop):
    """First rotation whose fan diagonals all avoid joining two edges of a common cube face."""
    n = len(loop)
    for r in range(n):
        rot = loop[r:] + loop[:r]
        if not any(edges_share_face(rot[0], rot[i]) for i in range(2, n - 1)):
            return r
    raise AssertionError(f"no valid fan for loop {loop}")


def case_triangles(mask):
    tris = []
    for loop in loops_of(mask):
        r = fan_rotation(loop)
        rot = loop[r:] + loop[:r]
        for i in range(1, len(rot) - 1):
            tris.append((rot[0], rot[i + 1], rot[i]))       # the loop runs clockwise round the outward normal: reverse it
    return tris


def build_table():
    return [case_triangles(m) for m in range(256)]


def rotation_census():
    """(loops fanned from rotation 0, loops fanned from a later rotation) over all cases."""
    rots = [fan_rotation(l) for m in range(256) for l in loops_of(m)]
    return sum(r == 0 for r in rots), sum(r > 0 for r in rots)


def header_text():
    table = build_table()
    total = sum(len(t) for t in table)
    lines = [
        "// GENERATED by tools/gen_mc_tables.py — do not edit; tests/test_mesh_cpu.py compares this file with the generator's output.",
        "// Marching-cubes case table.  Corner c sits at offsets (c & 1, (c >> 1) & 1, (c >> 2) & 1) along grid axes 0, 1, 2; bit c of",
        "// a case is set when that corner is inside (field >= iso).  Edge e = 4 * axis + slot runs along `axis` from the slot-th",
        "// corner whose `axis` bit is clear.  Row = 16 bytes: up to 5 triangles x 3 edges, 0xff padding, byte 15 = triangle count.",
        f"// {total} triangles over the 256 cases; normals point from inside to outside.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "#define PNR_MC_MAX_TRIS 5",
        f"#define PNR_MC_TOTAL_TRIS {total}",
        "",
        "// The includer defines PNR_MC_TABLE_DECL, the table's qualifiers (csrc/mesh.hip: 16-byte aligned device memory).",
        "PNR_MC_TABLE_DECL uint8_t PNR_MC_TABLE[256][16] = {",
    ]
    for m, tris in enumerate(table):
        assert len(tris) <= 5
        row = [e for t in tris for e in t]
        row += [0xFF] * (15 - len(row)) + [len(tris)]
        lines.append("    {" + ", ".join(f"{v:3d}" for v in row) + "},   // " + format(m, "08b"))
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv:
        same = os.path.exists(HEADER) and open(HEADER).read() == text
        print("mc_tables.h is", "current" if same else "STALE")
        sys.exit(0 if same else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER, "rotations (0, later):", rotation_census())
