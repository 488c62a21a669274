"""Generate mc_tables.h, the marching-cubes case table of mcubes.hip, from a stated rule (no table is copied).

    python 3dtopia-xl_amd/csrc/gen_mc_tables.py            # rewrites mc_tables.h next to this file
    python 3dtopia-xl_amd/csrc/gen_mc_tables.py --check    # exit 1 if the committed header differs

Conventions
  - corner bit b of a cell sits at offset (b & 1, b >> 1 & 1, b >> 2 & 1) along (axis 0, axis 1, axis 2);
  - a corner is INSIDE when value < iso (strict); cube index bit b = corner b inside;
  - edge e = 4 * axis + (o_lo + 2 * o_hi): the edge along `axis` whose start corner has offset o_lo / o_hi along the
    lower / higher of the two other axes (and 0 along `axis`); its end corner adds 1 along `axis`.

Rule
  On each of the six faces, walk the four corners counter-clockwise as seen from outside the cube.  Every edge whose two
  corners differ in sign is a crossing; a crossing entered from outside (out -> in) is joined by a directed segment to
  the next crossing left towards outside (in -> out).  With two crossings this separates the inside corners from the
  outside ones; with four (the ambiguous face) it cuts off each inside corner separately.  The rule depends on the
  face's four signs only, so two cells agree on every shared face and the surface has no cracks.  Each crossing edge
  lies on two faces that walk it in opposite directions, so it starts one segment and ends one: the segments chain
  into closed loops.  Each loop is fan-triangulated from its lowest edge, wound so that normals point from inside
  (lower values) to outside.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mc_tables.h")


def corner_offset(b):
    return (b & 1, b >> 1 & 1, b >> 2 & 1)


def corner_index(o):
    return o[0] | o[1] << 1 | o[2] << 2


def edges():
    """[(axis, start corner, end corner)] for e = 0..11."""
    out = []
    for axis in range(3):
        lo, hi = [a for a in range(3) if a != axis]
        for m in range(4):
            o = [0, 0, 0]
            o[lo], o[hi] = m & 1, m >> 1
            c0 = corner_index(o)
            o[axis] = 1
            out.append((axis, c0, corner_index(o)))
    return out


EDGES = edges()
EDGE_OF = {frozenset((c0, c1)): e for e, (_, c0, c1) in enumerate(EDGES)}


def faces():
    """Six faces, each as its four corners counter-clockwise about the outward normal."""
    out = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3        # e_b x e_c = e_a
        for side in (0, 1):
            ring = []
            for ob, oc in ((0, 0), (1, 0), (1, 1), (0, 1)):
                o = [0, 0, 0]
                o[a], o[b], o[c] = side, ob, oc
                ring.append(corner_index(o))
            out.append(ring if side == 1 else ring[::-1])   # the side-0 face looks along -e_a
    return out


FACES = faces()


def segments(case):
    """Directed face segments (edge from, edge to) of one cube index."""
    inside = [(case >> b) & 1 for b in range(8)]
    segs = []
    for ring in FACES:
        cross = []      # (position on the ring, 'in' = out -> in / 'out' = in -> out, edge)
        for k in range(4):
            c0, c1 = ring[k], ring[(k + 1) % 4]
            if inside[c0] != inside[c1]:
                cross.append((k, "in" if inside[c1] else "out", EDGE_OF[frozenset((c0, c1))]))
        for n, (k, kind, e) in enumerate(cross):
            if kind != "in":
                continue
            for m in range(1, len(cross)):      # the next in -> out crossing counter-clockwise
                k2, kind2, e2 = cross[(n + m) % len(cross)]
                if kind2 == "out":
                    segs.append((e, e2))
                    break
    return segs


def loops(case):
    nxt = dict(segments(case))
    assert len(nxt) == len(segments(case)), "an edge starts two segments"
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, "open chain"
        out.append(loop)
    return out


def triangles(case):
    """Fan triangles of every loop, wound outward (inside -> outside): out -> in then in -> out on every face makes each
    loop turn counter-clockwise about the inside -> outside direction, so the fan follows the loop order."""
    tris = []
    for loop in loops(case):
        r = loop[loop.index(min(loop)):] + loop[:loop.index(min(loop))]
        for i in range(1, len(r) - 1):
            tris.append((r[0], r[i], r[i + 1]))
    return tris


def tables():
    tri = [[e for t in triangles(c) for e in t] for c in range(256)]
    mask = []
    for c in range(256):
        m = 0
        for e, (_, c0, c1) in enumerate(EDGES):
            if (c >> c0 & 1) != (c >> c1 & 1):
                m |= 1 << e
        mask.append(m)
    return tri, mask


def render() -> str:
    tri, mask = tables()
    assert max(len(t) for t in tri) <= 15
    lines = ["// Generated by gen_mc_tables.py - do not edit.  The rule and the corner / edge conventions are stated there.",
             "#pragma once", "", "#include <stdint.h>", "",
             "// edge e: axis and start corner (bit b at offset (b & 1, b >> 1 & 1, b >> 2 & 1)); the end corner adds 1 along the axis",
             "static constexpr int8_t MC_EDGE_AXIS[12] = {" + ", ".join(str(a) for a, _, _ in EDGES) + "};",
             "static constexpr int8_t MC_EDGE_CORNER[12] = {" + ", ".join(str(c) for _, c, _ in EDGES) + "};", "",
             "// crossing edges of each cube index (bit b = corner b has value < iso)",
             "static constexpr uint16_t MC_EDGE_MASK[256] = {"]
    for r in range(0, 256, 16):
        lines.append("    " + ", ".join(f"0x{m:03x}" for m in mask[r:r + 16]) + ",")
    lines += ["};", "", "// number of triangles of each cube index",
              "static constexpr int8_t MC_NTRI[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t) // 3) for t in tri[r:r + 32]) + ",")
    lines += ["};", "", "// triangles of each cube index: edge triples, wound inside -> outside, -1 terminated (at most 5 triangles)",
              "static constexpr int8_t MC_TRI[256][16] = {"]
    for c in range(256):
        row = tri[c] + [-1] * (16 - len(tri[c]))
        lines.append("    {" + ", ".join(f"{v:2d}" for v in row) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == text else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(OUT)
