"""Numpy restatement of primitive fitting (include/primx_hip.h "Primitive fitting", csrc/meshfield.hip, fit.py) and the
fixtures its tests share.

There are no goldens from the reference: its PrimSDF._init_param is an empty `pass` (models/primsdf.py:48-50), so the rules
of the header are restated here - in float64 as the reference value, and in float32 (`dtype=np.float32`: the same
expressions, every operation rounded to float32 in the order the header gives) as the bit-exact model of areas, surface
points, FPS and `nn`, and as the measure of what fp32 costs the query (tests/test_hip_meshfield.py takes its bounds from
float32-against-float64 of this file on the test's own inputs).
"""
from __future__ import annotations

import numpy as np

INV_2PI = 0.15915494309189535          # the query multiplies the atan2 sum by this (2 sum / 4 pi)


# ------------------------------------------------------------------------------------------------------------ fixtures
def icosphere(level: int = 2, radius: float = 0.5, center=(0.0, 0.0, 0.0)):
    """Outward-oriented icosphere: 20 * 4^level faces, float32 vertices, int32 faces."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    vv = (np.asarray(v) * radius + np.asarray(center, dtype=np.float64)).astype(np.float32)
    return vv, np.asarray(f, dtype=np.int32)


def box(lo=(-0.3, -0.2, -0.4), hi=(0.35, 0.25, 0.15)):
    """Axis-aligned box of 12 outward-oriented triangles."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)]).astype(np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    f = []
    for a, b, c, d in quads:
        f += [(a, b, c), (a, c, d)]
    return v, np.asarray(f, dtype=np.int32)


def hemisphere(level: int = 2, radius: float = 0.5):
    """The faces of the icosphere whose centroid has z > 0: an open surface (unreferenced vertices stay in v)."""
    v, f = icosphere(level, radius)
    keep = v[f].astype(np.float64).mean(1)[:, 2] > 0
    return v, np.ascontiguousarray(f[keep])


def join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += v.shape[0]
    return np.concatenate(vs).astype(np.float32), np.concatenate(fs).astype(np.int32)


def mesh_with_faces(F: int):
    """A mesh of exactly F faces: icospheres, the box and the hemisphere concatenated, the face list cut at F."""
    parts = [icosphere(1), box(), hemisphere(1, 0.7), icosphere(2, 0.3, (0.2, -0.1, 0.1)), icosphere(2, 0.6, (-0.1, 0.1, 0.0)),
             icosphere(3, 0.45, (0.05, 0.05, -0.1))]
    v, f = join(*parts)
    assert F <= f.shape[0]
    return v, np.ascontiguousarray(f[:F])


def affine_attr(v, C: int = 5):
    """Per-vertex attributes affine in xyz, clipped to [0, 1]: [V, C] float32."""
    rng = np.random.default_rng(11)
    A, b = rng.uniform(-0.9, 0.9, (3, C)), rng.uniform(0.3, 0.7, C)
    return np.clip(v.astype(np.float64) @ A + b, 0.0, 1.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the query
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _xyz(a):
    """[..., 3] -> its three components, each contiguous (vectors are handled as (x, y, z) tuples below)."""
    return tuple(np.ascontiguousarray(a[..., k]) for k in range(3))


def face_kind(a, b, c):
    """a, b, c: (x, y, z) tuples of scalars.  0 triangle; 1 / 2 / 3: zero-area, measured as the segment ab / ac / bc (the
    longest, the first of equals)."""
    ab, ac, bc = _sub(b, a), _sub(c, a), _sub(c, b)
    n = _cross(ab, ac)
    if n[0] != 0 or n[1] != 0 or n[2] != 0:
        return 0
    best, kind = _dot(ab, ab), 1
    if _dot(ac, ac) > best:
        best, kind = _dot(ac, ac), 2
    if _dot(bc, bc) > best:
        kind = 3
    return kind


def pair(p, a, b, c, kind, dtype):
    """p, a, b, c: (x, y, z) tuples.  Points [n] against one face (scalars) -> (d2, v, w, term), each [n]; or points [n, 1]
    against a block of triangles [1, k] (kind 0 only) -> [n, k].  Every operation in `dtype`."""
    one, zero = dtype(1), dtype(0)
    ab, ac = _sub(b, a), _sub(c, a)
    ap, bp, cp = _sub(p, a), _sub(p, b), _sub(p, c)
    if kind != 0:
        e, o = (ab, ap) if kind == 1 else (ac, ap) if kind == 2 else (_sub(c, b), bp)
        l = _dot(e, e)
        t = _dot(o, e) / l if l > 0 else np.zeros(p[0].shape, dtype)
        t = np.minimum(np.maximum(t, zero), one)
        z = np.zeros_like(t)
        v, w = (t, z) if kind == 1 else (z, t) if kind == 2 else (one - t, t)
        d = tuple(p[k] - ((a[k] + ab[k] * v) + ac[k] * w) for k in range(3))
        return _dot(d, d), v, w, z
    la2, lb2, lc2 = _dot(ap, ap), _dot(bp, bp), _dot(cp, cp)
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e43, e56 = d4 - d3, d5 - d6
    z = np.zeros_like(d1)
    nv, nw, den, region = vb, vc, (va + vb) + vc, np.full(d1.shape, 6, np.int8)
    m = (va <= 0) & (e43 >= 0) & (e56 >= 0)
    nv, nw, den, region = np.where(m, z, nv), np.where(m, e43, nw), np.where(m, e43 + e56, den), np.where(m, np.int8(5), region)
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    nv, nw, den, region = np.where(m, z, nv), np.where(m, d2, nw), np.where(m, d2 - d6, den), np.where(m, np.int8(4), region)
    region = np.where((d6 >= 0) & (d5 <= d6), np.int8(3), region)
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    nv, nw, den, region = np.where(m, d1, nv), np.where(m, z, nw), np.where(m, d1 - d3, den), np.where(m, np.int8(2), region)
    region = np.where((d3 >= 0) & (d4 <= d3), np.int8(1), region)
    region = np.where((d1 <= 0) & (d2 <= 0), np.int8(0), region)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(den != 0, one / den, zero).astype(dtype)
    v, w = nv * inv, nw * inv
    v = np.where(region == 5, one - w, v)
    d = tuple(p[k] - ((a[k] + ab[k] * v) + ac[k] * w) for k in range(3))
    dd = _dot(d, d)
    for r, l2, vv, ww in ((0, la2, zero, zero), (1, lb2, one, zero), (3, lc2, zero, one)):
        m = region == r
        dd, v, w = np.where(m, l2, dd), np.where(m, vv, v), np.where(m, ww, w)
    la, lb, lc = np.sqrt(la2), np.sqrt(lb2), np.sqrt(lc2)
    num = -_dot(ap, _cross(bp, cp))
    dn = (((la * lb) * lc + _dot(ap, bp) * lc) + _dot(bp, cp) * la) + _dot(cp, ap) * lb
    return dd.astype(dtype), v.astype(dtype), w.astype(dtype), np.arctan2(num, dn).astype(dtype)


def _corner(v, f, k):
    return _xyz(v[f[..., k]])


def query(p, v, f, attr=None, dtype=np.float64, block=16, keep_d2=True):
    """-> dict(dist, face, wn[, attr][, d2 [n, F] of every face]).  The kind of a face is decided in `dtype`, as the kernel's
    preparation launch decides it in fp32.  Faces are evaluated `block` at a time (numpy's overhead); the running minimum
    (the first of equals) and the winding sum advance face by face, in face order, as the kernel's do."""
    p, v = np.asarray(p).astype(dtype), np.asarray(v).astype(dtype)
    n, F = p.shape[0], f.shape[0]
    best, face, acc = np.full(n, np.inf, dtype), np.zeros(n, np.int64), np.zeros(n, dtype)
    d2all = np.empty((n, F), dtype) if keep_d2 else None
    pc, pb = _xyz(p), _xyz(p[:, None, :])
    for lo in range(0, F, block):
        fb = f[lo:lo + block]
        a, b, c = (tuple(x[None] for x in _corner(v, fb, k)) for k in range(3))
        d2, _, _, term = pair(pb, a, b, c, 0, dtype)
        for j in range(fb.shape[0]):
            aj, bj, cj = (tuple(x[0, j] for x in t) for t in (a, b, c))
            kind = face_kind(aj, bj, cj)
            if kind != 0:
                d2[:, j], _, _, term[:, j] = pair(pc, aj, bj, cj, kind, dtype)
            m = d2[:, j] < best
            best, face = np.where(m, d2[:, j], best), np.where(m, lo + j, face)
            acc = acc + term[:, j]
        if keep_d2:
            d2all[:, lo:lo + block] = d2
    out = {"dist": np.sqrt(best), "face": face, "wn": acc * dtype(INV_2PI)}
    if keep_d2:
        out["d2"] = d2all
    if attr is not None:
        out["attr"] = attr_on_face(p, v, f, attr, face, dtype)
    return out


def query_threaded(p, v, f, attr=None, dtype=np.float64, threads=8, **kw):
    """`query` on `threads` slices of the points at once (numpy releases the interpreter lock inside its loops)."""
    from concurrent.futures import ThreadPoolExecutor
    p = np.asarray(p)
    cuts = np.linspace(0, p.shape[0], min(threads, max(p.shape[0] // 256, 1)) + 1).astype(int)
    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(lambda k: query(p[cuts[k]:cuts[k + 1]], v, f, attr, dtype, **kw), range(len(cuts) - 1)))
    return {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}


def attr_on_face(p, v, f, attr, face, dtype=np.float64):
    """The interpolation of attr at the closest point of each point's GIVEN face (one evaluation of `pair` with every point
    against its own face; zero-area faces one by one)."""
    p, v, attr = np.asarray(p).astype(dtype), np.asarray(v).astype(dtype), np.asarray(attr).astype(dtype)
    face = np.asarray(face, np.int64)
    fa = f[face]
    a, b, c = (_corner(v, fa, k) for k in range(3))
    n = _cross(_sub(b, a), _sub(c, a))
    _, vv, ww, _ = pair(_xyz(p), a, b, c, 0, dtype)
    for t in np.unique(face[(n[0] == 0) & (n[1] == 0) & (n[2] == 0)]):
        m = face == t
        aj, bj, cj = (tuple(x for x in v[f[t, k]]) for k in range(3))
        _, vv[m], ww[m], _ = pair(_xyz(p[m]), aj, bj, cj, face_kind(aj, bj, cj), dtype)
    u = (dtype(1) - vv) - ww
    return (attr[fa[:, 0]] * u[:, None] + attr[fa[:, 1]] * vv[:, None]) + attr[fa[:, 2]] * ww[:, None]


def sdf_of(q):
    return np.where(np.abs(q["wn"]) >= 0.5, -q["dist"], q["dist"])


# ------------------------------------------------------------------------------------------------ areas, points, fps
def face_areas(v, f):
    v = v.astype(np.float64)
    n = _cross(_xyz(v[f[:, 1]] - v[f[:, 0]]), _xyz(v[f[:, 2]] - v[f[:, 0]]))
    return 0.5 * np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])


def surface_points(v, f, cdf, u):
    """cdf [F] float64 inclusive, u [N, 3] float32 -> (pts [N, 3] float32, face [N])."""
    v, u = v.astype(np.float32), u.astype(np.float32)
    target = u[:, 0].astype(np.float64) * cdf[-1]
    face = np.minimum(np.searchsorted(cdf, target, side="right"), f.shape[0] - 1)
    one = np.float32(1)
    r = np.sqrt(u[:, 1])
    w0, w1, w2 = one - r, r * (one - u[:, 2]), r * u[:, 2]
    A, B, C = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    return (w0[:, None] * A + w1[:, None] * B) + w2[:, None] * C, face.astype(np.int32)


def _d2(pts, c):
    d = pts - c
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def fps(pts, K: int, start: int = 0):
    """float32 farthest point sampling -> (idx [K] int32, nn [K] float32)."""
    pts = pts.astype(np.float32)
    mind = np.full(pts.shape[0], np.inf, np.float32)
    idx = np.empty(K, np.int32)
    idx[0] = start
    for k in range(K):
        mind = np.minimum(mind, _d2(pts, pts[idx[k]]))
        if k + 1 < K:
            idx[k + 1] = np.argmax(mind)                 # the first of equal maxima
    cen = pts[idx]
    nn = np.zeros(K, np.float32)
    for k in range(K if K > 1 else 0):
        d2 = _d2(cen, cen[k])
        d2[k] = np.inf
        nn[k] = np.sqrt(d2.min())
    return idx, nn


# ------------------------------------------------------------------------------------------------ the whole fit
def normalize(v, extent=0.9):
    """float32, as fit.normalize_vertices: box centre to the origin, longest half side to `extent`."""
    v = v.astype(np.float32)
    lo, hi = v.min(0), v.max(0)
    c = (lo + hi) * np.float32(0.5)
    half = ((hi - lo) * np.float32(0.5)).max()
    s = np.float32(extent / float(half))
    return (v - c) * s, c, s


def mesh_to_primitives(v, f, attr, u, lin, num_prims, prim_shape, normalize_mesh=True, extent=0.9, dtype=np.float64,
                       field=None):
    """u: the [candidates, 3] float32 uniforms; lin: the float32 linspace(-1, 1, S) table of PrimSDF.  The geometry part
    (srt) is float32 by definition; the payload is evaluated in `dtype` (`field`: a replacement for `query`, for threads).
    -> (recon_param [P, 4 + 6 S^3] in dtype, info)."""
    v = v.astype(np.float32)
    if normalize_mesh:
        v, _, _ = normalize(v, extent)
    cdf = np.cumsum(face_areas(v, f))
    cand, cface = surface_points(v, f, cdf, u)
    idx, nn = fps(cand, num_prims, 0)
    pos, S = cand[idx], prim_shape
    lin = np.asarray(lin, np.float32)
    zz, yy, xx = np.meshgrid(lin, lin, lin, indexing="ij")
    grid = np.stack([xx, yy, zz], -1).reshape(-1, 3)                         # [z][y][x] order, (x, y, z) per row
    x = (pos[:, None, :] + nn[:, None, None] * grid[None]).astype(np.float32)
    q = (field or (lambda pts: query(pts, v, f, attr, dtype)))(x.reshape(-1, 3))
    sdf = sdf_of(q).reshape(num_prims, 1, S ** 3)
    a = np.clip(q["attr"], 0, 1).reshape(num_prims, S ** 3, -1).transpose(0, 2, 1)
    rp = np.concatenate([nn[:, None].astype(dtype), pos.astype(dtype), sdf.reshape(num_prims, -1),
                         a.reshape(num_prims, -1)], 1)
    return rp, {"v": v, "cand": cand, "cand_face": cface, "idx": idx, "x": x, "q": q}
