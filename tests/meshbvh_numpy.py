"""Numpy restatement of the mesh BVH (include/primx_hip.h "Mesh BVH", csrc/meshbvh.hip, fit.MeshBVH): the tree, held in
float32 as the kernel stores it and in float64 as it was summed, and both walks.

The per-pair arithmetic is tests/meshfield_numpy.py's (`MF.pair`), as the kernel's is csrc/meshfield_pair.h's.  A walk in
float64 takes its decisions - which node is skipped, which is opened - from the SAME float32 expressions as the float32 walk
and the kernel, so all three visit the same nodes and differ by rounding alone: decided in float64, a node on the edge of the
opening criterion would move wn by the approximation's error, not by rounding.  The distance walk goes left first where the
kernel takes the nearer child first: rule Q1 makes the result independent of the order, and `visits` tells what a walk cost.
"""
from __future__ import annotations

import numpy as np

from tests import meshfield_numpy as MF

LEAF = 8
DELTA_SCALE = 2.0 ** -17
BETA = 2.0
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------ fixtures
def shifted_icosphere(level=2, shift=37.0):
    """The icosphere moved by +shift on every axis, in float32: coordinates whose ulp is 2^-18 against a radius of 0.5."""
    v, f = MF.icosphere(level)
    return (v + F32(shift)).astype(F32), f


def slivers(n=600, seed=5):
    """n separate triangles of aspect 1e-7 .. 1e-3 (height over base) in [-0.6, 0.6]^3, of random orientation."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.6, 0.6, (n, 3))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    e = np.cross(d, rng.standard_normal((n, 3)))
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    base = rng.uniform(0.05, 0.3, (n, 1))
    aspect = 10.0 ** rng.uniform(-7, -3, (n, 1))
    b = a + d * base
    c = a + d * base * rng.uniform(0.2, 0.8, (n, 1)) + e * base * aspect
    v = np.stack([a, b, c], 1).reshape(-1, 3).astype(F32)
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def points(v, f, n=1000, seed=0):
    """The recipe of tests/test_hip_meshfield.py::_points about the mesh's own bounding box (that one assumes a mesh about the
    origin): uniform points of the neighbourhood, and points a little off the surface on both sides."""
    rng = np.random.default_rng(seed)
    c = ((v.min(0).astype(F64) + v.max(0)) / 2)
    far = c + rng.uniform(-0.8, 0.8, (n - n // 3, 3))
    cdf = np.cumsum(MF.face_areas(v, f))
    if not cdf[-1] > 0:
        return (c + rng.uniform(-0.8, 0.8, (n, 3))).astype(F32)
    on, _ = MF.surface_points(v, f, cdf, rng.random((n // 3, 3)).astype(F32))
    near = on + rng.normal(0, 0.01, on.shape)
    p = np.concatenate([far, near]).astype(F32)
    return p[rng.permutation(n)]


def surface_points(v, f, n, seed=0, offset=0.0):
    """n points on the surface (float32), moved by `offset` along +x, +y and +z."""
    cdf = np.cumsum(MF.face_areas(v, f))
    on, _ = MF.surface_points(v, f, cdf, np.random.default_rng(seed).random((n, 3)).astype(F32))
    return (on + F32(offset)).astype(F32)


# ------------------------------------------------------------------------------------------------------------ the tree
def _spread10(x):
    x = x.astype(np.int64)
    out = np.zeros_like(x)
    for b in range(10):
        out |= ((x >> b) & 1) << (3 * b)
    return out


def face_keys(v, f):
    """B1, B2 -> (keys [F] int64, lo [3], hi [3], m): fp32, expressions as written."""
    v = np.asarray(v, F32)
    lo, hi = v.min(0), v.max(0)
    m = F32(max(np.abs(lo).max(), np.abs(hi).max()))
    ext = max(max(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2])
    s = F32(1024) / ext if ext > 0 else F32(0)
    cen = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / F32(3)
    q = np.minimum(np.maximum((cen - lo) * s, F32(0)), F32(1023)).astype(np.int64)
    code = (_spread10(q[:, 0]) << 2) | (_spread10(q[:, 1]) << 1) | _spread10(q[:, 2])
    return (code << 32) | np.arange(f.shape[0], dtype=np.int64), lo, hi, m


def face_kinds(v, f):
    """The field query's fp32 decision per face: 0 a triangle, 1 / 2 / 3 zero-area."""
    v = np.asarray(v, F32)
    return np.array([MF.face_kind(*(tuple(v[t[k]]) for k in range(3))) for t in f], np.int8)


def _finish(lo, hi, mom, count):
    """B5's last step for a batch of nodes -> (float64 fields, float32 fields); empty nodes as the kernel leaves them."""
    lo64, hi64 = lo.astype(F64), hi.astype(F64)
    live = count > 0
    S = mom[:, 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(S > 0, mom[:, 4:7] / S, 0.5 * (lo64 + hi64))
        e = np.maximum(p - lo64, hi64 - p)
        r = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    N = mom[:, 0:3]
    Cm = mom[:, 7:16].reshape(-1, 3, 3) - p[:, :, None] * N[:, None, :]
    z = lambda a: np.where(live.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0.0)   # noqa: E731
    p, r, N, Cm = z(p), z(r), z(N), z(Cm)
    return {"p": p, "r": r, "N": N, "C": Cm}


def build(v, f, delta_scale=DELTA_SCALE, leaf=LEAF):
    """-> the tree: 'order' [F], 'L', 'nleaf', 'delta', per node i in 1 .. 2 L - 1 (row 0 unused) 'lo', 'hi' [2 L, 3] float32
    (inflated; +inf / -inf where empty), 'count' [2 L], 'mom' [2 L, 16] float64, and 'p', 'r', 'N', 'C' in float64 ('f64') and
    rounded to float32 once ('f32')."""
    v, f = np.asarray(v, F32), np.asarray(f)
    F = f.shape[0]
    keys, _, _, m = face_keys(v, f)
    order = np.argsort(keys, kind="stable")
    delta = F32(m * F32(delta_scale))
    nleaf = (F + leaf - 1) // leaf
    L = 1
    while L < nleaf:
        L *= 2
    lo = np.full((2 * L, 3), np.inf, F32)
    hi = np.full((2 * L, 3), -np.inf, F32)
    count = np.zeros(2 * L, np.int64)
    mom = np.zeros((2 * L, 16), F64)
    kinds = face_kinds(v, f)
    tri = v[f[order]]                                        # [F, 3 corners, 3] in sorted order
    for j in range(leaf):                                    # the j-th face of every leaf at once: sorted order within a leaf
        s = np.arange(nleaf) * leaf + j
        ok = s < F
        s, node = s[ok], L + np.arange(nleaf)[ok]
        t = tri[s]
        lo[node] = np.minimum(lo[node], t.min(1))
        hi[node] = np.maximum(hi[node], t.max(1))
        count[node] += 1
        a, b, c = (t[:, k].astype(F64) for k in range(3))
        ab, ac = b - a, c - a
        A = 0.5 * np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                            ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
        A = np.where((kinds[order[s]] == 0)[:, None], A, 0.0)                   # a zero-area face adds nothing
        ar = np.sqrt((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2])
        cen = ((a + b) + c) / 3.0
        mom[node, 0:3] += A
        mom[node, 3] += ar
        mom[node, 4:7] += ar[:, None] * cen
        mom[node, 7:16] += (cen[:, :, None] * A[:, None, :]).reshape(-1, 9)
    live = count[L:] > 0
    lo[L:][live] = lo[L:][live] - delta
    hi[L:][live] = hi[L:][live] + delta
    first = L // 2
    while first >= 1:
        i = np.arange(first, 2 * first)
        lo[i], hi[i] = np.minimum(lo[2 * i], lo[2 * i + 1]), np.maximum(hi[2 * i], hi[2 * i + 1])
        count[i] = count[2 * i] + count[2 * i + 1]
        mom[i] = mom[2 * i] + mom[2 * i + 1]
        first //= 2
    f64 = _finish(lo, hi, mom, count)
    f32 = {k: a.astype(F32) for k, a in f64.items()}
    return {"order": order, "L": L, "nleaf": nleaf, "leaf": leaf, "F": F, "delta": delta, "lo": lo, "hi": hi, "count": count,
            "mom": mom, "f64": f64, "f32": f32, "kinds": kinds}


def node_image(tree):
    """[2 L, 24] float32 as the kernel lays a node out (row 0 is not written by the kernel)."""
    L, t = tree["L"], tree["f32"]
    img = np.zeros((2 * L, 24), F32)
    img[:, 0:3], img[:, 3:6], img[:, 6] = tree["lo"], tree["hi"], t["r"]
    img[:, 7] = tree["count"].astype(np.int32).view(F32)
    img[:, 8:11], img[:, 11:14], img[:, 14:23] = t["p"], t["N"], t["C"].reshape(-1, 9)
    return img


def leaf_faces(tree, node):
    """The sorted positions of a leaf's faces."""
    first = tree["leaf"] * (node - tree["L"])
    return range(first, min(first + tree["leaf"], tree["F"]))


# ------------------------------------------------------------------------------------------------------------ the walks
def box_d2(p, lo, hi):
    """Q1's lb2 for points p [n, 3] (float32) against one box, as written."""
    e = np.maximum(np.maximum(lo - p, p - hi), F32(0))
    return (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]


def walk_distance(tree, p, v, f, prune=True):
    """Q1 in float32 -> dict(dist, face, d2 [n], visits [n] = nodes arrived at + faces measured).  prune=False skips nothing
    (every face of every leaf is measured once)."""
    p, v = np.asarray(p, F32), np.asarray(v, F32)
    n, L, order, kinds = p.shape[0], tree["L"], tree["order"], tree["kinds"]
    best, face, visits = np.full(n, np.inf, F32), np.zeros(n, np.int64), np.zeros(n, np.int64)
    pc = MF._xyz(p)

    def rec(node, idx):
        if tree["count"][node] == 0 or idx.size == 0:
            return
        visits[idx] += 1
        if prune:
            idx = idx[~(box_d2(p[idx], tree["lo"][node], tree["hi"][node]) > best[idx])]
            if idx.size == 0:
                return
        if node < L:
            rec(2 * node, idx)
            rec(2 * node + 1, idx)
            return
        sub = tuple(c[idx] for c in pc)
        for s in leaf_faces(tree, node):
            t = int(order[s])
            a, b, c = (tuple(v[f[t, k]]) for k in range(3))
            d2 = MF.pair(sub, a, b, c, int(kinds[t]), F32)[0]
            m = (d2 < best[idx]) | ((d2 == best[idx]) & (t < face[idx]))
            best[idx], face[idx] = np.where(m, d2, best[idx]), np.where(m, t, face[idx])
            visits[idx] += 1

    rec(1, np.arange(n))
    return {"dist": np.sqrt(best), "face": face, "d2": best, "visits": visits}


def walk_winding(tree, p, v, f, beta=BETA, dtype=F64):
    """Q2 -> dict(wn [n] in dtype, visits [n]).  The opening decision is the float32 one for both dtypes; the expansion and the
    exact terms are evaluated in `dtype` on the tree of that precision (a face's kind is decided in dtype, as MF.query does)."""
    p32 = np.asarray(p, F32)
    pd, vd = p32.astype(dtype), np.asarray(v, F32).astype(dtype)
    n, L, order = p32.shape[0], tree["L"], tree["order"]
    t32, td = tree["f32"], tree["f32" if dtype == F32 else "f64"]
    acc, visits = np.zeros(n, dtype), np.zeros(n, np.int64)
    pc = MF._xyz(pd)
    b32 = F32(beta)

    def rec(node, idx):
        if tree["count"][node] == 0 or idx.size == 0:
            return
        visits[idx] += 1
        x = t32["p"][node] - p32[idx]
        d2 = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
        br = b32 * t32["r"][node]
        with np.errstate(over="ignore"):
            opened = d2 <= br * br
        far = idx[~opened]
        if far.size:
            x = (td["p"][node].astype(dtype) - pd[far])
            N, Cm = td["N"][node].astype(dtype), td["C"][node].astype(dtype)
            d2 = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
            d = np.sqrt(d2)
            d3 = d2 * d
            d5 = d3 * d2
            nx = (N[0] * x[:, 0] + N[1] * x[:, 1]) + N[2] * x[:, 2]
            tr = (Cm[0, 0] + Cm[1, 1]) + Cm[2, 2]
            cx = [(Cm[i, 0] * x[:, 0] + Cm[i, 1] * x[:, 1]) + Cm[i, 2] * x[:, 2] for i in range(3)]
            xcx = (x[:, 0] * cx[0] + x[:, 1] * cx[1]) + x[:, 2] * cx[2]
            omega = (nx / d3 + tr / d3) - (dtype(3) * xcx) / d5
            acc[far] = acc[far] + dtype(0.5) * omega
        idx = idx[opened]
        if idx.size == 0:
            return
        if node < L:
            rec(2 * node, idx)
            rec(2 * node + 1, idx)
            return
        sub = tuple(c[idx] for c in pc)
        for s in leaf_faces(tree, node):
            t = int(order[s])
            a, b, c = (tuple(vd[f[t, k]]) for k in range(3))
            acc[idx] = acc[idx] + MF.pair(sub, a, b, c, MF.face_kind(a, b, c), dtype)[3]
            visits[idx] += 1

    rec(1, np.arange(n))
    return {"wn": acc * dtype(MF.INV_2PI), "visits": visits}


def query(p, v, f, attr=None, beta=BETA, dtype=F32, tree=None):
    """The whole accelerated query -> dict(dist, face, d2, wn[, attr]): dist, face and d2 are float32's whatever dtype is."""
    tree = tree or build(v, f)
    out = walk_distance(tree, p, v, f)
    out["wn"] = walk_winding(tree, p, v, f, beta, dtype)["wn"]
    if attr is not None:
        out["attr"] = MF.attr_on_face(p, v, f, attr, out["face"], F32)
    return out


def own_box_violations(p, v, f, delta):
    """The delta experiment: pairs (point, face) whose float32 d2 - the brute-force query's - lies below lb2 of the face's OWN box
    inflated by delta -> (violations, pairs)."""
    v = np.asarray(v, F32)
    d2 = MF.query(p, v, f, None, F32)["d2"]
    tri = v[f]
    lo, hi = tri.min(1) - F32(delta), tri.max(1) + F32(delta)
    bad = 0
    for t in range(f.shape[0]):
        bad += int((d2[:, t] < box_d2(np.asarray(p, F32), lo[t], hi[t])).sum())
    return bad, d2.size
