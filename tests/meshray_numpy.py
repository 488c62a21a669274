"""Numpy restatement of the mesh ray query (include/primx_hip.h "Mesh rays" R1-R6, csrc/meshray_pair.h, the ray kernels of
csrc/meshbvh.hip, fit.MeshBVH.raycast / .visibility): the watertight ray / triangle test of Woop, Benthin and Wald 2013, the box
test that is conservative with respect to it, the brute force over all faces, the walk through tests/meshbvh_numpy.py's tree, and
the visibility count.

`dtype=np.float32` is the bit-exact model of the kernels: the same expressions, every operation rounded to float32 in the order
the header gives (the edge functions recomputed in float64 where one of them is 0, as R2 says).  `dtype=np.float64` evaluates the
same rules on the same float32 inputs in float64: the reference the float32 restatement is held against away from the edges.
The walk visits the left child first where the kernel takes the nearer one: R4 and R5 make the result independent of the order.
"""
from __future__ import annotations

import numpy as np

from tests import meshbvh_numpy as MB
from tests import meshfield_numpy as MF

F32, F64 = np.float32, np.float64
T_MARGIN = 2.0 ** -20        # RAY_T_MARGIN of csrc/meshray_pair.h


# ------------------------------------------------------------------------------------------------------------ fixtures
def flipped(level=3, seed=7):
    """icosphere(level) with a seeded half of its faces reversed (b and c exchanged): the same surface, no consistent orientation.
    -> (v, f flipped, f as it was)."""
    v, f = MF.icosphere(level)
    pick = np.random.default_rng(seed).permutation(f.shape[0])[:f.shape[0] // 2]
    g = f.copy()
    g[pick] = f[pick][:, [0, 2, 1]]
    return v, np.ascontiguousarray(g), f


def exact_box():
    """A box whose corners, centre and edge midpoints are dyadic: rays from the centre pass EXACTLY through corners and edges."""
    return MF.box(lo=(-0.5, -0.25, -0.75), hi=(0.5, 0.75, 0.25)) + (np.array([0.0, 0.25, -0.25], F32),)


def edges_of(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0)


def interior_rays(v, f, centre=None, n_random=200, seed=0):
    """Rays from strictly interior points of a closed mesh about its bounding box's centre: the centre itself and two points
    a twentieth of the extent away; per origin n_random seeded directions, the directions to every referenced vertex and to every
    edge's midpoint (float32 differences, as a caller would form them).  -> (origins [n, 3], dirs [n, 3]) float32."""
    v = np.asarray(v, F32)
    lo, hi = v[np.unique(f)].min(0), v[np.unique(f)].max(0)
    c = ((lo + hi) * F32(0.5)).astype(F32) if centre is None else np.asarray(centre, F32)
    ext = F32((hi - lo).max())
    rng = np.random.default_rng(seed)
    e = edges_of(f)
    targets = np.concatenate([v[np.unique(f)], ((v[e[:, 0]] + v[e[:, 1]]) * F32(0.5)).astype(F32)])
    org, dirs = [], []
    for off in ((0, 0, 0), (0.05, -0.03, 0.02), (-0.02, 0.04, -0.05)):
        o = (c + np.asarray(off, F32) * ext).astype(F32)
        r = rng.standard_normal((n_random, 3)).astype(F32)
        d = np.concatenate([r, (targets - o).astype(F32)])
        d = d[np.abs(d).max(1) > 0]
        org.append(np.broadcast_to(o, d.shape)), dirs.append(d)
    return np.ascontiguousarray(np.concatenate(org)), np.ascontiguousarray(np.concatenate(dirs))


def ray_set(v, f, n=1000, seed=0, far=1.0):
    """n seeded rays, a fifth each and shuffled so that every prefix has of each kind: random rays through the bounding box; rays
    from outside aimed at vertices; rays aimed at edge midpoints; axis-parallel rays (through vertices' coordinates: they lie in
    the planes of axis-aligned faces); rays starting on the surface.  `far`: the distance of the outside origins in extents."""
    v = np.asarray(v, F32)
    used = np.unique(f)
    lo, hi = v[used].min(0).astype(F64), v[used].max(0).astype(F64)
    c, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-30)
    rng = np.random.default_rng(seed)
    k = n // 5
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)   # noqa: E731
    # 1. through the box
    p0, p1 = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (k, 3)), rng.uniform(lo, hi, (k, 3))
    o1, d1 = p0, p1 - p0
    # 2. from outside at vertices
    o2 = c + unit(rng.standard_normal((k, 3))) * ext * (0.9 + far)
    t2 = v[used[rng.integers(0, len(used), k)]].astype(F64)
    d2 = (t2.astype(F32) - o2.astype(F32)).astype(F64)
    # 3. at edge midpoints
    e = edges_of(f)
    pick = e[rng.integers(0, len(e), k)]
    o3 = c + unit(rng.standard_normal((k, 3))) * ext * (0.9 + far)
    mid = ((v[pick[:, 0]] + v[pick[:, 1]]) * F32(0.5)).astype(F32)
    d3 = (mid - o3.astype(F32)).astype(F64)
    # 4. axis-parallel, through a vertex's other two coordinates
    ax = rng.integers(0, 3, k)
    t4 = v[used[rng.integers(0, len(used), k)]].astype(F64)
    sign = rng.choice([-1.0, 1.0], k)
    d4 = np.zeros((k, 3))
    d4[np.arange(k), ax] = sign
    o4 = t4.copy()
    o4[np.arange(k), ax] = c[ax] - sign * ext * (0.9 + far)
    # 5. from the surface
    cdf = np.cumsum(MF.face_areas(v, f))
    m = n - 4 * k
    if cdf[-1] > 0:
        o5 = MF.surface_points(v, f, cdf, rng.random((m, 3)).astype(F32))[0].astype(F64)
    else:
        o5 = np.broadcast_to(c, (m, 3)).copy()
    d5 = rng.standard_normal((m, 3))
    o = np.concatenate([o1, o2, o3, o4, o5]).astype(F32)
    d = np.concatenate([d1, d2, d3, d4, d5]).astype(F32)
    perm = rng.permutation(n)
    return np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm])


def grazing_rays(tree, scale=1.0, seed=0, nodes=24):
    """The margin experiment's rays: for `nodes` seeded live nodes of the tree, rays that graze the node's box - through two of
    its corners, through a corner along each axis (axis-parallel rays lying in its face planes), along its edges, and through a
    corner and a face centre - from origins `scale` extents of the mesh away.  -> (origins, dirs) float32."""
    rng = np.random.default_rng(seed)
    live = np.flatnonzero(tree["count"] > 0)
    live = live[live >= 1]
    pick = live if len(live) <= nodes else np.concatenate([[1], rng.choice(live[1:], nodes - 1, replace=False)])
    root_lo, root_hi = tree["lo"][1].astype(F64), tree["hi"][1].astype(F64)
    ext = max(float((root_hi - root_lo).max()), 1e-30)
    org, dirs = [], []
    for i in pick:
        lo, hi = tree["lo"][i].astype(F64), tree["hi"][i].astype(F64)
        corners = np.array([[(hi if (b >> k) & 1 else lo)[k] for k in range(3)] for b in range(8)])
        centres = np.array([np.where(np.arange(3) == k, (lo, hi)[s][k], (lo + hi) / 2) for k in range(3) for s in range(2)])
        for a in range(8):
            for k in range(3):                                   # axis-parallel, in two face planes at once
                for s in (-1.0, 1.0):
                    d = np.zeros(3)
                    d[k] = s
                    o = corners[a].copy()
                    o[k] = (lo[k] + hi[k]) / 2 - s * ext * scale
                    org.append(o), dirs.append(d)
            for b in range(a + 1, 8):                            # through two corners: an edge or a diagonal
                d = corners[b] - corners[a]
                if np.abs(d).max() > 0:
                    org.append(corners[a] - d / np.abs(d).max() * ext * scale), dirs.append(d)
            c = centres[rng.integers(0, 6)]                      # through a corner and a face centre
            d = c - corners[a]
            if np.abs(d).max() > 0:
                org.append(corners[a] - d / np.abs(d).max() * ext * scale), dirs.append(d)
    return np.ascontiguousarray(np.asarray(org, F32)), np.ascontiguousarray(np.asarray(dirs, F32))


# ------------------------------------------------------------------------------------------------------------ R1: the ray
def setup(o, d, dtype=F32):
    """R1 -> dict(kx, ky, kz [n] int, o [n, 3] permuted, s [n, 3] = (sx, sy, sz), ok [n])."""
    o32, d32 = np.asarray(o, F32), np.asarray(d, F32)
    o, d = o32.astype(dtype), d32.astype(dtype)
    n = o.shape[0]
    a = np.abs(d)
    with np.errstate(invalid="ignore"):
        kz = np.zeros(n, np.int64)
        kz[a[:, 1] > a[:, 0]] = 1
        kz[a[:, 2] > np.fmax(a[:, 0], a[:, 1])] = 2
    kx = np.where(kz == 2, 0, kz + 1)
    ky = np.where(kx == 2, 0, kx + 1)
    r = np.arange(n)
    dk = d[r, kz]
    with np.errstate(invalid="ignore"):
        swap = dk < 0
    kx, ky = np.where(swap, ky, kx), np.where(swap, kx, ky)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.stack([d[r, kx] / dk, d[r, ky] / dk, dtype(1) / dk], 1).astype(dtype)
    ok = np.isfinite(o32).all(1) & np.isfinite(d32).all(1) & np.isfinite(s[:, 2])
    return {"kx": kx, "ky": ky, "kz": kz, "o": np.stack([o[r, kx], o[r, ky], o[r, kz]], 1), "s": s, "ok": ok, "n": n}


# ------------------------------------------------------------------------------------------------------------ R2, R3: a pair
def pairs(ray, a, b, c, kinds, tmin, tmax, dtype=F32):
    """Rays [n] against faces [k] (corners a, b, c [k, 3] float32, kinds [k]) -> (accepted, t, v, w), each [n, k]."""
    a, b, c = (np.asarray(x, F32).astype(dtype) for x in (a, b, c))
    kx, ky, kz = ray["kx"], ray["ky"], ray["kz"]
    ox, oy, oz = (ray["o"][:, k:k + 1] for k in range(3))
    sx, sy, sz = (ray["s"][:, k:k + 1] for k in range(3))
    tmin, tmax = dtype(tmin), dtype(tmax)
    with np.errstate(all="ignore"):
        az, bz, cz = a.T[kz] - oz, b.T[kz] - oz, c.T[kz] - oz
        ax, ay = (a.T[kx] - ox) - sx * az, (a.T[ky] - oy) - sy * az
        bx, by = (b.T[kx] - ox) - sx * bz, (b.T[ky] - oy) - sy * bz
        cx, cy = (c.T[kx] - ox) - sx * cz, (c.T[ky] - oy) - sy * cz
        U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
        neg, pos = (U < 0) | (V < 0) | (W < 0), (U > 0) | (V > 0) | (W > 0)
        zero = (U == 0) | (V == 0) | (W == 0)
        if zero.any():
            D = lambda x: x.astype(F64)   # noqa: E731
            Ud, Vd, Wd = D(cx) * D(by) - D(cy) * D(bx), D(ax) * D(cy) - D(ay) * D(cx), D(bx) * D(ay) - D(by) * D(ax)
            neg = np.where(zero, (Ud < 0) | (Vd < 0) | (Wd < 0), neg)
            pos = np.where(zero, (Ud > 0) | (Vd > 0) | (Wd > 0), pos)
            U, V, W = (np.where(zero, x.astype(dtype), y) for x, y in ((Ud, U), (Vd, V), (Wd, W)))
        det = (U + V) + W
        T = (U * (sz * az) + V * (sz * bz)) + W * (sz * cz)
        t, v, w = T / det, V / det, W / det
        ok = ~(neg & pos) & (det != 0) & (np.abs(det) < np.inf) & (tmin <= t) & (t <= tmax)
    ok &= (np.asarray(kinds) == 0)[None, :] & ray["ok"][:, None]
    return ok, t.astype(dtype), v.astype(dtype), w.astype(dtype)


def edge_functions(o, d, v, f):
    """The float64 edge functions of every (ray, face) -> min(|U|, |V|, |W|) / s^2 [n, F], s = the largest |P[k] - o[k]| of the
    face's corners: how far, in units of the fp32 error of an edge function (about 14 x 2^-24 s^2: three roundings per sheared
    coordinate, two products and a difference), a ray passes from every edge of a face.  For "away from 0"."""
    ray = setup(o, d, F64)
    a, b, c = (np.asarray(v, F32)[f[:, k]].astype(F64) for k in range(3))
    kx, ky, kz = ray["kx"], ray["ky"], ray["kz"]
    ox, oy, oz = (ray["o"][:, k:k + 1] for k in range(3))
    sx, sy = ray["s"][:, 0:1], ray["s"][:, 1:2]
    with np.errstate(all="ignore"):
        P = []
        for q in (a, b, c):
            z = q.T[kz] - oz
            P.append(((q.T[kx] - ox) - sx * z, (q.T[ky] - oy) - sy * z))
        (ax, ay), (bx, by), (cx, cy) = P
        U, V, W = cx * by - cy * bx, ax * cy - ay * cx, bx * ay - by * ax
        scale = np.maximum.reduce([np.abs(q.T[k] - o_) for q in (a, b, c) for k, o_ in ((kx, ox), (ky, oy), (kz, oz))]) ** 2
        return np.minimum.reduce([np.abs(U), np.abs(V), np.abs(W)]) / np.maximum(scale, 1e-300)


# ------------------------------------------------------------------------------------------------------------ R4: brute force
def _take(best, cand_ok, t, v, w, faces):
    """One block of candidates [n, k] with face indices `faces` [k] into the running (t, face) minimum."""
    bt, bf, bv, bw = best
    tm = np.where(cand_ok, t, np.inf)
    j = np.argmax(cand_ok & (tm == tm.min(1, keepdims=True)), axis=1)          # the first accepted one of the smallest t
    r = np.arange(t.shape[0])
    has, ct, cf = cand_ok[r, j], t[r, j], faces[j]
    m = has & ((bf < 0) | (ct < bt) | ((ct == bt) & (cf < bf)))
    return np.where(m, ct, bt), np.where(m, cf, bf), np.where(m, v[r, j], bv), np.where(m, w[r, j], bw)


def brute(o, d, v, f, tmin=0.0, tmax=np.inf, dtype=F32, block=64, kinds=None):
    """Every face against every ray -> dict(t [n] (inf on a miss), face [n] (-1), bary [n, 2] (0, 0), hit [n])."""
    v = np.asarray(v, F32)
    kinds = MB.face_kinds(v, f) if kinds is None else kinds
    ray = setup(o, d, dtype)
    n = ray["n"]
    best = (np.full(n, dtype(tmax), dtype), np.full(n, -1, np.int64), np.zeros(n, dtype), np.zeros(n, dtype))
    for lo in range(0, f.shape[0], block):
        fb = f[lo:lo + block]
        ok, t, vv, ww = pairs(ray, v[fb[:, 0]], v[fb[:, 1]], v[fb[:, 2]], kinds[lo:lo + block], tmin, tmax, dtype)
        best = _take(best, ok, t, vv, ww, np.arange(lo, lo + fb.shape[0]))
    bt, bf, bv, bw = best
    hit = bf >= 0
    return {"t": np.where(hit, bt, dtype(np.inf)).astype(dtype), "face": bf, "bary": np.stack([bv, bw], 1).astype(dtype), "hit": hit}


# ------------------------------------------------------------------------------------------------------------ R5: the box, the walk
def box_test(ray, idx, lo, hi, tmin, best, dtype=F32, margin=T_MARGIN):
    """R5 for the rays idx against one box -> (kept [m], tn [m])."""
    lo, hi = lo.astype(dtype), hi.astype(dtype)
    kx, ky, kz = ray["kx"][idx], ray["ky"][idx], ray["kz"][idx]
    o, s = ray["o"][idx], ray["s"][idx]
    with np.errstate(all="ignore"):
        z0, z1 = lo[kz] - o[:, 2], hi[kz] - o[:, 2]
        x0, x1 = lo[kx] - o[:, 0], hi[kx] - o[:, 0]
        y0, y1 = lo[ky] - o[:, 1], hi[ky] - o[:, 1]
        mx0, mx1 = np.fmin(s[:, 0] * z0, s[:, 0] * z1), np.fmax(s[:, 0] * z0, s[:, 0] * z1)
        my0, my1 = np.fmin(s[:, 1] * z0, s[:, 1] * z1), np.fmax(s[:, 1] * z0, s[:, 1] * z1)
        zl, zh = np.fmin(s[:, 2] * z0, s[:, 2] * z1), np.fmax(s[:, 2] * z0, s[:, 2] * z1)
        m = np.fmax(np.abs(zl), np.abs(zh)) * dtype(margin)
        tn, tf = zl - m, zh + m
        keep = ~(x0 - mx1 > 0) & ~(x1 - mx0 < 0) & ~(y0 - my1 > 0) & ~(y1 - my0 < 0) & ~(tn > best) & ~(tf < dtype(tmin))
    return keep, tn


def walk(tree, o, d, v, f, tmin=0.0, tmax=np.inf, dtype=F32, prune=True, margin=T_MARGIN):
    """The closest hit through the tree -> brute's dict plus 'visits' [n] (nodes arrived at + faces tested)."""
    v = np.asarray(v, F32)
    ray = setup(o, d, dtype)
    n, L, order, kinds = ray["n"], tree["L"], tree["order"], tree["kinds"]
    state = [np.full(n, dtype(tmax), dtype), np.full(n, -1, np.int64), np.zeros(n, dtype), np.zeros(n, dtype)]
    visits = np.zeros(n, np.int64)

    def rec(node, idx):
        if tree["count"][node] == 0 or idx.size == 0:
            return
        visits[idx] += 1
        if prune:
            idx = idx[box_test(ray, idx, tree["lo"][node], tree["hi"][node], tmin, state[0][idx], dtype, margin)[0]]
            if idx.size == 0:
                return
        if node < L:
            rec(2 * node, idx)
            rec(2 * node + 1, idx)
            return
        s = np.asarray(list(MB.leaf_faces(tree, node)))
        faces = order[s]
        sub = {k: (a[idx] if isinstance(a, np.ndarray) else a) for k, a in ray.items()}
        ok, t, vv, ww = pairs(sub, v[f[faces, 0]], v[f[faces, 1]], v[f[faces, 2]], kinds[faces], tmin, tmax, dtype)
        for j in range(len(faces)):                              # one by one: the sorted order is not the face order
            new = _take(tuple(a[idx] for a in state), ok[:, j:j + 1], t[:, j:j + 1], vv[:, j:j + 1], ww[:, j:j + 1], faces[j:j + 1])
            for a, b in zip(state, new):
                a[idx] = b
        visits[idx] += len(faces)

    rec(1, np.flatnonzero(ray["ok"]))
    bt, bf, bv, bw = state
    hit = bf >= 0
    return {"t": np.where(hit, bt, dtype(np.inf)).astype(dtype), "face": bf, "bary": np.stack([bv, bw], 1).astype(dtype), "hit": hit,
            "visits": visits}


def own_box_violations(o, d, v, f, delta, tmin=0.0, tmax=np.inf, margin=T_MARGIN):
    """The margin experiment: accepted (ray, face) pairs of the float32 brute force that R5 refuses for the face's OWN box inflated
    by delta, at best = the accepted t itself -> (violations, accepted pairs)."""
    v = np.asarray(v, F32)
    ray = setup(o, d, F32)
    kinds = MB.face_kinds(v, f)
    tri = v[f]
    lo, hi = tri.min(1) - F32(delta), tri.max(1) + F32(delta)
    bad = total = 0
    for t_ in range(f.shape[0]):
        ok, t, _, _ = pairs(ray, tri[t_:t_ + 1, 0], tri[t_:t_ + 1, 1], tri[t_:t_ + 1, 2], kinds[t_:t_ + 1], tmin, tmax, F32)
        idx = np.flatnonzero(ok[:, 0])
        if idx.size:
            keep, _ = box_test(ray, idx, lo[t_], hi[t_], tmin, t[idx, 0], F32, margin)
            bad += int((~keep).sum())
            total += idx.size
    return bad, total


# ------------------------------------------------------------------------------------------------------------ R6: visibility
def fibonacci(K):
    """mesh.occlusion_directions(K) as numpy (the one formula, imported)."""
    from topia_xl_amd import mesh
    return mesh.occlusion_directions(K).numpy()


def escapes(p, dirs, v, f, tmin=0.0, limit=0, dtype=F32):
    """int32 [n]: how many of the rays p + t dirs[k], t in [tmin, inf], are accepted by no face; with limit > 0 the count stops there."""
    p, dirs = np.asarray(p, F32), np.asarray(dirs, F32)
    kinds = MB.face_kinds(np.asarray(v, F32), f)
    esc = np.zeros(p.shape[0], np.int32)
    for k in range(dirs.shape[0]):
        live = np.flatnonzero(esc < limit) if limit > 0 else np.arange(p.shape[0])      # a saturated point casts no more rays
        if live.size == 0:
            break
        hit = brute(p[live], np.broadcast_to(dirs[k], (live.size, 3)), v, f, tmin, np.inf, dtype, kinds=kinds)["hit"]
        esc[live] += ~hit
    return esc


def attr_at(attr, f, face, bary, dtype=F32):
    """MeshBVH.raycast's out_attr: (a u + b v) + c w with u = (1 - v) - w on the hit face, 0 on a miss."""
    attr, bary = np.asarray(attr).astype(dtype), np.asarray(bary).astype(dtype)
    hit = face >= 0
    fa = f[np.where(hit, face, 0)]
    v, w = bary[:, 0:1], bary[:, 1:2]
    u = (dtype(1) - v) - w
    out = (attr[fa[:, 0]] * u + attr[fa[:, 1]] * v) + attr[fa[:, 2]] * w
    return np.where(hit[:, None], out, dtype(0)).astype(dtype)
