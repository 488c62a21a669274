"""numpy restatement of the mesh cleanup (csrc/meshclean.hip), written from rules R0-R8 in include/primx_hip.h: the
greedy vertex merge, duplicate / null faces, small components, non-manifold edges and vertices.  `clean` is the
sequential statement of the rules; `merge_rounds` is the round schedule the kernels run, which must give the same
centres and counts the rounds.  CPU only; shared by the CPU and GPU tests and tools/meshclean_bench.py."""
import numpy as np

F32 = np.float32
GRID_CAP = 128


def diag(p):
    """float64 diagonal of the fp32 bounding box of p [n, 3] (0 for no points): extents in float64, then
    sqrt((ex^2 + ey^2) + ez^2)."""
    if len(p) == 0:
        return 0.0
    p = np.asarray(p, dtype=F32)
    e = p.max(0).astype(np.float64) - p.min(0).astype(np.float64)
    return float(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def radius(v, f, v_pct):
    """R1: r = fp32(v_pct / 100 * D), D = the diagonal of the referenced vertices."""
    ref = np.unique(np.asarray(f, dtype=np.int64).reshape(-1))
    return F32((float(v_pct) / 100.0) * diag(np.asarray(v, dtype=F32)[ref]))


def within(d2, r):
    """R2's comparison: (dx dx + dy dy) + dz dz < r r in fp32, or exactly 0."""
    return (d2 < F32(r) * F32(r)) | (d2 == F32(0))


def _d2(a, b):
    d = (a - b).astype(F32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _cells(p, r):
    """Cell coordinates of a grid whose cells are at least r wide (any such grid serves the search)."""
    lo = p.min(0)
    ext = float((p.max(0) - lo).max())
    w = max(float(r) * 1.001, ext / (GRID_CAP - 1), 1e-30)
    return np.floor((p - lo).astype(np.float64) / w).astype(np.int64)


def merge(v, f, v_pct):
    """R0-R2, sequential: centre [V] int64 (the centre each referenced vertex joins, itself for a centre; -1 for an
    unreferenced vertex)."""
    v = np.asarray(v, dtype=F32)
    f = np.asarray(f, dtype=np.int64)
    centre = np.full(len(v), -1, dtype=np.int64)
    ref = np.unique(f.reshape(-1))
    if v_pct == 0 or len(ref) == 0:
        centre[ref] = ref
        return centre
    r = radius(v, f, v_pct)
    cell = _cells(v[ref], r)
    grid = {}
    for i, c in zip(ref.tolist(), map(tuple, cell.tolist())):
        best = -1
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    for j in grid.get((c[0] + dx, c[1] + dy, c[2] + dz), ()):
                        if (best < 0 or j < best) and within(_d2(v[i], v[j]), r):
                            best = j
        if best < 0:
            best = i
            grid.setdefault(c, []).append(i)
        centre[i] = best
    return centre


def lower_pairs(v, idx, r):
    """All pairs (i, j), j < i, of the vertices idx within r of each other: int64 [P] arrays i, j."""
    p = v[idx]
    cell = _cells(p, r)
    key = (cell[:, 0] * (GRID_CAP + 2) + cell[:, 1]) * (GRID_CAP + 2) + cell[:, 2]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    I, J = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                nk = key + (dx * (GRID_CAP + 2) + dy) * (GRID_CAP + 2) + dz
                lo = np.searchsorted(skey, nk, "left")
                hi = np.searchsorted(skey, nk, "right")
                n = hi - lo
                a = np.repeat(np.arange(len(idx)), n)
                b = order[np.repeat(lo - np.cumsum(n) + n, n) + np.arange(n.sum())]
                keep = idx[b] < idx[a]
                a, b = a[keep], b[keep]
                keep = within(_d2(p[a], p[b]), r)
                I.append(idx[a[keep]])
                J.append(idx[b[keep]])
    return np.concatenate(I), np.concatenate(J)


UNDECIDED, CENTRE, CAPTURED, FINAL = 0, 1, 2, 3


def merge_rounds(v, f, v_pct):
    """R0-R2 by the kernels' schedule -> (centre [V], rounds).  Every round reads the previous round's states: an
    undecided vertex becomes CAPTURED once a lower-index CENTRE lies within r, and is decided (CENTRE, or FINAL with
    its captor = the smallest such centre) once every lower-index vertex within r is decided.  `rounds` counts the
    rounds that changed a state.  A vertex's next state is a function of its own state and its lower neighbours', so a
    round evaluates only the open vertices with a lower neighbour that changed in the round before (all of them in the
    first round); every other vertex would get the state it has.  A large mesh then costs its pair list a few times over,
    not once per round."""
    v = np.asarray(v, dtype=F32)
    f = np.asarray(f, dtype=np.int64)
    V = len(v)
    centre = np.full(V, -1, dtype=np.int64)
    ref = np.unique(f.reshape(-1))
    if v_pct == 0 or len(ref) == 0:
        centre[ref] = ref
        return centre, 0
    r = radius(v, f, v_pct)
    I, J = lower_pairs(v, ref, r)
    o = np.argsort(I, kind="stable")                       # pairs grouped by the higher vertex ...
    I, J = I[o], J[o]
    cnt = np.bincount(I, minlength=V)
    start = np.cumsum(cnt) - cnt
    up = I[np.argsort(J, kind="stable")]                   # ... and every vertex's higher neighbours, grouped by it
    ucnt = np.bincount(J, minlength=V)
    ustart = np.cumsum(ucnt) - ucnt

    def rows(lo, n):
        return np.repeat(lo - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))

    st = np.full(V, UNDECIDED, dtype=np.int64)
    rounds = 0
    big = np.iinfo(np.int64).max
    active = ref
    while len(active):
        k = rows(start[active], cnt[active])
        i, j = I[k], J[k]
        sj = st[j]
        und = np.zeros(V, dtype=bool)
        und[i[sj == UNDECIDED]] = True
        mc = np.full(V, big, dtype=np.int64)
        m = sj == CENTRE
        np.minimum.at(mc, i[m], j[m])
        und, mc, old = und[active], mc[active], st[active]
        new = old.copy()
        new[~und & (mc == big)] = CENTRE
        new[~und & (mc != big)] = FINAL
        centre[active[~und & (mc != big)]] = mc[~und & (mc != big)]
        new[und & (mc != big) & (old == UNDECIDED)] = CAPTURED
        changed = active[new != old]
        if len(changed) == 0:
            break
        st[active] = new                                   # after every read of the round: the states are double-buffered
        rounds += 1
        nxt = np.unique(up[rows(ustart[changed], ucnt[changed])])
        active = nxt[(st[nxt] == UNDECIDED) | (st[nxt] == CAPTURED)]
    c = st == CENTRE
    centre[c] = np.nonzero(c)[0]
    return centre, rounds


def face_normal(v, f):
    """g = (v1 - v0) x (v2 - v0) in fp32 (primx_texbake_labels' formula) and |g| = sqrt((gx^2 + gy^2) + gz^2)."""
    v = np.asarray(v, dtype=F32)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F32)
    return g, np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F32)


def _edges(f):
    """[F, 3] undirected edge keys (min, max) as tuples' int64 codes, edge k = (corner k, corner k + 1)."""
    a = f
    b = np.roll(f, -1, axis=1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return lo * (np.int64(1) << 32) + hi


def edge_components(f):
    """Edge-connected components of faces f [F, 3] -> (ids [F] = rank of the smallest face, count)."""
    F = len(f)
    parent = np.arange(F)

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first = {}
    for t, keys in enumerate(_edges(f).tolist()):
        for k in keys:
            if k in first:
                a, b = root(t), root(first[k])
                if a != b:
                    parent[max(a, b)] = min(a, b)
            else:
                first[k] = t
    roots = np.array([root(t) for t in range(F)], dtype=np.int64)
    u = np.unique(roots)
    return np.searchsorted(u, roots), len(u)


def clean(v, f, v_pct=1.0, min_f=64, min_d=20, repair=True, stats=None):
    """R0-R8 -> (v' [V', 3] fp32, f' [F', 3] int64, vmap [V'] int64).  `stats` (a dict) receives the counts."""
    v = np.asarray(v, dtype=F32).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    st = {} if stats is None else stats
    # R0-R2
    centre = merge(v, f, v_pct)
    fr = centre[f] if len(f) else f
    ok = (fr[:, 0] != fr[:, 1]) & (fr[:, 1] != fr[:, 2]) & (fr[:, 0] != fr[:, 2])
    # R3: the lowest index of each vertex set
    s = np.sort(fr, 1)
    seen, dup = set(), np.zeros(len(f), dtype=bool)
    for t in np.nonzero(ok)[0]:
        k = tuple(s[t])
        dup[t] = k in seen
        seen.add(k)
    ok &= ~dup
    # R4
    g, _ = face_normal(v, fr) if len(f) else (np.zeros((0, 3), F32), None)
    ok &= ~((g[:, 0] == 0) & (g[:, 1] == 0) & (g[:, 2] == 0))
    f1 = fr[ok]
    st["faces_after_merge"] = int(ok.sum())
    # R5
    if len(f1):
        comp, nc = edge_components(f1)
        cnt = np.bincount(comp, minlength=nc)
        d2 = diag(v[np.unique(f1)])
        thr = (float(min_d) / 100.0) * d2
        drop = cnt < min_f
        for c in range(nc):
            if not drop[c] and diag(v[np.unique(f1[comp == c])]) < thr:
                drop[c] = True
        st["components"], st["components_removed"] = nc, int(drop.sum())
        f1 = f1[~drop[comp]]
    else:
        st["components"], st["components_removed"] = 0, 0
    st["nonmanifold_candidates"] = st["nonmanifold_faces_removed"] = st["vertices_split"] = 0
    newv = np.zeros(0, dtype=np.int64)
    if repair and len(f1):
        # R6
        e = _edges(f1)
        u, inv = np.unique(e.reshape(-1), return_inverse=True)
        cnt = np.bincount(inv, minlength=len(u))
        inv = inv.reshape(-1, 3)
        cand = np.nonzero((cnt[inv] > 2).any(1))[0]
        _, gn = face_normal(v, f1)
        order = cand[np.lexsort((cand, gn[cand]))]
        keep = np.ones(len(f1), dtype=bool)
        for t in order:
            if (cnt[inv[t]] > 2).any():
                keep[t] = False
                cnt[inv[t]] -= 1
        st["nonmanifold_candidates"] = len(cand)
        st["nonmanifold_faces_removed"] = int((~keep).sum())
        f1 = f1[keep]
        # R7: fans = components of the corners at each vertex joined through the directed edges (x -> y)
        n1 = len(f1)
        corner_v = f1.reshape(-1)
        parent = np.arange(3 * n1)

        def root(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        first = {}
        for c in range(3 * n1):
            t, k = divmod(c, 3)
            x = f1[t, k]
            for y in (f1[t, (k + 1) % 3], f1[t, (k + 2) % 3]):
                key = (int(x), int(y))
                if key in first:
                    a, b = root(c), root(first[key])
                    if a != b:
                        parent[max(a, b)] = min(a, b)
                else:
                    first[key] = c
        fan = np.array([root(c) for c in range(3 * n1)], dtype=np.int64)
        lowc = {}
        fans = {}
        for c in range(3 * n1):
            x = int(corner_v[c])
            lowc.setdefault(x, c)
            fans.setdefault(x, set()).add(int(fan[c]))
        split = sorted((lowc[x], x) for x in fans if len(fans[x]) > 1)
        st["vertices_split"] = len(split)
        out = f1.reshape(-1).copy()
        for n, (c0, x) in enumerate(split):
            sel = (corner_v == x) & (fan == fan[c0])
            out[sel] = len(v) + n          # provisional index, remapped below
        f1 = out.reshape(-1, 3)
        newv = np.array([x for _, x in split], dtype=np.int64)
    # R8
    used = np.unique(f1.reshape(-1))
    kept = used[used < len(v)]
    vmap = np.concatenate([kept, newv]).astype(np.int64)
    remap = np.full(len(v) + len(newv), -1, dtype=np.int64)
    remap[kept] = np.arange(len(kept))
    remap[len(v) + np.arange(len(newv))] = len(kept) + np.arange(len(newv))
    fo = remap[f1] if len(f1) else np.zeros((0, 3), dtype=np.int64)
    return v[vmap], fo.reshape(-1, 3), vmap


def check_invariants(v, f, min_f=0, repaired=True):
    """The properties of every output (R8): no unreferenced vertex, no repeated index, no duplicate or zero-area face;
    with repair no edge with more than 2 faces, without it every component at or above min_f faces (R6 can split a
    component afterwards)."""
    v = np.asarray(v, dtype=F32)
    f = np.asarray(f, dtype=np.int64)
    if len(f) == 0:
        assert len(v) == 0
        return
    assert np.array_equal(np.unique(f), np.arange(len(v))), "unreferenced vertex"
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all(), "repeated index"
    s = np.sort(f, 1)
    assert len(np.unique(s, axis=0)) == len(f), "duplicate face"
    g, _ = face_normal(v, f)
    assert not ((g[:, 0] == 0) & (g[:, 1] == 0) & (g[:, 2] == 0)).any(), "zero-area face"
    if repaired:
        _, cnt = np.unique(_edges(f).reshape(-1), return_counts=True)
        assert cnt.max() <= 2, "non-manifold edge"
    else:
        comp, nc = edge_components(f)
        assert np.bincount(comp, minlength=nc).min() >= min_f, "small component"
