"""numpy restatement of the mesh decimation (csrc/meshdecim.hip), written from rules D0-D10 in include/primx_hip.h:
quadric edge collapse in rounds of pairwise independent edges, float64, every sum in the order the rules give.
`decimate` is what the kernels must reproduce bit for bit; `greedy` applies the same D1-D4, D6, D9 one collapse at a time,
always the smallest valid key (the sequential algorithm the rounds stand in for); `check_invariants` and `topology` hold
the consequences the header states.  CPU only; shared by the CPU and GPU tests."""
import numpy as np

F64 = np.float64
FACTOR = 4                       # D5: candidates among the FACTOR * need smallest keys
KEY_NONE = np.iinfo(np.int64).max


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def face_g(p0, p1, p2):
    return cross(p1 - p0, p2 - p0)


def plane_quadric(n, d, w=None):
    """[m, 10] coefficients (a00, a01, a02, a11, a12, a22, q0, q1, q2, c) of the planes (n, d); with w each is (x y) w."""
    c = np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1], n[:, 1] * n[:, 2],
                  n[:, 2] * n[:, 2], n[:, 0] * d, n[:, 1] * d, n[:, 2] * d, d * d], 1)
    return c if w is None else c * w[:, None]


def live_faces(f):
    """D0: the faces that repeat no index."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    return f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]


def edge_table(f, V):
    """D2: (ukeys [U] = sorted unique lo V + hi, node [F, 3] = the id of edge k (corners k, k + 1), ecnt [U])."""
    a, b = f, np.roll(f, -1, axis=1)
    keys = np.minimum(a, b) * np.int64(V) + np.maximum(a, b)
    uk, inv = np.unique(keys.reshape(-1), return_inverse=True)
    return uk, inv.reshape(-1, 3), np.bincount(inv.reshape(-1), minlength=len(uk))


def classes(f, node, ecnt, V):
    """D2: (boundary [V], locked [V])."""
    boundary, locked = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
    for k in range(3):
        for flag, arr in ((ecnt[node[:, k]] == 1, boundary), (ecnt[node[:, k]] > 2, locked)):
            arr[f[flag, k]] = True
            arr[f[flag, (k + 1) % 3]] = True
    return boundary, locked


def quadrics(v, f):
    """D0, D1 -> (p [V, 3], Q [V, 10]) float64.  np.add.at adds in element order, which is arranged to be D1's."""
    p = np.asarray(v, dtype=np.float32).reshape(-1, 3).astype(F64)
    V, F = len(p), len(f)
    Q = np.zeros((V, 10), dtype=F64)
    if F == 0:
        return p, Q
    _, node, ecnt = edge_table(f, V)
    q = p[f]                                                         # [F, 3, 3]
    g = face_g(q[:, 0], q[:, 1], q[:, 2])
    # per face 9 slots: the face quadric at corners 0, 1, 2, then edge k at corners (k, k + 1) for k = 0, 1, 2
    idx = np.full((F, 9), -1, dtype=np.int64)
    con = np.zeros((F, 9, 10), dtype=F64)
    fq = plane_quadric(g, -dot(g, q[:, 0]))
    for k in range(3):
        idx[:, k] = f[:, k]
        con[:, k] = fq
    with np.errstate(all="ignore"):
        for k in range(3):
            kn = (k + 1) % 3
            e = q[:, kn] - q[:, k]
            l2 = dot(e, e)
            on = (ecnt[node[:, k]] == 1) & (l2 != 0.0)
            m = cross(e, g)
            bq = plane_quadric(m, -dot(m, q[:, k]), 1.0 / l2)
            for s, kk in enumerate((k, kn)):
                idx[on, 3 + 2 * k + s] = f[on, kk]
                con[on, 3 + 2 * k + s] = bq[on]
    idx, con = idx.reshape(-1), con.reshape(-1, 10)
    use = idx >= 0
    np.add.at(Q, idx[use], con[use])
    return p, Q


def quadric_cost(q, y):
    a0 = (q[:, 0] * y[:, 0] + q[:, 1] * y[:, 1]) + q[:, 2] * y[:, 2]
    a1 = (q[:, 1] * y[:, 0] + q[:, 3] * y[:, 1]) + q[:, 4] * y[:, 2]
    a2 = (q[:, 2] * y[:, 0] + q[:, 4] * y[:, 1]) + q[:, 5] * y[:, 2]
    yAy = (y[:, 0] * a0 + y[:, 1] * a1) + y[:, 2] * a2
    qy = (q[:, 6] * y[:, 0] + q[:, 7] * y[:, 1]) + q[:, 8] * y[:, 2]
    c = (yAy + 2.0 * qy) + q[:, 9]
    return np.where(c > 0.0, c, 0.0)


def placement(p, Q, a, b, optimalplacement=True):
    """D3 for the edges (a, b) -> (x [n, 3], cost [n])."""
    q = Q[a] + Q[b]
    pa, pb = p[a], p[b]
    mid = (pa + pb) * 0.5
    with np.errstate(all="ignore"):
        c00, c01, c02 = q[:, 3] * q[:, 5] - q[:, 4] * q[:, 4], q[:, 2] * q[:, 4] - q[:, 1] * q[:, 5], \
            q[:, 1] * q[:, 4] - q[:, 2] * q[:, 3]
        c11, c12, c22 = q[:, 0] * q[:, 5] - q[:, 2] * q[:, 2], q[:, 1] * q[:, 2] - q[:, 0] * q[:, 4], \
            q[:, 0] * q[:, 3] - q[:, 1] * q[:, 1]
        det = (q[:, 0] * c00 + q[:, 1] * c01) + q[:, 2] * c02
        t3 = ((q[:, 0] + q[:, 3]) + q[:, 5]) / 3.0
        thr = 1e-9 * ((t3 * t3) * t3)
        xo = np.stack([-((c00 * q[:, 6] + c01 * q[:, 7]) + c02 * q[:, 8]) / det,
                       -((c01 * q[:, 6] + c11 * q[:, 7]) + c12 * q[:, 8]) / det,
                       -((c02 * q[:, 6] + c12 * q[:, 7]) + c22 * q[:, 8]) / det], 1)
        use = (np.abs(det) > thr) & (dot(xo - mid, xo - mid) <= 4.0 * dot(pa - pb, pa - pb))
        if not optimalplacement:
            use[:] = False
        xo = np.where(use[:, None], xo, 0.0)
        co = quadric_cost(q, xo)
        ca, cb, cm = quadric_cost(q, pa), quadric_cost(q, pb), quadric_cost(q, mid)
    cx, x = ca.copy(), pa.copy()
    m = cb < cx
    cx[m], x[m] = cb[m], pb[m]
    m = cm < cx
    cx[m], x[m] = cm[m], mid[m]
    return np.where(use[:, None], xo, x), np.where(use, co, cx)


def costs(p, Q, uk, ecnt, boundary, locked, optimalplacement=True):
    """D3, D4 -> (x [U, 3], cost [U], key [U] int64, valid [U] bool)."""
    V = len(p)
    a, b = uk // V, uk % V
    x, cx = placement(p, Q, a, b, optimalplacement)
    key = ((cx.view(np.int64) >> 32) << 32) | np.arange(len(uk), dtype=np.int64)
    pinch = (ecnt == 2) & boundary[a] & boundary[b]
    valid = ~(locked[a] | locked[b]) & ~pinch & (ecnt >= 1) & (ecnt <= 2)
    return x, cx, key, valid


class Fans:
    """The corners sorted stably by vertex: the faces of vertex u are order[first[u]:last[u]] // 3 in ascending order."""

    def __init__(self, f, V):
        flat = f.reshape(-1)
        self.order = np.argsort(flat, kind="stable")
        sv = flat[self.order]
        self.first = np.searchsorted(sv, np.arange(V), "left")
        self.last = np.searchsorted(sv, np.arange(V), "right")

    def expand(self, u):
        """-> (r, c): for every row r of u, the corners c of vertex u[r]."""
        n = self.last[u] - self.first[u]
        r = np.repeat(np.arange(len(u)), n)
        off = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
        return r, self.order[self.first[u][r] + off]


def validate(p, f, node, uk, ecnt, fans, a, b, e, x):
    """D6 for the edges e = (a, b) with placements x -> ok [n] bool."""
    V, U, n = len(p), len(uk), len(a)
    ok = np.ones(n, dtype=bool)
    opp, nbr = [], None
    for u, other in ((a, b), (b, a)):
        r, c = fans.expand(u)
        t, k = c // 3, c % 3
        w1, w2 = f[t, (k + 1) % 3], f[t, (k + 2) % 3]
        shared = (w1 == other[r]) | (w2 == other[r])
        rr, tt, kk = r[~shared], t[~shared], k[~shared]
        q = p[f[tt]]
        n0 = face_g(q[:, 0], q[:, 1], q[:, 2])
        q[np.arange(len(tt)), kk] = x[rr]
        n1 = face_g(q[:, 0], q[:, 1], q[:, 2])
        ok[rr[~(dot(n0, n1) > 0.0)]] = False
        opp.append(rr * np.int64(U) + node[tt, (kk + 1) % 3])
        if nbr is None:                                              # the neighbours of a, each once
            rw = np.concatenate([r, r])
            w = np.concatenate([w1, w2])
            keep = w != other[rw]
            nbr = np.unique(rw[keep] * np.int64(V) + w[keep])
    ok[(opp[0][np.isin(opp[0], opp[1])] // U)] = False
    r, w = nbr // V, nbr % V
    adj = np.isin(np.minimum(w, b[r]) * np.int64(V) + np.maximum(w, b[r]), uk)
    common = np.bincount(r[adj], minlength=n)
    ok &= common == ecnt[e]
    return ok


def fan_min(f, fans, m1, u):
    """D7's m2 at the vertices u."""
    r, c = fans.expand(u)
    out = m1[u].copy()
    np.minimum.at(out, r, m1[f[c // 3]].min(1))
    return out


def decimate(v, f, target, optimalplacement=True, stats=None, trace=None):
    """D0-D10 -> (v' [V', 3] fp32, f' [F', 3] int64, vmap [V'] int64).  `stats` receives rounds, collapses, faces_before,
    faces_after, stalled and round_collapses; `trace` (a dict) receives Q0 and per round the edge table, placements,
    costs, keys, validity and selection."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    f_in = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    f = live_faces(f_in)
    V, target = len(v), int(target)
    st = {} if stats is None else stats
    st.update(rounds=0, collapses=0, faces_before=len(f_in), faces_after=len(f), stalled=False, round_collapses=[])
    p, Q = quadrics(v, f)
    if trace is not None:
        trace.update(p0=p.copy(), Q0=Q.copy(), rounds=[])
    while len(f) > target:
        F = len(f)
        uk, node, ecnt = edge_table(f, V)
        boundary, locked = classes(f, node, ecnt, V)
        x, cost, key, valid = costs(p, Q, uk, ecnt, boundary, locked, optimalplacement)
        need = -(-(F - target) // 2)
        cand = np.sort(key)[:min(len(uk), FACTOR * need)]
        e = cand & 0xffffffff
        a, b = uk[e] // V, uk[e] % V
        fans = Fans(f, V)
        ok = valid[e].copy()
        ok[ok] = validate(p, f, node, uk, ecnt, fans, a[ok], b[ok], e[ok], x[e[ok]])
        m1 = np.full(V, KEY_NONE, dtype=np.int64)
        np.minimum.at(m1, a[ok], cand[ok])
        np.minimum.at(m1, b[ok], cand[ok])
        sel = np.zeros(len(cand), dtype=bool)
        sel[ok] = (fan_min(f, fans, m1, a[ok]) == cand[ok]) & (fan_min(f, fans, m1, b[ok]) == cand[ok])
        # independence: no two selected edges share a vertex or have adjacent endpoints
        owner = np.full(V, -1, dtype=np.int64)
        ends = np.concatenate([a[sel], b[sel]])
        assert len(np.unique(ends)) == len(ends), "two collapses of a round share a vertex"
        owner[a[sel]] = owner[b[sel]] = np.nonzero(sel)[0]
        oa, ob = owner[uk // V], owner[uk % V]
        assert not ((oa >= 0) & (ob >= 0) & (oa != ob)).any(), "two collapses of a round have adjacent endpoints"
        w = np.where(sel, ecnt[e], 0)
        go = sel & (F - (np.cumsum(w) - w) > target)
        if trace is not None:
            trace["rounds"].append(dict(ukeys=uk, ecnt=ecnt, x=x, cost=cost, key=key, valid=valid, cand=cand, ok=ok, sel=sel,
                                        go=go))
        if not go.any():
            st["stalled"] = True
            break
        ga, gb, ge = a[go], b[go], e[go]
        p[ga] = x[ge]
        Q[ga] = Q[ga] + Q[gb]
        remap = np.arange(V)
        remap[gb] = ga
        f = live_faces(remap[f])
        st["rounds"] += 1
        st["collapses"] += int(go.sum())
        st["round_collapses"].append(int(go.sum()))
    st["faces_after"] = len(f)
    used = np.unique(f.reshape(-1))
    remap = np.full(V, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    return p[used].astype(np.float32), remap[f].reshape(-1, 3), used.astype(np.int64)


def greedy(v, f, target, optimalplacement=True, stats=None):
    """The sequential algorithm: D1-D4, D6, D9 one collapse at a time, always the smallest key that is valid over all
    edges.  Edge data are re-derived only where a collapse changed them: the edges with an endpoint within one ring of
    the kept vertex (their quadric sums, classes, fans or positions changed); every other edge keeps its cost and
    validity.  Keys carry (cost bits, lo, hi) instead of a dense edge id.  -> (v', f', vmap)."""
    import heapq
    v = np.asarray(v, dtype=np.float32).reshape(-1, 3)
    f = live_faces(f)
    V, target = len(v), int(target)
    p, Q = quadrics(v, f)
    faces = {t: tuple(int(i) for i in row) for t, row in enumerate(f)}
    vf = {}
    for t, row in faces.items():
        for i in row:
            vf.setdefault(i, set()).add(t)

    def edge_faces(a, b):
        return [t for t in vf[a] if b in faces[t]]

    def classes_of(u):
        bd = lk = False
        for t in vf[u]:
            for w in faces[t]:
                if w != u:
                    n = len(edge_faces(u, w))
                    bd |= n == 1
                    lk |= n > 2
        return bd, lk

    def evaluate(a, b):
        """-> (cost bits, x) when the edge is valid now, else None."""
        n = len(edge_faces(a, b))
        (ba, la), (bb, lb) = classes_of(a), classes_of(b)
        x, cx = placement(p, Q, np.array([a]), np.array([b]), optimalplacement)
        x, key = x[0], int(cx.view(np.int64)[0] >> 32)
        if la or lb or (n == 2 and ba and bb) or not 1 <= n <= 2:
            return key, None
        na = {w for t in vf[a] for w in faces[t]} - {a}
        nb = {w for t in vf[b] for w in faces[t]} - {b}
        if len((na & nb) - {a, b}) != n:
            return key, None
        oppa = {frozenset(set(faces[t]) - {a}) for t in vf[a] if b not in faces[t]}
        oppb = {frozenset(set(faces[t]) - {b}) for t in vf[b] if a not in faces[t]}
        if oppa & oppb:
            return key, None
        for u, o in ((a, b), (b, a)):
            for t in vf[u]:
                if o in faces[t]:
                    continue
                q = p[list(faces[t])]
                n0 = face_g(q[0], q[1], q[2])
                q[faces[t].index(u)] = x
                if not dot(n0, face_g(q[0], q[1], q[2])) > 0.0:
                    return key, None
        return key, x

    heap, stamp = [], {}

    def push(a, b):
        a, b = min(a, b), max(a, b)
        key, x = evaluate(a, b)
        stamp[(a, b)] = stamp.get((a, b), 0) + 1
        if x is not None:
            heapq.heappush(heap, (key, a, b, stamp[(a, b)], tuple(x)))

    for a, b in sorted({(min(i, j), max(i, j)) for row in faces.values() for i, j in zip(row, row[1:] + row[:1])}):
        push(a, b)
    collapses = 0
    while len(faces) > target and heap:
        key, a, b, s, x = heapq.heappop(heap)
        if stamp.get((a, b)) != s:
            continue
        p[a] = x
        Q[a] = Q[a] + Q[b]
        for t in list(vf.pop(b)):
            if a in faces[t]:
                for w in faces[t]:
                    if w != b:
                        vf[w].discard(t)
                del faces[t]
            else:
                faces[t] = tuple(a if w == b else w for w in faces[t])
                vf[a].add(t)
        for k in [k for k in stamp if b in k]:
            del stamp[k]
        collapses += 1
        ring1 = {w for t in vf[a] for w in faces[t]}
        dirty = set()
        for u in ring1:                                              # every edge with an endpoint in the closed 1-ring
            for t in vf[u]:
                for w in faces[t]:
                    if w != u:
                        dirty.add((min(u, w), max(u, w)))
        for i, j in sorted(dirty):
            push(i, j)
    if stats is not None:
        stats.update(collapses=collapses, faces_after=len(faces), stalled=len(faces) > target)
    fo = np.array([faces[t] for t in sorted(faces)], dtype=np.int64).reshape(-1, 3)
    used = np.unique(fo.reshape(-1))
    remap = np.full(V, -1, dtype=np.int64)
    remap[used] = np.arange(len(used))
    return p[used].astype(np.float32), remap[fo].reshape(-1, 3), used.astype(np.int64)


def topology(f):
    """(Euler characteristics of the edge-connected components, sorted; components; boundary loops) of faces f [F, 3]."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        return [], 0, 0
    V = int(f.max()) + 1
    uk, node, ecnt = edge_table(f, V)

    def labels(n, i, j):
        lab = np.arange(n)
        while True:
            new = lab.copy()
            np.minimum.at(new, i, lab[j])
            np.minimum.at(new, j, lab[i])
            new = new[new]
            if np.array_equal(new, lab):
                return lab
            lab = new

    # faces joined through shared edges: face - edge bipartite labels
    lab = labels(len(f) + len(uk), np.repeat(np.arange(len(f)), 3), len(f) + node.reshape(-1))
    fl, el = lab[:len(f)], lab[len(f):]
    chi = []
    for c in np.unique(fl):
        fc = f[fl == c]
        chi.append(len(np.unique(fc)) - int((el == c).sum()) + len(fc))
    bk = uk[ecnt == 1]
    loops = 0
    if len(bk):
        bl = labels(V, bk // V, bk % V)
        loops = len(np.unique(bl[np.unique(np.concatenate([bk // V, bk % V]))]))
    return sorted(chi), len(chi), loops


def check_invariants(v, f, f_in=None):
    """The properties of every output: no unreferenced vertex, no repeated index, no duplicate or zero-area face; with
    the input faces f_in (every edge with one or two faces, consistently wound) also manifold edges, consistent winding
    and the input's Euler characteristics, components and boundary loops."""
    v = np.asarray(v, dtype=np.float32).astype(F64)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    if len(f) == 0:
        assert len(v) == 0
        return
    assert np.array_equal(np.unique(f), np.arange(len(v))), "unreferenced vertex"
    assert len(live_faces(f)) == len(f), "repeated index"
    assert len(np.unique(np.sort(f, 1), axis=0)) == len(f), "duplicate face"
    g = face_g(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    assert (dot(g, g) > 0).all(), "zero-area face"
    if f_in is not None:
        _, _, ecnt = edge_table(f, len(v))
        assert ecnt.max() <= 2, "non-manifold edge"
        d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert len(np.unique(d[:, 0] * len(v) + d[:, 1])) == len(d), "a directed edge appears twice (winding)"
        assert topology(f) == topology(live_faces(f_in)), (topology(f), topology(live_faces(f_in)))


def surface_distance(vol, v, f, n=200000, seed=0):
    """(rms, max) of |trilinear(vol, x)| over n area-weighted samples of the mesh plus its vertices, in index units."""
    v = np.asarray(v, dtype=F64)
    rng = np.random.default_rng(seed)
    q = v[f]
    area = np.linalg.norm(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), axis=1)
    t = rng.choice(len(f), size=n, p=area / area.sum())
    r1, r2 = np.sqrt(rng.random(n)), rng.random(n)
    pts = (1 - r1)[:, None] * q[t, 0] + (r1 * (1 - r2))[:, None] * q[t, 1] + (r1 * r2)[:, None] * q[t, 2]
    pts = np.concatenate([pts, v])
    hi = np.array(vol.shape) - 1
    pts = np.clip(pts, 0, hi - 1e-9)
    i = np.floor(pts).astype(np.int64)
    w = pts - i
    d = np.zeros(len(pts))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wt = (w[:, 0] if dx else 1 - w[:, 0]) * (w[:, 1] if dy else 1 - w[:, 1]) * (w[:, 2] if dz else 1 - w[:, 2])
                d += wt * vol[i[:, 0] + dx, i[:, 1] + dy, i[:, 2] + dz]
    return float(np.sqrt((d * d).mean())), float(np.abs(d).max())
