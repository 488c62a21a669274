"""numpy restatement of the texture-bake kernels (csrc/texbake.hip), written from the rules in include/primx_hip.h:
face labels, charts, projection, the fixed-point snap, the atlas raster (face-id map + cover count), the barycentric
points and the texel fill.  CPU only; shared by the CPU and GPU tests."""
import numpy as np

PROJECTION = ((1, 2), (2, 1), (2, 0), (0, 2), (0, 1), (1, 0))
FIX = 256
F32 = np.float32


def _axis_label(s):
    """s [F, 3] fp32 -> 2a + (s[a] < 0), a = argmax |s| with ties to the lower axis."""
    a = np.abs(s)
    ax = np.zeros(len(s), dtype=np.int64)
    ax[a[:, 1] > a[:, 0]] = 1
    m = np.maximum(a[:, 0], a[:, 1])   # |s[ax]| after the first two axes
    ax[a[:, 2] > m] = 2
    sa = s[np.arange(len(s)), ax]
    return 2 * ax + (sa < 0).astype(np.int64)   # -0.0 < 0 is False: 0 counts as +


def face_labels(v, f, n=None):
    v = np.asarray(v, dtype=F32)
    f = np.asarray(f, dtype=np.int64)
    p0, p1, p2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    g = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1).astype(F32)
    if n is None:
        s = g
    else:
        n = np.asarray(n, dtype=F32)
        s = (n[f[:, 0]] + n[f[:, 1]]) + n[f[:, 2]]
    lab = _axis_label(s)
    a = lab // 2
    ga = g[np.arange(len(g)), a]
    ga = np.where(lab % 2 == 1, -ga, ga)
    gn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(F32)
    relabel = ga <= F32(0.2) * gn
    lab[relabel] = _axis_label(g[relabel])
    return lab, g


def components(node):
    """node [F, 3] int -> (component ids [F] = rank of the component's smallest face, count)."""
    node = np.asarray(node, dtype=np.int64)
    F = len(node)
    if F == 0:
        return np.zeros(0, dtype=np.int64), 0
    flat = node.reshape(-1)
    face = np.repeat(np.arange(F), 3)
    minface = np.full(flat.max() + 1, F, dtype=np.int64)
    np.minimum.at(minface, flat, face)
    a, b = face, minface[flat]
    parent = np.arange(F)
    while True:
        old = parent.copy()
        r = np.minimum(parent[a], parent[b])
        np.minimum.at(parent, parent[a], r)
        np.minimum.at(parent, parent[b], r)
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        if np.array_equal(parent, old):
            break
    roots = np.unique(parent)
    return np.searchsorted(roots, parent), len(roots)


def charts(v, f, n=None):
    lab, _ = face_labels(v, f, n)
    f = np.asarray(f, dtype=np.int64)
    comp, nc = components(f * 6 + lab[:, None])
    return lab, comp, nc


def project(v, f, lab):
    """-> [F, 3, 2] fp32 (u, v) of each corner in its label's projection."""
    v = np.asarray(v, dtype=F32)
    f = np.asarray(f, dtype=np.int64)
    proj = np.asarray(PROJECTION)[lab]                                 # [F, 2]
    c = v[f]                                                           # [F, 3, 3]
    return np.take_along_axis(c, np.broadcast_to(proj[:, None, :], (len(f), 3, 2)), 2)


def snap(uv, lo, scale, off):
    """Texel position (uv - lo) * scale + off in fp32, then to 1/256 texel (round half to even)."""
    x = (np.asarray(uv, F32) - np.asarray(lo, F32)) * F32(scale) + np.asarray(off, F32)
    return np.rint(x * F32(FIX)).astype(np.int64)


def _owned(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def raster(uv_fixed, ft, W, H):
    """-> (face_id [H, W] int64 (-1 empty, smallest covering face), cover count [H, W])."""
    uv = np.asarray(uv_fixed, dtype=np.int64)
    ft = np.asarray(ft, dtype=np.int64)
    fid = np.full((H, W), -1, dtype=np.int64)
    cnt = np.zeros((H, W), dtype=np.int64)
    for face in range(len(ft) - 1, -1, -1):                            # descending: the smallest face is written last
        A, B, Cc = uv[ft[face, 0]], uv[ft[face, 1]], uv[ft[face, 2]]
        area = (B[0] - A[0]) * (Cc[1] - A[1]) - (B[1] - A[1]) * (Cc[0] - A[0])
        if area <= 0:
            continue
        xs, ys = np.array([A[0], B[0], Cc[0]]), np.array([A[1], B[1], Cc[1]])
        j0, j1 = max(0, -((FIX // 2 - xs.min()) // FIX)), min(W - 1, (xs.max() - FIX // 2) // FIX)
        i0, i1 = max(0, -((FIX // 2 - ys.min()) // FIX)), min(H - 1, (ys.max() - FIX // 2) // FIX)
        if j0 > j1 or i0 > i1:
            continue
        J, I = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1))
        X, Y = FIX * J + FIX // 2, FIX * I + FIX // 2
        inside = np.ones(X.shape, dtype=bool)
        for P, Q in ((B, Cc), (Cc, A), (A, B)):
            dx, dy = Q[0] - P[0], Q[1] - P[1]
            e = dx * (Y - P[1]) - dy * (X - P[0])
            inside &= (e > 0) | ((e == 0) & _owned(dx, dy))
        fid[I[inside], J[inside]] = face
        cnt[I[inside], J[inside]] += 1
    return fid, cnt


def points(fid, uv_fixed, ft, v, f):
    """Covered texels in raster order -> (texel index [n], fp32 points [n, 3])."""
    H, W = fid.shape
    t = np.nonzero(fid.reshape(-1) >= 0)[0]
    face = fid.reshape(-1)[t]
    uv = np.asarray(uv_fixed, dtype=np.int64)[np.asarray(ft, dtype=np.int64)[face]]   # [n, 3, 2]
    X, Y = FIX * (t % W) + FIX // 2, FIX * (t // W) + FIX // 2
    A, B, Cc = uv[:, 0], uv[:, 1], uv[:, 2]

    def e(P, Q):
        return (Q[:, 0] - P[:, 0]) * (Y - P[:, 1]) - (Q[:, 1] - P[:, 1]) * (X - P[:, 0])

    area = (B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (Cc[:, 0] - A[:, 0])
    ar = area.astype(F32)
    lam = [e(B, Cc).astype(F32) / ar, e(Cc, A).astype(F32) / ar, e(A, B).astype(F32) / ar]
    vv = np.asarray(v, dtype=F32)[np.asarray(f, dtype=np.int64)[face]]   # [n, 3, 3]
    p = (lam[0][:, None] * vv[:, 0] + lam[1][:, None] * vv[:, 1]) + lam[2][:, None] * vv[:, 2]
    return t, p.astype(F32)


def quantize(x):
    return np.clip(np.trunc(np.asarray(x, dtype=F32) * F32(255)), 0, 255).astype(np.uint8)


def dilate(mask, iterations):
    """4-connected binary dilation, outside the image = 0 (scipy.ndimage.binary_dilation with its default structure)."""
    m = mask.copy()
    for _ in range(iterations):
        d = m.copy()
        d[1:] |= m[:-1]
        d[:-1] |= m[1:]
        d[:, 1:] |= m[:, :-1]
        d[:, :-1] |= m[:, 1:]
        m = d
    return m


def erode(mask, iterations):
    """4-connected binary erosion with border value 0."""
    m = mask.copy()
    for _ in range(iterations):
        e = m.copy()
        e[0] = False
        e[-1] = False
        e[:, 0] = False
        e[:, -1] = False
        e[1:] &= m[:-1]
        e[:-1] &= m[1:]
        e[:, 1:] &= m[:, :-1]
        e[:, :-1] &= m[:, 1:]
        m = e
    return m


def fill_regions(covered, radius=32, band=3):
    inpaint = dilate(covered, radius) & ~covered
    bandm = covered & ~erode(covered, band)
    return inpaint, bandm


def nearest_band(covered, radius=32, band=3):
    """-> (inpaint mask, bandm, src [H, W, 2] row / column of the chosen band texel (-1 where not inpainted), d2)."""
    H, W = covered.shape
    inpaint, bandm = fill_regions(covered, radius, band)
    best = np.full((H, W), np.iinfo(np.int64).max, dtype=np.int64)
    src = np.full((H, W, 2), -1, dtype=np.int64)
    pad = np.zeros((H + 2 * radius, W + 2 * radius), dtype=bool)
    pad[radius:radius + H, radius:radius + W] = bandm
    offs = sorted(((di * di + dj * dj, di, dj) for di in range(-radius, radius + 1) for dj in range(-radius, radius + 1)))
    I, J = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    todo = inpaint.copy()
    for d2, di, dj in offs:                          # ascending (d2, row offset, column offset): first hit wins
        if not todo.any():
            break
        hit = todo & pad[radius + di:radius + di + H, radius + dj:radius + dj + W]
        best[hit] = d2
        src[hit, 0] = I[hit] + di
        src[hit, 1] = J[hit] + dj
        todo &= ~hit
    return inpaint, bandm, src, best


def fill(attr, texel, covered, radius=32, band=3):
    """attr [n, 6] fp32 at covered texels (raster order) -> (albedo, metallic_roughness) uint8 [H, W, 3]."""
    H, W = covered.shape
    img = np.zeros((H * W, 6), dtype=np.uint8)
    q = quantize(np.asarray(attr)[:, 1:6]) if len(texel) else np.zeros((0, 5), np.uint8)
    img[texel, 0:3] = q[:, 0:3]
    img[texel, 4:6] = q[:, 3:5]
    img = img.reshape(H, W, 6)
    out = np.where(covered[..., None], img, 0).astype(np.uint8)
    inpaint, _, src, _ = nearest_band(covered, radius, band)
    ii, jj = np.nonzero(inpaint)
    out[ii, jj] = img[src[ii, jj, 0], src[ii, jj, 1]]
    return out[..., 0:3].copy(), out[..., 3:6].copy()


def shelf_overlaps(org, w, h, W, H):
    """True when two rectangles overlap or one leaves the W x H atlas."""
    org = np.asarray(org)
    if ((org[:, 0] < 0) | (org[:, 1] < 0) | (org[:, 0] + w > W) | (org[:, 1] + h > H)).any():
        return True
    occ = np.zeros((H, W), dtype=np.int64)
    for (x, y), ww, hh in zip(org, w, h):
        occ[y:y + hh, x:x + ww] += 1
    return bool((occ > 1).any())
