"""numpy restatement of the marching-cubes kernels (csrc/mcubes.hip) on the generated case table, in the kernels' exact
output order, plus the mesh checks the tests share.  CPU only."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "3dtopia-xl_amd", "csrc", "gen_mc_tables.py")


def gen_module():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_G = gen_module()
TRI, MASK = _G.tables()
TRI_PAD = np.array([t + [-1] * (15 - len(t)) for t in TRI], dtype=np.int64)   # [256, 15]
EDGE_AXIS = np.array([a for a, _, _ in _G.EDGES])
EDGE_CORNER = np.array([c for _, c, _ in _G.EDGES])


def _grad(vol, axis):
    """Central differences inside, one-sided at the borders, fp32 as the kernel computes them."""
    v = np.moveaxis(vol, axis, 0)
    g = np.empty_like(v)
    g[1:-1] = (v[2:] - v[:-2]) * np.float32(0.5)
    g[0] = v[1] - v[0]
    g[-1] = v[-1] - v[-2]
    return np.moveaxis(g, 0, axis)


def marching_cubes(vol, iso=0.0):
    """-> (vertices fp32 [V, 3] index coordinates, normals fp32 [V, 3], triangles int64 [F, 3]) in kernel order."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    iso = np.float32(iso)
    nx, ny, nz = vol.shape
    inside = vol < iso
    cross = np.zeros(vol.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.full(flat.shape, -1, dtype=np.int64)
    vid[flat] = np.arange(int(flat.sum()))
    vid = vid.reshape(-1, 3)
    p, a = np.nonzero(cross.reshape(-1, 3))                      # (owner point, axis) in order
    i, j, k = np.unravel_index(p, vol.shape)
    strides = np.array([ny * nz, nz, 1])
    q = p + strides[a]
    v0, v1 = vol.reshape(-1)[p], vol.reshape(-1)[q]
    t = (iso - v0) / (v1 - v0)
    pos = np.stack([i, j, k], 1).astype(np.float32)
    pos[np.arange(len(p)), a] += t
    g = np.stack([_grad(vol, b).reshape(-1) for b in range(3)], 1)
    g0, g1 = g[p], g[q]
    gi = (np.float32(1) - t)[:, None] * g0 + t[:, None] * g1
    l2 = (gi[:, 0] * gi[:, 0] + gi[:, 1] * gi[:, 1]) + gi[:, 2] * gi[:, 2]
    inv = np.where(l2 > 0, np.float32(1) / np.sqrt(np.maximum(l2, np.float32(1e-30))), np.float32(0)).astype(np.float32)
    nrm = gi * inv[:, None]
    # cells in point order, triangles in table order
    cube = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for b in range(8):
        di, dj, dk = b & 1, b >> 1 & 1, b >> 2 & 1
        cube |= inside[di:nx - 1 + di, dj:ny - 1 + dj, dk:nz - 1 + dk].astype(np.int64) << b
    ci, cj, ck = np.nonzero(cube)
    cells = (ci * ny + cj) * nz + ck
    rows = TRI_PAD[cube[ci, cj, ck]]                             # [n, 15]
    valid = rows >= 0
    e = rows[valid]
    cell = np.repeat(cells, valid.sum(1))
    c = EDGE_CORNER[e]
    owner = cell + (c & 1) * ny * nz + (c >> 1 & 1) * nz + (c >> 2 & 1)
    f = vid[owner, EDGE_AXIS[e]].reshape(-1, 3)
    assert (f >= 0).all()
    return pos, nrm.astype(np.float32), f


def sign_changing_edges(vol, iso=0.0):
    inside = vol < iso
    return int((inside[1:] != inside[:-1]).sum() + (inside[:, 1:] != inside[:, :-1]).sum() +
               (inside[:, :, 1:] != inside[:, :, :-1]).sum())


def ambiguous_faces(vol, iso=0.0):
    """Lattice faces whose four corners alternate in sign (the only faces where the triangulation has a choice)."""
    s = vol < iso
    n = 0
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        m = np.moveaxis(s, (b, c), (0, 1))
        c00, c10, c01, c11 = m[:-1, :-1], m[1:, :-1], m[:-1, 1:], m[1:, 1:]
        n += int(((c00 == c11) & (c10 == c01) & (c00 != c10)).sum())
    return n


def mesh_checks(v, f):
    """Watertight + consistently oriented + no degenerate index triples; returns (V - E + F, signed volume)."""
    f = np.asarray(f, dtype=np.int64)
    v = np.asarray(v, dtype=np.float64)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = d[:, 0] * (len(v) + 1) + d[:, 1]
    assert len(np.unique(key)) == len(key), "a directed edge appears twice (orientation)"
    und = np.sort(d, 1)
    _, cnt = np.unique(und[:, 0] * (len(v) + 1) + und[:, 1], return_counts=True)
    assert (cnt == 2).all(), "an undirected edge is not shared by exactly two triangles"
    E = len(cnt)
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
    return len(v) - E + len(f), vol


def analytic_fields(n):
    """{name: (lattice, analytic volume or None, Euler characteristic or None, unit gradient fn or None)} in index units."""
    x = np.arange(n, dtype=np.float64)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    c = (n - 1) / 2.0 + 0.137                                     # off-lattice centre
    out = {}
    r = 0.36 * n
    sph = np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2) - r
    out["sphere"] = (sph.astype(np.float32), 4.0 / 3.0 * np.pi * r ** 3, 2,
                     lambda p: (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True))
    R, rr = 0.26 * n, 0.12 * n
    q = np.sqrt((X - c) ** 2 + (Y - c) ** 2) - R
    out["torus"] = ((np.sqrt(q ** 2 + (Z - c) ** 2) - rr).astype(np.float32), 2 * np.pi ** 2 * R * rr ** 2, 0, None)
    blobs = np.zeros_like(X)
    for (bx, by, bz, s) in ((0.35, 0.4, 0.5, 0.10), (0.62, 0.45, 0.48, 0.12), (0.5, 0.66, 0.4, 0.09)):
        blobs += np.exp(-((X - bx * n) ** 2 + (Y - by * n) ** 2 + (Z - bz * n) ** 2) / (2 * (s * n) ** 2))
    out["blobs"] = ((0.5 - blobs).astype(np.float32), None, None, None)
    return out
