"""Numpy restatement of `primx_material_sample` (include/primx_hip.h "Textured meshes", csrc/material.hip) and the fixtures its
tests share: textures, material tables, the UV point set and the box with per-face UV charts.

The oracle is the glTF 2.0 specification's sampler and metallic-roughness rules as the header states them.  `sample(...,
dtype=np.float32)` performs the header's operations one by one, each rounded to float32: the bit-exact model of the kernel.
`dtype=np.float64` is the same expressions in float64 on the same (float32) inputs: the reference value, and the measure of what
fp32 costs (tests/test_hip_material.py takes its field-level bounds from float32-against-float64 of this file).
"""
from __future__ import annotations

import numpy as np

CLAMP, REPEAT, MIRROR = 0, 1, 2
X_LIMIT = 2.0 ** 30


def flags(wrap_s, wrap_t, nearest=False):
    return wrap_s | wrap_t << 2 | (16 if nearest else 0)


def wrap(i, n, mode):
    """Integer arrays i -> [0, n)."""
    i = np.asarray(i, np.int64)
    if mode == CLAMP:
        return np.minimum(np.maximum(i, 0), n - 1)
    if mode == REPEAT:
        return np.mod(i, n)
    t = np.mod(i, 2 * n)
    return np.where(t < n, t, 2 * n - 1 - t)


def _texel(blob, off, W, i, j, dtype):
    """RGB of texels (i, j) -> [n, 3] in dtype: float(byte) / 255."""
    return blob[off + j * W + i, :3].astype(dtype) / dtype(255.0)


def sample_texture(blob, desc_row, u, v, dtype):
    """One texture at (u, v) [n] (already finite, in dtype) -> [n, 3]."""
    off, W, H, fl = (int(x) for x in desc_row)
    ws, wt, nearest = fl & 3, (fl >> 2) & 3, bool(fl & 16)
    lim = dtype(X_LIMIT)
    Wf, Hf = dtype(W), dtype(H)
    with np.errstate(over="ignore"):
        if nearest:
            i = np.clip(np.floor(u * Wf), -lim, lim).astype(np.int64)
            j = np.clip(np.floor(v * Hf), -lim, lim).astype(np.int64)
            return _texel(blob, off, W, wrap(i, W, ws), wrap(j, H, wt), dtype)
        x = np.clip(u * Wf - dtype(0.5), -lim, lim)
        y = np.clip(v * Hf - dtype(0.5), -lim, lim)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    i0, j0 = xf.astype(np.int64), yf.astype(np.int64)
    ia, ib, ja, jb = wrap(i0, W, ws), wrap(i0 + 1, W, ws), wrap(j0, H, wt), wrap(j0 + 1, H, wt)
    t00, t10 = _texel(blob, off, W, ia, ja, dtype), _texel(blob, off, W, ib, ja, dtype)
    t01, t11 = _texel(blob, off, W, ia, jb, dtype), _texel(blob, off, W, ib, jb, dtype)
    gx, gy = dtype(1) - fx, dtype(1) - fy
    return (t00 * gx + t10 * fx) * gy + (t01 * gx + t11 * fx) * fy


def sample(uv, vattr, face, face_material, mat_factor, mat_tex, desc, blob, dtype=np.float64):
    """-> out [n, 5] in dtype.  uv [n, 2], vattr [n, 6] or None, face [n]; the tables as the kernel takes them (numpy arrays)."""
    uv = np.asarray(uv, np.float32)
    n = uv.shape[0]
    uvd = np.where(np.isfinite(uv), uv, np.float32(0)).astype(dtype)
    a = np.ones((n, 6), dtype) if vattr is None else np.asarray(vattr, np.float32).astype(dtype)
    m = np.asarray(face_material)[np.asarray(face, np.int64)].astype(np.int64)
    fac = np.asarray(mat_factor, np.float32).astype(dtype)[m]
    base, mr = np.ones((n, 3), dtype), np.ones((n, 3), dtype)
    mat_tex = np.asarray(mat_tex)
    for slot, dst in ((0, base), (1, mr)):
        t = mat_tex[m, slot]
        for k in np.unique(t[t >= 0]):
            sel = t == k
            dst[sel] = sample_texture(blob, desc[k], uvd[sel, 0], uvd[sel, 1], dtype)
    out = np.empty((n, 5), dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, :3] = (fac[:, :3] * a[:, :3]) * base
        out[:, 3] = (fac[:, 4] * a[:, 4]) * mr[:, 1]
        out[:, 4] = (fac[:, 5] * a[:, 5]) * mr[:, 2]
    return out


# ------------------------------------------------------------------------------------------------------------ fixtures
def random_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def pack(images, tex):
    """images: uint8 [H, W, 4] arrays; tex: (image index, flags) per texture -> (desc [T, 4] int64, blob [n, 4] uint8)."""
    offs, off = [], 0
    for im in images:
        offs.append(off)
        off += im.shape[0] * im.shape[1]
    desc = np.array([[offs[i], images[i].shape[1], images[i].shape[0], fl] for i, fl in tex], np.int64).reshape(-1, 4)
    blob = np.concatenate([im.reshape(-1, 4) for im in images]) if images else np.zeros((1, 4), np.uint8)
    return desc, np.ascontiguousarray(blob)


SIZES = ((1, 1), (3, 2), (7, 5), (64, 64))         # (H, W): textures 1 x 1, 2 x 3, 5 x 7 and 64 x 64 (W x H)


def uv_points(n=1000, seed=0):
    """[n, 2] float32: special values first (exact texel centres and edges of every size of SIZES, 0, 1, -0.0, +-1e30 and their
    mixes), then uniform in [-3, 4]."""
    rng = np.random.default_rng(seed)
    sp = [(0.0, 0.0), (1.0, 1.0), (-0.0, -0.0), (0.0, 1.0), (1.0, -0.0), (1e30, -1e30), (-1e30, 1e30), (1e30, 0.25), (0.75, -1e30)]
    for H, W in SIZES:
        for i in range(-W - 1, 2 * W + 2):
            j = (i * 3 + 1) % (3 * H) - H
            sp.append(((i + 0.5) / W, (j + 0.5) / H))              # centres
            sp.append((i / W, j / H))                               # edges
            sp.append((i / W, (j + 0.5) / H))
    sp = np.asarray(sp, np.float64)
    sp = np.concatenate([sp[:9], sp[9:][rng.permutation(sp.shape[0] - 9)][:n // 2 - 9]])      # the nine named ones always
    rest = rng.uniform(-3.0, 4.0, (n - sp.shape[0], 2))
    p = np.concatenate([sp, rest])[rng.permutation(n)].astype(np.float32)
    return np.ascontiguousarray(p)


def sampler_scene(wrap_s, wrap_t, nearest, size_index, seed=0, n=1000, F=37):
    """One kernel test case: three materials (0: base + metallic-roughness textures of SIZES[size_index]; 1: a base texture of the
    next size alone, other factors; 2: no textures), F faces cycling through them, n points.  -> dict of numpy arrays."""
    rng = np.random.default_rng(1000 * size_index + 100 * wrap_s + 10 * wrap_t + int(nearest) + seed)
    (h0, w0), (h1, w1) = SIZES[size_index], SIZES[(size_index + 1) % len(SIZES)]
    images = [random_image(h0, w0, seed + 1), random_image(h0, w0, seed + 2), random_image(h1, w1, seed + 3)]
    fl = flags(wrap_s, wrap_t, nearest)
    desc, blob = pack(images, [(0, fl), (1, fl), (2, flags(wrap_t, wrap_s, nearest))])
    mat_factor = np.array([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [0.8, 0.5, 0.25, 0.5, 0.7, 0.3], [0.9, 0.1, 0.6, 1.0, 0.4, 0.2]], np.float32)
    mat_tex = np.array([[0, 1], [2, -1], [-1, -1]], np.int32)
    face_material = (np.arange(F) % 3).astype(np.int32)
    return dict(uv=uv_points(n, seed), vattr=rng.uniform(0.0, 1.25, (n, 6)).astype(np.float32),
                face=rng.integers(0, F, n).astype(np.int32), face_material=face_material, mat_factor=mat_factor, mat_tex=mat_tex,
                desc=desc, blob=blob)


def restated(s, dtype, n=None, vattr=True):
    n = s["uv"].shape[0] if n is None else n
    return sample(s["uv"][:n], s["vattr"][:n] if vattr else None, s["face"][:n], s["face_material"], s["mat_factor"], s["mat_tex"],
                  s["desc"], s["blob"], dtype)


def uv_box(lo=(-0.3, -0.2, -0.4), hi=(0.35, 0.25, 0.15)):
    """The box of tests/meshfield_numpy.py with per-face UV charts: 24 split vertices, 12 faces (outward), one chart per side laid
    out on a 3 x 2 grid of [0, 1]^2 with a margin, and sides 0 .. 2 / 3 .. 5 under materials 0 / 1.
    -> (v [24, 3], f [12, 3], vt [24, 2], face_material [12])."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    corner = np.array([[(hi if (i >> k) & 1 else lo)[k] for k in range(3)] for i in range(8)])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    v, f, vt, fm = [], [], [], []
    for s, q in enumerate(quads):
        cu, cv = (s % 3) / 3.0, (s // 3) / 2.0
        uvq = [(cu + 0.02, cv + 0.03), (cu + 0.31, cv + 0.03), (cu + 0.31, cv + 0.47), (cu + 0.02, cv + 0.47)]
        base = len(v)
        v += [corner[i] for i in q]
        vt += uvq
        f += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
        fm += [s // 3, s // 3]
    return (np.asarray(v).astype(np.float32), np.asarray(f, np.int32), np.asarray(vt).astype(np.float32),
            np.asarray(fm, np.int32))


def box_scene(seed=0):
    """The textured box of the field-level and fit tests: a 5 x 7 (W x H) base texture under material 0 (REPEAT), an 8 x 8 base and a
    5 x 7 metallic-roughness texture under material 1 (CLAMP / MIRROR), LINEAR, per-vertex colours and multipliers."""
    v, f, vt, fm = uv_box()
    rng = np.random.default_rng(seed + 77)
    images = [random_image(7, 5, seed + 11), random_image(8, 8, seed + 12)]
    tex = [(0, flags(REPEAT, REPEAT)), (1, flags(CLAMP, MIRROR)), (0, flags(MIRROR, CLAMP))]
    desc, blob = pack(images, tex)
    mat_factor = np.array([[1.0, 0.9, 0.8, 1.0, 0.9, 0.5], [0.7, 1.0, 0.6, 1.0, 1.0, 0.8]], np.float32)
    mat_tex = np.array([[0, -1], [1, 2]], np.int32)
    color = rng.uniform(0.5, 1.0, (24, 4)).astype(np.float32)
    rm = rng.uniform(0.5, 1.0, (24, 2)).astype(np.float32)
    return dict(v=v, f=f, vt=vt, color=color, rm=rm, face_material=fm, mat_factor=mat_factor, mat_tex=mat_tex, desc=desc, blob=blob,
                images=images, tex_image=np.array([0, 1, 0], np.int32),
                tex_sampler=np.array([[REPEAT, REPEAT, 0], [CLAMP, MIRROR, 0], [MIRROR, CLAMP, 0]], np.int32))


def box_attr(s):
    return np.concatenate([s["vt"], s["color"], s["rm"]], 1).astype(np.float32)


def field_attributes(MF, p, v, face, s, dtype):
    """The restated pipeline behind MeshField.query with a material, on a GIVEN face assignment: interpolate [vt | color | rm] at
    each point's closest point of its face (tests/meshfield_numpy.attr_on_face), round to float32 when dtype is float32 (the
    kernel's hand-over), then the restated sampler; clipped to [0, 1] -> [n, 5] in dtype."""
    a = MF.attr_on_face(p, v, s["f"], box_attr(s), face, dtype)
    uv, va = a[:, :2], a[:, 2:]
    if dtype == np.float32:
        out = sample(uv, va, face, s["face_material"], s["mat_factor"], s["mat_tex"], s["desc"], s["blob"], np.float32)
    else:
        out = _sample64(uv, va, face, s)
    return np.clip(out, 0, 1)


def _sample64(uv, va, face, s):
    """`sample` in float64 on float64 uv / vattr (not rounded to float32 on the way in)."""
    n = uv.shape[0]
    m = s["face_material"][np.asarray(face, np.int64)].astype(np.int64)
    fac = s["mat_factor"].astype(np.float64)[m]
    base, mr = np.ones((n, 3)), np.ones((n, 3))
    for slot, dst in ((0, base), (1, mr)):
        t = s["mat_tex"][m, slot]
        for k in np.unique(t[t >= 0]):
            sel = t == k
            dst[sel] = sample_texture(s["blob"], s["desc"][k], uv[sel, 0], uv[sel, 1], np.float64)
    out = np.empty((n, 5))
    out[:, :3] = (fac[:, :3] * va[:, :3]) * base
    out[:, 3] = (fac[:, 4] * va[:, 4]) * mr[:, 1]
    out[:, 4] = (fac[:, 5] * va[:, 5]) * mr[:, 2]
    return out
