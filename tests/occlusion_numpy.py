"""Restatement of the ambient-occlusion rules A1-A4 of include/primx_hip.h (primx_texbake_occlusion) and of
mesh.occlusion_directions, written from the header's text.  Every function takes `dtype`: float64 is the truth, float32 the same
arithmetic at the kernel's precision, whose distance from float64 sets the tolerance of tests/test_hip_occlusion.py (4 x that
distance, pooled over all cases).  The operands are the kernel's own: the fp32 lattice, points, normals and direction table, and
the fp32 values of radius, bias and isovalue, cast to `dtype`.

* `directions`: the Fibonacci sphere, float64 then cast to float32;
* `phi`: rule A1, the clamped trilinear lookup minus the isovalue;
* `occlusion`: rules A2-A4; with `exact=` the same estimator on a function of the position instead of the lattice;
* `quantize`: the fill's byte, trunc(fp32(ao * 255)) clamped to [0, 255].
"""
from __future__ import annotations

import numpy as np


def directions(K: int) -> np.ndarray:
    k = np.arange(K, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / K
    r = np.sqrt(1.0 - z * z)
    a = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(a), r * np.sin(a), z], 1).astype(np.float32)


def _lerp(p, q, t):
    return p + t * (q - p)


def phi(lattice, x, isovalue=0.0, dtype=np.float64):
    """A1: lattice [R, R, R], x [..., 3] -> [...] in `dtype`."""
    dt = np.dtype(dtype).type
    lat = np.asarray(lattice, dtype=dtype)                         # no copy when the caller has cast it
    R = lat.shape[0]
    x = np.asarray(x).astype(dtype)
    c = np.minimum(np.maximum(x, dt(-1)), dt(1))
    u = ((c + dt(1)) * dt(0.5)) * dt(R - 1)
    i = np.minimum(np.floor(u).astype(np.int64), R - 2)
    f = u - i.astype(dtype)
    ix, iy, iz = i[..., 0], i[..., 1], i[..., 2]
    fx, fy, fz = f[..., 0], f[..., 1], f[..., 2]
    z00 = _lerp(lat[ix, iy, iz], lat[ix, iy, iz + 1], fz)
    z01 = _lerp(lat[ix, iy + 1, iz], lat[ix, iy + 1, iz + 1], fz)
    z10 = _lerp(lat[ix + 1, iy, iz], lat[ix + 1, iy, iz + 1], fz)
    z11 = _lerp(lat[ix + 1, iy + 1, iz], lat[ix + 1, iy + 1, iz + 1], fz)
    return _lerp(_lerp(z00, z01, fy), _lerp(z10, z11, fy), fx) - dt(np.float32(isovalue))


def occlusion(lattice, pts, nrm, dirs, steps=8, radius=0.25, bias=None, isovalue=0.0, dtype=np.float64, exact=None):
    """A2-A4 -> ao [n] in `dtype`.  `bias` None: 1.5 lattice spacings, as mesh.texel_occlusion passes it (3 / (R - 1) rounded to
    fp32).  `exact`: a function x [..., 3] (dtype) -> [...] that replaces the lattice lookup (the lattice then only gives R)."""
    dt = np.dtype(dtype).type
    R = np.asarray(lattice).shape[0]
    bias = np.float32(3.0 / max(R - 1.0, 1.0)) if bias is None else np.float32(bias)
    radius, iso = dt(np.float32(radius)), np.float32(isovalue)
    lat = np.asarray(lattice, dtype=np.float32).astype(dtype)
    field = (lambda x: exact(x) - dt(iso)) if exact is not None else (lambda x: phi(lat, x, iso, dtype))
    p, n, d = (np.asarray(a, dtype=np.float32).astype(dtype) for a in (pts, nrm, dirs))
    h = dt(2) / dt(R - 1)
    o = p + dt(bias) * n
    phi0 = np.maximum(field(o), dt(0.5) * h)
    num, den = np.zeros(len(p), dtype), np.zeros(len(p), dtype)
    ts = [(radius * dt(j + 1)) / dt(steps) for j in range(steps)]
    for k in range(len(d)):
        c = np.maximum(dt(0), (n[:, 0] * d[k, 0] + n[:, 1] * d[k, 1]) + n[:, 2] * d[k, 2])
        act = c > 0
        if not act.any():
            continue
        oa = o[act]
        m = None
        for t in ts:
            v = field(oa + t * d[k])
            m = v if m is None else np.minimum(m, v)
        V = np.minimum(np.maximum(m / phi0[act], dt(0)), dt(1))
        num[act] = num[act] + c[act] * (dt(1) - V)
        den[act] = den[act] + c[act]
    ao = np.ones(len(p), dtype)
    pos = den > 0
    ao[pos] = dt(1) - num[pos] / den[pos]
    assert ao.dtype == np.dtype(dtype)
    return ao


def quantize(ao) -> np.ndarray:
    y = np.asarray(ao, dtype=np.float32) * np.float32(255)
    return np.clip(np.trunc(y), 0, 255).astype(np.uint8)
