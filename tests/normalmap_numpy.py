"""Float64 restatement of the normal-map rules of include/primx_hip.h (primx_primsdf_query_grad, primx_texbake_tangents,
primx_texbake_normal_texels) and of mesh.encode_normals, written from the header's text.  Every function takes `dtype`: float64 is
the reference, float32 the same arithmetic at the kernels' precision, whose distance from float64 sets the tolerances of
tests/test_hip_normalmap.py (4 x that distance + one fp32 ulp of the largest entry, the convention of
tests/test_hip_primsdf_grad.py).

* `point_grad`: d sdf / d x by autograd through tests/primsdf_grad_ref.field with x.requires_grad_() - the covered points and the
  training-mode zero of the uncovered ones;
* `fill_value_grad`: the eval-mode fill of an uncovered point and its gradient, written out, with the tie margins;
* `tangents`: rules T1-T4;
* `uv_derivatives`: d pos / d u and d pos / d v of a face from its corners' positions and UVs;
* `barycentrics`: tests/texbake_numpy.points' rule for the covering face's weights;
* `texel_normals`: the texel transform, also returning the interpolated frame;
* `encode` / `decode`: the bytes.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import primsdf_grad_ref as G
from tests import texbake_numpy as tb

PROJECTION = np.asarray(tb.PROJECTION)
T1_THRESHOLD = 1e-4            # |N_c| > T1_THRESHOLD max|N|: rule T1, else T2
T2_DEGENERATE = 1e-8           # |d|^2 below this after Gram-Schmidt: N lies along e_a


# ------------------------------------------------------------------------------------------------ the point gradient
def point_grad(x, srt, feat, S: int, dtype=torch.float64):
    """-> (out [n, C], grad [n, 3]) of the training-mode field in `dtype`: grad = d out[:, 0] / d x by autograd (the points are
    independent, so the gradient of the sum is the per-point gradient).  Uncovered points get out = 0 and grad = 0."""
    x = x.detach().to(dtype).clone().requires_grad_(True)
    out = G.field(x, srt.detach().to(dtype), feat.detach().to(dtype), S)
    out[:, 0].sum().backward()
    return out.detach(), x.grad.detach()


def central_differences(x, srt, feat, S: int, h: float = 1e-6):
    """d out[:, 0] / d x by central differences of the float64 field, step h."""
    x, srt, feat = x.double(), srt.double(), feat.double()
    cols = []
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        cols.append((G.field(x + e, srt, feat, S)[:, 0] - G.field(x - e, srt, feat, S)[:, 0]) / (2 * h))
    return torch.stack(cols, 1)


def covered(x, srt):
    """bool [n]: some primitive covers the point (max_a |d_a| < |s|), in float64."""
    d = (x.double()[:, None, :] - srt.double()[None, :, 1:4]).abs().amax(-1)
    return (d < srt.double()[None, :, 0].abs()).any(1)


def fill_value_grad(x, srt, feat, S: int, dtype=np.float64):
    """The eval-mode fill of primx_primsdf_query at EVERY point as if it were uncovered -> (value [n], grad [n, 3], margin [n]):
    nearest primitive by ||x - pos||_2 (first minimum), per axis the nearest of its S grid points pos + s lin (first minimum; lin =
    the fp32 torch.linspace(-1, 1, S) table), stored sdf there, value = sdf + dist sign(sdf), grad = sign(sdf) (x - g) / dist,
    0 where dist == 0 or sdf == 0.  margin = the smallest gap (in distance units, float64) between the chosen and the runner-up
    primitive or grid point: the caller drops points whose margin is under its delta."""
    X, SRT = np.asarray(x, dtype=dtype), np.asarray(srt, dtype=dtype)
    FEAT = np.asarray(feat, dtype=dtype)
    lin = torch.linspace(-1, 1, S).numpy().astype(dtype)
    n, P = X.shape[0], SRT.shape[0]
    d2 = ((X[:, None, :] - SRT[None, :, 1:4]) ** 2).sum(-1)
    best = d2.argmin(1)
    dist_p = np.sqrt(np.sort(d2.astype(np.float64), 1)[:, :2])
    margin = dist_p[:, 1] - dist_p[:, 0] if P > 1 else np.full(n, np.inf)
    q = SRT[best]
    e = X[:, :, None] - (q[:, 1:4, None] + q[:, 0, None, None] * lin[None, None, :])          # [n, 3, S]
    idx = (e * e).argmin(2)                                                                      # [n, 3] = (ix, iy, iz)
    off = np.take_along_axis(e, idx[:, :, None], 2)[:, :, 0]
    ae = np.sort(np.abs(e.astype(np.float64)), 2)
    margin = np.minimum(margin, (ae[:, :, 1] - ae[:, :, 0]).min(1))
    C = FEAT.shape[1] // S ** 3
    s = FEAT.reshape(P, C, S, S, S)[best, 0, idx[:, 2], idx[:, 1], idx[:, 0]]
    dist = np.sqrt((off * off).sum(1))
    sgn = np.sign(s)
    value = s + dist * sgn
    with np.errstate(divide="ignore", invalid="ignore"):
        grad = np.where((dist > 0)[:, None], sgn[:, None] * off / dist[:, None], 0.0)
    return value.astype(dtype), grad.astype(dtype), margin


def unit(g, dtype=np.float64):
    """Rows of g normalised; (0, 0, 0) where the row is zero."""
    g = np.asarray(g, dtype=dtype)
    l = np.sqrt((g * g).sum(-1, keepdims=True))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(l > 0, g / l, 0).astype(dtype)


# ------------------------------------------------------------------------------------------------ tangents
def vertex_labels(ft, label, nuv):
    """int [NUV]: the label of any incident face of each split vertex (they agree), -1 for a vertex no face names."""
    vl = np.full(nuv, -1, dtype=np.int64)
    vl[np.asarray(ft, dtype=np.int64).reshape(-1)] = np.repeat(np.asarray(label, dtype=np.int64), 3)
    return vl


def tangents(nrm, ft, label, dtype=np.float64):
    """Rules T1-T4 -> [NUV, 4] (unit T, w); zeros for a vertex no face names."""
    N = np.asarray(nrm, dtype=dtype)
    nuv = N.shape[0]
    vl = vertex_labels(ft, label, nuv)
    out = np.zeros((nuv, 4), dtype=dtype)
    rows = np.arange(nuv)
    lab = np.where(vl >= 0, vl, 0)
    a, c = PROJECTION[lab, 0], lab // 2
    sigma = np.where(lab & 1, -1.0, 1.0).astype(dtype)
    Na, Nc = N[rows, a], N[rows, c]
    m = np.abs(N).max(1)
    ea = np.zeros((nuv, 3), dtype=dtype)
    ea[rows, a] = 1
    ec = np.zeros((nuv, 3), dtype=dtype)
    ec[rows, c] = 1
    nn = (N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        d1 = ea - (Na / Nc)[:, None] * ec                                             # T1
        d2 = ea - N * (Na / nn)[:, None]                                              # T2, Gram-Schmidt of e_a
        e = np.where(Nc >= 0, -np.sign(Na), np.sign(Na)).astype(dtype)
        d3 = e[:, None] * ec - N * (e * Nc / nn)[:, None]                             # T2, N along e_a
    small = ((d2 * d2).sum(1) < T2_DEGENERATE)
    d = np.where((np.abs(Nc) > dtype(T1_THRESHOLD) * m)[:, None], d1, np.where((m > 0)[:, None], np.where(small[:, None], d3, d2), ea))
    l = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        out[:, :3] = np.where((l > 0)[:, None], d / l[:, None], ea)
    out[:, 3] = np.where(sigma * Nc < 0, 1.0, -1.0)
    out[vl < 0] = 0
    return out


def uv_derivatives(p, uv):
    """p [F, 3, 3] corner positions, uv [F, 3, 2] corner UVs (float64) -> (d pos / d u [F, 3], d pos / d v [F, 3], det [F]): the
    affine map of each face, det = du1 dv2 - du2 dv1 (twice its signed UV area)."""
    p, uv = np.asarray(p, dtype=np.float64), np.asarray(uv, dtype=np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    du1, dv1 = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 1, 1] - uv[:, 0, 1]
    du2, dv2 = uv[:, 2, 0] - uv[:, 0, 0], uv[:, 2, 1] - uv[:, 0, 1]
    det = du1 * dv2 - du2 * dv1
    with np.errstate(divide="ignore", invalid="ignore"):
        dpdu = (e1 * dv2[:, None] - e2 * dv1[:, None]) / det[:, None]
        dpdv = (e2 * du1[:, None] - e1 * du2[:, None]) / det[:, None]
    return dpdu, dpdv, det


# ------------------------------------------------------------------------------------------------ texels
def barycentrics(texel, fid, uv_fixed, ft):
    """tests/texbake_numpy.points' rule: fp32 (la, lb, lc) [n, 3] of the covering face at each listed texel, and the faces [n]."""
    H, W = fid.shape
    t = np.asarray(texel, dtype=np.int64)
    face = np.asarray(fid).reshape(-1)[t]
    uv = np.asarray(uv_fixed, dtype=np.int64)[np.asarray(ft, dtype=np.int64)[face]]
    X, Y = tb.FIX * (t % W) + tb.FIX // 2, tb.FIX * (t // W) + tb.FIX // 2
    A, B, Cc = uv[:, 0], uv[:, 1], uv[:, 2]

    def e(P, Q):
        return (Q[:, 0] - P[:, 0]) * (Y - P[:, 1]) - (Q[:, 1] - P[:, 1]) * (X - P[:, 0])

    ar = ((B[:, 0] - A[:, 0]) * (Cc[:, 1] - A[:, 1]) - (B[:, 1] - A[:, 1]) * (Cc[:, 0] - A[:, 0])).astype(np.float32)
    lam = np.stack([e(B, Cc).astype(np.float32) / ar, e(Cc, A).astype(np.float32) / ar, e(A, B).astype(np.float32) / ar], 1)
    return lam, face


def _norm(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def texel_normals(lam, face, ft, nrm, tang, g, dtype=np.float64):
    """The texel transform in `dtype` -> (n_ts [n, 3], frame = (T_i, B, N_i) each [n, 3], ok [n]): N_i = normalize(sum l N),
    T_i = normalize(T' - N_i (N_i . T')), B = w cross(N_i, T_i) with the first corner's w, n_ts = normalize(g . T_i, g . B,
    g . N_i); (0, 0, 1) where g, sum l N or the projected T' is zero (ok = False there)."""
    lam = np.asarray(lam, dtype=dtype)
    vi = np.asarray(ft, dtype=np.int64)[face]
    N, T, g = np.asarray(nrm, dtype=dtype), np.asarray(tang, dtype=dtype), np.asarray(g, dtype=dtype)
    Ni = (lam[:, 0:1] * N[vi[:, 0]] + lam[:, 1:2] * N[vi[:, 1]]) + lam[:, 2:3] * N[vi[:, 2]]
    Tp = (lam[:, 0:1] * T[vi[:, 0], :3] + lam[:, 1:2] * T[vi[:, 1], :3]) + lam[:, 2:3] * T[vi[:, 2], :3]
    w = T[vi[:, 0], 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        ln = _norm(Ni)
        Ni = Ni / ln[:, None]
        Ti = Tp - Ni * _dot(Ni, Tp)[:, None]
        lt = _norm(Ti)
        Ti = Ti / lt[:, None]
        B = w[:, None] * np.cross(Ni, Ti)
        q = np.stack([_dot(g, Ti), _dot(g, B), _dot(g, Ni)], 1)
        lq = _norm(q)
        n_ts = q / lq[:, None]
    ok = (ln > 0) & (lt > 0) & (lq > 0)
    flat = np.asarray([0, 0, 1], dtype=dtype)
    return np.where(ok[:, None], n_ts, flat).astype(dtype), (Ti, B, Ni), ok


# ------------------------------------------------------------------------------------------------ the bytes
def encode(n_ts, dtype=np.float64):
    """byte = round(255 (0.5 n + 0.5)), ties to even, every operation in `dtype` (float32: the kernel's own bytes)."""
    n = np.asarray(n_ts, dtype=dtype)
    return np.clip(np.rint(dtype(255) * (dtype(0.5) * n + dtype(0.5))), 0, 255).astype(np.uint8)


def decode(img):
    """byte / 255 * 2 - 1 (glTF 2.0 section 3.9.3), not renormalised."""
    return np.asarray(img, dtype=np.float64) / 255.0 * 2.0 - 1.0
