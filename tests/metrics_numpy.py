"""Rules N1-N3 and S1-S5 of include/primx_hip.h "Quality metrics" and the definitions of `metrics.compare_points`, restated in
numpy: in float32 line by line as csrc/metrics.hip evaluates them (numpy never contracts a product into a sum), and in float64.

`nearest` walks the rows of `a` in slabs so that no n x m matrix larger than `SLAB` pairs exists at once; `argmin` returns the
FIRST minimum, which is what the strict `<` of rule N2 keeps; a NaN or +inf pair is set to +inf first and so never wins, and a row
without a finite pair keeps (+inf, 0).
"""
import math

import numpy as np

SLAB = 1 << 22


def nearest(a, b, dtype=np.float32):
    """a [n, 3], b [m, 3] -> (dist [n] dtype, idx [n] int32) by N1-N3 in `dtype`."""
    a, b = np.asarray(a, dtype=dtype).reshape(-1, 3), np.asarray(b, dtype=dtype).reshape(-1, 3)
    n, m = len(a), len(b)
    assert m >= 1
    dist, idx = np.empty(n, dtype=dtype), np.zeros(n, dtype=np.int32)
    rows = max(1, SLAB // m)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, n, rows):
            s = a[lo:lo + rows]
            dx, dy, dz = (s[:, None, k] - b[None, :, k] for k in range(3))                 # N1
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(d2 < np.inf, d2, dtype(np.inf))                                   # N2: NaN and +inf never win
            j = np.argmin(d2, axis=1)                                                       #     the first minimum
            best = d2[np.arange(len(s)), j]
            idx[lo:lo + rows] = np.where(best < np.inf, j, 0)
            dist[lo:lo + rows] = np.sqrt(best)                                              # N3
    return dist, idx


def stats(dist, idx=None, na=None, nb=None, thresholds=()):
    """S1-S5 -> a list of 4 + T Python floats; the sums are exact (`math.fsum` of the float64 terms), which is what the kernel's
    fixed-order float64 sums are held against."""
    dist = np.asarray(dist, dtype=np.float32)
    d = dist.astype(np.float64)
    out = [math.fsum(d), math.fsum(d * d), float(np.fmax.reduce(dist, initial=np.float32(0.0))) if len(dist) else 0.0, 0.0]
    if na is not None and nb is not None:
        na, nbk = np.asarray(na, dtype=np.float32), np.asarray(nb, dtype=np.float32)[np.asarray(idx, dtype=np.int64)]
        dot = (na[:, 0] * nbk[:, 0] + na[:, 1] * nbk[:, 1]) + na[:, 2] * nbk[:, 2]           # S4: fp32
        out[3] = math.fsum(np.abs(dot).astype(np.float64))
    out += [float(np.count_nonzero(dist <= np.float32(t))) for t in thresholds]              # S5: an fp32 compare
    return out


def abs_sums(dist, idx=None, na=None, nb=None):
    """Sum of |x| of the three sums of `stats` (all terms are non-negative: the sums themselves) - the scale of their bound."""
    s = stats(dist, idx, na, nb)
    return [s[0], s[1], s[3]]


def report(sa, sb, n, m, thresholds, normals):
    """The definitions of `compare_points` from two rows of `stats`."""
    acc, comp = sa[0] / n, sb[0] / m
    out = {"accuracy": acc, "completeness": comp, "chamfer_l1": (acc + comp) / 2, "chamfer_l2": sa[1] / n + sb[1] / m,
           "hausdorff": max(sa[2], sb[2]), "precision": {}, "recall": {}, "fscore": {}}
    for t, tau in enumerate(thresholds):
        p, r = sa[4 + t] / n, sb[4 + t] / m
        out["precision"][tau], out["recall"][tau] = p, r
        out["fscore"][tau] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    if normals:
        out["normal_consistency"] = (sa[3] / n + sb[3] / m) / 2
    return out


def compare_points(a, b, na=None, nb=None, thresholds=(0.01, 0.02, 0.05), dtype=np.float32):
    """`metrics.compare_points` with the nearest-neighbour search in `dtype`.  In float64 the distances are NOT rounded to fp32
    before they are summed and compared: that is the truth the kernel's numbers are held against."""
    normals = na is not None and nb is not None
    dab, iab = nearest(a, b, dtype)
    dba, iba = nearest(b, a, dtype)
    if dtype == np.float32:
        sa = stats(dab, iab, na if normals else None, nb if normals else None, thresholds)
        sb = stats(dba, iba, nb if normals else None, na if normals else None, thresholds)
    else:
        sa, sb = _stats64(dab, iab, na, nb, thresholds, normals), _stats64(dba, iba, nb, na, thresholds, normals)
    return report(sa, sb, len(dab), len(dba), tuple(thresholds), normals)


def _stats64(d, idx, na, nb, thresholds, normals):
    out = [math.fsum(d), math.fsum(d * d), float(d.max()) if len(d) else 0.0, 0.0]
    if normals:
        na, nbk = np.asarray(na, dtype=np.float64), np.asarray(nb, dtype=np.float64)[idx]
        out[3] = math.fsum(np.abs((na * nbk).sum(1)))
    return out + [float(np.count_nonzero(d <= t)) for t in thresholds]


def two_planes(k=8, h=0.125):
    """Two coincident k x k lattices of spacing 1/8 in z = 0 and z = h, normals +z: every nearest distance is exactly h."""
    g = np.arange(k, dtype=np.float32) / np.float32(8.0) - np.float32(0.5)
    X, Y = np.meshgrid(g, g, indexing="ij")
    a = np.stack([X.ravel(), Y.ravel(), np.zeros(k * k, dtype=np.float32)], 1).astype(np.float32)
    b = a.copy()
    b[:, 2] = np.float32(h)
    nrm = np.tile(np.float32([0, 0, 1]), (k * k, 1))
    return a, b, nrm, nrm.copy()
