"""TEST INFRASTRUCTURE ONLY: numpy restatement of the ray generator (`raydirs_kernel` of csrc/raymarch.hip) with a rigorous
per-element enclosure of what a correct fp32 evaluation may return, the exact classes of its slab test, and the cameras that
tests/test_raydirs_cpu.py (no GPU) and tests/test_hip_raydirs.py (the kernel) share.

Semantics (the header of csrc/raymarch.hip):
  origin     o = campos / volradius
  direction  d = normalize(row0 * px + row1 * py + row2),  (px, py) = ((pixel - princpt) / focal),  normalize(v) = v * rsqrt(v . v)
  t-range    per axis i the candidates (-1 - o_i) / d_i and (1 - o_i) / d_i; tmin = fmax_i fmin(pair), tmax = fmin_i fmax(pair) with the
             NaN-DROPPING fminf / fmaxf (np.fmin / np.fmax, not np.minimum); tmin is clamped to 0, tmax is not clamped

What `bound` assumes of the build, and where that comes from:
  u = 2^-24, round to nearest; every +, -, * and fma rounds once.
  csrc/build.py compiles with `-O3` and no fast-math, reciprocal-math or unsafe-math flag (FLAGS, EXTRA_FLAGS is empty), so
    - fp32 division is correctly rounded (hipcc's default; an approximate divide needs -ffast-math or
      -fno-hip-fp32-correctly-rounded-divide-sqrt, neither of which is passed) and a / d is not rewritten as a * (1 / d);
    - sums are not re-associated, but a product may be contracted into the following addition (clang's default for HIP):
      a sum of k terms carries at most k roundings on every term, with or without contraction -> gamma_k = k u / (1 - k u);
  rsqrtf is within 2 ulp (the figure DESIGN.md section 7 uses for the device library) = 4 u relative.

Derivation.  o, (pixel - princpt) / focal and the numerators -1 - o, 1 - o are single correctly rounded operations on fp32 values (no
product in front of an addition: nothing to contract), so they are computed here in numpy fp32 and are EXACT statements of what the
kernel holds.  From there, in float64:
  D_j = R_0j px + R_1j py + R_2j            computed dhat_j = D_j + delta_j,  |delta_j| <= gamma_3 (|R_0j px| + |R_1j py| + |R_2j|)
  shat = sum dhat_j^2 (1 + theta_3), inv = shat^-1/2 (1 + 4 u), out_j = dhat_j inv (1 + u)
                                            = g_j(dhat) (1 + eta),  g_j(d) = d_j / |d|,  |eta| <= RHO = (1 - gamma_3)^-1/2 (1 + 4u)(1 + u) - 1
  g_j is increasing in d_j and, for fixed d_j, monotone in the sum of the other squares: its range over the box of dhat is
  attained at corners, which gives the enclosure [dlo_j, dhi_j] of out_j without a first-order expansion.
  A component whose three terms all vanish (|R_0j px| + |R_1j py| + |R_2j| = 0) has delta_j = 0: the kernel holds an exact zero there,
  of either sign, and the enclosure is [0, 0].
  The unit-length residual |sum out_j^2 - 1| <= 2 RHO + RHO^2 follows from the same line (sum g_j^2 = 1).
t-range in interval form: a candidate is ONE correctly rounded division fl(a / out_i) of the exact numerator a by the kernel's own
direction component, which lies in [dlo_i, dhi_i] (an interval that does not contain 0 unless it is [0, 0]; `bound` refuses a case
where it straddles 0).  a / d is monotone in d, rounding is monotone, so fl(a / out_i) lies between the fp32 roundings of the two
end quotients.  fmin, fmax and the clamp are monotone in every argument, so they are applied to the lower ends and to the upper
ends.  A huge discarded candidate (a component near 0) never enters the winner's enclosure this way.
An exact-zero component gives a / (+-0) = +-inf, or NaN where a = 0; the sign of the zero is not decided by the contract (it
depends on contraction and on the signs of the vanishing products), so every sign assignment of the zero components is a
SCENARIO with its own enclosure, and a pixel's (tmin, tmax) must lie inside one scenario's enclosure, both values in the same one.

Exact classes of a pixel, per axis i whose direction component is an exact zero (`classes`; checked with no tolerance by
`class_violations`, separately from the enclosure):
  (a) |o_i| < 1   the pair is (-inf, +inf) for either sign of the zero: the axis drops out, the pixel is decided by the other axes.
  (b) |o_i| > 1   both candidates are the same infinity: the ray misses - tmin > tmax or tmax < 0.  Not a value: +0 gives
                  tmax = -inf, -0 gives tmin = +inf.
  (c) |o_i| = 1   one candidate is 0 / 0 = NaN and is dropped; the other is (+-2) / (+-0), an infinity, and becomes BOTH the
                  axis' fmin and its fmax.  So no NaN comes out and the ray misses as in (b): with +0 tmax = -inf and tmin is the
                  clamped enclosure of the remaining axes; with -0 tmin = +inf and tmax is that of the remaining axes.  (The ray
                  lies in a face plane of the volume.  A NaN-PROPAGATING min / max returns NaN for both values instead.)
  (d) camera inside the volume (|o_i| < 1 for all i): the two candidates of every axis have opposite signs, tmin clamps to 0.0 exactly.
  (e) raypos is bit-exact: one correctly rounded division.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149            # fp32 subnormal spacing: absolute slack for a result that underflows
E64 = 2.0 ** -48              # the float64 evaluation of the bound itself (a handful of 2^-53 roundings)
RSQRT_ULPS = 2.0


def gamma(k):
    return k * U / (1.0 - k * U)


RHO = (1.0 - gamma(3)) ** -0.5 * (1.0 + RSQRT_ULPS * 2.0 * U) * (1.0 + U) - 1.0 + E64
UNIT_RESIDUAL = 2.0 * RHO + RHO * RHO + 8 * 2.0 ** -53     # + the float64 sum of three squares of fp32 values

FAULTS = ("rot_transposed", "focal_swapped", "princpt_swapped", "hw_swapped", "camera0", "no_volradius", "no_normalise",
          "tmin_unclamped", "tmax_clamped", "nan_propagating", "rsqrt11")


def pixel_grid(N, H, W, dtype=np.float32):
    """[N, H, W, 2] (x, y) = (w, h): what the kernel takes when its `pixelcoords` pointer is null."""
    ys, xs = np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype), indexing="ij")
    return np.broadcast_to(np.stack([xs, ys], -1)[None], (N, H, W, 2)).copy()


def _operands(viewpos, viewrot, focal, princpt, pixelcoords, hw, T):
    vp, rot = np.asarray(viewpos, np.float32), np.asarray(viewrot, np.float32).reshape(-1, 3, 3)
    f, pp = np.asarray(focal, np.float32), np.asarray(princpt, np.float32)
    N = vp.shape[0]
    pc = pixel_grid(N, hw[0], hw[1]) if pixelcoords is None else np.asarray(pixelcoords, np.float32)
    return vp.astype(T), rot.astype(T), f.astype(T), pp.astype(T), pc.astype(T)


def rays(viewpos, viewrot, focal, princpt, pixelcoords, volradius, dtype=np.float64, hw=None, fault=None):
    """-> (raypos [N,H,W,3], raydir [N,H,W,3], tminmax [N,H,W,2]) evaluated in `dtype` (float64: the reference; float32: the
    kernel's arithmetic without contraction) from the fp32 operands.  pixelcoords None: the integer grid of hw = (H, W).
    `fault`: one of FAULTS, the injected mistakes of tests/test_raydirs_cpu.py."""
    T = np.dtype(dtype).type
    vp, rot, f, pp, pc = _operands(viewpos, viewrot, focal, princpt, pixelcoords, hw, T)
    assert fault is None or fault in FAULTS, fault
    if fault == "rot_transposed":
        rot = np.ascontiguousarray(rot.transpose(0, 2, 1))
    if fault == "focal_swapped":
        f = f[:, ::-1]
    if fault == "princpt_swapped":
        pp = pp[:, ::-1]
    if fault == "hw_swapped":
        pc = pc[..., ::-1]
    if fault == "camera0":
        vp, rot, f, pp = (np.broadcast_to(a[:1], a.shape) for a in (vp, rot, f, pp))
    N, H, W = pc.shape[:3]
    with np.errstate(all="ignore"):
        o = vp / (T(1) if fault == "no_volradius" else T(volradius))
        px = (pc[..., 0] - pp[:, None, None, 0]) / f[:, None, None, 0]
        py = (pc[..., 1] - pp[:, None, None, 1]) / f[:, None, None, 1]
        d = (rot[:, None, None, 0, :] * px[..., None] + rot[:, None, None, 1, :] * py[..., None]) + rot[:, None, None, 2, :]
        s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        inv = T(1) / np.sqrt(s)
        if fault == "rsqrt11":          # an approximate reciprocal square root: 11 significant bits
            m, e = np.frexp(inv)
            inv = np.ldexp(np.floor(m * 2048.0) / 2048.0, e).astype(T)
        if fault != "no_normalise":
            d = d * inv[..., None]
        t1, t2 = (T(-1) - o)[:, None, None, :] / d, (T(1) - o)[:, None, None, :] / d
        lo_of, hi_of = (np.minimum, np.maximum) if fault == "nan_propagating" else (np.fmin, np.fmax)
        lo, hi = lo_of(t1, t2), hi_of(t1, t2)
        tmin = hi_of(lo[..., 0], hi_of(lo[..., 1], lo[..., 2]))
        tmax = lo_of(hi[..., 0], lo_of(hi[..., 1], hi[..., 2]))
        if fault != "tmin_unclamped":
            tmin = hi_of(tmin, T(0))
        if fault == "tmax_clamped":
            tmax = hi_of(tmax, T(0))
    raypos = np.ascontiguousarray(np.broadcast_to(o[:, None, None, :], (N, H, W, 3)))
    return raypos, np.ascontiguousarray(d), np.stack([tmin, tmax], -1)


class Bound:
    """raypos [N,H,W,3] fp32 (exact); dlo, dhi [N,H,W,3] float64; tlo, thi [S,N,H,W,2] float64, one enclosure of (tmin, tmax) per
    sign scenario of the exact-zero components (end points are fp32 values or infinities); zero [N,H,W,3]; o [N,3] fp32."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _t_enclosures(a1, a2, dlo, dhi, zero, signs, drop=None):
    """Enclosure [.., 2] (lower ends), [.., 2] (upper ends) of (clamped tmin, tmax).  a1, a2 [N,1,1,3] exact numerators (float64 of
    fp32), [dlo, dhi] the direction enclosure, zero = exact-zero components with the sign signs[k] (+-1) on axis k, drop = axes left
    out of the test altogether (they contribute (-inf, +inf))."""
    inf = math.inf
    with np.errstate(all="ignore"):
        ends = []
        for a in (a1, a2):
            a = np.broadcast_to(a, dlo.shape)
            qa, qb = a / np.where(zero, 1.0, dlo), a / np.where(zero, 1.0, dhi)
            cl = np.nextafter(np.minimum(qa, qb), -inf).astype(np.float32).astype(np.float64)   # rounding is monotone
            ch = np.nextafter(np.maximum(qa, qb), inf).astype(np.float32).astype(np.float64)
            z = np.where(a == 0, np.nan, np.sign(a) * np.asarray(signs, np.float64) * inf)      # a / (+-0)
            ends.append((np.where(zero, z, cl), np.where(zero, z, ch)))
        (l1, h1), (l2, h2) = ends
        Ll, Lh = np.fmin(l1, l2), np.fmin(h1, h2)            # the axis' fmin: lower / upper end
        Hl, Hh = np.fmax(l1, l2), np.fmax(h1, h2)            # the axis' fmax
        if drop is not None:
            Ll, Lh = np.where(drop, -inf, Ll), np.where(drop, -inf, Lh)
            Hl, Hh = np.where(drop, inf, Hl), np.where(drop, inf, Hh)
        tmin_l, tmin_h = np.maximum(Ll.max(-1), 0.0), np.maximum(Lh.max(-1), 0.0)
        tmax_l, tmax_h = Hl.min(-1), Hh.min(-1)
    return np.stack([tmin_l, tmax_l], -1), np.stack([tmin_h, tmax_h], -1)


def bound(viewpos, viewrot, focal, princpt, pixelcoords, volradius, hw=None) -> Bound:
    """The enclosure of a correct fp32 evaluation (module docstring).  Raises ValueError for a case it cannot decide: a direction
    component whose enclosure straddles 0 without being an exact zero, or a direction that may vanish."""
    vp, rot, f, pp, pc = _operands(viewpos, viewrot, focal, princpt, pixelcoords, hw, np.float32)
    N, H, W = pc.shape[:3]
    o32 = vp / np.float32(volradius)
    px32 = (pc[..., 0] - pp[:, None, None, 0]) / f[:, None, None, 0]
    py32 = (pc[..., 1] - pp[:, None, None, 1]) / f[:, None, None, 1]
    if not (np.isfinite(o32).all() and np.isfinite(px32).all() and np.isfinite(py32).all()):
        raise ValueError("non-finite camera")
    R, px, py = rot.astype(np.float64), px32.astype(np.float64)[..., None], py32.astype(np.float64)[..., None]
    t0, t1, t2 = R[:, None, None, 0, :] * px, R[:, None, None, 1, :] * py, np.broadcast_to(R[:, None, None, 2, :], (N, H, W, 3))
    D, A = t0 + t1 + t2, np.abs(t0) + np.abs(t1) + np.abs(t2)
    zero = A == 0
    e = np.where(zero, 0.0, (gamma(3) + E64) * A + 3 * TINY)
    lo, hi = D - e, D + e
    if bool(((lo < 0) & (hi > 0)).any()):
        raise ValueError("a direction component straddles 0 without being an exact zero")
    sqlo, sqhi = np.minimum(lo * lo, hi * hi), np.maximum(lo * lo, hi * hi)
    if float(sqlo.sum(-1).min()) < 2.0 ** -60:
        raise ValueError("the direction may vanish")
    dlo, dhi = np.empty_like(D), np.empty_like(D)
    for j in range(3):
        k = [i for i in range(3) if i != j]
        r2lo, r2hi = sqlo[..., k].sum(-1), sqhi[..., k].sum(-1)
        gu = hi[..., j] / np.sqrt(hi[..., j] ** 2 + np.where(hi[..., j] >= 0, r2lo, r2hi))
        gl = lo[..., j] / np.sqrt(lo[..., j] ** 2 + np.where(lo[..., j] >= 0, r2hi, r2lo))
        dhi[..., j] = np.where(gu >= 0, gu * (1 + RHO), gu * (1 - RHO)) + TINY
        dlo[..., j] = np.where(gl >= 0, gl * (1 - RHO), gl * (1 + RHO)) - TINY
    dlo, dhi = np.where(zero, 0.0, dlo), np.where(zero, 0.0, dhi)
    if bool((~zero & (dlo <= 0) & (dhi >= 0)).any()):
        raise ValueError("a normalised component straddles 0 without being an exact zero")
    a1 = (np.float32(-1) - o32).astype(np.float64)[:, None, None, :]
    a2 = (np.float32(1) - o32).astype(np.float64)[:, None, None, :]
    axes = [k for k in range(3) if bool(zero[..., k].any())]
    tlo, thi = [], []
    for bits in range(1 << len(axes)):
        signs = [1.0, 1.0, 1.0]
        for i, k in enumerate(axes):
            if bits >> i & 1:
                signs[k] = -1.0
        l, h = _t_enclosures(a1, a2, dlo, dhi, zero, signs)
        tlo.append(l)
        thi.append(h)
    raypos = np.ascontiguousarray(np.broadcast_to(o32[:, None, None, :], (N, H, W, 3)))
    return Bound(raypos=raypos, dlo=dlo, dhi=dhi, tlo=np.stack(tlo), thi=np.stack(thi), zero=zero, o=o32, a1=a1, a2=a2)


def trange_of(raypos, raydir):
    """(clamped tmin, tmax) [.., 2] fp32 from the kernel's OWN fp32 origin and direction: every candidate is one correctly rounded
    division of two values that are known exactly here, fmin / fmax / the clamp round nothing, and the sign of an exact zero is in
    `raydir` itself - so the kernel's t-range equals this one in value (the clamp may return either zero for tmin = -0)."""
    o, d = np.asarray(raypos, np.float32), np.asarray(raydir, np.float32)
    with np.errstate(all="ignore"):
        t1, t2 = (np.float32(-1) - o) / d, (np.float32(1) - o) / d
        lo, hi = np.fmin(t1, t2), np.fmax(t1, t2)
        tmin = np.fmax(np.fmax(lo[..., 0], np.fmax(lo[..., 1], lo[..., 2])), np.float32(0))
        tmax = np.fmin(hi[..., 0], np.fmin(hi[..., 1], hi[..., 2]))
    return np.stack([tmin, tmax], -1)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def violations(B: Bound, raypos, raydir, tminmax) -> dict:
    """name -> bool mask of the elements (raypos, raydir: [N,H,W,3]; tminmax, unit: [N,H,W]) that leave the contract.  A NaN is
    outside every enclosure."""
    rp, rd, tm = (np.asarray(x, np.float32) for x in (raypos, raydir, tminmax))
    rd64, tm64 = rd.astype(np.float64), tm.astype(np.float64)
    inside = (tm64[None] >= B.tlo) & (tm64[None] <= B.thi)                 # [S,N,H,W,2]
    unit = np.abs((rd64 * rd64).sum(-1) - 1.0)
    return {"raypos": _bits(rp) != _bits(B.raypos),
            "raydir": ~((rd64 >= B.dlo) & (rd64 <= B.dhi)),
            "tminmax": ~inside.all(-1).any(0),
            "unit": ~(unit <= UNIT_RESIDUAL)}


def share(B: Bound, raydir, tminmax) -> float:
    """Largest |value - centre| / half-width over the elements whose enclosure is finite and not a point: 1.0 is the edge."""
    rd64, tm64 = np.asarray(raydir, np.float64), np.asarray(tminmax, np.float64)
    worst = 0.0
    with np.errstate(all="ignore"):
        sel = (B.dhi > B.dlo)
        if sel.any():
            worst = float((np.abs(rd64 - (B.dhi + B.dlo) / 2) / ((B.dhi - B.dlo) / 2))[sel].max())
        inside = ((tm64[None] >= B.tlo) & (tm64[None] <= B.thi)).all(-1, keepdims=True)
        sel = inside & np.isfinite(B.tlo) & np.isfinite(B.thi) & (B.thi > B.tlo)
        if sel.any():
            r = np.abs(tm64[None] - (B.thi + B.tlo) / 2) / ((B.thi - B.tlo) / 2)
            worst = max(worst, float(r[sel].max()))
    return worst


def classes(viewpos, viewrot, focal, princpt, pixelcoords, volradius, hw=None) -> dict:
    """The exact classes in arithmetic on the operands (not through `bound`): zero [N,H,W,3] = every term of the component
    vanishes; a, b, c [N,H,W,3] = such an axis with |o| < 1, > 1, = 1; d [N] = camera inside the volume."""
    vp, rot, f, pp, pc = _operands(viewpos, viewrot, focal, princpt, pixelcoords, hw, np.float32)
    o = np.abs(vp / np.float32(volradius))
    px = ((pc[..., 0] - pp[:, None, None, 0]) / f[:, None, None, 0])[..., None]
    py = ((pc[..., 1] - pp[:, None, None, 1]) / f[:, None, None, 1])[..., None]
    zero = ((rot[:, None, None, 0, :] == 0) | (px == 0)) & ((rot[:, None, None, 1, :] == 0) | (py == 0)) & (rot[:, None, None, 2, :] == 0)
    ob = o[:, None, None, :]
    return {"zero": zero, "a": zero & (ob < 1), "b": zero & (ob > 1), "c": zero & (ob == 1), "d": (o < 1).all(-1)}


def class_violations(B: Bound, C: dict, raypos, raydir, tminmax) -> dict:
    """class -> bool mask [N,H,W] of the pixels that break the class' statement (module docstring); no tolerance anywhere."""
    rp, rd, tm = (np.asarray(x, np.float32) for x in (raypos, raydir, tminmax))
    tm64 = tm.astype(np.float64)
    tmin, tmax = tm64[..., 0], tm64[..., 1]
    nan = np.isnan(tm64).any(-1)
    miss = (tmin > tmax) | (tmax < 0)
    has = {k: C[k].any(-1) for k in "abc"}
    out = {"zero": (C["zero"] & (rd != 0)).any(-1)}
    # the enclosure of the axes that are NOT an exact zero, computed without them
    l, h = _t_enclosures(B.a1, B.a2, B.dlo, B.dhi, np.zeros_like(C["zero"]), [1.0, 1.0, 1.0], drop=C["zero"])
    rest = (tm64 >= l) & (tm64 <= h)                                        # [N,H,W,2]
    out["a"] = has["a"] & ~has["b"] & ~has["c"] & ~rest.all(-1)
    out["b"] = has["b"] & (nan | ~miss)
    face = (np.isneginf(tmax) & rest[..., 0]) | (np.isposinf(tmin) & rest[..., 1])
    out["c"] = has["c"] & (nan | ~miss | (~has["b"] & ~face))
    out["d"] = C["d"][:, None, None] & ~(tmin == 0.0)
    out["e"] = (_bits(rp) != _bits(B.raypos)).any(-1)
    return out


def population(C: dict) -> dict:
    return {"zero": int(C["zero"].any(-1).sum()), "a": int(C["a"].any(-1).sum()), "b": int(C["b"].any(-1).sum()),
            "c": int(C["c"].any(-1).sum()), "d": int(C["d"].sum())}


# ------------------------------------------------------------------------------------------------ the cameras
def _rot(yaw, pitch=0.0):
    """World-to-camera rotation (rows = the camera's axes in the world), fp32: pitch about x after yaw about y."""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return (Rx @ Ry).astype(np.float32)


def _centre(R, c):
    """Camera centre R^T c for the camera-frame offset c (c = (0, 0, -dist): the camera looks at the origin), fp32."""
    return (R.astype(np.float64).T @ np.asarray(c, np.float64)).astype(np.float32)


def _case(viewpos, viewrot, focal, princpt, H, W, volradius=1.0, pixelcoords=None):
    vp = np.asarray(viewpos, np.float32).reshape(-1, 3)
    N = vp.shape[0]
    pc = pixel_grid(N, H, W) if pixelcoords is None else np.ascontiguousarray(pixelcoords, dtype=np.float32)
    return dict(viewpos=vp, viewrot=np.asarray(viewrot, np.float32).reshape(N, 3, 3), focal=np.asarray(focal, np.float32).reshape(N, 2),
                princpt=np.asarray(princpt, np.float32).reshape(N, 2), pixelcoords=pc, volradius=float(volradius))


NZ = -0.0
EYE = np.eye(3, dtype=np.float32)
# looks down +z like EYE with x and y kept, but every vanishing entry is a NEGATIVE zero and y is mirrored: the exact-zero
# components of its rays come out as -0 where EYE's are +0
EYE_NEG = np.array([[1.0, NZ, NZ], [NZ, -1.0, NZ], [NZ, NZ, 1.0]], np.float32)


def _generic_batch3():
    Rs = [_rot(0.3, 0.2), _rot(-0.8, -0.4), _rot(2.1, 0.1)]
    cs = [_centre(Rs[0], (0.05, 0.1, -3.0)), _centre(Rs[1], (-0.1, 0.02, -2.5)), _centre(Rs[2], (0.0, -0.15, -4.0))]
    return _case(cs, Rs, [[38.0, 41.0], [30.0, 36.5], [45.25, 33.0]], [[13.3, 6.7], [12.1, 5.9], [14.6, 7.2]], 13, 27)


def _principal_cross():
    Rs = [_rot(0.3), EYE, EYE_NEG]
    cs = [_centre(Rs[0], (0, 0, -3.0)), (0, 0, -3.0), (0, 0, -3.0)]
    return _case(cs, Rs, [[24.0, 24.0]] * 3, [[8.0, 8.0]] * 3, 17, 17)


def _axis_on_face():
    return _case([(0, 1, -3.0), (2, 0, -3.0), (0, 1, -3.0), (-1, 0, -3.0)], [EYE, EYE, EYE_NEG, EYE_NEG],
                 [[24.0, 24.0]] * 4, [[8.0, 8.0]] * 4, 17, 17)


def _inside():
    R = _rot(0.3)
    return _case([_centre(R, (0, 0.1, -0.9)), (0, 0, 0)], [R, _rot(-0.8, 0.3)], [[22.4, 22.4]] * 2, [[8.0, 8.0], [7.5, 8.5]], 16, 16)


def _looking_away():
    R = _rot(0.3 + math.pi)
    return _case([_centre(_rot(0.3), (0, 0.1, -3.0))], [R], [[22.4, 22.4]], [[8.0, 8.0]], 16, 16)


def _grazing():
    R = _rot(0.5, 0.1)
    return _case([_centre(R, (0, 0, -30.0))], [R], [[300.0, 300.0]], [[15.0, 3.5]], 8, 31)


def _one_pixel():
    R = _rot(0.3, 0.2)
    return _case([_centre(R, (0, 0, -3.0))], [R], [[1.5, 1.25]], [[0.25, -0.5]], 1, 1)


def _package():
    from topia_xl_amd import raymarch
    return raymarch


def _subsampled_eval():
    m = _package().RayMarcher(13, 27, 1.0)
    pc = m._pixel_coords(2, 2, "cpu").numpy()
    Rs = [_rot(0.3, 0.2), _rot(-0.8, -0.4)]
    return _case([_centre(Rs[0], (0, 0.1, -3.0)), _centre(Rs[1], (0.1, 0, -2.5))], Rs, [[38.0, 41.0], [30.0, 36.5]],
                 [[13.3, 6.7], [12.1, 5.9]], pc.shape[1], pc.shape[2], pixelcoords=pc)


def _subsampled_train():
    import torch
    rm = _package()
    state = torch.random.get_rng_state()
    try:
        torch.manual_seed(20)
        pc = rm.training_pixel_coords(rm.base_pixel_coords(13, 27), 3, 3).numpy()
    finally:
        torch.random.set_rng_state(state)
    Rs = [_rot(0.3, 0.2), _rot(-0.8, -0.4), _rot(2.1, 0.1)]
    cs = [_centre(Rs[0], (0, 0.1, -3.0)), _centre(Rs[1], (0.1, 0, -2.5)), _centre(Rs[2], (0, 0, -4.0))]
    return _case(cs, Rs, [[38.0, 41.0], [30.0, 36.5], [45.25, 33.0]], [[13.3, 6.7], [12.1, 5.9], [14.6, 7.2]], pc.shape[1], pc.shape[2],
                 pixelcoords=pc)


def _volradius(vr):
    def make():
        Rs = [_rot(0.3, 0.2), np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)]      # the second: the preview camera's rotation
        cs = [_centre(Rs[0], (0.05 * vr, 0.1 * vr, -3.0 * vr)), (0.0, 0.0, 5.0 * vr)]
        return _case(cs, Rs, [[38.0, 41.0], [40.0, 40.0]], [[13.3, 6.7], [13.5, 6.5]], 13, 27, volradius=vr)
    return make


CASES = {
    "generic_batch3": _generic_batch3, "principal_cross": _principal_cross, "axis_on_face": _axis_on_face, "inside": _inside,
    "looking_away": _looking_away, "grazing": _grazing, "one_pixel": _one_pixel, "subsampled_eval": _subsampled_eval,
    "subsampled_train": _subsampled_train, "volradius_100": _volradius(100.0), "volradius_10000": _volradius(10000.0),
}


def case(name) -> dict:
    return CASES[name]()


def operands(c: dict):
    return c["viewpos"], c["viewrot"], c["focal"], c["princpt"], c["pixelcoords"], c["volradius"]
