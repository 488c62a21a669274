"""Asset quality metrics on MI355X - SURVEY.md section 8(f) row N9: how far one surface is from another.

Chamfer distance, F-score, Hausdorff distance and normal consistency between two point sets, two meshes, or a mesh and the mesh
extracted from a PrimSDF field.  Neither the reference nor its paper's released code has an evaluation step; the definitions
below are the ones the 3DTopia-XL paper and the reconstruction literature report, stated in `compare_points`.

Kernels (csrc/metrics.hip, rules in include/primx_hip.h "Quality metrics"): `primx_nearest_points` (brute force nearest
neighbour, bitwise deterministic) and `primx_distance_stats` (sums, maximum and threshold counts of the per-point distances in
float64, in a fixed order).  Everything else is plumbing on fit.py: `primx_mesh_surface_points` draws the area-weighted samples
and, with `surface=True`, `primx_mesh_field_query` measures each sample against the other mesh's exact surface.  There is no CPU
path.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _lib, fit, ops
from .fit import _need_cuda

NEAREST_CHUNK = 1024       # points of b per LDS chunk of primx_nearest_points (NN_CHUNK of csrc/metrics.hip)
NEAREST_THREADS = 256      # threads per block; each carries one point of a, and four from NEAREST_WIDE points on (NN_WIDE)
NEAREST_WIDE = 409600
STATS_BLOCKS = 256         # blocks of primx_distance_stats at most (ST_MAXB) ...
STATS_PER_BLOCK = 1024     # ... each over a slice of at least this many elements (ST_PER_BLOCK)
MAX_THRESHOLDS = 8
STATS_WS_BYTES = STATS_BLOCKS * (4 + MAX_THRESHOLDS) * 8
DEFAULT_THRESHOLDS = (0.01, 0.02, 0.05)


def nearest_points_per_thread(n: int) -> int:
    """The points of `a` each thread of primx_nearest_points carries at n points (the results do not depend on it)."""
    return 4 if n >= NEAREST_WIDE else 1


def _points(t, name):
    """[n, 3] -> float32, contiguous.  Shapes are refused (ValueError) before devices are (RuntimeError), on any device."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a HIP device tensor; there is no CPU path")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name} must be [n, 3], got {tuple(t.shape)}")
    return t.float().contiguous()


@ops.on_input_device
def nearest_points(a: torch.Tensor, b: torch.Tensor):
    """a [n, 3], b [m, 3] (m >= 1) -> (dist [n] float32, idx [n] int32): for every point of `a` the distance to the nearest point
    of `b` and its index, the lowest among equals: primx_nearest_points.  A point without a finite pair gets (+inf, 0)."""
    a, b = _points(a, "a"), _points(b, "b")
    n, m = a.shape[0], b.shape[0]
    if m == 0:
        raise ValueError("b has no points")
    _need_cuda("nearest_points", a, b)
    dist = torch.empty(n, dtype=torch.float32, device=a.device)
    idx = torch.empty(n, dtype=torch.int32, device=a.device)
    _lib.check(_lib.load().primx_nearest_points(ops._dev(a, "a", torch.float32) if n else None, n, ops._dev(b, "b", torch.float32), m,
                                                dist.data_ptr() if n else None, idx.data_ptr() if n else None, ops._stream()),
               "primx_nearest_points")
    return dist, idx


@ops.on_input_device
def distance_stats(dist: torch.Tensor, idx: Optional[torch.Tensor] = None, na: Optional[torch.Tensor] = None,
                   nb: Optional[torch.Tensor] = None, thresholds: Sequence[float] = ()) -> torch.Tensor:
    """dist [n] float32, idx [n] int32 (rows of nb), na [n, 3], nb [*, 3], T thresholds (T <= 8) -> float64 [4 + T] on the device:
    (sum of dist, sum of dist^2, max of dist, sum of |na . nb[idx]|, the number of dist <= each threshold): primx_distance_stats.
    Without both normal sets element 3 is 0 and idx is not needed.  Nothing is synchronised or read back."""
    tau = [float(t) for t in thresholds]
    T = len(tau)
    if T > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds (got {T})")
    _need_cuda("distance_stats", *(t for t in (dist, idx, na, nb) if not isinstance(t, torch.Tensor)))
    if dist.dim() != 1:
        raise ValueError(f"dist must be [n], got {tuple(dist.shape)}")
    dist = dist.float().contiguous()
    n, dev = dist.shape[0], dist.device
    normals = na is not None and nb is not None
    if normals:
        if idx is None:
            raise ValueError("normals need idx")
        idx, na, nb = idx.int().contiguous(), _points(na, "na"), _points(nb, "nb")
        if idx.shape != (n,) or na.shape[0] != n or (n and nb.shape[0] == 0):
            raise ValueError(f"idx must be [n] and na [n, 3] with n = {n}, nb non-empty; got {tuple(idx.shape)}, {tuple(na.shape)}, "
                             f"{tuple(nb.shape)}")
    _need_cuda("distance_stats", dist, idx, na, nb)
    out = torch.empty(4 + T, dtype=torch.float64, device=dev)
    ws = torch.empty(STATS_WS_BYTES, dtype=torch.uint8, device=dev)
    p = lambda t, name, dt: ops._dev(t, name, dt) if normals and n else None   # noqa: E731
    _lib.check(_lib.load().primx_distance_stats(
        ops._dev(dist, "dist", torch.float32) if n else None, p(idx, "idx", torch.int32), p(na, "na", torch.float32),
        p(nb, "nb", torch.float32), n, (ctypes.c_float * max(T, 1))(*tau), T, ws.data_ptr(), ws.numel(), out.data_ptr(),
        ops._stream()), "primx_distance_stats")
    return out


def _vf(mesh, dev):
    t = lambda a: torch.as_tensor(a).to(dev)   # noqa: E731
    v, f = (mesh[0], mesh[1]) if isinstance(mesh, (tuple, list)) else (mesh.v, mesh.f)
    return fit._mesh_args(t(v).float(), t(f).int())


def _device_of(mesh):
    v0 = mesh[0] if isinstance(mesh, (tuple, list)) else mesh.v
    return v0.device if isinstance(v0, torch.Tensor) and v0.is_cuda else torch.device("cuda", torch.cuda.current_device())


def face_normals(v: torch.Tensor, f: torch.Tensor, face: torch.Tensor) -> torch.Tensor:
    """[k, 3] fp32: the unit normal (b - a) x (c - a) / |.| of each listed face, the zero vector for a zero-area face (torch)."""
    tri = v[f[face.long()].long()]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    l = n.norm(dim=1, keepdim=True)
    return torch.where(l > 0, n / l, torch.zeros_like(n))


def sample_surface(mesh, n: int, seed: int = 0):
    """mesh: a `mesh.TriMesh`, `MaterialMesh`, `TexturedMesh`, anything with `.v` and `.f`, or a tuple whose first two entries
    are (v, f) -> (pts [n, 3] float32, normals [n, 3] float32, face [n] int32): n area-weighted surface samples drawn with `seed`
    (`fit.surface_uniforms` / `fit.surface_points`: the same numbers on every device) and the unit normal of each sample's face
    (zero for a zero-area face)."""
    dev = _device_of(mesh)
    with torch.cuda.device(dev), torch.no_grad():
        v, f = _vf(mesh, dev)
        pts, face = fit.surface_points(v, f, fit.area_cdf(fit.face_areas(v, f)), fit.surface_uniforms(int(n), seed).to(dev))
        return pts, face_normals(v, f, face), face


def _report(sa: Sequence[float], sb: Sequence[float], n: int, m: int, thresholds: Sequence[float], normals: bool) -> dict:
    """The definitions of `compare_points` from the two rows of primx_distance_stats (host floats)."""
    acc, comp = sa[0] / n, sb[0] / m
    out = {"accuracy": acc, "completeness": comp, "chamfer_l1": 0.5 * (acc + comp), "chamfer_l2": sa[1] / n + sb[1] / m,
           "hausdorff": max(sa[2], sb[2]), "precision": {}, "recall": {}, "fscore": {}}
    for t, tau in enumerate(thresholds):
        p, r = sa[4 + t] / n, sb[4 + t] / m
        out["precision"][tau], out["recall"][tau] = p, r
        out["fscore"][tau] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    if normals:
        out["normal_consistency"] = 0.5 * (sa[3] / n + sb[3] / m)
    return out


def _finish(stats_a, stats_b, n, m, thresholds, normals):
    rows = torch.stack([stats_a, stats_b]).cpu().tolist()                     # the one read-back
    return _report(rows[0], rows[1], n, m, thresholds, normals)


def compare_points(a: torch.Tensor, b: torch.Tensor, na: Optional[torch.Tensor] = None, nb: Optional[torch.Tensor] = None,
                   thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> dict:
    """a [n, 3], b [m, 3] (both non-empty), optional unit normals na [n, 3], nb [m, 3] -> a dict of Python floats.  With d(a->B) the
    distance from each point of `a` to its nearest point of `b`, and d(b->A) likewise:

        accuracy            mean d(a->B)
        completeness        mean d(b->A)
        chamfer_l1          (accuracy + completeness) / 2
        chamfer_l2          mean d(a->B)^2 + mean d(b->A)^2
        hausdorff           max(max d(a->B), max d(b->A))
        precision[tau]      the share of a with d(a->B) <= tau          (a dict keyed by the thresholds as given)
        recall[tau]         the share of b with d(b->A) <= tau
        fscore[tau]         2 P R / (P + R), 0 when P + R = 0
        normal_consistency  (mean |na . nb[nearest]| + mean |nb . na[nearest]|) / 2, only when both normal sets are given

    Papers differ on the factor 1/2 and on squaring: chamfer_l1 is the mean of the two unsquared means, chamfer_l2 the sum of the two
    mean squares.  The default thresholds are this project's choice, in the units of PrimSDF's [-1, 1]^3 domain (0.5 %, 1 % and
    2.5 % of the cube's side).  Two nearest-neighbour searches and two reductions are enqueued; the single synchronisation is the
    read-back of their 2 x (4 + T) float64 results at the end."""
    thresholds = tuple(float(t) for t in thresholds)
    a, b = _points(a, "a"), _points(b, "b")
    if a.shape[0] == 0 or b.shape[0] == 0:
        raise ValueError("both point sets must be non-empty")
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f"at most {MAX_THRESHOLDS} thresholds (got {len(thresholds)})")
    normals = na is not None and nb is not None
    if normals and (tuple(na.shape) != tuple(a.shape) or tuple(nb.shape) != tuple(b.shape)):
        raise ValueError(f"na and nb must have the shapes of a and b, got {tuple(na.shape)} and {tuple(nb.shape)}")
    _need_cuda("compare_points", a, b, na, nb)
    with torch.cuda.device(a.device), torch.no_grad():
        dab, iab = nearest_points(a, b)
        dba, iba = nearest_points(b, a)
        sa = distance_stats(dab, iab, na if normals else None, nb if normals else None, thresholds)
        sb = distance_stats(dba, iba, nb if normals else None, na if normals else None, thresholds)
        return _finish(sa, sb, a.shape[0], b.shape[0], thresholds, normals)


def compare_meshes(mesh_a, mesh_b, n: int = 100_000, seed: int = 0, surface: bool = False,
                   thresholds: Sequence[float] = DEFAULT_THRESHOLDS, accel=None) -> dict:
    """`compare_points` of n area-weighted samples of each mesh (A drawn with `seed`, B with `seed + 1`: `sample_surface`) with
    the sampled faces' normals.  The keys are `compare_points`'s.

    surface=False: sample to nearest sample, the form in which the numbers are published.  A mesh compared with itself does NOT
    give 0 but the sampling spacing (about sqrt(area / n)); distances well above it are meaningful.
    surface=True: each side's samples to the other mesh's exact surface (`fit.mesh_field_query`'s distance and closest face, with
    that face's normal), reduced by the same `primx_distance_stats`.  A mesh compared with itself gives 0 up to the query's fp32
    error.  The query is brute force over the faces and synchronises once per call for its index check.  accel="bvh" (with
    surface=True; it changes nothing otherwise) measures through a `fit.MeshBVH` of each mesh instead, the samples in Morton
    order: the same distances and closest faces bit for bit, so the same dict, at a cost that no longer grows with the faces."""
    thresholds = tuple(float(t) for t in thresholds)
    fit._check_accel(accel)
    dev = _device_of(mesh_a)
    with torch.cuda.device(dev), torch.no_grad():
        pa, na, _ = sample_surface(mesh_a, n, seed)
        pb, nb, _ = sample_surface(mesh_b, n, seed + 1)
        if not surface:
            return compare_points(pa, pb.to(dev), na, nb.to(dev), thresholds)
        if len(thresholds) > MAX_THRESHOLDS:
            raise ValueError(f"at most {MAX_THRESHOLDS} thresholds (got {len(thresholds)})")
        (va, fa), (vb, fb) = _vf(mesh_a, dev), _vf(mesh_b, dev)
        pb, nb = pb.to(dev), nb.to(dev)
        if accel == "bvh":
            dab, face_b, _, _ = fit.MeshBVH(vb, fb).query(pa, sort_points=True)
            dba, face_a, _, _ = fit.MeshBVH(va, fa).query(pb, sort_points=True)
        else:
            dab, face_b, _, _ = fit.mesh_field_query(pa, vb, fb)
            dba, face_a, _, _ = fit.mesh_field_query(pb, va, fa)
        ident = torch.arange(int(n), dtype=torch.int32, device=dev)          # row i of the closest faces' normals belongs to sample i
        sa = distance_stats(dab, ident, na, face_normals(vb, fb, face_b), thresholds)
        sb = distance_stats(dba, ident, nb, face_normals(va, fa, face_a), thresholds)
        return _finish(sa, sb, int(n), int(n), thresholds, True)


def compare_to_field(mesh, field, resolution: int = 256, **kw) -> dict:
    """`compare_meshes(mesh, mesh.extract_mesh(field, resolution), **kw)`: the round-trip number of `fit.mesh_to_primitives` -
    how far the surface extracted from the fitted field is from the mesh it was fitted to.  `mesh` must be in the field's
    coordinates (the normalised vertices, `info['v']` of `mesh_to_primitives`)."""
    from .mesh import extract_mesh
    return compare_meshes(mesh, extract_mesh(field, resolution), **kw)
