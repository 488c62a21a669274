"""Quality metrics on the MI355X: `primx_nearest_points` bit for bit against the float32 restatement of rules N1-N3
(tests/metrics_numpy.py) and within its derived bound of float64, `primx_distance_stats` (exact counts and maximum, sums within
the bound of any summation order, equal bits on every run), the wrappers of metrics.py on cases with known answers, and the
footprint and stream-order case of both entry points.

The module imports without a GPU: it registers its stream-order case in the table of tests/test_hip_streams.py at import (that
file stays as it is) and runs it here; the point sets below are numpy and serve tests/test_metrics_cpu.py too.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import metrics_numpy as MN
from tests import streamorder as so
from tests import test_hip_streams as TS
from tests.test_hip_normalmap import E, mods  # noqa: F401  (fixtures: the built package; one side stream of this module's own)
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STREAM_CASE = "quality_metrics"
C, B, WIDE = 1024, 256, 409600           # metrics.NEAREST_CHUNK, NEAREST_THREADS, NEAREST_WIDE (checked against the module below)
SLICE = 256 * 1024                       # metrics.STATS_BLOCKS * metrics.STATS_PER_BLOCK: above it the slices grow past 1024
U = 2.0 ** -24                           # fp32 unit roundoff
REL = 4 * U                              # rule N1-N3 against float64: one rounding in each subtraction (1 u on dx), one per product
#                                          (dx^2: 2 u + 1 u), two in the sum of the non-negative terms (5 u on d2), the square root halves
#                                          it (2.5 u) and rounds once more: 3.5 u <= 4 u, relative to the float64 nearest distance


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def MT(mods):
    from topia_xl_amd import metrics
    assert (metrics.NEAREST_CHUNK, metrics.NEAREST_THREADS, metrics.NEAREST_WIDE) == (C, B, WIDE)
    assert metrics.STATS_BLOCKS * metrics.STATS_PER_BLOCK == SLICE
    assert [metrics.nearest_points_per_thread(n) for n in (1, WIDE - 1, WIDE, WIDE + 1)] == [1, 1, 4, 4]
    return metrics


# ------------------------------------------------------------------------------------------------ 1. nearest, bit for bit
def _nearest_sets():
    """name -> (a, b): every (n, m) the kernel takes another path at, ties inside and across an LDS chunk, and non-finite input."""
    rng = np.random.default_rng(5)
    u = lambda n: _f32(rng.uniform(-1, 1, (n, 3)))   # noqa: E731
    out = {}
    for n, m in ((1, 1), (1, 257), (63, 1), (64, 64), (65, C + 1), (1000, 3 * C + 5), (4099, 10007)):
        out[f"{n} x {m}"] = (u(n), u(m))
    for m in (C - 1, C, C + 1):
        out[f"m = {m}"] = (u(300), u(m))
    for n in (B - 1, B, B + 1):
        out[f"n = {n}"] = (u(n), u(77))
    # the threshold between 1 and 4 points per thread; WIDE is also a whole number of the blocks' 1024 points
    for n in (WIDE - 1, WIDE, WIDE + 1):
        out[f"n = {n}"] = (u(n), u(5))
    # duplicates of b exactly C apart: the tie between b[j], b[j + C] and b[j + 2 C] crosses chunks, and the first must win
    b = u(2 * C + 40)
    b[C:C + 40], b[2 * C:2 * C + 40] = b[:40], b[:40]
    out["duplicates a chunk apart"] = (np.concatenate([b[:40], b[:40] + np.float32(1e-3), u(60)]), b)
    # a = b + 1/16 on an 8^3 lattice of spacing 1/8: every interior point of a has 8 lattice points at exactly the same distance
    g = np.arange(8, dtype=np.float32) / np.float32(8)
    lat = _f32(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))
    out["lattice, a = b + 1/16"] = (lat + np.float32(1 / 16), lat)
    p = u(700)
    out["a == b"] = (p, p.copy())
    out["coordinates near 1e3"] = (_f32(1000 + rng.uniform(-1, 1, (500, 3))), _f32(1000 + rng.uniform(-1, 1, (1500, 3))))
    a, b = u(130), u(C + 7)
    b[5, 1], b[C + 2, 0] = np.inf, np.inf
    a[3, 2], a[129, 0] = np.nan, np.nan
    out["+inf in b, NaN in a"] = (a, b)
    out["only a +inf point in b"] = (u(70), _f32([[np.inf, 0.0, 0.0]]))
    return out


NEAREST_SETS = _nearest_sets()
TILED = (WIDE + 1025,)                   # 4 points per thread over ten chunks of b: the rows of "4099 x 10007", repeated


@functools.lru_cache(maxsize=None)
def _nearest_ref(name):
    return MN.nearest(*NEAREST_SETS[name], dtype=np.float32)


def test_the_tie_cases_have_the_ties_they_claim():
    """Checked on the CPU: up to 8 exact ties per point of the shifted lattice, 3 per duplicated point."""
    a, b = NEAREST_SETS["lattice, a = b + 1/16"]
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2)
    d2 = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
    ties = (d2 == d2.min(1, keepdims=True)).sum(1)
    assert int(ties.max()) == 8 and int(ties.min()) == 1
    d, i = _nearest_ref("duplicates a chunk apart")
    assert bool((d[:40] == 0).all()) and i[:40].tolist() == list(range(40)) and bool((i[40:80] < 40).all())
    d, i = _nearest_ref("+inf in b, NaN in a")
    assert np.isinf(d[3]) and np.isinf(d[129]) and i[3] == 0 and i[129] == 0 and bool(np.isfinite(np.delete(d, [3, 129])).all())
    assert 5 not in i.tolist() and C + 2 not in i.tolist()
    d, i = _nearest_ref("only a +inf point in b")
    assert bool(np.isinf(d).all()) and not i.any()


@pytest.mark.parametrize("name", list(NEAREST_SETS))
def test_nearest_points_equals_the_float32_restatement(MT, name):
    a, b = NEAREST_SETS[name]
    want_d, want_i = _nearest_ref(name)
    d, i = MT.nearest_points(_t(a), _t(b))
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and tuple(d.shape) == tuple(i.shape) == (len(a),)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(i, want_i), f"{int((i != want_i).sum())} of {len(i)} indices differ"
    assert np.array_equal(d.view(np.uint32), want_d.view(np.uint32)), f"{int((d.view(np.uint32) != want_d.view(np.uint32)).sum())} distances differ"


@pytest.mark.parametrize("n", TILED)
def test_nearest_points_with_several_points_per_thread_over_many_chunks(MT, n):
    """The 4099 x 10007 case with its rows of `a` repeated up to n: the restatement's result is the same rows repeated."""
    a, b = NEAREST_SETS["4099 x 10007"]
    want_d, want_i = _nearest_ref("4099 x 10007")
    rows = torch.arange(n, device=DEV) % len(a)
    d, i = MT.nearest_points(_t(a)[rows].contiguous(), _t(b))
    assert MT.nearest_points_per_thread(n) == 4
    assert torch.equal(i, _t(want_i)[rows]) and fp.same_bits(d, _t(want_d)[rows])


def test_nearest_points_without_points(MT):
    d, i = MT.nearest_points(torch.empty(0, 3, device=DEV), _t(NEAREST_SETS["64 x 64"][1]))
    assert tuple(d.shape) == (0,) and tuple(i.shape) == (0,)
    with pytest.raises(ValueError):
        MT.nearest_points(_t(NEAREST_SETS["64 x 64"][0]), torch.empty(0, 3, device=DEV))


# ------------------------------------------------------------------------------------------------ 2. nearest against float64
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_nearest_distance_is_within_its_bound_of_float64(MT, scale):
    """Every dist within REL = 4 x 2^-24, relative, of the float64 nearest distance (the derivation: at REL above).  The index
    may differ at near-ties; the minimum may not leave the bound.  Measured on the MI355X: DESIGN.md "Quality metrics"."""
    rng = np.random.default_rng(int(round(math.log10(scale))) + 20)
    a, b = _f32(scale * rng.uniform(-1, 1, (600, 3))), _f32(scale * rng.uniform(-1, 1, (577, 3)))
    d64, i64 = MN.nearest(a, b, dtype=np.float64)
    d32, _ = MN.nearest(a, b, dtype=np.float32)
    d, i = MT.nearest_points(_t(a), _t(b))
    d, i = d.cpu().numpy().astype(np.float64), i.cpu().numpy()
    ratio, own = float((np.abs(d - d64) / d64).max()) / U, float((np.abs(d32 - d64) / d64).max()) / U
    print(f"scale {scale:g}: largest relative error {ratio:.2f} x 2^-24 (the float32 restatement on the CPU: {own:.2f}; bound 4); "
          f"{int((i != i64).sum())} of {len(i)} indices differ from float64's")
    assert bool((d64 > 0).all()) and ratio <= 4.0


# ------------------------------------------------------------------------------------------------ 3. distance_stats
STATS_N = (0, 1, 255, 256, 257, 65539, SLICE + 1)
STATS_MODES = [(0, False), (3, False), (8, False), (0, True), (3, True), (8, True)]
NB_ROWS = 1000


@functools.lru_cache(maxsize=None)
def _stats_input(n):
    """dist >= 0 of mixed magnitude, idx into NB_ROWS unit normals, and 8 thresholds of which the first EQUALS a dist value."""
    rng = np.random.default_rng(100 + n % 1000)
    dist = _f32(rng.uniform(0, 1, n) * 10.0 ** rng.integers(-3, 2, n))
    idx = rng.integers(0, NB_ROWS, n).astype(np.int32)
    na, nb = rng.standard_normal((n, 3)), rng.standard_normal((NB_ROWS, 3))
    na, nb = _f32(na / np.linalg.norm(na, axis=1, keepdims=True)), _f32(nb / np.linalg.norm(nb, axis=1, keepdims=True))
    tau = [float(dist[n // 2]) if n else 0.5, 0.001, 0.01, 0.1, 0.5, 1.0, 5.0, 100.0]
    return dist, idx, na, nb, tau


@functools.lru_cache(maxsize=None)
def _stats_ref(n, normals):
    dist, idx, na, nb, tau = _stats_input(n)
    return MN.stats(dist, idx, na if normals else None, nb if normals else None, tau)


@pytest.mark.parametrize("T,normals", STATS_MODES)
@pytest.mark.parametrize("n", STATS_N)
def test_distance_stats(MT, n, T, normals):
    """Counts and the maximum exact; every sum within (n - 1) 2^-53 sum|x| of the exact sum (math.fsum), the bound that holds for
    ANY order of summation; two calls give the same 64-bit patterns."""
    dist, idx, na, nb, tau = _stats_input(n)
    want = _stats_ref(n, normals)
    args = (_t(dist), _t(idx), _t(na) if normals else None, _t(nb) if normals else None, tau[:T])
    out = MT.distance_stats(*args)
    again = MT.distance_stats(*args)
    assert out.dtype == torch.float64 and tuple(out.shape) == (4 + T,) and out.is_cuda
    assert fp.same_bits(out, again)
    got = out.cpu().tolist()
    assert got[2] == want[2] and got[4:] == want[4:4 + T], (got, want)
    if T and n:
        assert got[4] >= 1                                            # the threshold that equals a dist value counts that point
    for k in (0, 1, 3):
        bound = max(n - 1, 0) * 2.0 ** -53 * want[k]                  # (every term is non-negative: sum|x| is the sum)
        print(f"n = {n}, T = {T}, out[{k}] = {got[k]!r}: error {abs(got[k] - want[k]):.3e}, bound {bound:.3e}")
        assert abs(got[k] - want[k]) <= bound, (k, got[k], want[k])
    if not normals:
        assert got[3] == 0.0
        assert fp.same_bits(MT.distance_stats(args[0], None, None, None, tau[:T]), out)     # idx may be left out


def test_distance_stats_refuses_more_than_8_thresholds(MT):
    with pytest.raises(ValueError):
        MT.distance_stats(_t(_stats_input(255)[0]), thresholds=[0.1] * 9)
    with pytest.raises(ValueError):
        MT.distance_stats(_t(_stats_input(255)[0])[:, None])


# ------------------------------------------------------------------------------------------------ 4. the wrappers
TAUS = (0.03125, 0.0625, 0.125)          # exactly representable: float64 and the kernel's fp32 compare mean the same threshold


@functools.lru_cache(maxsize=None)
def _cloud():
    """2000 x 3000 points with unit normals, and the float64 nearest neighbours.  A property of the seeded data, asserted here: the
    float32 search picks the same neighbours (no near-tie within REL), so the normals compared are the same ones."""
    rng = np.random.default_rng(42)
    a, b = _f32(rng.uniform(-1, 1, (2000, 3))), _f32(rng.uniform(-1, 1, (3000, 3)))
    na, nb = rng.standard_normal((2000, 3)), rng.standard_normal((3000, 3))
    na, nb = _f32(na / np.linalg.norm(na, axis=1, keepdims=True)), _f32(nb / np.linalg.norm(nb, axis=1, keepdims=True))
    d_ab, i_ab = MN.nearest(a, b, np.float64)
    d_ba, i_ba = MN.nearest(b, a, np.float64)
    assert np.array_equal(MN.nearest(a, b)[1], i_ab) and np.array_equal(MN.nearest(b, a)[1], i_ba)
    return a, b, na, nb, d_ab, d_ba


def test_compare_points_against_float64(MT):
    """Means and maxima within REL (relative; 2 REL + REL^2 for the mean squares) plus the summation bound (n - 1) 2^-53; a share
    between the shares of the float64 distances stretched and shrunk by REL (a distance that close to a threshold may fall on
    either side), the F-score between the F-scores of those shares (it grows with both); the normal consistency within 3 x 2^-24
    (three roundings on products whose absolute sum is at most 1 for unit vectors) plus the summation bound."""
    a, b, na, nb, d_ab, d_ba = _cloud()
    want = MN.compare_points(a, b, na, nb, TAUS, dtype=np.float64)
    got = MT.compare_points(_t(a), _t(b), _t(na), _t(nb), TAUS)
    assert set(got) == set(want) and all(isinstance(got[k], float) for k in got if k not in ("precision", "recall", "fscore"))
    sumerr = 3000 * 2.0 ** -53
    for key, rel in (("accuracy", REL), ("completeness", REL), ("chamfer_l1", REL), ("hausdorff", REL), ("chamfer_l2", 2 * REL + REL * REL)):
        err = abs(got[key] - want[key])
        print(f"{key}: {got[key]!r} vs float64 {want[key]!r}: relative error {err / want[key] / U:.3f} x 2^-24")
        assert err <= (rel + sumerr) * want[key], key
    lo_hi = {}
    for key, d in (("precision", d_ab), ("recall", d_ba)):
        for tau in TAUS:
            lo, hi = float((d * (1 + REL) <= tau).mean()), float((d * (1 - REL) <= tau).mean())
            lo_hi[key, tau] = (lo, hi)
            assert lo <= got[key][tau] <= hi, (key, tau, lo, got[key][tau], hi)
    assert sum(0.01 < lo < 0.99 for lo, _ in lo_hi.values()) >= 4     # the thresholds cut through the distances, not past them
    f = lambda p, r: 2 * p * r / (p + r) if p + r > 0 else 0.0   # noqa: E731
    for tau in TAUS:
        (pl, ph), (rl, rh) = lo_hi["precision", tau], lo_hi["recall", tau]
        assert f(pl, rl) - 1e-15 <= got["fscore"][tau] <= f(ph, rh) + 1e-15, tau
    err = abs(got["normal_consistency"] - want["normal_consistency"])
    print(f"normal_consistency: {got['normal_consistency']!r} vs float64 {want['normal_consistency']!r}: error {err:.3e}")
    assert err <= 3 * U + sumerr
    plain = MT.compare_points(_t(a), _t(b), thresholds=TAUS)
    assert "normal_consistency" not in plain and plain["chamfer_l1"] == got["chamfer_l1"] and plain["fscore"] == got["fscore"]
    assert list(MT.compare_points(_t(a), _t(b))["fscore"]) == [0.01, 0.02, 0.05]


def test_two_planes_give_h_exactly(MT):
    h = 0.125
    a, b, na, nb = MN.two_planes(8, h)
    got = MT.compare_points(_t(a), _t(b), _t(na), _t(nb), (0.0625, h, 0.25))
    assert got["accuracy"] == got["completeness"] == got["hausdorff"] == got["chamfer_l1"] == h and got["chamfer_l2"] == 2 * h * h
    assert got["fscore"] == {0.0625: 0.0, h: 1.0, 0.25: 1.0} and got["normal_consistency"] == 1.0
    assert got == MN.compare_points(a, b, na, nb, (0.0625, h, 0.25))


def torus(nu=24, nv=16, R=0.6, r=0.25):
    """(v [nu nv, 3] float32, f [2 nu nv, 3] int32): a closed torus, outward oriented."""
    u, w = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    q = lambda a, b: ((a % nu) * nv + (b % nv)).ravel()   # noqa: E731
    f = np.concatenate([np.stack([q(i, j), q(i + 1, j), q(i + 1, j + 1)], 1), np.stack([q(i, j), q(i + 1, j + 1), q(i, j + 1)], 1)])
    return _f32(v), np.ascontiguousarray(f, dtype=np.int32)


def square(half, z, cells=1):
    """A flat square [-half, half]^2 at height z as 2 cells^2 triangles, normal +z."""
    g = np.linspace(-half, half, cells + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([X.ravel(), Y.ravel(), np.full(X.size, z)], 1)
    i, j = (k.ravel() for k in np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij"))
    q = lambda a, b: a * (cells + 1) + b   # noqa: E731
    f = np.concatenate([np.stack([q(i, j), q(i + 1, j), q(i + 1, j + 1)], 1), np.stack([q(i, j), q(i + 1, j + 1), q(i, j + 1)], 1)])
    return _f32(v), np.ascontiguousarray(f, dtype=np.int32)


def test_a_mesh_against_itself_on_the_exact_surface_is_zero(MT):
    """surface=True: every mean and the maximum under 1e-6 (the mesh query's recorded fp32 error is 9.6e-8); sample to sample the
    same comparison gives the sampling spacing instead."""
    v, f = torus()
    mesh = (_t(v), _t(f))
    got = MT.compare_meshes(mesh, mesh, n=3000, surface=True)
    print({k: got[k] for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff", "normal_consistency")})
    for key in ("accuracy", "completeness", "chamfer_l1", "hausdorff"):
        assert 0 <= got[key] < 1e-6, key
    assert got["chamfer_l2"] < 1e-12 and got["fscore"][0.01] == 1.0
    assert got["normal_consistency"] > 0.97                           # (a sample on an edge may find the neighbouring face: 15-degree facets)
    spaced = MT.compare_meshes(mesh, mesh, n=3000)
    assert 0.005 < spaced["chamfer_l1"] < 0.1 and spaced["hausdorff"] > spaced["chamfer_l1"]
    # the same mesh as a TriMesh-like object and as a longer tuple
    obj = type("M", (), dict(v=mesh[0], f=mesh[1]))()
    assert MT.compare_meshes(obj, mesh + (None, None, None), n=3000, surface=True) == got
    pts, nrm, face = MT.sample_surface(mesh, 500, seed=3)
    assert tuple(pts.shape) == tuple(nrm.shape) == (500, 3) and face.dtype == torch.int32
    assert float((nrm.norm(dim=1) - 1).abs().max()) < 1e-6


def test_a_square_against_a_larger_square_above_it(MT):
    """A = [-0.3, 0.3]^2 at z = 0 against B = [-0.8, 0.8]^2 (4 x 4 cells) at z = h: every closest point of a sample of A on B is its
    foot point, so accuracy and the maximum of d(a -> B) are h to 1e-6.  The dict's `hausdorff` is the LARGER of the two directed
    maxima, and B reaches past A, so it is held to the analytic distance of B's own samples to the square A instead (float64 from
    the sampled points), as is the completeness; the directed maximum a -> B is read from primx_distance_stats itself."""
    from topia_xl_amd import fit
    h = 0.125
    A, Bm = tuple(_t(x) for x in square(0.3, 0.0)), tuple(_t(x) for x in square(0.8, h, cells=4))
    got = MT.compare_meshes(A, Bm, n=4000, seed=7, surface=True, thresholds=(0.1, 0.2))
    pa, _, _ = MT.sample_surface(A, 4000, 7)
    pb, _, _ = MT.sample_surface(Bm, 4000, 8)
    d = fit.mesh_field_query(pa, Bm[0], Bm[1])[0]
    directed = MT.distance_stats(d).cpu().tolist()
    p = pb.cpu().numpy().astype(np.float64)
    out = np.maximum(np.abs(p[:, :2]) - 0.3, 0.0)
    exact = np.sqrt((out ** 2).sum(1) + p[:, 2] ** 2)
    print(f"accuracy {got['accuracy']!r}, max d(a -> B) {directed[2]!r}, hausdorff {got['hausdorff']!r} (analytic {exact.max()!r}), "
          f"completeness {got['completeness']!r} (analytic {exact.mean()!r})")
    assert abs(got["accuracy"] - h) <= 1e-6 and abs(directed[2] - h) <= 1e-6 and abs(directed[0] / 4000 - got["accuracy"]) <= 1e-12
    assert abs(got["hausdorff"] - exact.max()) <= 1e-6 and abs(got["completeness"] - exact.mean()) <= 1e-6
    assert got["precision"] == {0.1: 0.0, 0.2: 1.0} and got["normal_consistency"] == 1.0


def test_compare_to_field_runs_on_the_two_sphere_field(MT, mods):
    """The two-sphere field of tests/test_hip_occlusion.py at 48^3 against its own extracted mesh, sample to sample: finite values
    and fscore[0.05] > 0.9.  A sanity floor, derived rather than measured: both sides sample the SAME surface (its area is under
    2 x 4 pi 0.35^2 = 3.1), so a sample's nearest neighbour lies about sqrt(3.1 / 20000) = 0.012 away, and even a surface displaced
    by one whole cell of the lattice, 2 / 47 = 0.043, would stay inside 0.05.  Only a broken sampler, search or reduction puts more
    than a tenth of the samples beyond it.  Nothing is asserted about quality at shipped scale."""
    from tests import test_hip_occlusion as TO
    from topia_xl_amd import pipeline
    field = TO._crease_field()
    mesh = mods.M.extract_mesh(field, 48)
    got = MT.compare_to_field(mesh, field, 48, n=20000)
    print(got)
    flat = [got[k] for k in ("accuracy", "completeness", "chamfer_l1", "chamfer_l2", "hausdorff", "normal_consistency")]
    assert all(math.isfinite(x) for x in flat + list(got["fscore"].values()))
    assert got["fscore"][0.05] > 0.9
    recon = torch.cat([field.srt_param.detach(), field.feat_param.detach()], 1)
    assert pipeline.primitives_vs_mesh(recon, mesh, 48, n=20000) == got


# ------------------------------------------------------------------------------------------------ 5. footprint
def test_footprint_of_both_entry_points(MT):
    """Inside footprint.hold: intact guards around the outputs and the workspace, untouched const operands, no allocation past the
    wrappers, and results that depend neither on the fill of torch.empty nor on the guard (bit for bit: nothing here is atomic)."""
    a, b = NEAREST_SETS[f"1000 x {3 * C + 5}"]
    rng = np.random.default_rng(9)
    na, nb = _f32(rng.standard_normal((len(a), 3))), _f32(rng.standard_normal((len(b), 3)))

    def case(g):
        gi = lambda t, name: g.guard_input(_t(t), name).t   # noqa: E731
        ta, tb, tna, tnb = gi(a, "a"), gi(b, "b"), gi(na, "na"), gi(nb, "nb")
        d, i = MT.nearest_points(ta, tb)
        return [d, i, MT.distance_stats(d, i, tna, tnb, (0.01, 0.05, 0.1)), MT.distance_stats(d)]

    out = fp.hold(case)
    want_d, want_i = _nearest_ref(f"1000 x {3 * C + 5}")
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), want_d.view(np.uint32)) and np.array_equal(out[1].cpu().numpy(), want_i)


# ------------------------------------------------------------------------------------------------ 6. stream order
@TS.case(STREAM_CASE, ["primx_nearest_points", "primx_distance_stats"])
def _stream_metrics(E, dtype):  # noqa: F811
    """4099 x 3077 points with normals: the search, then the reduction of its results.  All four operands are late (their poison
    is NaN, which no pair wins with: every index stays 0, inside nb)."""
    from topia_xl_amd import metrics

    def make(k):
        rng = np.random.default_rng(70 + k)
        return {"a": _t(_f32(rng.uniform(-1, 1, (4099, 3)))), "b": _t(_f32(rng.uniform(-1, 1, (3 * C + 5, 3)))),
                "na": _t(_f32(rng.standard_normal((4099, 3)))), "nb": _t(_f32(rng.standard_normal((3 * C + 5, 3))))}

    def call(ctx, i, probe):
        d, idx = metrics.nearest_points(i["a"], i["b"])
        return [d, idx, metrics.distance_stats(d, idx, i["na"], i["nb"], (0.01, 0.05))]
    return make, call, None


def test_stream_order_of_the_metrics_entry_points(E, called):  # noqa: F811  (`called` is the imported fixture)
    """The body of tests/test_hip_streams.py::test_stream_order for the case registered above; no host synchronisation is documented."""
    c = TS.CASES[STREAM_CASE]
    make, call, setup = c.build(E, None)
    rep = so.run(STREAM_CASE, make, call, E.S, E.blocker, setup=setup, must_sync=False)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{STREAM_CASE} declares entry points it did not call: {missing}"
