"""The mesh ray queries on the MI355X (the ray kernels of csrc/meshbvh.hip, fit.MeshBVH.raycast / .visibility, MeshField(sign=
"visibility")) against the numpy restatement tests/meshray_numpy.py.

Held, on the fixtures of tests/test_hip_meshbvh.py plus "flipped" (icosphere(3) with a seeded half of its faces reversed):
  1. t, face and bary of the closest hit equal the float32 restatement's brute force bit for bit, for every prefix n = 1, 255,
     257, 1000 of a seeded ray set (a fifth each: through the box, at vertices, at edge midpoints, axis-parallel, from the surface;
     no ray excluded), with tmin / tmax windows that cut first hits away and with origins 64 extents away; any_hit's hit / miss
     equals "some face accepted";
  2. no ray from a strictly interior point of a closed fixture misses, the rays at every vertex and edge midpoint among them;
  3. the visibility count equals the restatement's for K = 1, 8, 64 and limit = 0, 1;
  4. the visibility sign gives the ground truth on "flipped" where the winding sign does not, agrees with it on consistently
     oriented closed meshes, and leaves dist, face, tex and mat alone;
  5. a fit of the flipped sphere under sign="visibility" carries the sphere's own sign and, everywhere else, its winding fit's bits
     (the test says why the bits of the unflipped sphere's fit cannot be asked);
  6. the defaults call neither new entry point;
  7. the argument checks; 8. footprint and stream order of both entry points.

The module imports without a GPU (its references serve tests/test_meshray_cpu.py, and it registers its stream-order cases in the
table of tests/test_hip_streams.py at import, as tests/test_hip_meshbvh.py does and for the reasons given there).
"""
import functools

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import meshbvh_numpy as MB
from tests import meshfield_numpy as MF
from tests import meshray_numpy as MR
from tests import streamorder as so
from tests import test_hip_meshbvh as TB
from tests import test_hip_streams as TS
from tests.test_hip_normalmap import E, mods  # noqa: F401  (fixtures: the built package; one side stream of this module's own)
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = TB.NS
RAY_CASE, VIS_CASE = "mesh_bvh_raycast", "mesh_bvh_visibility"
NAMES = ("primx_mesh_bvh_raycast", "primx_mesh_bvh_visibility")
INF = float("inf")

_FLIPPED = MR.flipped(3)
FIXTURES = dict(TB.FIXTURES)
FIXTURES["flipped"] = (_FLIPPED[0], _FLIPPED[1], True)
CLOSED = [k for k, m in FIXTURES.items() if m[2]]
VIS_FIXTURES = ("F=1", "F=9", "F=549", "box", "hemisphere", "degenerate", "shifted", "flipped")
FAR_FIXTURES = ("box", "icosphere", "shifted", "slivers")
_t, _bits = TB._t, TB._bits


@functools.lru_cache(maxsize=None)
def tree_of(name):
    v, f, _ = FIXTURES[name]
    return TB.tree_of(name) if name in TB.FIXTURES else MB.build(v, f)


@functools.lru_cache(maxsize=None)
def rays_of(name, far=1.0):
    v, f, _ = FIXTURES[name]
    return MR.ray_set(v, f, 1000, sum(name.encode()) + 1, far)


@functools.lru_cache(maxsize=None)
def windows_of(name):
    """(tmin, tmax) pairs: everything; a tmin and a tmax at the median first hit (each cuts the first hit of about half the rays
    away); a window between the quartiles."""
    t = reference(name)["t"]
    t = np.sort(t[np.isfinite(t)])
    if t.size < 4:
        return ((0.0, INF),)
    q1, q2, q3 = (float(t[(k * t.size) // 4]) for k in (1, 2, 3))
    return ((0.0, INF), (q2, INF), (0.0, q2), (q1, q3))


@functools.lru_cache(maxsize=None)
def reference(name, tmin=0.0, tmax=INF, far=1.0):
    """The float32 restatement's brute force on the fixture's rays, once."""
    v, f, _ = FIXTURES[name]
    o, d = rays_of(name, far)
    return MR.brute(o, d, v, f, tmin, tmax)


@functools.lru_cache(maxsize=None)
def interior_of(name):
    v, f, _ = FIXTURES[name]
    return MR.interior_rays(v, f, n_random=200, seed=sum(name.encode()))


@functools.lru_cache(maxsize=None)
def sign_reference(name):
    """The points of the sign checks and what holds there: 'p'; 'inside' = the float64 brute-force winding sign of the
    consistently oriented mesh; 'held' = the float64 distance exceeds the float32 distance floor (`on_surface` of
    tests/test_hip_meshbvh.py::reference)."""
    if name == "flipped":
        v, _, f = _FLIPPED                                            # the unflipped faces: the ground truth
        p = MB.points(v, f, 1000, 3)
        b64 = MF.query(p, v, f, None, np.float64, keep_d2=False)
        b32 = MF.query(p, v, f, None, np.float32, keep_d2=False)
        floor = float(np.abs(b32["dist"].astype(np.float64) - b64["dist"]).max())
        return {"p": p, "inside": np.abs(b64["wn"]) >= 0.5, "held": b64["dist"] > floor, "dist": b64["dist"]}
    ref = TB.reference(name)
    return {"p": TB.points_of(name), "inside": np.abs(ref["b64"]["wn"]) >= 0.5, "held": ~ref["on_surface"], "dist": ref["b64"]["dist"]}


@pytest.fixture(scope="module")
def fit(E):  # noqa: F811
    from topia_xl_amd import fit
    assert fit.SIGNS == ("winding", "visibility")
    return fit


@functools.lru_cache(maxsize=None)
def _bvh(name):
    from topia_xl_amd import fit
    v, f, _ = FIXTURES[name]
    return fit.MeshBVH(_t(v), _t(f))


def _same(got, want, n, tag):
    t, face, bary, _ = got
    assert tuple(t.shape) == (n,) and tuple(face.shape) == (n,) and tuple(bary.shape) == (n, 2) and face.dtype == torch.int32, tag
    bad = np.flatnonzero(face.cpu().numpy() != want["face"][:n])
    assert bad.size == 0, (tag, "face", bad.size, bad[:5])
    assert np.array_equal(_bits(t), want["t"][:n].view(np.uint32)), (tag, "t", int((_bits(t) != want["t"][:n].view(np.uint32)).sum()))
    assert np.array_equal(_bits(bary), np.ascontiguousarray(want["bary"][:n]).view(np.uint32)), (tag, "bary")


# ------------------------------------------------------------------------------------------------ 1. closest hit
@pytest.mark.parametrize("name", list(FIXTURES))
def test_closest_hit_equals_the_restatement_bit_for_bit(fit, name):
    bvh = _bvh(name)
    o, d = rays_of(name)
    ref = reference(name)
    print(f"{name}: {int(ref['hit'].sum())} of 1000 rays hit")
    for n in NS:
        to, td = _t(o[:n]), _t(d[:n])
        _same(bvh.raycast(to, td), ref, n, (name, n))
        anyf = bvh.raycast(to, td, any_hit=True)[1].cpu().numpy()
        assert np.array_equal(anyf >= 0, ref["hit"][:n]), (name, n, "any_hit")
    for tmin, tmax in windows_of(name)[1:]:
        w = reference(name, tmin, tmax)
        _same(bvh.raycast(_t(o), _t(d), tmin, tmax), w, 1000, (name, tmin, tmax))
        anyf = bvh.raycast(_t(o), _t(d), tmin, tmax, any_hit=True)[1].cpu().numpy()
        assert np.array_equal(anyf >= 0, w["hit"]), (name, tmin, tmax, "any_hit")


@pytest.mark.parametrize("name", FAR_FIXTURES)
def test_closest_hit_from_64_extents_away(fit, name):
    o, d = rays_of(name, 64.0)
    ref = reference(name, 0.0, INF, 64.0)
    assert ref["hit"].sum() > 100
    _same(_bvh(name).raycast(_t(o), _t(d)), ref, 1000, (name, "far"))


def test_attributes_at_the_hit_and_degenerate_rays(fit):
    v, f, _ = FIXTURES["icosphere"]
    o, d = (a.copy() for a in rays_of("icosphere"))
    o[0], d[1], d[2], o[3] = np.nan, 0.0, np.inf, np.inf           # R1: a miss with the miss outputs, never a NaN
    d[4] = (1e-42, 0.0, 0.0)                                         # 1 / d overflows
    want = MR.brute(o, d, v, f)
    attr = MF.affine_attr(v)
    got = _bvh("icosphere").raycast(_t(o), _t(d), attr=_t(attr))
    _same(got, want, 1000, "degenerate rays")
    assert not want["hit"][:5].any() and bool(torch.isinf(got[0][:5]).all()) and bool((got[2][:5] == 0).all())
    assert np.array_equal(_bits(got[3]), MR.attr_at(attr, f, want["face"], want["bary"]).view(np.uint32))
    assert bool((got[3][:5] == 0).all()) and got[3].shape == (1000, 5)


# ------------------------------------------------------------------------------------------------ 2. watertight
@pytest.mark.parametrize("name", CLOSED)
def test_no_interior_ray_leaves_a_closed_mesh(fit, name):
    o, d = interior_of(name)
    t, face, _, _ = _bvh(name).raycast(_t(o), _t(d))
    miss = np.flatnonzero(face.cpu().numpy() < 0)
    assert miss.size == 0, (name, miss.size, o[miss[:3]], d[miss[:3]])
    assert bool(torch.isfinite(t).all()) and bool((t >= 0).all())
    esc = _bvh(name).raycast(_t(o), _t(d), any_hit=True)[1]
    assert bool((esc >= 0).all())


def test_rays_through_the_corners_and_edges_of_the_exact_box(fit):
    v, f, c = MR.exact_box()
    o, d = MR.interior_rays(v, f, centre=c, n_random=0)
    k = o.shape[0] // 3                                              # the centre's own rays: exactly through corners and edges
    t, face, _, _ = fit.MeshBVH(_t(v), _t(f)).raycast(_t(o[:k]), _t(d[:k]))
    want = MR.brute(o[:k], d[:k], v, f)
    assert k == 26 and bool((face >= 0).all()) and np.array_equal(_bits(t), want["t"].view(np.uint32))
    assert float((t - 1).abs().max()) <= 2.0 ** -22                   # the hit is the corner, the edge's midpoint: t = 1


# ------------------------------------------------------------------------------------------------ 3. visibility
@functools.lru_cache(maxsize=None)
def vis_reference(name, K, n=200):
    v, f, _ = FIXTURES[name]
    p = sign_reference(name)["p"][:n] if name == "flipped" else TB.points_of(name)[:n]
    return p, MR.escapes(p, MR.fibonacci(K), v, f)


@pytest.mark.parametrize("name", VIS_FIXTURES)
def test_visibility_counts_equal_the_restatement(fit, name):
    bvh = _bvh(name)
    for K in (1, 8, 64):
        p, want = vis_reference(name, K)
        got = bvh.visibility(_t(p), K)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), (name, K, int((got.cpu().numpy() != want).sum()))
        one = bvh.visibility(_t(p), K, limit=1)
        assert np.array_equal(one.cpu().numpy(), np.minimum(want, 1)) and torch.equal(one, got.clamp(max=1)), (name, K)
        given = bvh.visibility(_t(p), _t(MR.fibonacci(K)), limit=0)                      # a tensor is taken as given
        assert torch.equal(given, got)
    assert sorted(bvh._directions) == [1, 8, 64]                                         # uploaded once per tree and K
    kept = bvh._directions[8]
    bvh.visibility(_t(p), 8)
    assert bvh._directions[8] is kept


# ------------------------------------------------------------------------------------------------ 4. the sign
def _fields(fit, name):
    v, f, _ = FIXTURES[name]
    attr = _t(MF.affine_attr(v))
    return (fit.MeshField(_t(v), _t(f), attr, accel="bvh", sign=s) for s in ("winding", "visibility"))


def test_the_visibility_sign_is_right_on_the_flipped_sphere_where_the_winding_sign_is_not(fit):
    ref = sign_reference("flipped")
    wind, vis = _fields(fit, "flipped")
    p = _t(ref["p"])
    qw, qv = wind.query(p), vis.query(p)
    held, inside = ref["held"], ref["inside"]
    got = (qv["sdf"][:, 0] < 0).cpu().numpy()
    assert held.mean() >= 0.99 and np.array_equal(got[held], inside[held]), int((got != inside)[held].sum())
    wrong = ((qw["sdf"][:, 0] < 0).cpu().numpy() != inside) & held & inside
    print(f"flipped: the winding sign is wrong at {int(wrong.sum())} of {int((held & inside).sum())} inside points, visibility at 0")
    assert wrong.sum() > 0.5 * (held & inside).sum()
    assert set(qv) == set(qw) | {"escapes"} and qv["escapes"].dtype == torch.int32 and int(qv["escapes"].max()) <= 1
    for k in ("face", "tex", "mat", "wn"):
        assert fp.same_bits(qv[k], qw[k]), k
    assert fp.same_bits(qv["sdf"].abs(), qw["sdf"].abs())


@pytest.mark.parametrize("name", ["box", "icosphere", "shifted"])
def test_both_signs_agree_on_consistently_oriented_meshes(fit, name):
    ref = sign_reference(name)
    wind, vis = _fields(fit, name)
    p = _t(ref["p"])
    qw, qv = wind.query(p), vis.query(p)
    held = ref["held"]
    sw, sv = ((q["sdf"][:, 0] < 0).cpu().numpy() for q in (qw, qv))
    assert np.array_equal(sw[held], sv[held]) and np.array_equal(sv[held], ref["inside"][held]), (name, int((sw != sv)[held].sum()))
    for k in ("face", "tex", "mat", "wn"):
        assert fp.same_bits(qv[k], qw[k]), k
    assert fp.same_bits(qv["sdf"].abs(), qw["sdf"].abs())
    two = fit.MeshField(_t(FIXTURES[name][0]), _t(FIXTURES[name][1]), accel="bvh", sign="visibility", sign_directions=8, min_escapes=2)
    q2 = two.query(p)
    want = MR.escapes(ref["p"][:100], MR.fibonacci(8), *FIXTURES[name][:2], limit=2)
    assert np.array_equal(q2["escapes"][:100].cpu().numpy(), want)
    nz = (q2["sdf"][:100, 0] != 0).cpu().numpy()
    assert np.array_equal((q2["sdf"][:100, 0] < 0).cpu().numpy()[nz], (want < 2)[nz])


# ------------------------------------------------------------------------------------------------ 5. end to end
def _mesh(v, f):
    attr = MF.affine_attr(v)
    return (_t(v), _t(f), _t(attr[:, :3]), _t(attr[:, 3]), _t(attr[:, 4]))


def _payload_truth(fit, recon, nv, f, count=1500):
    """`count` seeded points of a fit's payload grid (pos + scale * grid, as mesh_to_primitives forms them) -> (their flat
    indices, inside by the float64 brute-force winding number of the consistently oriented faces f, the held-point rule)."""
    x = (recon[:, None, 1:4] + recon[:, None, 0:1] * fit._local_grid(8, DEV)[None]).reshape(-1, 3).cpu().numpy()
    sub = np.random.default_rng(0).permutation(x.shape[0])[:count]
    b64 = MF.query(x[sub], nv, f, None, np.float64, keep_d2=False)
    b32 = MF.query(x[sub], nv, f, None, np.float32, keep_d2=False)
    held = b64["dist"] > float(np.abs(b32["dist"].astype(np.float64) - b64["dist"]).max())
    return sub, np.abs(b64["wn"]) >= 0.5, held


def test_a_fit_of_the_flipped_sphere_is_the_fit_of_the_sphere(fit):
    """The smallest whole fit (64 primitives of 8^3).  Bit for bit against the unflipped sphere's fit cannot be asked: the surface
    sampler weighs a face's corners in the order the face lists them (`primx_mesh_surface_points`, whose bits stay), so reversing
    a face moves its candidates and with them every centre.  Asked instead, bit for bit: the flipped sphere's fit under
    sign="visibility" is its own winding fit in every column but the SDF's, in the SDF's magnitude, and carries the sign of the
    sphere itself (float64 brute force on the consistently oriented faces) wherever the held-point rule applies, where the
    winding fit of the flipped sphere does not; and on the sphere itself both signs give the same fit there."""
    v, g, f = _FLIPPED
    kw = dict(num_prims=64, prim_shape=8, accel="bvh")
    vis_flipped, info = fit.mesh_to_primitives(_mesh(v, g), sign="visibility", **kw)
    wind_flipped, _ = fit.mesh_to_primitives(_mesh(v, g), **kw)
    vis_plain, pinfo = fit.mesh_to_primitives(_mesh(v, f), sign="visibility", **kw)
    wind_plain, _ = fit.mesh_to_primitives(_mesh(v, f), **kw)
    sdf = lambda r: r[:, 4:4 + 512]   # noqa: E731
    for a, b in ((vis_flipped, wind_flipped), (vis_plain, wind_plain)):
        assert tuple(a.shape) == (64, 4 + 6 * 512) and fp.same_bits(a[:, :4], b[:, :4]) and fp.same_bits(a[:, 4 + 512:], b[:, 4 + 512:])
        assert fp.same_bits(sdf(a).abs(), sdf(b).abs())
    pick = lambda r, sub: sdf(r).reshape(-1)[torch.from_numpy(sub).to(DEV)].cpu().numpy()   # noqa: E731
    sub, inside, held = _payload_truth(fit, vis_flipped, info["v"].cpu().numpy(), f)
    assert held.mean() > 0.99 and inside[held].sum() > 100
    assert np.array_equal((pick(vis_flipped, sub) < 0)[held], inside[held])
    wrong = ((pick(wind_flipped, sub) < 0) != inside) & held & inside
    print(f"flipped fit: the winding sign is wrong at {int(wrong.sum())} of {int((held & inside).sum())} inside payload points")
    assert wrong.sum() > 0.5 * (held & inside).sum()
    sub, inside, held = _payload_truth(fit, vis_plain, pinfo["v"].cpu().numpy(), f)
    assert np.array_equal(pick(vis_plain, sub).view(np.uint32)[held], pick(wind_plain, sub).view(np.uint32)[held])
    assert np.array_equal((pick(vis_plain, sub) < 0)[held], inside[held])
    refined, rinfo = fit.mesh_to_primitives(_mesh(v, g), sign="visibility", refine=1, refine_kw=dict(samples_per_prim=16), **kw)
    assert len(rinfo["refine"]["loss"]) == 1 and bool(torch.isfinite(refined).all())


# ------------------------------------------------------------------------------------------------ 6. non-interference
def test_the_defaults_call_neither_entry_point(fit, called):  # noqa: F811
    v, f, _ = FIXTURES["icosphere"]
    p = _t(TB.points_of("icosphere"))
    for accel in (None, "bvh"):
        field = fit.MeshField(_t(v), _t(f), _t(MF.affine_attr(v)), accel=accel)
        a, b = field.query(p), field.query(p)
        assert set(a) == {"sdf", "tex", "mat", "face", "wn"} and all(fp.same_bits(a[k], b[k]) for k in a)
        kw = dict(num_prims=32, prim_shape=4, candidates=256, accel=accel)
        r1, r2 = fit.mesh_to_primitives(_mesh(v, f), **kw)[0], fit.mesh_to_primitives(_mesh(v, f), **kw)[0]
        assert fp.same_bits(r1, r2)
    assert not set(NAMES) & called, called & set(NAMES)
    fit.MeshField(_t(v), _t(f), accel="bvh", sign="visibility").query(p[:10])
    assert NAMES[1] in called and NAMES[0] not in called


# ------------------------------------------------------------------------------------------------ 7. argument checks
def test_argument_checks(fit, E):  # noqa: F811
    from topia_xl_amd import _lib
    lib = E.lib
    bvh = _bvh("F=65")
    F, ws, n = 65, bvh.ws, 16
    o, d = _t(rays_of("F=65")[0][:n]), _t(rays_of("F=65")[1][:n])
    dirs = _t(MR.fibonacci(8))
    t, face = torch.full((n,), 7.0, device=DEV), torch.full((n,), 7, dtype=torch.int32, device=DEV)
    bary, esc = torch.full((n, 2), 7.0, device=DEV), torch.full((n,), 7, dtype=torch.int32, device=DEV)
    P = lambda x: x.data_ptr()   # noqa: E731
    f = P(bvh.f)

    def ray(org=P(o), dr=P(d), tmin=0.0, tmax=INF, ff=f, tree=P(ws), nbytes=ws.numel(), tt=P(t), fc=P(face), bb=P(bary)):
        return lib.primx_mesh_bvh_raycast(org, dr, n, tmin, tmax, 0, ff, F, tree, nbytes, tt, fc, bb, None)

    def vis(pts=P(o), dd=P(dirs), D=8, tmin=0.0, limit=0, ff=f, tree=P(ws), nbytes=ws.numel(), out=P(esc)):
        return lib.primx_mesh_bvh_visibility(pts, n, dd, D, tmin, limit, ff, F, tree, nbytes, out, None)

    bad = [ray(org=None), ray(dr=None), ray(ff=None), ray(tree=None), ray(tt=None), ray(fc=None), ray(bb=None), ray(tmin=2.0, tmax=1.0),
           ray(tmin=float("nan")), ray(nbytes=ws.numel() - 8192 - 1), ray(tree=P(ws) + 4),
           vis(pts=None), vis(dd=None), vis(ff=None), vis(tree=None), vis(out=None), vis(D=0), vis(D=-1), vis(limit=-1),
           vis(tmin=float("nan")), vis(nbytes=fit.bvh_layout(F)["total"] - 1), vis(tree=P(ws) + 8)]
    assert all(r != 0 for r in bad), bad
    assert b"primx_mesh_bvh_visibility" in lib.primx_last_error()
    torch.cuda.synchronize()
    assert bool((t == 7).all()) and bool((face == 7).all()) and bool((bary == 7).all()) and bool((esc == 7).all())   # no launch
    assert ray() == 0 and vis() == 0 and lib.primx_mesh_bvh_raycast(None, None, 0, 0.0, INF, 0, f, F, P(ws), ws.numel(), None, None, None, None) == 0
    # the Python side
    v, fa, _ = FIXTURES["box"]
    with pytest.raises(ValueError, match="accel"):
        fit.MeshField(_t(v), _t(fa), sign="visibility")
    with pytest.raises(ValueError, match="sign"):
        fit.MeshField(_t(v), _t(fa), accel="bvh", sign="parity")
    with pytest.raises(ValueError, match="sign"):
        fit.mesh_to_primitives(_mesh(v, fa), num_prims=4, candidates=16, sign="visibility")
    with pytest.raises(ValueError):
        fit.MeshField(_t(v), _t(fa), accel="bvh", sign="visibility", min_escapes=0)
    box = _bvh("box")
    e = box.raycast(torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV), attr=_t(MF.affine_attr(v)))
    assert tuple(e[0].shape) == (0,) and tuple(e[1].shape) == (0,) and tuple(e[2].shape) == (0, 2) and tuple(e[3].shape) == (0, 5)
    assert tuple(box.visibility(torch.empty(0, 3, device=DEV)).shape) == (0,)
    for call in (lambda: box.raycast(o, d[:5]), lambda: box.raycast(o[:, :2], d[:, :2]), lambda: box.raycast(o, d, 2.0, 1.0),
                 lambda: box.visibility(o[:, :2]), lambda: box.visibility(o, 0), lambda: box.visibility(o, 8, limit=-1),
                 lambda: box.visibility(o, dirs[:, :2]), lambda: box.raycast(o, d, attr=_t(MF.affine_attr(v))[:3])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: box.raycast(o.cpu(), d), lambda: box.visibility(o.cpu()), lambda: box.visibility(o, dirs.cpu())):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    assert isinstance(_lib.SIGNATURES[NAMES[0]], list)


# ------------------------------------------------------------------------------------------------ 8. footprint, stream order
def test_footprint_of_raycast_and_visibility(fit):
    """Inside footprint.hold: intact guards around the outputs, unchanged rays, points, directions and tree, and results that
    depend neither on what torch.empty holds nor on the guard."""
    v, f, _ = FIXTURES["F=549"]
    o, d = rays_of("F=549")
    tree = _bvh("F=549")

    def case(g):
        gi = lambda a, name: g.guard_input(a if isinstance(a, torch.Tensor) else _t(a), name).t   # noqa: E731
        bvh = fit.MeshBVH(gi(v, "v"), gi(f, "f"), ws=gi(tree.ws, "tree"))
        to, td, tp, dirs = gi(o[:257], "origins"), gi(d[:257], "dirs"), gi(TB.points_of("F=549")[:257], "x"), gi(MR.fibonacci(8), "directions")
        return [bvh.raycast(to, td)[:3], bvh.raycast(to, td, any_hit=True)[1] >= 0, bvh.visibility(tp, dirs), bvh.visibility(tp, dirs, limit=1)]

    out = fp.hold(case)
    ref = reference("F=549")
    assert np.array_equal(out[0][1].cpu().numpy(), ref["face"][:257]) and np.array_equal(out[1].cpu().numpy(), ref["hit"][:257])


@TS.case(RAY_CASE, ["primx_mesh_bvh_raycast"])
def _stream_raycast(E, dtype):  # noqa: F811
    """257 rays on a late tree, late origins and late directions: one launch, nothing read back.  The tree travels as int32
    words, whose poison is 0: a root without faces, so a walk that ran early would follow no index."""
    from topia_xl_amd import fit
    v, f, _ = FIXTURES["F=549"]
    o, d = rays_of("F=549")
    trees = [fit.MeshBVH(_t(v) * (1.0 + 0.25 * k), _t(f)) for k in range(2)]

    def make(k):
        return {"o": _t(o[:257]) * (1.0 + 0.25 * k), "d": _t(d[:257]), "ws": trees[k].ws.view(torch.int32).clone()}

    def call(ctx, i, probe):
        return list(fit.MeshBVH(trees[0].v, trees[0].f, ws=i["ws"].view(torch.uint8)).raycast(i["o"], i["d"])[:3])
    return make, call, None


@TS.case(VIS_CASE, ["primx_mesh_bvh_visibility"])
def _stream_visibility(E, dtype):  # noqa: F811
    """257 points with K = 8 given as a late tensor, on a late tree: one launch, nothing read back."""
    from topia_xl_amd import fit
    v, f, _ = FIXTURES["F=549"]
    trees = [fit.MeshBVH(_t(v) * (1.0 + 0.25 * k), _t(f)) for k in range(2)]
    dirs = MR.fibonacci(8)

    def make(k):
        return {"x": _t(TB.points_of("F=549")[:257]) * (1.0 + 0.25 * k), "dirs": _t(np.roll(dirs, k, axis=0)),
                "ws": trees[k].ws.view(torch.int32).clone()}

    def call(ctx, i, probe):
        return [fit.MeshBVH(trees[0].v, trees[0].f, ws=i["ws"].view(torch.uint8)).visibility(i["x"], i["dirs"])]
    return make, call, None


@pytest.mark.parametrize("name", [RAY_CASE, VIS_CASE])
def test_stream_order_of_the_ray_entry_points(E, called, name):  # noqa: F811  (`called` is the imported fixture)
    """The body of tests/test_hip_streams.py::test_stream_order for the cases registered above: neither documents a
    synchronisation."""
    c = TS.CASES[name]
    make, call, setup = c.build(E, None)
    rep = so.run(name, make, call, E.S, E.blocker, setup=setup, must_sync=name in TS.MUST_SYNC)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{name} declares entry points it did not call: {missing}"
