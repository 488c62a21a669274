"""The mesh BVH on the MI355X (csrc/meshbvh.hip, fit.MeshBVH) against the brute-force query it replaces and against the numpy
restatement tests/meshbvh_numpy.py.

Held, on every fixture below and every prefix n = 1, 255, 257, 1000 of its points:
  1. the tree equals the restatement's bit for bit (order, boxes, moments), and dist, face and out_attr equal
     `primx_mesh_field_query`'s on the same inputs bit for bit - with and without sorted points, for C = 0, 5 and 8 - and dist and
     face the float32 restatement's;
  2. wn within 4 x the float32 restatement's own error of the float64 restatement of the SAME walk (the project's usual margin:
     it covers atan2f and the division of a correct fp32 kernel);
  3. the approximation: E = max |wn of the float64 walk - wn of the float64 brute force| per fixture, printed; inside / outside of
     the accelerated query equals the brute-force float64 sign at every point with ||wn| - 0.5| > 2 E, and at most 5 % of the
     points lie inside that band;
  4. on the closed fixtures the sign equals the brute-force KERNEL's at every point.
A point that float32 cannot tell from the surface - its float64 distance is not above the float32 restatement's own distance
error on these inputs - has no sign to hold in 3: whether its own face's term is +pi or -pi is decided by the last bit of a
float32 triple product (an exactly coplanar point has the float64 winding number 0.5 itself and falls in the band).  Those points
are held by 1, 2 and 4, where both kernels share the per-pair code and so that bit.

The module imports without a GPU: it registers its stream-order cases in the table of tests/test_hip_streams.py at import
(that file stays as it is) and runs them here; the fixtures are numpy and serve tests/test_meshbvh_cpu.py too.  Its side stream is
the one of tests/test_hip_normalmap.py::E, created for the module and destroyed after it: the table's own `E` would take two streams
from torch's pool for good and move the later modules' streams onto other hardware queues (tests/test_hip_primsdf_grad.py explains).
"""
import functools

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import meshbvh_numpy as MB
from tests import meshfield_numpy as MF
from tests import streamorder as so
from tests import test_hip_streams as TS
from tests.test_hip_normalmap import E, mods  # noqa: F401  (fixtures: the built package; one side stream of this module's own)
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 255, 257, 1000)
BUILD_CASE, QUERY_CASE = "mesh_bvh_build", "mesh_bvh_query"
NAMES = ("primx_mesh_bvh_workspace", "primx_mesh_bvh_build", "primx_mesh_bvh_query")
TS.MUST_SYNC[BUILD_CASE] = "the tree pass of primx_mesh_bvh_build reads its index check back before it returns (the one read-back of the feature)"


def _bad_mesh():
    """tests/test_hip_meshfield.py::_bad_mesh, rebuilt: the box with zero-area faces in every edge role, a point, one face thrice."""
    v, f = MF.box()
    extra = np.array([[0.5, 0.5, 0.5], [0.75, 0.25, 0.625], [0.625, 0.375, 0.5625]], np.float32)
    deg = np.array([[8, 8, 9], [8, 9, 8], [8, 10, 9], [10, 10, 10], [8, 8, 9], [10, 8, 9], [8, 8, 9]], np.int32)
    return np.concatenate([v, extra]), np.concatenate([f[:5], deg, f[5:]]).astype(np.int32)


def _fixtures():
    """name -> (v, f, closed).  F = 1, 7, 8, 9: one short leaf, one full leaf, two leaves; 65: nine leaves under L = 16 (seven empty
    slots); 549: 69 leaves, a ragged last one."""
    out = {f"F={F}": MF.mesh_with_faces(F) + (False,) for F in (1, 7, 8, 9, 65, 549)}
    out["box"] = MF.box() + (True,)
    out["icosphere"] = MF.icosphere(3) + (True,)
    out["hemisphere"] = MF.hemisphere(3) + (False,)
    out["icosphere+box"] = MF.join(MF.icosphere(3), MF.box()) + (True,)
    out["degenerate"] = _bad_mesh() + (True,)
    out["shifted"] = MB.shifted_icosphere(2) + (True,)
    out["slivers"] = MB.slivers() + (False,)
    return out


FIXTURES = _fixtures()
CLOSED = [k for k, m in FIXTURES.items() if m[2]]


@functools.lru_cache(maxsize=None)
def points_of(name):
    """1000 points, shuffled so that every prefix has of each kind: the neighbourhood recipe, up to 40 vertices of the mesh, 10
    points on the surface and 10 each moved by +1e-6 and -1e-6.  Ten each, because of check 3's budget: at a point that close to
    an OPEN surface |wn| is 0.5 to within its distance over the face's size whatever computes it (F = 1 is one lone triangle), so
    all 30 may lie in the band, and 3 % leaves room under the 5 % for the points the approximation itself puts there."""
    v, f, _ = FIXTURES[name]
    seed = sum(name.encode())
    used = np.unique(f)[:40]
    on = [MB.surface_points(v, f, 10, seed + k, off) for k, off in enumerate((0.0, 1e-6, -1e-6))]
    p = np.concatenate([MB.points(v, f, 1000 - len(used) - 30, seed), v[used]] + on).astype(np.float32)
    return np.ascontiguousarray(p[np.random.default_rng(seed).permutation(1000)])


@functools.lru_cache(maxsize=None)
def tree_of(name):
    v, f, _ = FIXTURES[name]
    return MB.build(v, f)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Everything the checks need from the CPU, computed once per fixture: the restated walks (float32 and float64), the float64
    brute force, the float32 distance error, E and the band."""
    v, f, _ = FIXTURES[name]
    p, tree = points_of(name), tree_of(name)
    b64 = MF.query(p, v, f, None, np.float64, keep_d2=False)
    b32 = MF.query(p, v, f, None, np.float32, keep_d2=False)
    dist = MB.walk_distance(tree, p, v, f)
    w32 = MB.walk_winding(tree, p, v, f, MB.BETA, np.float32)["wn"]
    w64 = MB.walk_winding(tree, p, v, f, MB.BETA, np.float64)["wn"]
    E_ = float(np.abs(w64 - b64["wn"]).max())
    floor_d = float(np.abs(b32["dist"].astype(np.float64) - b64["dist"]).max())
    on = b64["dist"] <= floor_d
    return {"b64": b64, "b32": b32, "dist": dist, "w32": w32, "w64": w64, "E": E_, "floor_wn": float(np.abs(w32 - w64)[~on].max()),
            "floor_wn_all": float(np.abs(w32 - w64).max()), "band": np.abs(np.abs(b64["wn"]) - 0.5) <= 2 * E_, "on_surface": on}


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def fit(E):  # noqa: F811
    from topia_xl_amd import fit
    assert (fit.BVH_LEAF, fit.BVH_DELTA_SCALE, fit.BVH_BETA) == (MB.LEAF, MB.DELTA_SCALE, MB.BETA)
    return fit


def _defined(fit, bvh):
    """The bytes of a tree's workspace that the build defines: the records and the order, the nodes and the float64 sums from node 1
    on (node 0 does not exist; the head and the bounding-box partials are scratch)."""
    lay, F, L = bvh.layout, bvh.f.shape[0], bvh.layout["L"]
    return [bvh.ws[lay["recs"]:lay["orig"] + 4 * F], bvh.ws[lay["nodes"] + fit.BVH_NODE_BYTES:lay["nodes"] + fit.BVH_NODE_BYTES * 2 * L],
            bvh.ws[lay["mom"] + fit.BVH_MOMENT_BYTES:lay["mom"] + fit.BVH_MOMENT_BYTES * 2 * L]]


@functools.lru_cache(maxsize=None)
def _bvh(name):
    from topia_xl_amd import fit
    v, f, _ = FIXTURES[name]
    return fit.MeshBVH(_t(v), _t(f))


# ------------------------------------------------------------------------------------------------ 1. the tree
@pytest.mark.parametrize("name", list(FIXTURES))
def test_tree_equals_the_restatement(fit, name):
    bvh, tree = _bvh(name), tree_of(name)
    lay, F, L = bvh.layout, tree["F"], tree["L"]
    assert (lay["L"], lay["nleaf"]) == (L, tree["nleaf"]) and bvh.ws.numel() == lay["total"]
    assert np.array_equal(bvh.order.cpu().numpy(), tree["order"])
    ws = bvh.ws.cpu().numpy()
    assert np.array_equal(ws[lay["orig"]:lay["orig"] + 4 * F].view(np.int32), tree["order"])
    nodes = ws[lay["nodes"]:lay["nodes"] + fit.BVH_NODE_BYTES * 2 * L].view(np.uint32).reshape(2 * L, 24)
    want = MB.node_image(tree).view(np.uint32)
    diff = np.argwhere(nodes[1:] != want[1:])
    assert diff.size == 0, f"{len(diff)} words of {nodes[1:].size} differ; the first at node {diff[0][0] + 1}, word {diff[0][1]}"
    mom = ws[lay["mom"]:lay["mom"] + fit.BVH_MOMENT_BYTES * 2 * L].view(np.float64).reshape(2 * L, 16)
    assert np.array_equal(mom[1:], tree["mom"][1:])
    again = fit.MeshBVH(bvh.v, bvh.f)                                             # two builds: the same bits
    assert all(torch.equal(a, b) for a, b in zip(_defined(fit, again), _defined(fit, bvh)))


# ------------------------------------------------------------------------------------------------ 2. the query
def _queries(fit, name, n, C, sort_points, beta=MB.BETA):
    v, f, _ = FIXTURES[name]
    p = _t(points_of(name)[:n])
    attr = None if C == 0 else _t(MF.affine_attr(v, C))
    got = fit.mesh_field_query(p, _t(v), _t(f), attr, bvh=_bvh(name), beta=beta, sort_points=sort_points)
    brute = fit.mesh_field_query(p, _t(v), _t(f), attr)
    return got, brute


@pytest.mark.parametrize("name", list(FIXTURES))
def test_query_against_the_brute_force_kernel_and_the_restatement(fit, name):
    v, f, closed = FIXTURES[name]
    ref = reference(name)
    E_, floor = ref["E"], ref["floor_wn"]
    print(f"{name}: F = {f.shape[0]}, E = {E_:.4f}, {100 * ref['band'].mean():.1f} % of the points in the band, "
          f"{int(ref['on_surface'].sum())} on the surface to float32, float32 walk against float64 walk {floor:.3e}")
    assert ref["band"].mean() <= 0.05
    worst = 0.0
    for n in NS:
        for C, sort_points in ((5, False), (5, True)) + (((0, False), (8, True)) if n == 1000 else ()):
            (d, face, wn, a), (bd, bface, bwn, ba) = _queries(fit, name, n, C, sort_points)
            tag = (name, n, C, sort_points)
            assert tuple(d.shape) == tuple(face.shape) == tuple(wn.shape) == (n,) and face.dtype == torch.int32
            # 1. bit for bit the brute-force kernel's, and the float32 restatement's
            assert torch.equal(face, bface), (tag, int((face != bface).sum()))
            assert fp.same_bits(d, bd), (tag, int((_bits(d) != _bits(bd)).sum()))
            assert (a is None and ba is None and C == 0) or (tuple(a.shape) == (n, C) and fp.same_bits(a, ba)), tag
            assert np.array_equal(face.cpu().numpy(), ref["dist"]["face"][:n]), tag
            assert np.array_equal(_bits(d), ref["dist"]["dist"][:n].view(np.uint32)), tag
            # 2. wn against the float64 restatement of the same walk.  The float32 walk's own error over ALL points is 1.0 wherever a
            # point lies on the surface to float32 (its face's term is +pi in one precision and -pi in the other), and 4 x that
            # holds nothing: the bound is taken over the other points and held there, and a point on the surface is held to the
            # same bound against the float32 walk, whose side of pi the kernel must share.  (The bound over all points follows.)
            w, on = wn.cpu().numpy().astype(np.float64), ref["on_surface"][:n]
            err = float(np.abs(w - np.where(on, ref["w32"][:n].astype(np.float64), ref["w64"][:n])).max())
            worst = max(worst, err)
            assert np.isfinite(w).all() and err <= 4 * floor, (tag, err, 4 * floor)
            assert float(np.abs(w - ref["w64"][:n]).max()) <= 4 * ref["floor_wn_all"], tag
            # 3. inside / outside against the float64 brute force, outside the band
            inside, clear = np.abs(w) >= 0.5, ~ref["band"][:n] & ~on
            assert np.array_equal(inside[clear], (np.abs(ref["b64"]["wn"][:n]) >= 0.5)[clear]), tag
            # 4. the brute-force kernel's sign on a closed mesh
            if closed:
                assert np.array_equal(inside, np.abs(bwn.cpu().numpy()) >= 0.5), tag
    print(f"{name}: wn within {worst:.3e} of the float64 walk (bound {4 * floor:.3e})")


def test_opening_every_node_gives_the_brute_force_winding_number(fit):
    """beta = 1e9: nothing is approximated, and wn is the exact sum in the tree's order - within the fp32 bound of check 2 of the
    float64 brute force: 4 x the float32 brute-force restatement's own error, taken over the points that are not on the surface to
    float32; those are held to the same bound against the float32 brute force, as in check 2."""
    for name in ("icosphere", "hemisphere", "degenerate"):
        ref = reference(name)
        (d, face, wn, _), (bd, bface, _, _) = _queries(fit, name, 1000, 0, False, beta=1e9)
        on, b32, b64 = ref["on_surface"], ref["b32"]["wn"].astype(np.float64), ref["b64"]["wn"]
        bound = 4 * float(np.abs(b32 - b64)[~on].max())
        err = float(np.abs(wn.cpu().numpy().astype(np.float64) - np.where(on, b32, b64)).max())
        print(f"{name}: beta = 1e9: {err:.3e} from the float64 brute force (bound {bound:.3e})")
        assert err <= bound and torch.equal(face, bface) and fp.same_bits(d, bd)


def test_query_without_points_and_bad_arguments(fit):
    v, f, _ = FIXTURES["box"]
    bvh = _bvh("box")
    e = bvh.query(torch.empty(0, 3, device=DEV), _t(MF.affine_attr(v)))
    assert tuple(e[0].shape) == (0,) and tuple(e[3].shape) == (0, 5)
    with pytest.raises(ValueError):
        bvh.query(_t(points_of("box")), beta=-1.0)
    with pytest.raises(ValueError):
        fit.mesh_field_query(_t(points_of("box")), _t(v), _t(f[:5]), bvh=bvh)       # another mesh's tree
    cached = fit.MeshBVH(_t(v), _t(f), ws=bvh.ws)                                   # a cached workspace serves as it is
    assert fp.same_bits(cached.query(_t(points_of("box")))[2], bvh.query(_t(points_of("box")))[2])


def test_out_of_range_indices_raise_at_the_constructor(fit):
    from topia_xl_amd._lib import PrimxError
    v, f, _ = FIXTURES["F=65"]
    for bad in (v.shape[0], -1, 2 ** 31 - 1):
        fb = f.copy()
        fb[7, 1] = bad
        with pytest.raises(PrimxError, match=r"outside \[0, V\)"):
            fit.MeshBVH(_t(v), _t(fb))
        with pytest.raises(PrimxError, match=r"outside \[0, V\)"):
            fit.MeshField(_t(v), _t(fb), accel="bvh")
    d = fit.MeshBVH(_t(v), _t(f)).query(_t(points_of("F=65")))[0]                   # and the next good mesh is served
    assert bool(torch.isfinite(d).all())


# ------------------------------------------------------------------------------------------------ 3. whole paths
def _ico_mesh():
    v, f, _ = FIXTURES["icosphere"]
    attr = MF.affine_attr(v)
    return (_t(v), _t(f), _t(attr[:, :3]), _t(attr[:, 3]), _t(attr[:, 4]))


def test_mesh_to_primitives_is_bit_identical_with_the_tree(fit):
    """P = 256 primitives of 4^3 voxels from 2048 candidates on the icosphere (closed: check 4 says the signs are the brute-force
    kernel's, and dist and the attributes are its bits)."""
    kw = dict(num_prims=256, prim_shape=4, candidates=2048)
    brute, _ = fit.mesh_to_primitives(_ico_mesh(), **kw)
    fast, info = fit.mesh_to_primitives(_ico_mesh(), accel="bvh", **kw)
    assert tuple(fast.shape) == (256, 4 + 6 * 64) and fp.same_bits(fast, brute)
    with pytest.raises(ValueError):
        fit.mesh_to_primitives(_ico_mesh(), accel="grid", **kw)


def test_refine_runs_with_the_tree(fit):
    kw = dict(num_prims=64, prim_shape=4, candidates=1024, refine_kw=dict(samples_per_prim=32))
    recon, info = fit.mesh_to_primitives(_ico_mesh(), accel="bvh", refine=2, **kw)
    assert len(info["refine"]["loss"]) == 2 and bool(torch.isfinite(recon).all()) and all(np.isfinite(info["refine"]["loss"]))
    start, _ = fit.mesh_to_primitives(_ico_mesh(), accel="bvh", **{k: kw[k] for k in ("num_prims", "prim_shape", "candidates")})
    mesh = (info["v"], info["f"]) + _ico_mesh()[2:]
    again, rinfo = fit.refine_primitives(start, mesh, 2, samples_per_prim=32, accel="bvh")     # a field built there, from the mesh
    assert bool(torch.isfinite(again).all()) and fp.same_bits(rinfo["target"], info["refine"]["target"])


def test_compare_meshes_on_the_exact_surface_equals_the_brute_force_dict(fit):
    from topia_xl_amd import metrics
    a = tuple(_t(x) for x in FIXTURES["icosphere"][:2])
    b = tuple(_t(x) for x in FIXTURES["icosphere+box"][:2])
    brute = metrics.compare_meshes(a, b, n=3000, surface=True)
    fast = metrics.compare_meshes(a, b, n=3000, surface=True, accel="bvh")
    assert fast == brute and fast["hausdorff"] > 0
    assert metrics.compare_meshes(a, b, n=3000, accel="bvh") == metrics.compare_meshes(a, b, n=3000)   # sample to sample: untouched


# ------------------------------------------------------------------------------------------------ 4. footprint
def test_footprint_of_build_and_query(fit):
    """Inside footprint.hold: intact guards around the tree's workspace, the keys and the outputs, unchanged const operands, and
    results that depend neither on what torch.empty holds (the workspace may hold anything at entry) nor on the guard."""
    v, f, _ = FIXTURES["F=549"]
    p, attr = points_of("F=549"), MF.affine_attr(v)

    def case(g):
        gi = lambda a, name: g.guard_input(_t(a), name).t   # noqa: E731
        tv, tf, tp, ta = gi(v, "v"), gi(f, "f"), gi(p, "x"), gi(attr, "attr")
        bvh = fit.MeshBVH(tv, tf)
        return [bvh.order, _defined(fit, bvh), bvh.query(tp, ta), bvh.query(tp[:257], None, sort_points=True)]

    out = fp.hold(case)
    ref = reference("F=549")
    assert np.array_equal(out[2][1].cpu().numpy(), ref["dist"]["face"]) and tuple(out[2][3].shape) == (1000, 5)


# ------------------------------------------------------------------------------------------------ 5. stream order
@TS.case(BUILD_CASE, ["primx_mesh_bvh_build"])
def _stream_build(E, dtype):  # noqa: F811
    """Both passes and torch's sort between them on late v and f (the poison of f is 0, a wrong but addressable value)."""
    from topia_xl_amd import fit
    v, f, _ = FIXTURES["F=549"]

    def make(k):
        return {"v": _t(v) * (1.0 + 0.25 * k), "f": _t(np.roll(f, k, axis=0))}

    def call(ctx, i, probe):
        bvh = fit.MeshBVH(i["v"], i["f"])
        return [bvh.order, _defined(fit, bvh)]
    return make, call, None


@TS.case(QUERY_CASE, ["primx_mesh_bvh_query"])
def _stream_query(E, dtype):  # noqa: F811
    """The query alone, on a late tree, late points and late attributes: one launch, nothing read back.  The tree travels as
    int32 words, whose poison is 0: a root without faces, so a walk that ran early would follow no index."""
    from topia_xl_amd import fit
    v, f, _ = FIXTURES["F=549"]
    trees = [fit.MeshBVH(_t(v) * (1.0 + 0.25 * k), _t(f)) for k in range(2)]

    def make(k):
        return {"x": _t(points_of("F=549")) * (1.0 + 0.25 * k), "attr": _t(MF.affine_attr(v)) + k, "ws": trees[k].ws.view(torch.int32).clone()}

    def call(ctx, i, probe):
        return list(fit.MeshBVH(trees[0].v, trees[0].f, ws=i["ws"].view(torch.uint8)).query(i["x"], i["attr"]))
    return make, call, None


@pytest.mark.parametrize("name", [BUILD_CASE, QUERY_CASE])
def test_stream_order_of_the_bvh_entry_points(E, called, name):  # noqa: F811  (`called` is the imported fixture)
    """The body of tests/test_hip_streams.py::test_stream_order for the cases registered above: the build's read-back is its
    documented synchronisation, the query documents none."""
    c = TS.CASES[name]
    make, call, setup = c.build(E, None)
    rep = so.run(name, make, call, E.S, E.blocker, setup=setup, must_sync=name in TS.MUST_SYNC)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{name} declares entry points it did not call: {missing}"
