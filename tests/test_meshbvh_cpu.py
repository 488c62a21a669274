"""tests/meshbvh_numpy.py and the Python surface of the mesh BVH without a GPU: the tree's invariants, the restated walk against
the brute-force restatement, the experiment that sets the boxes' inflation, the ABI bookkeeping of the three entry points, the
closure of the stream-order table once tests/test_hip_meshbvh.py has registered its cases, and the wrappers' argument checks."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import meshbvh_numpy as MB
from tests import meshfield_numpy as MF
from tests import test_hip_meshbvh as TB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dtopia-xl_amd", "csrc")
NAMES = TB.NAMES
SMALL = ("F=1", "F=7", "F=8", "F=9", "F=65", "box", "degenerate", "shifted", "hemisphere")


# ------------------------------------------------------------------------------------------------ 1. the tree
@pytest.mark.parametrize("name", list(TB.FIXTURES))
def test_tree_invariants(name):
    v, f, _ = TB.FIXTURES[name]
    t = TB.tree_of(name)
    F, L, nleaf = f.shape[0], t["L"], t["nleaf"]
    assert nleaf == -(-F // 8) and L >= nleaf and L & (L - 1) == 0 and (L == 1 or L // 2 < nleaf)
    # every face in exactly one leaf: the leaves' ranges tile the sorted order, which is a permutation
    assert sorted(t["order"].tolist()) == list(range(F))
    seen = [s for leaf in range(L, 2 * L) if t["count"][leaf] for s in MB.leaf_faces(t, leaf)]
    assert seen == list(range(F)) and [int(c) for c in t["count"][L:L + nleaf]] == [min(8, F - 8 * k) for k in range(nleaf)]
    assert not t["count"][L + nleaf:].any() and t["count"][1] == F
    keys = MB.face_keys(v, f)[0]
    assert bool((np.diff(keys[t["order"]]) > 0).all()) and bool(((keys >> 32) < 2 ** 30).all())
    # boxes contain their faces (inflated by delta), and a parent its children
    tri = v[f[t["order"]]]
    for leaf in range(L, L + nleaf):
        s = list(MB.leaf_faces(t, leaf))
        assert bool((tri[s].min((0, 1)) - t["delta"] == t["lo"][leaf]).all()) and bool((tri[s].max((0, 1)) + t["delta"] == t["hi"][leaf]).all())
    for i in range(1, L):
        for c in (2 * i, 2 * i + 1):
            if t["count"][c]:
                assert bool((t["lo"][i] <= t["lo"][c]).all()) and bool((t["hi"][i] >= t["hi"][c]).all())
        assert t["count"][i] == t["count"][2 * i] + t["count"][2 * i + 1]
    # every vertex of a node within r of p (float32, as the kernel holds them)
    for i in range(1, 2 * L):
        if t["count"][i]:
            s = [k for leaf in _leaves_below(i, L) if t["count"][leaf] for k in MB.leaf_faces(t, leaf)]
            far = np.sqrt(((tri[s].reshape(-1, 3).astype(np.float64) - t["f32"]["p"][i]) ** 2).sum(1)).max()
            assert far <= t["f32"]["r"][i], (i, far, t["f32"]["r"][i])
    # the root's moments are the direct sums (to the rounding of another order of summation)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    A = 0.5 * np.cross(b - a, c - a) * (t["kinds"] == 0)[:, None]
    area, cen = np.linalg.norm(A, axis=1), (a + b + c) / 3
    scale = max(float(np.abs(v).max()), 1e-30)
    assert np.allclose(t["f64"]["N"][1], A.sum(0), rtol=0, atol=1e-12 * scale ** 2 * F)
    if area.sum() > 0:
        p = (area[:, None] * cen).sum(0) / area.sum()
        assert np.allclose(t["f64"]["p"][1], p, rtol=0, atol=1e-12 * scale)
        Cm = ((cen - p)[:, :, None] * A[:, None, :]).sum(0)
        assert np.allclose(t["f64"]["C"][1], Cm, rtol=0, atol=1e-10 * scale ** 3 * F)
    img = MB.node_image(t)
    assert img.shape == (2 * L, 24) and img[:, 7].view(np.int32).tolist() == t["count"].tolist()


def _leaves_below(i, L):
    lo, hi = i, i
    while lo < L:
        lo, hi = 2 * lo, 2 * hi + 1
    return range(lo, hi + 1)


@pytest.mark.parametrize("name", SMALL)
def test_the_walk_with_nothing_pruned_reaches_every_face_once(name):
    v, f, _ = TB.FIXTURES[name]
    t, p = TB.tree_of(name), TB.points_of(name)[:64]
    w = MB.walk_distance(t, p, v, f, prune=False)
    live = int((t["count"][1:] > 0).sum())
    assert bool((w["visits"] == live + f.shape[0]).all())
    pruned = MB.walk_distance(t, p, v, f)
    assert np.array_equal(pruned["face"], w["face"]) and np.array_equal(pruned["d2"].view(np.uint32), w["d2"].view(np.uint32))
    assert bool((pruned["visits"] <= w["visits"]).all())
    every = MB.walk_winding(t, p, v, f, beta=np.inf, dtype=np.float64)          # every node opened: every face's term once
    assert bool((every["visits"] == live + f.shape[0]).all())
    exact = MF.query(p, v, f, None, np.float64, keep_d2=False)["wn"]
    assert np.abs(every["wn"] - exact).max() <= 1e-12


@pytest.mark.parametrize("name", SMALL)
def test_the_restated_walk_equals_the_brute_force_restatement(name):
    """dist, face and d2 identical to MF.query(..., np.float32): the pruning never skips the first minimum."""
    v, f, _ = TB.FIXTURES[name]
    ref, p = TB.reference(name), TB.points_of(name)
    assert np.array_equal(ref["dist"]["face"], ref["b32"]["face"])
    assert np.array_equal(ref["dist"]["dist"].view(np.uint32), ref["b32"]["dist"].view(np.uint32))
    d2 = MF.query(p[:200], v, f, None, np.float32)["d2"]
    assert np.array_equal(ref["dist"]["d2"][:200].view(np.uint32), d2[np.arange(200), ref["dist"]["face"][:200]].view(np.uint32))
    assert np.array_equal(ref["dist"]["d2"][:200].view(np.uint32), d2.min(1).view(np.uint32))
    q = MB.query(p[:50], v, f, MF.affine_attr(v), tree=TB.tree_of(name))
    assert set(q) == {"dist", "face", "d2", "wn", "visits", "attr"} and q["attr"].shape == (50, 5) and q["wn"].dtype == np.float32


@pytest.mark.parametrize("name", SMALL)
def test_the_approximation_error_and_its_band(name):
    """E per fixture, on the CPU (the figures of DESIGN.md "Mesh BVH"); the float32 walk's inside / outside equals the float64 brute
    force's outside the band, the points on the surface to float32 aside (tests/test_hip_meshbvh.py says why)."""
    ref = TB.reference(name)
    print(f"{name}: E = {ref['E']:.4f}, band {100 * ref['band'].mean():.1f} %, float32 walk within {ref['floor_wn']:.3e} of the float64 walk")
    assert ref["E"] < 0.1 and ref["band"].mean() <= 0.05
    clear = ~ref["band"] & ~ref["on_surface"]
    assert np.array_equal((np.abs(ref["w32"]) >= 0.5)[clear], (np.abs(ref["b64"]["wn"]) >= 0.5)[clear])
    assert clear.mean() > 0.5 or name == "slivers"


# ------------------------------------------------------------------------------------------------ 2. the inflation
def _delta_points(v, f):
    return np.concatenate([MB.points(v, f, 1000, 3), MB.surface_points(v, f, 600, 4), MB.surface_points(v, f, 600, 5, 1e-6),
                           MB.surface_points(v, f, 600, 6, -1e-6)])


@pytest.mark.parametrize("name", ["icosphere", "shifted", "slivers"])
def test_delta_zero_is_wrong_and_the_chosen_delta_is_not(name):
    """The brute-force restatement's float32 d2 against the float32 bound of the face's OWN box: without inflation d2 falls below
    the bound on the shifted icosphere (and on the level-3 one); with delta = 2^-17 max|v| it never does, nor with the 2^-20 max|v|
    that is an eighth of it.  DESIGN.md "Mesh BVH" derives 25 x 2^-24 max|v| = 2^-19.4 max|v| as what the argument needs."""
    v, f, _ = TB.FIXTURES[name]
    p, m = _delta_points(v, f), float(np.abs(v).max())
    zero, pairs = MB.own_box_violations(p, v, f, 0.0)
    eighth, _ = MB.own_box_violations(p, v, f, np.float32(m * 2.0 ** -20))
    chosen, _ = MB.own_box_violations(p, v, f, np.float32(m * MB.DELTA_SCALE))
    print(f"{name}: {zero} of {pairs} pairs below the bound at delta = 0, {eighth} at 2^-20 max|v|, {chosen} at 2^-17 max|v|")
    assert chosen == 0 and eighth == 0
    if name == "shifted":
        assert zero > 0
    assert MB.DELTA_SCALE == 2.0 ** -17 and MB.DELTA_SCALE >= 4 * 25 * 2.0 ** -24


def test_the_inflated_tree_keeps_every_first_minimum_on_the_delta_points():
    """The same through the walk: with the chosen delta the pruned walk equals the brute force on the delta experiment's points."""
    v, f, _ = TB.FIXTURES["shifted"]
    p = _delta_points(v, f)[::3]
    want = MF.query(p, v, f, None, np.float32, keep_d2=False)
    got = MB.walk_distance(MB.build(v, f), p, v, f)
    assert np.array_equal(got["face"], want["face"]) and np.array_equal(got["dist"].view(np.uint32), want["dist"].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. ABI
@pytest.mark.parametrize("name,names", [
    (NAMES[0], ["F", "bytes"]),
    (NAMES[1], ["v", "f", "V", "F", "order", "keys", "ws", "ws_bytes", "stream"]),
    (NAMES[2], ["pts", "n", "f", "F", "attr", "C", "bvh", "bvh_bytes", "beta", "dist", "face", "wn", "out_attr", "stream"])])
def test_abi_35_declares_the_entry_points_with_the_bound_signatures(name, names):
    from topia_xl_amd import _lib
    assert _lib.ABI_VERSION == 35 and _lib._SINCE[name] == 35 and name not in _lib._FEATURES.values() and _lib._PROBE == 0
    with open(os.path.join(ROOT, "include", "primx_hip.h")) as fh:
        text = fh.read()
    assert "#define PRIMX_ABI_VERSION 35" in text
    section = text[text.index(" * Mesh BVH ("):]
    assert "added to ABI 35 without a new number" in section and "16-byte aligned, any contents" in section
    assert "2^-17" in section and "the one read-back" in section
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", section)
    assert m, "the header's section does not declare it"
    ctype = {"const float*": _lib._p, "float*": _lib._p, "const int*": _lib._p, "int*": _lib._p, "void*": _lib._p, "const void*": _lib._p,
             "int": _lib._i, "int64_t": _lib._l, "float": _lib._f}
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[1] for a in args] == names
    want = [ctype[a.rsplit(" ", 1)[0]] if a.rsplit(" ", 1)[0] != "int64_t*" else (_lib.C.POINTER(_lib._l) if name == NAMES[0] else _lib._p)
            for a in args]
    assert want == _lib.SIGNATURES[name]


def test_an_ab_build_of_version_35_from_before_the_bvh_still_loads(monkeypatch, tmp_path):
    from tests import test_lib_capabilities_cpu as TL
    from topia_xl_amd import _lib
    rest = set(_lib.SIGNATURES) - set(NAMES)
    lib = TL.StandIn(35, rest)
    assert TL._load(monkeypatch, tmp_path, lib) == TL.ALL and lib.bound() == rest
    with pytest.raises(AttributeError):                               # ... and as the package's own library it is refused
        TL._load(monkeypatch, tmp_path, lib, ab=False)
    for one in NAMES:                                                 # each of the three is probed on its own
        part = TL.StandIn(35, rest | {one})
        assert TL._load(monkeypatch, tmp_path, part) == TL.ALL and part.bound() == rest | {one}


def test_the_kernels_constants_are_the_modules_and_the_pair_arithmetic_is_shared():
    from topia_xl_amd import fit
    src = {n: open(os.path.join(CSRC, n)).read() for n in ("meshbvh.hip", "meshfield.hip", "meshfield_pair.h", "build.py")}
    bvh = src["meshbvh.hip"]
    const = {k: int(v) for k, v in re.findall(r"constexpr int(?:64_t)? (\w+) = (\d+);", bvh)}
    assert (const["LEAF"], const["NODE_F4"] * 16, const["MOM"] * 8, const["HEAD"]) == \
        (fit.BVH_LEAF, fit.BVH_NODE_BYTES, fit.BVH_MOMENT_BYTES, fit.BVH_HEAD_BYTES)
    assert "DELTA_SCALE = 0x1p-17f" in bvh and fit.BVH_DELTA_SCALE == 2.0 ** -17 == MB.DELTA_SCALE and fit.BVH_LEAF == MB.LEAF
    assert "#pragma clang fp contract(off)" in bvh and not re.search(r"\batomic[A-Z]\w*\(", bvh)        # no atomic call on the tree
    # the per-pair arithmetic exists once: in the header both translation units include
    for unit in ("meshbvh.hip", "meshfield.hip"):
        assert '#include "meshfield_pair.h"' in src[unit] and "void pair(" not in src[unit] and "struct Rec" not in src[unit]
    pairh = src["meshfield_pair.h"]
    assert "void pair(" in pairh and "struct Rec" in pairh and "mf_prep_kernel" in pairh and "atan2f(num, dn)" in pairh
    assert '"meshbvh.hip"' in src["build.py"] and '"meshfield_pair.h"' in src["build.py"]
    # no per-thread stack in the query: no array is declared between the kernel's head and its end
    body = bvh[bvh.index("void bvh_query_kernel"):bvh.index("int bounding_box")]
    assert not re.search(r"\b(?:int|unsigned|float)\s+\w+\[", body)
    lay = fit.bvh_layout(549)
    assert (lay["nleaf"], lay["L"], lay["recs"]) == (69, 128, 256) and all(lay[k] % 16 == 0 for k in ("recs", "orig", "nodes", "mom", "part", "total"))
    assert lay["total"] <= 180 * 549 + 10240 and fit.bvh_layout(1)["L"] == 1


# ------------------------------------------------------------------------------------------------ 4. stream table, validation
def test_stream_table_is_closed_with_the_bvh_cases():
    from tests import test_hip_material, test_hip_metrics, test_hip_normalmap, test_hip_occlusion, test_hip_primsdf_grad, test_hip_raymarch_grad  # noqa: F401  (the other registering modules)
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    assert {TB.BUILD_CASE, TB.QUERY_CASE} <= set(TS.CASES) and {NAMES[1], NAMES[2]} <= set(TS.declared())
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n in (TB.BUILD_CASE, TB.QUERY_CASE)]       # they run in their own module, not twice
    assert TB.BUILD_CASE in TS.MUST_SYNC and "read" in TS.MUST_SYNC[TB.BUILD_CASE]     # the build's read-back is documented
    assert TB.QUERY_CASE not in TS.MUST_SYNC and TB.QUERY_CASE not in TS.FIRST_CALL_MAY_SYNC   # the query documents none
    with open(os.path.join(ROOT, "include", "primx_hip.h")) as fh:
        from tests import streamorder as so
        assert NAMES[0] not in so.stream_prototypes(fh.read())                        # the size query takes no stream


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from topia_xl_amd import fit, metrics
    v, f = (torch.from_numpy(a) for a in MF.box())
    p = torch.zeros(5, 3)
    for call in (lambda: fit.MeshBVH(v, f), lambda: fit.MeshField(v, f, accel="bvh")):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    for call in (lambda: fit.MeshField(v, f, accel="grid"), lambda: fit.mesh_to_primitives((v, f, None, None, None), accel="grid"),
                 lambda: fit.refine_primitives(torch.zeros(4, 4 + 6 * 8), (v, f), 1, accel="octree"),
                 lambda: metrics.compare_meshes((v, f), (v, f), n=10, surface=True, accel="grid")):
        with pytest.raises((ValueError, RuntimeError)) as e:
            call()
        assert "accel" in str(e.value) or "HIP device" in str(e.value)
    with pytest.raises(ValueError, match="accel"):
        fit._check_accel("grid")
    assert fit.ACCELS == (None, "bvh") and fit.BVH_BETA == 2.0
    for fn in (fit.mesh_to_primitives, fit.refine_primitives, fit.MeshField.__init__, fit.mesh_field):
        s = inspect.signature(fn).parameters
        assert s["accel"].default is None and s["beta"].default == 2.0, fn
    s = inspect.signature(fit.mesh_field_query).parameters
    assert (s["bvh"].default, s["beta"].default, s["sort_points"].default) == (None, 2.0, False)
    assert inspect.signature(fit.MeshBVH.query).parameters["sort_points"].default is False
    assert inspect.signature(metrics.compare_meshes).parameters["accel"].default is None
    assert "accel" in fit.mesh_to_primitives.__doc__ and "MeshBVH" in metrics.compare_meshes.__doc__


def test_morton_order_is_a_permutation_that_sorts_by_cell():
    """`sort_points`' plumbing on the CPU (torch): a stable permutation; points of one cell stay in their order."""
    from topia_xl_amd import fit
    g = torch.Generator().manual_seed(3)
    x = torch.rand(500, 3, generator=g)
    perm = fit.morton_order(x)
    assert sorted(perm.tolist()) == list(range(500))
    same = torch.zeros(7, 3)                                          # no extent: every code is 0, the order stays
    assert fit.morton_order(same).tolist() == list(range(7))
    corners = torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert fit.morton_order(corners).tolist() == [1, 3, 2, 0]         # x is the highest bit of a cell, z the lowest
