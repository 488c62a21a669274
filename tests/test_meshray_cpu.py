"""tests/meshray_numpy.py and the Python surface of the mesh ray queries without a GPU: the float32 restatement against float64
away from the edges, watertightness from interior points, the restated walk against the restated brute force on rays that graze
the tree's boxes (the experiment behind rule R5's margin), the visibility sign on the flipped sphere - the reason the feature
exists - and the ABI bookkeeping of the two entry points."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import meshbvh_numpy as MB
from tests import meshfield_numpy as MF
from tests import meshray_numpy as MR
from tests import test_hip_meshray as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "3dtopia-xl_amd", "csrc")
NAMES = TR.NAMES
AWAY = 2.0 ** -18        # an edge function counts as away from 0 above 4 x its fp32 error, 14 x 2^-24 s^2 (MR.edge_functions)


def _same(a, b):
    return np.array_equal(a["face"], b["face"]) and np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)) and \
        np.array_equal(np.ascontiguousarray(a["bary"]).view(np.uint32), np.ascontiguousarray(b["bary"]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 1. against ground truth
@pytest.mark.parametrize("name", list(TR.FIXTURES))
def test_float32_agrees_with_float64_away_from_the_edges(name):
    """Hit / miss and face of the float32 brute force equal the float64 one's for every ray whose float64 edge functions are all
    away from 0.  Along the whole line (tmin = -inf): a ray that starts ON the surface has its first t within rounding of tmin = 0
    in both precisions, which is a matter of t, not of the edge functions; the tmin / tmax windows are held bit for bit against
    the float32 restatement on the device."""
    v, f, _ = TR.FIXTURES[name]
    o, d = TR.rays_of(name)
    b32 = MR.brute(o, d, v, f, -np.inf, np.inf, np.float32)
    b64 = MR.brute(o, d, v, f, -np.inf, np.inf, np.float64)
    away = MR.edge_functions(o, d, v, f)[:, MB.face_kinds(v, f) == 0].min(1) > AWAY       # (a zero-area face is never hit: R2)
    print(f"{name}: {int(away.sum())} of 1000 rays pass every edge at a distance, {int(b64['hit'][away].sum())} of them hit")
    assert away.sum() >= 250                                          # (two fifths of the set aim at vertices and edges)
    assert np.array_equal(b32["hit"][away], b64["hit"][away]) and np.array_equal(b32["face"][away], b64["face"][away])
    hit = away & b64["hit"]
    scale = np.abs(v).max() + np.abs(o).max(1) + np.abs(b64["t"])
    assert np.all(np.abs(b32["t"][hit] - b64["t"][hit]) <= 2.0 ** -12 * scale[hit])      # t itself: near grazing it is ill-conditioned
    assert np.all(b32["t"][~b32["hit"]] == np.inf) and np.all(b32["face"][~b32["hit"]] == -1) and not b32["bary"][~b32["hit"]].any()
    assert not np.isnan(b32["t"]).any() and not np.isnan(b32["bary"]).any()


@pytest.mark.parametrize("name", TR.CLOSED)
def test_no_interior_ray_of_the_restatement_misses(name):
    """From strictly interior points of a closed mesh: 200 seeded directions and the directions to every vertex and every edge
    midpoint, where the hit lies on or next to shared edges and vertices."""
    v, f, _ = TR.FIXTURES[name]
    o, d = TR.interior_of(name)
    b = MR.brute(o, d, v, f)
    assert b["hit"].all(), (name, int((~b["hit"]).sum()), o[~b["hit"]][:3], d[~b["hit"]][:3])
    assert np.isfinite(b["t"]).all() and (b["t"] >= 0).all()


def test_the_boxes_corners_and_edges_are_watertight():
    """The sharp case: from the centre of a box with dyadic coordinates the rays pass EXACTLY through its corners and its edges'
    midpoints (and, on a quad's diagonal, through the shared edge of two faces): two or all three edge functions are exactly 0,
    and Moeller-Trumbore may miss both faces there.  Then the box fixture from its fp32 centre."""
    v, f, c = MR.exact_box()
    o, d = MR.interior_rays(v, f, centre=c, n_random=0)
    k = o.shape[0] // 3
    ray = MR.setup(o[:k], d[:k])
    ok, t, _, _ = MR.pairs(ray, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]], MB.face_kinds(v, f), 0.0, np.inf)
    assert k == 26 and ok.any(1).all()
    assert (ok.sum(1)[:8] >= 3).all()                                 # a corner: the three faces' triangles that meet there, at least
    assert np.abs(np.where(ok, t, 1) - 1).max() <= 2.0 ** -22
    b = MR.brute(o, d, v, f)
    assert b["hit"].all() and (b["face"][:k] == np.where(ok, np.arange(12), 99).min(1)).all()       # the lowest face among equals
    v, f, _ = TR.FIXTURES["box"]
    o, d = MR.interior_rays(v, f, n_random=0)
    assert MR.brute(o, d, v, f)["hit"].all()


def test_the_order_is_t_then_face_and_other_kinds_are_never_hit():
    """The degenerate fixture holds one face three times (5, 9 and 11 are (8, 8, 9) - zero area; the box's own faces each once)."""
    v, f, _ = TR.FIXTURES["degenerate"]
    kinds = MB.face_kinds(v, f)
    o, d = TR.rays_of("degenerate")
    b = TR.reference("degenerate")
    assert (kinds != 0).sum() == 7 and not np.isin(b["face"][b["hit"]], np.flatnonzero(kinds != 0)).any()
    twice = np.concatenate([f, f[:4]])                                 # faces 0 .. 3 again, as 19 .. 22: the first of equals wins
    b2 = MR.brute(o, d, v, twice)
    assert _same(b, b2) and (b["face"] < 4).sum() > 50


# ------------------------------------------------------------------------------------------------ 2. the walk, the margin
@pytest.mark.parametrize("name", ["box", "icosphere", "shifted", "slivers", "F=65"])
def test_the_restated_walk_equals_the_brute_force_on_grazing_rays(name):
    """R5 never refuses a node that holds an accepted record: on rays through the corners, along the edges and in the face planes
    (axis-parallel) of the tree's own boxes, from 1, 4 and 64 extents away, and on the fixture's ray set."""
    v, f, _ = TR.FIXTURES[name]
    tree = TR.tree_of(name)
    for scale in (1.0, 4.0, 64.0):
        o, d = MR.grazing_rays(tree, scale, seed=int(scale), nodes=10)
        b, w = MR.brute(o, d, v, f), MR.walk(tree, o, d, v, f)
        assert _same(b, w), (name, scale, int((b["face"] != w["face"]).sum()))
        assert b["hit"].sum() >= 10 or name in ("slivers", "box")
    o, d = TR.rays_of(name)
    b, w = TR.reference(name), MR.walk(tree, o, d, v, f)
    assert _same(b, w)
    live = int((tree["count"][1:] > 0).sum())
    every = MR.walk(tree, o[:64], d[:64], v, f, prune=False)
    ok = MR.setup(o[:64], d[:64])["ok"]
    assert (every["visits"][ok] == live + f.shape[0]).all() and _same(every, {k: a[:64] for k, a in b.items()})
    assert w["visits"].mean() < 0.5 * (live + f.shape[0]) or f.shape[0] < 100
    for tmin, tmax in TR.windows_of(name)[1:]:
        assert _same(MR.brute(o[:300], d[:300], v, f, tmin, tmax), MR.walk(tree, o[:300], d[:300], v, f, tmin, tmax))


@pytest.mark.parametrize("name", ["shifted", "slivers", "F=65"])
def test_the_margin_experiment(name):
    """R5 against each face's OWN box at best = the accepted t: never refused with the chosen margin 2^-20, nor with the 7 x 2^-24
    that DESIGN.md "Mesh rays" derives.  With margin 0 (and even with delta = 0, margin 0) the count is printed: a finding, not a
    requirement - the sheared-frame tests need no margin by construction, only the t interval does."""
    v, f, _ = TR.FIXTURES[name]
    tree = TR.tree_of(name)
    go, gd = MR.grazing_rays(tree, 4.0, seed=2, nodes=6)
    o, d = np.concatenate([TR.rays_of(name)[0], go]), np.concatenate([TR.rays_of(name)[1], gd])
    delta = tree["delta"]
    chosen, pairs = MR.own_box_violations(o, d, v, f, delta)
    derived, _ = MR.own_box_violations(o, d, v, f, delta, margin=7 * 2.0 ** -24)
    zero, _ = MR.own_box_violations(o, d, v, f, delta, margin=0.0)
    bare, _ = MR.own_box_violations(o, d, v, f, 0.0, margin=0.0)
    print(f"{name}: of {pairs} accepted pairs R5 refuses {chosen} at margin 2^-20, {derived} at 7 x 2^-24, {zero} at margin 0, "
          f"{bare} at margin 0 without the boxes' inflation")
    assert pairs > 500 and chosen == 0 and derived == 0
    assert MR.T_MARGIN == 2.0 ** -20 and MR.T_MARGIN >= 2 * 7 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ 3. the sign
def test_visibility_gives_the_sign_on_the_flipped_sphere_and_winding_does_not():
    v, g, f = TR._FLIPPED
    ref = TR.sign_reference("flipped")
    p, held, inside = ref["p"], ref["held"], ref["inside"]
    assert np.array_equal(np.sort(g, 1), np.sort(f, 1)) and (g != f).any(1).sum() == f.shape[0] // 2
    esc = MR.escapes(p, MR.fibonacci(64), v, g, limit=1)
    outside = esc >= 1
    print(f"flipped: {int((~held).sum())} of 1000 points within the float32 distance floor (the nearest at {ref['dist'].min():.2e}); "
          f"visibility wrong at {int((outside == inside)[held].sum())}")
    assert (~held).mean() <= 0.01
    assert np.array_equal(outside[held], ~inside[held])
    wn = MF.query(p, v, g, None, np.float64, keep_d2=False)["wn"]
    wrong = ((np.abs(wn) >= 0.5) != inside) & inside & held
    print(f"flipped: the winding rule is wrong at {int(wrong.sum())} of {int((inside & held).sum())} inside points")
    assert wrong.sum() > 0.5 * (inside & held).sum()
    nearest = np.flatnonzero(held & ~inside)[np.argmin(ref["dist"][held & ~inside])]
    full = MR.escapes(p[nearest:nearest + 1], MR.fibonacci(64), v, g)
    print(f"flipped: the nearest outside point, at {ref['dist'][nearest]:.2e}, has {int(full[0])} escaping rays of 64")
    assert full[0] >= 16
    # the count saturates at the limit, and the orientation does not enter
    some = MR.escapes(p[:60], MR.fibonacci(8), v, g)
    assert np.array_equal(MR.escapes(p[:60], MR.fibonacci(8), v, g, limit=2), np.minimum(some, 2))
    assert np.array_equal(some, MR.escapes(p[:60], MR.fibonacci(8), v, f))


# ------------------------------------------------------------------------------------------------ 4. ABI, Python surface
@pytest.mark.parametrize("name,names", [
    (NAMES[0], ["org", "dir", "n", "tmin", "tmax", "any_hit", "f", "F", "bvh", "bvh_bytes", "t", "face", "bary", "stream"]),
    (NAMES[1], ["pts", "n", "dirs", "D", "tmin", "limit", "f", "F", "bvh", "bvh_bytes", "escapes", "stream"])])
def test_abi_35_declares_the_entry_points_with_the_bound_signatures(name, names):
    from topia_xl_amd import _lib
    assert _lib.ABI_VERSION == 35 and _lib._SINCE[name] == 35 and name not in _lib._FEATURES.values() and _lib._PROBE == 0
    with open(os.path.join(ROOT, "include", "primx_hip.h")) as fh:
        text = fh.read()
    assert "#define PRIMX_ABI_VERSION 35" in text
    section = text[text.index(" * Mesh rays ("):]
    assert "added to ABI 35 without a new number" in section and "Woop" in section
    assert all(f"  R{k}  " in section for k in range(1, 7)) and "2^-20" in section
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", section)
    assert m, "the header's section does not declare it"
    ctype = {"const float*": _lib._p, "float*": _lib._p, "const int*": _lib._p, "int*": _lib._p, "void*": _lib._p, "const void*": _lib._p,
             "int": _lib._i, "int64_t": _lib._l, "float": _lib._f}
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[1] for a in args] == names
    assert [ctype[a.rsplit(" ", 1)[0]] for a in args] == _lib.SIGNATURES[name]


def test_an_ab_build_of_version_35_from_before_the_rays_still_loads(monkeypatch, tmp_path):
    from tests import test_lib_capabilities_cpu as TL
    from topia_xl_amd import _lib
    rest = set(_lib.SIGNATURES) - set(NAMES)
    lib = TL.StandIn(35, rest)
    assert TL._load(monkeypatch, tmp_path, lib) == TL.ALL and lib.bound() == rest
    with pytest.raises(AttributeError):                               # ... and as the package's own library it is refused
        TL._load(monkeypatch, tmp_path, lib, ab=False)
    for one in NAMES:                                                 # each of the two is probed on its own
        part = TL.StandIn(35, rest | {one})
        assert TL._load(monkeypatch, tmp_path, part) == TL.ALL and part.bound() == rest | {one}


def test_the_ray_arithmetic_has_a_header_of_its_own_and_no_stack():
    src = {n: open(os.path.join(CSRC, n)).read() for n in ("meshbvh.hip", "meshray_pair.h", "build.py")}
    bvh, ray = src["meshbvh.hip"], src["meshray_pair.h"]
    assert '#include "meshray_pair.h"' in bvh and '"meshray_pair.h"' in src["build.py"]
    assert "bool ray_pair(" in ray and "bool ray_box(" in ray and "struct Rec" not in ray and "void pair(" not in ray
    assert "RAY_T_MARGIN = 0x1p-20f" in ray and MR.T_MARGIN == 2.0 ** -20 and "(double)cx * (double)by" in ray
    for kernel in ("bvh_raycast_kernel", "bvh_visibility_kernel", "ray_walk"):
        assert kernel in bvh
    body = bvh[bvh.index("void ray_walk"):bvh.index("int bounding_box")] + ray
    assert not re.search(r"\b(?:int|unsigned|float|double)\s+\w+\[", body) and not re.search(r"\batomic[A-Z]\w*\(", body)


def test_stream_table_is_closed_with_the_ray_cases():
    from tests import test_hip_material, test_hip_meshbvh, test_hip_metrics, test_hip_normalmap, test_hip_occlusion, test_hip_primsdf_grad, test_hip_raymarch_grad  # noqa: F401  (the other registering modules)
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    assert {TR.RAY_CASE, TR.VIS_CASE} <= set(TS.CASES) and set(NAMES) <= set(TS.declared())
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n in (TR.RAY_CASE, TR.VIS_CASE)]             # they run in their own module, not twice
    for case in (TR.RAY_CASE, TR.VIS_CASE):
        assert case not in TS.MUST_SYNC and case not in TS.FIRST_CALL_MAY_SYNC           # nothing is read back


def test_the_python_surface():
    import torch

    from topia_xl_amd import fit
    assert fit.SIGNS == ("winding", "visibility")
    for fn in (fit.mesh_to_primitives, fit.refine_primitives, fit.MeshField.__init__, fit.mesh_field):
        s = inspect.signature(fn).parameters
        assert (s["sign"].default, s["sign_directions"].default, s["min_escapes"].default) == ("winding", 64, 1), fn
    s = inspect.signature(fit.MeshBVH.raycast).parameters
    assert list(s)[1:] == ["origins", "dirs", "tmin", "tmax", "any_hit", "attr"]
    assert (s["tmin"].default, s["tmax"].default, s["any_hit"].default, s["attr"].default) == (0.0, float("inf"), False, None)
    s = inspect.signature(fit.MeshBVH.visibility).parameters
    assert list(s)[1:] == ["x", "directions", "tmin", "limit"] and (s["directions"].default, s["tmin"].default, s["limit"].default) == (64, 0.0, 0)
    v, f = (torch.from_numpy(a) for a in MF.box())
    for call in (lambda: fit.MeshField(v, f, sign="visibility"), lambda: fit.MeshField(v, f, accel="bvh", sign="parity"),
                 lambda: fit.mesh_to_primitives((v, f, None, None, None), sign="visibility"),
                 lambda: fit.mesh_to_primitives((v, f, None, None, None), accel="bvh", sign="hits")):
        with pytest.raises((ValueError, RuntimeError)) as e:
            call()
        assert "sign" in str(e.value) or "HIP device" in str(e.value)
    with pytest.raises(ValueError, match="accel"):
        fit._check_sign("visibility", None)
    for doc in (fit.MeshField.__doc__, fit.mesh_to_primitives.__doc__):
        assert "visibility" in doc
    for words in ("unsigned distance", "pocket", "min_escapes", "unmeasured"):
        assert words in fit.MeshField.__doc__, words
    with open(os.path.join(ROOT, "examples", "tokenize_mesh.py")) as fh:
        assert '"--sign"' in fh.read()
    assert np.array_equal(MR.fibonacci(64), __import__("topia_xl_amd.mesh", fromlist=["x"]).occlusion_directions(64).numpy())
