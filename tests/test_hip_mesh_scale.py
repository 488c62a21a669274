"""The mesh export kernels at the size that ships (csrc/mcubes.hip, meshclean.hip, meshdecim.hip, texbake.hip, mesh.py):
a 256^3 lattice, meshes of 0.15-6.9 M faces and 2048^2 textures, against the same numpy restatements and with the same
comparisons as the small-size tests (tests/test_hip_mesh.py, test_hip_meshclean.py, test_hip_meshdecim.py,
test_hip_texbake.py), whose helpers this module calls.  Every test first asserts, in plain arithmetic on the sizes, that it
reaches the path it is there for: the one-workgroup scan with more than one block sum per thread (`per >= 2`: more than
2^20 items), its ragged last run and idle trailing threads, several chunks per field query, the saturated merge grid.
Where a case is a row of DESIGN.md's "Mesh cleanup" / "Mesh decimation" tables or of README's status paragraph, the quoted
counts are asserted as literals.

Meshes (V vertices, F faces):

    gyroid256       sin x cos y + sin y cos z + sin z cos x over [0, 6 pi]^3 at 256^3:   V   952 848, F 1 892 268
    gyroid256_8pi   the same over [0.25, 0.25 + 8 pi]^3:                                 V 1 269 786, F 2 521 828
    ellipsoid       a perturbed ellipsoid on a 131 x 257 x 67 lattice (2 255 689 points, nblk 2203, per 3: thread 734
                    scans one block sum, the threads after it none), iso 0 and 0.0137:   V 49 154 / 50 520, F 98 304 / 101 036
    sphere256       extract_mesh(oracle.synth.sphere_field, 256):                        V    77 118, F   154 232
    sample256       extract_mesh(oracle.synth.sample_field, 256):                        V 3 517 979, F 6 917 478
    sample128       the same at 128:                                                     V   799 132, F 1 520 544

The 8 pi gyroid is shifted by 0.25 because the unshifted one (V 1 269 660) has 41 zero-area faces (vertices that round onto
one lattice point), which `meshdecim_numpy.check_invariants` does not admit in an output; the shifted one has none, so the
decimation is held to every invariant.  The 6 pi gyroid keeps its 28 zero-area faces for the cleanup (rule R4).

Single-thread restatement times seen when the module was written (seconds): marching cubes 4 (256^3), 0.2 (ellipsoid);
`meshclean_numpy.clean` 31 / 57 (gyroid256, 1 % / 0.3 %), 37 / 64 (gyroid256_8pi), 38 (sample128), its `merge_rounds` 31 and
15 (gyroid256 1 %, sample128; it evaluates only vertices whose neighbours changed - rescanning every pair in each of 456
rounds took 295); the cleanup of sample256, restatement and GPU together, 153; `meshdecim_numpy.decimate` 69 plus 66 for the
invariants of input and output (gyroid256_8pi to 3/4); raster and points 0.6, fill 18 (2048^2).  The whole module: 7 minutes.
"""
import time

import numpy as np
import pytest
import torch

from oracle import synth
from tests import mc_numpy
from tests import meshclean_numpy as MC
from tests import meshdecim_numpy as D
from tests import test_hip_mesh as TM
from tests import test_hip_meshclean as TC
from tests import test_hip_meshdecim as TD
from tests import test_hip_texbake as TT
from tests import texbake_numpy as T

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
KW = dict(v_pct=1, min_f=8, min_d=5)                 # inference.py:126
KW_CAPPED = dict(v_pct=0.3, min_f=64, min_d=20)      # the existing small-v_pct case: the merge grid is at its cap
PTS, SCAN_THREADS = 1024, 1024                       # csrc/mesh_common.h: items per block sum, scan threads
ATTRS = ("v", "f", "normals", "albedo", "roughness", "metallic")
_CACHE = {}


@pytest.fixture(scope="module")
def mesh():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import mesh as M
    yield M
    _CACHE.clear()


def _once(key, make):
    """Every lattice, mesh and field of the module is made once."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def scan_shape(items):
    """(nblk, per) of the one-workgroup scan over `items` items: thread t scans block sums [t * per, t * per + per)."""
    nblk = -(-items // PTS)
    return nblk, -(-nblk // SCAN_THREADS)


def reaches_scan_runs(items):
    """More than one block sum per scan thread: the serial carry inside a thread's run is used."""
    return items > 2 ** 20 and scan_shape(items)[1] >= 2


# ---------------------------------------------------------------------------------------------------------------- fields
def gyroid(periods, n=256, phase=0.0):
    """test_vertex_count_at_256's field over [phase, phase + periods * pi]^3."""
    x = np.linspace(phase, phase + periods * np.pi, n, dtype=np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (np.sin(X) * np.cos(Y) + np.sin(Y) * np.cos(Z) + np.sin(Z) * np.cos(X)).astype(np.float32)


def ellipsoid(shape=(131, 257, 67)):
    """A perturbed ellipsoid (semi-axes 0.36 of each extent, off-lattice centre) on a non-cubic lattice."""
    ax = [np.arange(n, dtype=np.float64) for n in shape]
    X, Y, Z = (((a - ((n - 1) / 2.0 + 0.137)) / (0.36 * n)) for a, n in zip(np.meshgrid(*ax, indexing="ij"), shape))
    r = np.sqrt(X * X + Y * Y + Z * Z)
    return (r - 1.0 + 0.08 * np.sin(5 * X) * np.sin(4 * Y + 1.0) * np.cos(3 * Z)).astype(np.float32)


def _mc_mesh(name):
    """(v, normals, f) of a closed-form lattice by the restatement."""
    vol = _once(("vol", name), {"gyroid256": lambda: gyroid(6), "gyroid256_8pi": lambda: gyroid(8, phase=0.25)}[name])
    return _once(("mc", name), lambda: mc_numpy.marching_cubes(vol))


def _field(name):
    return _once(("field", name), lambda: getattr(synth, name + "_field")(DEV))


def _extracted(M, name, R):
    """The bench's own call: extract_mesh(field, resolution=R) with its defaults."""
    return _once(("extract", name, R), lambda: M.extract_mesh(_field(name), resolution=R))


def _host(m):
    return m.v.cpu().numpy(), m.f.cpu().numpy().astype(np.int64)


def _filtered(M, name):
    """The field extract_mesh queries with filter_noise=True."""
    def make():
        field = _field(name)
        return M._filtered_copy(field, M.noise_filter_mask(field.srt_param.detach()))
    return _once(("filtered", name), make)


def _lattice(M, name, R, chunk):
    """The [R, R, R] lattice of the filtered field, assembled from `field.query` in chunks of `chunk` points."""
    def make():
        field = _filtered(M, name)
        with torch.no_grad():
            pts = M.lattice_points(R, DEV)
            grid = torch.empty(pts.shape[0], dtype=torch.float32, device=DEV)
            for lo in range(0, pts.shape[0], chunk):
                grid[lo:lo + chunk] = field.query(pts[lo:lo + chunk])[:, 0]
        return grid.reshape(R, R, R)
    return _once(("lattice", name, R, chunk), make)


# ---------------------------------------------------------------------------------------------------------------- 1. marching cubes
def _mc_exact(M, vol, iso, ref=None):
    n = vol.size
    nblk, per = scan_shape(n)
    assert n > 2 ** 20 and per >= 2, (n, nblk, per)                           # reach: a run of block sums per scan thread
    t0 = time.perf_counter()
    rv, rn, rf = ref if ref is not None else mc_numpy.marching_cubes(vol, iso)
    t1 = time.perf_counter()
    v, nrm, f = TM._mc(M, vol, iso)
    print(f"{vol.shape} iso {iso}: V {len(rv)}, F {len(rf)}, nblk {nblk}, per {per}, restatement {t1 - t0:.1f} s")
    assert v.shape == rv.shape and f.shape == rf.shape and len(f) > 0
    np.testing.assert_allclose(v, rv, rtol=0, atol=1e-6)
    np.testing.assert_allclose(nrm, rn, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(f, rf)
    return rv, rf


def test_mc_exact_order_gyroid256(mesh):
    """256^3 = 2^24 points: nblk = 16 384, 16 block sums per scan thread."""
    vol = _once(("vol", "gyroid256"), lambda: gyroid(6))
    assert scan_shape(vol.size) == (16384, 16)
    rv, rf = _mc_exact(mesh, vol, 0.0, _mc_mesh("gyroid256"))
    assert (len(rv), len(rf)) == (952848, 1892268)


@pytest.mark.parametrize("iso", [0.0, 0.0137])
def test_mc_exact_order_non_cubic_ragged_scan(mesh, iso):
    """131 x 257 x 67: the last block is partly filled, the last scanning thread has a short run and 289 threads none."""
    vol = _once(("vol", "ellipsoid"), ellipsoid)
    n = vol.size
    nblk, per = scan_shape(n)
    assert len(set(vol.shape)) == 3 and n % PTS != 0                         # reach: non-cubic, ragged last block
    assert per >= 2 and nblk % per != 0 and -(-nblk // per) < SCAN_THREADS   # reach: ragged last run, idle threads
    if iso != 0.0:
        assert not (vol == np.float32(iso)).any()                            # not a lattice value
    _mc_exact(mesh, vol, iso)


def test_mc_exact_order_sample_like_256(mesh):
    """The read-back lattice of the sample-like field: the 6.9 M-face mesh README and DESIGN.md quote."""
    vol = _lattice(mesh, "sample", 256, 1000003).cpu().numpy()
    rv, rf = _mc_exact(mesh, vol, 0.0)
    assert (len(rv), len(rf)) == (3517979, 6917478)                          # DESIGN.md, both mesh tables
    assert reaches_scan_runs(len(rv)) and reaches_scan_runs(len(rf))


def test_mc_topology_on_analytic_fields_256(mesh):
    """test_topology_on_analytic_fields (watertight, oriented, Euler characteristic, volume within 1 %, normals) at 256."""
    assert reaches_scan_runs(256 ** 3)
    TM.test_topology_on_analytic_fields(mesh, 256)


# ---------------------------------------------------------------------------------------------------------------- 2. chunked queries
@pytest.mark.parametrize("chunk", [100003, 1009])
def test_chunking_changes_nothing_at_48(mesh, chunk):
    field = _field("sphere")
    R = 48
    ref = mesh.extract_mesh(field, R)
    V = ref.v.shape[0]
    assert R ** 3 > chunk and R ** 3 % chunk != 0 and V % chunk != 0         # reach: several lattice chunks, ragged
    if chunk == 1009:
        assert V > chunk                                                     # reach: several vertex chunks too
    got = mesh.extract_mesh(field, R, chunk=chunk)
    for k in ATTRS:
        assert torch.equal(getattr(got, k), getattr(ref, k)), k


def test_chunking_changes_nothing_sample_like_256(mesh):
    R, default = 256, 1 << 21
    out = _extracted(mesh, "sample", R)
    V = out.v.shape[0]
    assert -(-R ** 3 // default) == 8 and -(-V // default) == 2              # reach: 8 lattice chunks, 2 vertex chunks
    grid = _lattice(mesh, "sample", R, 1000003)
    assert R ** 3 % 1000003 != 0
    v, f, n = mesh.marching_cubes(grid, 0.0, return_normals=True)
    assert torch.equal(out.v, v / (R - 1.0) * 2.0 - 1.0) and torch.equal(out.f, f) and torch.equal(out.normals, n)
    field, c = _filtered(mesh, "sample"), 700001
    assert V % c != 0 and V > c
    with torch.no_grad():
        q = torch.cat([field.query(out.v[lo:lo + c]) for lo in range(0, V, c)])
    assert torch.equal(out.albedo, q[:, 1:4]) and torch.equal(out.roughness, q[:, 4]) and torch.equal(out.metallic, q[:, 5])


# ---------------------------------------------------------------------------------------------------------------- 3. cleanup
def _clean_case(M, name):
    if name in ("gyroid256", "gyroid256_8pi"):
        v, _, f = _mc_mesh(name)
        return v, f
    return _host(_extracted(M, name[:-3], int(name[-3:])))


def _grid_is_capped(v, f, v_pct):
    """The merge grid's cell width is max(1.001 r, largest extent / (GRID_CAP - 1)): capped when the second is larger."""
    p = np.asarray(v, dtype=np.float32)[np.unique(f)]
    ext = float((p.max(0) - p.min(0)).max())
    return ext / (1.001 * float(MC.radius(v, f, v_pct))) > MC.GRID_CAP - 1


CLEAN_DOCUMENTED = {   # DESIGN.md "Mesh cleanup": V, F, V', F', components, removed, non-manifold faces removed, split, rounds
    "sphere256": (77118, 154232, 8037, 15887, 1, 0, 359, 34, 275),
    "sample128": (799132, 1520544, 77088, 95085, 3203, 3049, 45093, 21468, 353),
    "sample256": (3517979, 6917478, 106412, 125061, 4144, 3991, 74121, 33702, 563),
}


def _assert_documented_clean(name, V, F, vo, fo, st):
    got = (V, F, len(vo), len(fo), st["components"], st["components_removed"], st["nonmanifold_faces_removed"],
           st["vertices_split"], st["merge_rounds"])
    print(f"{name}: {got}")
    assert got == CLEAN_DOCUMENTED[name], (name, got, CLEAN_DOCUMENTED[name])


@pytest.mark.parametrize("name,kw", [("sphere256", KW), ("sphere256", KW_CAPPED), ("gyroid256", KW), ("gyroid256", KW_CAPPED),
                                     ("gyroid256_8pi", KW), ("gyroid256_8pi", KW_CAPPED), ("sample128", KW)],
                         ids=lambda x: x if isinstance(x, str) else f"v_pct{x['v_pct']}")
def test_cleanup_bit_exact_at_scale(mesh, name, kw):
    """test_hip_meshclean._check: v', f', vmap, every stats entry, the merge rounds and the invariants."""
    v, f = _clean_case(mesh, name)
    V, F = len(v), len(f)
    if name == "gyroid256_8pi":
        assert reaches_scan_runs(V) and reaches_scan_runs(F) and reaches_scan_runs(3 * F)   # reach: scans over V, F, 3 F
    elif name != "sphere256":
        assert reaches_scan_runs(F) and reaches_scan_runs(3 * F)
    if kw == KW_CAPPED:
        assert _grid_is_capped(v, f, kw["v_pct"])                            # reach: GRID_CAP cells on the longest axis
    t0 = time.perf_counter()
    (vo, fo, _), st = TC._check(mesh, v, f, **kw)
    print(f"{name} {kw}: V {V} -> {len(vo)}, F {F} -> {len(fo)}, {st}; GPU + restatement {time.perf_counter() - t0:.1f} s")
    if kw == KW and name in CLEAN_DOCUMENTED:
        _assert_documented_clean(name, V, F, vo, fo, st)


def _cleaned_sample256(M):
    def make():
        raw = _extracted(M, "sample", 256)
        st = {}
        return M.clean_trimesh(raw, stats=st, **M.CLEAN_ARGS), st
    return _once(("cleaned", "sample256"), make)


def test_cleanup_sample_like_256_documented_and_deterministic(mesh):
    """The largest mesh of the module through `clean_mesh`: the documented counts, the invariants of its output, and a
    second run that gives the same bits."""
    raw = _extracted(mesh, "sample", 256)
    V, F = raw.v.shape[0], raw.f.shape[0]
    assert reaches_scan_runs(V) and reaches_scan_runs(F) and 9 * F < 2 ** 31 and 3 * V < 2 ** 31
    assert dict(mesh.CLEAN_ARGS, repair=True) == dict(KW, repair=True)
    cleaned, st = _cleaned_sample256(mesh)
    _assert_documented_clean("sample256", V, F, cleaned.v, cleaned.f, st)
    MC.check_invariants(*_host(cleaned), KW["min_f"], repaired=True)
    again = mesh.clean_trimesh(raw, **mesh.CLEAN_ARGS)
    for k in ATTRS:
        assert torch.equal(getattr(again, k), getattr(cleaned, k)), k


# ---------------------------------------------------------------------------------------------------------------- 4. decimation
@pytest.mark.parametrize("optimal", [True, False])
def test_decimation_sphere_256_bit_exact(mesh, optimal):
    v, f = _host(_extracted(mesh, "sphere", 256))
    assert len(f) > 100000
    t0 = time.perf_counter()
    (vo, fo, _), st = TD._check(mesh, v, f, 100000, optimalplacement=optimal)
    print(f"GPU + restatement {time.perf_counter() - t0:.1f} s")
    assert not st["stalled"] and len(fo) in (100000, 99999)
    if optimal:                                                              # DESIGN.md "Mesh decimation", README
        assert (len(v), len(vo), len(f), len(fo), st["rounds"]) == (77118, 50002, 154232, 100000, 16)


def test_decimation_above_2_20_vertices_bit_exact(mesh):
    """A quarter of 2.5 M faces in few rounds: many collapses per round, scans over V, F and 3 F items."""
    v, _, f = _mc_mesh("gyroid256_8pi")
    assert (len(v), len(f)) == (1269786, 2521828)
    assert reaches_scan_runs(len(v)) and reaches_scan_runs(len(f)) and reaches_scan_runs(3 * len(f))
    target = 3 * len(f) // 4
    t0 = time.perf_counter()
    (vo, fo, _), st = TD._check(mesh, v, f, target)
    print(f"GPU + restatement {time.perf_counter() - t0:.1f} s")
    assert not st["stalled"] and len(fo) in (target, target - 1)
    assert max(st["round_collapses"]) > 2 ** 14                              # reach: many collapses in one round


def test_decimation_cleaned_sample_like_stalls_bit_exact(mesh):
    """The shipped path's decimation input (cleanup first): the restatement stalls at the face count the GPU stalls at.
    The cleaned mesh has merged vertices, so the input-topology part of the invariants is left out, as for the other
    stalling mesh of the decimation tests."""
    cleaned, _ = _cleaned_sample256(mesh)
    v, f = _host(cleaned)
    (vo, fo, _), st = TD._check(mesh, v, f, 100000, manifold=False)
    assert st["stalled"] and len(fo) > 100000
    print(f"cleaned sample256: V {len(v)} -> {len(vo)}, F {len(f)} -> {len(fo)}, rounds {st['rounds']}")
    assert (len(v), len(vo), len(f), len(fo), st["rounds"]) == (106412, 87586, 125061, 100191, 42)   # DESIGN.md, README


def test_decimation_raw_sample_like_256_documented_and_deterministic(mesh):
    """6.9 M faces through `decimate_mesh` (no restatement at this size: 276 rounds of it): the documented counts, and a
    second run that gives the same bits.  `decimate_mesh` on the module's largest restated mesh is run twice as well."""
    raw = _extracted(mesh, "sample", 256)
    assert reaches_scan_runs(raw.v.shape[0]) and reaches_scan_runs(3 * raw.f.shape[0])
    st = {}
    a = mesh.decimate_mesh(raw.v, raw.f, 100000, return_vmap=True, stats=st)
    b = mesh.decimate_mesh(raw.v, raw.f, 100000, return_vmap=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert (a[0].shape[0], a[1].shape[0], st["rounds"], st["stalled"]) == (103697, 137478, 276, True)
    v, _, f = _mc_mesh("gyroid256_8pi")
    vd, fd = TD._dev(v, f)
    a = mesh.decimate_mesh(vd, fd, 3 * len(f) // 4, return_vmap=True)
    b = mesh.decimate_mesh(vd, fd, 3 * len(f) // 4, return_vmap=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------- 5. texture bake
@pytest.mark.parametrize("size", [(2048, 2048), (2048, 1536)])
def test_texture_bake_2048(mesh, size):
    """The shipped mesh of the sphere field (cleanup, then the 100 000-face cap) on a 2048-wide atlas: raster, compacted
    texels and points in raster order, and the fill."""
    W, H = size
    nblk, per = scan_shape(W * H)
    assert W * H > 2 ** 20 and per >= 2                                      # reach: texel compaction, per = 4 and 3
    field = _filtered(mesh, "sphere")
    m = _once(("shipped", "sphere256"), lambda: mesh.extract_mesh(_field("sphere"), 256, clean=True,
                                                                  decimate=mesh.DECIMATE_TARGET))
    v, f = _host(m)
    assert 0 < len(f) <= mesh.DECIMATE_TARGET
    a = mesh.uv_unwrap(m.v, m.f, m.normals, size)
    assert a.size == (W, H) and tuple(a.face_id.shape) == (H, W)
    t0 = time.perf_counter()
    texel, pts = TT._check_atlas(mesh, a, v, f)                              # T.raster, T.points and the atlas's layout
    t1 = time.perf_counter()
    fid, cover, covered, doubly, _ = mesh.atlas_raster(a.uv_fixed, a.f, W, H)
    assert torch.equal(fid, a.face_id) and (covered, doubly) == (a.n_covered, 0)
    np.testing.assert_array_equal(cover.cpu().numpy(), (a.face_id >= 0).cpu().numpy().astype(np.int32))
    assert texel.shape[0] == a.n_covered > 2 ** 20 // 4
    with torch.no_grad():
        q = torch.cat([field.query(pts[lo:lo + (1 << 21)]) for lo in range(0, pts.shape[0], 1 << 21)])
    alb, mr = mesh.fill_textures(q, texel, a.face_id)
    t2 = time.perf_counter()
    ralb, rmr = T.fill(q.cpu().numpy(), texel.cpu().numpy(), (a.face_id >= 0).cpu().numpy())
    print(f"{W} x {H}: F {len(f)}, covered {a.n_covered}, charts {a.n_charts}, split rounds {a.split_rounds}; "
          f"raster + points restatement {t1 - t0:.1f} s, fill restatement {time.perf_counter() - t2:.1f} s")
    np.testing.assert_array_equal(alb.cpu().numpy(), ralb)
    np.testing.assert_array_equal(mr.cpu().numpy(), rmr)


def test_labels_and_components_above_2_20_faces(mesh):
    v, n, f = _mc_mesh("gyroid256")
    assert reaches_scan_runs(len(f))                                         # reach: face components with F > 2^20
    vd, fd = TT._dev(v), TT._dev(f, torch.int32)
    for normals in (n, None):
        lab = mesh.face_labels(vd, fd, None if normals is None else TT._dev(normals)).cpu().numpy()
        rlab, rcomp, rnc = T.charts(v, f, normals)
        np.testing.assert_array_equal(lab, rlab)
        assert 6 * len(v) + 5 < 2 ** 31
        comp, nc = mesh.face_components(TT._dev(f * 6 + rlab[:, None], torch.int32), 6 * len(v))
        assert nc == rnc, (nc, rnc)
        np.testing.assert_array_equal(comp.cpu().numpy(), rcomp)
        print(f"gyroid256: {len(f)} faces, {rnc} charts")


# ---------------------------------------------------------------------------------------------------------------- the largest case
def test_cleanup_sample_like_256_bit_exact(mesh):
    """The 6.9 M-face mesh against the restatement, last because it is the module's longest case by far."""
    v, f = _host(_extracted(mesh, "sample", 256))
    V, F = len(v), len(f)
    assert reaches_scan_runs(V) and reaches_scan_runs(F) and reaches_scan_runs(3 * F)
    t0 = time.perf_counter()
    (vo, fo, _), st = TC._check(mesh, v, f, **KW)
    print(f"sample256 {KW}: V {V} -> {len(vo)}, F {F} -> {len(fo)}, {st}; GPU + restatement {time.perf_counter() - t0:.1f} s")
    _assert_documented_clean("sample256", V, F, vo, fo, st)
