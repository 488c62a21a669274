"""Mesh cleanup on the MI355X (csrc/meshclean.hip, mesh.clean_mesh): bit-exact against the numpy restatement of rules
R0-R8 (tests/meshclean_numpy.py) on marching-cubes and hand-built meshes, the invariants of every output, edge cases and
call shapes, the wiring into extract_mesh / extract_texmesh, and one end-to-end case where only the cleaned mesh bakes."""
import numpy as np
import pytest
import torch

from tests import mc_numpy
from tests import meshclean_numpy as MC
from tests import test_meshclean_cpu as H
from tests.test_hip_mesh import _synthetic_field

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
KW = dict(v_pct=1, min_f=8, min_d=5)


@pytest.fixture(scope="module")
def mesh():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import mesh as M
    return M


def _gpu_clean(M, v, f, stats=None, **kw):
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(DEV)
    fd = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)).to(DEV)
    vo, fo, vmap = M.clean_mesh(vd, fd, return_vmap=True, stats=stats, **kw)
    assert vo.dtype == torch.float32 and fo.dtype == torch.int32 and vmap.dtype == torch.int64 and vo.is_cuda
    return vo.cpu().numpy(), fo.cpu().numpy().astype(np.int64), vmap.cpu().numpy()


def _check(M, v, f, **kw):
    st = {}
    got = _gpu_clean(M, v, f, stats=st, **kw)
    ref_st = {}
    ref = MC.clean(v, f, stats=ref_st, **kw)
    for a, b, name in zip(got, ref, ("v", "f", "vmap")):
        assert a.shape == b.shape and np.array_equal(a, b), (name, kw, a.shape, b.shape)
    for k, x in ref_st.items():
        assert st[k] == x, (k, st[k], x, kw)
    if kw.get("v_pct", 1.0) > 0 and len(f):
        assert st["merge_rounds"] == MC.merge_rounds(v, f, kw.get("v_pct", 1.0))[1]
    MC.check_invariants(got[0], got[1], kw.get("min_f", 64), repaired=kw.get("repair", True))
    return got, st


PARAMS = [dict(v_pct=1, min_f=8, min_d=5), dict(v_pct=0, min_f=0, min_d=0), dict(v_pct=2.5, min_f=64, min_d=20),
          dict(v_pct=0.5, min_f=0, min_d=5, repair=False), dict(v_pct=1, min_f=8, min_d=0)]


@pytest.mark.parametrize("kw", PARAMS)
def test_analytic_fields_bit_exact(mesh, kw):
    for name, (vol, *_) in mc_numpy.analytic_fields(64).items():
        v, _, f = mc_numpy.marching_cubes(vol)
        _check(mesh, v, f, **kw)


@pytest.mark.parametrize("kw", PARAMS)
def test_noise_bit_exact(mesh, kw):
    vol = np.random.default_rng(4).standard_normal((24, 24, 24)).astype(np.float32)
    v, _, f = mc_numpy.marching_cubes(vol, 0.2)
    (_, _, _), st = _check(mesh, v, f, **kw)
    if kw.get("repair", True) and kw["v_pct"] > 0:
        assert st["nonmanifold_candidates"] > 0 and st["vertices_split"] > 0     # the merge makes the mesh non-manifold


def test_synthetic_field_bit_exact(mesh):
    field = _synthetic_field()
    m = mesh.extract_mesh(field, resolution=64, filter_noise=False)
    v, f = m.v.cpu().numpy(), m.f.cpu().numpy()
    for kw in (KW, dict(v_pct=0.3, min_f=64, min_d=20), dict(v_pct=0, min_f=8, min_d=5)):
        (_, _, _), st = _check(mesh, v, f, **kw)
        assert st["components_removed"] > 0                                       # the noise primitives' blobs


def test_hand_built_meshes_bit_exact(mesh):
    cases = [H.tetra(), H.join(H.strip(7), H.strip(8, origin=(0, 0, 5))),
             H.join(H.strip(10), H.strip(8, origin=(0, 0, 5), scale=0.01))]
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0, 1], [0.5, -0.1, -0.1]], dtype=np.float32)
    cases.append((v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])))                  # a fin
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.05, 0], [0.5, 1, 1], [0.5, -1, 1], [1, 1, -1], [1, -1, -1]], dtype=np.float32)
    cases.append((v, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4], [1, 2, 5], [2, 1, 6]])))   # two fins, a shared candidate
    v = np.array([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0], [0, 1, 1], [0, -1, 1]], dtype=np.float32)
    cases.append((v, np.array([[0, 1, 2], [0, 3, 4], [0, 5, 6]])))                  # three fans
    v = np.array([[0, 0, 0], [0.6, 0, 0], [1.2, 0, 0], [0, 8, 0], [0, 0, 6]], dtype=np.float32)
    cases.append((v, np.array([[0, 1, 3], [1, 2, 4], [0, 3, 4]])))                  # the merge chain
    for v, f in cases:
        for kw in (dict(v_pct=0, min_f=0, min_d=0), dict(v_pct=100.0 / MC.diag(v[np.unique(f)]), min_f=0, min_d=0),
                   dict(v_pct=1, min_f=8, min_d=5)):
            _check(mesh, v, f, **kw)


def test_deterministic_empty_and_call_shapes(mesh):
    vol = np.random.default_rng(9).standard_normal((24, 24, 24)).astype(np.float32)
    v, _, f = mc_numpy.marching_cubes(vol, 0.2)
    a = _gpu_clean(mesh, v, f, **KW)
    b = _gpu_clean(mesh, v, f, **KW)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    vn, fn, vmap = mesh.clean_mesh(v, f, return_vmap=True, **KW)                   # numpy in, numpy out
    assert vn.dtype == np.float64 and fn.dtype == np.int64 and vmap.dtype == np.int64
    assert np.array_equal(vn, a[0].astype(np.float64)) and np.array_equal(fn, a[1]) and np.array_equal(vmap, a[2])
    vn, fn = mesh.clean_mesh(v, f, **KW)
    assert np.array_equal(fn, a[1])
    # empty input; every face removed
    vo, fo, vmap = _gpu_clean(mesh, np.zeros((0, 3)), np.zeros((0, 3)), **KW)
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and vmap.shape == (0,)
    vo, fo, vmap = _gpu_clean(mesh, v, f, v_pct=1, min_f=10 ** 6, min_d=5)
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and vmap.shape == (0,)
    vo, fo, vmap = _gpu_clean(mesh, np.ones((5, 3)), np.array([[0, 1, 2], [2, 3, 4]]), **KW)   # all merged into one point
    assert vo.shape == (0, 3) and fo.shape == (0, 3)
    with pytest.raises(ValueError):
        _gpu_clean(mesh, v, np.array([[0, 1, len(v)]]))


def test_extract_mesh_and_texmesh_wiring(mesh):
    field = _synthetic_field()
    R, S = 48, 256
    raw = mesh.extract_mesh(field, R, filter_noise=False)
    exp = mesh.clean_trimesh(raw, **KW)
    got = mesh.extract_mesh(field, R, filter_noise=False, clean=True)
    for k in ("v", "f", "normals", "albedo", "roughness", "metallic"):
        assert torch.equal(getattr(got, k), getattr(exp, k)), k
    assert got.f.shape[0] < raw.f.shape[0]
    vo, fo, vmap = mesh.clean_mesh(raw.v, raw.f, return_vmap=True, **KW)
    assert torch.equal(exp.v, vo) and torch.equal(exp.albedo, raw.albedo[vmap])
    # the default keeps the raw mesh
    again = mesh.extract_mesh(field, R, filter_noise=False)
    assert torch.equal(again.f, raw.f) and torch.equal(again.v, raw.v)
    tm = mesh.extract_texmesh(field, R, S, filter_noise=False, clean=True)
    ref = mesh.bake_textures(field, exp, S)
    for k in ("v", "f", "normals", "vt", "vmap", "albedo", "metallic_roughness", "covered"):
        assert torch.equal(getattr(tm, k), getattr(ref, k)), k


def _floaters(n=48, k=300, seed=7):
    """A sphere of radius n / 4 and up to k balls of radius 0.7-1 lattice units around it, in index units."""
    x = np.arange(n, dtype=np.float64)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    c = (n - 1) / 2 + 0.137
    d = np.sqrt((X - c) ** 2 + (Y - c) ** 2 + (Z - c) ** 2) - 0.25 * n
    rng = np.random.default_rng(seed)
    for _ in range(k):
        p = rng.uniform(2, n - 3, 3)
        if np.linalg.norm(p - c) < 0.25 * n + 3:
            continue
        d = np.minimum(d, np.sqrt((X - p[0]) ** 2 + (Y - p[1]) ** 2 + (Z - p[2]) ** 2) - rng.uniform(0.7, 1.0))
    return d.astype(np.float32)


def test_cleaned_mesh_bakes_where_the_raw_one_cannot(mesh):
    """1324 charts (restatement: texbake_numpy.charts) cannot fit 128^2 (at most 25 x 25 rectangles of 5 texels); after
    the cleanup 12 charts remain and the atlas packs."""
    from tests import texbake_numpy as T
    vol = torch.from_numpy(_floaters()).to(DEV)
    v, f, n = mesh.marching_cubes(vol, 0.0, return_normals=True)
    assert T.charts(v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy())[2] > 25 * 25
    with pytest.raises(ValueError, match="charts do not fit"):
        mesh.uv_unwrap(v, f, n, (128, 128))
    vo, fo, vmap = mesh.clean_mesh(v, f, return_vmap=True, **KW)
    assert T.charts(vo.cpu().numpy(), fo.cpu().numpy(), n[vmap].cpu().numpy())[2] < 50
    atlas = mesh.uv_unwrap(vo, fo, n[vmap], (128, 128))
    assert atlas.doubly == 0 and atlas.n_covered > 0
