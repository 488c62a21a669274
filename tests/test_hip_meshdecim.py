"""Mesh decimation on the MI355X (csrc/meshdecim.hip, mesh.decimate_mesh): the quadric and cost stages and the whole
decimation bit for bit against the numpy restatement of rules D0-D10 (tests/meshdecim_numpy.py) on marching-cubes and
hand-built meshes, the invariants of every output, a non-manifold input that stalls, edge cases and call shapes, the
wiring into extract_mesh / extract_texmesh, and one end-to-end textured export."""
import json
import struct

import numpy as np
import pytest
import torch

from tests import mc_numpy
from tests import meshdecim_numpy as D
from tests import test_meshdecim_cpu as H
from tests.test_hip_mesh import _synthetic_field

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mesh():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import mesh as M
    return M


def _dev(v, f):
    vd = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)).to(DEV)
    fd = torch.from_numpy(np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3)).to(DEV)
    return vd, fd


def _gpu(M, v, f, target, stats=None, **kw):
    vo, fo, vmap = M.decimate_mesh(*_dev(v, f), target, return_vmap=True, stats=stats, **kw)
    assert vo.dtype == torch.float32 and fo.dtype == torch.int32 and vmap.dtype == torch.int64 and vo.is_cuda
    return vo.cpu().numpy(), fo.cpu().numpy().astype(np.int64), vmap.cpu().numpy()


def _check(M, v, f, target, manifold=True, invariants=True, **kw):
    st, ref_st = {}, {}
    got = _gpu(M, v, f, target, stats=st, **kw)
    ref = D.decimate(v, f, target, stats=ref_st, **kw)
    print(f"F {len(f)} -> {len(got[1])} (restatement {len(ref[1])}), target {target}, {kw}: {st}")
    for a, b, name in zip(got, ref, ("v", "f", "vmap")):
        assert a.shape == b.shape and np.array_equal(a, b), (name, target, kw, a.shape, b.shape)
    assert st == ref_st, (st, ref_st)
    if invariants:
        D.check_invariants(got[0], got[1], f if manifold else None)
    return got, st


def _fields64():
    for name, (vol, *_) in mc_numpy.analytic_fields(64).items():
        v, _, f = mc_numpy.marching_cubes(vol)
        yield name, v, f


def test_quadrics_and_costs_bit_exact(mesh):
    """The two float64 stages on their own: a one-bit difference in a cost would cascade through every later round."""
    for name, v, f in _fields64():
        for optimal in (True, False):
            tr, ref = {}, {}
            mesh._decimate_dev(*_dev(v, f), len(f) // 4, optimal, None, tr)
            D.decimate(v, f, len(f) // 4, optimal, trace=ref)
            assert np.array_equal(tr["p0"].cpu().numpy(), ref["p0"]), name
            assert np.array_equal(tr["Q0"].cpu().numpy(), ref["Q0"]), name
            g, r = tr["rounds"][0], ref["rounds"][0]
            for k in ("ukeys", "ecnt", "x", "cost", "key"):
                assert np.array_equal(g[k].cpu().numpy(), r[k]), (name, k)
            assert np.array_equal(g["valid"].cpu().numpy() != 0, r["valid"]), name
            assert len(tr["rounds"]) == len(ref["rounds"])
            for g, r in zip(tr["rounds"], ref["rounds"]):                        # every round's selection too
                for k in ("cand", "ok", "sel"):
                    assert np.array_equal(g[k].cpu().numpy().astype(np.int64), r[k].astype(np.int64)), (name, k)


@pytest.mark.parametrize("optimal", [True, False])
def test_analytic_fields_bit_exact(mesh, optimal):
    for name, v, f in _fields64():
        for div in (4, 50):
            target = len(f) // div
            (vo, fo, _), st = _check(mesh, v, f, target, optimalplacement=optimal)
            assert not st["stalled"] and len(fo) in (target, target - 1), (name, div, len(fo))


@pytest.mark.parametrize("optimal", [True, False])
def test_open_sphere_bit_exact(mesh, optimal):
    v, f = H.open_sphere(64)
    for div in (4, 50):
        (vo, fo, _), st = _check(mesh, v, f, len(f) // div, optimalplacement=optimal)
        assert D.topology(fo)[2] == 1


def test_synthetic_field_bit_exact(mesh):
    m = mesh.extract_mesh(_synthetic_field(), resolution=64, filter_noise=False)
    v, f = m.v.cpu().numpy(), m.f.cpu().numpy().astype(np.int64)
    for div in (4, 50):
        for optimal in (True, False):
            _check(mesh, v, f, len(f) // div, optimalplacement=optimal)


def test_hand_built_meshes_bit_exact(mesh):
    for (v, f), target, manifold in H.hand_built():
        for optimal in (True, False):
            _check(mesh, v, f, target, manifold=manifold, optimalplacement=optimal)


def test_noise_mesh_stalls_bit_exact(mesh):
    """The 24^3 noise mesh of the cleanup tests is not manifold (236 edges with more than two faces, 3 027 with one, and
    118 faces that occur twice): locked vertices leave too few valid edges, and the restatement stalls after 22 rounds
    at 20 027 faces for a target of 19 625.  The input's duplicate faces rule out `check_invariants`; neither they nor
    the edges with more than two faces may grow in number."""
    vol = np.random.default_rng(4).standard_normal((24, 24, 24)).astype(np.float32)
    v, _, f = mc_numpy.marching_cubes(vol, 0.2)
    over = lambda ff: int((D.edge_table(D.live_faces(ff), int(np.max(ff)) + 1)[2] > 2).sum())   # noqa: E731
    dup = lambda ff: len(ff) - len(np.unique(np.sort(ff, 1), axis=0))                            # noqa: E731
    (vo, fo, _), st = _check(mesh, v, f, len(f) // 2, manifold=False, invariants=False)
    assert st["stalled"] and len(fo) > len(f) // 2
    assert over(fo) <= over(f) and dup(fo) <= dup(f)
    assert np.array_equal(np.unique(fo), np.arange(len(vo))) and len(D.live_faces(fo)) == len(fo)


def test_identity_empty_call_shapes_and_errors(mesh):
    v, f = next(iter(_fields64()))[1:]
    for target in (len(f), len(f) + 7):
        st = {}
        vo, fo, vmap = _gpu(mesh, v, f, target, stats=st)
        assert np.array_equal(vo, v.astype(np.float32)) and np.array_equal(fo, f) and np.array_equal(vmap, np.arange(len(v)))
        assert st["rounds"] == 0 and not st["stalled"] and st["faces_after"] == len(f)
    vo, fo, vmap = _gpu(mesh, np.zeros((0, 3)), np.zeros((0, 3)), 10)
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and vmap.shape == (0,)
    a, b = _gpu(mesh, v, f, len(f) // 4), _gpu(mesh, v, f, len(f) // 4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    vn, fn, vm = mesh.decimate_mesh(v, f, len(f) // 4, return_vmap=True)            # numpy in, numpy out
    assert vn.dtype == np.float64 and fn.dtype == np.int64 and vm.dtype == np.int64
    assert np.array_equal(vn, a[0].astype(np.float64)) and np.array_equal(fn, a[1]) and np.array_equal(vm, a[2])
    assert len(mesh.decimate_mesh(v, f, len(f) // 4)) == 2
    with pytest.raises(ValueError):
        _gpu(mesh, v, np.array([[0, 1, len(v)]]), 1)
    with pytest.raises(ValueError):
        _gpu(mesh, v, f, -1)
    with pytest.raises(NotImplementedError):
        mesh.decimate_mesh(*_dev(v, f), 10, remesh=True)


def test_vertex_normals(mesh):
    v, nrm, f = mc_numpy.marching_cubes(mc_numpy.analytic_fields(32)["sphere"][0])
    got = mesh.vertex_normals(*_dev(v, f)).cpu().numpy()
    p = v.astype(np.float64)
    g = D.face_g(p[f[:, 0]], p[f[:, 1]], p[f[:, 2]])
    s = np.zeros_like(p)
    for k in range(3):
        np.add.at(s, f[:, k], g)
    ref = s / np.linalg.norm(s, axis=1, keepdims=True)
    assert np.abs(got - ref).max() < 1e-6
    assert ((got * nrm).sum(1) > 0.9).all()                                        # the side of the lattice gradient


def test_extract_mesh_and_texmesh_wiring(mesh):
    field = _synthetic_field()
    R, S = 48, 256
    raw = mesh.extract_mesh(field, R, filter_noise=False)
    N = raw.f.shape[0] // 3
    exp = mesh.decimate_trimesh(raw, N, field)
    got = mesh.extract_mesh(field, R, filter_noise=False, decimate=N)
    for k in ("v", "f", "normals", "albedo", "roughness", "metallic"):
        assert torch.equal(getattr(got, k), getattr(exp, k)), k
    assert got.f.shape[0] <= N < raw.f.shape[0]
    for k in ("albedo", "roughness", "metallic"):
        assert float(getattr(got, k).min()) >= 0.0 and float(getattr(got, k).max()) <= 1.0, k
    gathered = mesh.decimate_trimesh(raw, N)                                        # no field: attributes through vmap
    vo, fo, vmap = mesh.decimate_mesh(raw.v, raw.f, N, return_vmap=True)
    assert torch.equal(gathered.v, vo) and torch.equal(gathered.albedo, raw.albedo[vmap])
    # decimate = 0 and a cap above the face count keep today's mesh
    for again in (mesh.extract_mesh(field, R, filter_noise=False, decimate=0),
                  mesh.extract_mesh(field, R, filter_noise=False, decimate=raw.f.shape[0])):
        for k in ("v", "f", "normals", "albedo", "roughness", "metallic"):
            assert torch.equal(getattr(again, k), getattr(raw, k)), k
    cleaned = mesh.extract_mesh(field, R, filter_noise=False, clean=True)
    N = cleaned.f.shape[0] // 2
    tm = mesh.extract_texmesh(field, R, S, filter_noise=False, clean=True, decimate=N)
    ref = mesh.bake_textures(field, mesh.decimate_trimesh(cleaned, N, field), S)
    for k in ("v", "f", "normals", "vt", "vmap", "albedo", "metallic_roughness", "covered"):
        assert torch.equal(getattr(tm, k), getattr(ref, k)), k
    plain = mesh.extract_texmesh(field, R, S, filter_noise=False, clean=True)
    ref = mesh.bake_textures(field, cleaned, S)
    for k in ("v", "f", "vt", "albedo", "metallic_roughness"):
        assert torch.equal(getattr(plain, k), getattr(ref, k)), k


def test_end_to_end_textured_export(mesh, tmp_path):
    field = _synthetic_field()
    cleaned = mesh.extract_mesh(field, 64, filter_noise=False, clean=True)
    N = cleaned.f.shape[0] // 2
    st = {}
    D.decimate(cleaned.v.cpu().numpy(), cleaned.f.cpu().numpy(), N, stats=st)
    assert not st["stalled"], st                                                   # else the input is badly chosen
    tm = mesh.extract_texmesh(field, 64, 256, filter_noise=False, clean=True, decimate=N)
    F1 = tm.f.shape[0]
    assert 0 < F1 <= N
    dec = mesh.decimate_trimesh(cleaned, N, field)
    atlas = mesh.uv_unwrap(dec.v, dec.f, dec.normals, (256, 256))
    assert atlas.doubly == 0 and atlas.n_covered > 0 and int(tm.covered.sum()) == atlas.n_covered
    path = tmp_path / "decimated.glb"
    tm.write_glb(str(path))
    blob = path.read_bytes()
    magic, version, total = struct.unpack("<III", blob[:12])
    assert magic == 0x46546C67 and version == 2 and total == len(blob)
    n, kind = struct.unpack("<II", blob[12:20])
    assert kind == 0x4E4F534A
    gltf = json.loads(blob[20:20 + n])
    prim = gltf["meshes"][0]["primitives"][0]
    assert gltf["accessors"][prim["indices"]]["count"] == 3 * F1
