"""The compactions of the mesh export path at the block edges (csrc/mesh_common.h and the kernels of mcubes.hip,
meshclean.hip, meshdecim.hip and texbake.hip that count, scan and place on it), against the numpy restatements and with
the comparisons of the small-size tests, whose helpers this module calls.  Every scan of the path covers blocks of
PTS = 1024 items by 256 threads in 4 rounds, sums the blocks in one workgroup and places by block offset + prefix; the
item counts at which that can go wrong are one less / exactly / one more than 256 (a wave short of, at and past a round),
than 1024 (a block) and a ragged third block (2049).  The small-size tests reach them only by accident; here the face,
lattice-point and texel counts are those numbers.  More than one block sum per scan thread needs more than 2^20 items:
tests/test_hip_mesh_scale.py.

Restatement times at 2049 faces when the module was written (seconds, one thread): cleanup 0.03, decimation 0.02."""
import types

import numpy as np
import pytest
import torch

from tests import mc_numpy
from tests import test_hip_mesh as TM
from tests import test_hip_meshclean as TC
from tests import test_hip_meshdecim as TD
from tests import test_hip_texbake as TT
from tests import texbake_numpy as T
from tests.test_hip_mesh_scale import ellipsoid
from tests.test_meshclean_cpu import tetra

pytestmark = pytest.mark.gpu
FACES = [1, 255, 256, 257, 1023, 1024, 1025, 2049]
EXTRA = 10                                               # faces of `dirty` that are not the patch's


@pytest.fixture(scope="module")
def mesh():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import mesh as M
    return M


def patch(F):
    """A triangulated grid patch over a gentle height field with exactly F faces: cells row by row, two triangles each,
    the last triangle dropped where F is odd (the vertices of an unfinished last row stay, unreferenced)."""
    cells = (F + 1) // 2
    nx = int(np.ceil(np.sqrt(cells)))
    rows = -(-cells // nx)
    I, J = np.meshgrid(np.arange(rows + 1), np.arange(nx + 1), indexing="ij")
    x, y = I.reshape(-1).astype(np.float64), J.reshape(-1).astype(np.float64)
    v = np.stack([x, y, 0.35 * np.sin(0.9 * x + 0.3) * np.cos(0.7 * y)], 1).astype(np.float32)
    c = np.arange(cells)
    a = (c // nx) * (nx + 1) + c % nx
    b, d, e = a + (nx + 1), a + (nx + 1) + 1, a + 1
    f = np.stack([np.stack([a, b, d], 1), np.stack([a, d, e], 1)], 1).reshape(-1, 3)[:F]
    return v, f.astype(np.int64)


def dirty(F):
    """Exactly F faces with mixed keep / drop / rank flags: the patch of F - 10 faces, three of its faces again (one of
    them rotated), three zero-area faces (two that repeat an index, one on three collinear new vertices) and a detached
    tetrahedron above the patch, spread evenly through the face list.  F = 1 is the bare triangle."""
    if F <= EXTRA:
        return patch(F)
    v, f = patch(F - EXTRA)
    n, k = len(v), len(f)
    tv, tf = tetra()
    line = np.array([[0.25, 0.25, 2.0], [0.5, 0.5, 2.0], [1.0, 1.0, 2.0]], dtype=np.float32)
    centre = np.array([v[:, 0].mean(), v[:, 1].mean(), 3.0], dtype=np.float32)
    v = np.concatenate([v, line, tv + centre])
    extra = np.concatenate([f[[0, k // 2]], np.roll(f[[k - 1]], 1, 1),
                            [[f[1, 0], f[1, 0], f[1, 1]], [f[k // 3, 0], f[k // 3, 1], f[k // 3, 1]], [n, n + 1, n + 2]],
                            tf + n + 3])
    assert len(extra) == EXTRA
    f = np.insert(f, np.linspace(0, k, EXTRA).astype(np.int64), extra, axis=0)
    assert len(f) == F
    return v, f


@pytest.mark.parametrize("F", FACES)
def test_face_components(mesh, F):
    v, f = dirty(F)
    comp, nc = mesh.face_components(TT._dev(f, torch.int32), len(v))
    rcomp, rnc = T.components(f)
    assert nc == rnc and (F <= EXTRA or nc >= 3), (nc, rnc)      # the patch, the collinear face, the tetrahedron
    np.testing.assert_array_equal(comp.cpu().numpy(), rcomp)


@pytest.mark.parametrize("kw", [TC.KW, dict(v_pct=0, min_f=0, min_d=0)], ids=["shipped", "keep_all"])
@pytest.mark.parametrize("F", FACES)
def test_cleanup(mesh, F, kw):
    v, f = dirty(F)
    (vo, fo, vmap), st = TC._check(mesh, v, f, **kw)
    if F > EXTRA:
        assert 0 < len(fo) < F and 0 < len(vo) < len(v)           # kept and dropped faces and vertices: mixed flags
        assert st["components_removed"] >= (1 if kw["min_f"] else 0)     # the tetrahedron


@pytest.mark.parametrize("F", FACES)
def test_decimation(mesh, F):
    v, f = patch(F)
    assert len(f) == F
    target = 3 * F // 4
    (vo, fo, _), st = TD._check(mesh, v, f, target)
    if F > 1:
        assert st["rounds"] >= 1 and len(fo) < F


@pytest.mark.parametrize("shape", [(2, 2, 2), (7, 9, 16), (8, 8, 16), (8, 8, 17), (9, 16, 15)])
def test_marching_cubes(mesh, shape):
    """8, 1008, 1024, 1088 and 2160 lattice points."""
    vol = ellipsoid(shape)
    v, n, f = TM._mc(mesh, vol)
    rv, rn, rf = mc_numpy.marching_cubes(vol)
    assert v.shape == rv.shape and f.shape == rf.shape and len(f) > 0
    np.testing.assert_allclose(v, rv, rtol=0, atol=1e-6)
    np.testing.assert_allclose(n, rn, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(f, rf)


@pytest.mark.parametrize("size", [(31, 33), (32, 32), (25, 41)])
def test_atlas_raster_and_points(mesh, size):
    """1023, 1024 and 1025 texels under overlapping random triangles: the face-id map, the cover counts, the two totals
    of the scan, and the covered texels with their points in raster order."""
    W, H = size
    rng = np.random.default_rng(W * H)
    uv = rng.integers(-300, (max(W, H) + 6) * 256, size=(120, 2)).astype(np.int32)
    ft = rng.integers(0, 120, size=(60, 3)).astype(np.int32)
    ft[:5] = [[0, 1, 2], [2, 1, 0], [3, 3, 4], [5, 6, 7], [7, 6, 5]]
    v = rng.random((120, 3)).astype(np.float32)
    uvd, ftd = TT._dev(uv, torch.int32), TT._dev(ft, torch.int32)
    fid, cover, covered, doubly, ws = mesh.atlas_raster(uvd, ftd, W, H)
    rfid, rcnt = T.raster(uv, ft, W, H)
    np.testing.assert_array_equal(fid.cpu().numpy(), rfid)
    np.testing.assert_array_equal(cover.cpu().numpy(), rcnt)
    assert covered == int((rcnt > 0).sum()) and doubly == int((rcnt > 1).sum())
    assert 0 < doubly < covered < W * H                              # covered, doubly covered and empty texels
    atlas = types.SimpleNamespace(size=(W, H), n_covered=covered, face_id=fid, _raster_ws=ws, uv_fixed=uvd, f=ftd)
    texel, pts = mesh.atlas_points(atlas, TT._dev(v), ftd)
    rt, rp = T.points(rfid, uv, ft, v, ft)
    np.testing.assert_array_equal(texel.cpu().numpy(), rt)
    np.testing.assert_allclose(pts.cpu().numpy(), rp, rtol=0, atol=1e-6)
