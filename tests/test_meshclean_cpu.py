"""Mesh cleanup without a GPU: the numpy restatement of rules R0-R8 (tests/meshclean_numpy.py) on hand-built meshes with
known answers, its round schedule against its sequential statement, and the host-side argument checks of the cleanup
entry points (csrc/meshclean.hip) and of mesh.clean_mesh."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mc_numpy
from tests import meshclean_numpy as MC


def strip(n, origin=(0.0, 0.0, 0.0), scale=1.0, base=0):
    """An edge-connected strip of n triangles in the z = const plane: (vertices, faces indexed from `base`)."""
    m = n // 2 + 2
    v = [(i, 0, 0) for i in range(m)] + [(i, 1, 0) for i in range(m)]
    v = np.asarray(v, dtype=np.float32) * scale + np.asarray(origin, dtype=np.float32)
    f = []
    for i in range(m - 1):
        f += [(i, i + 1, m + i), (i + 1, m + i + 1, m + i)]
    return v, np.asarray(f[:n], dtype=np.int64) + base


def join(*parts):
    vs, fs, off = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(f - f.min() + off if len(f) else f)
        off += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def tetra():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
    return v, f


NO_FILTER = dict(min_f=0, min_d=0)


def test_chain_merge_keeps_the_far_end_a_centre():
    # a - b - c on the x axis, 0.6 apart, r = 1: a captures b, c (1.2 from a) stays a centre even though b is within r
    v = np.array([[0, 0, 0], [0.6, 0, 0], [1.2, 0, 0], [0, 8, 0], [0, 0, 6]], dtype=np.float32)
    f = np.array([[0, 1, 3], [1, 2, 4], [0, 3, 4]], dtype=np.int64)
    D = MC.diag(v)
    v_pct = 100.0 / D
    assert abs(float(MC.radius(v, f, v_pct)) - 1.0) < 1e-6
    centre = MC.merge(v, f, v_pct)
    np.testing.assert_array_equal(centre, [0, 0, 2, 3, 4])
    c2, rounds = MC.merge_rounds(v, f, v_pct)
    np.testing.assert_array_equal(c2, centre)
    assert rounds >= 2
    vo, fo, vmap = MC.clean(v, f, v_pct, repair=False, **NO_FILTER)
    np.testing.assert_array_equal(vmap, [0, 2, 3, 4])                   # b is gone, the face (a, a, p) dropped
    np.testing.assert_array_equal(fo, [[0, 1, 3], [0, 2, 3]])
    np.testing.assert_array_equal(vo, v[vmap])


def test_equal_positions_merge_at_any_radius():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 0, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64)
    centre = MC.merge(v, f, 1e-6)
    np.testing.assert_array_equal(centre, [0, 1, 2, 1])
    vo, fo, vmap = MC.clean(v, f, 1e-6, repair=False, **NO_FILTER)
    np.testing.assert_array_equal(fo, [[0, 1, 2]])                      # face 1 became a reversed duplicate of face 0


def test_duplicate_face_with_reversed_winding():
    v, f = tetra()
    f = np.concatenate([f, f[2:3, ::-1]])
    vo, fo, vmap = MC.clean(v, f, 0, repair=False, **NO_FILTER)
    np.testing.assert_array_equal(fo, tetra()[1])


def test_collinear_face_is_dropped():
    v, f = tetra()
    v = np.concatenate([v, [[2, 0, 0]]]).astype(np.float32)
    f = np.concatenate([f, [[0, 1, 4]]])                                  # (0,0,0), (1,0,0), (2,0,0)
    vo, fo, vmap = MC.clean(v, f, 0, repair=False, **NO_FILTER)
    np.testing.assert_array_equal(fo, tetra()[1])
    np.testing.assert_array_equal(vmap, [0, 1, 2, 3])


def test_component_face_count():
    v, f = join(strip(7), strip(8, origin=(0, 0, 5)))
    _, fo, vmap = MC.clean(v, f, 0, min_f=8, min_d=0, repair=False)
    assert len(fo) == 8 and vmap.min() >= len(strip(7)[0])               # the 7-face strip goes, the 8-face one stays
    _, fo, _ = MC.clean(v, f, 0, min_f=7, min_d=0, repair=False)
    assert len(fo) == 15


def test_component_diameter():
    v, f = join(strip(10), strip(8, origin=(0, 0, 5), scale=0.01))
    st = {}
    _, fo, vmap = MC.clean(v, f, 0, min_f=0, min_d=5, repair=False, stats=st)
    assert len(fo) == 10 and vmap.max() < len(strip(10)[0]) and st["components_removed"] == 1
    _, fo, _ = MC.clean(v, f, 0, min_f=0, min_d=0, repair=False)
    assert len(fo) == 18


def test_fin_drops_the_smallest_face():
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0, 1], [0.5, -0.1, -0.1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int64)
    st = {}
    _, fo, vmap = MC.clean(v, f, 0, repair=True, stats=st, **NO_FILTER)
    np.testing.assert_array_equal(fo, [[0, 1, 2], [1, 0, 3]])
    assert st["nonmanifold_candidates"] == 3 and st["nonmanifold_faces_removed"] == 1
    np.testing.assert_array_equal(vmap, [0, 1, 2, 3])


def test_two_fins_share_a_candidate():
    # face 0 sits on both non-manifold edges (0, 1) and (1, 2) and is the smallest: dropping it repairs both
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.05, 0], [0.5, 1, 1], [0.5, -1, 1], [1, 1, -1], [1, -1, -1]],
                 dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4], [1, 2, 5], [2, 1, 6]], dtype=np.int64)
    st = {}
    _, fo, vmap = MC.clean(v, f, 0, repair=True, stats=st, **NO_FILTER)
    assert st["nonmanifold_candidates"] == 5 and st["nonmanifold_faces_removed"] == 1
    # vertex 1 is left with two fans, {1, 2} and {3, 4}: the first one's moves to the new vertex 7
    np.testing.assert_array_equal(vmap, [0, 1, 2, 3, 4, 5, 6, 1])
    np.testing.assert_array_equal(fo, [[0, 7, 3], [7, 0, 4], [1, 2, 5], [2, 1, 6]])
    # the same fins with face 0 the largest: the smaller faces go first, one per edge, and face 0 stays
    v[2] = [0.5, 3, 3]
    _, fo, _ = MC.clean(v, f, 0, repair=True, **NO_FILTER)
    assert len(fo) == 3 and (fo == f[0]).all(1).any()
    MC.check_invariants(*MC.clean(v, f, 0, repair=True, **NO_FILTER)[:2])


def test_bowtie_vertex_is_split_once():
    v = np.array([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0]], dtype=np.float32)
    f = np.array([[0, 3, 4], [0, 1, 2]], dtype=np.int64)
    st = {}
    vo, fo, vmap = MC.clean(v, f, 0, repair=True, stats=st, **NO_FILTER)
    np.testing.assert_array_equal(vmap, [0, 1, 2, 3, 4, 0])              # one new vertex, at vertex 0's position
    np.testing.assert_array_equal(fo, [[5, 3, 4], [0, 1, 2]])           # it carries face 0's fan (the lowest index)
    np.testing.assert_array_equal(vo, v[vmap])
    assert st["vertices_split"] == 1


def test_three_fans_split_once():
    v = np.array([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0], [0, 1, 1], [0, -1, 1]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 3, 4], [0, 5, 6]], dtype=np.int64)
    vo, fo, vmap = MC.clean(v, f, 0, repair=True, **NO_FILTER)
    np.testing.assert_array_equal(vmap, [0, 1, 2, 3, 4, 5, 6, 0])
    np.testing.assert_array_equal(fo, [[7, 1, 2], [0, 3, 4], [0, 5, 6]])   # vertex 0 keeps two fans


def test_v_pct_zero_and_clean_input_unchanged():
    v, f = tetra()
    v = np.concatenate([v, [[9, 9, 9]]]).astype(np.float32)               # an unreferenced vertex goes
    vo, fo, vmap = MC.clean(v, f, 0, repair=True, **NO_FILTER)
    np.testing.assert_array_equal(fo, f)
    np.testing.assert_array_equal(vmap, [0, 1, 2, 3])
    assert np.array_equal(MC.merge(v, f, 0), [0, 1, 2, 3, -1])
    vo, fo, vmap = MC.clean(np.zeros((0, 3)), np.zeros((0, 3)), 1.0)
    assert vo.shape == (0, 3) and fo.shape == (0, 3) and vmap.shape == (0,)


@pytest.mark.parametrize("v_pct", [0.5, 1.0, 3.0])
def test_round_schedule_matches_the_sequential_rule(v_pct):
    for name, (vol, *_ ) in mc_numpy.analytic_fields(40).items():
        v, _, f = mc_numpy.marching_cubes(vol)
        c1 = MC.merge(v, f, v_pct)
        c2, rounds = MC.merge_rounds(v, f, v_pct)
        np.testing.assert_array_equal(c1, c2, err_msg=name)
        assert 0 < rounds < 200, (name, rounds)
    vol = np.random.default_rng(5).standard_normal((20, 20, 20)).astype(np.float32)
    v, _, f = mc_numpy.marching_cubes(vol, 0.2)
    np.testing.assert_array_equal(MC.merge(v, f, v_pct), MC.merge_rounds(v, f, v_pct)[0])


def test_invariants_on_a_noise_mesh():
    vol = np.random.default_rng(2).standard_normal((16, 16, 16)).astype(np.float32)
    v, _, f = mc_numpy.marching_cubes(vol, 0.2)
    st = {}
    vo, fo, vmap = MC.clean(v, f, 1.0, min_f=8, min_d=5, repair=True, stats=st)
    MC.check_invariants(vo, fo)
    assert st["components_removed"] > 0 and st["nonmanifold_candidates"] > 0
    vo, fo, _ = MC.clean(v, f, 1.0, min_f=8, min_d=5, repair=False)
    MC.check_invariants(vo, fo, min_f=8, repaired=False)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd._lib as L
    return L


def test_meshclean_entry_points_reject_bad_arguments_without_gpu(lib):
    """Checks run on the host before any launch: PRIMX_EINVAL (-1) + a message."""
    h = lib.load()
    err = lambda: h.primx_last_error()   # noqa: E731
    ws = C.c_int64(0)
    assert h.primx_meshclean_workspace(100, 200, C.byref(ws)) == 0 and ws.value >= 8 * 4 * 600
    assert h.primx_meshclean_workspace(100, 200, None) == -1 and b"null" in err()
    assert h.primx_meshclean_workspace(-1, 200, C.byref(ws)) == -1 and b">= 0" in err()
    assert h.primx_meshclean_workspace(100, 1 << 29, C.byref(ws)) == -1 and b"2^31" in err()
    rounds, r = C.c_int64(7), C.c_float(1)
    assert h.primx_meshclean_merge(None, None, 0, 0, 1.0, None, 0, None, C.byref(rounds), C.byref(r), None) == 0
    assert rounds.value == 0 and r.value == 0.0                                       # nothing to do
    assert h.primx_meshclean_merge(1, 1, 4, 2, -1.0, 1, 1 << 40, 1, C.byref(rounds), C.byref(r), None) == -1
    assert b"v_pct" in err()
    assert h.primx_meshclean_merge(1, 1, 4, 2, 1.0, 1, 1 << 40, 1, None, C.byref(r), None) == -1 and b"null" in err()
    assert h.primx_meshclean_merge(None, 1, 4, 2, 1.0, 1, 1 << 40, 1, C.byref(rounds), C.byref(r), None) == -1
    assert h.primx_meshclean_merge(1, 1, 4, 2, 1.0, 1, 16, 1, C.byref(rounds), C.byref(r), None) == -1
    assert b"workspace" in err()
    n = C.c_int64(5)
    assert h.primx_meshclean_faces(None, None, None, 0, 0, None, 0, None, C.byref(n), None) == 0 and n.value == 0
    assert h.primx_meshclean_faces(1, None, 1, 4, 2, 1, 1 << 40, 1, C.byref(n), None) == -1 and b"null" in err()
    assert h.primx_meshclean_faces(1, 1, 1, 0, 2, 1, 1 << 40, 1, C.byref(n), None) == -1 and b"V = 0" in err()
    assert h.primx_meshclean_faces(1, 1, 1, 4, 2, 1, 16, 1, C.byref(n), None) == -1 and b"workspace" in err()
    cnt = (C.c_int64 * 3)()
    assert h.primx_meshclean_components(1, 1, 1, 1, 4, 2, 6, 3, 8, 5.0, 1, 1, 1 << 40, 1, 1, 1, cnt, None) == -1
    assert b"n_comp" in err()
    assert h.primx_meshclean_components(1, 1, 1, 1, 4, 2, 6, 1, -1, 5.0, 1, 1, 1 << 40, 1, 1, 1, cnt, None) == -1
    assert b"min_f" in err()
    assert h.primx_meshclean_components(1, 1, 1, 1, 4, 2, 6, 1, 8, 5.0, 1, 1, 1 << 40, 1, 1, 1, None, None) == -1
    assert h.primx_meshclean_edges(1, 1, 2, 6, 1, 3, 1, 1 << 40, 1, C.byref(n), None) == -1 and b"n_cand" in err()
    assert h.primx_meshclean_edges(1, 1, 2, 7, 1, 1, 1, 1 << 40, 1, C.byref(n), None) == -1
    cnt2 = (C.c_int64 * 2)()
    assert h.primx_meshclean_fans(1, 1, 4, 2, 7, 1, 1 << 40, 1, 1, cnt2, None) == -1 and b"n_fans" in err()
    assert h.primx_meshclean_fans(1, None, 4, 2, 0, 1, 16, 1, 1, cnt2, None) == -1 and b"workspace" in err()


def test_clean_mesh_has_no_cpu_path(lib):
    from topia_xl_amd import mesh as M
    v, f = tetra()
    with pytest.raises(RuntimeError, match="no CPU path"):
        M.clean_mesh(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(NotImplementedError):
        M.clean_mesh(torch.from_numpy(v), torch.from_numpy(f), remesh=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            M.clean_mesh(v, f)
    assert M.CLEAN_ARGS == dict(v_pct=1.0, min_f=8, min_d=5, repair=True)
