"""The workspace sizes of the mesh export path, pinned without a GPU: the five workspace queries return, byte for byte, what
tests/golden/mesh_workspace.json recorded (tests/golden/make_golden_mesh_workspace.py) - the footprint tests prove that a
stage stays inside the workspace it asked for, this one that the workspace itself did not move - and the sizes the
*_cpu.py tests of the mesh modules see refused are still refused, with the same words."""
import ctypes as C
import json

import pytest

from tests.golden import make_golden_mesh_workspace as G


@pytest.fixture(scope="module")
def h():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd._lib as L
    return L.load()


@pytest.fixture(scope="module")
def recorded():
    with open(G.OUT) as f:
        return json.load(f)


def test_golden_file_covers_the_grid(recorded):
    cases = G.cases()
    assert set(recorded) == set(cases)
    for name, rows in cases.items():
        assert [tuple(r[:-1]) for r in recorded[name]] == rows, name
        assert all(r[-1] > 0 and r[-1] % 256 == 0 for r in recorded[name]), name


@pytest.mark.parametrize("name", sorted(G.cases()))
def test_workspace_bytes_equal_the_recorded_ones(h, recorded, name):
    assert G.measure(h)[name] == recorded[name]


def test_rejected_sizes_stay_rejected(h):
    for name, args, words in G.REJECTED:
        b = C.c_int64(-7)
        assert getattr(h, name)(*args, C.byref(b)) == -1, (name, args)
        assert words in h.primx_last_error(), (name, args, h.primx_last_error())
        assert b.value == -7, (name, args)
    for name, rows in G.cases().items():
        assert getattr(h, name)(*rows[0], None) == -1 and b"null" in h.primx_last_error(), name
