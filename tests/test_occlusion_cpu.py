"""tests/occlusion_numpy.py and the ambient occlusion's Python surface without a GPU: the direction table, the restated estimator
on analytic lattices (plane, sphere, two spheres, hollow sphere), the ABI bookkeeping of primx_texbake_occlusion, the GLB writer
with and without `occlusion`, and the closure of the stream-order table once tests/test_hip_occlusion.py has registered its case."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from tests import occlusion_numpy as ON
from tests import test_hip_occlusion as TO
from tests.test_normalmap_cpu import _glb, _tiny_textured_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 65
DTYPES = (np.float64, np.float32)


# ------------------------------------------------------------------------------------------------ 1. the direction table
@pytest.mark.parametrize("K", [1, 2, 16, 64, 256])
def test_direction_table(K):
    """Unit rows, float32, the restatement's table bit for bit, and a mean direction that vanishes: z sums to 0 by the symmetry
    z_k = -z_(K-1-k); the spiral's x, y sum is not exactly 0, but under 1 % of K - opposite normals then see cosine-weighted
    hemispheres whose weights differ by under 1 %."""
    from topia_xl_amd import mesh as M
    d = M.occlusion_directions(K)
    assert isinstance(d, torch.Tensor) and d.dtype == torch.float32 and tuple(d.shape) == (K, 3) and not d.is_cuda
    assert np.array_equal(d.numpy(), ON.directions(K))
    d64 = d.numpy().astype(np.float64)
    assert float(np.abs(np.linalg.norm(d64, axis=1) - 1).max()) <= 1e-7
    s = d64.sum(0)
    print(f"K = {K}: sum of the directions {s.tolist()}")
    assert abs(s[2]) <= 1e-6
    if K == 1:
        assert np.array_equal(d.numpy(), np.array([[1.0, 0.0, 0.0]], dtype=np.float32))    # z = 0, angle 0
    else:
        assert float(np.linalg.norm(s)) <= 0.01 * K or K < 16
    with pytest.raises(ValueError):
        M.occlusion_directions(0)


def test_defaults_are_the_documented_ones():
    import inspect

    from topia_xl_amd import mesh as M
    p = inspect.signature(M.texel_occlusion).parameters
    assert (p["directions"].default, p["steps"].default, p["radius"].default, p["bias"].default, p["isovalue"].default) == \
        (None, 8, 0.25, None, 0.0)
    assert tuple(M.occlusion_directions().shape) == (64, 3)
    for fn in (M.bake_textures, M.extract_texmesh):
        assert inspect.signature(fn).parameters["occlusion"].default is False
    assert inspect.signature(M.fill_textures).parameters["occlusion"].default is None
    q = inspect.signature(M.bake_textures).parameters
    assert (q["lattice"].default, q["occlusion_resolution"].default, q["occlusion_args"].default) == (None, 256, None)
    assert list(inspect.signature(M.field_lattice).parameters) == ["field", "resolution", "chunk"]


# ------------------------------------------------------------------------------------------------ 2. analytic lattices
def test_plane_is_exactly_open():
    rng = np.random.default_rng(0)
    lat = TO.plane_lattice(R)
    p = np.stack([rng.uniform(-0.8, 0.8, 300), rng.uniform(-0.8, 0.8, 300), np.full(300, 0.1)], 1).astype(np.float32)
    n = np.tile(np.float32([0, 0, 1]), (300, 1))
    for dt in DTYPES:
        ao = ON.occlusion(lat, p, n, ON.directions(64), dtype=dt)
        assert ao.dtype == dt and bool((ao == 1.0).all())


def test_sphere_exterior_is_exactly_open():
    u = TO.unit_vectors(500, seed=1)
    lat = TO.sphere_lattice(R, 0.5)
    for dt in DTYPES:
        ao = ON.occlusion(lat, (0.5 * u).astype(np.float32), u.astype(np.float32), ON.directions(64), dtype=dt)
        assert bool((ao == 1.0).all())


def test_two_spheres_darken_towards_the_crease():
    """A meridian of the sphere at x = +0.3 from its far pole (angle 0) to the pole inside the other sphere (angle pi): open on the
    far side, falling monotonically, under 0.2 at the last sample before the crease (cos = -0.3 / 0.35) and 0 inside the other
    sphere."""
    lat = TO.two_spheres_lattice(R)
    th = np.linspace(0.0, np.pi, 41)
    n = np.stack([np.cos(th), np.sin(th), 0 * th], 1)
    p = np.array([0.3, 0.0, 0.0]) + 0.35 * n
    inside = np.linalg.norm(p - np.array([-0.3, 0.0, 0.0]), axis=1) < 0.35
    crease = int(np.nonzero(inside)[0][0]) - 1
    for dt in DTYPES:
        ao = ON.occlusion(lat, p.astype(np.float32), n.astype(np.float32), ON.directions(64), dtype=dt)
        print(f"{np.dtype(dt).name}: {np.round(ao, 3).tolist()}")
        assert bool((ao[:20] == 1.0).all()) and bool((np.diff(ao) <= 0).all())
        assert 0 < ao[crease] < 0.2 and bool((ao[inside] == 0).all())
        assert float(ao.min()) >= 0 and float(ao.max()) <= 1


def test_hollow_sphere_agrees_with_the_exact_distance():
    """The inner wall of a hollow sphere of radius 0.6: occluded everywhere, and the lattice estimator within the lattice's
    interpolation error of the same estimator on the exact distance 0.6 - |x| (measured 3.9e-4 at R = 65; bound 1e-3)."""
    u = TO.unit_vectors(500, seed=2)
    lat = TO.hollow_lattice(R)
    p, n, d = (0.6 * u).astype(np.float32), (-u).astype(np.float32), ON.directions(64)
    ao = ON.occlusion(lat, p, n, d)
    ex = ON.occlusion(lat, p, n, d, exact=lambda x: 0.6 - np.linalg.norm(x, axis=-1))
    err = float(np.abs(ao - ex).max())
    print(f"hollow sphere: ao in [{ao.min():.4f}, {ao.max():.4f}], lattice vs exact distance {err:.3e}")
    assert float(ao.max()) < 1 and float(ao.min()) > 0.9 and err <= 1e-3


def test_zero_normal_and_points_beyond_the_cube():
    lat = TO.two_spheres_lattice(R)
    p = np.float32([[0.0, 0.2, 0.0], [1.5, -2.0, 0.3], [1.0, 1.0, 1.0], [-1.0, 0.0, 0.0]])
    n = np.float32([[0, 0, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 0]])
    for dt in DTYPES:
        ao = ON.occlusion(lat, p, n, ON.directions(64), dtype=dt)
        assert ao[0] == 1.0 and bool(np.isfinite(ao).all()) and float(ao.min()) >= 0 and float(ao.max()) <= 1
    # the clamp: a position beyond the cube reads the value of its projection onto the cube
    assert np.array_equal(ON.phi(lat, np.float32([[1.5, -2.0, 0.3]])), ON.phi(lat, np.float32([[1.0, -1.0, 0.3]])))


def test_quantize_is_the_fills_byte():
    ao = np.float32([0.0, 0.5, 0.999, 1.0, 1.0 / 255, 254.999 / 255])
    assert ON.quantize(ao).tolist() == [0, 127, 254, 255, 1, 254]


# ------------------------------------------------------------------------------------------------ 3. ABI
def test_abi_35_declares_the_entry_point_with_the_bound_signature():
    from topia_xl_amd import _lib
    name = "primx_texbake_occlusion"
    assert _lib.ABI_VERSION == 35 and _lib._SINCE[name] == 35 and name not in _lib._FEATURES.values()
    with open(os.path.join(ROOT, "include", "primx_hip.h")) as fh:
        text = fh.read()
    assert "#define PRIMX_ABI_VERSION 35" in text
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", text)
    assert m, "the header does not declare it"
    ctype = {"const float*": _lib._p, "float*": _lib._p, "void*": _lib._p, "int": _lib._i, "int64_t": _lib._l, "float": _lib._f}
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    names = [a.rsplit(" ", 1)[1] for a in args]
    assert names == ["lattice", "R", "pts", "nrm", "n", "dirs", "K", "steps", "radius", "bias", "isovalue", "occ", "stream"]
    assert [ctype[a.rsplit(" ", 1)[0]] for a in args] == _lib.SIGNATURES[name]


def test_an_ab_build_of_version_35_from_before_the_occlusion_still_loads(monkeypatch, tmp_path):
    from tests import test_lib_capabilities_cpu as TL
    from topia_xl_amd import _lib
    rest = set(_lib.SIGNATURES) - {"primx_texbake_occlusion"}
    lib = TL.StandIn(35, rest)
    assert TL._load(monkeypatch, tmp_path, lib) == TL.ALL and lib.bound() == rest
    with pytest.raises(AttributeError):                               # ... and as the package's own library it is refused
        TL._load(monkeypatch, tmp_path, lib, ab=False)


def test_stream_table_is_closed_with_the_occlusion_case():
    from tests import test_hip_material, test_hip_normalmap, test_hip_primsdf_grad, test_hip_raymarch_grad  # noqa: F401  (the other registering modules)
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    assert TO.STREAM_CASE in TS.CASES and "primx_texbake_occlusion" in TS.declared()
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n == TO.STREAM_CASE]       # it runs in its own module, not twice


# ------------------------------------------------------------------------------------------------ 4. the GLB
def test_write_glb_with_and_without_occlusion(tmp_path):
    M, tm, tang, nmap = _tiny_textured_mesh()
    assert tm.occlusion is False
    assert [f.name for f in dataclasses.fields(tm)][-3:] == ["occlusion", "tangents", "normal_map"]
    plain, with_ao = str(tmp_path / "plain.glb"), str(tmp_path / "ao.glb")
    tm.write_glb(plain)
    dataclasses.replace(tm, occlusion=True).write_glb(with_ao)
    assert b"occlusionTexture" not in open(plain, "rb").read()
    _, js0, blob0 = _glb(plain)
    _, js1, blob1 = _glb(with_ao)
    assert js1["materials"][0]["occlusionTexture"] == {"index": 1, "strength": 1.0}
    assert list(js1["materials"][0]) == ["name", "pbrMetallicRoughness", "occlusionTexture"]
    del js1["materials"][0]["occlusionTexture"]
    assert js1 == js0 and blob1 == blob0                              # nothing else differs
    # off: the bytes of a TexturedMesh built without the field
    fields = {f.name: getattr(tm, f.name) for f in dataclasses.fields(tm) if f.name != "occlusion"}
    M.TexturedMesh(**fields).write_glb(str(tmp_path / "without.glb"))
    dataclasses.replace(tm, occlusion=False).write_glb(str(tmp_path / "off.glb"))
    assert open(plain, "rb").read() == open(str(tmp_path / "without.glb"), "rb").read() == open(str(tmp_path / "off.glb"), "rb").read()
    # with a normal map as well: both entries, the normal map's file otherwise unchanged
    full = dataclasses.replace(tm, tangents=tang, normal_map=nmap)
    full.write_glb(str(tmp_path / "n.glb"))
    dataclasses.replace(full, occlusion=True).write_glb(str(tmp_path / "n_ao.glb"))
    _, jn, bn = _glb(str(tmp_path / "n.glb"))
    _, jb, bb = _glb(str(tmp_path / "n_ao.glb"))
    assert jb["materials"][0]["normalTexture"] == {"index": 2, "scale": 1.0}
    assert jb["materials"][0].pop("occlusionTexture") == {"index": 1, "strength": 1.0} and jb == jn and bb == bn
    # read_glb ignores occlusion maps: the file still parses, as the plain one
    a, b = M.read_glb(with_ao), M.read_glb(plain)
    for name in ("v", "f", "vt", "normals", "face_material", "mat_factor", "mat_tex"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # write_textures keeps its file names
    dataclasses.replace(tm, occlusion=True).write_textures(str(tmp_path / "tex"))
    assert sorted(os.listdir(str(tmp_path / "tex"))) == ["roughness_metallic.png", "texture.png"]
