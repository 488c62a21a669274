"""tests/normalmap_numpy.py and the normal map's Python surface without a GPU: the restated point gradient against central
differences, the tangent rule's geometry and handedness, the texel transform on frames it must reproduce, the encoding, the GLB
writer with and without a normal map, the ABI bookkeeping, and the closure of the stream-order table once
tests/test_hip_normalmap.py has registered its cases."""
import dataclasses
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import normalmap_numpy as NM
from tests import primsdf_grad_ref as G
from tests import test_hip_normalmap as TN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ (a) the point gradient
@pytest.mark.parametrize("P,S,n", TN.CASES)
def test_restated_gradient_agrees_with_central_differences(P, S, n):
    """Float64 autograd through the restated field against central differences of the same field, step h = 1e-7: the step stays
    inside the cell, the argmax axis and the box of every point that keeps DELTA = 1e-5 from a kink (h / s <= 7e-7 in u,
    <= 2.4e-6 in f at S = 8).  The differences' own error is eps |o| / h ~ 1e-9 relative plus the curvature of 1 / (W + 1e-6),
    which only matters where W itself is of the order of h / s: those few points are counted, not compared."""
    x, srt, feat, _ = TN._inputs(P, S, n)
    keep = ~G.kinks(x, srt, feat, S, TN.DELTA)
    x = x[keep]
    _, ad = NM.point_grad(x, srt, feat, S, torch.float64)
    cd = NM.central_differences(x, srt, feat, S, h=1e-7)
    cov = NM.covered(x, srt)
    assert float(ad[~cov].abs().max() if (~cov).any() else 0.0) == 0.0 and float(ad[cov].abs().max()) > 0
    scale = ad.abs().amax(1).clamp_min(1.0)
    rel = ((ad - cd).abs().amax(1) / scale)[cov]
    W = G._pairs(x.double(), srt.double())[1].sum(1)[cov]
    thin = W < 1e-3
    print(f"({P}, {S}, {n}): {int(cov.sum())} covered points, median |autograd - central differences| {float(rel.median()):.2e}, "
          f"largest {float(rel[~thin].max()):.2e} (relative; {int(thin.sum())} points with sum w < 1e-3 counted apart: {float(rel.max()):.2e})")
    assert float(rel.median()) <= 1e-8
    assert float(rel[~thin].max()) <= 1e-5 and float(thin.float().mean()) <= 0.01


def test_fill_gradient_is_the_gradient_of_the_fill_value():
    """The written-out fill gradient against central differences of the written-out fill value, away from ties."""
    x, srt, feat, _ = TN._inputs(33, 3, 600)
    x = x[~NM.covered(x, srt)]
    v, g, margin = NM.fill_value_grad(x, srt, feat, 3)
    keep = margin > 1e-4
    h = 1e-6
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        cd = (NM.fill_value_grad(x.double().numpy() + e, srt, feat, 3)[0] - NM.fill_value_grad(x.double().numpy() - e, srt, feat, 3)[0]) / (2 * h)
        assert float(np.abs(cd - g[:, a])[keep].max()) <= 1e-6
    assert keep.sum() > 50 and float(np.abs(np.linalg.norm(g[keep], axis=1) - 1).max()) < 1e-12


# ------------------------------------------------------------------------------------------------ (b) tangents
def _random_frames(n=600, seed=0):
    rng = np.random.default_rng(seed)
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[:6] = np.eye(3)[[0, 0, 1, 1, 2, 2]] * np.array([1, -1, 1, -1, 1, -1])[:, None]      # along the axes
    nrm[6] = 0                                                                              # no normal at all
    label = rng.integers(0, 6, n // 3)
    ft = np.arange(n).reshape(-1, 3)                                                       # one face per three vertices
    return nrm, ft, label


def test_tangent_rule_is_unit_orthogonal_and_handed_as_derived():
    """T1-T4 in float64 on random normals under every label, the axes and a zero normal included: unit T orthogonal to N, and
    w * cross(N, T) along -d pos / d v of the vertex's own plane wherever that plane is not edge-on (rule T1) - the derivation of
    the header, checked with the cross product itself."""
    nrm, ft, label = _random_frames()
    t = NM.tangents(nrm, ft, label)
    T, w = t[:, :3], t[:, 3]
    assert float(np.abs(np.linalg.norm(T, axis=1) - 1).max()) < 1e-12 and set(np.unique(w)) <= {-1.0, 1.0}
    assert float(np.abs((T * nrm).sum(1)).max()) < 1e-12
    vl = NM.vertex_labels(ft, label, len(nrm))
    a, b, c = NM.PROJECTION[vl, 0], NM.PROJECTION[vl, 1], vl // 2
    rows = np.arange(len(nrm))
    t1 = np.abs(nrm[rows, c]) > NM.T1_THRESHOLD * np.abs(nrm).max(1)
    assert t1.sum() > 500 and (~t1).sum() >= 3
    dv = np.zeros_like(nrm)
    dv[rows, b] = 1
    dv[rows, c] = -nrm[rows, b] / np.where(t1, nrm[rows, c], 1)                             # d pos / d v at constant u on the plane
    du = np.zeros_like(nrm)
    du[rows, a] = 1
    du[rows, c] = -nrm[rows, a] / np.where(t1, nrm[rows, c], 1)
    B = w[:, None] * np.cross(nrm, T)
    assert bool(((T * du).sum(1)[t1] > 0).all()) and bool(((B * -dv).sum(1)[t1] > 0).all())
    sigma = np.where(vl & 1, -1, 1)
    assert np.array_equal(w[t1], np.where(sigma * nrm[rows, c] > 0, -1.0, 1.0)[t1])         # a matching label gives w = -1
    # float32 follows within rounding; a vertex no face names stays zero
    t32 = NM.tangents(nrm.astype(np.float32), ft, label, np.float32)
    assert t32.dtype == np.float32 and float(np.abs(t32 - NM.tangents(nrm.astype(np.float32), ft, label)).max()) < 1e-5
    assert not NM.tangents(nrm, ft[:-1], label[:-1])[-3:].any()


def test_uv_derivatives_of_an_affine_map():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((3, 2))
    uv = rng.standard_normal((5, 3, 2))
    p = uv @ A.T + rng.standard_normal(3)
    dpdu, dpdv, det = NM.uv_derivatives(p, uv)
    assert np.allclose(dpdu, A[:, 0]) and np.allclose(dpdv, A[:, 1]) and bool((det != 0).all())


# ------------------------------------------------------------------------------------------------ (c) the texel transform
def test_texel_transform_reproduces_its_own_frame():
    nrm, ft, label = _random_frames(seed=2)
    nrm[6] = (0.6, 0.0, 0.8)
    tang = NM.tangents(nrm, ft, label)
    rng = np.random.default_rng(3)
    lam = rng.dirichlet((8, 8, 8), len(ft)).astype(np.float32)
    lam[:, 1:] *= 1e-3
    lam[:, 0] = 1 - lam[:, 1] - lam[:, 2]                                                   # close to the first corner: a tame frame
    face = np.arange(len(ft))
    _, (Ti, B, Ni), ok = NM.texel_normals(lam, face, ft, nrm, tang, np.tile([0.0, 0.0, 1.0], (len(ft), 1)))
    assert ok.all()
    for vec, want in ((Ti, (1, 0, 0)), (B, (0, 1, 0)), (Ni, (0, 0, 1))):
        got, _, _ = NM.texel_normals(lam, face, ft, nrm, tang, vec)
        assert float(np.abs(got - np.asarray(want, dtype=np.float64)).max()) < 1e-12
    w = tang[ft[:, 0], 3]
    assert float(np.abs((np.cross(Ni, Ti) * B).sum(1) - w).max()) < 1e-12                   # B = w cross(N, T)
    flat, _, ok = NM.texel_normals(lam, face, ft, nrm, tang, np.zeros((len(ft), 3)))
    assert not ok.any() and np.array_equal(flat, np.tile([0.0, 0.0, 1.0], (len(ft), 1)))


# ------------------------------------------------------------------------------------------------ (d) the encoding
def test_encoding_round_trips():
    from topia_xl_amd import mesh as M
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(NM.encode(NM.decode(every)), every)
    assert NM.encode(np.array([0.0, 0.0, 1.0])).tolist() == [128, 128, 255] == list(M.FLAT_NORMAL)
    assert NM.encode(np.array([-1.0, 1.0])).tolist() == [0, 255]
    rng = np.random.default_rng(4)
    n = rng.standard_normal((5000, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert float(np.abs(NM.decode(NM.encode(n)) - n).max()) <= 1.0 / 255.0 + 1e-15           # half a step of 2 / 255
    assert not (NM.encode(n) == 0).all(1).any()                                            # no unit vector encodes as (0, 0, 0)
    n32 = n.astype(np.float32)
    assert np.array_equal(M.encode_normals(n), NM.encode(n)) and np.array_equal(M.encode_normals(torch.from_numpy(n32)).numpy(),
                                                                                NM.encode(n32, np.float32))
    assert np.array_equal(M.decode_normals(torch.from_numpy(every)).numpy(), NM.decode(every))
    # the fill's quantiser gives the byte back from (byte + 0.5) / 255
    x = (every.astype(np.float32) + np.float32(0.5)) / np.float32(255)
    assert np.array_equal(np.trunc(x * np.float32(255)).astype(np.uint8), every)


# ------------------------------------------------------------------------------------------------ (e) the GLB
def _glb(path):
    with open(path, "rb") as fh:
        data = fh.read()
    magic, version, total = struct.unpack_from("<III", data, 0)
    n, kind = struct.unpack_from("<II", data, 12)
    assert magic == 0x46546C67 and version == 2 and total == len(data) and kind == 0x4E4F534A
    m, kind2 = struct.unpack_from("<II", data, 20 + n)
    assert kind2 == 0x004E4942 and 28 + n + m == len(data)
    return json.loads(data[20:20 + n], object_pairs_hook=lambda kv: kv), json.loads(data[20:20 + n]), data[28 + n:]


def _tiny_textured_mesh():
    from topia_xl_amd import mesh as M
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]])
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    nrm = torch.tensor([[0.0, 0, 1]]).repeat(4, 1)
    vt = v[:, :2].contiguous() * 0.5 + 0.25
    rng = np.random.default_rng(5)
    img = lambda: torch.from_numpy(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8))   # noqa: E731
    tang = torch.tensor([[1.0, 0, 0, -1]]).repeat(4, 1)
    return M, M.TexturedMesh(v=v, f=f, normals=nrm, vt=vt, vmap=torch.arange(4), albedo=img(), metallic_roughness=img(),
                             covered=torch.ones(8, 8, dtype=torch.bool)), tang, img()


def test_write_glb_with_and_without_a_normal_map(tmp_path):
    M, tm, tang, nmap = _tiny_textured_mesh()
    assert tm.tangents is None and tm.normal_map is None                                   # the fields come last and default to None
    assert [f.name for f in dataclasses.fields(tm)][-2:] == ["tangents", "normal_map"]
    plain = str(tmp_path / "plain.glb")
    tm.write_glb(plain)
    pairs, js, _ = _glb(plain)
    assert [k for k, _ in pairs] == ["asset", "scene", "scenes", "nodes", "meshes", "images", "samplers", "textures", "materials", "buffers",
                                     "bufferViews", "accessors"]
    prim = js["meshes"][0]["primitives"][0]
    assert list(prim["attributes"]) == ["POSITION", "NORMAL", "TEXCOORD_0"] and len(js["images"]) == 2 and len(js["accessors"]) == 4
    assert js["textures"] == [{"sampler": 0, "source": 0}, {"sampler": 0, "source": 1}]
    assert list(js["materials"][0]) == ["name", "pbrMetallicRoughness"] and b"normalTexture" not in open(plain, "rb").read()
    assert b"TANGENT" not in open(plain, "rb").read()

    full = dataclasses.replace(tm, tangents=tang, normal_map=nmap)
    path = str(tmp_path / "normal.glb")
    full.write_glb(path)
    _, js, blob = _glb(path)
    prim = js["meshes"][0]["primitives"][0]
    assert list(prim["attributes"]) == ["POSITION", "NORMAL", "TEXCOORD_0", "TANGENT"]
    acc = js["accessors"][prim["attributes"]["TANGENT"]]
    assert acc["type"] == "VEC4" and acc["componentType"] == 5126 and acc["count"] == 4
    view = js["bufferViews"][acc["bufferView"]]
    assert view["target"] == 34962 and view["byteLength"] == 64 and view["byteOffset"] % 4 == 0
    got = np.frombuffer(blob[view["byteOffset"]:view["byteOffset"] + 64], dtype="<f4").reshape(4, 4)
    assert np.array_equal(got, tang.numpy())
    assert len(js["images"]) == 3 and js["textures"][2] == {"sampler": 0, "source": 2}
    assert js["materials"][0]["normalTexture"] == {"index": 2, "scale": 1.0}
    assert js["materials"][0]["pbrMetallicRoughness"]["baseColorTexture"] == {"index": 0}
    for k, img in enumerate((full.albedo, full.metallic_roughness, full.normal_map)):
        vw = js["bufferViews"][js["images"][k]["bufferView"]]
        assert "target" not in vw and js["images"][k]["mimeType"] == "image/png"
        assert np.array_equal(M.decode_png(blob[vw["byteOffset"]:vw["byteOffset"] + vw["byteLength"]])[..., :3], img.numpy())
    # the same mesh without the two fields is the plain file, byte for byte; a map without tangents is refused
    dataclasses.replace(full, tangents=None, normal_map=None).write_glb(str(tmp_path / "again.glb"))
    assert open(plain, "rb").read() == open(str(tmp_path / "again.glb"), "rb").read()
    with pytest.raises(ValueError, match="TANGENT"):
        dataclasses.replace(full, tangents=None).write_glb(str(tmp_path / "bad.glb"))
    full.write_textures(str(tmp_path / "tex"))
    assert sorted(os.listdir(str(tmp_path / "tex"))) == ["normal.png", "roughness_metallic.png", "texture.png"]
    assert np.array_equal(M.decode_png(open(str(tmp_path / "tex" / "normal.png"), "rb").read())[..., :3], nmap.numpy())
    tm.write_textures(str(tmp_path / "tex2"))
    assert sorted(os.listdir(str(tmp_path / "tex2"))) == ["roughness_metallic.png", "texture.png"]


def test_read_glb_reads_a_glb_with_a_normal_map_as_before(tmp_path):
    """Reading normalTexture back is out of scope; the file must still load, with the material pointing at the same two textures."""
    M, tm, tang, nmap = _tiny_textured_mesh()
    tm.write_glb(str(tmp_path / "plain.glb"))
    dataclasses.replace(tm, tangents=tang, normal_map=nmap).write_glb(str(tmp_path / "normal.glb"))
    a, b = M.read_glb(str(tmp_path / "normal.glb")), M.read_glb(str(tmp_path / "plain.glb"))
    for name in ("v", "f", "vt", "normals", "face_material", "mat_factor", "mat_tex"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert len(a.images) == 3 and len(b.images) == 2 and all(np.array_equal(x, y) for x, y in zip(a.images, b.images))


def test_public_signatures_default_to_no_normal_map():
    import inspect

    from topia_xl_amd import mesh as M
    for fn in (M.bake_textures, M.extract_texmesh):
        assert inspect.signature(fn).parameters["normal_map"].default is False
    assert inspect.signature(M.field_normals).parameters["chunk"].default == 1 << 21


# ------------------------------------------------------------------------------------------------ (f) stream table, (g) ABI
def test_stream_table_is_closed_with_the_normal_map_cases():
    """tests/test_hip_streams.py may not be edited, so tests/test_hip_normalmap.py registers its cases in that table when it is
    imported.  With them the closure of tests/test_streamorder_cpu.py holds for the header with the three new prototypes."""
    from tests import test_hip_material, test_hip_primsdf_grad, test_hip_raymarch_grad  # noqa: F401  (the other registering modules)
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    for name in TN.STREAM_CASES:
        assert name in TS.CASES
    for name in ("primx_primsdf_query_grad", "primx_texbake_tangents", "primx_texbake_normal_texels"):
        assert name in TS.declared()
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n in TN.STREAM_CASES]      # they run in their own module, not twice


def test_abi_35_declares_the_three_entry_points():
    from topia_xl_amd import _lib
    assert _lib.ABI_VERSION == 35
    want = {"primx_primsdf_query_grad": 12, "primx_texbake_tangents": 7, "primx_texbake_normal_texels": 15}
    with open(os.path.join(ROOT, "include", "primx_hip.h")) as fh:
        text = fh.read()
    assert "#define PRIMX_ABI_VERSION 35" in text
    for name, nargs in want.items():
        sig = _lib.SIGNATURES[name]
        assert len(sig) == nargs and sig[-1] is _lib._p and f"int {name}(" in text, name
        assert _lib._SINCE[name] == 35 and name not in _lib._FEATURES.values()
    assert _lib.SIGNATURES["primx_primsdf_query_grad"][:5] + _lib.SIGNATURES["primx_primsdf_query_grad"][6:] == _lib.SIGNATURES["primx_primsdf_query"]
    assert _lib.SIGNATURES["primx_texbake_normal_texels"][1] is _lib._l


def test_an_ab_build_of_version_35_from_before_the_normal_map_still_loads(monkeypatch, tmp_path):
    from tests import test_lib_capabilities_cpu as TL
    from topia_xl_amd import _lib
    new = {"primx_primsdf_query_grad", "primx_texbake_tangents", "primx_texbake_normal_texels"}
    lib = TL.StandIn(35, set(_lib.SIGNATURES) - new)
    assert TL._load(monkeypatch, tmp_path, lib) == TL.ALL and lib.bound() == set(_lib.SIGNATURES) - new
    with pytest.raises(AttributeError):                               # ... and as the package's own library it is refused
        TL._load(monkeypatch, tmp_path, lib, ab=False)
