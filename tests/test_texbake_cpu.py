"""Texture bake without a GPU: the numpy restatement (tests/texbake_numpy.py) on hand-built and marching-cubes meshes,
its fill against scipy / scikit-learn, the shelf packer, the PNG and textured-GLB writers of mesh.TexturedMesh, and the
host-side argument checks of the texture-bake entry points (csrc/texbake.hip)."""
import ctypes as C
import json
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import mc_numpy
from tests import texbake_numpy as T
from tests.test_mesh_cpu import parse_glb


def cube():
    """12 outward-wound triangles of the unit cube [-1, 1]^3."""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in quads:
        f += [(a, b, c), (a, c, d)]
    f = np.array(f, dtype=np.int32)
    g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("ij,ij->i", g, v[f].mean(1)) > 0).all()          # outward
    return v, f


def test_cube_gives_six_charts():
    v, f = cube()
    lab, comp, nc = T.charts(v, f)
    assert nc == 6
    assert sorted(np.bincount(comp).tolist()) == [2] * 6
    assert len(set(lab.tolist())) == 6
    for c in range(6):                                                 # one label per chart
        assert len(set(lab[comp == c].tolist())) == 1
    uv = T.project(v, f, lab)
    area = (uv[:, 1, 0] - uv[:, 0, 0]) * (uv[:, 2, 1] - uv[:, 0, 1]) - (uv[:, 1, 1] - uv[:, 0, 1]) * (uv[:, 2, 0] - uv[:, 0, 0])
    assert (area > 0).all()


def test_sphere_charts():
    vol = mc_numpy.analytic_fields(64)["sphere"][0]
    v, n, f = mc_numpy.marching_cubes(vol)
    lab, comp, nc = T.charts(v, f, n)
    uv = T.project(v, f, lab)
    area = (uv[:, 1, 0] - uv[:, 0, 0]) * (uv[:, 2, 1] - uv[:, 0, 1]) - (uv[:, 1, 1] - uv[:, 0, 1]) * (uv[:, 2, 0] - uv[:, 0, 0])
    assert (area > 0).all()
    sizes = np.sort(np.bincount(comp))[::-1]
    assert sizes[:6].sum() >= 0.99 * len(f)
    print(f"sphere: {len(f)} faces, {nc} charts ({nc - 6} beyond the six axis charts)")
    # without vertex normals every face is labelled by its own geometric normal
    lab_g, _ = T.face_labels(v, f)
    _, g = T.face_labels(v, f)
    a = lab_g // 2
    sgn = np.where(lab_g % 2 == 1, -1.0, 1.0)
    assert (sgn * g[np.arange(len(g)), a] > 0).all()


def test_charts_follow_shared_vertices_only():
    # two triangles with the same label that touch only through a vertex are one chart; a third, apart, is its own
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0], [5, 5, 0], [6, 5, 0], [5, 6, 0]], np.float32)
    f = np.array([[0, 1, 2], [1, 4, 3], [5, 6, 7]], np.int32)
    lab, comp, nc = T.charts(v, f)
    assert (lab == 4).all() and nc == 2 and comp.tolist() == [0, 0, 1]


def test_fill_restatement_matches_scipy_and_kdtree():
    ndimage = pytest.importorskip("scipy.ndimage")
    neighbors = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(5)
    for trial in range(6):
        H, W = int(rng.integers(20, 70)), int(rng.integers(20, 70))
        blobs = rng.random((H // 6 + 1, W // 6 + 1)) < 0.3
        covered = np.kron(blobs, np.ones((6, 6), bool))[:H, :W]
        covered &= rng.random((H, W)) > 0.05
        if trial % 2 == 0:
            covered[0, :] = True                                       # touching the border
            covered[:, -1] = True
        radius, band = (32, 3) if trial < 4 else (5, 2)
        inpaint, bandm = T.fill_regions(covered, radius, band)
        ref_inpaint = ndimage.binary_dilation(covered, iterations=radius)
        ref_inpaint[covered] = False
        ref_band = covered.copy()
        ref_band[ndimage.binary_erosion(covered, iterations=band)] = False
        np.testing.assert_array_equal(inpaint, ref_inpaint)
        np.testing.assert_array_equal(bandm, ref_band)
        inp, _, src, d2 = T.nearest_band(covered, radius, band)
        sc, ic = np.argwhere(bandm), np.argwhere(inp)
        dist, _ = neighbors.NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(sc).kneighbors(ic)
        np.testing.assert_allclose(np.sqrt(d2[inp]), dist[:, 0], rtol=0, atol=1e-9)
        assert bandm[src[inp][:, 0], src[inp][:, 1]].all()
        # ties go to the smallest row, then column
        for (i, j) in ic[:50]:
            cand = sc[((sc - [i, j]) ** 2).sum(1) == d2[i, j]]
            assert tuple(src[i, j]) == tuple(cand[np.lexsort((cand[:, 1], cand[:, 0]))][0])


def test_fill_restatement_copies_and_quantizes():
    covered = np.zeros((12, 12), bool)
    covered[4:8, 4:8] = True
    t = np.nonzero(covered.reshape(-1))[0]
    attr = np.zeros((len(t), 6), np.float32)
    attr[:, 1:6] = np.linspace(0, 1, len(t) * 5, dtype=np.float32).reshape(-1, 5)
    alb, mr = T.fill(attr, t, covered, radius=2, band=1)
    assert (mr[..., 0] == 0).all()
    np.testing.assert_array_equal(alb.reshape(-1, 3)[t], np.trunc(attr[:, 1:4] * np.float32(255)).astype(np.uint8))
    np.testing.assert_array_equal(mr.reshape(-1, 3)[t][:, 1:], np.trunc(attr[:, 4:6] * np.float32(255)).astype(np.uint8))
    assert (alb[0, 0] == 0).all() and (alb[3, 4] == alb[4, 4]).all() and (alb[2, 4] == alb[4, 4]).all()
    assert (alb[2, 3] == 0).all()                                          # city-block 3 > radius 2: not filled
    assert T.quantize(np.float32(1.0)) == 255 and T.quantize(np.float32(0.999)) == 254


def test_shelf_packer():
    from topia_xl_amd import mesh
    rng = np.random.default_rng(0)
    for W, H, n in ((256, 256, 40), (512, 128, 200), (64, 64, 1)):
        ext = rng.random((n, 2)).astype(np.float32) * rng.random((n, 1)).astype(np.float32) + 1e-3
        s, org = mesh.pack_charts(ext, W, H, gutter=2)
        w, h = mesh._rects(ext, s, 2)
        assert not T.shelf_overlaps(org, w, h, W, H)
        if n > 1:
            assert (w * h).sum() > 0.3 * W * H                           # the scale search fills the atlas
        else:
            assert w[0] > 0.9 * W or h[0] > 0.9 * H
    assert mesh.shelf_pack([300], [5], 256, 256) is None
    org = mesh.shelf_pack([100, 100, 100], [10, 30, 20], 256, 256)
    assert org.tolist() == [[0, 30], [0, 0], [100, 0]]
    with pytest.raises(ValueError):
        mesh.pack_charts(np.ones((5000, 2), np.float32), 32, 32, gutter=2)


def _decode_png(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.setdefault(tag, b"")
        chunks[tag] += body
        pos += 12 + n
    w, h, depth, ctype, _, _, _ = struct.unpack(">IIBBBBB", chunks[b"IHDR"])
    assert depth == 8 and ctype == 2 and b"IEND" in chunks
    raw = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 3)


def test_png_round_trip():
    import io
    from topia_xl_amd.mesh import encode_png
    img = np.random.default_rng(1).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    data = encode_png(img)
    np.testing.assert_array_equal(_decode_png(data), img)
    try:
        from PIL import Image
    except ImportError:
        return
    np.testing.assert_array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), img)


def _textured(nf=2):
    from topia_xl_amd.mesh import TexturedMesh
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [1, 3, 2]][:nf], dtype=torch.int32).reshape(-1, 3)
    vt = torch.tensor([[0.1, 0.1], [0.9, 0.1], [0.1, 0.9], [0.9, 0.9]])
    alb = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (8, 16, 3), dtype=np.uint8))
    mr = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (8, 16, 3), dtype=np.uint8))
    return TexturedMesh(v=v, f=f, normals=torch.tensor([[0, 0, 1.0]] * 4), vt=vt, vmap=torch.arange(4), albedo=alb,
                        metallic_roughness=mr, covered=torch.ones(8, 16, dtype=torch.bool))


def parse_textured_glb(path):
    """-> (json, {accessor: array}, [decoded images]); a GLB without accessors (no faces) is checked here directly."""
    with open(path, "rb") as fh:
        data = fh.read()
    (jlen,) = struct.unpack_from("<I", data, 12)
    gltf = json.loads(data[20:20 + jlen])
    arrays = {}
    if "accessors" in gltf:
        gltf, arrays = parse_glb(path)
    blen, btype = struct.unpack_from("<II", data, 20 + jlen)
    assert btype == 0x004E4942 and 28 + jlen + blen == len(data) == struct.unpack_from("<I", data, 8)[0]
    blob = data[28 + jlen:]
    images = []
    for im in gltf["images"]:
        view = gltf["bufferViews"][im["bufferView"]]
        assert im["mimeType"] == "image/png"
        images.append(_decode_png(blob[view["byteOffset"]:view["byteOffset"] + view["byteLength"]]))
    return gltf, arrays, images


def test_textured_glb_round_trip(tmp_path):
    m = _textured()
    path = str(tmp_path / "t.glb")
    m.write_glb(path)
    gltf, arrays, images = parse_textured_glb(path)
    prim = gltf["meshes"][0]["primitives"][0]
    att = prim["attributes"]
    assert set(att) == {"POSITION", "NORMAL", "TEXCOORD_0"}
    assert gltf["accessors"][att["TEXCOORD_0"]]["type"] == "VEC2"
    np.testing.assert_array_equal(arrays[att["TEXCOORD_0"]], m.vt.numpy())
    np.testing.assert_array_equal(arrays[att["POSITION"]], m.v.numpy())
    np.testing.assert_array_equal(arrays[prim["indices"]].reshape(-1, 3), m.f.numpy())
    assert gltf["accessors"][prim["indices"]]["componentType"] == 5125
    assert len(images) == 2
    np.testing.assert_array_equal(images[0], m.albedo.numpy())
    np.testing.assert_array_equal(images[1], m.metallic_roughness.numpy())
    pbr = gltf["materials"][prim["material"]]["pbrMetallicRoughness"]
    assert pbr["baseColorTexture"]["index"] == 0 and pbr["metallicRoughnessTexture"]["index"] == 1
    assert pbr["metallicFactor"] == 1.0 and pbr["roughnessFactor"] == 1.0 and pbr["baseColorFactor"] == [1.0] * 4
    assert gltf["textures"][0]["source"] == 0 and gltf["textures"][1]["source"] == 1
    assert gltf["samplers"][0] == {"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}
    m.write_textures(str(tmp_path / "tex"))
    for name, img in (("texture.png", m.albedo), ("roughness_metallic.png", m.metallic_roughness)):
        with open(tmp_path / "tex" / name, "rb") as fh:
            np.testing.assert_array_equal(_decode_png(fh.read()), img.numpy())
    # a mesh without faces still parses, with its two images and the material
    e = _textured(0)
    e.write_glb(str(tmp_path / "e.glb"))
    gltf, arrays, images = parse_textured_glb(str(tmp_path / "e.glb"))
    assert "meshes" not in gltf and len(images) == 2 and len(gltf["materials"]) == 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd._lib as L
    return L


def test_texbake_entry_points_reject_bad_arguments_without_gpu(lib):
    """Checks run on the host before any launch: PRIMX_EINVAL (-1) + a message."""
    h = lib.load()
    err = lambda: h.primx_last_error()   # noqa: E731
    assert h.primx_texbake_labels(None, None, None, 0, 0, None, None) == 0          # F == 0: nothing to do
    assert h.primx_texbake_labels(None, None, None, 4, 2, None, None) == -1 and b"null" in err()
    assert h.primx_texbake_labels(1, None, 1, 4, -1, 1, None) == -1 and b">= 0" in err()
    assert h.primx_texbake_labels(1, None, 1, 1 << 29, 2, 1, None) == -1 and b"2^31" in err()
    assert h.primx_texbake_labels(1, None, 1, 0, 2, 1, None) == -1 and b"V = 0" in err()
    ws = C.c_int64(0)
    assert h.primx_texbake_components_workspace(100, 600, C.byref(ws)) == 0 and ws.value >= 4 * (600 + 4 * 100)
    assert h.primx_texbake_components_workspace(100, 600, None) == -1 and b"null" in err()
    assert h.primx_texbake_components_workspace(1 << 30, 6, C.byref(ws)) == -1 and b"2^31" in err()
    assert h.primx_texbake_components_workspace(10, 0, C.byref(ws)) == -1 and b"U >= 1" in err()
    cnt = C.c_int64(7)
    assert h.primx_texbake_components(None, 0, 1, None, 0, None, C.byref(cnt), None) == 0 and cnt.value == 0
    assert h.primx_texbake_components(None, 5, 30, 1, 1 << 20, 1, C.byref(cnt), None) == -1 and b"null" in err()
    assert h.primx_texbake_components(1, 5, 30, 1, 16, 1, C.byref(cnt), None) == -1 and b"workspace" in err()
    assert h.primx_texbake_components(1, -2, 30, 1, 1 << 20, 1, C.byref(cnt), None) == -1
    assert h.primx_texbake_raster_workspace(1024, 1024, C.byref(ws)) == 0 and ws.value >= 16 * 1024
    for W, H in ((0, 16), (16, 0), (16385, 16), (16, 1 << 20)):
        assert h.primx_texbake_raster_workspace(W, H, C.byref(ws)) == -1 and b"[1, 16384]" in err()
        assert h.primx_texbake_raster(1, 1, 3, 1, W, H, 1, 1, 1, 1 << 30, 1, None) == -1
    assert h.primx_texbake_raster(1, 1, 3, 1, 64, 64, None, 1, 1, 1 << 30, 1, None) == -1 and b"null" in err()
    assert h.primx_texbake_raster(None, None, 3, 1, 64, 64, 1, 1, 1, 1 << 30, 1, None) == -1 and b"null" in err()
    assert h.primx_texbake_raster(1, 1, 3, -1, 64, 64, 1, 1, 1, 1 << 30, 1, None) == -1 and b">= 0" in err()
    assert h.primx_texbake_raster(1, 1, 1 << 30, 1, 64, 64, 1, 1, 1, 1 << 30, 1, None) == -1 and b"2^31" in err()
    assert h.primx_texbake_raster(1, 1, 3, 1, 64, 64, 1, 1, 1, 8, 1, None) == -1 and b"workspace" in err()
    assert h.primx_texbake_compact(1, 64, 64, 1, 1 << 20, 1, 1, 3, 1, 1, 3, 1, 0, None, None, None) == 0   # n == 0
    assert h.primx_texbake_compact(1, 64, 64, 1, 1 << 20, 1, 1, 3, 1, 1, 3, 1, 64 * 64 + 1, 1, 1, None) == -1
    assert b"count of texels" in err()
    assert h.primx_texbake_compact(1, 64, 64, 1, 1 << 20, 1, 1, 3, None, 1, 3, 1, 5, 1, 1, None) == -1 and b"null" in err()
    assert h.primx_texbake_compact(1, 64, 64, 1, 8, 1, 1, 3, 1, 1, 3, 1, 5, 1, 1, None) == -1 and b"workspace" in err()
    assert h.primx_texbake_compact(1, 64, 64, 1, 1 << 20, 1, 1, 3, 1, 1, 1 << 30, 1, 5, 1, 1, None) == -1
    assert b"2^31" in err()
    assert h.primx_texbake_fill_workspace(64, 64, C.byref(ws)) == 0 and ws.value >= 9 * 64 * 64
    assert h.primx_texbake_fill_workspace(0, 64, C.byref(ws)) == -1
    big = 1 << 30
    assert h.primx_texbake_fill(1, 1, 5, 1, 64, 64, 0, 3, 1, big, 1, 1, None) == -1 and b"radius" in err()
    assert h.primx_texbake_fill(1, 1, 5, 1, 64, 64, 65, 3, 1, big, 1, 1, None) == -1 and b"radius" in err()
    assert h.primx_texbake_fill(1, 1, 5, 1, 64, 64, 32, 0, 1, big, 1, 1, None) == -1 and b"band" in err()
    assert h.primx_texbake_fill(1, 1, -1, 1, 64, 64, 32, 3, 1, big, 1, 1, None) == -1 and b"count of texels" in err()
    assert h.primx_texbake_fill(None, None, 5, 1, 64, 64, 32, 3, 1, big, 1, 1, None) == -1 and b"null" in err()
    assert h.primx_texbake_fill(1, 1, 5, 1, 64, 64, 32, 3, 1, big, None, 1, None) == -1 and b"null" in err()
    assert h.primx_texbake_fill(1, 1, 5, 1, 64, 64, 32, 3, 1, 100, 1, 1, None) == -1 and b"workspace" in err()
    assert h.primx_texbake_fill(1, 1, 5, 1, 1 << 15, 64, 32, 3, 1, big, 1, 1, None) == -1 and b"[1, 16384]" in err()


def test_texbake_has_no_cpu_path():
    from topia_xl_amd import mesh
    v, f = cube()
    v, f = torch.from_numpy(v), torch.from_numpy(f)
    with pytest.raises(RuntimeError):
        mesh.face_labels(v, f)
    with pytest.raises(RuntimeError):
        mesh.face_components(f, 8)
    with pytest.raises(RuntimeError):
        mesh.uv_unwrap(v, f)
    with pytest.raises(RuntimeError):
        mesh.atlas_raster(torch.zeros(3, 2, dtype=torch.int32), f[:1], 16, 16)
    with pytest.raises(RuntimeError):
        mesh.fill_textures(torch.zeros(0, 6), torch.zeros(0, dtype=torch.int32), torch.full((8, 8), -1, dtype=torch.int32))
    tri = mesh.TriMesh(v, f, v.clone(), v.clone(), torch.zeros(8), torch.zeros(8))
    with pytest.raises(RuntimeError):
        mesh.bake_textures(None, tri, 64)
    from topia_xl_amd.primsdf import PrimSDF
    with pytest.raises(RuntimeError):
        mesh.extract_texmesh(PrimSDF(num_prims=4, prim_shape=4), resolution=8, texture_size=64)
    from topia_xl_amd import pipeline
    with pytest.raises(RuntimeError):
        pipeline.primitives_to_texmesh(torch.zeros(4, 4 + 6 * 8), resolution=8, texture_size=64)
    atlas_fields = {"vt", "vmap", "f", "chart", "n_charts", "scale", "split_rounds", "coverage"}
    assert atlas_fields <= {x.name for x in __import__("dataclasses").fields(mesh.UVAtlas)}
