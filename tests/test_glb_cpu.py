"""glTF in, without a GPU: `mesh.decode_png` against `mesh.encode_png` and Pillow, `mesh.read_glb` on both layouts this project
writes (bit for bit) and on a hand-assembled GLB (u16 indices, an interleaved strided vertex buffer, normalised-u8 UVs, two
primitives under two materials, a parent / child TRS pair, a mirrored node, a primitive without a material), malformed input,
and the float32 restatement of `primx_material_sample` (tests/material_numpy.py) against its float64 self on the inputs of
tests/test_hip_material.py.  The oracle is the glTF 2.0 specification."""
import base64
import io
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import material_numpy as MN
from tests import meshfield_numpy as MF


@pytest.fixture(scope="module")
def M():
    from topia_xl_amd import mesh
    return mesh


# ------------------------------------------------------------------------------------------------ PNG
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (33, 64)])
def test_decode_png_inverts_encode_png(M, shape):
    x = np.random.default_rng(sum(shape)).integers(0, 256, shape + (3,), dtype=np.uint8)
    out = M.decode_png(M.encode_png(x))
    assert out.dtype == np.uint8 and out.shape == shape + (4,)
    assert np.array_equal(out[..., :3], x) and (out[..., 3] == 255).all()


def _smooth(h, w, ch, seed):
    """Pixels with gradients, flat runs and noise, so that an adaptive encoder picks every row filter somewhere."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * (3 + c) + yy * (5 - c)) % 256 for c in range(ch)], -1).astype(np.int64)
    img[h // 5:2 * h // 5] = rng.integers(0, 256, (2 * h // 5 - h // 5, w, ch))
    img[2 * h // 5:3 * h // 5] = 200
    img[3 * h // 5] = rng.integers(0, 256, (w, ch))
    for y in range(3 * h // 5 + 1, 4 * h // 5):             # each pixel the mean of its left and upper neighbours, plus 1: the Average filter's case
        for x in range(w):
            left = img[y, x - 1] if x else 0
            img[y, x] = (((left + img[y - 1, x]) >> 1) + 1) % 256
    img[4 * h // 5:] = ((xx[4 * h // 5:, :, None] ** 2 // 5 + yy[4 * h // 5:, :, None] * 11) + rng.integers(0, 2, (h - 4 * h // 5, w, ch)))
    return (img % 256).astype(np.uint8)


def test_pillow_pngs_decode_to_pillows_pixels_with_all_five_filters(M):
    Image = pytest.importorskip("PIL.Image")
    from topia_xl_amd import gltf
    seen = set()
    for mode, ch in (("RGB", 3), ("RGBA", 4), ("L", 1), ("LA", 2)):
        for k, (h, w) in enumerate(((40, 37), (64, 64), (5, 3))):
            px = _smooth(h, w, ch, 10 * ch + k)
            im = Image.fromarray(px[..., 0] if ch == 1 else px, mode)
            buf = io.BytesIO()
            im.save(buf, "PNG")
            seen |= set(gltf.png_row_filters(buf.getvalue()))
            want = np.asarray(im.convert("RGBA"))
            assert np.array_equal(M.decode_png(buf.getvalue()), want), (mode, h, w)
    pal = Image.fromarray(_smooth(40, 37, 3, 99), "RGB").quantize(17)
    buf = io.BytesIO()
    pal.save(buf, "PNG")
    assert np.array_equal(M.decode_png(buf.getvalue()), np.asarray(pal.convert("RGBA")))
    pal.info["transparency"] = bytes(range(0, 170, 10))
    buf = io.BytesIO()
    pal.save(buf, "PNG", transparency=bytes(range(0, 170, 10)))
    assert np.array_equal(M.decode_png(buf.getvalue()), np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGBA")))
    print("row filters seen in Pillow's files:", sorted(seen))
    assert seen >= {0, 1, 2, 4}
    # Pillow's adaptive encoder did not choose Average (3) for any image tried here (blurred noise, mean-of-neighbours recurrences:
    # it took Paeth even where Average leaves a constant residual), so files whose rows cycle through all five filters are written
    # by `_png_with_filters` below; Pillow decodes each to the pixels that went in, which makes it the oracle for them as well.
    for ctype, ch, mode in ((2, 3, "RGB"), (6, 4, "RGBA"), (0, 1, "L"), (4, 2, "LA")):
        px = _smooth(23, 19, ch, 50 + ch)
        data = _png_with_filters(px, ctype, [(y + ch) % 5 for y in range(23)])
        assert set(gltf.png_row_filters(data)) == {0, 1, 2, 3, 4}
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
        assert Image.open(io.BytesIO(data)).mode == mode and np.array_equal(want[..., :ch] if ch > 2 else want[..., 0], px if ch > 2 else px[..., 0])
        assert np.array_equal(M.decode_png(data), want), mode
        seen |= set(gltf.png_row_filters(data))
    assert seen == {0, 1, 2, 3, 4}


def _png_with_filters(px, ctype, filters):
    """An 8-bit PNG of px [H, W, ch] whose row y uses filter type filters[y] (PNG specification, section 9)."""
    import zlib
    h, w, ch = px.shape
    rows = px.reshape(h, w * ch).astype(np.int64)
    raw = bytearray()
    for y in range(h):
        cur, up = rows[y], rows[y - 1] if y else np.zeros(w * ch, np.int64)
        left = np.concatenate([np.zeros(ch, np.int64), cur[:-ch]])
        upleft = np.concatenate([np.zeros(ch, np.int64), up[:-ch]])
        p = left + up - upleft
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
        paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        pred = (np.zeros_like(cur), left, up, (left + up) >> 1, paeth)[filters[y]]
        raw += bytes([filters[y]]) + ((cur - pred) % 256).astype(np.uint8).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(bytes(raw), 6)) + chunk(b"IEND", b""))


def test_decode_png_refuses_what_it_does_not_read(M):
    good = M.encode_png(np.zeros((2, 2, 3), np.uint8))
    with pytest.raises(ValueError):
        M.decode_png(b"not a png")
    for cut in (7, 20, 40, len(good) - 1):
        with pytest.raises(ValueError):
            M.decode_png(good[:cut])
    bad = bytearray(good)
    bad[30] ^= 1                                            # inside IHDR: the CRC fails
    with pytest.raises(ValueError):
        M.decode_png(bytes(bad))


# ------------------------------------------------------------------------------------------------ the project's own layouts
def _icosphere_trimesh(M):
    v, f = MF.icosphere(1)
    rng = np.random.default_rng(5)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    t = torch.from_numpy
    return M.TriMesh(t(v), t(f), t(n.astype(np.float32)), t(rng.random((v.shape[0], 3)).astype(np.float32)),
                     t(rng.random(v.shape[0]).astype(np.float32)), t(rng.random(v.shape[0]).astype(np.float32)))


def test_trimesh_glb_round_trip_is_bit_exact(M, tmp_path):
    from tests import footprint as fp
    m = _icosphere_trimesh(M)
    path = os.path.join(tmp_path, "tri.glb")
    m.write_glb(path)
    b = M.read_glb(path)
    assert isinstance(b, M.MaterialMesh) and b.f.dtype == torch.int32 and b.face_material.dtype == torch.int32
    assert fp.same_bits(b.v, m.v) and torch.equal(b.f, m.f) and fp.same_bits(b.normals, m.normals)
    assert fp.same_bits(b.color[:, :3].contiguous(), m.albedo) and bool((b.color[:, 3] == 1).all())
    assert fp.same_bits(b.rm, torch.stack([m.roughness, m.metallic], 1))
    assert float(b.vt.abs().max()) == 0 and int(b.face_material.abs().max()) == 0
    assert torch.equal(b.mat_factor, torch.ones(1, 6)) and torch.equal(b.mat_tex, torch.full((1, 2), -1, dtype=torch.int32))
    assert b.images == [] and b.tex_image.shape == (0,) and b.tex_sampler.shape == (0, 3)
    desc, blob = b.texture_tables()
    assert desc.shape == (0, 4) and desc.dtype == torch.int64 and blob.shape == (1, 4)


def test_texturedmesh_glb_round_trip_is_bit_exact(M, tmp_path):
    from tests import footprint as fp
    s = MN.box_scene()
    rng = np.random.default_rng(3)
    t = torch.from_numpy
    alb, mr = rng.integers(0, 256, (6, 9, 3), dtype=np.uint8), rng.integers(0, 256, (6, 9, 3), dtype=np.uint8)
    nrm = rng.standard_normal((24, 3)).astype(np.float32)
    tm = M.TexturedMesh(v=t(s["v"]), f=t(s["f"]), normals=t(nrm), vt=t(s["vt"]), vmap=torch.arange(24), albedo=t(alb),
                        metallic_roughness=t(mr), covered=torch.ones(6, 9, dtype=torch.bool))
    path = os.path.join(tmp_path, "tex.glb")
    tm.write_glb(path)
    b = M.read_glb(path)
    assert fp.same_bits(b.v, tm.v) and torch.equal(b.f, tm.f) and fp.same_bits(b.vt, tm.vt) and fp.same_bits(b.normals, tm.normals)
    assert len(b.images) == 2 and torch.equal(b.images[0][..., :3], tm.albedo) and torch.equal(b.images[1][..., :3], tm.metallic_roughness)
    assert bool((b.images[0][..., 3] == 255).all())
    assert b.mat_tex.tolist() == [[0, 1]] and b.tex_image.tolist() == [0, 1]
    assert b.tex_sampler.tolist() == [[MN.CLAMP, MN.CLAMP, 0]] * 2 and bool((b.color == 1).all()) and bool((b.rm == 1).all())
    desc, blob = b.texture_tables()
    assert desc.tolist() == [[0, 9, 6, 0], [54, 9, 6, 0]] and blob.shape == (108, 4)


# ------------------------------------------------------------------------------------------------ a hand-assembled GLB
def _glb(gltf, blob=b""):
    js = json.dumps(gltf).encode()
    js += b" " * (-len(js) % 4)
    blob = bytes(blob) + b"\0" * (-len(blob) % 4)
    chunks = struct.pack("<II", len(js), 0x4E4F534A) + js
    if blob:
        chunks += struct.pack("<II", len(blob), 0x004E4942) + blob
    return struct.pack("<III", 0x46546C67, 2, 12 + len(chunks)) + chunks


def _quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return [float(x) for x in a * np.sin(angle / 2)] + [float(np.cos(angle / 2))]


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _hand_glb(M):
    """Primitive A: 4 vertices interleaved at stride 24 (position 12 bytes, normalised-u8 UV 2 bytes, normalised-u16 RGB colour
    6 bytes, 4 bytes of padding), u16 indices with a byteOffset, material 1.  Primitive B: 3 vertices, tightly packed floats, u8
    indices, no material.  Nodes: 0 parent (translation + rotation) -> 1 child (scale + translation) with mesh 0 (A and B);
    2 a mirrored node (scale -1 on x) with mesh 1 (A alone, material 0); 3 an identity node with mesh 1."""
    rng = np.random.default_rng(8)
    posA = rng.uniform(-1, 1, (4, 3)).astype(np.float32)
    uvA = rng.integers(0, 256, (4, 2), dtype=np.uint8)
    colA = rng.integers(0, 65536, (4, 3), dtype=np.uint16)
    inter = bytearray()
    for i in range(4):
        inter += posA[i].tobytes() + uvA[i].tobytes() + colA[i].tobytes() + b"\xAA" * 4
    idxA = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    posB = rng.uniform(-1, 1, (3, 3)).astype(np.float32)
    idxB = np.array([2, 1, 0], np.uint8)
    blob = bytearray()
    views = []

    def view(data, stride=None):
        while len(blob) % 4:
            blob.append(0)
        v = {"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)}
        if stride:
            v["byteStride"] = stride
        views.append(v)
        blob.extend(data)
        return len(views) - 1
    vi = view(bytes(inter), 24)
    vx = view(b"\x55" * 2 + idxA.tobytes())                                 # indices behind a 2-byte accessor offset
    vb = view(posB.tobytes())
    vxb = view(idxB.tobytes())
    img = np.random.default_rng(9).integers(0, 256, (4, 3, 3), dtype=np.uint8)
    vimg = view(M.encode_png(img))
    accessors = [
        {"bufferView": vi, "byteOffset": 0, "componentType": 5126, "count": 4, "type": "VEC3"},
        {"bufferView": vi, "byteOffset": 12, "componentType": 5121, "normalized": True, "count": 4, "type": "VEC2"},
        {"bufferView": vi, "byteOffset": 14, "componentType": 5123, "normalized": True, "count": 4, "type": "VEC3"},
        {"bufferView": vx, "byteOffset": 2, "componentType": 5123, "count": 6, "type": "SCALAR"},
        {"bufferView": vb, "componentType": 5126, "count": 3, "type": "VEC3"},
        {"bufferView": vxb, "componentType": 5121, "count": 3, "type": "SCALAR"},
    ]
    primA = {"attributes": {"POSITION": 0, "TEXCOORD_0": 1, "COLOR_0": 2}, "indices": 3}
    q = _quat((1, 2, 3), 0.7)
    gltf = {
        "asset": {"version": "2.0"}, "extensionsUsed": ["KHR_materials_emissive_strength"], "scene": 0,
        "scenes": [{"nodes": [0, 2, 3]}],
        "nodes": [{"translation": [0.5, -1.0, 2.0], "rotation": q, "children": [1]},
                  {"scale": [2.0, 0.5, 1.5], "translation": [0.0, 0.25, 0.0], "mesh": 0},
                  {"scale": [-1.0, 1.0, 1.0], "mesh": 1}, {"mesh": 1}],
        "meshes": [{"primitives": [dict(primA, material=1), {"attributes": {"POSITION": 4}, "indices": 5},
                                   {"attributes": {"POSITION": 4}, "mode": 1}]},
                   {"primitives": [dict(primA, material=0, mode=4)]}],
        "materials": [{"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "roughnessFactor": 0.5}, "alphaMode": "BLEND"},
                      {"pbrMetallicRoughness": {"baseColorFactor": [0.1, 0.2, 0.3, 0.4], "metallicFactor": 0.25,
                                                "metallicRoughnessTexture": {"index": 1, "texCoord": 0}}}],
        "textures": [{"source": 0, "sampler": 0}, {"source": 0}],
        "samplers": [{"magFilter": 9728, "wrapS": 33648, "wrapT": 33071}],
        "images": [{"bufferView": vimg, "mimeType": "image/png"}],
        "buffers": [{"byteLength": len(blob)}], "bufferViews": views, "accessors": accessors,
    }
    return gltf, bytes(blob), dict(posA=posA, uvA=uvA, colA=colA, idxA=idxA, posB=posB, idxB=idxB, q=q, img=img)


def test_hand_assembled_glb(M, tmp_path):
    gltf, blob, d = _hand_glb(M)
    path = os.path.join(tmp_path, "hand.glb")
    with open(path, "wb") as fh:
        fh.write(_glb(gltf, blob))
    m = M.read_glb(path)
    assert m.v.shape == (15, 3) and m.f.shape == (7, 3) and m.normals is None
    # the parent / child pair, composed in float64 and rounded once: p' = T0 R0 (T1 S1 p)
    R = _rot(d["q"])

    def world(p):
        p = p.astype(np.float64) * np.array([2.0, 0.5, 1.5]) + np.array([0.0, 0.25, 0.0])
        return (p @ R.T + np.array([0.5, -1.0, 2.0])).astype(np.float32)
    v = m.v.numpy()
    assert np.abs(v[0:4].astype(np.float64) - world(d["posA"])).max() <= 2.0 ** -22     # one rounding of values below 8
    assert np.abs(v[4:7].astype(np.float64) - world(d["posB"])).max() <= 2.0 ** -22
    mirrored = d["posA"] * np.array([-1, 1, 1], np.float32)
    assert np.array_equal(v[7:11].view(np.uint32), mirrored.view(np.uint32))              # exact in float64, rounded once
    assert np.array_equal(v[11:15].view(np.uint32), d["posA"].view(np.uint32))             # the identity node: the stored bits
    fa = d["idxA"].reshape(2, 3).astype(np.int32)
    f = m.f.numpy()
    assert np.array_equal(f[0:2], fa) and np.array_equal(f[2], d["idxB"].astype(np.int32) + 4)
    assert np.array_equal(f[3:5], fa[:, ::-1] + 7)                                        # the mirror reverses the vertex order
    assert np.array_equal(f[5:7], fa + 11)
    # attributes: normalised u8 / u16 in float32; a VEC3 colour gets alpha 1; absent ones their defaults
    uv = d["uvA"].astype(np.float32) / np.float32(255)
    col = d["colA"].astype(np.float32) / np.float32(65535)
    for lo in (0, 7, 11):
        assert np.array_equal(m.vt.numpy()[lo:lo + 4], uv) and np.array_equal(m.color.numpy()[lo:lo + 4, :3], col)
    assert bool((m.color[:, 3] == 1).all()) and bool((m.vt[4:7] == 0).all()) and bool((m.color[4:7] == 1).all())
    assert bool((m.rm == 1).all())
    # materials: two named ones and the default for the primitive without one
    assert m.face_material.tolist() == [1, 1, 2, 0, 0, 0, 0]
    want = np.array([[1, 1, 1, 1, 0.5, 1], [0.1, 0.2, 0.3, 0.4, 1, 0.25], [1, 1, 1, 1, 1, 1]], np.float32)
    assert np.array_equal(m.mat_factor.numpy(), want)
    assert m.mat_tex.tolist() == [[0, -1], [-1, 1], [-1, -1]]
    assert m.tex_image.tolist() == [0, 0] and m.tex_sampler.tolist() == [[MN.MIRROR, MN.CLAMP, 1], [MN.REPEAT, MN.REPEAT, 0]]
    assert len(m.images) == 1 and np.array_equal(m.images[0].numpy()[..., :3], d["img"])
    desc, texels = m.texture_tables()
    assert desc.tolist() == [[0, 3, 4, MN.flags(MN.MIRROR, MN.CLAMP, True)], [0, 3, 4, MN.flags(MN.REPEAT, MN.REPEAT)]]
    assert texels.shape == (12, 4)
    # the winding number keeps its sign under the mirror: signed volume of the mirrored quad's faces against the original's
    vol = lambda vv, ff: float(np.einsum("ij,ij->i", vv[ff[:, 0]], np.cross(vv[ff[:, 1]], vv[ff[:, 2]])).sum())   # noqa: E731
    assert np.sign(vol(v.astype(np.float64), f[3:5])) == np.sign(vol(v.astype(np.float64), f[5:7]))


def test_external_and_data_uris(M, tmp_path):
    gltf, blob, d = _hand_glb(M)
    png = blob[gltf["bufferViews"][4]["byteOffset"]:][:gltf["bufferViews"][4]["byteLength"]]
    with open(os.path.join(tmp_path, "side tex.png"), "wb") as fh:
        fh.write(png)
    with open(os.path.join(tmp_path, "geo.bin"), "wb") as fh:
        fh.write(blob)
    gltf["buffers"] = [{"byteLength": len(blob), "uri": "geo.bin"}]
    gltf["images"] = [{"uri": "side%20tex.png"}]
    path = os.path.join(tmp_path, "ext.glb")
    with open(path, "wb") as fh:
        fh.write(_glb(gltf))
    a = M.read_glb(path)
    gltf["buffers"] = [{"byteLength": len(blob), "uri": "data:application/octet-stream;base64," + base64.b64encode(blob).decode()}]
    gltf["images"] = [{"uri": "data:image/png;base64," + base64.b64encode(png).decode()}]
    with open(path, "wb") as fh:
        fh.write(_glb(gltf))
    b = M.read_glb(path)
    for m in (a, b):
        assert m.v.shape == (15, 3) and np.array_equal(m.images[0].numpy()[..., :3], d["img"])
    assert torch.equal(a.v, b.v) and torch.equal(a.f, b.f)
    gltf["images"] = [{"uri": "missing.png"}]
    with open(path, "wb") as fh:
        fh.write(_glb(gltf))
    with pytest.raises(ValueError, match="missing.png"):
        M.read_glb(path)


# ------------------------------------------------------------------------------------------------ malformed input
def _write(tmp_path, data, name="bad.glb"):
    path = os.path.join(tmp_path, name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def test_truncated_files_raise_value_error(M, tmp_path):
    gltf, blob, _ = _hand_glb(M)
    data = _glb(gltf, blob)
    json_end = 20 + struct.unpack("<I", data[12:16])[0]
    for cut in (0, 5, 11, 12, 19, 20, 100, json_end - 1, json_end, json_end + 4, json_end + 8, json_end + 50, len(data) - 4, len(data) - 1):
        with pytest.raises(ValueError):
            M.read_glb(_write(tmp_path, data[:cut]))
        # ... and with the header's length patched to the bytes present, so that the chunk and accessor checks are reached
        if cut >= 12:
            with pytest.raises(ValueError):
                M.read_glb(_write(tmp_path, data[:8] + struct.pack("<I", cut) + data[12:cut]))
    # a BIN chunk shorter than the buffer states; an accessor past its bufferView; a bufferView past the buffer; bad indices
    short = _glb(gltf, blob[:len(blob) - 8])
    with pytest.raises(ValueError, match="bytes"):
        M.read_glb(_write(tmp_path, short))
    for edit in (lambda g: g["accessors"][0].update(count=5), lambda g: g["bufferViews"][0].update(byteLength=10 ** 6),
                 lambda g: g["accessors"][3].update(byteOffset=4), lambda g: g["bufferViews"][0].update(byteStride=8),
                 lambda g: g["accessors"][5].update(componentType=5126), lambda g: g["meshes"][0]["primitives"][0].update(material=7),
                 lambda g: g["nodes"][1].update(children=[0]), lambda g: g["accessors"][0].update(bufferView=99),
                 lambda g: g["textures"][0].update(source=3), lambda g: g["nodes"][0].update(rotation=[0, 0, 1]),
                 lambda g: g["accessors"].__setitem__(4, "nonsense"), lambda g: g.update(scene=5)):
        g2 = json.loads(json.dumps(gltf))
        edit(g2)
        with pytest.raises(ValueError):
            M.read_glb(_write(tmp_path, _glb(g2, blob)))
    g2 = json.loads(json.dumps(gltf))
    g2["accessors"][5] = dict(g2["accessors"][5], count=3)
    raw = bytearray(blob)
    raw[gltf["bufferViews"][3]["byteOffset"]] = 9                                          # an index past the vertices
    with pytest.raises(ValueError, match="index"):
        M.read_glb(_write(tmp_path, _glb(g2, bytes(raw))))
    for junk in (b"", b"glTF", b"\0" * 64, _glb(gltf, blob).replace(b"glTF", b"glTX", 1)):
        with pytest.raises(ValueError):
            M.read_glb(_write(tmp_path, junk))
    with pytest.raises(ValueError, match="version"):
        M.read_glb(_write(tmp_path, b"glTF" + struct.pack("<II", 1, 12)))


def test_required_extensions_sparse_and_texcoord1_raise(M, tmp_path):
    gltf, blob, _ = _hand_glb(M)
    g2 = json.loads(json.dumps(gltf))
    g2["extensionsRequired"] = ["KHR_draco_mesh_compression", "KHR_texture_transform"]
    with pytest.raises(ValueError, match="KHR_draco_mesh_compression, KHR_texture_transform"):
        M.read_glb(_write(tmp_path, _glb(g2, blob)))
    g2 = json.loads(json.dumps(gltf))
    g2["accessors"][0]["sparse"] = {"count": 1, "indices": {"bufferView": 3, "componentType": 5123}, "values": {"bufferView": 2}}
    with pytest.raises(NotImplementedError, match="sparse"):
        M.read_glb(_write(tmp_path, _glb(g2, blob)))
    g2 = json.loads(json.dumps(gltf))
    g2["materials"][1]["pbrMetallicRoughness"]["metallicRoughnessTexture"]["texCoord"] = 1
    with pytest.raises(ValueError, match="texCoord"):
        M.read_glb(_write(tmp_path, _glb(g2, blob)))
    # extensions that are only used are ignored (the fixture itself lists one)
    assert M.read_glb(_write(tmp_path, _glb(gltf, blob))).f.shape == (7, 3)


def test_identity_node_keeps_position_bits(M, tmp_path):
    """Positions with every kind of float32 payload (denormals, -0.0, huge values) under a node without a transform, under an explicit
    identity matrix and under unit TRS: the stored bits come back."""
    bits = np.array([0x00000001, 0x80000000, 0x7F7FFFFF, 0x3F800001, 0x00800000, 0xBF7FFFFF, 0x33800000, 0x4B000001, 0x00000000],
                    np.uint32)
    pos = bits.view(np.float32).reshape(3, 3)
    ident = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0]
    for node in ({}, {"matrix": ident}, {"translation": [0, 0, 0], "rotation": [0, 0, 0, 1], "scale": [1, 1, 1]}):
        gltf = {"asset": {"version": "2.0"}, "scenes": [{"nodes": [0]}], "nodes": [dict(node, mesh=0)],
                "meshes": [{"primitives": [{"attributes": {"POSITION": 0}}]}], "buffers": [{"byteLength": 36}],
                "bufferViews": [{"buffer": 0, "byteLength": 36}],
                "accessors": [{"bufferView": 0, "componentType": 5126, "count": 3, "type": "VEC3"}]}
        m = M.read_glb(_write(tmp_path, _glb(gltf, pos.tobytes()), "ident.glb"))
        assert np.array_equal(m.v.numpy().view(np.uint32), pos.view(np.uint32)), node
        assert m.f.tolist() == [[0, 1, 2]] and m.face_material.tolist() == [0] and m.mat_tex.tolist() == [[-1, -1]]


# ------------------------------------------------------------------------------------------------ the restatement
def test_wrap_modes_follow_the_specification():
    i = np.arange(-9, 10)
    assert MN.wrap(i, 4, MN.CLAMP).tolist() == [0] * 9 + [0, 1, 2, 3] + [3] * 6
    assert MN.wrap(i, 4, MN.REPEAT).tolist() == [3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    assert MN.wrap(i, 4, MN.MIRROR).tolist() == [0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1]
    assert MN.wrap(np.array([-3, 0, 5]), 1, MN.MIRROR).tolist() == [0, 0, 0]


def test_restated_sampler_on_hand_values():
    """A 2 x 2 texture: at a texel centre LINEAR returns that texel, halfway between two centres their mean, NEAREST the texel
    whose cell holds the point; factors, colours and multipliers multiply; a material without a texture samples 1."""
    img = np.zeros((2, 2, 4), np.uint8)
    img[0, 0, :3], img[0, 1, :3], img[1, 0, :3], img[1, 1, :3] = (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 255)
    for near in (False, True):
        desc, blob = MN.pack([img], [(0, MN.flags(MN.CLAMP, MN.CLAMP, near))])
        args = (np.zeros(5, np.int32), np.array([0], np.int32), np.ones((1, 6), np.float32), np.array([[0, 0]], np.int32), desc, blob)
        uv = np.array([[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.5, 0.25], [-5.0, 9.0]], np.float32)
        out = MN.sample(uv, None, *args, np.float64)
        assert np.array_equal(out[0], [1, 0, 0, 0, 0]) and np.array_equal(out[1], [0, 1, 0, 1, 0]) and np.array_equal(out[2], [0, 0, 1, 0, 1])
        assert np.array_equal(out[3], [0, 1, 0, 1, 0] if near else [0.5, 0.5, 0, 0.5, 0]) and np.array_equal(out[4], [0, 0, 1, 0, 1])
    fac = np.array([[0.5, 0.25, 1.0, 9.0, 0.5, 0.25]], np.float32)
    va = np.array([[0.5, 1.0, 0.5, 7.0, 0.5, 2.0]], np.float32)
    out = MN.sample(np.array([[np.nan, np.inf]], np.float32), va, np.zeros(1, np.int32), np.array([0], np.int32), fac,
                    np.array([[-1, -1]], np.int32), np.zeros((0, 4), np.int64), np.zeros((1, 4), np.uint8), np.float32)
    assert out.dtype == np.float32 and np.array_equal(out[0], [0.25, 0.25, 0.5, 0.25, 0.5])


def test_float32_restatement_against_float64_on_the_gpu_tests_inputs():
    """The floor of the GPU tests: the float32 restatement's distance from its float64 self, per sampler configuration (the kernel test
    itself compares bit for bit), LINEAR inside a few float32 roundings of values in [0, 1.25]; NEAREST identical wherever both
    precisions pick the same texel.  Printed."""
    worst = 0.0
    for size in range(len(MN.SIZES)):
        for ws in (MN.CLAMP, MN.REPEAT, MN.MIRROR):
            for wt in (MN.CLAMP, MN.REPEAT, MN.MIRROR):
                s = MN.sampler_scene(ws, wt, False, size)
                r64, r32 = MN.restated(s, np.float64), MN.restated(s, np.float32)
                assert r32.dtype == np.float32 and np.isfinite(r32).all() and np.isfinite(r64).all()
                worst = max(worst, float(np.abs(r32.astype(np.float64) - r64).max()))
    print(f"sampler, LINEAR: float32 restatement against float64, max-abs {worst:.3e}")
    # u * W carries up to half an ulp of |u| W <= 4 x 64 (2^-16 absolute), which the texel slope (at most 1 per texel) passes on
    assert 0 < worst <= 2.0 ** -14
    s = MN.box_scene()
    v, f = s["v"], s["f"]
    from tests.test_hip_meshfield import _points
    p = _points(v, f, 1000, seed=4)
    face = MF.query(p, v, f, None, np.float64, keep_d2=False)["face"]
    a64, a32 = (MN.field_attributes(MF, p, v, face, s, t) for t in (np.float64, np.float32))
    floor = float(np.abs(a32.astype(np.float64) - a64).max())
    print(f"textured box, 1000 points: float32 pipeline against float64, max-abs {floor:.3e} (the field-level bound is 4 x this)")
    assert 0 < floor <= 2.0 ** -16 and a64.min() >= 0 and a64.max() <= 1 and a64[:, :3].std() > 0.05


def test_abi_declares_the_material_sampler():
    from tests import test_hip_material as TM
    from tests import test_hip_primsdf_grad, test_hip_raymarch_grad  # noqa: F401  (they register their cases in the same table)
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    from topia_xl_amd import _lib
    assert _lib.ABI_VERSION >= 35 and len(_lib.SIGNATURES["primx_material_sample"]) == 16
    assert _lib.SIGNATURES["primx_material_sample"][3] is _lib._l and _lib.SIGNATURES["primx_material_sample"][12] is _lib._l
    for name in TM.STREAM_CASES:
        assert name in TS.CASES and name in TS.MUST_SYNC
    assert "primx_material_sample" in TS.declared()
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n in TM.STREAM_CASES]
