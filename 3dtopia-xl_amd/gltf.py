"""glTF 2.0 in: `read_glb` -> `MaterialMesh` (a triangle mesh with UVs, vertex colours, a material table and its images), and
`decode_png`, the counterpart of `mesh.encode_png`.  Host code: Python's standard library and numpy; Pillow only for the image
formats `decode_png` does not read.  `mesh.py` re-exports the three names; `fit.MeshField` evaluates the material on the device
(csrc/material.hip, include/primx_hip.h "Textured meshes").

The oracle of this file is the glTF 2.0 specification (and the PNG specification): the reference loads its assets through
trimesh and pygltflib (utils/mesh.py), neither of which is a dependency here.
"""
from __future__ import annotations

import base64
import dataclasses
import json
import os
import struct
import zlib
from typing import List, Optional
from urllib.parse import unquote

import numpy as np
import torch

WRAP_CLAMP, WRAP_REPEAT, WRAP_MIRROR = 0, 1, 2          # the codes of tex_sampler and of the kernel's descriptor flags
_WRAP = {33071: WRAP_CLAMP, 10497: WRAP_REPEAT, 33648: WRAP_MIRROR}
_COMP = {5120: np.dtype("i1"), 5121: np.dtype("u1"), 5122: np.dtype("<i2"), 5123: np.dtype("<u2"), 5125: np.dtype("<u4"),
         5126: np.dtype("<f4")}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}
_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


# ---------------------------------------------------------------------------------------------------------------- PNG
def _unfilter(raw: bytes, h: int, stride: int, bpp: int) -> np.ndarray:
    """The five row filters of PNG undone: raw = h rows of (filter byte, stride bytes) -> [h, stride] uint8.  None, Sub and Up are
    numpy operations on a whole row; Average and Paeth depend on the byte to the left and run byte by byte."""
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.uint8)
    data = np.frombuffer(raw, np.uint8).reshape(h, stride + 1)
    for y in range(h):
        ft, line = int(data[y, 0]), data[y, 1:]
        if ft == 0:
            cur = line.copy()
        elif ft == 1:
            n = -(-stride // bpp)
            pad = np.zeros(n * bpp, np.uint8)
            pad[:stride] = line
            cur = np.cumsum(pad.reshape(n, bpp), axis=0, dtype=np.uint8).reshape(-1)[:stride]
        elif ft == 2:
            cur = line + prev
        elif ft in (3, 4):
            cur_b, up = bytearray(line.tobytes()), prev.tobytes()
            if ft == 3:
                for i in range(stride):
                    left = cur_b[i - bpp] if i >= bpp else 0
                    cur_b[i] = (cur_b[i] + ((left + up[i]) >> 1)) & 255
            else:
                for i in range(stride):
                    a = cur_b[i - bpp] if i >= bpp else 0
                    b = up[i]
                    c = up[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                    cur_b[i] = (cur_b[i] + pred) & 255
            cur = np.frombuffer(bytes(cur_b), np.uint8)
        else:
            raise ValueError(f"PNG: row {y} has filter type {ft}")
        out[y] = cur
        prev = out[y]
    return out


def png_row_filters(data: bytes) -> List[int]:
    """The filter byte of every row of an 8-bit non-interlaced PNG (what the encoder chose; for tests and diagnostics)."""
    w, h, ch, _, _, raw = _png_parts(data)
    return [raw[y * (w * ch + 1)] for y in range(h)]


def _png_parts(data: bytes):
    if data[:8] != _PNG_MAGIC:
        raise ValueError("not a PNG file")
    pos, ihdr, plte, trns, idat, ended = 8, None, None, None, [], False
    while pos < len(data) and not ended:
        if pos + 8 > len(data):
            raise ValueError("PNG: truncated chunk header")
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise ValueError(f"PNG: chunk {tag!r} runs past the end of the data")
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"PNG: chunk {tag!r} fails its CRC")
        if tag == b"IHDR":
            ihdr = body
        elif tag == b"PLTE":
            plte = body
        elif tag == b"tRNS":
            trns = body
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            ended = True
        pos += 12 + n
    if ihdr is None or len(ihdr) != 13 or not idat or not ended:
        raise ValueError("PNG: IHDR, IDAT or IEND is missing")
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ihdr)
    if w < 1 or h < 1 or comp != 0 or filt != 0 or ctype not in (0, 2, 3, 4, 6):
        raise ValueError("PNG: malformed IHDR")
    if depth != 8 or lace != 0:
        raise NotImplementedError(f"PNG with bit depth {depth}, interlace {lace}: decode_png reads 8-bit non-interlaced files")
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError(f"PNG: the image data does not inflate ({e})") from None
    if len(raw) != h * (w * ch + 1):
        raise ValueError(f"PNG: {len(raw)} bytes of image data for {w} x {h} x {ch}")
    return w, h, ch, ctype, (plte, trns), raw


def decode_png(data: bytes) -> np.ndarray:
    """An 8-bit, non-interlaced PNG of colour type 0 (grey), 2 (RGB), 3 (palette), 4 (grey + alpha) or 6 (RGBA), with any of the
    five row filters -> uint8 [H, W, 4]; stdlib only.  Grey expands to RGB; a missing alpha channel is 255 (a palette's tRNS
    chunk is its alpha; the colour key of types 0 and 2 is not applied).  16-bit and interlaced files raise NotImplementedError,
    anything malformed ValueError.  `decode_png(encode_png(x))[..., :3] == x`."""
    w, h, ch, ctype, (plte, trns), raw = _png_parts(bytes(data))
    px = _unfilter(raw, h, w * ch, ch).reshape(h, w, ch)
    out = np.full((h, w, 4), 255, np.uint8)
    if ctype == 0:
        out[..., :3] = px
    elif ctype == 2:
        out[..., :3] = px
    elif ctype == 4:
        out[..., :3], out[..., 3] = px[..., :1], px[..., 1]
    elif ctype == 6:
        out[...] = px
    else:
        if plte is None or len(plte) % 3 or not plte:
            raise ValueError("PNG: a palette image without a PLTE chunk")
        pal = np.full((256, 4), 255, np.uint8)
        n = len(plte) // 3
        pal[:n, :3] = np.frombuffer(plte, np.uint8).reshape(n, 3)
        if trns:
            pal[:min(len(trns), 256), 3] = np.frombuffer(trns[:256], np.uint8)
        if int(px.max()) >= n:
            raise ValueError("PNG: a palette index past the end of PLTE")
        out = pal[px[..., 0]]
    return np.ascontiguousarray(out)


def decode_image(data: bytes) -> np.ndarray:
    """Image bytes -> uint8 [H, W, 4].  8-bit non-interlaced PNGs go through `decode_png`; everything else (JPEG, 16-bit or
    interlaced PNG, ...) through Pillow where it imports, converted to 8-bit RGBA, and raises ValueError where it does not."""
    data = bytes(data)
    if data[:8] == _PNG_MAGIC:
        try:
            return decode_png(data)
        except NotImplementedError:
            pass
    try:
        from PIL import Image
    except ImportError:
        raise ValueError("this image is not an 8-bit non-interlaced PNG and Pillow is not installed: only such PNGs are read "
                         "without it") from None
    import io
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.ascontiguousarray(np.asarray(im.convert("RGBA"), dtype=np.uint8))
    except Exception as e:   # noqa: BLE001  (Pillow raises many kinds)
        raise ValueError(f"the image could not be decoded ({e})") from None


# ---------------------------------------------------------------------------------------------------------------- the mesh type
@dataclasses.dataclass
class MaterialMesh:
    """A triangle mesh with glTF metallic-roughness materials (CPU or device tensors):

    v [V, 3] float32, f [F, 3] int32, vt [V, 2] float32 (TEXCOORD_0; zeros if absent), color [V, 4] float32 (COLOR_0; ones if
    absent), rm [V, 2] float32 (this project's `_ROUGHNESS_METALLIC` attribute: per-vertex multipliers of the roughness and
    metallic factors, as `color` multiplies the base colour; ones if absent), face_material [F] int32 into the material table,
    normals [V, 3] float32 or None.  The material table, one row per material (the last row is glTF's default material when a
    primitive names none): mat_factor [M, 6] float32 = (baseColorFactor r, g, b, a, roughnessFactor, metallicFactor), mat_tex
    [M, 2] int32 = (base-colour texture, metallic-roughness texture), -1 for none.  Per texture: tex_image [T] int32 into
    `images`, tex_sampler [T, 3] int32 = (wrapS, wrapT, nearest) with wrap 0 CLAMP_TO_EDGE, 1 REPEAT, 2 MIRRORED_REPEAT and
    nearest 1 when the magnification filter is NEAREST.  images: uint8 [H, W, 4] tensors (RGBA, row 0 first, as stored: no sRGB
    decode)."""
    v: torch.Tensor
    f: torch.Tensor
    vt: torch.Tensor
    color: torch.Tensor
    rm: torch.Tensor
    face_material: torch.Tensor
    mat_factor: torch.Tensor
    mat_tex: torch.Tensor
    tex_image: torch.Tensor
    tex_sampler: torch.Tensor
    images: List[torch.Tensor]
    normals: Optional[torch.Tensor] = None

    def to(self, device) -> "MaterialMesh":
        m = lambda t: None if t is None else t.to(device)   # noqa: E731
        return MaterialMesh(**{k.name: ([m(i) for i in getattr(self, k.name)] if k.name == "images" else m(getattr(self, k.name)))
                               for k in dataclasses.fields(self)})

    def vertex_attr(self) -> torch.Tensor:
        """[V, 8] float32 = [vt | color | rm]: the per-vertex attributes `primx_mesh_field_query` interpolates."""
        return torch.cat([self.vt.float().reshape(-1, 2), self.color.float().reshape(-1, 4), self.rm.float().reshape(-1, 2)],
                         1).contiguous()

    def texture_tables(self):
        """-> (tex_desc [T, 4] int64 = (texel offset, W, H, wrapS | wrapT << 2 | nearest << 4), texels [n, 4] uint8): the
        descriptor table and the packed RGBA8 blob of `primx_material_sample`, on the CPU.  Every image is packed once, however
        many textures use it; the blob has at least one texel."""
        offs, parts, off = [], [], 0
        for img in self.images:
            if img.dim() != 3 or img.shape[2] != 4 or img.dtype != torch.uint8:
                raise ValueError(f"images must be uint8 [H, W, 4], got {tuple(img.shape)} {img.dtype}")
            offs.append(off)
            parts.append(img.reshape(-1, 4).cpu())
            off += img.shape[0] * img.shape[1]
        rows = []
        for t in range(self.tex_image.shape[0]):
            i = int(self.tex_image[t])
            if not 0 <= i < len(self.images):
                raise ValueError(f"texture {t} names image {i} of {len(self.images)}")
            ws, wt, near = (int(x) for x in self.tex_sampler[t])
            rows.append([offs[i], self.images[i].shape[1], self.images[i].shape[0], ws | wt << 2 | (1 if near else 0) << 4])
        desc = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4)
        blob = torch.cat(parts) if parts else torch.zeros(1, 4, dtype=torch.uint8)
        return desc, blob.contiguous()


def material_mesh(v, f, vt=None, color=None, rm=None, face_material=None, mat_factor=None, mat_tex=None, tex_image=None,
                  tex_sampler=None, images=(), normals=None) -> MaterialMesh:
    """A `MaterialMesh` from its parts, with the reader's defaults for the ones left out: zero UVs, white colour, unit
    multipliers, one untextured material with factors 1, LINEAR / REPEAT samplers, texture t -> image t."""
    t = torch.as_tensor
    v, f = t(v).float(), t(f).int()
    V, F, dev = v.shape[0], f.shape[0], v.device
    z = lambda *s, dt=torch.float32, val=0: torch.full(s, val, dtype=dt, device=dev)   # noqa: E731
    images = [t(i) for i in images]
    tex_image = torch.arange(len(images), dtype=torch.int32) if tex_image is None else t(tex_image).int()
    T = tex_image.shape[0]
    return MaterialMesh(
        v=v, f=f, vt=z(V, 2) if vt is None else t(vt).float(), color=z(V, 4, val=1) if color is None else t(color).float(),
        rm=z(V, 2, val=1) if rm is None else t(rm).float(),
        face_material=z(F, dt=torch.int32) if face_material is None else t(face_material).int(),
        mat_factor=torch.ones(1, 6) if mat_factor is None else t(mat_factor).float().reshape(-1, 6),
        mat_tex=torch.full((1, 2), -1, dtype=torch.int32) if mat_tex is None else t(mat_tex).int().reshape(-1, 2),
        tex_image=tex_image,
        tex_sampler=torch.tensor([[WRAP_REPEAT, WRAP_REPEAT, 0]] * T, dtype=torch.int32).reshape(-1, 3) if tex_sampler is None
        else t(tex_sampler).int().reshape(-1, 3),
        images=images, normals=None if normals is None else t(normals).float())


# ---------------------------------------------------------------------------------------------------------------- the reader
def _need(cond, msg):
    if not cond:
        raise ValueError(msg)


def _index(x, n, what):
    _need(isinstance(x, int) and not isinstance(x, bool) and 0 <= x < n, f"{what} {x!r} is not an index into {n} entries")
    return x


def _uri_bytes(uri, base_dir, what):
    _need(isinstance(uri, str), f"{what}: the uri is not a string")
    if uri.startswith("data:"):
        head, sep, payload = uri.partition(",")
        _need(bool(sep), f"{what}: malformed data: URI")
        try:
            return base64.b64decode(payload, validate=False) if head.endswith(";base64") else unquote(payload).encode("latin-1")
        except Exception as e:   # noqa: BLE001
            raise ValueError(f"{what}: the data: URI does not decode ({e})") from None
    _need("://" not in uri and base_dir is not None, f"{what}: only data: URIs and relative file URIs are read, got {uri[:40]!r}")
    path = os.path.join(base_dir, unquote(uri))
    try:
        with open(path, "rb") as fh:
            return fh.read()
    except OSError as e:
        raise ValueError(f"{what}: {path} cannot be read ({e})") from None


def _accessor(g, buffers, idx, what):
    """Accessor idx -> numpy [count, components] in the component type (a copy).  byteOffset, byteStride and every length are
    checked against the bytes present."""
    accs = g.get("accessors") or []
    a = accs[_index(idx, len(accs), f"{what}: accessor")]
    if "sparse" in a:
        raise NotImplementedError(f"{what}: sparse accessors are not read")
    comp, typ, count = a.get("componentType"), a.get("type"), a.get("count")
    _need(comp in _COMP and typ in _NCOMP, f"{what}: accessor type {comp!r} / {typ!r} is not read")
    _need(isinstance(count, int) and count >= 0, f"{what}: accessor count {count!r}")
    dt, nc = _COMP[comp], _NCOMP[typ]
    if "bufferView" not in a:
        return np.zeros((count, nc), dt), bool(a.get("normalized"))
    views = g.get("bufferViews") or []
    bv = views[_index(a["bufferView"], len(views), f"{what}: bufferView")]
    buf = buffers[_index(bv.get("buffer"), len(buffers), f"{what}: buffer")]
    v_off, v_len, a_off = bv.get("byteOffset", 0), bv.get("byteLength"), a.get("byteOffset", 0)
    esize = dt.itemsize * nc
    stride = bv.get("byteStride") or esize
    for x in (v_off, v_len, a_off, stride):
        _need(isinstance(x, int) and not isinstance(x, bool) and x >= 0, f"{what}: a byte offset, length or stride is {x!r}")
    _need(stride >= esize, f"{what}: byteStride {stride} is smaller than an element ({esize})")
    _need(v_off + v_len <= len(buf), f"{what}: the bufferView ends at byte {v_off + v_len} of a buffer of {len(buf)}")
    if count:
        _need(a_off + stride * (count - 1) + esize <= v_len,
              f"{what}: {count} elements of {esize} bytes at stride {stride} from byte {a_off} do not fit a bufferView of {v_len} bytes")
    arr = np.ndarray((count, nc), dt, buffer=buf, offset=v_off + a_off, strides=(stride, dt.itemsize)) if count else \
        np.zeros((0, nc), dt)
    return np.array(arr), bool(a.get("normalized"))


def _unit_float(arr, normalized, what):
    """TEXCOORD / COLOR components -> float32: floats as stored, normalised u8 / u16 as x / 255 and x / 65535 in float32."""
    if arr.dtype == np.dtype("<f4"):
        return arr.astype(np.float32)
    _need(normalized and arr.dtype in (np.dtype("u1"), np.dtype("<u2")), f"{what}: only float and normalised u8 / u16 are read")
    return arr.astype(np.float32) / np.float32(255.0 if arr.dtype == np.dtype("u1") else 65535.0)


def _node_matrix(node):
    """The node's local transform in float64 (column vectors: p' = M p)."""
    if "matrix" in node:
        m = np.asarray(node["matrix"], np.float64)
        _need(m.shape == (16,), "a node matrix needs 16 numbers")
        return m.reshape(4, 4).T                                   # glTF stores column-major
    T, R, S = np.eye(4), np.eye(4), np.eye(4)
    if "translation" in node:
        t = np.asarray(node["translation"], np.float64)
        _need(t.shape == (3,), "a node translation needs 3 numbers")
        T[:3, 3] = t
    if "rotation" in node:
        q = np.asarray(node["rotation"], np.float64)
        _need(q.shape == (4,), "a node rotation needs 4 numbers")
        x, y, z, w = q
        R[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    if "scale" in node:
        s = np.asarray(node["scale"], np.float64)
        _need(s.shape == (3,), "a node scale needs 3 numbers")
        S[0, 0], S[1, 1], S[2, 2] = s
    return T @ R @ S


def _split_glb(data: bytes, path: str):
    _need(len(data) >= 12, f"{path}: {len(data)} bytes are no GLB header")
    magic, version, total = struct.unpack("<III", data[:12])
    _need(magic == 0x46546C67, f"{path}: not a GLB file")
    _need(version == 2, f"{path}: GLB version {version}, only 2 is read")
    _need(total == len(data), f"{path}: the header states {total} bytes, the file has {len(data)}")
    pos, js, bin_chunk = 12, None, None
    while pos < total:
        _need(pos + 8 <= total, f"{path}: truncated chunk header at byte {pos}")
        n, kind = struct.unpack("<II", data[pos:pos + 8])
        _need(pos + 8 + n <= total, f"{path}: a chunk of {n} bytes at byte {pos} runs past the end")
        body = data[pos + 8:pos + 8 + n]
        if kind == 0x4E4F534A and js is None:
            js = body
        elif kind == 0x004E4942 and bin_chunk is None:
            bin_chunk = body
        pos += 8 + n
    _need(js is not None, f"{path}: no JSON chunk")
    try:
        g = json.loads(js.decode("utf-8"))
    except (UnicodeDecodeError, ValueError) as e:
        raise ValueError(f"{path}: the JSON chunk does not parse ({e})") from None
    _need(isinstance(g, dict), f"{path}: the JSON chunk is not an object")
    return g, bin_chunk


def _read(path: str):
    with open(path, "rb") as fh:
        data = fh.read()
    g, bin_chunk = _split_glb(data, path)
    base_dir = os.path.dirname(os.path.abspath(path))
    required = g.get("extensionsRequired") or []
    _need(not required, f"{path}: required extensions are not supported: {', '.join(map(str, required))}")
    buffers = []
    for i, b in enumerate(g.get("buffers") or []):
        if "uri" in b:
            raw = _uri_bytes(b["uri"], base_dir, f"buffer {i}")
        else:
            _need(i == 0 and bin_chunk is not None, f"buffer {i} has no uri and there is no BIN chunk for it")
            raw = bin_chunk
        n = b.get("byteLength")
        _need(isinstance(n, int) and 0 <= n <= len(raw), f"buffer {i} states {n!r} bytes, {len(raw)} are present")
        buffers.append(raw)

    # ---- images, textures, materials
    image_cache = {}

    def image(i):
        if i not in image_cache:
            im = (g.get("images") or [])[_index(i, len(g.get("images") or []), "image")]
            if "bufferView" in im:
                views = g.get("bufferViews") or []
                bv = views[_index(im["bufferView"], len(views), f"image {i}: bufferView")]
                buf = buffers[_index(bv.get("buffer"), len(buffers), f"image {i}: buffer")]
                off, n = bv.get("byteOffset", 0), bv.get("byteLength")
                _need(isinstance(off, int) and isinstance(n, int) and 0 <= off and 0 <= n and off + n <= len(buf),
                      f"image {i}: its bufferView does not fit the buffer")
                raw = buf[off:off + n]
            else:
                _need("uri" in im, f"image {i} has neither a bufferView nor a uri")
                raw = _uri_bytes(im["uri"], base_dir, f"image {i}")
            image_cache[i] = len(image_cache), decode_image(raw)
        return image_cache[i][0]

    textures, samplers = g.get("textures") or [], g.get("samplers") or []
    tex_image, tex_sampler = [], []
    for ti, tx in enumerate(textures):
        _need("source" in tx, f"texture {ti} has no source image (extension-only textures are not read)")
        tex_image.append(image(tx["source"]))
        s = samplers[_index(tx["sampler"], len(samplers), f"texture {ti}: sampler")] if "sampler" in tx else {}
        ws, wt = s.get("wrapS", 10497), s.get("wrapT", 10497)
        _need(ws in _WRAP and wt in _WRAP, f"texture {ti}: wrap modes {ws!r}, {wt!r}")
        tex_sampler.append([_WRAP[ws], _WRAP[wt], 1 if s.get("magFilter") == 9728 else 0])

    def tex_ref(info, what):
        if info is None:
            return -1
        _need(info.get("texCoord", 0) == 0, f"{what} uses texCoord {info.get('texCoord')}: only TEXCOORD_0 is read")
        return _index(info.get("index"), len(textures), what)

    mat_factor, mat_tex = [], []
    for mi, m in enumerate(g.get("materials") or []):
        pbr = m.get("pbrMetallicRoughness") or {}
        bc = [float(x) for x in pbr.get("baseColorFactor", [1.0, 1.0, 1.0, 1.0])]
        _need(len(bc) == 4, f"material {mi}: baseColorFactor needs 4 numbers")
        mat_factor.append(bc + [float(pbr.get("roughnessFactor", 1.0)), float(pbr.get("metallicFactor", 1.0))])
        mat_tex.append([tex_ref(pbr.get("baseColorTexture"), f"material {mi}: baseColorTexture"),
                        tex_ref(pbr.get("metallicRoughnessTexture"), f"material {mi}: metallicRoughnessTexture")])
    n_named = len(mat_factor)

    # ---- scene traversal
    nodes, meshes = g.get("nodes") or [], g.get("meshes") or []
    scenes = g.get("scenes") or []
    if scenes:
        roots = scenes[_index(g.get("scene", 0), len(scenes), "scene")].get("nodes") or []
    else:
        kids = {c for n in nodes for c in (n.get("children") or [])}
        roots = [i for i in range(len(nodes)) if i not in kids]
    out = {k: [] for k in ("v", "f", "vt", "color", "rm", "fm", "n")}
    state = {"V": 0, "default": False, "normals": True}

    def primitive(p, M, where):
        mode = p.get("mode", 4)
        if mode != 4:
            return                                                  # points, lines, strips and fans are not read
        attrs = p.get("attributes") or {}
        _need("POSITION" in attrs, f"{where}: no POSITION")
        pos, _ = _accessor(g, buffers, attrs["POSITION"], f"{where}: POSITION")
        _need(pos.dtype == np.dtype("<f4") and pos.shape[1] == 3, f"{where}: POSITION must be float VEC3")
        V = pos.shape[0]
        if "indices" in p:
            idx, _ = _accessor(g, buffers, p["indices"], f"{where}: indices")
            _need(idx.shape[1] == 1 and idx.dtype.kind == "u", f"{where}: indices must be unsigned scalars")
            idx = idx.reshape(-1).astype(np.int64)
        else:
            idx = np.arange(V, dtype=np.int64)
        _need(idx.shape[0] % 3 == 0, f"{where}: {idx.shape[0]} indices are no triangle list")
        _need(idx.size == 0 or int(idx.max()) < V, f"{where}: an index reaches past the {V} vertices")
        _need(state["V"] + V < 2 ** 31, "more than 2^31 vertices")
        faces = idx.reshape(-1, 3)
        identity = np.array_equal(M, np.eye(4))
        if not identity:
            pos = (pos.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)   # rounded once
            if np.linalg.det(M[:3, :3]) < 0:
                faces = faces[:, ::-1]                              # a mirror: keep the winding number's sign
        nrm = None
        if "NORMAL" in attrs:
            nrm, _ = _accessor(g, buffers, attrs["NORMAL"], f"{where}: NORMAL")
            _need(nrm.dtype == np.dtype("<f4") and nrm.shape == (V, 3), f"{where}: NORMAL must be float VEC3, one per vertex")
            if not identity:
                lin = M[:3, :3]
                _need(abs(np.linalg.det(lin)) > 0, f"{where}: a singular node transform")
                n64 = nrm.astype(np.float64) @ np.linalg.inv(lin)                       # (lin^-T n)^T
                ln = np.linalg.norm(n64, axis=1, keepdims=True)
                nrm = (n64 / np.where(ln > 0, ln, 1.0)).astype(np.float32)
        else:
            state["normals"] = False

        def attribute(name, width, fill):
            if name not in attrs:
                return np.full((V, width), fill, np.float32)
            a, norm = _accessor(g, buffers, attrs[name], f"{where}: {name}")
            _need(a.shape[0] == V, f"{where}: {name} has {a.shape[0]} entries for {V} vertices")
            a = _unit_float(a, norm, f"{where}: {name}")
            if name == "COLOR_0" and a.shape[1] == 3:
                a = np.concatenate([a, np.ones((V, 1), np.float32)], 1)
            _need(a.shape[1] == width, f"{where}: {name} has {a.shape[1]} components")
            return a
        if "material" in p:
            mat = _index(p["material"], n_named, f"{where}: material")
        else:
            mat, state["default"] = n_named, True
        out["v"].append(pos)
        out["f"].append(faces + state["V"])
        out["vt"].append(attribute("TEXCOORD_0", 2, 0.0))
        out["color"].append(attribute("COLOR_0", 4, 1.0))
        out["rm"].append(attribute("_ROUGHNESS_METALLIC", 2, 1.0))
        out["fm"].append(np.full(faces.shape[0], mat, np.int32))
        out["n"].append(nrm)
        state["V"] += V

    def visit(ni, parent, path_):
        _index(ni, len(nodes), "node")
        _need(ni not in path_, f"node {ni} is its own ancestor")
        node = nodes[ni]
        M = parent @ _node_matrix(node)
        if "mesh" in node:
            mesh = meshes[_index(node["mesh"], len(meshes), f"node {ni}: mesh")]
            for pi, p in enumerate(mesh.get("primitives") or []):
                primitive(p, M, f"mesh {node['mesh']} primitive {pi}")
        for c in node.get("children") or []:
            visit(c, M, path_ | {ni})

    for r in roots:
        visit(r, np.eye(4), frozenset())
    if state["default"]:
        mat_factor.append([1.0] * 6)
        mat_tex.append([-1, -1])
    if not mat_factor:                                              # no faces at all: the table still has one row
        mat_factor.append([1.0] * 6)
        mat_tex.append([-1, -1])

    def cat(key, width, dt):
        return np.concatenate(out[key]).astype(dt) if out[key] else np.zeros((0,) + width, dt)
    images = [None] * len(image_cache)
    for slot, img in image_cache.values():
        images[slot] = img
    normals = cat("n", (3,), np.float32) if state["normals"] and out["n"] else None
    return dict(v=cat("v", (3,), np.float32), f=cat("f", (3,), np.int32), vt=cat("vt", (2,), np.float32),
                color=cat("color", (4,), np.float32), rm=cat("rm", (2,), np.float32), face_material=cat("fm", (), np.int32),
                mat_factor=np.asarray(mat_factor, np.float32).reshape(-1, 6), mat_tex=np.asarray(mat_tex, np.int32).reshape(-1, 2),
                tex_image=np.asarray(tex_image, np.int32).reshape(-1), tex_sampler=np.asarray(tex_sampler, np.int32).reshape(-1, 3),
                images=images, normals=normals)


def read_glb(path: str, device=None) -> MaterialMesh:
    """A glTF 2.0 binary file -> `MaterialMesh` (CPU tensors, or on `device`).  What is read, and how:

    * the container: `.glb` version 2 with a JSON chunk and an optional BIN chunk; buffers and images may also come from `data:`
      URIs and from relative file URIs, resolved against the file's directory;
    * every node of the scene (`scene`, else scene 0, else every root node) is visited depth first; the hierarchy, `matrix` and
      translation / rotation / scale are composed in float64, positions are transformed in float64 and rounded once to float32,
      an identity transform leaves the stored float32 bits untouched, and a transform with a negative determinant reverses each
      face's vertex order, so that the winding number keeps its sign; all primitives are concatenated in traversal order (a mesh
      instanced by two nodes appears twice); normals are transformed by the inverse transpose and normalised, and are None
      unless every primitive has them;
    * only triangle lists (`mode` 4 or absent; other modes are skipped); indices u8, u16, u32 or absent; accessors honour
      `byteOffset` and `byteStride`; TEXCOORD_0, COLOR_0 (VEC3 gets alpha 1) and `_ROUGHNESS_METALLIC` accept float and
      normalised u8 / u16 (x / 255, x / 65535 in float32); sparse accessors raise NotImplementedError;
    * anything in `extensionsRequired` (Draco, meshopt, texture transform, ...) raises ValueError naming it; extensions that are
      only `extensionsUsed` are ignored;
    * materials: the metallic-roughness factors, base-colour and metallic-roughness textures with their samplers' wrap modes and
      magnification filter (glTF's defaults: REPEAT, and LINEAR here); a texture with `texCoord` != 0 raises; alpha and
      `alphaMode` are ignored (the geometry stays); normal, occlusion and emissive maps are not read; a primitive without a
      material gets glTF's default material (factors 1, no textures), the last row of the table;
    * images: 8-bit non-interlaced PNGs of colour type 0, 2, 3, 4, 6 through `decode_png` (stdlib); everything else (JPEG, 16-bit
      or interlaced PNG, ...) through Pillow where it imports, else ValueError.  Grey expands to RGB, a missing alpha is 255, the
      bytes are kept as stored (no sRGB decode); only images a texture uses are decoded;
    * every accessor, bufferView and chunk length is checked against the bytes present: a truncated or inconsistent file raises
      ValueError.

    Both layouts this project writes come back bit for bit: `TexturedMesh.write_glb` (v, f, vt, normals, both images) and
    `TriMesh.write_glb` (v, f, normals, color[:, :3] = albedo, rm = (roughness, metallic))."""
    try:
        parts = _read(path)
    except (KeyError, IndexError, TypeError, AttributeError, struct.error, OverflowError, RecursionError) as e:
        raise ValueError(f"{path}: malformed glTF ({type(e).__name__}: {e})") from None
    dev = device if device is not None else "cpu"
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return MaterialMesh(**{k: ([t(i) for i in x] if k == "images" else t(x)) for k, x in parts.items()})
