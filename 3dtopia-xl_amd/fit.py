"""Fit PrimX primitives to a mesh on MI355X - SURVEY.md section 8(f) row N7.

The reference never released this step: `PrimSDF._init_param` is an empty `pass` (models/primsdf.py:48-50).  What is built
here is the initialisation the 3DTopia-XL paper describes: sample candidate points uniformly on the surface, farthest-point-
sample N of them as primitive centres, set each scale to the distance to the nearest other centre, and fill each primitive's
S^3 payload with the mesh's signed distance, colour and material at `t_k + s_k * I`.  The short gradient refinement the paper
runs afterwards is `refine_primitives` (`refine=N` of `mesh_to_primitives` / `PrimSDF.from_mesh`): full-batch Adam steps on the
payload and, optionally, on scale and position, against the mesh's own field at a fixed seeded point set
(`primx_primsdf_query_backward`, csrc/primsdf.hip; `primx_adam_step`, csrc/rowops.hip).  The paper's hyper-parameters are not in
the reference tree: the defaults below are this project's choice, measured on the example torus (DESIGN.md "Refinement").

Kernels (csrc/meshfield.hip, rules in include/primx_hip.h "Primitive fitting"): `primx_mesh_field_query` (brute force over
the faces: exact point-triangle distance, generalized winding number, attributes at the closest point),
`primx_mesh_face_areas`, `primx_mesh_surface_points`, `primx_fps`; csrc/meshbvh.hip ("Mesh BVH"): `MeshBVH`, the same query
through a bounding volume hierarchy (`accel="bvh"`: the same dist, face and attributes bit for bit, the winding number by a
far-field expansion; `accel=None`, the default, is the brute-force call; `MeshBVH.raycast` and `MeshBVH.visibility` cast
watertight rays through the same tree - "Mesh rays" - and `sign="visibility"` takes inside / outside from them); csrc/material.hip ("Textured meshes"): `primx_material_sample`
(the glTF material of a `mesh.MaterialMesh` at the closest point).  Torch does the plumbing: the float64 inclusive sum of the
areas (on the host, where it is sequential and therefore reproducible to the bit), the seeded uniforms (a CPU generator, as the
sampler draws its noise), the normalisation and the assembly of `recon_param`.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops

QUERY_CHUNK = 256          # triangle records per LDS chunk of primx_mesh_field_query (MF_CHUNK of csrc/meshfield.hip)
RECORD_BYTES = 64
N_ATTR = 5                 # r, g, b, roughness, metallic
BVH_LEAF = 8               # faces per leaf of a MeshBVH (LEAF of csrc/meshbvh.hip)
BVH_NODE_BYTES = 96        # six float4 per node
BVH_MOMENT_BYTES = 128     # 16 float64 of build scratch per node
BVH_HEAD_BYTES = 256       # the index-check flag at 0; the vertices' box, the largest |coordinate| and delta (8 fp32) at 64
BVH_DELTA_SCALE = 2.0 ** -17   # the boxes are inflated by this times the largest |coordinate| (DESIGN.md "Mesh BVH")
BVH_BETA = 2.0             # a node farther than beta * its radius adds its far-field expansion to the winding number
ACCELS = (None, "bvh")


def _need_cuda(name, *tensors):
    for t in tensors:
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise RuntimeError(f"{name} needs HIP device tensors; there is no CPU path")


def _mesh_args(v, f):
    v, f = v.float().contiguous(), f.int().contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"v must be [V, 3] and f [F, 3], got {tuple(v.shape)} and {tuple(f.shape)}")
    if v.shape[0] == 0 or f.shape[0] == 0:
        raise ValueError("the mesh has no vertices or no faces")
    return v, f


def bvh_layout(F: int) -> dict:
    """Where a MeshBVH of F faces keeps what, in bytes from the start of its workspace (`layout` of csrc/meshbvh.hip; 'total' is
    what primx_mesh_bvh_workspace returns): 'recs' [F] 64-byte face records in sorted order, 'orig' [F] int32 (the face each one
    is), 'nodes' [2 L] of BVH_NODE_BYTES (node 0 unused, 1 the root, L + l leaf l), 'mom' [2 L] of 16 float64, 'part'."""
    up = lambda x: (x + 15) & ~15   # noqa: E731
    nleaf = (F + BVH_LEAF - 1) // BVH_LEAF
    L = 1
    while L < nleaf:
        L *= 2
    recs = BVH_HEAD_BYTES
    orig = recs + 64 * F
    nodes = orig + up(4 * F)
    mom = nodes + BVH_NODE_BYTES * 2 * L
    part = mom + BVH_MOMENT_BYTES * 2 * L
    return {"nleaf": nleaf, "L": L, "recs": recs, "orig": orig, "nodes": nodes, "mom": mom, "part": part, "total": part + 8192}


def morton_order(x: torch.Tensor) -> torch.Tensor:
    """The permutation that puts the points x [n, 3] in the order of their 30-bit Morton codes (1024 steps of the longest side of
    their bounding box): torch plumbing for `sort_points`, no host synchronisation."""
    lo = x.min(0).values
    ext = (x.max(0).values - lo).max()
    s = torch.where(ext > 0, 1024.0 / ext, torch.zeros_like(ext))
    q = ((x - lo) * s).clamp(0, 1023).nan_to_num(0.0).long()
    code = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
    for b in range(10):
        bit = (q >> b) & 1
        code |= (bit[:, 0] << (3 * b + 2)) | (bit[:, 1] << (3 * b + 1)) | (bit[:, 2] << (3 * b))
    return torch.sort(code, stable=True).indices


class MeshBVH:
    """The bounding volume hierarchy of a triangle mesh (include/primx_hip.h "Mesh BVH"): built once, here, and reusable for any
    number of `query`, `raycast` and `visibility` calls.  v [V, 3] float32, f [F, 3] int32 on a HIP device; face indices outside [0, V) raise (the one
    read-back of the tree: `query` has none and does not make the host wait).  The sort of the faces' Morton keys is torch's.
    `ws`: the `.ws` of a tree built earlier from the same v and f (a cached one): nothing is built or checked then."""

    def __init__(self, v: torch.Tensor, f: torch.Tensor, ws: Optional[torch.Tensor] = None):
        _need_cuda("MeshBVH", v, f, ws)
        self.v, self.f = _mesh_args(v, f)
        V, F, dev = self.v.shape[0], self.f.shape[0], self.v.device
        self.layout = bvh_layout(F)
        self._directions = {}                                    # K -> the Fibonacci sphere on the device (`visibility`)
        if ws is not None:
            if ws.dtype != torch.uint8 or ws.dim() != 1 or ws.numel() < self.layout["total"] or not ws.is_contiguous():
                raise ValueError(f"ws must be the {self.layout['total']} bytes of a MeshBVH of {F} faces")
            self.ws, self.order = ws, None
            return
        with torch.cuda.device(dev):
            lib = _lib.load()
            nbytes = _lib.C.c_int64(0)
            _lib.check(lib.primx_mesh_bvh_workspace(F, _lib.C.byref(nbytes)), "primx_mesh_bvh_workspace")
            assert nbytes.value == self.layout["total"], (nbytes.value, self.layout)
            self.ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
            keys = torch.empty(F, dtype=torch.int64, device=dev)
            vp, fp = ops._dev(self.v, "v", torch.float32), ops._dev(self.f, "f", torch.int32)
            _lib.check(lib.primx_mesh_bvh_build(vp, fp, V, F, None, keys.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                ops._stream()), "primx_mesh_bvh_build")
            self.order = torch.sort(keys, stable=True).indices.int().contiguous()
            _lib.check(lib.primx_mesh_bvh_build(vp, fp, V, F, self.order.data_ptr(), None, self.ws.data_ptr(), self.ws.numel(),
                                                ops._stream()), "primx_mesh_bvh_build")

    def matches(self, v: torch.Tensor, f: torch.Tensor) -> bool:
        """Whether this tree was built for a mesh of these shapes on this device (the contents are the caller's business)."""
        return v.shape[0] == self.v.shape[0] and f.shape[0] == self.f.shape[0] and v.device == self.v.device

    def query(self, x: torch.Tensor, attr: Optional[torch.Tensor] = None, beta: float = BVH_BETA, sort_points: bool = False):
        """x [n, 3], attr [V, C] or None -> (dist [n], face [n] int32, wn [n], out_attr [n, C] or None): primx_mesh_bvh_query.
        `sort_points` runs the points in Morton order and scatters the results back (for incoherent point sets; every point's
        result is the same either way)."""
        _need_cuda("MeshBVH.query", x, attr)
        x = x.float().contiguous()
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError(f"x must be [n, 3], got {tuple(x.shape)}")
        if not float(beta) >= 0:
            raise ValueError(f"beta must be at least 0, got {beta}")
        n, F, dev = x.shape[0], self.f.shape[0], self.v.device
        C = 0 if attr is None else attr.shape[1]
        if attr is not None:
            attr = attr.float().contiguous()
            if attr.shape[0] != self.v.shape[0]:
                raise ValueError("attr must have one row per vertex")
        with torch.cuda.device(dev):
            perm = morton_order(x) if sort_points and n > 1 else None
            xs = x if perm is None else x[perm].contiguous()
            dist = torch.empty(n, dtype=torch.float32, device=dev)
            face = torch.empty(n, dtype=torch.int32, device=dev)
            wn = torch.empty(n, dtype=torch.float32, device=dev)
            out = torch.empty(n, C, dtype=torch.float32, device=dev) if C else None
            _lib.check(_lib.load().primx_mesh_bvh_query(
                ops._dev(xs, "x", torch.float32), n, ops._dev(self.f, "f", torch.int32), F,
                ops._dev(attr, "attr", torch.float32) if C else None, C, self.ws.data_ptr(), self.ws.numel(), float(beta),
                dist.data_ptr(), face.data_ptr(), wn.data_ptr(), out.data_ptr() if C else None, ops._stream()),
                "primx_mesh_bvh_query")
            if perm is not None:
                back = lambda t: torch.empty_like(t).index_copy_(0, perm, t)   # noqa: E731
                dist, face, wn, out = back(dist), back(face), back(wn), None if out is None else back(out)
        return dist, face, wn, out

    def _rays(self, name, *pairs):
        out = []
        for label, t in pairs:
            t = t.float().contiguous()
            if t.dim() != 2 or t.shape[1] != 3:
                raise ValueError(f"{name}: {label} must be [n, 3], got {tuple(t.shape)}")
            out.append(t)
        return out

    def raycast(self, origins: torch.Tensor, dirs: torch.Tensor, tmin: float = 0.0, tmax: float = float("inf"),
                any_hit: bool = False, attr: Optional[torch.Tensor] = None):
        """origins, dirs [n, 3] -> (t [n], face [n] int32, bary [n, 2], out_attr [n, C] or None): primx_mesh_bvh_raycast, the
        closest hit of each ray o + t d with t in [tmin, tmax] (include/primx_hip.h "Mesh rays": the watertight test of Woop et
        al. 2013, two-sided; d need not be normalised, t is in units of its length).  A miss - also a zero or non-finite ray -
        has t = inf, face = -1 and bary = 0.  hit = a + bary[0] (b - a) + bary[1] (c - a) on face `face` (the lowest face index
        among equal t).  `any_hit` stops at the first hit met: only face >= 0 means something then.  `attr` [V, C] is
        interpolated here, in torch, as (a u + b v) + c w with u = (1 - v) - w, and is 0 on a miss.  One launch, nothing read
        back."""
        _need_cuda("MeshBVH.raycast", origins, dirs, attr)
        o, d = self._rays("MeshBVH.raycast", ("origins", origins), ("dirs", dirs))
        if o.shape != d.shape:
            raise ValueError(f"origins and dirs must have the same shape, got {tuple(o.shape)} and {tuple(d.shape)}")
        if not float(tmin) <= float(tmax):
            raise ValueError(f"tmin must not exceed tmax, got {tmin} and {tmax}")
        if attr is not None:
            attr = attr.float().contiguous()
            if attr.dim() != 2 or attr.shape[0] != self.v.shape[0]:
                raise ValueError("attr must have one row per vertex")
        n, F, dev = o.shape[0], self.f.shape[0], self.v.device
        with torch.cuda.device(dev):
            t = torch.empty(n, dtype=torch.float32, device=dev)
            face = torch.empty(n, dtype=torch.int32, device=dev)
            bary = torch.empty(n, 2, dtype=torch.float32, device=dev)
            _lib.check(_lib.load().primx_mesh_bvh_raycast(
                ops._dev(o, "origins", torch.float32) if n else None, ops._dev(d, "dirs", torch.float32) if n else None, n,
                float(tmin), float(tmax), int(bool(any_hit)), ops._dev(self.f, "f", torch.int32), F, self.ws.data_ptr(),
                self.ws.numel(), t.data_ptr() if n else None, face.data_ptr() if n else None, bary.data_ptr() if n else None,
                ops._stream()), "primx_mesh_bvh_raycast")
            out = None
            if attr is not None:
                hit = face >= 0
                fa = self.f[face.clamp(min=0).long()].long()
                v, w = bary[:, 0:1], bary[:, 1:2]
                u = (1.0 - v) - w
                out = (attr[fa[:, 0]] * u + attr[fa[:, 1]] * v) + attr[fa[:, 2]] * w
                out = torch.where(hit[:, None], out, torch.zeros_like(out))
        return t, face, bary, out

    def visibility(self, x: torch.Tensor, directions=64, tmin: float = 0.0, limit: int = 0) -> torch.Tensor:
        """x [n, 3] -> int32 [n]: how many of the rays from x along `directions` reach infinity without a hit
        (primx_mesh_bvh_visibility; each ray stops at its first hit).  `directions`: an int K for the Fibonacci sphere of
        `mesh.occlusion_directions(K)` (uploaded once per tree and K), or a tensor [D, 3] taken as given.  `limit` > 0 stops a
        point once that many rays have escaped, so the count saturates there: a point outside usually costs one ray.  One
        launch, nothing read back."""
        _need_cuda("MeshBVH.visibility", x)
        x, = self._rays("MeshBVH.visibility", ("x", x))
        dev = self.v.device
        if isinstance(directions, torch.Tensor):
            _need_cuda("MeshBVH.visibility", directions)
            dirs, = self._rays("MeshBVH.visibility", ("directions", directions))
        else:
            K = int(directions)
            if K not in self._directions:
                from . import mesh
                self._directions[K] = mesh.occlusion_directions(K).to(dev).contiguous()
            dirs = self._directions[K]
        D, limit = dirs.shape[0], int(limit)
        if D < 1 or limit < 0:
            raise ValueError(f"visibility needs at least one direction and limit >= 0, got {D} and {limit}")
        if not float(tmin) <= float("inf"):
            raise ValueError(f"tmin must be a number, got {tmin}")
        n, F = x.shape[0], self.f.shape[0]
        with torch.cuda.device(dev):
            esc = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().primx_mesh_bvh_visibility(
                ops._dev(x, "x", torch.float32) if n else None, n, ops._dev(dirs, "directions", torch.float32), D, float(tmin), limit,
                ops._dev(self.f, "f", torch.int32), F, self.ws.data_ptr(), self.ws.numel(), esc.data_ptr() if n else None,
                ops._stream()), "primx_mesh_bvh_visibility")
        return esc


SIGNS = ("winding", "visibility")


def _check_sign(sign, accel):
    if sign not in SIGNS:
        raise ValueError(f"sign must be one of {SIGNS}, got {sign!r}")
    if sign == "visibility" and accel != "bvh":
        raise ValueError('sign="visibility" casts rays through the tree: it needs accel="bvh"')
    return sign


def _check_accel(accel):
    if accel not in ACCELS:
        raise ValueError(f"accel must be one of {ACCELS}, got {accel!r}")
    return accel


@ops.on_input_device
def mesh_field_query(x: torch.Tensor, v: torch.Tensor, f: torch.Tensor, attr: Optional[torch.Tensor] = None,
                     bvh: Optional[MeshBVH] = None, beta: float = BVH_BETA, sort_points: bool = False):
    """x [n, 3], v [V, 3] float32, f [F, 3] int32, attr [V, C] or None -> (dist [n], face [n] int32, wn [n], out_attr [n, C]
    or None): primx_mesh_field_query.  Face indices outside [0, V) raise.  With `bvh` (a `MeshBVH` of the same v and f) the
    tree answers instead (`MeshBVH.query`: the same dist, face and out_attr, wn approximated under `beta`)."""
    _need_cuda("mesh_field_query", x, v, f, attr)
    if bvh is not None:
        if not isinstance(bvh, MeshBVH) or not bvh.matches(v, f):
            raise ValueError("bvh must be a MeshBVH built from the same v and f")
        return bvh.query(x, attr, beta, sort_points)
    v, f = _mesh_args(v, f)
    x = x.float().contiguous()
    n, F, dev = x.shape[0], f.shape[0], x.device
    C = 0 if attr is None else attr.shape[1]
    if attr is not None:
        attr = attr.float().contiguous()
        if attr.shape[0] != v.shape[0]:
            raise ValueError("attr must have one row per vertex")
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    wn = torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.empty(n, C, dtype=torch.float32, device=dev) if C else None
    ws = torch.empty(64 + RECORD_BYTES * F, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().primx_mesh_field_query(
        ops._dev(x, "x", torch.float32), n, ops._dev(v, "v", torch.float32), ops._dev(f, "f", torch.int32), v.shape[0], F,
        ops._dev(attr, "attr", torch.float32) if C else None, C, ws.data_ptr(), ws.numel(), dist.data_ptr(), face.data_ptr(),
        wn.data_ptr(), out.data_ptr() if C else None, ops._stream()), "primx_mesh_field_query")
    return dist, face, wn, out


@ops.on_input_device
def material_sample(uv: torch.Tensor, vattr: Optional[torch.Tensor], face: torch.Tensor, face_material: torch.Tensor,
                    mat_factor: torch.Tensor, mat_tex: torch.Tensor, tex_desc: torch.Tensor, texels: torch.Tensor) -> torch.Tensor:
    """uv [n, 2], vattr [n, 6] = (color rgba, rm) or None (all ones), face [n] int32, face_material [F] int32, mat_factor [M, 6],
    mat_tex [M, 2] int32, tex_desc [T, 4] int64, texels [n_texels, 4] uint8 -> [n, 5] float32 (r, g, b, roughness, metallic), not
    clipped: primx_material_sample (the rules: include/primx_hip.h "Textured meshes").  Indices outside their tables raise."""
    _need_cuda("material_sample", uv, vattr, face, face_material, mat_factor, mat_tex, tex_desc, texels)
    uv, face = uv.float().contiguous(), face.int().contiguous()
    n, dev = uv.shape[0], uv.device
    if uv.dim() != 2 or uv.shape[1] != 2 or face.shape != (n,):
        raise ValueError(f"uv must be [n, 2] and face [n], got {tuple(uv.shape)} and {tuple(face.shape)}")
    if vattr is not None:
        vattr = vattr.float().contiguous()
        if tuple(vattr.shape) != (n, 6):
            raise ValueError(f"vattr must be [n, 6] (color r, g, b, a, rm x, y), got {tuple(vattr.shape)}")
    face_material, mat_tex = face_material.int().contiguous(), mat_tex.int().contiguous()
    mat_factor, tex_desc, texels = mat_factor.float().contiguous(), tex_desc.long().contiguous(), texels.contiguous()
    F, M, T = face_material.shape[0], mat_factor.shape[0], tex_desc.shape[0]
    if face_material.dim() != 1 or tuple(mat_factor.shape) != (M, 6) or tuple(mat_tex.shape) != (M, 2) or \
            tuple(tex_desc.shape) != (T, 4) or texels.dtype != torch.uint8 or texels.dim() != 2 or texels.shape[1] != 4:
        raise ValueError("face_material must be [F], mat_factor [M, 6], mat_tex [M, 2], tex_desc [T, 4] and texels uint8 [n, 4]")
    out = torch.empty(n, N_ATTR, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().primx_material_sample(
        ops._dev(uv, "uv", torch.float32) if n else None, ops._dev(vattr, "vattr", torch.float32) if vattr is not None and n else None,
        ops._dev(face, "face", torch.int32) if n else None, n, ops._dev(face_material, "face_material", torch.int32), F,
        ops._dev(mat_factor, "mat_factor", torch.float32), ops._dev(mat_tex, "mat_tex", torch.int32), M,
        ops._dev(tex_desc, "tex_desc", torch.int64) if T else None, T, texels.data_ptr() if texels.shape[0] else None,
        texels.shape[0], status.data_ptr(), out.data_ptr() if n else None, ops._stream()), "primx_material_sample")
    return out


class MeshField:
    """The signed distance, colour and material functions of a triangle mesh: `query(x)` -> {'sdf' [n, 1], 'tex' [n, 3],
    'mat' [n, 2], 'face' [n], 'wn' [n]}.  sdf = the distance to the closest triangle outside and its negative inside, where
    inside means |winding number| >= 0.5 (negative inside, as PrimSDF stores it); tex / mat are the vertex attributes at the
    closest point, clipped to [0, 1] (zeros without attributes).

    With `material` (a `mesh.MaterialMesh`; its v and f are not used, `v` and `f` are) tex / mat are the mesh's glTF material at
    the closest point instead: the field query interpolates [vt | color | rm] (C = 8) and `primx_material_sample` evaluates
    factors and textures there.  The tables and the texel blob are uploaded once, here.

    `accel="bvh"` builds a `MeshBVH` here and answers every query through it: sdf magnitude, face, tex and mat as without it, bit
    for bit; the sign from the winding number approximated under `beta`.  `accel=None` is the brute-force query.

    `sign="visibility"` (needs `accel="bvh"`) takes the sign from rays instead of the winding number, for meshes whose faces are
    not oriented consistently (flipped faces, two-sided sheets, mirrored parts), where |wn| >= 0.5 fails outright: a point is
    outside iff at least `min_escapes` of `sign_directions` fixed directions (`MeshBVH.visibility`) reach infinity without
    hitting the mesh, sdf = dist there and -dist elsewhere; the dict gains 'escapes' (the count, saturated at `min_escapes`) and
    keeps 'wn'.  What the rule does not do: an open sheet is outside everywhere, so its field is an unsigned distance; a deep
    pocket narrower than the direction set resolves may count as inside; `min_escapes` > 1 closes pinholes in the surface at
    the price of more such pockets.  The defaults (64 directions, 1 escape) are this project's choice and unmeasured on real
    assets.  `sign="winding"`, the default, is the rule above and calls no ray kernel."""

    def __init__(self, v: torch.Tensor, f: torch.Tensor, attr: Optional[torch.Tensor] = None, material=None, accel=None,
                 beta: float = BVH_BETA, sort_points: bool = False, sign: str = "winding", sign_directions=64,
                 min_escapes: int = 1):
        _need_cuda("mesh_field", v, f, attr)
        self.v, self.f = _mesh_args(v, f)
        self.accel, self.beta, self.sort_points = _check_accel(accel), float(beta), bool(sort_points)
        self.sign, self.sign_directions, self.min_escapes = _check_sign(sign, accel), sign_directions, int(min_escapes)
        if self.min_escapes < 1:
            raise ValueError(f"min_escapes must be at least 1, got {min_escapes}")
        self.bvh = MeshBVH(self.v, self.f) if accel == "bvh" else None      # built once, for every chunk and refinement step
        self.material = None
        if material is not None:
            if attr is not None:
                raise ValueError("give attr or material, not both")
            dev = self.v.device
            attr = material.vertex_attr().to(dev)
            if attr.shape[0] != self.v.shape[0] or material.face_material.shape[0] != self.f.shape[0]:
                raise ValueError("the material needs one row of vt / color / rm per vertex and one face_material per face")
            desc, texels = material.texture_tables()
            self.material = tuple(t.to(dev).contiguous() for t in (material.face_material.int(), material.mat_factor.float(),
                                                                   material.mat_tex.int(), desc, texels))
            self.attr = attr.float().contiguous()
            return
        if attr is not None and tuple(attr.shape) != (self.v.shape[0], N_ATTR):
            raise ValueError(f"attr must be [V, {N_ATTR}] (r, g, b, roughness, metallic), got {tuple(attr.shape)}")
        self.attr = None if attr is None else attr.float().contiguous()

    def query(self, x: torch.Tensor) -> dict:
        if self.bvh is None:
            dist, face, wn, a = mesh_field_query(x, self.v, self.f, self.attr)
        else:
            dist, face, wn, a = self.bvh.query(x, self.attr, self.beta, self.sort_points)
        escapes = None
        if self.sign == "visibility":
            escapes = self.bvh.visibility(x, self.sign_directions, limit=self.min_escapes)
            sdf = torch.where(escapes >= self.min_escapes, dist, -dist)[:, None]
        else:
            sdf = torch.where(wn.abs() >= 0.5, -dist, dist)[:, None]
        if self.material is not None:
            a = material_sample(a[:, 0:2], a[:, 2:8], face, *self.material)
        if a is None:
            a = torch.zeros(x.shape[0], N_ATTR, dtype=torch.float32, device=dist.device)
        a = a.clip(0, 1)
        out = {"sdf": sdf, "tex": a[:, 0:3], "mat": a[:, 3:5], "face": face, "wn": wn}
        if escapes is not None:
            out["escapes"] = escapes
        return out

    __call__ = query


def mesh_field(v: torch.Tensor, f: torch.Tensor, attr: Optional[torch.Tensor] = None, material=None, accel=None,
               beta: float = BVH_BETA, sign: str = "winding", sign_directions=64, min_escapes: int = 1) -> MeshField:
    return MeshField(v, f, attr, material, accel=accel, beta=beta, sign=sign, sign_directions=sign_directions,
                     min_escapes=min_escapes)


@ops.on_input_device
def face_areas(v: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """float64 [F]: primx_mesh_face_areas."""
    _need_cuda("face_areas", v, f)
    v, f = _mesh_args(v, f)
    area = torch.empty(f.shape[0], dtype=torch.float64, device=v.device)
    status = torch.empty(1, dtype=torch.int32, device=v.device)
    _lib.check(_lib.load().primx_mesh_face_areas(ops._dev(v, "v", torch.float32), ops._dev(f, "f", torch.int32), v.shape[0],
                                                 f.shape[0], area.data_ptr(), status.data_ptr(), ops._stream()),
               "primx_mesh_face_areas")
    return area


def area_cdf(area: torch.Tensor) -> torch.Tensor:
    """The inclusive float64 sum, taken on the host: sequential, so the same bits on every machine (a device scan adds in an
    order of its own)."""
    return torch.cumsum(area.double().cpu(), 0).to(area.device)


def surface_uniforms(n: int, seed: int = 0) -> torch.Tensor:
    """[n, 3] float32 in [0, 1) from a seeded CPU generator (the same numbers on every device)."""
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


@ops.on_input_device
def surface_points(v: torch.Tensor, f: torch.Tensor, cdf: torch.Tensor, u: torch.Tensor):
    """cdf [F] float64 (inclusive), u [N, 3] in [0, 1) -> (pts [N, 3] float32, face [N] int32): primx_mesh_surface_points."""
    _need_cuda("surface_points", v, f, cdf, u)
    v, f = _mesh_args(v, f)
    cdf, u = cdf.double().contiguous(), u.float().contiguous()
    if cdf.shape != (f.shape[0],) or u.dim() != 2 or u.shape[1] != 3:
        raise ValueError("cdf must be [F] and u [N, 3]")
    N = u.shape[0]
    pts = torch.empty(N, 3, dtype=torch.float32, device=v.device)
    face = torch.empty(N, dtype=torch.int32, device=v.device)
    status = torch.empty(1, dtype=torch.int32, device=v.device)
    _lib.check(_lib.load().primx_mesh_surface_points(
        ops._dev(v, "v", torch.float32), ops._dev(f, "f", torch.int32), v.shape[0], f.shape[0], ops._dev(cdf, "cdf", torch.float64),
        ops._dev(u, "u", torch.float32), N, pts.data_ptr(), face.data_ptr(), status.data_ptr(), ops._stream()),
        "primx_mesh_surface_points")
    return pts, face


@ops.on_input_device
def fps(pts: torch.Tensor, K: int, start: int = 0):
    """pts [N, 3] -> (idx [K] int32, nn [K] float32): primx_fps (ties to the lowest index; nn = the distance from each chosen
    centre to the nearest other one, 0 when K == 1)."""
    _need_cuda("fps", pts)
    pts = pts.float().contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"pts must be [N, 3], got {tuple(pts.shape)}")
    N, dev = pts.shape[0], pts.device
    idx = torch.empty(K, dtype=torch.int32, device=dev)
    nn = torch.empty(K, dtype=torch.float32, device=dev)
    ws = torch.empty(((4 * N + 7) & ~7) + 4096, dtype=torch.uint8, device=dev)
    _lib.check(_lib.load().primx_fps(ops._dev(pts, "pts", torch.float32), N, K, start, ws.data_ptr(), ws.numel(),
                                     idx.data_ptr(), nn.data_ptr(), ops._stream()), "primx_fps")
    return idx, nn


def normalize_vertices(v: torch.Tensor, extent: float = 0.9):
    """fp32: the bounding box's centre to the origin, its longest half side to `extent` -> (v', centre [3], scale).  The
    value 0.9 is this project's choice (PrimSDF's domain is [-1, 1]^3 and the outermost primitives reach past their
    centres); the reference's own normalisation of its training meshes is not in its tree."""
    lo, hi = v.min(0).values, v.max(0).values
    c = (lo + hi) * 0.5
    half = float(((hi - lo) * 0.5).max())
    if not half > 0:
        raise ValueError("the mesh has no extent")
    s = torch.tensor(extent / half, dtype=torch.float32, device=v.device)     # rounded to fp32 once, on the host
    return (v - c) * s, c, s


def _local_grid(S: int, dev) -> torch.Tensor:
    xx = torch.linspace(-1, 1, S)                                             # PrimSDF's own table (models/primsdf.py:35-41)
    mx, my, mz = torch.meshgrid(xx, xx, xx, indexing="ij")
    return torch.stack((mz, my, mx), dim=-1).reshape(-1, 3).to(dev)


def _mesh_parts(mesh, dev):
    """-> (v, f, attr [V, 5] or None, material or None): a `mesh.MaterialMesh` keeps its material, everything else today's attr."""
    t = lambda a: torch.as_tensor(a).to(dev)   # noqa: E731
    if hasattr(mesh, "face_material"):
        return t(mesh.v).float(), t(mesh.f).int(), None, mesh
    if isinstance(mesh, (tuple, list)):
        v, f, albedo, rough, metal = mesh
    else:
        v, f, albedo, rough, metal = mesh.v, mesh.f, mesh.albedo, mesh.roughness, mesh.metallic
    v, f = t(v).float(), t(f).int()
    attr = torch.cat([t(albedo).float().reshape(-1, 3), t(rough).float().reshape(-1, 1), t(metal).float().reshape(-1, 1)], 1)
    return v, f, attr.contiguous(), None


REFINE_SCALE_FLOOR = 1e-4  # the scale is clamped to this after every step (fitted scales are positive; 0 would cover nothing)


def refine_points(srt: torch.Tensor, samples_per_prim: int, seed: int = 0) -> torch.Tensor:
    """[P * samples_per_prim, 3] fp32: pos + scale * U(-1, 1)^3 per primitive, the uniforms from a seeded CPU generator (the same
    numbers on every device), the product and the sum as two fp32 operations."""
    P = srt.shape[0]
    u = torch.rand(P, int(samples_per_prim), 3, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32) * 2 - 1
    u = u.to(srt.device)
    return (srt[:, None, 1:4] + srt[:, None, 0:1] * u).reshape(-1, 3).contiguous()


def refine_primitives(recon: torch.Tensor, field, steps: int, lr: float = 1e-3, samples_per_prim: int = 256, seed: int = 0,
                      refine_srt: bool = False, weights=(1.0, 1.0, 1.0), lr_srt: Optional[float] = None, chunk: int = 1 << 20,
                      accel=None, beta: float = BVH_BETA, sign: str = "winding", sign_directions=64, min_escapes: int = 1):
    """`steps` full-batch Adam steps on recon [P, 4 + 6 S^3] (fp32, HIP device) against `field.query` (a `MeshField`, or anything
    returning {'sdf' [n, 1], 'tex' [n, 3], 'mat' [n, 2]}) -> (recon', info).  `recon` itself is not modified.

    The training set is fixed: `refine_points(recon[:, :4], samples_per_prim, seed)`, taken from the initial srt, with targets
    from one `field.query` (the only host synchronisation here is that query's own; the loop has none).  Per step: the
    training-mode query, loss = sum(diff^2 * coef / 2) with coef = 2 w / (n * channels) per group (= w_sdf mse(sdf) +
    w_tex mse(tex) + w_mat mse(mat), on the clipped outputs), `primx_primsdf_query_backward` on gout = diff * coef, then
    `primx_adam_step` (betas 0.9 / 0.999, eps 1e-8) on the payload with `lr` and, if `refine_srt`, on srt with `lr_srt`
    (default lr / 100: an Adam step moves every element by about its rate, and a centre that drifts by a fraction of a voxel
    without need costs more than the payload gains), after which the scale is clamped to
    REFINE_SCALE_FLOOR.  `info`: 'loss' (the per-step losses BEFORE each step, read back once at the end), 'points',
    'target'.  The gradient sums are atomic: the last bits differ from run to run.

    `field` may also be a mesh (anything `mesh_to_primitives` takes, already in the primitives' frame): the field is then built
    here, with `accel`, `beta`, `sign`, `sign_directions` and `min_escapes` as `MeshField` takes them.  A field that is given
    keeps its own."""
    from . import primsdf
    _need_cuda("refine_primitives", recon)
    _check_accel(accel)
    if not hasattr(field, "query"):
        v, f, attr, material = _mesh_parts(field, recon.device)
        field = MeshField(v, f, attr, material, accel=accel, beta=beta, sign=sign, sign_directions=sign_directions,
                          min_escapes=min_escapes)
    if recon.dim() != 2 or recon.dtype != torch.float32:
        raise ValueError("recon must be fp32 [P, 4 + 6 S^3]")
    P = recon.shape[0]
    S = round(((recon.shape[1] - 4) / 6) ** (1.0 / 3.0))
    if P == 0 or S < 2 or 4 + 6 * S ** 3 != recon.shape[1]:
        raise ValueError(f"recon must be [P, 4 + 6 S^3] with P > 0 and S >= 2, got {tuple(recon.shape)}")
    steps = int(steps)
    if steps < 0 or samples_per_prim < 1:
        raise ValueError("steps must be >= 0 and samples_per_prim >= 1")
    lr_srt = 0.01 * lr if lr_srt is None else lr_srt
    dev = recon.device
    with torch.cuda.device(dev), torch.no_grad():
        srt, feat = recon[:, :4].clone().contiguous(), recon[:, 4:].clone().contiguous()
        pts = refine_points(srt, samples_per_prim, seed)
        n = pts.shape[0]
        parts = [field.query(pts[lo:lo + chunk]) for lo in range(0, n, chunk)]
        target = torch.cat([torch.cat([q["sdf"], q["tex"], q["mat"]], 1) for q in parts]).float().contiguous()
        w_sdf, w_tex, w_mat = (float(w) for w in weights)
        coef = torch.tensor([2 * w_sdf / n] + [2 * w_tex / (3 * n)] * 3 + [2 * w_mat / (2 * n)] * 2, dtype=torch.float32).to(dev)
        half_coef = coef * 0.5
        lin = torch.linspace(-1, 1, S).to(dev)
        losses = torch.zeros(max(steps, 1), dtype=torch.float32, device=dev)
        gf, mf, vf = (torch.zeros_like(feat) for _ in range(3))
        gs, ms, vs = (torch.zeros_like(srt) for _ in range(3)) if refine_srt else (None, None, None)
        for t in range(1, steps + 1):
            diff = primsdf._query_train(pts, srt, feat, lin, S) - target
            losses[t - 1] = (diff * diff * half_coef).sum()
            primsdf.query_backward(pts, srt, feat, diff * coef, S, gsrt=gs, gfeat=gf, want_srt=refine_srt)
            ops.adam_step(feat, gf, mf, vf, t, lr, zero_grad=True)
            if refine_srt:
                ops.adam_step(srt, gs, ms, vs, t, lr_srt, zero_grad=True)
                srt[:, 0].clamp_(min=REFINE_SCALE_FLOOR)
        out = torch.cat([srt, feat], 1).contiguous()
        loss = losses[:steps].cpu().tolist()                                  # the one read-back, after the loop
    return out, {"loss": loss, "points": pts, "target": target, "steps": steps}


def mesh_to_primitives(mesh, num_prims: int = 2048, prim_shape: int = 8, candidates: Optional[int] = None, seed: int = 0,
                       normalize: bool = True, extent: float = 0.9, device=None, chunk: int = 1 << 20, refine: int = 0,
                       refine_kw: Optional[dict] = None, accel=None, beta: float = BVH_BETA, sign: str = "winding",
                       sign_directions=64, min_escapes: int = 1):
    """mesh: a `mesh.TriMesh`, (v, f, albedo [V, 3], roughness [V], metallic [V]) or a `mesh.MaterialMesh` (e.g. from
    `mesh.read_glb`: colour and material come from its textures and factors) -> (recon_param [P, 4 + 6 S^3], info).

    `candidates` (default 32 P) surface samples drawn with `seed`; P of them by farthest point sampling from candidate 0;
    scale = distance to the nearest other centre; payload in `PrimSDF.feat_param`'s layout [sdf | rgb | roughness, metallic],
    each [z][y][x], evaluated at pos + scale * local_grid; colours and materials clipped to [0, 1], the SDF raw
    (`primitives_to_latents` applies the x5).  `normalize`: see `normalize_vertices`.  `info` has the normalisation
    (`center`, `scale`: v' = (v - center) * scale), the candidates (`candidates`, `candidate_face`) and the chosen ones (`idx`).
    `refine=N` > 0 follows the initialisation with N steps of `refine_primitives(recon, field, N, **refine_kw)` against the
    normalised mesh's field (`info['refine']` is its info); 0 is the initialisation alone.  `accel="bvh"` answers the payload's
    and the refinement's field queries through one `MeshBVH` of the normalised mesh (`MeshField(accel=, beta=)`).
    `sign="visibility"` (with `accel="bvh"`; `sign_directions`, `min_escapes`) takes inside / outside from rays through that tree
    instead of the winding number, for meshes without a consistent orientation - `MeshField` says what the rule does and does not
    do; the refinement runs against the same field."""
    _check_accel(accel)
    _check_sign(sign, accel)
    if device is None:
        v0 = mesh[0] if isinstance(mesh, (tuple, list)) else mesh.v
        device = v0.device if isinstance(v0, torch.Tensor) and v0.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    P, S = int(num_prims), int(prim_shape)
    N = int(candidates) if candidates is not None else 32 * P
    if not 1 <= P <= N:
        raise ValueError(f"num_prims must lie in 1 .. candidates (got {P} of {N})")
    with torch.cuda.device(dev), torch.no_grad():
        v, f, attr, material = _mesh_parts(mesh, dev)
        v, f = _mesh_args(v, f)
        center, scale = torch.tensor([0.0, 0.0, 0.0], device=dev), torch.tensor(1.0, device=dev)
        if normalize:
            v, center, scale = normalize_vertices(v, extent)
        cdf = area_cdf(face_areas(v, f))
        cand, cface = surface_points(v, f, cdf, surface_uniforms(N, seed).to(dev))
        idx, nn = fps(cand, P, 0)
        pos = cand[idx.long()]
        x = (pos[:, None, :] + nn[:, None, None] * _local_grid(S, dev)[None]).reshape(-1, 3)
        field = MeshField(v, f, attr, material, accel=accel, beta=beta, sign=sign, sign_directions=sign_directions,
                          min_escapes=min_escapes)
        parts = [field.query(x[lo:lo + chunk]) for lo in range(0, x.shape[0], chunk)]
        sdf = torch.cat([q["sdf"] for q in parts]).reshape(P, S ** 3)
        a = torch.cat([torch.cat([q["tex"], q["mat"]], 1) for q in parts]).reshape(P, S ** 3, N_ATTR)
        recon = torch.cat([nn[:, None], pos, sdf, a.transpose(1, 2).reshape(P, -1)], 1).contiguous()
        rinfo = None
        if int(refine) > 0:
            recon, rinfo = refine_primitives(recon, field, int(refine), **{"chunk": chunk, **(refine_kw or {})})
    info = {"center": center, "scale": scale, "v": v, "f": f, "attr": field.attr if material is not None else attr, "candidates": cand, "candidate_face": cface, "idx": idx}
    if rinfo is not None:
        info["refine"] = rinfo
    return recon, info


def primsdf_from_mesh(cls, mesh, num_prims: int = 2048, prim_shape: int = 8, return_info: bool = False, **kw):
    """`PrimSDF.from_mesh`: a module in eval mode on the mesh's device holding `mesh_to_primitives(mesh, ...)`, ready for
    `query`, `mesh.extract_mesh` and `pipeline.primitives_to_latents` (through `recon_param`).  `refine=N` (in `kw`) refines."""
    recon, info = mesh_to_primitives(mesh, num_prims=num_prims, prim_shape=prim_shape, **kw)
    m = cls(num_prims=recon.shape[0], dim_feat=6, prim_shape=prim_shape)
    m.srt_param = torch.nn.Parameter(recon[:, :4].contiguous(), requires_grad=False)
    m.feat_param = torch.nn.Parameter(recon[:, 4:].contiguous(), requires_grad=False)
    m = m.to(recon.device).eval()
    return (m, info) if return_info else m
