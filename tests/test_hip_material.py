"""Textured meshes on the MI355X (csrc/material.hip, fit.py, gltf.py) against the numpy restatement tests/material_numpy.py.

`primx_material_sample` is compared with the float32 restatement bit for bit, fed the same uv / vattr / face arrays.  At field level
(`MeshField(..., material=)`: the brute-force closest-point query, then the sampler) the attributes are compared with the float64
restatement evaluated on the face the GPU chose, within 4 x the error of the float32 restatement against float64 on that same face
assignment (the margin covers a different region choice and rounding of the interpolation weights in a correct fp32 query, as in
tests/test_hip_meshfield.py); LINEAR only, no point left out.  A `MaterialMesh` without textures gives the `TriMesh` path's bits.
Figures are printed before they are asserted; the ones seen are recorded in DESIGN.md "Textured meshes".

The module imports without a GPU: it registers its stream-order cases in the table of tests/test_hip_streams.py at import (that
file stays as it is) and runs them here, like tests/test_hip_raymarch_grad.py does.
"""
import os

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import material_numpy as MN
from tests import meshfield_numpy as MF
from tests import streamorder as so
from tests import test_hip_streams as TS
from tests.test_hip_meshfield import NS, _points
from tests.test_hip_primsdf_grad import E  # noqa: F401  (one side stream of its own, destroyed at teardown: see that module)
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WRAPS = (MN.CLAMP, MN.REPEAT, MN.MIRROR)
P, S, CAND = 16, 8, 512


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import _lib, fit, mesh, ops, primsdf
    return type("Mods", (), dict(lib=_lib.load(), fit=fit, mesh=mesh, ops=ops, primsdf=primsdf, PrimxError=_lib.PrimxError))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _tables(s):
    return [_dev(s["face_material"]), _dev(s["mat_factor"]), _dev(s["mat_tex"]), _dev(s["desc"]), _dev(s["blob"])]


def _gpu_sample(fit, s, n, vattr=True, **over):
    t = dict(zip(("face_material", "mat_factor", "mat_tex", "desc", "blob"), _tables(s)))
    t.update({k: _dev(v) for k, v in over.items() if k in t})
    face = over.get("face", s["face"][:n])
    out = fit.material_sample(_dev(s["uv"][:n]), _dev(s["vattr"][:n]) if vattr else None, _dev(face), t["face_material"],
                              t["mat_factor"], t["mat_tex"], t["desc"], t["blob"])
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the sampler, bit for bit
@pytest.mark.parametrize("nearest", [False, True], ids=["linear", "nearest"])
@pytest.mark.parametrize("size", range(len(MN.SIZES)), ids=[f"{w}x{h}" for h, w in MN.SIZES])
def test_sampler_matches_the_float32_restatement_bit_for_bit(mods, size, nearest):
    """Textures of W x H = 1 x 1, 2 x 3, 5 x 7, 64 x 64 (and the next size under material 1), the nine wrap pairs, both filters, three
    materials (one without textures), uv in [-3, 4] with exact texel centres and edges, 0, 1, -0.0 and +-1e30; prefixes n = 1,
    255, 257, 1000 of one point set."""
    for ws in WRAPS:
        for wt in WRAPS:
            s = MN.sampler_scene(ws, wt, nearest, size)
            r32, r64 = MN.restated(s, np.float32), MN.restated(s, np.float64)
            assert np.isfinite(r32).all()
            for n in NS:
                got = _gpu_sample(mods.fit, s, n)
                assert got.shape == (n, 5) and got.dtype == np.float32 and np.isfinite(got).all()
                same = got.view(np.uint32) == r32[:n].view(np.uint32)
                if not same.all():
                    bad = np.argwhere(~same)[0]
                    print(f"size {MN.SIZES[size]} wrap ({ws}, {wt}) nearest {nearest} n {n}: {int((~same).sum())} of {same.size} differ; first at "
                          f"{bad.tolist()}: uv {s['uv'][bad[0]].tolist()}, got {got[bad[0], bad[1]]!r}, want {r32[bad[0], bad[1]]!r}, "
                          f"max-abs difference {float(np.abs(got - r32[:n]).max()):.3e} (float64 floor {float(np.abs(r32 - r64).max()):.3e})")
                assert same.all(), (size, ws, wt, nearest, n)
            assert np.array_equal(_gpu_sample(mods.fit, s, 1000, vattr=False).view(np.uint32),
                                  MN.restated(s, np.float32, vattr=False).view(np.uint32))       # vattr = NULL: all ones


def test_sampler_without_any_texture(mods):
    """T = 0: every material samples 1.0, with an empty and with a one-texel blob; n = 0 returns an empty result."""
    s = MN.sampler_scene(MN.REPEAT, MN.REPEAT, False, 2)
    s = dict(s, mat_tex=np.full((3, 2), -1, np.int32), desc=np.zeros((0, 4), np.int64))
    want = MN.restated(s, np.float32)
    for blob in (np.zeros((0, 4), np.uint8), np.zeros((1, 4), np.uint8)):
        for n in NS:
            got = _gpu_sample(mods.fit, dict(s, blob=blob), n)
            assert np.array_equal(got.view(np.uint32), want[:n].view(np.uint32))
    assert np.array_equal(want[:, :3], s["mat_factor"][s["face_material"][s["face"]], :3] * s["vattr"][:, :3])
    assert _gpu_sample(mods.fit, s, 0).shape == (0, 5)


def test_bad_indices_are_refused_and_nothing_faults(mods):
    """Validation paths: each broken link of face -> material -> texture -> descriptor returns PRIMX_EINVAL (nothing is dereferenced
    past a broken link), and the next good call is served."""
    s = MN.sampler_scene(MN.REPEAT, MN.CLAMP, False, 2)
    F, n_texels = s["face_material"].shape[0], s["blob"].shape[0]

    def edited(key, index, value):
        a = s[key].copy()
        a[index] = value
        return {key: a}
    cases = []
    for bad in (F, -1, 2 ** 31 - 1, -2 ** 31):
        face = s["face"][:257].copy()
        face[100] = bad
        cases.append((r"face lies outside \[0, F\)", dict(face=face)))
    for bad in (3, -1, 2 ** 31 - 1):
        cases.append((r"material index lies outside \[0, M\)", edited("face_material", 5, bad)))
        cases.append((r"material index lies outside \[0, M\)", edited("face_material", F - 1, bad)))
    for bad in (3, -2, 2 ** 31 - 1, -2 ** 31):
        cases.append((r"texture index lies outside \[-1, T\)", edited("mat_tex", (0, 1), bad)))
        cases.append((r"texture index lies outside \[-1, T\)", edited("mat_tex", (1, 0), bad)))
    for row, col, bad in ((0, 0, n_texels), (2, 0, n_texels - 1), (1, 0, -1), (0, 0, 2 ** 62), (0, 1, 0), (0, 1, 65537), (1, 2, -4),
                          (2, 1, 2 ** 40), (0, 2, 2 ** 33), (1, 3, 3), (1, 3, 12), (2, 3, 32), (0, 3, -1)):
        cases.append((r"descriptor is malformed or runs past", edited("desc", (row, col), bad)))
    cases.append((r"descriptor is malformed or runs past", dict(blob=s["blob"][:-1])))
    for match, over in cases:
        with pytest.raises(mods.PrimxError, match=match):
            _gpu_sample(mods.fit, s, 257, **over)
    torch.cuda.synchronize()
    got = _gpu_sample(mods.fit, s, 257)                                                       # the process is healthy
    assert np.array_equal(got.view(np.uint32), MN.restated(s, np.float32, 257).view(np.uint32))
    with pytest.raises(ValueError):
        mods.fit.material_sample(_dev(s["uv"]), _dev(s["vattr"][:, :5]), _dev(s["face"]), *_tables(s))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mods.fit.material_sample(torch.from_numpy(s["uv"]), None, _dev(s["face"]), *_tables(s))


# ------------------------------------------------------------------------------------------------ 2. field level
def _material_mesh(mods, s, device=None, **over):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    d = dict(s, **over)
    m = mods.mesh.MaterialMesh(v=t(d["v"]), f=t(d["f"]), vt=t(d["vt"]), color=t(d["color"]), rm=t(d["rm"]),
                               face_material=t(d["face_material"]), mat_factor=t(d["mat_factor"]), mat_tex=t(d["mat_tex"]),
                               tex_image=t(d["tex_image"]), tex_sampler=t(d["tex_sampler"]), images=[t(i) for i in d["images"]])
    return m if device is None else m.to(device)


def _field_bound(p, v, face, s):
    a64, a32 = (MN.field_attributes(MF, p, v, face, s, t) for t in (np.float64, np.float32))
    return a64, float(np.abs(a32.astype(np.float64) - a64).max())


def test_field_attributes_on_the_textured_box(mods):
    """The box with per-face UV charts (24 split vertices, 12 faces), a 5 x 7 and an 8 x 8 random texture under two materials, LINEAR."""
    s = MN.box_scene()
    mm = _material_mesh(mods, s)
    desc, blob = mm.texture_tables()
    assert np.array_equal(desc.numpy(), s["desc"]) and np.array_equal(blob.numpy(), s["blob"])
    field = mods.fit.MeshField(_dev(s["v"]), _dev(s["f"]), material=mm)
    p = _points(s["v"], s["f"], 1000, seed=4)
    worst = 0.0
    for n in NS:
        q = field.query(_dev(p[:n]))
        assert set(q) == {"sdf", "tex", "mat", "face", "wn"} and q["tex"].shape == (n, 3) and q["mat"].shape == (n, 2)
        face = q["face"].cpu().numpy().astype(np.int64)
        got = torch.cat([q["tex"], q["mat"]], 1).cpu().numpy().astype(np.float64)
        a64, floor = _field_bound(p[:n], s["v"], face, s)
        err = float(np.abs(got - a64).max())
        print(f"textured box, n = {n}: attributes max-abs error {err:.3e}, fp32 restatement {floor:.3e}, error / (4 x floor) = "
              f"{err / (4 * floor):.3f}")
        assert np.isfinite(got).all() and got.min() >= 0 and got.max() <= 1 and floor > 0
        assert err <= 4 * floor, (n, err, floor)
        worst = max(worst, err / (4 * floor))
        plain = mods.fit.MeshField(_dev(s["v"]), _dev(s["f"])).query(_dev(p[:n]))              # the geometry does not see the material
        assert torch.equal(plain["sdf"], q["sdf"]) and torch.equal(plain["face"], q["face"]) and torch.equal(plain["wn"], q["wn"])
    assert len(np.unique(s["face_material"][face])) == 2 and a64[:, :3].std() > 0.05            # both materials, real texture contrast


# ------------------------------------------------------------------------------------------------ 3. equivalence, no tolerance
def test_untextured_material_mesh_is_the_trimesh_path_bit_for_bit(mods, tmp_path):
    v, f = MF.icosphere(2, 0.5, (0.1, -0.2, 0.05))
    attr = MF.affine_attr(v)
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    tm = mods.mesh.TriMesh(_dev(v), _dev(f), _dev(nrm), _dev(attr[:, :3]), _dev(attr[:, 3]), _dev(attr[:, 4]))
    kw = dict(num_prims=P, prim_shape=S, candidates=CAND, seed=2)
    want, winfo = mods.fit.mesh_to_primitives(tm, **kw)
    tup, _ = mods.fit.mesh_to_primitives((tm.v, tm.f, tm.albedo, tm.roughness, tm.metallic), **kw)
    assert torch.equal(want, tup)
    mm = mods.mesh.material_mesh(v, f, color=np.concatenate([attr[:, :3], np.ones((v.shape[0], 1), np.float32)], 1), rm=attr[:, 3:5])
    for mesh in (mm, mm.to(DEV)):
        got, info = mods.fit.mesh_to_primitives(mesh, device=DEV, **kw)
        assert fp.same_bits(got, want) and torch.equal(info["idx"], winfo["idx"]) and info["attr"].shape == (v.shape[0], 8)
    path = os.path.join(tmp_path, "tri.glb")
    tm.write_glb(path)
    back = mods.mesh.read_glb(path)
    got, _ = mods.fit.mesh_to_primitives(back, device=DEV, **kw)
    assert fp.same_bits(got, want)
    got, _ = mods.fit.mesh_to_primitives(mods.mesh.read_glb(path, device=DEV), **kw)
    assert fp.same_bits(got, want)
    m = mods.primsdf.PrimSDF.from_mesh(back.to(DEV), **kw)
    assert fp.same_bits(torch.cat([m.srt_param, m.feat_param], 1), want)


# ------------------------------------------------------------------------------------------------ 4. the fit
def test_fit_of_the_textured_box(mods):
    s = MN.box_scene()
    mm = _material_mesh(mods, s, DEV)
    kw = dict(num_prims=P, prim_shape=S, candidates=CAND, seed=1)
    recon, info = mods.fit.mesh_to_primitives(mm, **kw)
    z = torch.zeros(24, device=DEV)
    plain, _ = mods.fit.mesh_to_primitives((_dev(s["v"]), _dev(s["f"]), torch.zeros(24, 3, device=DEV), z, z), **kw)
    s3 = S ** 3
    assert recon.shape == (P, 4 + 6 * s3) and fp.same_bits(recon[:, :4 + s3].contiguous(), plain[:, :4 + s3].contiguous())   # srt and sdf
    # the payload against the restated pipeline at the fit's own voxel positions, on the faces the kernel chose
    vn = info["v"].cpu().numpy()
    lin = torch.linspace(-1, 1, S).numpy()
    zz, yy, xx = np.meshgrid(lin, lin, lin, indexing="ij")
    grid = np.stack([xx, yy, zz], -1).reshape(-1, 3)
    srt = recon[:, :4].cpu().numpy()
    x = (srt[:, None, 1:4] + srt[:, None, 0:1] * grid[None]).astype(np.float32).reshape(-1, 3)
    face = mods.fit.mesh_field_query(_dev(x), info["v"], info["f"], None)[1].cpu().numpy().astype(np.int64)
    a64, floor = _field_bound(x, vn, face, s)
    ga = recon[:, 4 + s3:].cpu().numpy().astype(np.float64).reshape(P, 5, s3).transpose(0, 2, 1).reshape(-1, 5)
    err = float(np.abs(ga - a64).max())
    print(f"textured box fit, {P} x {s3} voxels: payload colours max-abs error {err:.3e}, fp32 restatement {floor:.3e}, "
          f"error / (4 x floor) = {err / (4 * floor):.3f}")
    assert floor > 0 and err <= 4 * floor and ga.min() >= 0 and ga.max() <= 1 and ga[:, :3].std() > 0.05
    refined, rinfo = mods.fit.mesh_to_primitives(mm, refine=2, **kw)
    loss = rinfo["refine"]["loss"]
    print("textured box fit, refine=2, loss before each step:", " ".join(f"{v:.6e}" for v in loss))
    assert len(loss) == 2 and all(np.isfinite(loss)) and loss[1] <= loss[0]
    assert torch.equal(refined[:, :4], recon[:, :4]) and not torch.equal(refined[:, 4:], recon[:, 4:])


# ------------------------------------------------------------------------------------------------ 5. footprint and stream order
def test_footprint_of_the_sampler_and_of_the_material_field(mods):
    s = MN.sampler_scene(MN.MIRROR, MN.REPEAT, False, 2)
    for n in (1, 257, 1000):
        def case(g, n=n):
            i = lambda a, name: g.guard_input(_dev(a), name).t   # noqa: E731
            return mods.fit.material_sample(i(s["uv"][:n], "uv"), i(s["vattr"][:n], "vattr"), i(s["face"][:n], "face"),
                                            i(s["face_material"], "face_material"), i(s["mat_factor"], "mat_factor"),
                                            i(s["mat_tex"], "mat_tex"), i(s["desc"], "desc"), i(s["blob"], "blob"))
        out = fp.hold(case)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), MN.restated(s, np.float32, n).view(np.uint32))
    b = MN.box_scene()
    p = _points(b["v"], b["f"], 257, seed=6)

    def field_case(g):
        field = mods.fit.MeshField(g.guard_input(_dev(b["v"]), "v").t, g.guard_input(_dev(b["f"]), "f").t, material=_material_mesh(mods, b))
        q = field.query(g.guard_input(_dev(p), "x").t)
        return [q["sdf"], q["tex"], q["mat"], q["face"], q["wn"]]
    out = fp.hold(field_case)
    assert out[1].shape == (257, 3) and bool(torch.isfinite(out[1]).all())


_TABLES = ("face_material", "mat_factor", "mat_tex", "desc", "blob")


@TS.case("material_sample", ["primx_material_sample"])
def _stream_material_sample(E, dtype):  # noqa: F811
    from topia_xl_amd import fit

    def make(k):
        s = MN.sampler_scene(MN.REPEAT, MN.MIRROR, False, 3, seed=k, n=70001)
        return {key: _dev(s[key]) for key in ("uv", "vattr", "face") + _TABLES}
    return make, (lambda ctx, i, probe: fit.material_sample(i["uv"], i["vattr"], i["face"], *(i[key] for key in _TABLES))), None


@TS.case("mesh_field_material", ["primx_mesh_field_query", "primx_material_sample"])
def _stream_material_field(E, dtype):  # noqa: F811
    """The material (host tensors) is the context; `MeshField(...)` uploads its tables and texels inside the call, on the stream."""
    from topia_xl_amd import fit, mesh
    b = MN.box_scene()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731

    def setup():
        return mesh.MaterialMesh(v=t(b["v"]), f=t(b["f"]), vt=t(b["vt"]), color=t(b["color"]), rm=t(b["rm"]),
                                 face_material=t(b["face_material"]), mat_factor=t(b["mat_factor"]), mat_tex=t(b["mat_tex"]),
                                 tex_image=t(b["tex_image"]), tex_sampler=t(b["tex_sampler"]), images=[t(i) for i in b["images"]])

    def make(k):
        return {"v": _dev(b["v"]) * (1.0 + 0.1 * k), "f": _dev(b["f"]), "x": TS.R(k, "mfm.x", 4097, 3, scale=0.4)}

    def call(ctx, i, probe):
        q = fit.MeshField(i["v"], i["f"], material=ctx).query(i["x"])
        return [q["sdf"], q["tex"], q["mat"], q["face"], q["wn"]]
    return make, call, setup


STREAM_CASES = ("material_sample", "mesh_field_material")
_READBACK = "the C host reads the index check of primx_material_sample back (csrc/material.hip) before it returns"
TS.MUST_SYNC["material_sample"] = _READBACK
TS.MUST_SYNC["mesh_field_material"] = TS.MUST_SYNC["mesh_field_query"] + "; " + _READBACK


@pytest.mark.parametrize("name", STREAM_CASES)
def test_stream_order_of_the_material_entry_point(E, called, name):  # noqa: F811  (`E`, `called` are the imported fixtures)
    """The body of tests/test_hip_streams.py::test_stream_order for the cases registered above."""
    c = TS.CASES[name]
    make, call, setup = c.build(E, None)
    rep = so.run(name, make, call, E.S, E.blocker, setup=setup, must_sync=name in TS.MUST_SYNC)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{name} declares entry points it did not call: {missing}"
