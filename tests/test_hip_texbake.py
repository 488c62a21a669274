"""Texture bake on the MI355X (csrc/texbake.hip, mesh.py): labels and charts, the atlas raster, the barycentric points and
the texel fill against the numpy restatement (tests/texbake_numpy.py), the overlap fallback, the baked texels against the
field query, and the end-to-end bake of a field whose albedo is linear in position."""
import numpy as np
import pytest
import torch

from tests import mc_numpy
from tests import texbake_numpy as T
from tests.test_hip_mesh import _synthetic_field

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import mesh
    return mesh


def _meshes():
    out = {}
    for name, (vol, *_rest) in mc_numpy.analytic_fields(64).items():
        out[name] = mc_numpy.marching_cubes(vol)
    vol = np.random.default_rng(4).standard_normal((24, 24, 24)).astype(np.float32)
    out["random"] = mc_numpy.marching_cubes(vol, 0.2)
    return out


def _dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def test_labels_and_charts_match_restatement(M):
    for name, (v, n, f) in _meshes().items():
        for normals in (n, None):
            lab = M.face_labels(_dev(v), _dev(f, torch.int32), None if normals is None else _dev(normals)).cpu().numpy()
            rlab, rcomp, rnc = T.charts(v, f, normals)
            np.testing.assert_array_equal(lab, rlab, err_msg=name)
            comp, nc = M.face_components(_dev(f.astype(np.int64) * 6 + rlab[:, None], torch.int32), 6 * len(v))
            assert nc == rnc, (name, nc, rnc)
            np.testing.assert_array_equal(comp.cpu().numpy(), rcomp, err_msg=name)
        print(f"{name}: {len(f)} faces, {rnc} charts")
        a = M.uv_unwrap(_dev(v), _dev(f, torch.int32), _dev(n), (1024, 1024))
        if a.split_rounds == 0:
            np.testing.assert_array_equal(a.chart.cpu().numpy(), T.charts(v, f, n)[1], err_msg=name)


def _check_atlas(M, a, v, f):
    W, H = a.size
    fid, cnt = T.raster(a.uv_fixed.cpu().numpy(), a.f.cpu().numpy(), W, H)
    np.testing.assert_array_equal(a.face_id.cpu().numpy(), fid)
    assert a.doubly == int((cnt > 1).sum()) == 0
    assert a.n_covered == int((fid >= 0).sum())
    # vt is the fixed-point corner; every chart is its projection under one scale and a translation
    uvf = a.uv_fixed.cpu().numpy()
    np.testing.assert_array_equal(a.vt.cpu().numpy(), (uvf / np.array([256.0 * W, 256.0 * H])).astype(np.float32))
    lab = a.label.cpu().numpy()
    proj = T.project(v, f, lab)                                         # [F, 3, 2]
    x = uvf[a.f.cpu().numpy()] / 256.0
    chart = a.chart.cpu().numpy()
    d = x - proj * a.scale
    for c in np.unique(chart)[:200]:
        dc = d[chart == c].reshape(-1, 2)
        assert np.abs(dc - dc[0]).max() < 4e-3 + 1e-6 * a.scale, c
    # split vertices map back to the input
    vm = a.vmap.cpu().numpy()
    np.testing.assert_array_equal(vm[a.f.cpu().numpy()], f)
    # barycentric points
    texel, pts = M.atlas_points(a, _dev(v), _dev(f, torch.int32))
    rt, rp = T.points(fid, uvf, a.f.cpu().numpy(), v, f)
    np.testing.assert_array_equal(texel.cpu().numpy(), rt)
    np.testing.assert_allclose(pts.cpu().numpy(), rp, rtol=0, atol=1e-6)
    return texel, pts


def test_raster_and_points_match_restatement(M):
    v, n, f = _meshes()["sphere"]
    a = M.uv_unwrap(_dev(v), _dev(f, torch.int32), _dev(n), (512, 384))
    assert a.split_rounds == 0 and a.coverage > 0.3
    _check_atlas(M, a, v, f)
    # overlapping random triangles: the face-id map, the cover counts and the doubly covered count
    rng = np.random.default_rng(7)
    uv = rng.integers(-300, 70 * 256, size=(300, 2)).astype(np.int32)
    ft = rng.integers(0, 300, size=(400, 3)).astype(np.int32)
    ft[:5] = [[0, 1, 2], [2, 1, 0], [3, 3, 4], [5, 6, 7], [7, 6, 5]]
    fid, cover, covered, doubly, _ = M.atlas_raster(_dev(uv, torch.int32), _dev(ft, torch.int32), 64, 48)
    rfid, rcnt = T.raster(uv, ft, 64, 48)
    np.testing.assert_array_equal(fid.cpu().numpy(), rfid)
    np.testing.assert_array_equal(cover.cpu().numpy(), rcnt)
    assert covered == int((rcnt > 0).sum()) and doubly == int((rcnt > 1).sum()) > 0
    # a square split along its diagonal on exact texel centres: every centre of the square covered exactly once
    sq = np.array([[128, 128], [128 + 256 * 10, 128], [128 + 256 * 10, 128 + 256 * 10], [128, 128 + 256 * 10]], np.int32)
    fq = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    fid, cover, covered, doubly, _ = M.atlas_raster(_dev(sq, torch.int32), _dev(fq, torch.int32), 16, 16)
    assert doubly == 0 and covered == int((T.raster(sq, fq, 16, 16)[1] > 0).sum())
    np.testing.assert_array_equal(cover.cpu().numpy(), T.raster(sq, fq, 16, 16)[1])


def helicoid(turns=1.5, nt=240, nr=8, pitch=0.04):
    t = np.linspace(0, 2 * np.pi * turns, nt)
    r = np.linspace(0.3, 1.0, nr)
    T_, R_ = np.meshgrid(t, r, indexing="ij")
    v = np.stack([R_ * np.cos(T_), R_ * np.sin(T_), pitch * T_], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(nt * nr).reshape(nt, nr)
    a, b, c, d = idx[:-1, :-1], idx[:-1, 1:], idx[1:, 1:], idx[1:, :-1]
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    f[g[:, 2] < 0] = f[g[:, 2] < 0][:, ::-1]
    return v, f.astype(np.int32)


def test_overlap_fallback(M):
    v, f = helicoid()
    lab, comp, nc = T.charts(v, f)
    assert (lab == 4).mean() > 0.95 and nc <= 3                      # one +z chart that wraps over itself
    a = M.uv_unwrap(_dev(v), _dev(f, torch.int32), None, (512, 512))
    assert a.split_rounds > 0 and a.doubly == 0 and a.n_charts > nc
    _check_atlas(M, a, v, f)
    print(f"helicoid: {len(f)} faces, {nc} charts -> {a.n_charts} after {a.split_rounds} split rounds")


def _linear_field(P=256, S=8):
    """A sphere of radius 0.5 (exact distance payload) with albedo = 0.5 + 0.4 (x, y, z) and roughness / metallic
    linear too.  The primitives (scale 0.2) sit on a Fibonacci sphere, so every surface point lies well inside some
    primitive and the query is linear there (the trilinear payload and the weighted blend both keep linear functions)."""
    from topia_xl_amd.primsdf import PrimSDF
    k = torch.arange(P, dtype=torch.float64) + 0.5
    z = 1 - 2 * k / P
    phi = k * np.pi * (3 - np.sqrt(5.0))
    r = torch.sqrt(1 - z * z)
    pos = (0.5 * torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], 1)).float()
    srt = torch.cat([torch.full((P, 1), 0.2), pos], 1)
    lin = torch.linspace(-1, 1, S)
    Zg, Yg, Xg = torch.meshgrid(lin, lin, lin, indexing="ij")
    local = torch.stack([Xg, Yg, Zg], -1).reshape(1, -1, 3)
    pts = srt[:, None, 1:4] + srt[:, None, 0:1] * local                 # [P, S^3, 3]
    ch = [pts.norm(dim=-1) - 0.5, 0.5 + 0.4 * pts[..., 0], 0.5 + 0.4 * pts[..., 1], 0.5 + 0.4 * pts[..., 2],
          0.5 + 0.3 * pts[..., 0], 0.5 - 0.3 * pts[..., 2]]
    m = PrimSDF(num_prims=P, prim_shape=S)
    m.srt_param.data = srt
    m.feat_param.data = torch.cat(ch, 1)
    return m.eval().to(DEV)


def _bilinear(img, uv):
    H, W = img.shape[:2]
    x, y = uv[:, 0] * W - 0.5, uv[:, 1] * H - 0.5
    x0, y0 = np.clip(np.floor(x).astype(int), 0, W - 2), np.clip(np.floor(y).astype(int), 0, H - 2)
    fx, fy = np.clip(x - x0, 0, 1)[:, None], np.clip(y - y0, 0, 1)[:, None]
    im = img.astype(np.float64)
    return ((im[y0, x0] * (1 - fx) + im[y0, x0 + 1] * fx) * (1 - fy) + (im[y0 + 1, x0] * (1 - fx) + im[y0 + 1, x0 + 1] * fx) * fy)


def test_bake_matches_query_and_fill(M):
    field = _linear_field()
    mesh = M.extract_mesh(field, resolution=64, filter_noise=False)
    snap = {k: getattr(mesh, k).clone() for k in ("v", "f", "normals", "albedo")}
    srt0, feat0 = field.srt_param.detach().clone(), field.feat_param.detach().clone()
    tm = M.bake_textures(field, mesh, size=256)
    a = M.uv_unwrap(mesh.v, mesh.f, mesh.normals, (256, 256))
    texel, pts = M.atlas_points(a, mesh.v, mesh.f)
    q = field.query(pts)
    cov = tm.covered.cpu().numpy()
    assert torch.equal(tm.covered, a.face_id >= 0)
    alb, mr = tm.albedo.cpu().numpy().reshape(-1, 3), tm.metallic_roughness.cpu().numpy().reshape(-1, 3)
    t = texel.cpu().numpy()
    qq = (q * 255.0).float()                                            # fp32(x * 255), truncated
    assert torch.equal(torch.from_numpy(alb[t]).to(DEV), qq[:, 1:4].to(torch.uint8))
    assert torch.equal(torch.from_numpy(mr[t][:, 1:]).to(DEV), qq[:, 4:6].to(torch.uint8)) and (mr[:, 0] == 0).all()
    ralb, rmr = T.fill(q.cpu().numpy(), t, cov)
    np.testing.assert_array_equal(tm.albedo.cpu().numpy(), ralb)
    np.testing.assert_array_equal(tm.metallic_roughness.cpu().numpy(), rmr)
    for k, x in snap.items():
        assert torch.equal(getattr(mesh, k), x), k
    assert torch.equal(field.srt_param.detach(), srt0) and torch.equal(field.feat_param.detach(), feat0)
    # the split mesh: v = input v[vmap], faces in the input order
    assert torch.equal(tm.v, mesh.v[tm.vmap]) and torch.equal(tm.vmap[tm.f.long()], mesh.f.long())


def test_end_to_end_linear_albedo(M, tmp_path):
    field = _linear_field()
    tm = M.extract_texmesh(field, resolution=96, texture_size=512, filter_noise=False)
    a = M.uv_unwrap(*(lambda m: (m.v, m.f, m.normals))(M.extract_mesh(field, resolution=96, filter_noise=False)),
                    size=(512, 512))
    assert a.coverage >= 0.30, a.coverage
    f = tm.f.long()
    cen = tm.v[f].mean(1)
    q = field.query(cen).cpu().numpy()
    uv = tm.vt[f].mean(1).cpu().numpy()
    got = _bilinear(tm.albedo.cpu().numpy(), uv) / 255.0
    tol = 2 / 255 + 0.4 * 1.5 / a.scale
    err = np.abs(got - q[:, 1:4]).max(1)
    print(f"end to end: {len(f)} faces, scale {a.scale:.1f} texels / unit, max err {err.max():.4f} (tol {tol:.4f}), "
          f"coverage {a.coverage:.3f}, {a.n_charts} charts")
    assert err.max() <= tol
    got_mr = _bilinear(tm.metallic_roughness.cpu().numpy(), uv) / 255.0
    assert np.abs(got_mr[:, 1:] - q[:, 4:6]).max() <= 2 / 255 + 0.3 * 1.5 / a.scale
    path = str(tmp_path / "pbr.glb")
    tm.write_glb(path)
    from tests.test_texbake_cpu import parse_textured_glb
    gltf, arrays, images = parse_textured_glb(path)
    np.testing.assert_array_equal(images[0], tm.albedo.cpu().numpy())
    np.testing.assert_array_equal(arrays[gltf["meshes"][0]["primitives"][0]["attributes"]["TEXCOORD_0"]], tm.vt.cpu().numpy())


def test_deterministic_pipeline_and_empty(M):
    field = _synthetic_field()
    a = M.extract_texmesh(field, resolution=64, texture_size=256)
    b = M.extract_texmesh(field, resolution=64, texture_size=256)
    for k in ("v", "f", "normals", "vt", "vmap", "albedo", "metallic_roughness", "covered"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    from topia_xl_amd import pipeline
    recon = torch.cat([field.srt_param.detach(), field.feat_param.detach()], 1)
    c = pipeline.primitives_to_texmesh(recon, resolution=64, texture_size=256)
    for k in ("v", "f", "vt", "albedo", "metallic_roughness"):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    # an empty mesh: all-zero textures and a GLB that parses
    empty = M.TriMesh(torch.empty(0, 3, device=DEV), torch.empty(0, 3, dtype=torch.int32, device=DEV),
                      torch.empty(0, 3, device=DEV), torch.empty(0, 3, device=DEV), torch.empty(0, device=DEV),
                      torch.empty(0, device=DEV))
    e = M.bake_textures(field, empty, size=64)
    assert e.f.shape == (0, 3) and int(e.albedo.sum()) == 0 and int(e.metallic_roughness.sum()) == 0
    assert not bool(e.covered.any())
    import tempfile, os
    from tests.test_texbake_cpu import parse_textured_glb
    with tempfile.TemporaryDirectory() as d:
        e.write_glb(os.path.join(d, "e.glb"))
        gltf, _, images = parse_textured_glb(os.path.join(d, "e.glb"))
        assert len(images) == 2 and (images[0] == 0).all()
