"""Primitive fitting on the MI355X (csrc/meshfield.hip, fit.py) against the numpy restatement tests/meshfield_numpy.py.

There are no goldens from the reference: its PrimSDF._init_param is an empty `pass` (models/primsdf.py:48-50).  Areas,
surface points, FPS, `nn` and the srt columns of a fit are compared bit for bit with the float32 restatement.  The query's
bounds are not constants: each is 4 x the largest error of the SAME restatement evaluated in numpy float32 against itself in
float64 on the test's own mesh and points (the margin 4 covers a different summation order, atan2 and region choice of a correct
fp32 kernel); the kernel runs on prefixes of those points (n = 1, 255, 257, 1000) and every point of every prefix is compared.
The figures are printed before they are asserted; the ones seen are recorded in DESIGN.md "Primitive fitting".
"""
import os

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import meshfield_numpy as MF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 255, 257, 1000)


@pytest.fixture(scope="module")
def fit():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import fit
    return fit


def _chunk_sizes(fit):
    c = fit.QUERY_CHUNK
    return (1, c - 1, c, c + 1, 2 * c + 37)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _points(v, f, n=1000, seed=0):
    """Uniform points of the mesh's neighbourhood, and points a little off its surface (both sides)."""
    rng = np.random.default_rng(seed)
    far = rng.uniform(-0.8, 0.8, (n - n // 3, 3))
    cdf = np.cumsum(MF.face_areas(v, f))
    if not cdf[-1] > 0:
        return rng.uniform(-0.8, 0.8, (n, 3)).astype(np.float32)
    on, _ = MF.surface_points(v, f, cdf, rng.random((n // 3, 3)).astype(np.float32))
    near = on + rng.normal(0, 0.01, on.shape)
    p = np.concatenate([far, near]).astype(np.float32)
    return p[rng.permutation(n)]


def _gpu_query(fit, p, v, f, attr):
    d, face, wn, a = fit.mesh_field_query(_dev(p), _dev(v), _dev(f), None if attr is None else _dev(attr))
    return d.cpu().numpy(), face.cpu().numpy().astype(np.int64), wn.cpu().numpy(), None if a is None else a.cpu().numpy()


def _check_query(fit, v, f, p, ns, label):
    """Every point of every prefix of p: dist, face, out_attr and wn inside 4 x the fp32 restatement's own error; inside /
    outside as float64 wherever the distance exceeds its bound.  -> the figures."""
    attr = MF.affine_attr(v)
    q64, q32 = MF.query(p, v, f, attr, np.float64), MF.query(p, v, f, attr, np.float32)
    floor_d = float(np.abs(q32["dist"].astype(np.float64) - q64["dist"]).max())
    floor_w = float(np.abs(q32["wn"].astype(np.float64) - q64["wn"]).max())
    bd, bw = 4 * floor_d, 4 * floor_w
    fig = {"F": f.shape[0], "floor_dist": floor_d, "floor_wn": floor_w, "err_dist": 0.0, "err_wn": 0.0, "err_face": 0.0,
           "floor_attr": 0.0, "err_attr": 0.0}
    checks = []
    for n in ns:
        d, face, wn, a = _gpu_query(fit, p[:n], v, f, attr)
        assert d.shape == (n,) and face.shape == (n,) and wn.shape == (n,) and a.shape == (n, 5)
        assert np.isfinite(d).all() and np.isfinite(wn).all() and np.isfinite(a).all()
        assert (face >= 0).all() and (face < f.shape[0]).all()
        a64 = MF.attr_on_face(p[:n], v, f, attr, face, np.float64)
        a32 = MF.attr_on_face(p[:n], v, f, attr, face, np.float32)
        floor_a = float(np.abs(a32.astype(np.float64) - a64).max())
        e_d = float(np.abs(d.astype(np.float64) - q64["dist"][:n]).max())
        e_f = float((np.sqrt(q64["d2"][np.arange(n), face]) - q64["dist"][:n]).max())
        e_w = float(np.abs(wn.astype(np.float64) - q64["wn"][:n]).max())
        e_a = float(np.abs(a.astype(np.float64) - a64).max())
        clear = q64["dist"][:n] > bd
        signs = bool(((np.abs(wn) >= 0.5) == (np.abs(q64["wn"][:n]) >= 0.5))[clear].all())
        for k, x in (("err_dist", e_d), ("err_face", e_f), ("err_wn", e_w), ("err_attr", e_a), ("floor_attr", floor_a)):
            fig[k] = max(fig[k], x)
        checks.append((n, e_d, e_f, e_w, e_a, 4 * floor_a, signs))
    print(f"{label}: " + ", ".join(f"{k} = {x:.3e}" if isinstance(x, float) else f"{k} = {x}" for k, x in fig.items()))
    for n, e_d, e_f, e_w, e_a, ba, signs in checks:
        assert e_d <= bd, (label, n, "dist", e_d, bd)
        assert e_f <= bd, (label, n, "face", e_f, bd)
        assert e_w <= bw, (label, n, "wn", e_w, bw)
        assert e_a <= ba, (label, n, "attr", e_a, ba)
        assert signs, (label, n, "inside / outside differs from float64 away from the surface")
    return fig


@pytest.mark.parametrize("which", range(5))
def test_query_at_the_chunk_edges(fit, which):
    """F = 1, one below, at, one above and a little over twice the kernel's triangle chunk; n = 1, 255, 257, 1000."""
    F = _chunk_sizes(fit)[which]
    v, f = MF.mesh_with_faces(F)
    _check_query(fit, v, f, _points(v, f, 1000, seed=F), NS, f"query F={F}")


def test_query_on_the_closed_fixtures_and_the_open_hemisphere(fit):
    for name, (v, f) in (("box", MF.box()), ("icosphere", MF.icosphere(2)), ("hemisphere", MF.hemisphere(2))):
        fig = _check_query(fit, v, f, _points(v, f, 1000, seed=len(name)), (1000,), name)
        assert fig["floor_wn"] > 0 and fig["floor_dist"] > 0


def test_query_without_attributes(fit):
    v, f = MF.icosphere(1)
    p = _points(v, f, 257, 3)
    d, face, wn, a = _gpu_query(fit, p, v, f, None)
    d2, face2, wn2, _ = _gpu_query(fit, p, v, f, MF.affine_attr(v))
    assert a is None and np.array_equal(d, d2) and np.array_equal(face, face2) and np.array_equal(wn, wn2)
    out = fit.mesh_field(_dev(v), _dev(f)).query(_dev(p))
    assert set(out) == {"sdf", "tex", "mat", "face", "wn"} and float(out["tex"].abs().max()) == 0.0
    assert np.array_equal(out["sdf"][:, 0].cpu().numpy(), np.where(np.abs(wn) >= 0.5, -d, d))
    e = fit.mesh_field_query(_dev(p[:0]), _dev(v), _dev(f), _dev(MF.affine_attr(v)))
    assert e[0].shape == (0,) and e[3].shape == (0, 5)


def _bad_mesh():
    v, f = MF.box()
    extra = np.array([[0.5, 0.5, 0.5], [0.75, 0.25, 0.625], [0.625, 0.375, 0.5625]], np.float32)
    deg = np.array([[8, 8, 9], [8, 9, 8], [8, 10, 9], [10, 10, 10], [8, 8, 9], [10, 8, 9], [8, 8, 9]], np.int32)
    return np.concatenate([v, extra]), np.concatenate([f[:5], deg, f[5:]]).astype(np.int32), extra


def test_degenerate_faces_and_points_on_the_mesh(fit):
    """A mesh with zero-area triangles (segments in every edge role, a point, a face given three times) and points exactly on
    a vertex, an edge and a face, of the box and of the degenerate faces: every output finite, and inside the same bounds."""
    v, f, extra = _bad_mesh()
    lo, hi = v[:8].min(0), v[:8].max(0)
    mid = ((lo.astype(np.float64) + hi) / 2).astype(np.float32)
    special = np.array([lo, hi, [lo[0], lo[1], mid[2]], [mid[0], hi[1], hi[2]], [mid[0], mid[1], lo[2]], [hi[0], mid[1], mid[2]],
                        extra[0], extra[1], extra[2], (extra[0] + extra[2]) / 2], np.float32)
    p = np.concatenate([special, _points(v, f, 246, 1)])
    attr = MF.affine_attr(v)
    d, face, wn, a = _gpu_query(fit, p, v, f, attr)
    assert np.isfinite(d).all() and np.isfinite(wn).all() and np.isfinite(a).all()
    assert (d[[0, 1, 6, 7, 8]] == 0).all()                    # on a vertex: exactly 0 (edge and face points: inside the bound below)
    q64, q32 = MF.query(p, v, f, attr, np.float64), MF.query(p, v, f, attr, np.float32)
    bd = 4 * float(np.abs(q32["dist"].astype(np.float64) - q64["dist"]).max())
    e_d = float(np.abs(d.astype(np.float64) - q64["dist"]).max())
    e_f = float((np.sqrt(q64["d2"][np.arange(p.shape[0]), face]) - q64["dist"]).max())
    a64, a32 = (MF.attr_on_face(p, v, f, attr, face, t) for t in (np.float64, np.float32))
    ba, e_a = 4 * float(np.abs(a32.astype(np.float64) - a64).max()), float(np.abs(a - a64).max())
    print(f"degenerate: dist {e_d:.3e} / face {e_f:.3e} (bound {bd:.3e}), attr {e_a:.3e} (bound {ba:.3e})")
    assert e_d <= bd and e_f <= bd and e_a <= ba
    # the zero-area faces add nothing to the winding number: the box alone gives the same one, to the bound of the box
    off = p[10:]
    w_box = MF.query(off, v[:8], MF.box()[1], None, np.float64)["wn"]
    w32 = MF.query(off, v[:8], MF.box()[1], None, np.float32)["wn"]
    assert np.abs(wn[10:] - w_box).max() <= 4 * np.abs(w32 - w_box).max()


def test_out_of_range_indices_are_refused(fit):
    from topia_xl_amd._lib import PrimxError
    v, f = MF.box()
    p = _points(v, f, 10)
    cdf = _dev(np.cumsum(MF.face_areas(v, f)))
    u = _dev(np.random.default_rng(0).random((64, 3)).astype(np.float32))
    for bad in (8, -1, 2 ** 31 - 1):
        fb = f.copy()
        fb[7, 1] = bad
        with pytest.raises(PrimxError, match=r"outside \[0, V\)"):
            fit.mesh_field_query(_dev(p), _dev(v), _dev(fb), None)
        with pytest.raises(PrimxError, match=r"outside \[0, V\)"):
            fit.face_areas(_dev(v), _dev(fb))
        fb = f.copy()
        fb[:, 2] = bad                                        # whichever face a sample lands on
        with pytest.raises(PrimxError, match=r"outside \[0, V\)"):
            fit.surface_points(_dev(v), _dev(fb), cdf, u)
    d = fit.mesh_field_query(_dev(p), _dev(v), _dev(f), None)[0]      # and the next good call is served
    assert bool(torch.isfinite(d).all())
    with pytest.raises(PrimxError):
        fit.fps(_dev(p), 11)                                  # K > N
    with pytest.raises(PrimxError):
        fit.fps(_dev(p), 2, start=10)


def test_face_areas_bit_exact(fit):
    for F in (1, 255, 600):
        v, f = MF.mesh_with_faces(F)
        got = fit.face_areas(_dev(v), _dev(f)).cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got, MF.face_areas(v, f))
    v, f, _ = _bad_mesh()
    got = fit.face_areas(_dev(v), _dev(f)).cpu().numpy()
    assert np.array_equal(got, MF.face_areas(v, f)) and (got[5:12] == 0).all()
    assert np.array_equal(fit.area_cdf(_dev(got)).cpu().numpy(), np.cumsum(got))      # the host sum is numpy's, bit for bit


@pytest.mark.parametrize("N", [1, 256, 1000, 4097])
def test_surface_points_bit_exact(fit, N):
    v, f, _ = _bad_mesh()                                     # zero-area faces: equal CDF entries, never chosen
    for vv, ff in ((v, f), MF.mesh_with_faces(600)):
        cdf = np.cumsum(MF.face_areas(vv, ff))
        u = fit.surface_uniforms(N, seed=N).numpy()
        u[0, 0] = 0.0
        u[-1, 0] = np.float32(1) - np.float32(2) ** -24
        pts, face = fit.surface_points(_dev(vv), _dev(ff), _dev(cdf), _dev(u))
        rp, rf = MF.surface_points(vv, ff, cdf, u)
        assert np.array_equal(face.cpu().numpy(), rf) and np.array_equal(pts.cpu().numpy().view(np.uint32), rp.view(np.uint32))
        assert (MF.face_areas(vv, ff)[rf] > 0).all()


def _candidates(N, seed):
    """Surface samples of the level-2 icosphere with duplicated rows (ties), and a symmetric part (equal distances)."""
    v, f = MF.icosphere(2)
    cdf = np.cumsum(MF.face_areas(v, f))
    pts, _ = MF.surface_points(v, f, cdf, np.random.default_rng(seed).random((N, 3)).astype(np.float32))
    pts[::7] = pts[3 % N]
    if N >= 16:
        pts[8:16] = [[sx * 0.5, sy * 0.5, sz * 0.5] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    return pts


@pytest.mark.parametrize("K", [1, 2, 256])
def test_fps_bit_exact(fit, K):
    """N in {K, 1000, 4097} (one block, and five blocks whose partial argmaxes the next launch reduces), K in {1, 2, 256}, with
    duplicated candidates; and 300001 candidates on the full grid of 256 blocks."""
    for N, start in ((K, 0), (1000, 0), (1000, 999), (4097, 5), (300001, 17)):
        if N < K or (N == 300001 and K != 256) or (N == K and start):
            continue
        pts = _candidates(N, seed=N + K)
        idx, nn = fit.fps(_dev(pts), K, start)
        ri, rn = MF.fps(pts, K, start)
        assert np.array_equal(idx.cpu().numpy(), ri), (N, K)
        assert np.array_equal(nn.cpu().numpy().view(np.uint32), rn.view(np.uint32)), (N, K)


# ------------------------------------------------------------------------------------------------ the whole fit
P, S, CAND = 256, 4, 2048


@pytest.fixture(scope="module")
def fitted(fit):
    """The level-3 icosphere (off centre, so that the normalisation does something) fitted with P = 256 primitives of 4^3
    voxels from 2048 candidates, on the GPU and by the restatement in float64 and float32 (computed once, shared)."""
    v, f = MF.icosphere(3, 0.5, (0.1, -0.2, 0.05))
    attr = MF.affine_attr(v)
    mesh = (_dev(v), _dev(f), _dev(attr[:, :3]), _dev(attr[:, 3]), _dev(attr[:, 4]))
    recon, info = fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S, candidates=CAND, seed=3)
    u, lin = fit.surface_uniforms(CAND, 3).numpy(), torch.linspace(-1, 1, S).numpy()
    out = {"recon": recon, "info": info, "v": v, "f": f, "attr": attr, "mesh": mesh}
    for name, dt in (("r64", np.float64), ("r32", np.float32)):
        field = lambda pts, dt=dt: MF.query_threaded(pts, vn, f, attr, dt, block=128, keep_d2=False)   # noqa: E731
        vn = MF.normalize(v)[0]
        out[name], out["rinfo"] = MF.mesh_to_primitives(v, f, attr, u, lin, P, S, dtype=dt, field=field)
    out["cand_sdf"] = MF.sdf_of(MF.query_threaded(out["rinfo"]["cand"], out["rinfo"]["v"], f, None, np.float64, block=128,
                                                  keep_d2=False))
    return out


def test_fit_geometry_is_bit_exact(fit, fitted):
    got, info, ri = fitted["recon"].cpu().numpy(), fitted["info"], fitted["rinfo"]
    assert got.shape == (P, 4 + 6 * S ** 3) and got.dtype == np.float32
    assert np.array_equal(info["v"].cpu().numpy().view(np.uint32), ri["v"].view(np.uint32))
    assert np.array_equal(info["candidates"].cpu().numpy().view(np.uint32), ri["cand"].view(np.uint32))
    assert np.array_equal(info["candidate_face"].cpu().numpy(), ri["cand_face"])
    assert np.array_equal(info["idx"].cpu().numpy(), ri["idx"])
    assert np.array_equal(got[:, :4].view(np.uint32), fitted["r64"][:, :4].astype(np.float32).view(np.uint32))
    assert abs(float(np.abs(ri["v"]).max()) - 0.9) < 1e-6 and (got[:, 0] > 0).all()


def test_fit_payload_is_inside_the_bounds(fit, fitted):
    got, r64, r32 = fitted["recon"].cpu().numpy().astype(np.float64), fitted["r64"], fitted["r32"].astype(np.float64)
    s3 = S ** 3
    floor_sdf = float(np.abs(np.abs(r32[:, 4:4 + s3]) - np.abs(r64[:, 4:4 + s3])).max())
    e_sdf = float(np.abs(np.abs(got[:, 4:4 + s3]) - np.abs(r64[:, 4:4 + s3])).max())
    clear = np.abs(r64[:, 4:4 + s3]) > 4 * floor_sdf
    signs = bool((np.sign(got[:, 4:4 + s3]) == np.sign(r64[:, 4:4 + s3]))[clear].all())
    # attributes: on the face the KERNEL chose (a near-tie between two faces excludes nothing)
    x = fitted["rinfo"]["x"].reshape(-1, 3)
    vn, f, attr = fitted["rinfo"]["v"], fitted["f"], fitted["attr"]
    face = fit.mesh_field_query(_dev(x), _dev(vn), _dev(f), None)[1].cpu().numpy().astype(np.int64)
    a64, a32 = (np.clip(MF.attr_on_face(x, vn, f, attr, face, t), 0, 1) for t in (np.float64, np.float32))
    ga = got[:, 4 + s3:].reshape(P, 5, s3).transpose(0, 2, 1).reshape(-1, 5)
    floor_a, e_a = float(np.abs(a32.astype(np.float64) - a64).max()), float(np.abs(ga - a64).max())
    print(f"fit payload: sdf err {e_sdf:.3e} (fp32 restatement {floor_sdf:.3e}), attr err {e_a:.3e} (fp32 restatement {floor_a:.3e})")
    assert e_sdf <= 4 * floor_sdf and signs and e_a <= 4 * floor_a
    assert (ga >= 0).all() and (ga <= 1).all() and clear.mean() > 0.9


def test_fitted_field_agrees_with_the_mesh_sdf_at_the_candidates(fit, fitted):
    """PrimSDF.from_mesh(...).query at the surface candidates against the true float64 mesh SDF: within 2 x the error of the
    restatement's own primitives through oracle/primsdf_ref.py; every candidate lies inside a primitive."""
    from oracle.primsdf_ref import primsdf_forward
    from topia_xl_amd.primsdf import PrimSDF
    cand, true = torch.from_numpy(fitted["rinfo"]["cand"]), fitted["cand_sdf"]
    r = torch.from_numpy(fitted["r64"]).float()
    w = torch.relu(1 - ((cand[:, None, :] - r[None, :, 1:4]) / r[None, :, 0:1]).abs().amax(-1))
    assert bool((w.sum(1) > 0).all())                         # checked on the restatement, on the CPU
    ref = primsdf_forward(r[:, :4], r[:, 4:], cand, S)["sdf"][:, 0].double().numpy()
    e_ref = float(np.abs(ref - true).max())
    m, info = PrimSDF.from_mesh(fitted["mesh"], num_prims=P, prim_shape=S, candidates=CAND, seed=3, return_info=True)
    assert not m.training and m.srt_param.is_cuda and torch.equal(torch.cat([m.srt_param, m.feat_param], 1), fitted["recon"])
    got = m(cand.to(DEV))["sdf"][:, 0].double().cpu().numpy()
    e_got = float(np.abs(got - true).max())
    print(f"fitted field at the {CAND} candidates: |sdf - mesh sdf| max {e_got:.3e} (restatement through the oracle {e_ref:.3e})")
    assert e_got <= 2 * e_ref


def test_from_mesh_extracts_a_mesh_and_encodes(fit):
    """The shipped payload shape (8^3): extract_mesh(resolution=64) of the fitted field is a non-empty mesh near the sphere."""
    from topia_xl_amd import mesh as M
    from topia_xl_amd.primsdf import PrimSDF
    v, f = MF.icosphere(3)
    attr = MF.affine_attr(v)
    tm = M.TriMesh(_dev(v), _dev(f), _dev(v * 2), _dev(attr[:, :3]), _dev(attr[:, 3]), _dev(attr[:, 4]))
    field = PrimSDF.from_mesh(tm, num_prims=P, prim_shape=8)
    assert field.feat_param.shape == (P, 6 * 512) and bool(torch.isfinite(field.feat_param).all())
    out = M.extract_mesh(field, resolution=64)
    assert out.v.shape[0] > 100 and out.f.shape[0] > 100
    r = out.v.norm(dim=1)
    assert float((r - 0.9).abs().median()) < 0.03             # the normalised sphere has radius 0.9; a lattice cell is 0.03
    with pytest.raises(NotImplementedError, match="training-side"):
        PrimSDF(f_sdf=lambda x: x)


def test_read_ply_returns_what_write_ply_wrote(fit, tmp_path):
    from topia_xl_amd import mesh as M
    from topia_xl_amd import pipeline
    v, f = MF.icosphere(1)
    rng = np.random.default_rng(5)
    alb = (rng.integers(0, 256, (v.shape[0], 3)).astype(np.float32) / np.float32(255.0))
    m = M.TriMesh(*(torch.from_numpy(a) for a in (v, f, rng.standard_normal(v.shape).astype(np.float32), alb,
                                                  rng.random(v.shape[0]).astype(np.float32), rng.random(v.shape[0]).astype(np.float32))))
    path = os.path.join(tmp_path, "m.ply")
    m.write_ply(path)
    back = pipeline.read_ply(path)
    for name in ("v", "f", "normals", "albedo", "roughness", "metallic"):
        a, b = getattr(m, name), getattr(back, name)
        assert a.dtype == b.dtype and a.shape == b.shape and fp.same_bits(a, b), name
    back.write_ply(path + "2")
    assert open(path, "rb").read() == open(path + "2", "rb").read()
    with open(path, "wb") as fh:
        fh.write(b"ply\nformat ascii 1.0\nend_header\n")
    with pytest.raises(ValueError):
        M.read_ply(path)


# ------------------------------------------------------------------------------------------------ footprint
def _in(g, a, name):
    return g.guard_input(_dev(a) if isinstance(a, np.ndarray) else a, name).t


@pytest.mark.parametrize("n,F", [(1, 1), (257, 257), (1000, 549)])
def test_query_footprint(fit, n, F):
    v, f = MF.mesh_with_faces(F)
    p, attr = _points(v, f, 1000, 2)[:n], MF.affine_attr(v)
    out = fp.hold(lambda g: fit.mesh_field_query(_in(g, p, "x"), _in(g, v, "v"), _in(g, f, "f"), _in(g, attr, "attr")))
    assert out[0].shape == (n,) and out[3].shape == (n, 5)


def test_areas_points_fps_footprint(fit):
    v, f = MF.mesh_with_faces(549)
    cdf = np.cumsum(MF.face_areas(v, f))
    u = fit.surface_uniforms(1000, 1).numpy()
    area = fp.hold(lambda g: fit.face_areas(_in(g, v, "v"), _in(g, f, "f")))
    assert area.shape == (549,)
    pts = fp.hold(lambda g: fit.surface_points(_in(g, v, "v"), _in(g, f, "f"), _in(g, cdf, "cdf"), _in(g, u, "u")))
    assert pts[0].shape == (1000, 3)
    for N, K in ((4097, 256), (1000, 1), (2, 2)):
        c = _candidates(N, 1)
        idx, nn = fp.hold(lambda g: fit.fps(_in(g, c, "pts"), K, 1))
        assert idx.shape == (K,) and nn.shape == (K,)


def test_mesh_to_primitives_footprint(fit):
    v, f = MF.icosphere(1)
    attr = MF.affine_attr(v)

    def case(g):
        mesh = (_in(g, v, "v"), _in(g, f, "f"), _in(g, attr[:, :3], "albedo"), _in(g, attr[:, 3], "roughness"),
                _in(g, attr[:, 4], "metallic"))
        recon, info = fit.mesh_to_primitives(mesh, num_prims=33, prim_shape=3, candidates=300)
        return recon, info["candidates"], info["idx"]
    recon = fp.hold(case)[0]
    assert recon.shape == (33, 4 + 6 * 27) and bool(torch.isfinite(recon).all())
