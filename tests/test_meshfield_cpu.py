"""The restatement of primitive fitting (tests/meshfield_numpy.py) held to closed forms, in float64: the GPU tests compare
the kernels with it, so it is checked here against things that do not share its code.  (No goldens from the reference exist
for this step: its PrimSDF._init_param is an empty `pass`.)"""
import numpy as np
import torch

from tests import meshfield_numpy as MF

TOL = 1e-12


def _pts(n=400, seed=0, lim=0.8):
    return np.random.default_rng(seed).uniform(-lim, lim, (n, 3))


def test_box_sdf_is_the_closed_form():
    v, f = MF.box()
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    p = np.concatenate([_pts(), (lo + hi)[None] / 2, lo[None], ((lo + hi) / 2 + [0, 0, (hi - lo)[2] / 2])[None]])
    q = MF.query(p, v, f)
    d = np.abs(p - (lo + hi) / 2) - (hi - lo) / 2
    ref = np.linalg.norm(np.maximum(d, 0), axis=1) + np.minimum(d.max(1), 0)
    on = np.abs(ref) < TOL                                   # on the surface the sign is the winding number's to choose
    assert np.abs(np.abs(q["dist"]) - np.abs(ref)).max() <= TOL
    assert np.abs(MF.sdf_of(q) - ref)[~on].max() <= TOL and (~on).sum() >= 400


def test_winding_number_is_one_inside_and_zero_outside():
    for v, f, inside in ((*MF.box(), None), (*MF.icosphere(2), 0.5)):
        p = _pts(300, 3, 0.6)
        q = MF.query(p, v, f)
        if inside is None:
            lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
            m = ((p > lo) & (p < hi)).all(1)
        else:
            r = np.linalg.norm(p, axis=1)
            keep = (r < 0.5 * 0.93) | (r > 0.5)               # between the inscribed and the circumscribed sphere: either
            p, q, m = p[keep], {k: x[keep] for k, x in q.items()}, r[keep] < 0.5 * 0.93
        assert m.sum() > 10 and (~m).sum() > 10
        assert np.abs(q["wn"] - m).max() <= TOL


def test_open_hemisphere_has_a_fractional_winding_number():
    v, f = MF.hemisphere(2)
    q = MF.query(np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0], [0.0, 0.0, -2.0]]), v, f)
    assert 0.3 < q["wn"][0] < 0.7 and abs(q["wn"][1]) < 0.1 and abs(q["wn"][2]) < 0.1


def test_zero_area_faces_are_their_longest_edge_or_point_and_add_nothing_to_wn():
    v, f = MF.box()
    extra = np.array([[0.5, 0.5, 0.5], [0.75, 0.25, 0.625], [0.625, 0.375, 0.5625]], np.float32)   # exact: the third is the midpoint
    v2 = np.concatenate([v, extra])
    deg = np.array([[8, 8, 9], [8, 9, 8], [9, 8, 8], [8, 10, 9], [10, 10, 10], [8, 8, 9], [10, 8, 9]], np.int32)   # segments, a point, a repeat
    f2 = np.concatenate([f[:5], deg, f[5:]]).astype(np.int32)
    p = np.concatenate([_pts(200, 5), extra.astype(np.float64), [[0.6, 0.4, 0.55]]])
    q, q0 = MF.query(p, v2, f2), MF.query(p, v, f)
    a, b = extra[0].astype(np.float64), extra[1].astype(np.float64)
    t = np.clip((p - a) @ (b - a) / ((b - a) @ (b - a)), 0, 1)
    seg = np.linalg.norm(p - (a + t[:, None] * (b - a)), axis=1)
    assert np.abs(q["dist"] - np.minimum(q0["dist"], seg)).max() <= TOL
    assert np.abs(q["wn"] - q0["wn"]).max() <= TOL and np.isfinite(q["d2"]).all()
    kinds = [MF.face_kind(*(tuple(x) for x in v2[f2[5 + k]].astype(np.float64))) for k in range(7)]
    assert kinds == [2, 1, 1, 2, 1, 2, 3]                    # the longest edge, the first of equals (ab, ac, bc); a point is ab
    pt = MF.query(p, v2, deg[4:5])                           # the point alone
    assert np.abs(pt["dist"] - np.linalg.norm(p - extra[2].astype(np.float64), axis=1)).max() <= TOL and (pt["wn"] == 0).all()
    # attributes on a degenerate face: interpolated along the segment
    attr = MF.affine_attr(v2)
    got = MF.attr_on_face(p, v2, f2, attr, np.full(p.shape[0], 8))          # face a, m, b -> the segment a b
    ref = attr[8].astype(np.float64) * (1 - t)[:, None] + attr[9].astype(np.float64) * t[:, None]
    assert np.abs(got - ref).max() <= TOL


def test_attributes_are_barycentric_at_the_closest_point():
    v, f = MF.icosphere(1)
    rng = np.random.default_rng(2)
    A, b = rng.uniform(-1, 1, (3, 5)), rng.uniform(-1, 1, 5)
    attr = v.astype(np.float64) @ A + b                       # affine and unclipped: interpolation reproduces it at q
    p = _pts(200, 9)
    q = MF.query(p, v, f, attr)
    t = q["face"]
    a, ab, ac = (v[f[t, 0]].astype(np.float64), v[f[t, 1]].astype(np.float64) - v[f[t, 0]], v[f[t, 2]].astype(np.float64) - v[f[t, 0]])
    n = np.cross(ab, ac)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    # the closest point lies on the face's plane at distance dist from p, and attr(q) = A q + b there
    assert np.abs(q["d2"].min(1) - q["dist"] ** 2).max() <= TOL
    inplane = np.abs(np.abs(((p - a) * n).sum(1)) - q["dist"]) < 1e-9       # face-region points: q = p - ((p - a).n) n
    qq = p - ((p - a) * n).sum(1)[:, None] * n
    assert inplane.sum() > 20 and np.abs(q["attr"] - (qq @ A + b))[inplane].max() <= 1e-11


def test_areas_and_surface_points():
    v, f = MF.box()
    area = MF.face_areas(v, f)
    ext = v.astype(np.float64).max(0) - v.astype(np.float64).min(0)
    assert abs(area.sum() - 2 * (ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0])) <= TOL
    f2 = np.concatenate([f[:3], [[0, 0, 1]], f[3:]]).astype(np.int32)         # a zero-area face is never chosen
    cdf = np.cumsum(MF.face_areas(v, f2))
    u = np.random.default_rng(0).random((2000, 3)).astype(np.float32)
    u[:4, 0] = [0.0, np.float32(1) - np.float32(2) ** -24, 0.5, 0.25]
    pts, face = MF.surface_points(v, f2, cdf, u)
    assert pts.dtype == np.float32 and (face != 3).all() and face[0] == 0 and face[1] == f2.shape[0] - 1
    assert MF.query(pts, v, f2)["dist"].max() < 1e-6
    share = np.bincount(face, minlength=f2.shape[0]) / 2000.0
    assert np.abs(share - MF.face_areas(v, f2) / cdf[-1]).max() < 0.04


def test_fps_breaks_ties_to_the_lowest_index():
    pts = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 0.5, 0]], np.float32)
    idx, nn = MF.fps(pts, 5, 0)
    assert idx.tolist() == [0, 1, 2, 4, 0]                   # 1 before its copy 3 and before 2; then 4; then all minima are 0
    assert nn.tolist() == [0.0, 1.0, 1.0, 0.5, 0.0]          # centre 0 was chosen twice: its nearest other centre is itself
    idx, nn = MF.fps(pts, 1, 3)
    assert idx.tolist() == [3] and nn.tolist() == [0.0]
    idx, _ = MF.fps(pts, 3, 4)
    assert idx.tolist() == [4, 1, 2]


def test_payload_layout_matches_the_primsdf_oracle():
    """The oracle's query (oracle/primsdf_ref.py) at a primitive's own voxel positions returns the stored values wherever one
    primitive covers: the [sdf | rgb | roughness, metallic] x [z][y][x] layout is the one PrimSDF reads."""
    from oracle.primsdf_ref import primsdf_forward
    v, f = MF.icosphere(1, 0.5, (0.1, -0.05, 0.2))
    attr = MF.affine_attr(v)
    P, S = 8, 4
    from topia_xl_amd import fit
    u, lin = fit.surface_uniforms(64, 1).numpy(), torch.linspace(-1, 1, S).numpy()
    rp, info = MF.mesh_to_primitives(v, f, attr, u, lin, P, S)
    assert rp.shape == (P, 4 + 6 * S ** 3) and np.isfinite(rp).all()
    srt, feat = torch.from_numpy(rp[:, :4]).float(), torch.from_numpy(rp[:, 4:]).float()
    x = torch.from_numpy(info["x"].reshape(-1, 3))
    out = primsdf_forward(srt, feat, x, S)
    sp = (x[:, None, :] - srt[None, :, 1:4]) / srt[None, :, 0:1]
    w = torch.relu(1 - sp.abs().amax(-1))
    own = torch.arange(P).repeat_interleave(S ** 3)
    one = ((w > 0).sum(1) == 1) & (w[torch.arange(x.shape[0]), own] > 0.5)
    assert int(one.sum()) >= 8
    stored = torch.from_numpy(rp[:, 4:].reshape(P, 6, S ** 3)).float().permute(0, 2, 1).reshape(-1, 6)
    got = torch.cat([out["sdf"], out["tex"], out["mat"]], 1)
    k = (w.sum(1, keepdim=True) + 1e-6) / w.sum(1, keepdim=True).clamp_min(1e-3)   # undo the oracle's 1e-6 in the weight sum
    assert float(((got * k - stored)[one]).abs().max()) < 1e-5
    assert float((stored[:, 1] - stored[:, 2]).abs().max()) > 0.05                # channels and axes are distinguishable
    # every candidate lies strictly inside some primitive's cube (FPS: covering radius <= centre separation <= every nn)
    c = torch.from_numpy(info["cand"])
    wc = torch.relu(1 - ((c[:, None, :] - srt[None, :, 1:4]) / srt[None, :, 0:1]).abs().amax(-1))
    assert bool((wc.sum(1) > 0).all())


def test_normalize_puts_the_longest_half_side_at_the_extent():
    v, _ = MF.box()
    vn, c, s = MF.normalize(v, 0.9)
    assert vn.dtype == np.float32 and abs(np.abs(vn).max() - 0.9) < 1e-6 and np.abs(vn.max(0) + vn.min(0)).max() < 1e-6
