"""PrimSDF field query (csrc/primsdf.hip) against a float64 restatement of models/primsdf.py with a derived per-element
bound, plus designs whose exact value does not depend on grid_sample's rounding.  Also latent_denorm, which writes the
srt these kernels consume, bit for bit against torch's fp32 arithmetic."""
import math

import numpy as np
import pytest
import torch

DEV = "cuda:0"
U = 2.0 ** -24
EPS = float(np.float32(1e-6))     # the normaliser's epsilon as the fp32 kernel (and the fp32 reference module) hold it


def ref64(srt, feat, x, S, training=False, exact_w=False):
    """float64 PrimSDF.forward on fp32 inputs -> (out [n, 6] before the fill, bound [n, 6], covered [n]).
    w_i = relu(1 - ||x - pos_i||_inf / |s_i|) (the reference's ||(x - pos) / s||_inf), sampled at (x - pos_i) / s_i
    (signed), trilinear with align_corners.  Bound of the fp32 kernel: dx and the division round (w within 4u, the grid
    coordinate within 4u (S - 1) per axis), 8 fp32 weights / lerps (10u of sum |q| w), the sums over covering primitives
    (n_cov u), the normalisation (2u).  exact_w: the inputs make every weight exact in fp32 (x - pos, m / |s| and
    1 - m / |s| round to themselves), so the weights' rounding drops out of the bound."""
    srt, feat, x = (t.double() for t in (srt, feat, x))
    P, C = srt.shape[0], feat.shape[1] // S ** 3
    s, pos = srt[:, 0], srt[:, 1:4]
    d = x[:, None, :] - pos[None]                                                  # [n, P, 3]
    m = d.abs().amax(-1)
    w = torch.clamp(1.0 - m / s.abs()[None], min=0.0)
    cov = w > 0
    vol = feat.reshape(P, C, S, S, S)
    n = x.shape[0]
    acc = torch.zeros(n, C, dtype=torch.float64)
    eacc = torch.zeros(n, C, dtype=torch.float64)
    ew = torch.zeros(n, dtype=torch.float64)
    ii, pp = cov.nonzero(as_tuple=True)
    if ii.numel():
        g = (d[ii, pp] / s[pp, None] + 1.0) * 0.5 * (S - 1)                          # x -> W, y -> H, z -> D
        i0 = torch.clamp(torch.floor(g).long(), 0, S - 2)
        f = g - i0
        val = torch.zeros(ii.shape[0], C, dtype=torch.float64)
        qabs = torch.zeros_like(val)
        qs = []
        for c in range(8):
            bx, by, bz = c & 1, (c >> 1) & 1, c >> 2
            wt = (f[:, 0] if bx else 1 - f[:, 0]) * (f[:, 1] if by else 1 - f[:, 1]) * (f[:, 2] if bz else 1 - f[:, 2])
            q = vol[pp, :, i0[:, 2] + bz, i0[:, 1] + by, i0[:, 0] + bx]
            val += q * wt[:, None]
            qabs += q.abs() * wt[:, None]
            qs.append(q)
        qs = torch.stack(qs)
        qd = qs.amax(0) - qs.amin(0)
        wv = w[ii, pp]
        e_s = U * (10 * qabs + 12 * (S - 1) * qd)
        acc.index_add_(0, ii, wv[:, None] * val)
        ew_i = 0.0 if exact_w else 4 * U
        eacc.index_add_(0, ii, wv[:, None] * e_s + ew_i * val.abs() + 4 * U * (wv[:, None] * val).abs())
        ew.index_add_(0, ii, torch.full_like(wv, ew_i))
    ncov = cov.sum(1).double()
    W = w.sum(1)
    eacc = eacc + ncov[:, None] * U * acc.abs()
    ew = ew + ncov * U * W
    out = acc / (W + EPS)[:, None]
    bound = eacc / (W + EPS)[:, None] + out.abs() * (ew / (W + EPS) + 3 * U)[:, None] + 1e-30
    return out, bound, W > 0


def fill_options(srt, feat, x, S, tol=5e-7):
    """Eval-mode fill of an uncovered point: every (primitive, grid node) whose float64 distance is within `tol` of the
    minimum - the primitive's centre distance, and per axis the node offset - in the reference's preference order (first
    primitive index, first flattened local_grid index = z-major [z][y][x]).  tol covers the fp32 kernel's rounding of
    coordinates <= 1 (x - pos, pos + s lin[k] and the sums: ~1.2e-7), so a near-tie below fp32 resolution admits both
    choices.  -> list of (value, p, node) per point."""
    srt, feat, x = (t.double() for t in (srt, feat, x))
    s, pos = srt[:, 0], srt[:, 1:4]
    lin = torch.linspace(-1, 1, S).double()
    outs = []
    for i in range(x.shape[0]):
        dist = ((x[i] - pos) ** 2).sum(-1).sqrt()
        cand = (dist <= dist.min() + tol).nonzero()[:, 0]
        opts = []
        for p in cand.tolist():
            node = pos[p][None, :] + s[p] * lin[:, None]                           # [S, 3]: per-axis coordinates
            e = (x[i][None, :] - node).abs()
            e2 = e ** 2
            ax = [(e[:, a] <= e[:, a].min() + tol).nonzero()[:, 0].tolist() for a in range(3)]
            for kz in ax[2]:
                for ky in ax[1]:
                    for kx in ax[0]:
                        dd = math.sqrt(float(e2[kx, 0] + e2[ky, 1] + e2[kz, 2]))
                        v = float(feat[p, (kz * S + ky) * S + kx])
                        opts.append((v + dd * float(np.sign(v)), p, (kz, ky, kx)))
        outs.append(opts)
    return outs


def _query(srt, feat, x, S, training=False):
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd.primsdf import PrimSDF
    m = PrimSDF(num_prims=srt.shape[0], prim_shape=S)
    m.srt_param.data, m.feat_param.data = srt.clone(), feat.clone()
    m.to(DEV).train(training)
    return m.query(x.to(DEV)).cpu().double()


def _check_fill(got, srt, feat, x, S, cov, exact_ties=0):
    """Uncovered points (eval mode): the sdf is one of fill_options' choices, the first one for the first `exact_ties`
    points (exact ties on representable coordinates take the reference's first index); other channels are 0."""
    idx = (~cov).nonzero()[:, 0]
    opts = fill_options(srt, feat, x[idx], S)
    for i, o in zip(idx.tolist(), opts):
        g = float(got[i, 0])
        vals = [v for v, _, _ in o] if i >= exact_ties else [o[0][0]]
        assert min(abs(g - v) - 4e-7 * (1 + abs(v)) for v in vals) <= 0, (i, g, o[:3])
    assert bool((got[idx, 1:] == 0).all())
    return idx.numel()


def _check_weighted(name, srt, feat, x, S):
    got = _query(srt, feat, x, S)
    out, bnd, cov = ref64(srt, feat, x, S)
    exp = out.clone()
    exp[:, 1:] = exp[:, 1:].clamp(0, 1)
    err = (got - exp).abs()[cov]
    share = float((err / bnd[cov]).max()) if cov.any() else 0.0
    print(f"{name}: {int(cov.sum())} covered of {x.shape[0]}, max err {float(err.max()) if cov.any() else 0:.2e}, "
          f"largest bound share {share:.3f}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bnd[cov]).all()), (name, share)
    return got, cov


def _prims(gen, P, S, lo=0.05, hi=0.2, spread=0.8):
    srt = torch.cat([lo + (hi - lo) * torch.rand(P, 1, generator=gen), spread * (2 * torch.rand(P, 3, generator=gen) - 1)], 1)
    feat = torch.randn(P, 6 * S ** 3, generator=gen) * 0.5 + 0.3
    return srt, feat


@pytest.mark.gpu
@pytest.mark.parametrize("P,n", [(1, 1), (255, 255), (1023, 257), (1024, 255), (1025, 257), (3000, 257)])
def test_hip_query_chunk_edges_random_features(P, n):
    """Covering primitives at indices 1023, 1024 and P - 1 (the LDS chunk is 1024), ragged point counts."""
    gen = torch.Generator().manual_seed(P * 7 + n)
    S = 8
    srt, feat = _prims(gen, P, S, lo=0.01, hi=0.03)
    x = 1.6 * torch.rand(n, 3, generator=gen) - 0.8
    for j, p in enumerate(q for q in (1023, 1024, P - 1) if q < P):               # a point well inside each of them
        srt[p, 0] = 0.3
        srt[p, 1:4] = x[j] + 0.05 * (j + 1)
    got, cov = _check_weighted(f"P={P} n={n}", srt, feat, x, S)
    # the fill's nearest primitive is tracked across the 1024-primitive chunks
    assert _check_fill(got, srt, feat, x, S, cov) == int((~cov).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 3, 8, 16])
def test_hip_query_grid_sizes_overlaps_and_clipping(S):
    """Random features spread beyond [0, 1] (the clip of tex / mat), overlapping identical primitives."""
    gen = torch.Generator().manual_seed(100 + S)
    srt, feat = _prims(gen, 64, S, lo=0.1, hi=0.4, spread=0.5)
    feat = feat * 3.0
    srt[32:40] = srt[24:32]                                                          # identical pairs
    feat[32:40] = feat[24:32]
    x = torch.cat([srt[24:40, 1:4] + 0.03 * torch.randn(16, 3, generator=gen), 1.2 * torch.rand(300, 3, generator=gen) - 0.6])
    got, cov = _check_weighted(f"S={S}", srt, feat, x, S)
    assert float(got[cov][:, 1:].min()) == 0.0 and float(got[cov][:, 1:].max()) == 1.0   # the clip is exercised


@pytest.mark.gpu
def test_hip_query_constant_channel_is_the_weight_sum():
    """Channel 0 == 1 everywhere: the output is W / (W + 1e-6) exactly (trilinear of a constant), exposing the weight sum."""
    gen = torch.Generator().manual_seed(21)
    S = 8
    srt, feat = _prims(gen, 1500, S, lo=0.05, hi=0.3)
    feat[:, :S ** 3] = 1.0
    x = 1.6 * torch.rand(2000, 3, generator=gen) - 0.8
    got = _query(srt, feat, x, S, training=True)
    out, bnd, cov = ref64(srt, feat, x, S)
    s, pos = srt[:, 0].double(), srt[:, 1:4].double()
    W = torch.clamp(1 - (x.double()[:, None] - pos[None]).abs().amax(-1) / s[None], min=0).sum(1)
    exact = W / (W + EPS)
    err = (got[:, 0] - exact).abs()
    assert bool((err <= bnd[:, 0]).all()), float((err / bnd[:, 0]).max())
    assert float(exact.max()) > 0.99 and bool((got[~cov] == 0).all())             # training mode: no fill, zeros


@pytest.mark.gpu
def test_hip_query_linear_fields():
    """Features linear in the local node coordinates, f_c(u) = a_c + b_c . u: trilinear reproduces them exactly, so the
    expected value is the closed float64 sum over covering primitives of w_i f_c((x - pos_i) / s_i) / (W + 1e-6)."""
    gen = torch.Generator().manual_seed(22)
    S, P = 5, 300
    srt, _ = _prims(gen, P, S, lo=0.05, hi=0.3)
    lin = torch.linspace(-1, 1, S).double()
    uz, uy, ux = torch.meshgrid(lin, lin, lin, indexing="ij")
    a = torch.randn(P, 6, 1, generator=gen).double()
    b = torch.randn(P, 6, 3, generator=gen).double() * 0.3
    feat = (a + b[..., 0:1] * ux.reshape(1, 1, -1) + b[..., 1:2] * uy.reshape(1, 1, -1) + b[..., 2:3] * uz.reshape(1, 1, -1))
    feat = feat.reshape(P, -1).float()
    x = 1.6 * torch.rand(1500, 3, generator=gen) - 0.8
    got = _query(srt, feat, x, S)
    _, bnd, cov = ref64(srt, feat, x, S)
    s, pos = srt[:, 0].double(), srt[:, 1:4].double()
    u = (x.double()[:, None] - pos[None]) / s[None, :, None]
    w = torch.clamp(1 - u.abs().amax(-1), min=0)
    val = a[None, :, :, 0] + (b[None] * u[:, :, None, :]).sum(-1)                    # [n, P, 6]
    exp = (w[..., None] * val).sum(1) / (w.sum(1) + EPS)[:, None]
    exp[:, 1:] = exp[:, 1:].clamp(0, 1)
    # the float32 cast of the node values moves each by <= u |f|: add it to the bound
    slack = (w[..., None] * val.abs()).sum(1) / (w.sum(1) + EPS)[:, None] * 2 * U
    err = (got - exp).abs()[cov]
    assert bool((err <= (bnd + slack)[cov]).all()), float((err / (bnd + slack)[cov]).max())
    assert int(cov.sum()) > 500


@pytest.mark.gpu
def test_hip_query_faces_and_negative_scale():
    """Points exactly on a face (|dx| = s: weight 0, not covered) and one ulp inside; a negative scale acts as |s| for the
    weight (the reference's ||(x - pos) / s||_inf) and samples at the signed (x - pos) / s."""
    S = 4
    gen = torch.Generator().manual_seed(23)
    srt = torch.tensor([[0.25, 0.0, 0.0, 0.0], [-0.25, 0.5, 0.0, 0.0]])
    feat = torch.rand(2, 6 * S ** 3, generator=gen)
    inside = float(np.nextafter(np.float32(0.25), np.float32(0)))                   # one ulp inside the face of prim 0
    inside1 = float(np.nextafter(np.float32(0.75), np.float32(0)))                  # one ulp inside the face of prim 1
    x = torch.tensor([[0.25, 0.0, 0.0], [inside, 0.0, 0.0], [0.5 + 0.25, 0.1, 0.0], [inside1, 0.0, -0.1],
                      [0.55, 0.05, -0.02], [0.45, -0.1, 0.2]])
    got = _query(srt, feat, x, S, training=True)
    out, bnd, cov = ref64(srt, feat, x, S)
    assert cov.tolist() == [False, True, False, True, True, True]
    exp = out.clone()
    exp[:, 1:] = exp[:, 1:].clamp(0, 1)
    assert bool(((got - exp).abs() <= bnd).all()), (got, exp)
    assert bool((got[~cov] == 0).all())
    # one ulp inside: the weight is exactly 2^-24 (prim 0) / 2^-22 (prim 1) in fp32, the output w f / (w + 1e-6) is held
    # to a bound without the weight's rounding - tight enough that dropping the point (0) fails
    one = torch.tensor([1, 3])
    out1, bnd1, cov1 = ref64(srt, feat, x[one], S, exact_w=True)
    exp1 = out1.clone()
    exp1[:, 1:] = exp1[:, 1:].clamp(0, 1)
    W1 = torch.clamp(1 - (x[one].double()[:, None] - srt[None, :, 1:4].double()).abs().amax(-1) / srt[None, :, 0].double().abs(),
                     min=0).sum(1)
    assert W1.tolist() == [2.0 ** -24, 2.0 ** -22] and bool(cov1.all())
    assert bool((bnd1 < 0.01 * exp1.abs()).all()), (bnd1, exp1)
    assert bool(((got[one] - exp1).abs() <= bnd1).all()), (got[one], exp1, bnd1)


@pytest.mark.gpu
def test_hip_query_fill_path():
    """Eval mode, points no primitive covers: the nearest primitive and nearest grid node against the float64 argmin.
    Exact ties (representable coordinates) must take the reference's first index; near-ties below fp32 resolution may
    take either, but the value must be that choice's; sign(0) gives sdf 0."""
    S = 4
    gen = torch.Generator().manual_seed(24)
    srt = torch.tensor([[0.125, -0.5, 0.0, 0.0], [0.125, 0.5, 0.0, 0.0], [0.25, 0.0, 0.5, 0.0], [0.125, 0.0, 0.0, 0.75]])
    feat = torch.randn(4, 6 * S ** 3, generator=gen)
    feat[3, :S ** 3] = 0.0                                                          # sign(0): sdf 0
    # the first two are equidistant from prims 0, 1 and 2 (prim 0 must win); prim 2 is strictly nearest to the third
    ties = torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, -0.25], [0.0, 0.125, 0.0]])
    near = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 0.95]])                        # nearest is prim 3 (sdf 0)
    rnd = 2.0 * torch.rand(200, 3, generator=gen) - 1.0
    x = torch.cat([ties, near, rnd])
    full = _query(srt, feat, x, S)
    got = full[:, 0]
    _, _, cov = ref64(srt, feat, x, S)
    assert _check_fill(full, srt, feat, x, S, cov, exact_ties=ties.shape[0] + near.shape[0]) > 100
    assert float(got[ties.shape[0]]) == 0.0 and float(got[ties.shape[0] + 1]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 255, 257, 4099])
def test_hip_latent_denorm_bitwise(rows):
    """v = x / nf * std + mean per channel, split into srt (first 4 channels) and z: bitwise equal to torch's fp32
    x / nf * std + mean (the kernel has contraction off), at ragged row counts."""
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    gen = torch.Generator().manual_seed(rows)
    C = 68
    x = torch.randn(2, rows, C, generator=gen) * 3
    mean = torch.randn(C, generator=gen)
    std = torch.rand(C, generator=gen) + 0.1
    nf = 0.7371
    srt, z = ops.latent_denorm(x.to(DEV), mean.to(DEV), std.to(DEV), nf, 4)
    ref = x / nf * std + mean
    assert srt.shape == (2, rows, 4) and z.shape == (2, rows, C - 4)
    assert torch.equal(srt.cpu(), ref[..., :4]) and torch.equal(z.cpu(), ref[..., 4:])


def test_ref64_matches_oracle_on_golden(golden):
    """The float64 restatement agrees with the oracle (pinned to the real module) on the golden's covered points."""
    from oracle import primsdf_ref
    from tests.golden.make_golden import PRIMSDF_CFG, primsdf_params
    srt, feat, pts = primsdf_params()
    S = PRIMSDF_CFG["prim_shape"]
    out, bnd, cov = ref64(srt, feat, pts, S, training=True)
    ref = primsdf_ref.primsdf_forward(srt, feat, pts, S, training=True)
    r = torch.cat([ref["sdf"], ref["tex"], ref["mat"]], 1).double()
    exp = out.clone()
    exp[:, 1:] = exp[:, 1:].clamp(0, 1)
    # both are fp32 evaluations under the same error model: each within `bnd` of the exact value (a point whose weight
    # sum is comparable to the 1e-6 epsilon amplifies the rounding of W, and the bound says by how much)
    assert bool(((exp - r).abs() <= 2 * bnd + 1e-7)[cov].all()) and int(cov.sum()) > 10
    opts = fill_options(srt, feat, pts[~cov][:50], S)
    ev = primsdf_ref.primsdf_forward(srt, feat, pts[~cov][:50], S, training=False)["sdf"][:, 0]
    for i, o in enumerate(opts):
        assert min(abs(float(ev[i]) - v) for v, _, _ in o) < 1e-5
