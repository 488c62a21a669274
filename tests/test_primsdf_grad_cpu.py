"""tests/primsdf_grad_ref.py without a GPU: the restated field's autograd against the real reference's gradients
(tests/golden/primsdf_grad.npz), the restated Adam step against torch.optim.Adam, the restated refinement loop on an icosphere,
and the closure of the stream-order table once the cases of tests/test_hip_primsdf_grad.py are registered."""
import os

import numpy as np
import torch

from tests import primsdf_grad_ref as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "primsdf_grad.npz")


def test_restated_gradients_match_the_reference_module_in_float64():
    """models/primsdf.py in .train().double() (index_add of grid_sample, weights normalised first) against the restatement
    (explicit corners, the sum normalised afterwards): the same function, so the gradients differ by float64 rounding.  A weight
    w = 1 - m / |s| carries an absolute error of one float64 ulp of 1 (2.2e-16); weights go down to ~1e-7 at the rim of a
    primitive, where inv = 1 / (w + 1e-6) turns that into a relative error of ~1e-10 of the entry: the bound is 1e-9 of each
    tensor's largest magnitude."""
    from tests.golden.make_golden import PRIMSDF_CFG, primsdf_params
    z = np.load(GOLDEN)
    srt, feat, pts = (t.double() for t in primsdf_params())
    S = PRIMSDF_CFG["prim_shape"]
    assert not bool(G.kinks(pts, srt, feat, S, 1e-9).any())          # the comparison is of smooth points only
    gs, gf = G.grads(pts, srt, feat, torch.from_numpy(z["gout"]), S)
    for name, got, ref in (("srt", gs.numpy(), z["srt_grad"]), ("feat", gf.numpy()[::2], z["feat_grad_even"]),
                           ("feat row sums", gf.numpy().sum(1), z["feat_grad_rowsum"])):
        err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        print(f"restatement vs reference, {name}: max-abs error {err:.3e} of {top:.3e}")
        assert top > 0 and err <= 1e-9 * top, (name, err, top)


def test_restated_adam_matches_torch_optim_adam():
    """Three steps of torch.optim.Adam (CPU, fp32) against the fp32 numpy restatement.  torch evaluates the same formulas with
    other roundings (lerp and addcmul may fuse a multiply-add), each worth an ulp or two of its operands:
    v (a sum of positive terms) within 8 ulps of itself; m = m + w1 (g - m) can cancel, so within 8 ulps of |m_prev| + |g|;
    the parameter within one ulp of itself plus the update's error.  The update is (lr / bc1) m / denom with bc1 >= 0.1,
    denom >= max |g| / sqrt(3) over the steps so far and an error of m of at most 16 ulps of max |g|: 300 ulps of lr."""
    gen = torch.Generator().manual_seed(5)
    n, lr = 2000, 1e-2
    p0 = torch.randn(n, generator=gen)
    scale = 10.0 ** torch.randint(-4, 2, (n,), generator=gen).float()      # gradient magnitudes 1e-4 .. 10, fixed per element
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    q, m, v = p0.numpy().copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    ulp = float(np.finfo(np.float32).eps)
    for t in range(1, 4):
        g = torch.randn(n, generator=gen) * scale
        p.grad = g.clone()
        opt.step()
        m_prev = m
        q, m, v = G.adam_step(q, g.numpy(), m, v, t, lr)
        st = opt.state[p]
        assert np.all(np.abs(m - st["exp_avg"].numpy()) <= 8 * ulp * (np.abs(m_prev) + np.abs(g.numpy())))
        assert np.all(np.abs(v - st["exp_avg_sq"].numpy()) <= 8 * ulp * np.abs(v))
        assert np.all(np.abs(q - p.detach().numpy()) <= ulp * np.abs(q) + 300 * ulp * lr)
    assert float(np.abs(q - p0.numpy()).max()) > 1e-3                 # (the three steps moved the parameters)


def test_restated_refinement_lowers_its_loss_on_an_icosphere():
    recon, target, pts = G.icosphere_problem()
    assert recon.shape == (33, 4 + 6 * 27) and pts.shape == (33 * 64, 3)
    out, loss = G.refine(recon, target, pts, 20, 3, dtype=torch.float64)
    print("restated refinement, float64, loss per step:", " ".join(f"{x:.4e}" for x in loss))
    assert len(loss) == 20 and all(np.isfinite(loss)) and loss[-1] < loss[0]
    assert bool(torch.isfinite(out).all()) and float(out[:, 0].min()) >= G.SCALE_FLOOR
    frozen, loss_f = G.refine(recon, target, pts, 5, 3, refine_srt=False, dtype=torch.float64)
    assert torch.equal(frozen[:, :4], torch.as_tensor(recon).double()[:, :4]) and loss_f[-1] < loss_f[0]


def test_stream_table_is_closed_with_the_refinement_cases():
    """tests/test_hip_streams.py may not be edited, so tests/test_hip_primsdf_grad.py registers its cases in that table when it is
    imported.  With both modules imported the closure of tests/test_streamorder_cpu.py holds: every prototype of the header
    that takes a `void* stream` is declared by a case, and nothing else is."""
    from tests import test_hip_primsdf_grad as TG
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    for name in TG.STREAM_CASES:
        assert name in TS.CASES
    assert {"primx_primsdf_query_backward", "primx_adam_step"} <= set(TS.declared())
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n in TG.STREAM_CASES]      # they run in their own module, not twice
