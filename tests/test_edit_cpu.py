"""Editing on the host: tests/edit_ref.py (the restatement the GPU tests compare against) equals the REAL reference's
q_sample / ddim_reverse_sample bit for bit (tests/golden/edit.npz), the two new columns of the coefficient table are the
reverse step's scalars in the reference's float32 arithmetic, and the new API refuses what it cannot do."""
import numpy as np
import pytest
import torch

from oracle import diffusion_ref as dref
from tests import edit_ref as er
from tests.golden.make_golden_edit import STEP_CASES, step_inputs


def test_restatement_equals_the_reference_bit_for_bit(golden):
    """q_sample and the reverse step: ddim5 at (2, 12, 68) - three parameterisations, clip on and off - and ddim25 at
    (1, 8, 68), every step, 0 mismatching elements."""
    g = golden("edit")
    for n, shape, pars, clips in STEP_CASES:
        tab, _ = dref.make("squaredcos_cap_v2", 1000, f"ddim{n}")
        x, mo, noise = step_inputs(n, shape)
        for i in range(n):
            assert np.array_equal(er.q_sample(tab, i, x, noise).numpy(), g[f"q{n}"][i]), (n, i)
            for par in pars:
                for clip in clips:
                    got = er.reverse_step(tab, i, x, mo, par, clip)["sample"].numpy()
                    want = g[f"rev{n}_{par}_clip{int(clip)}"][i]
                    assert np.array_equal(got, want), (n, par, clip, i, int((got != want).sum()))


def test_keep_step_restatement_is_the_two_steps_it_joins():
    tab, _ = dref.make("squaredcos_cap_v2", 1000, "ddim5")
    x, mo, noise = step_inputs(5, (2, 12, 68))
    known, kn = x * 0.5, noise * 2
    keep = torch.zeros(2, 12, dtype=torch.bool)
    keep[0, ::2] = True
    mo = mo.clone()
    mo[0, 0] = float("nan")                                           # a kept row: the model output there is ignored
    for i in (4, 1, 0):
        out = er.keep_step(tab, i, x, mo, known, kn, keep)
        free = dref.ddim_step(tab, i, x, mo)
        held = er.q_sample(tab, i - 1, known, kn) if i else known
        assert torch.equal(out["sample"][keep], held[keep]) and torch.equal(out["pred_xstart"][keep], known[keep])
        assert torch.equal(out["sample"][~keep], free["sample"][~keep]) and bool(torch.isfinite(out["sample"]).all())


@pytest.mark.parametrize("n", [5, 25, 100])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_reverse_columns_of_the_coefficient_table(pkg, n, eta):
    """Columns 14 / 15 = the correctly rounded fp32 square roots of the float32-cast alphas_cumprod_next and of its complement
    (gaussian_diffusion.py:611-614 on a device whose sqrtf is correctly rounded); columns 0..13 are what they were."""
    from topia_xl_amd.diffusion import sampler as S
    assert (S.C_REV_X0, S.C_REV_EPS, S.COEF_STRIDE) == (14, 15, 16)
    d = pkg.create_diffusion(f"ddim{n}", noise_schedule="squaredcos_cap_v2", parameterization="v")
    c = d.step_coefficients(eta)
    assert c.shape == (n, 16) and c.dtype == np.float32
    nxt = torch.from_numpy(np.append(d.alphas_cumprod[1:], 0.0).astype(np.float32))
    assert np.array_equal(c[:, 14], dref._sqrt32(nxt).numpy()) and np.array_equal(c[:, 15], dref._sqrt32(1 - nxt).numpy())
    assert c[n - 1, 14] == 0.0 and c[n - 1, 15] == 1.0
    # columns 0 .. 13 restated independently of the product (test_schedule.py holds 0 .. 12 the same way for its own cases)
    tab, _ = dref.make("squaredcos_cap_v2", 1000, f"ddim{n}")
    sq = dref._sqrt32
    for i in range(n):
        ex = lambda arr: torch.full((1,), float(np.float32(arr[i])))
        abar, abar_prev = ex(tab.acp), ex(tab.acp_prev)
        sigma = eta * sq((1 - abar_prev) / (1 - abar)) * sq(1 - abar / abar_prev)
        want = {0: ex(tab.sqrt_acp), 1: ex(tab.sqrt_1m_acp), 2: ex(tab.sqrt_recip_acp), 3: ex(tab.sqrt_recipm1_acp),
                4: ex(tab.post_c1), 5: ex(tab.post_c2), 6: ex(tab.post_logvar_clipped), 7: ex(np.log(tab.betas)),
                8: torch.zeros(1), 9: sq(abar_prev), 10: sq(1 - abar_prev - sigma ** 2), 11: sigma,
                12: torch.ones(1) * (0.0 if i == 0 else 1.0), 13: torch.zeros(1)}       # 8 / 13: fixed variance, unused by learned-range
        for col, w in want.items():
            assert np.float32(w.item()) == c[i, col] or (np.isnan(w.item()) and np.isnan(c[i, col])), (i, col)


def test_new_api_refuses_what_it_cannot_do(pkg):
    d = pkg.create_diffusion("ddim5", noise_schedule="squaredcos_cap_v2", parameterization="v")
    model = lambda x, t, **kw: torch.cat([x, x], -1)
    x = torch.zeros(1, 4, 2)
    t = torch.zeros(1, dtype=torch.int64)
    # CPU tensors
    with pytest.raises(RuntimeError, match="HIP device"):
        d.q_sample(x, t, x)
    with pytest.raises(RuntimeError, match="HIP device"):
        d.ddim_reverse_sample(model, x, t)
    with pytest.raises(RuntimeError, match="HIP device"):
        d.ddim_reverse_sample_loop(model, x)
    with pytest.raises(RuntimeError, match="HIP device"):
        d.ddim_sample_loop(model, x.shape, noise=x, start_step=2, device="cpu")
    # the reference's assertion, and the hooks
    with pytest.raises(AssertionError, match="deterministic"):
        d.ddim_reverse_sample(model, x, t, eta=0.5)
    with pytest.raises(NotImplementedError):
        d.ddim_reverse_sample(model, x, t, cond_fn=lambda: 0)
    with pytest.raises(NotImplementedError):
        d.ddim_reverse_sample(model, x, t, denoised_fn=lambda v: v)
    # keep / known / known_noise come together
    keep = torch.ones(1, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="together"):
        list(d.ddim_sample_loop_progressive(model, x.shape, noise=x, keep=keep))
    with pytest.raises(ValueError, match="together"):
        d.ddim_sample_loop(model, x.shape, noise=x, known=x, known_noise=x)
    assert "keep" not in d.p_sample_loop.__code__.co_varnames and "start_step" not in d.p_sample_loop.__code__.co_varnames
    # ranges
    for bad in (-1, 5, 7):
        with pytest.raises(ValueError, match="start_step"):
            d.ddim_sample_loop(model, x.shape, noise=x, start_step=bad)
    for start, stop in ((0, 0), (3, 2), (4, None), (0, 6), (-1, 3)):
        with pytest.raises(ValueError, match="start_step"):
            d.ddim_reverse_sample_loop(model, x, start_step=start, stop_step=stop)


def test_redenoise_primitives_refusals_and_keep_mask(pkg):
    from topia_xl_amd import pipeline
    d = pkg.create_diffusion("ddim5", noise_schedule="squaredcos_cap_v2", parameterization="v")
    rp = torch.zeros(1, 4, 4 + 6 * 512)
    keep = torch.ones(1, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="invert"):
        pipeline.redenoise_primitives(rp, None, None, d, None, start_step=3, mode="invert", keep=keep)
    with pytest.raises(ValueError, match="mode"):
        pipeline.redenoise_primitives(rp, None, None, d, None, start_step=3, mode="other")
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="start_step"):
            pipeline.redenoise_primitives(rp, None, None, d, None, start_step=bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        pipeline.redenoise_primitives(rp, None, None, d, None, start_step=3, latent_mean=[0.0] * 68, latent_std=[1.0] * 68)
    m = torch.tensor([[True, False, True]])
    full = pipeline.keep_mask(m)
    assert full.shape == (1, 3, 68) and full.dtype == torch.bool and torch.equal(full.all(-1), m) and torch.equal(full.any(-1), m)
    srt, lat = pipeline.keep_mask(m, "srt"), pipeline.keep_mask(m, "latent")
    assert bool(srt[0, 0, :4].all()) and not bool(srt[0, 0, 4:].any()) and not bool(srt[0, 1].any())
    assert torch.equal(srt | lat, full) and not bool((srt & lat).any())
    with pytest.raises(ValueError):
        pipeline.keep_mask(m, "xyz")
    with pytest.raises(ValueError):
        pipeline.keep_mask(m.float())
