"""DPM-Solver++(2M) on the host: the 2M coefficient table is the DDIM table except where k != 0, and there only in columns 9
and 11; k equals the float64 restatement (tests/dpm_ref.py); the table form `DDIM + k (x0 - x0_prev)` is the exponential-
integrator form; the float32 restatement of the kernel's step converges on the closed-form denoiser as the issue states and
follows the float64 loop to float32 rounding."""
import numpy as np
import pytest

from oracle import diffusion_ref as dref
from tests import dpm_ref as R

SCHEDULES = ("squaredcos_cap_v2", "linear")
SHAPE = (2, 97, 68)


def _proc(pkg, schedule, n, par="v"):
    d = pkg.create_diffusion(f"ddim{n}", noise_schedule=schedule, parameterization=par)
    tab, _ = dref.make(schedule, 1000, f"ddim{n}")
    return d, tab


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("n", [5, 10, 25])
def test_first_order_rows_are_the_ddim_rows(pkg, schedule, n):
    """order = 1: the whole table; order = 2: row 0, the rows below lower_order_final, row first_step and the last row - bit
    for bit step_coefficients(0.0).  No column other than 9 and 11 is ever touched, and both are touched where k != 0."""
    d, _ = _proc(pkg, schedule, n)
    ddim = d.step_coefficients(0.0)
    assert _same_bits(d.dpm_solver_coefficients(order=1), ddim)
    assert _same_bits(d.dpm_solver_coefficients(order=1, lower_order_final=1, first_step=2), ddim)
    for lof in (1, 2, 3):
        for first in (None, n - 1, n - 2, 2, 0):
            t = d.dpm_solver_coefficients(order=2, lower_order_final=lof, first_step=first)
            assert t.shape == ddim.shape and t.dtype == np.float32
            first_row = n - 1 if first is None else first
            plain = sorted({0, first_row, n - 1} | set(range(min(lof, n))))
            assert _same_bits(t[plain], ddim[plain]), (lof, first)
            others = [c for c in range(16) if c not in (9, 11)]
            assert _same_bits(t[:, others], ddim[:, others]), (lof, first)
            second = [i for i in range(n) if i not in plain]
            assert (t[second, 11] < 0).all() and (t[second, 9] > ddim[second, 9]).all(), (lof, first)
            assert (ddim[:, 11] == 0).all()
    assert _same_bits(d.dpm_solver_coefficients(), d.dpm_solver_coefficients(2, 2, n - 1))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("n", [5, 10, 25])
def test_k_and_table_equal_the_restatement(pkg, schedule, n):
    """k to 1e-12 relative against tests/dpm_ref.py (a) (float64, an independent schedule); columns 9 / 11 are
    float32(float64(col 9) + k) and float32(-k); the restatement's own table (b) has the same bits in every column it fills."""
    d, tab = _proc(pkg, schedule, n)
    for lof, first in ((2, None), (1, None), (2, n - 2), (1, 2)):
        k = d.dpm_solver_k(2, lof, first)
        want = R.k_all(tab.acp, tab.acp_prev, 2, lof, first)
        assert k.dtype == np.float64 and ((k == 0) == (want == 0)).all()
        on = want != 0
        assert on.sum() == n - 2 - (lof - 1) - (0 if first in (None, 0) or first < lof else 1)
        rel = np.abs(k[on] - want[on]) / np.abs(want[on])
        assert (rel <= 1e-12).all(), rel.max()
        assert (want[on] > 0).all()
        t, ddim = d.dpm_solver_coefficients(2, lof, first), d.step_coefficients(0.0)
        assert _same_bits(t[on, 9], (ddim[on, 9].astype(np.float64) + k[on]).astype(np.float32))
        assert _same_bits(t[on, 11], (-k[on]).astype(np.float32))
        mine = R.table32(tab, want)
        cols = [0, 1, 2, 3, 9, 10, 11, 12]
        assert _same_bits(mine[:, cols], t[:, cols]), (lof, first)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_table_form_is_the_exponential_integrator_form(schedule):
    """float64, random operands, every second-order row of ddim5 / ddim10 / ddim25: DDIM + k (x0 - x0_prev) equals
    (sigma_next / sigma_t) x - alpha_next expm1(-h) D to 1e-12 of the operands' scale."""
    g = np.random.default_rng(3)
    for n in (5, 10, 25):
        tab, _ = dref.make(schedule, 1000, f"ddim{n}")
        for i in range(1, n - 1):
            x, x0, x0p = g.standard_normal((3, 64)) * 3
            a = R.ddim64(x, x0, tab.acp[i], tab.acp_prev[i]) + R.k_of(tab.acp, tab.acp_prev, i) * (x0 - x0p)
            b = R.step64(x, x0, x0p, tab.acp, tab.acp_prev, i)
            scale = max(1.0, float(np.abs(b).max()))
            assert float(np.abs(a - b).max()) <= 1e-12 * scale, (n, i)


def test_refusals(pkg):
    d, _ = _proc(pkg, "squaredcos_cap_v2", 5)
    for order in (0, 3, 2.5, None):
        with pytest.raises(ValueError, match="order"):
            d.dpm_solver_coefficients(order=order)
    for lof in (0, -1):
        with pytest.raises(ValueError, match="lower_order_final"):
            d.dpm_solver_coefficients(lower_order_final=lof)
    for first in (-1, 5):
        with pytest.raises(ValueError, match="first_step"):
            d.dpm_solver_coefficients(first_step=first)
    import torch
    model = lambda x, t, **kw: torch.cat([x, x], -1)
    x = torch.zeros(1, 4, 2)
    with pytest.raises(ValueError, match="order"):
        d.dpm_solver_sample_loop(model, x.shape, noise=x, order=3)
    with pytest.raises(ValueError, match="lower_order_final"):
        d.dpm_solver_sample_loop(model, x.shape, noise=x, lower_order_final=0)
    with pytest.raises(ValueError, match="start_step"):
        d.dpm_solver_sample_loop(model, x.shape, noise=x, start_step=5)
    with pytest.raises(ValueError, match="together"):
        d.dpm_solver_sample_loop(model, x.shape, noise=x, keep=torch.ones(1, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError):
        d.dpm_solver_sample_loop(model, x.shape, noise=x, cond_fn=lambda: 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        d.dpm_solver_sample_loop(model, x.shape, noise=x)
    assert "eta" not in d.dpm_solver_sample_loop.__code__.co_varnames


def closed_form_error(tab, n, order, par, seed=5, lower_order_final=2):
    """RMS error against the exact ODE solution of a whole loop of the float32 restatement (b) on the closed-form denoiser."""
    mu, s, xT = R.gaussian_data(seed, SHAPE)
    den = {"eps": R.denoiser_eps, "v": R.denoiser_v}[par]
    model = lambda x, i: den(x.astype(np.float64), tab.acp[i], mu, s).astype(np.float32)
    table = R.table32(tab, R.k_all(tab.acp, tab.acp_prev, order, lower_order_final))
    final = R.loop32(model, xT.astype(np.float32), table, range(n - 1, -1, -1), R.MEAN[par], False)[-1][0]
    return R.rms(final, R.exact_solution(xT.astype(np.float32).astype(np.float64), tab.acp[n - 1], mu, s))


@pytest.mark.parametrize("par", ["v", "eps"])
def test_convergence_on_the_closed_form_denoiser(par):
    """(2, 97, 68), seed 5, through the restatement (b).  Cosine: 2M(ddim10) <= 0.5 DDIM(ddim10) and 2M(ddim12) <= 0.75
    DDIM(ddim25); linear: 2M(ddim10) <= 0.8 DDIM(ddim10).  Measured: 0.31, 0.49, 0.61 for both parameterisations.  And the
    finding behind the default: on linear ddim10, lower_order_final = 1 ends worse than DDIM itself."""
    err = {}
    for schedule in SCHEDULES:
        for n in (10, 12, 25):
            tab, _ = dref.make(schedule, 1000, f"ddim{n}")
            for order in (1, 2):
                err[schedule, n, order] = closed_form_error(tab, n, order, par)
    for key, e in err.items():
        print(f"closed form {par} {key[0]} ddim{key[1]} order {key[2]}: rms {e:.4f}")
    cos, lin = SCHEDULES
    ratios = (err[cos, 10, 2] / err[cos, 10, 1], err[cos, 12, 2] / err[cos, 25, 1], err[lin, 10, 2] / err[lin, 10, 1])
    print(f"ratios {par}: " + " ".join(f"{r:.3f}" for r in ratios))
    assert ratios[0] <= 0.5 and ratios[1] <= 0.75 and ratios[2] <= 0.8, ratios
    tab, _ = dref.make(lin, 1000, "ddim10")
    lof1 = closed_form_error(tab, 10, 2, par, lower_order_final=1)
    print(f"linear ddim10 2M lower_order_final=1: rms {lof1:.4f}")
    assert lof1 > err[lin, 10, 1]


@pytest.mark.parametrize("clip,bound", [(False, 8.7e-6), (True, 3.5e-5)])
def test_float32_restatement_follows_the_float64_loop(clip, bound):
    """(b) against (a) over a whole ddim25 loop on stored random model outputs (v, c_out = 2C), every step's sample and x0:
    the largest difference relative to the largest magnitude of the step's float64 values.  Measured 2.16e-6 without clipping
    and 8.75e-6 with it (the clamp takes x0 off the trajectory, and the last steps' division by sqrt(1 / acp - 1) << 1 then
    amplifies what the earlier steps rounded); each is asserted at four times its figure.  The bound is the float32 rounding
    of one restatement against the other in float64 - a ~10-operation step of 6e-8 per operation, carried through 25 steps -
    and is not measured on the code under test."""
    n = 25
    tab, _ = dref.make("squaredcos_cap_v2", 1000, f"ddim{n}")
    g = np.random.default_rng(11)
    x = g.standard_normal(SHAPE).astype(np.float32)
    mos = [g.standard_normal(SHAPE[:2] + (136,)).astype(np.float32) for _ in range(n)]
    k = R.k_all(tab.acp, tab.acp_prev)
    steps = range(n - 1, -1, -1)
    a = R.loop32(mos, x, R.table32(tab, k), steps, 2, clip)
    b = R.loop64(mos, x, tab.acp, tab.acp_prev, k, steps, 2, clip)
    worst = 0.0
    for (s32, x32), (s64, x64) in zip(a, b):
        for u, v in ((s32, s64), (x32, x64)):
            worst = max(worst, float(np.abs(u - v).max() / np.abs(v).max()))
    print(f"float32 restatement against float64 over ddim25, clip {clip}: largest relative difference {worst:.3e}")
    assert worst <= bound
