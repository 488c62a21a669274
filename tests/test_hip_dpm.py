"""GPU tests of DPM-Solver++(2M) on the fused DDIM step: order 1 is the DDIM loop bit for bit; every step of an order-2 loop
is the float32 restatement (tests/dpm_ref.py) bit for bit; the closed-form denoiser converges on the device as on the host;
partial and masked loops; timestep planning and the fold guard; pipeline.redenoise_primitives(sampler="dpm").

Figures that are printed and not asserted (a tiny DiT with random weights) are recorded in DESIGN.md "Few-step sampling"."""
import gc
import warnings

import numpy as np
import pytest
import torch

from oracle import diffusion_ref as dref
from oracle import synth
from tests import dpm_ref as R
from tests import test_hip_dit as TD
from tests.golden.make_golden import SEED, VAE_CFG
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
SMALL, BIG = (2, 97, 68), (2, 4096, 68)      # odd rows, no multiple of the block; 557 056 elements > 2048 x 256 threads of a launch
COS, LIN = "squaredcos_cap_v2", "linear"


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd
    return topia_xl_amd


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


class Stored:
    """A model that returns stored tensors, one per call in order (`again()` rewinds)."""

    def __init__(self, outs):
        self.outs, self.pos = outs, 0

    def again(self):
        self.pos = 0
        return self

    def __call__(self, x, t, **kw):
        self.pos += 1
        return self.outs[self.pos - 1]


def _stored(seed, n, shape, dtype, c_out=None):
    B, N, C = shape
    return [synth.tensor(seed, f"mo{j}", (B, N, c_out or 2 * C)).to(dtype) for j in range(n)]


def _same_items(a, b):
    assert len(a) == len(b)
    for j, (u, v) in enumerate(zip(a, b)):
        assert set(u) == {"sample", "pred_xstart"}
        assert torch.equal(u["sample"], v["sample"]) and torch.equal(u["pred_xstart"], v["pred_xstart"]), j


# ------------------------------------------------------------------------------------------------ order 1
@pytest.mark.parametrize("par", ["eps", "xstart", "v"])
def test_order_1_is_the_ddim_loop(pkg, par):
    """dpm_solver_sample_loop(order=1) against ddim_sample_loop(eta=0): the sample and every yielded pred_xstart, bit for bit,
    for fp16 / bf16 / fp32 model outputs and clip on and off (ddim5, stored model outputs)."""
    d = pkg.create_diffusion("ddim5", noise_schedule=COS, parameterization=par)
    x = synth.tensor(61, "x", SMALL).to(DEV)
    for dt in (F16, BF16, F32):
        m = Stored([o.to(DEV) for o in _stored(61, 5, SMALL, dt)])
        for clip in (False, True):
            want = list(d.ddim_sample_loop_progressive(m.again(), SMALL, noise=x, clip_denoised=clip, eta=0.0))
            got = list(d.dpm_solver_sample_loop_progressive(m.again(), SMALL, noise=x, clip_denoised=clip, order=1))
            _same_items(got, want)
            assert torch.equal(d.dpm_solver_sample_loop(m.again(), SMALL, noise=x, clip_denoised=clip, order=1), want[-1]["sample"])


# ------------------------------------------------------------------------------------------------ order 2
def _against_restatement(pkg, schedule, n, shape, par, dt, clip, learn_sigma, start=None, lof=2):
    d = pkg.create_diffusion(f"ddim{n}", noise_schedule=schedule, parameterization=par, learn_sigma=learn_sigma)
    tab, _ = dref.make(schedule, 1000, f"ddim{n}")
    steps = list(range(n - 1 if start is None else start, -1, -1))
    x = synth.tensor(62, "x", shape)
    mos = _stored(62, len(steps), shape, dt, None if learn_sigma else shape[2])
    table = R.table32(tab, R.k_all(tab.acp, tab.acp_prev, 2, lof, steps[0]))
    ref = R.loop32([o.float().numpy() for o in mos], x.numpy(), table, steps, R.MEAN[par], clip)
    got = list(d.dpm_solver_sample_loop_progressive(Stored([o.to(DEV) for o in mos]), shape, noise=x.to(DEV), clip_denoised=clip,
                                                    lower_order_final=lof, start_step=start))
    assert len(got) == len(ref)
    for j, (g, (s, x0)) in enumerate(zip(got, ref)):
        assert np.array_equal(g["pred_xstart"].cpu().numpy(), x0), (n, par, dt, clip, j)
        assert np.array_equal(g["sample"].cpu().numpy(), s), (n, par, dt, clip, j)
    return d, got, x, mos


@pytest.mark.parametrize("n", [5, 25])
@pytest.mark.parametrize("clip", [False, True])
def test_order_2_is_the_restatement_at_every_step(pkg, n, clip):
    """Every step of a ddim5 and a ddim25 loop at (2, 97, 68), fed the same stored model outputs as the restatement (b):
    sample and pred_xstart bit for bit.  v with fp16 outputs and c_out = 2C (the shipped configuration), eps with fp32
    outputs and c_out = C, x0-prediction with bf16; the linear schedule; lower_order_final = 1."""
    d, got, x, mos = _against_restatement(pkg, COS, n, SMALL, "v", F16, clip, True)
    _against_restatement(pkg, COS, n, SMALL, "eps", F32, clip, False)
    _against_restatement(pkg, LIN, n, SMALL, "xstart", BF16, clip, True)
    _against_restatement(pkg, LIN, n, SMALL, "v", F16, clip, False, lof=1)
    # and it is not the DDIM loop: the second-order rows moved the sample
    ddim = d.ddim_sample_loop(Stored([o.to(DEV) for o in mos]), SMALL, noise=x.to(DEV), clip_denoised=clip)
    assert not torch.equal(ddim, got[-1]["sample"])


def test_order_2_grid_stride_wraps(pkg):
    """(2, 4096, 68): more elements than one launch has threads - the grid-stride loop takes a second trip with a history."""
    _against_restatement(pkg, COS, 5, BIG, "v", F16, True, True)


# ------------------------------------------------------------------------------------------------ convergence
def _device_error(pkg, schedule, n, order, par="v"):
    d = pkg.create_diffusion(f"ddim{n}", noise_schedule=schedule, parameterization=par)
    tab, tmap = dref.make(schedule, 1000, f"ddim{n}")
    mu, s, xT = (torch.from_numpy(a).to(DEV) for a in R.gaussian_data(5, SMALL))
    acp_of_t = torch.zeros(1000, dtype=torch.float64, device=DEV)
    acp_of_t[torch.tensor(tmap, device=DEV)] = torch.from_numpy(tab.acp).to(DEV)

    def model(x, t, **kw):          # tests/dpm_ref.py denoiser_v / denoiser_eps in torch, float64, no read-back
        a2 = acp_of_t[t][:, None, None]
        x = x.double()
        x0 = mu + a2.sqrt() * s * s * (x - a2.sqrt() * mu) / (a2 * s * s + (1 - a2))
        eps = (x - a2.sqrt() * x0) / (1 - a2).sqrt()
        out = eps if par == "eps" else a2.sqrt() * eps - (1 - a2).sqrt() * x0
        return torch.cat([out, torch.zeros_like(out)], -1).float()

    x = xT.float()
    final = d.dpm_solver_sample_loop(model, SMALL, noise=x, clip_denoised=False, order=order)
    if order == 1:
        assert torch.equal(final, d.ddim_sample_loop(model, SMALL, noise=x, clip_denoised=False))
    exact = R.exact_solution(x.double().cpu().numpy(), tab.acp[n - 1], mu.cpu().numpy(), s.cpu().numpy())
    return R.rms(final.cpu().numpy(), exact)


def test_convergence_on_the_closed_form_denoiser(pkg):
    """The three conditions of tests/test_dpm_cpu.py on the device, the denoiser a torch callable, (2, 97, 68), seed 5: cosine
    2M(ddim10) <= 0.5 DDIM(ddim10), 2M(ddim12) <= 0.75 DDIM(ddim25); linear 2M(ddim10) <= 0.8 DDIM(ddim10)."""
    e = {(sch, n, o): _device_error(pkg, sch, n, o) for sch, n, o in
         ((COS, 10, 1), (COS, 10, 2), (COS, 12, 2), (COS, 25, 1), (LIN, 10, 1), (LIN, 10, 2))}
    for key, v in e.items():
        print(f"closed form on the device, {key[0]} ddim{key[1]} order {key[2]}: rms {v:.4f}")
    ratios = (e[COS, 10, 2] / e[COS, 10, 1], e[COS, 12, 2] / e[COS, 25, 1], e[LIN, 10, 2] / e[LIN, 10, 1])
    print("ratios: " + " ".join(f"{r:.3f}" for r in ratios))
    assert ratios[0] <= 0.5 and ratios[1] <= 0.75 and ratios[2] <= 0.8, ratios


# ------------------------------------------------------------------------------------------------ partial and masked loops
def test_partial_loop_starts_without_history(pkg):
    """start_step = 12 of ddim25: the first step is the DDIM step bit for bit (row 12 of that loop's table has k = 0) and the
    whole loop is the restatement's with first_step = 12; the full loop's row 12 is second-order, so the tables differ."""
    d, got, x, mos = _against_restatement(pkg, COS, 25, SMALL, "v", F16, False, True, start=12)
    assert len(got) == 13
    first = next(iter(d.ddim_sample_loop_progressive(Stored([mos[0].to(DEV)]), SMALL, noise=x.to(DEV), clip_denoised=False,
                                                     start_step=12)))
    assert torch.equal(first["sample"], got[0]["sample"]) and torch.equal(first["pred_xstart"], got[0]["pred_xstart"])
    assert d.dpm_solver_coefficients()[12, 11] != 0 and d.dpm_solver_coefficients(first_step=12)[12, 11] == 0


@pytest.mark.parametrize("per_element", [False, True])
def test_masked_loop(pkg, per_element):
    """keep all false: the unmasked 2M loop bit for bit.  With a mask: kept elements are q_sample(known, known_noise, level) at
    every step and `known` at the end, bit for bit, whatever the model returned there (NaN / inf: neither the model output nor
    the history is read at a kept element); the free elements, whose stored model outputs are the unmasked loop's, are the
    unmasked loop's."""
    n, start = 25, 12
    d = pkg.create_diffusion(f"ddim{n}", noise_schedule=COS, parameterization="v")
    steps = list(range(start, -1, -1))
    x, known, kn = (synth.tensor(63, s, SMALL).to(DEV) for s in ("x", "known", "kn"))
    mos = [o.to(DEV) for o in _stored(63, len(steps), SMALL, F16)]
    kw = dict(noise=x, clip_denoised=False, start_step=start)
    plain = list(d.dpm_solver_sample_loop_progressive(Stored(mos), SMALL, **kw))
    none = torch.zeros(SMALL if per_element else SMALL[:2], dtype=torch.bool, device=DEV)
    _same_items(list(d.dpm_solver_sample_loop_progressive(Stored(mos), SMALL, known=known, keep=none, known_noise=kn, **kw)), plain)
    g = torch.Generator().manual_seed(6)
    keep = (torch.rand(SMALL if per_element else SMALL[:2], generator=g) < 0.5).to(DEV)
    full = keep if per_element else keep[..., None].expand(SMALL)
    bad = []
    for j, o in enumerate(mos):
        o = o.clone()
        o[torch.cat([full, full], -1)] = (float("nan"), float("inf"), float("-inf"))[j % 3]
        bad.append(o)
    got = list(d.dpm_solver_sample_loop_progressive(Stored(bad), SMALL, known=known, keep=keep, known_noise=kn, **kw))
    assert len(got) == len(steps)
    for item, i, ref in zip(got, steps, plain):
        level = d.q_sample(known, torch.full((SMALL[0],), i - 1, dtype=torch.int64, device=DEV), kn) if i else known
        assert torch.equal(item["sample"][full], level[full]) and torch.equal(item["pred_xstart"][full], known[full]), i
        assert torch.equal(item["sample"][~full], ref["sample"][~full]) and torch.equal(item["pred_xstart"][~full], ref["pred_xstart"][~full]), i
        assert bool(torch.isfinite(item["sample"]).all()) and bool(torch.isfinite(item["pred_xstart"]).all()), i
    assert torch.equal(got[-1]["sample"][full], known[full]) and 0.4 < float(full.float().mean()) < 0.6


# ------------------------------------------------------------------------------------------------ planner, tiny real DiT
def test_tiny_dit_loop_is_planned_and_cleared(pkg):
    """A ddim10 2M loop over the tiny DiT of tests/test_hip_dit.py under forward_with_cfg: ten rows are planned, in loop order,
    and the plan is dropped afterwards - also when the consumer abandons the generator.  The sample is finite.

    Printed, not asserted (random weights under CFG 6 are no denoiser): rel-L2 against DDIM at ddim250 from the same noise.
    Measured on an MI355X: 2M at ddim10 0.187, ddim12 0.142, ddim15 0.147, DDIM at ddim25 0.098 (DESIGN.md "Few-step sampling")."""
    name, sd, heads, m, x, y, t = TD._case(pkg, 1)
    kw = dict(y=y.to(DEV), cfg_scale=6.0, precision_dtype=F16, enable_amp=True)
    xd = x.to(DEV)
    proc = lambda n: pkg.create_diffusion(f"ddim{n}", noise_schedule=COS, parameterization="v")
    d = proc(10)
    plans = []
    real = m.plan_timesteps
    m.plan_timesteps = lambda ts: (plans.append(ts.tolist()), real(ts))[1]
    try:
        gen = d.dpm_solver_sample_loop_progressive(m.forward_with_cfg, x.shape, noise=xd, clip_denoised=False, model_kwargs=kw)
        first = next(gen)
        assert m._t_plan is not None and m._t_plan["t"].numel() == 10
        rest = list(gen)
        assert m._t_plan is None and len(rest) == 9
        assert plans == [list(d.timestep_map)]
        final = rest[-1]["sample"]
        assert bool(torch.isfinite(final).all()) and bool(torch.isfinite(first["pred_xstart"]).all())
        assert torch.equal(final, d.dpm_solver_sample_loop(m.forward_with_cfg, x.shape, noise=xd, clip_denoised=False, model_kwargs=kw))
        gen = d.dpm_solver_sample_loop_progressive(m.forward_with_cfg, x.shape, noise=xd, clip_denoised=False, model_kwargs=kw,
                                                   start_step=6)
        next(gen)
        assert m._t_plan is not None and m._t_plan["t"].tolist() == [d.timestep_map[i] for i in range(6, -1, -1)]
        gen.close()
        assert m._t_plan is None
    finally:
        del m.plan_timesteps
    fine = proc(250).ddim_sample_loop(m.forward_with_cfg, x.shape, noise=xd, clip_denoised=False, model_kwargs=kw)
    figures = {f"2M ddim{n}": rel_l2(proc(n).dpm_solver_sample_loop(m.forward_with_cfg, x.shape, noise=xd, clip_denoised=False,
                                                                    model_kwargs=kw), fine) for n in (10, 12, 15)}
    figures["DDIM ddim25"] = rel_l2(proc(25).ddim_sample_loop(m.forward_with_cfg, x.shape, noise=xd, clip_denoised=False,
                                                              model_kwargs=kw), fine)
    print("tiny DiT, rel-L2 against DDIM ddim250: " + ", ".join(f"{k} {v:.3e}" for k, v in figures.items()))


# ------------------------------------------------------------------------------------------------ fold guard
def test_fold_guard_repeats_the_loop_without_history(pkg):
    """A stand-in planner whose fold_overflowed says yes once: the loop is run again with the fold off, from the first step and
    without the first run's history, and its sample is what a fresh 2M loop with the fold off returns.  The stand-in's output
    depends on fold_ln, so the first run's history is not the second's."""

    class Model:
        def __init__(self, fold):
            self.fold_ln, self.calls, self.asked = fold, [], 0

        def plan_timesteps(self, ts):
            pass

        def select_planned_timestep(self, row):
            pass

        def clear_timestep_plan(self):
            pass

        def fold_overflowed(self, sample):
            self.asked += 1
            return self.fold_ln and self.asked == 1

        def __call__(self, x, t, **kw):
            self.calls.append(bool(self.fold_ln))
            return torch.cat([(0.3 if self.fold_ln else 0.1) * x, torch.zeros_like(x)], -1).half()

    d = pkg.create_diffusion("ddim10", noise_schedule=COS, parameterization="v")
    shape = (1, 16, 68)
    x = synth.tensor(64, "x", shape).to(DEV)
    m = Model(True)
    with pytest.warns(RuntimeWarning, match="LayerNorm fold"):
        items = list(d.dpm_solver_sample_loop_progressive(m, shape, noise=x))
    assert len(items) == 10 and m.calls == [True] * 10 + [False] * 10 and m.fold_ln is True and m.asked == 1
    m2 = Model(False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want = d.dpm_solver_sample_loop(m2, shape, noise=x)
        ddim = d.ddim_sample_loop(Model(False), shape, noise=x)
    assert torch.equal(items[-1]["sample"], want) and m2.calls == [False] * 10
    assert not torch.equal(want, ddim)                                    # second-order steps were taken
    assert not torch.equal(items[0]["sample"], next(iter(d.dpm_solver_sample_loop_progressive(Model(False), shape, noise=x)))["sample"])


# ------------------------------------------------------------------------------------------------ redenoise_primitives
def test_redenoise_primitives_with_the_2m_sampler(pkg):
    """Tiny VAE + tiny DiT, 2 x 128 primitives, ddim10, start_step = 6, half of the primitives kept: the kept ones come out as
    the encode -> decode round trip of the input, bit for bit - the property the DDIM path documents; the others change, and
    differ from the DDIM path's."""
    from topia_xl_amd import pipeline
    name, sd, heads, m, x, y, t = TD._case(pkg, 1)
    vae = pkg.VAE(**VAE_CFG).eval()
    vae.load_state_dict(synth.state_dict_like(SEED, vae.state_dict()), strict=True)
    vae.to(DEV)
    B, N = 2, 128
    d = pkg.create_diffusion("ddim10", noise_schedule=COS, parameterization="v")
    mean, std = synth.tensor(41, "mean", (68,), 0.5).tolist(), synth.tensor(41, "std", (68,), 0.2, 1.0).abs().tolist()
    stats = dict(latent_mean=mean, latent_std=std, latent_nf=1.1)
    rp = pipeline.latents_to_primitives(synth.tensor(42, "edit.tokens", (B, N, 68)).to(DEV), vae, mean, std, 1.1)
    yy = synth.tensor(SEED, name + ".y2", (B,) + tuple(y.shape[1:])).to(DEV)
    tokens = pipeline.primitives_to_latents(rp, vae, mean, std, 1.1)
    trip = pipeline.latents_to_primitives(tokens, vae, mean, std, 1.1)
    keep = (torch.rand(B, N, generator=torch.Generator().manual_seed(1)) < 0.5).to(DEV)
    noise = torch.randn(tokens.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    out = pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=6, keep=keep, noise=noise, sampler="dpm", **stats)
    assert out.shape == rp.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert torch.equal(out[keep], trip[keep])
    assert bool((out[~keep] != trip[~keep]).any(-1).all())
    same_draw = pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=6, keep=keep, sampler="dpm",
                                              generator=torch.Generator(device=DEV).manual_seed(9), **stats)
    assert torch.equal(same_draw, out)                                    # the generator is used as the DDIM path uses it
    ddim = pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=6, keep=keep, noise=noise, **stats)
    assert torch.equal(ddim[keep], out[keep]) and not torch.equal(ddim[~keep], out[~keep])
    assert torch.equal(ddim, pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=6, keep=keep, noise=noise, sampler="ddim",
                                                           **stats))
    with pytest.raises(ValueError, match="sampler"):
        pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=6, sampler="euler", **stats)
