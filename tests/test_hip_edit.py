"""GPU tests of editing: primx_q_sample, primx_diffusion_reverse_step and primx_diffusion_step_keep bit for bit against
tests/edit_ref.py and the REAL reference (tests/golden/edit.npz); the reverse, partial and masked loops, their timestep
planning and their overflow guard; the tiny real DiT's inversion / re-denoise trajectories against the reference in fp32;
pipeline.redenoise_primitives end to end; the three entry points between guards (tests/footprint.py).

Every comparison with a tolerance prints its measured figure; those of an MI355X run are in the docstring of
test_real_dit_trajectories_against_reference and in DESIGN.md "Editing"."""
import gc
import warnings

import numpy as np
import pytest
import torch

from oracle import diffusion_ref as dref
from oracle import synth
from tests import edit_ref as er
from tests import footprint as fp
from tests import test_hip_dit as TD
from tests.golden.make_golden import SEED, VAE_CFG
from tests.golden.make_golden_edit import STEP_CASES, dit_noise, step_inputs
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
MEAN = {"eps": 0, "xstart": 1, "v": 2}
SMALL, BIG = (2, 97, 68), (2, 4096, 68)      # odd rows, no multiple of the block; 557 056 elements > 2048 x 256 threads of a launch


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


@pytest.fixture(scope="module")
def pkg(ops):
    import topia_xl_amd
    return topia_xl_amd


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _proc(pkg, n, par="v", eta=0.0):
    d = pkg.create_diffusion(f"ddim{n}", noise_schedule="squaredcos_cap_v2", parameterization=par)
    tab, tmap = dref.make("squaredcos_cap_v2", 1000, f"ddim{n}")
    return d, tab, tmap, torch.from_numpy(d.step_coefficients(eta)).to(DEV)


def _operands(seed, shape):
    B, N, C = shape
    return (synth.tensor(seed, "x", shape), synth.tensor(seed, "mo", (B, N, 2 * C)), synth.tensor(seed, "noise", shape))


# ------------------------------------------------------------------------------------------------ q_sample, reverse step
@pytest.mark.parametrize("n,steps", [(5, (0, 1, 2, 3, 4)), (25, (0, 1, 12, 23, 24))])
def test_q_sample_and_reverse_step_bit_exact(ops, pkg, n, steps):
    """Bit for bit against the restatement at (2, 97, 68): fp16 / bf16 / fp32 model output, three mean types, clip on and off."""
    x, mo, noise = _operands(11, SMALL)
    xd, nd = x.to(DEV), noise.to(DEV)
    for par in ("v", "eps", "xstart"):
        d, tab, _, coef = _proc(pkg, n, par)
        for i in steps:
            if par == "v":
                assert torch.equal(ops.q_sample(xd, nd, coef, i).cpu(), er.q_sample(tab, i, x, noise)), (n, i)
            for dt in (F16, BF16, F32):
                mod = mo.to(dt).to(DEV)
                for clip in (False, True):
                    ref = er.reverse_step(tab, i, x, mo.to(dt), par, clip)
                    s, x0 = ops.diffusion_reverse_step(xd, mod, coef, i, mean_type=MEAN[par], clip_denoised=clip)
                    assert torch.equal(x0.cpu(), ref["pred_xstart"].float()), (n, par, i, dt, clip)
                    assert torch.equal(s.cpu(), ref["sample"]), (n, par, i, dt, clip)
                    if dt == F32 and not clip:     # a model output without the variance channels (c_out = C) reads the same columns
                        s1, _ = ops.diffusion_reverse_step(xd, mod[..., :68].contiguous(), coef, i, mean_type=MEAN[par], clip_denoised=clip)
                        assert torch.equal(s1, s)


def test_q_sample_and_reverse_step_grid_stride_wraps(ops, pkg):
    """(2, 4096, 68): more elements than one launch has threads - the grid-stride loop takes a second trip."""
    x, mo, noise = _operands(12, BIG)
    d, tab, _, coef = _proc(pkg, 25)
    assert torch.equal(ops.q_sample(x.to(DEV), noise.to(DEV), coef, 12).cpu(), er.q_sample(tab, 12, x, noise))
    mo16 = mo.to(F16)
    ref = er.reverse_step(tab, 12, x, mo16, "v", True)
    s, x0 = ops.diffusion_reverse_step(x.to(DEV), mo16.to(DEV), coef, 12, mean_type=2, clip_denoised=True)
    assert torch.equal(s.cpu(), ref["sample"]) and torch.equal(x0.cpu(), ref["pred_xstart"])


def test_q_sample_and_reverse_step_against_the_reference(ops, pkg, golden):
    """The kernels against the REAL reference's recorded outputs, bit for bit, at the goldens' own shapes; through the
    sampler's methods with the reference's signatures."""
    g = golden("edit")
    for n, shape, pars, clips in STEP_CASES:
        x, mo, noise = step_inputs(n, shape)
        xd, mod, nd = x.to(DEV), mo.to(DEV), noise.to(DEV)
        for par in pars:
            d = pkg.create_diffusion(f"ddim{n}", noise_schedule="squaredcos_cap_v2", parameterization=par)
            for i in range(n):
                t = torch.full((shape[0],), i, dtype=torch.int64, device=DEV)
                if par == pars[0]:
                    assert np.array_equal(d.q_sample(xd, t, nd).cpu().numpy(), g[f"q{n}"][i]), (n, i)
                for clip in clips:
                    out = d.ddim_reverse_sample(lambda x_, t_, **kw: mod, xd, t, clip_denoised=clip)
                    assert set(out) == {"sample", "pred_xstart"}
                    assert np.array_equal(out["sample"].cpu().numpy(), g[f"rev{n}_{par}_clip{int(clip)}"][i]), (n, par, clip, i)
    d = pkg.create_diffusion("ddim5", noise_schedule="squaredcos_cap_v2", parameterization="v")
    x = synth.tensor(13, "x", (2, 8, 68)).to(DEV)
    torch.manual_seed(3)
    a = d.q_sample(x, torch.full((2,), 3, dtype=torch.int64, device=DEV))          # noise=None draws randn_like
    torch.manual_seed(3)
    assert torch.equal(a, d.q_sample(x, torch.full((2,), 3, dtype=torch.int64, device=DEV), torch.randn_like(x)))
    with pytest.raises(ValueError):
        d.q_sample(x, torch.full((2,), 5, dtype=torch.int64, device=DEV))
    with pytest.raises(NotImplementedError):
        d.q_sample(x, torch.tensor([1, 2], device=DEV))


# ------------------------------------------------------------------------------------------------ the keep step
def _keep(shape, per_element, seed):
    g = torch.Generator().manual_seed(seed)
    B, N, C = shape
    keep = torch.rand((B, N, C) if per_element else (B, N), generator=g) < 0.5
    keep[0, 0], keep[0, 1] = True, False                             # one all-kept row, one all-free row
    return keep


@pytest.mark.parametrize("shape", [SMALL, BIG])
@pytest.mark.parametrize("per_element", [False, True])
def test_keep_step(ops, pkg, shape, per_element):
    """Flag 0: torch.equal to ops.diffusion_step on the same inputs.  Flag set: pred_xstart = known and the sample is
    ops.q_sample(known, known_noise, step - 1), `known` at step 0 - finite even where the model output is NaN / inf."""
    n = 25
    x, mo, noise = _operands(21, shape)
    known, kn = synth.tensor(21, "known", shape, 0.7), synth.tensor(21, "kn", shape)
    keep = _keep(shape, per_element, 5)
    full = keep if per_element else keep[..., None].expand(shape)
    assert 0.4 < float(full.float().mean()) < 0.6
    mo = mo.to(F16)
    bad = mo.clone()
    badmask = torch.cat([full, full], -1)
    bad[badmask] = torch.tensor([float("nan"), float("inf"), float("-inf")], dtype=F16)[torch.arange(int(badmask.sum())) % 3]
    xd, nd, kd, knd, keepd, fulld = (a.to(DEV) for a in (x, noise, known, kn, keep, full))
    ku8 = keepd.view(torch.uint8)
    for eta in (0.0, 0.5):
        d, tab, _, coef = _proc(pkg, n, "v", eta)
        for i in (n - 1, 1, 0):
            kw = dict(mean_type=2, var_type=3, ancestral=False, clip_denoised=bool(i % 2), noise=nd if eta else None)
            free_s, free_x0 = ops.diffusion_step(xd, mo.to(DEV), coef, i, **kw)
            held = ops.q_sample(kd, knd, coef, i - 1) if i else kd
            for m in (mo, bad):
                s, x0 = ops.diffusion_step_keep(xd, m.to(DEV), coef, i, known=kd, known_noise=knd, keep=ku8, **kw)
                assert torch.equal(s[~fulld], free_s[~fulld]) and torch.equal(x0[~fulld], free_x0[~fulld]), (eta, i)
                assert torch.equal(s[fulld], held[fulld]) and torch.equal(x0[fulld], kd[fulld]), (eta, i)
                assert bool(torch.isfinite(s[fulld]).all())
            if shape == SMALL:                                       # and the restatement says the same
                ref = er.keep_step(tab, i, x, mo, known, kn, keep, "v", eta, bool(i % 2), noise if eta else None)
                assert torch.equal(s.cpu()[~full], ref["sample"][~full]) and torch.equal(s.cpu()[full], ref["sample"][full])
    # ancestral arguments pass through where nothing is kept
    none = torch.zeros_like(ku8)
    kw = dict(mean_type=2, var_type=3, ancestral=True, clip_denoised=False, noise=nd)
    a = ops.diffusion_step_keep(xd, mo.to(DEV), coef, 7, known=kd, known_noise=knd, keep=none, **kw)
    b = ops.diffusion_step(xd, mo.to(DEV), coef, 7, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_entry_points_refuse_bad_arguments(ops, pkg):
    from topia_xl_amd import _lib
    h = _lib.load()
    d, tab, _, coef = _proc(pkg, 5)
    x = torch.zeros(1, 4, 68, device=DEV)
    mo = torch.zeros(1, 4, 136, device=DEV)
    k = torch.zeros(1, 4, dtype=torch.uint8, device=DEV)
    p = lambda t: t.data_ptr()
    assert h.primx_q_sample(None, p(x), 4, p(coef), 0, p(x), None) == -1 and b"null" in h.primx_last_error()
    assert h.primx_q_sample(p(x), p(x), 4, p(coef), -1, p(x), None) == -1
    assert h.primx_diffusion_reverse_step(p(x), None, 0, 4, 68, 136, p(coef), 0, 2, 0, p(x), p(x), None) == -1
    assert h.primx_diffusion_reverse_step(p(x), p(mo), 0, 4, 68, 136, p(coef), 0, 3, 0, p(x), p(x), None) == -1      # mean type
    assert h.primx_diffusion_reverse_step(p(x), p(mo), 7, 4, 68, 136, p(coef), 0, 2, 0, p(x), p(x), None) == -1      # dtype
    assert h.primx_diffusion_reverse_step(p(x), p(mo), 0, 4, 68, 100, p(coef), 0, 2, 0, p(x), p(x), None) == -1      # c_out
    args = lambda known, keep, stride, var=3: (p(x), p(mo), 0, 4, 68, 136, p(coef), 1, 2, var, 0, 0, None, known, p(x), keep, stride,
                                               p(x), p(x), None)
    assert h.primx_diffusion_step_keep(*args(None, p(k), 1)) == -1 and b"null" in h.primx_last_error()
    assert h.primx_diffusion_step_keep(*args(p(x), None, 1)) == -1
    assert h.primx_diffusion_step_keep(*args(p(x), p(k), 2)) == -1 and b"keep_stride" in h.primx_last_error()
    assert h.primx_diffusion_step_keep(*args(p(x), p(k), 0)) == -1
    assert h.primx_diffusion_step_keep(*args(p(x), p(k), 1, var=4)) == -1
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="keep must be"):
        ops.diffusion_step_keep(x, mo, coef, 1, mean_type=2, var_type=3, ancestral=False, clip_denoised=False, noise=None,
                                known=x, known_noise=x, keep=torch.zeros(1, 4, 2, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ loops, stand-in model
class StandIn:
    """Bit-reproducible on the CPU and the GPU: one fp32 product per element, its factor looked up by the MODEL timestep.  On the
    GPU it also plays the planner and checks the call sequence: `expect` = the loop's steps in order."""

    def __init__(self, tmap, expect=None, plan=True):
        self.c = 0.05 + 0.9 * ((torch.arange(1000) * 37) % 100).float() / 100
        self.cd = self.c.to(DEV)
        self.tmap, self.expect, self.pos = tmap, expect, 0
        self.planned, self.rows, self.cleared, self.row = [], [], 0, None
        if not plan:
            self.plan_timesteps = None

    def plan_timesteps(self, ts):
        assert ts.dim() == 1 and ts.dtype == torch.int64 and ts.is_cuda
        self.planned.append(ts.tolist())

    def select_planned_timestep(self, row):
        self.row = row
        if row is not None:
            self.rows.append(row)

    def clear_timestep_plan(self):
        self.cleared += 1

    def __call__(self, x, t, **kw):
        c = (self.cd if x.is_cuda else self.c)[t][:, None, None]
        if x.is_cuda and self.expect is not None:
            want = self.tmap[self.expect[self.pos % len(self.expect)]]
            assert t.tolist() == [want] * x.shape[0], (t.tolist(), want)
            if self.planned:
                assert self.planned[-1][self.row] == want          # the selected row of the announced table is this call's timestep
            self.pos += 1
        return torch.cat([x * c, 0 * x], -1)


def _same(items, ref):
    assert len(items) == len(ref)
    for k, (a, b) in enumerate(zip(items, ref)):
        assert set(a) == {"sample", "pred_xstart"}
        assert torch.equal(a["sample"].cpu(), b["sample"]) and torch.equal(a["pred_xstart"].cpu(), b["pred_xstart"]), k


@pytest.mark.parametrize("n,start", [(5, 3), (5, 4), (25, 12)])
def test_loops_bit_exact_and_planned_by_sub_range(pkg, n, start):
    """The reverse loop, the partial loop and the masked loop against the restatement's loops at every yielded step; the planner
    sees exactly the loop's rows in loop order, every forward gets timestep_map[i], the plan is cleared on exit."""
    d, tab, tmap, _ = _proc(pkg, n)
    assert d.timestep_map == tmap
    shape = (2, 33, 68)
    x = synth.tensor(31, "x", shape)
    # reverse: level 0 -> level `start`, then on to level n (stop_step = n is allowed)
    for lo, hi in ((0, start), (start, n), (0, None)):
        steps = list(range(lo, n - 1 if hi is None else hi))
        m = StandIn(tmap, steps)
        items = list(d.ddim_reverse_sample_loop_progressive(m, x.to(DEV), clip_denoised=False, start_step=lo, stop_step=hi))
        _same(items, er.reverse_loop(StandIn(tmap), x, tab, tmap, "v", False, lo, hi))
        assert m.planned == [[tmap[i] for i in steps]] and m.rows == list(range(len(steps))) and m.cleared == 1
        assert torch.equal(d.ddim_reverse_sample_loop(StandIn(tmap, steps), x.to(DEV), clip_denoised=False, start_step=lo,
                                                      stop_step=hi), items[-1]["sample"])
    # partial: level `start` -> clean
    steps = list(range(start, -1, -1))
    m = StandIn(tmap, steps)
    items = list(d.ddim_sample_loop_progressive(m, shape, noise=x.to(DEV), start_step=start))
    _same(items, er.partial_loop(StandIn(tmap), x, tab, tmap, "v", 0.0, True, start))
    assert m.planned == [[tmap[i] for i in steps]] and m.rows == list(range(len(steps))) and m.cleared == 1 and m.row is None
    partial_final = items[-1]["sample"]
    # masked: rows and elements
    known, kn = synth.tensor(31, "known", shape, 0.6), synth.tensor(31, "kn", shape)
    for keep in (_keep(shape, False, 7), _keep(shape, False, 7)[..., None], _keep(shape, True, 8)):
        m = StandIn(tmap, steps)
        items = list(d.ddim_sample_loop_progressive(m, shape, noise=x.to(DEV), clip_denoised=False, start_step=start,
                                                    known=known.to(DEV), keep=keep.to(DEV), known_noise=kn.to(DEV)))
        _same(items, er.partial_loop(StandIn(tmap), x, tab, tmap, "v", 0.0, False, start, known, keep, kn))
        full = keep.expand(shape) if keep.dim() == 3 else keep[..., None].expand(shape)
        assert torch.equal(items[-1]["sample"].cpu()[full], known[full])
        assert m.planned == [[tmap[i] for i in steps]] and m.cleared == 1
    # a masked FULL loop (start_step=None) stays on the full loop's path: every row announced, selected by step index
    keep = _keep(shape, False, 7)
    m = StandIn(tmap, list(range(n - 1, -1, -1)))
    items = list(d.ddim_sample_loop_progressive(m, shape, noise=x.to(DEV), known=known.to(DEV), keep=keep.to(DEV), known_noise=kn.to(DEV)))
    _same(items, er.partial_loop(StandIn(tmap), x, tab, tmap, "v", 0.0, True, None, known, keep, kn))
    assert m.planned == [tmap] and m.rows == list(range(n - 1, -1, -1))
    # an abandoned generator clears its plan too
    m = StandIn(tmap, steps)
    gen = d.ddim_sample_loop_progressive(m, shape, noise=x.to(DEV), start_step=start)
    next(gen)
    assert m.cleared == 0
    gen.close()
    assert m.cleared == 1
    m = StandIn(tmap, list(range(0, n - 1)))
    gen = d.ddim_reverse_sample_loop_progressive(m, x.to(DEV))
    next(gen)
    del gen
    gc.collect()
    assert m.cleared == 1
    # a model that cannot plan is simply called
    m = StandIn(tmap, steps, plan=False)
    assert torch.equal(d.ddim_sample_loop(m, shape, noise=x.to(DEV), start_step=start), partial_final)
    assert m.pos == len(steps) and m.planned == []


def test_default_path_is_unchanged(pkg):
    """start_step=None and no keep: the samples of a loop written out with ddim_sample step by step, the planner handed the
    whole table and rows selected by step index - as before."""
    n = 5
    d, tab, tmap, _ = _proc(pkg, n)
    shape = (2, 33, 68)
    x = synth.tensor(32, "x", shape).to(DEV)
    m = StandIn(tmap, list(range(n - 1, -1, -1)))
    items = list(d.ddim_sample_loop_progressive(m, shape, noise=x))
    assert m.planned == [tmap] and m.rows == [4, 3, 2, 1, 0] and m.cleared == 1
    plain = StandIn(tmap, plan=False)
    img = x
    for k, i in enumerate(range(n - 1, -1, -1)):
        out = d.ddim_sample(plain, img, torch.full((2,), i, dtype=torch.int64, device=DEV))
        assert torch.equal(out["sample"], items[k]["sample"]) and torch.equal(out["pred_xstart"], items[k]["pred_xstart"])
        img = out["sample"]
    _same(items, dref.ddim_loop(StandIn(tmap), x.cpu(), tab, tmap, "v", 0.0, True))
    # start_step = n - 1 is the same loop, planned by position
    again = d.ddim_sample_loop(StandIn(tmap), shape, noise=x, start_step=n - 1)
    assert torch.equal(again, items[-1]["sample"])


def test_fold_guard_repeats_the_partial_masked_loop(pkg):
    """`_fold_guard` repeats the loop that ran - 4 steps from start_step = 3 with kept rows - not the full one (modelled on
    test_hip_rowops.test_sampling_loop_repeats_an_overflowed_folded_fp16_loop; the stand-in overflows exactly when it "folds")."""

    class Model:
        def __init__(self):
            self.fold_ln, self.calls, self._used, self.plans, self.ts = True, [], False, [], []

        def plan_timesteps(self, ts):
            self.plans.append(ts.tolist())

        def select_planned_timestep(self, row):
            pass

        def clear_timestep_plan(self):
            self._used = False

        def fold_overflowed(self, sample):
            used, self._used = self._used, False
            return used and not bool(torch.isfinite(sample).all())

        def __call__(self, x, t, **kw):
            self.calls.append(bool(self.fold_ln))
            self.ts.append(int(t[0]))
            out = torch.cat([0.1 * x, torch.zeros_like(x)], -1).half()
            if self.fold_ln:
                self._used = True
                if int(t[0]) < 300:
                    out[0, 1, 0] = float("nan")                    # a free row (row 0 is kept: a NaN there would be ignored)
            return out

    d = pkg.create_diffusion("ddim5", noise_schedule="squaredcos_cap_v2", parameterization="v")
    shape = (1, 16, 68)
    x, known, kn = (synth.tensor(33, s, shape).to(DEV) for s in ("x", "known", "kn"))
    keep = torch.zeros(1, 16, dtype=torch.bool, device=DEV)
    keep[0, 0] = keep[0, 5] = True
    kw = dict(noise=x, start_step=3, known=known, keep=keep, known_noise=kn)
    m = Model()
    with pytest.warns(RuntimeWarning, match="LayerNorm fold"):
        items = list(d.ddim_sample_loop_progressive(m, shape, **kw))
    assert len(items) == 4 and m.calls == [True] * 4 + [False] * 4 and m.fold_ln is True
    assert m.ts == [600, 400, 200, 0] * 2 and m.plans == [[600, 400, 200, 0]]
    assert bool(torch.isfinite(items[-1]["sample"]).all())
    m2 = Model()
    m2.fold_ln = False
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        want = d.ddim_sample_loop(m2, shape, **kw)
    assert torch.equal(items[-1]["sample"], want) and m2.calls == [False] * 4
    assert torch.equal(want[0, 0], known[0, 0]) and torch.equal(want[0, 5], known[0, 5])


# ------------------------------------------------------------------------------------------------ the tiny real DiT
@pytest.mark.parametrize("dtype", [F16, F32])
def test_real_dit_trajectories_against_reference(pkg, golden, dtype):
    """The `dit_dh72` case under forward_with_cfg, ddim5, against the REAL reference in fp32 on the CPU: the inversion level
    0 -> 4 at cfg 1, the re-denoise 4 -> clean at cfg 6 from THIS run's inversion end (errors of the inversion carry over, as
    in use), and q_sample at step 2 + the partial loop.  Bound: the project's trajectory bound for this case, rel-L2 < 2e-2
    per stored step (tests/test_hip_dit.py).

    Measured on an MI355X, rel-L2 per stored step: fp16 with amp - inversion 1.45e-4 1.97e-4 2.34e-4 2.58e-4, re-denoise 7.10e-4
    1.15e-3 1.53e-3 1.76e-3 1.76e-3, partial 7.29e-4 9.13e-4 9.11e-4; fp32 - inversion 5e-7 each, re-denoise 1.3e-6 .. 2.7e-6,
    partial 1.1e-6 .. 1.3e-6."""
    name, sd, heads, m, x, y, t = TD._case(pkg, 1)
    g = golden("edit")
    d = pkg.create_diffusion("ddim5", noise_schedule="squaredcos_cap_v2", parameterization="v")
    amp = dict(precision_dtype=dtype, enable_amp=dtype != F32)
    kw1, kw6 = dict(y=y.to(DEV), cfg_scale=1.0, **amp), dict(y=y.to(DEV), cfg_scale=6.0, **amp)
    inv = [s["sample"] for s in d.ddim_reverse_sample_loop_progressive(m.forward_with_cfg, x.to(DEV), clip_denoised=False,
                                                                       model_kwargs=kw1, stop_step=4)]
    red = [s["sample"] for s in d.ddim_sample_loop_progressive(m.forward_with_cfg, x.shape, noise=inv[-1], clip_denoised=False,
                                                               model_kwargs=kw6, start_step=4)]
    q2 = d.q_sample(x.to(DEV), torch.full((x.shape[0],), 2, dtype=torch.int64, device=DEV), dit_noise(x.shape).to(DEV))
    part = [s["sample"] for s in d.ddim_sample_loop_progressive(m.forward_with_cfg, x.shape, noise=q2, clip_denoised=False,
                                                                model_kwargs=kw6, start_step=2)]
    assert np.array_equal(q2.cpu().numpy(), g["dit_q2"])
    figures = {"invert": [rel_l2(a, b) for a, b in zip(inv, g["dit_invert"])],
               "redenoise": [rel_l2(a, b) for a, b in zip(red, g["dit_redenoise"])],
               "partial": [rel_l2(a, b) for a, b in zip(part, g["dit_partial2"])]}
    for k, v in figures.items():
        print(f"real DiT {dtype} {k}: rel-L2 per step " + " ".join(f"{e:.2e}" for e in v))
    assert [len(v) for v in figures.values()] == [4, 5, 3]
    for k, v in figures.items():
        for i, e in enumerate(v):
            assert e < 2e-2, (k, i, e)


# ------------------------------------------------------------------------------------------------ redenoise_primitives
def test_redenoise_primitives_end_to_end(pkg):
    """Tiny VAE + tiny DiT, 2 x 128 primitives, ddim5, start_step = 3.  Kept primitives come out as the encode -> decode round
    trip of the input, bit for bit (the kept tokens are bit-identical and the decoder is deterministic); the others change."""
    from topia_xl_amd import pipeline
    name, sd, heads, m, x, y, t = TD._case(pkg, 1)
    vae = pkg.VAE(**VAE_CFG).eval()
    vae.load_state_dict(synth.state_dict_like(SEED, vae.state_dict()), strict=True)
    vae.to(DEV)
    B, N = 2, 128
    d = pkg.create_diffusion("ddim5", noise_schedule="squaredcos_cap_v2", parameterization="v")
    mean, std = synth.tensor(41, "mean", (68,), 0.5).tolist(), synth.tensor(41, "std", (68,), 0.2, 1.0).abs().tolist()
    stats = dict(latent_mean=mean, latent_std=std, latent_nf=1.1)
    rp = pipeline.latents_to_primitives(synth.tensor(42, "edit.tokens", (B, N, 68)).to(DEV), vae, mean, std, 1.1)
    yy = synth.tensor(SEED, name + ".y2", (B,) + tuple(y.shape[1:])).to(DEV)
    tokens = pipeline.primitives_to_latents(rp, vae, mean, std, 1.1)
    trip = pipeline.latents_to_primitives(tokens, vae, mean, std, 1.1)
    keep = torch.rand(B, N, generator=torch.Generator().manual_seed(1)) < 0.5
    keep = keep.to(DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(9)
    out = pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=3, keep=keep, generator=gen(), **stats)
    assert out.shape == rp.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    assert torch.equal(out[keep][:, :4], trip[keep][:, :4]) and torch.equal(out[keep][:, 4:], trip[keep][:, 4:])
    changed = (out[~keep] != trip[~keep]).any(-1)
    assert bool(changed.all())
    # the same generator state gives the same asset; explicit noise is what the generator would have drawn
    noise = torch.randn(tokens.shape, device=DEV, generator=gen())
    assert torch.equal(pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=3, keep=keep, noise=noise, **stats), out)
    # no keep: everything is regenerated; the kept run's free primitives depended on the kept ones through attention
    free = pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=3, noise=noise, **stats)
    assert bool((free != trip).any(-1).all()) and not torch.equal(free[~keep], out[~keep])
    # keep the layout (scale + xyz), regenerate the appearance
    srt = pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=3, noise=noise,
                                        keep=pipeline.keep_mask(torch.ones(B, N, dtype=torch.bool, device=DEV), "srt"), **stats)
    assert torch.equal(srt[..., :4], trip[..., :4]) and bool((srt[..., 4:] != trip[..., 4:]).any(-1).all())
    # and in token space: channels 0..3 of every token of the final sample are the input tokens
    kw = dict(y=yy, cfg_scale=6.0, precision_dtype=F16, enable_amp=True)
    lvl = d.q_sample(tokens, torch.full((B,), 3, dtype=torch.int64, device=DEV), noise)
    final = d.ddim_sample_loop(m.forward_with_cfg, tuple(tokens.shape), noise=lvl, clip_denoised=False, model_kwargs=kw, start_step=3,
                               known=tokens, known_noise=noise,
                               keep=pipeline.keep_mask(torch.ones(B, N, dtype=torch.bool, device=DEV), "srt"))
    assert torch.equal(final[..., :4], tokens[..., :4]) and not torch.equal(final[..., 4:], tokens[..., 4:])
    # inversion instead of noise
    inv = pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=3, mode="invert", **stats)
    assert inv.shape == rp.shape and bool(torch.isfinite(inv).all())
    with pytest.raises(ValueError, match="invert"):
        pipeline.redenoise_primitives(rp, vae, m, d, yy, start_step=3, mode="invert", keep=keep, **stats)


# ------------------------------------------------------------------------------------------------ footprint
def _I(g, t, name):
    return None if t is None else g.guard_input(t, name).t


@pytest.mark.parametrize("out_dtype", [F16, BF16, F32])
def test_edit_entry_points_footprint(ops, pkg, out_dtype):
    """primx_q_sample, primx_diffusion_reverse_step and primx_diffusion_step_keep (both keep strides) between guards under both
    fills, at the shapes of test_hip_footprint.test_diffusion_step_footprint: 2 x 97 x 68, step 0 and a middle step."""
    d = pkg.create_diffusion("ddim25", noise_schedule="squaredcos_cap_v2", parameterization="v")
    coef0 = torch.from_numpy(d.step_coefficients(0.5)).to(DEV)
    x0, mo0, n0 = (a.to(DEV) for a in _operands(51, SMALL))
    mo0 = mo0.to(out_dtype)
    kn0, kk0 = synth.tensor(51, "known", SMALL).to(DEV), synth.tensor(51, "kn", SMALL).to(DEV)
    keeps = {1: _keep(SMALL, False, 3).to(DEV).view(torch.uint8), 68: _keep(SMALL, True, 4).to(DEV).view(torch.uint8)}

    def q_case(g):
        x, noise, coef = _I(g, x0, "x_start"), _I(g, n0, "noise"), _I(g, coef0, "coef")
        return {i: ops.q_sample(x, noise, coef, i) for i in (0, 7, 24)}
    fp.hold(q_case)

    def reverse_case(g):
        x, mo, coef = _I(g, x0, "x"), _I(g, mo0, "model_out"), _I(g, coef0, "coef")
        return {(i, mt, clip): ops.diffusion_reverse_step(x, mo, coef, i, mean_type=mt, clip_denoised=clip)
                for i in (0, 7, 24) for mt in (0, 1, 2) for clip in (False, True)}
    fp.hold(reverse_case)

    def keep_case(g):
        x, mo, noise, coef = _I(g, x0, "x"), _I(g, mo0, "model_out"), _I(g, n0, "noise"), _I(g, coef0, "coef")
        known, kn = _I(g, kn0, "known"), _I(g, kk0, "known_noise")
        out = {}
        for stride, k0 in keeps.items():
            keep = _I(g, k0, f"keep {stride}")
            for i in (0, 7):
                for mt in (0, 1, 2):
                    out[(stride, i, mt)] = ops.diffusion_step_keep(x, mo, coef, i, mean_type=mt, var_type=3, ancestral=False,
                                                                   clip_denoised=bool(i), noise=noise if i else None, known=known,
                                                                   known_noise=kn, keep=keep)
            out[(stride, "ancestral")] = ops.diffusion_step_keep(x, mo, coef, 24, mean_type=2, var_type=2, ancestral=True,
                                                                 clip_denoised=False, noise=noise, known=known, known_noise=kn, keep=keep)
        return out
    fp.hold(keep_case)
