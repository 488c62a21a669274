"""Self-tests of the LayerNorm-fold references of tests/contract_ref.py (CPU only): a numpy restatement of the fold CONSUMER
(fold_stats_finish / fold_apply / fold_out4 of csrc/gemm.hip, fp32 step by step) meets fold_consumer_ref under check_contract,
its center_out meets fold_stats_ref's bound, and its output meets the site bound against the unfolded float64 reference - while
each mutant that breaks one documented step FAILS the new check.  Each mutant also reports whether the old criterion of
tests/test_hip_fold.py (rel-L2 < 2 TOL and < 1.5 x the unfolded path's + 1e-4) lets it through.  Run with `-rP` to see the table."""

import numpy as np
import pytest
import torch

from tests import contract_ref as cr
from tests.test_contract_cpu import _fails, _trunc16

F16, BF16 = torch.float16, torch.bfloat16
TOL = {F16: 1.5e-3, BF16: 1.2e-2}      # tests/test_hip_fold.py
EPS = 1e-6
M, D, N = 512, 1152, 576               # rows (two batch entries of 256), LayerNorm width = K of the consumer, consumer columns
S0 = 72 ** -0.5                        # the heads scale0 of to_q
f32 = np.float32


def _site(dtype, seed, spread):
    """Residual rows x (fp32, per-row mean 0.3 x the spread), the stale (c, rho_p) pairs of the previous site (mean moved by a
    tenth of the spread, rstd by 10 %), modulation m = cast16(1 + scale) and shift, consumer weights W, b (16-bit values)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((M, D)) * spread
    x = (x + 0.3 * spread * rng.standard_normal((M, 1))).astype(f32)
    xd = x.astype(np.float64)
    c = xd.mean(-1) + 0.1 * xd.std(-1) * rng.standard_normal(M)
    rp = (1 + 0.1 * np.clip(rng.standard_normal(M), -2, 2)) / np.sqrt(xd.var(-1) + EPS)
    cen = np.stack([c, rp], -1).astype(f32)
    m = cr.round16(1.0 + cr.round16(0.4 * rng.standard_normal(D), dtype), dtype)
    shift = cr.round16(0.4 * rng.standard_normal(D), dtype)
    W = cr.round16(rng.standard_normal((N, D)) * D ** -0.5, dtype)
    b = cr.round16(0.3 * rng.standard_normal(N), dtype)
    return x, cen, m, shift, W, b


def _producer(x, cen, m, dtype):
    """a16 = cast16(((x - c) rho_p) m) and the 144-column partial sums of (x - c), (x - c)^2, all in fp32."""
    d = (x - cen[:, :1]).astype(f32)
    a16 = cr.round16(((d * cen[:, 1:]).astype(f32) * m.astype(f32)).astype(np.float64), dtype)
    dt = d.reshape(M, D // 144, 144)
    part = np.stack([dt.sum(-1, dtype=f32), (dt * dt).astype(f32).sum(-1, dtype=f32)], -1)
    return a16, part


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _gelu32(y):
    return cr.gelu_tanh64(y.astype(np.float64)).astype(f32)


def _consumer(a16, W, part, cen, u, v, dtype, act=0, scale0=1.0, mut=None):
    """The consumer epilogue in fp32, as csrc/gemm.hip computes it; `mut` breaks one step.  Returns (out, center_out)."""
    P = part.shape[1]
    s1, s2 = np.zeros(M, f32), np.zeros(M, f32)
    for i in range(P):                                              # fixed order
        s1, s2 = (s1 + part[:, i, 0]).astype(f32), (s2 + part[:, i, 1]).astype(f32)
    inv = f32(1.0) / f32(D)
    mu = (s1 * inv).astype(f32)
    if mut == "unbiased variance":
        var = ((s2 - f32(D) * mu * mu) / f32(D - 1)).astype(f32)
    else:
        var = (s2 * inv - mu * mu).astype(f32)
    var = np.maximum(var, f32(0))
    if mut == "eps outside the sqrt":
        rho = (f32(1) / (np.sqrt(var) + f32(EPS))).astype(f32)
    else:
        rho = (f32(1) / np.sqrt(var + f32(EPS))).astype(f32)
    st0 = (cen[:, 1] * mu).astype(f32)
    st1 = rho if mut == "rho_p not divided out" else (rho / cen[:, 1]).astype(f32)
    cout = np.stack([mu if mut == "center_out without c" else (cen[:, 0] + mu).astype(f32), rho], -1)
    acc = a16.astype(f32) @ W.astype(f32).T
    y = _fma(st1[:, None], _fma(-st0[:, None], u[None, :], acc), v[None, :])
    if mut == "scale0 with a single rounding":
        return cr.round16((f32(scale0) * y).astype(np.float64), dtype), cout
    if mut == "GELU without the inner cast16":
        return cr.round16(_gelu32(y).astype(np.float64), dtype), cout
    y16 = (_trunc16 if mut == "truncation" else cr.round16)(y.astype(np.float64), dtype)
    if f32(scale0) != 1.0:
        y16 = cr.round16((f32(scale0) * y16.astype(f32)).astype(np.float64), dtype)
    if act:
        y16 = cr.round16(_gelu32(y16.astype(f32)).astype(np.float64), dtype)
    return y16, cout


class Site:
    def __init__(self, dtype, seed, spread):
        self.dtype = dtype
        self.x, self.cen, self.m, self.shift, self.W, self.b = _site(dtype, seed, spread)
        self.a16, self.part = _producer(self.x, self.cen, self.m, dtype)
        self.u = (self.m @ self.W.T).astype(f32)                                   # fp32 rows of the fold (primx_linear_f32out)
        self.v = (self.shift @ self.W.T + self.b).astype(f32)
        self.acc = self.a16 @ self.W.T                                             # exact
        self.mag = np.maximum(np.sqrt((self.a16 ** 2) @ (self.W ** 2).T), np.abs(self.acc))
        self.stats = cr.fold_stats_ref(self.part, self.cen, D, EPS)
        self.stats_x = cr.fold_stats_ref(self.part, self.cen, D, EPS, part_err=cr.fold_partials_err(self.x, self.cen))
        # the unfolded path (LayerNorm -> modulate rounded, fp32 Linear) and the float64 reference of the old tests
        xd = self.x.astype(np.float64)
        mu = xd.mean(-1, keepdims=True)
        ln = (xd - mu) / np.sqrt(((xd - mu) ** 2).mean(-1, keepdims=True) + EPS)
        self.ref64 = torch.from_numpy((ln * self.m + self.shift) @ self.W.T + self.b)
        xn = cr.round16(ln * self.m + self.shift, dtype)
        self.unf = (xn.astype(f32) @ self.W.T.astype(f32) + self.b.astype(f32)).astype(np.float64)

    def check(self, out, cout, act=0, scale0=1.0, what=""):
        """The new criterion: the consumer contract, center_out within its derived bound, the site bound."""
        pre, ref = cr.fold_consumer_ref(self.acc, self.stats, self.u, self.v, self.dtype, act, scale0)
        kw = cr.fold_contract_kw(self.acc, self.mag, self.stats, self.u, self.v, self.dtype, D, act, scale0)
        rep = cr.check_contract(out, pre, ref, self.dtype, D, what=what, **kw)
        cf = cr.check_fold_center(cout, self.stats, what)
        ref_out, bound, edge = cr.fold_site_bound(self.x, self.cen, self.m, self.shift, self.W, self.b, self.a16, self.stats_x, self.u,
                                                  self.v, self.dtype, act, scale0, EPS)
        sf = cr.check_fold_site(out, ref_out, bound, edge, self.dtype, what)
        return rep, cf, sf

    def old_criterion(self, out, act=0, scale0=1.0):
        """(passes, err, err_unfolded) of tests/test_hip_fold.py's rel-L2 criterion."""
        dt = self.dtype
        want = self.ref64.to(dt)
        unf = torch.from_numpy(cr.round16(self.unf, dt))
        if scale0 != 1.0:
            want = (scale0 * want.float()).to(dt)
            unf = torch.from_numpy(cr.round16(f32(scale0) * unf.numpy().astype(f32), dt))
        if act:
            want = torch.nn.functional.gelu(want.double(), approximate="tanh")
            unf = torch.from_numpy(cr.round16(_gelu32(unf.numpy().astype(f32)), dt))
        rel = lambda a: float((torch.as_tensor(a).double() - want.double()).norm() / want.double().norm())
        err, err_u = rel(out), rel(unf)
        return err < 2 * TOL[dt] and err < 1.5 * err_u + 1e-4, err, err_u


FORMS = {"plain": dict(), "scale0": dict(scale0=S0), "gelu": dict(act=1)}


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("spread", [2.0, 1e-3])
def test_fold_consumer_emulation_meets_its_contract(dtype, spread):
    """The restated consumer passes every new check, in each output form, at a normal row spread and at one where var ~ eps."""
    site = Site(dtype, 11, spread)
    for form, kw in FORMS.items():
        out, cout = _consumer(site.a16, site.W, site.part, site.cen, site.u, site.v, dtype, **kw)
        rep, cf, sf = site.check(out, cout, what=f"{form} spread {spread:g}", **kw)
        print(f"fold emulation {dtype} spread {spread:g} {form}: {rep}; center_out {cf:.3f} of its bound; site {sf:.3f} of its bound")


# mutant -> (output form, row spread that exposes it, does the old criterion pass it (the issue's prediction) or None = not predicted)
MUTANTS = {
    "truncation": ("plain", 2.0, None),
    "scale0 with a single rounding": ("scale0", 2.0, True),
    "GELU without the inner cast16": ("gelu", 2.0, None),
    "unbiased variance": ("plain", 2.0, True),
    "eps outside the sqrt": ("plain", 1e-3, None),
    "center_out without c": ("plain", 2.0, None),
    "rho_p not divided out": ("plain", 2.0, None),
}


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("mut", list(MUTANTS))
def test_fold_mutant_fails_the_new_check(dtype, mut):
    form, spread, old_predicted = MUTANTS[mut]
    kw = FORMS[form]
    site = Site(dtype, 11, spread)
    out, cout = _consumer(site.a16, site.W, site.part, site.cen, site.u, site.v, dtype, mut=mut, **kw)
    msg = _fails(lambda: site.check(out, cout, what=mut, **kw))
    old, err, err_u = site.old_criterion(out, **kw)
    print(f"mutant {mut!r} {dtype} ({form}, spread {spread:g}): old criterion rel-L2 {err:.3e} vs unfolded {err_u:.3e} -> "
          f"{'passes' if old else 'fails'}; new check: {'fails' if msg else 'PASSES'} ({msg and msg.splitlines()[0][:160]})")
    assert msg is not None, f"mutant {mut} passes the new check"
    if old_predicted is not None:
        assert old == old_predicted, f"mutant {mut}: the old criterion {'passes' if old else 'fails'} it, not as predicted"
