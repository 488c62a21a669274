"""Self-tests of tests/contract_ref.py (CPU only): round16 / ulp16 against independent references, and mutation tests -
emulated kernels that break one documented rounding point each must FAIL check_contract while the correct emulation (fp32
accumulation, then a correct rounding) passes.  Each mutant also reports the rel-L2 the GEMM / row-op tests compare with,
to show that the old tolerance (1.5e-3 fp16, 1.2e-2 bf16) would have let it through.  Run with `-rP` to see the table."""
import math

import numpy as np
import pytest
import torch

from tests import contract_ref as cr

F16, BF16 = torch.float16, torch.bfloat16
OLD_TOL = {F16: 1.5e-3, BF16: 1.2e-2}    # the rel-L2 tolerance of tests/test_hip_gemm.py / test_hip_rowops.py / test_hip_vae.py


# ------------------------------------------------------------------------------------------------ round16 / ulp16
def _edge_values():
    """Ties, near-ties, overflow and subnormals of both formats, plus random float64 values over every exponent."""
    rng = np.random.default_rng(0)
    vals = [0.0, -0.0, 1.0, -1.0, 65504.0, 65519.99, 65520.0, 65520.01, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * 1.0001,
            3 * 2.0 ** -26, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -40,
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8 - 2.0 ** -40,
            float.fromhex("0x1.fep127"), float.fromhex("0x1.ff0p127"), float.fromhex("0x1.fefffffp127"), 2.0 ** -133,
            2.0 ** -134, 2.0 ** -134 * 1.5, 2.0 ** -126, 1e300, np.inf, -np.inf]
    ties = []
    for p, lo, hi in ((11, -24, 16), (8, -133, 128)):
        e = rng.integers(lo, hi, 20000)
        m = rng.integers(1 << (p - 1), 1 << p, 20000)
        t = np.ldexp(m + 0.5, e - (p - 1))                   # exact midpoints
        ties += [t, np.nextafter(t, 0), np.nextafter(t, np.inf), -t]
    rnd = np.ldexp(rng.uniform(-1, 1, 400000), rng.integers(-140, 130, 400000))
    return np.concatenate([np.array(vals), *ties, rnd])


def test_round16_fp16_matches_numpy_and_the_generic_rounding():
    x = _edge_values()
    with np.errstate(over="ignore"):
        want = x.astype(np.float16).astype(np.float64)
    got = cr.round16(x, F16)
    assert np.array_equal(got, want, equal_nan=True)
    p, emin, fmax = cr._FMT[F16]
    assert np.array_equal(cr._round_binary(x, p, emin, fmax), want, equal_nan=True)
    assert np.array_equal(np.signbit(got), np.signbit(want))
    # the torch route double-rounds (why round16 exists)
    assert float(torch.tensor(1 + 2 ** -11 + 2 ** -40, dtype=torch.float64).to(F16)) == 1.0
    assert cr.round16(1 + 2 ** -11 + 2 ** -40, F16) == 1 + 2 ** -10
    assert cr.round16(65520.0, F16) == np.inf and cr.round16(65519.99, F16) == 65504.0
    assert cr.round16(3 * 2.0 ** -26, F16) == 2.0 ** -24 and cr.round16(2.0 ** -25, F16) == 0.0


def _bf16_bits_ref(x: np.ndarray) -> np.ndarray:
    """Independent bf16 rounding on the float64 bit pattern: keep 7 fraction bits of a normal bf16 (more dropped bits
    below 2^-126), add half the dropped range minus one plus the kept lsb, clear the dropped bits; a carry that leaves the
    bf16 exponent range is an overflow."""
    x = np.asarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    sign = bits & np.uint64(1 << 63)
    mag = bits & np.uint64((1 << 63) - 1)
    exp = ((mag >> np.uint64(52)).astype(np.int64)) - 1023
    fin = np.isfinite(x) & (x != 0)
    # drop = 45 dropped fraction bits for normal bf16 values, more below the bf16 normal range (2^-126)
    drop = np.where(exp >= -126, 45, 45 + (-126 - exp)).astype(np.int64)
    big = fin & (drop <= 60)                                          # (further down everything rounds to zero)
    d = drop[big].astype(np.uint64)
    m = mag[big]
    # value bits below bf16 normal: rebuild as an explicit integer significand so that the hidden bit takes part in rounding
    sig = (m & np.uint64((1 << 52) - 1)) | np.uint64(1 << 52)
    e = exp[big]
    lsb = (sig >> d) & np.uint64(1)
    half = (np.uint64(1) << (d - np.uint64(1)))
    rnd = (sig + half - np.uint64(1) + lsb) >> d                      # integer significand in units of 2^(e - 52 + d)
    val = np.ldexp(rnd.astype(np.float64), (e - 52 + drop[big]).astype(np.int64))
    res_f = np.zeros(x.shape)
    res_f[big] = val
    res_f = np.where(np.abs(res_f) >= 2.0 ** 128, np.inf, res_f)
    out = np.where(fin, np.where(sign != 0, -res_f, res_f), x)        # zero / inf / nan unchanged
    return out


def test_round16_bf16_matches_a_bit_level_reference():
    x = _edge_values()
    rng = np.random.default_rng(1)
    every_exp = np.ldexp(rng.uniform(1, 2, (300, 2000)), np.arange(-150, 150)[:, None]).ravel()   # every exponent 2^-150 .. 2^149
    x = np.concatenate([x, every_exp, -every_exp])
    assert x.size >= 10 ** 6
    got, want = cr.round16(x, BF16), _bf16_bits_ref(x)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (x[bad][:5], got[bad][:5], want[bad][:5])
    assert float(torch.tensor(1 + 2 ** -8 + 2 ** -40, dtype=torch.float64).to(BF16)) == 1.0    # torch's double rounding
    assert cr.round16(1 + 2 ** -8 + 2 ** -40, BF16) == 1 + 2 ** -7
    assert cr.round16(1 + 2 ** -8, BF16) == 1.0 and cr.round16(1 + 3 * 2 ** -8, BF16) == 1 + 2 ** -6     # ties to even
    assert cr.round16(float.fromhex("0x1.ffp127"), BF16) == np.inf
    assert cr.round16(2.0 ** -134, BF16) == 0.0 and cr.round16(2.0 ** -134 * 1.5, BF16) == 2.0 ** -133


def test_ulp16():
    assert cr.ulp16(1.0, F16) == 2.0 ** -10 and cr.ulp16(1.5, BF16) == 2.0 ** -7
    assert cr.ulp16(0.0, F16) == 2.0 ** -24 and cr.ulp16(1e-6, F16) == 2.0 ** -24 and cr.ulp16(2.0 ** -14, F16) == 2.0 ** -24
    assert cr.ulp16(0.0, BF16) == 2.0 ** -133 and cr.ulp16(40000.0, F16) == 32.0 and cr.ulp16(np.inf, F16) == 32.0
    x = _edge_values()
    x = x[np.isfinite(x) & (np.abs(x) < 60000)]
    for dt in (F16, BF16):
        r = cr.round16(x, dt)
        u = cr.ulp16(r, dt)
        assert np.all(np.abs(r - x) <= u / 2)                # round-to-nearest never moves more than half a spacing
        assert np.all(cr.round16(r + u, dt) == r + u)        # r + ulp is the next representable value


# ------------------------------------------------------------------------------------------------ mutation tests
def _trunc16(x, dtype):
    """Rounding toward zero (what a bit-shift conversion without rounding gives)."""
    p, emin, _ = cr._FMT[dtype]
    x = np.asarray(x, np.float64)
    out = x.copy()
    f = np.isfinite(x) & (x != 0)
    _, e = np.frexp(x[f])
    q = np.maximum(e - 1, emin) - (p - 1)
    out[f] = np.ldexp(np.trunc(np.ldexp(x[f], -q)), q)
    return out


def _old_rel_l2(got, exact):
    g, e = np.asarray(got, np.float64).ravel(), np.asarray(exact, np.float64).ravel()
    m = np.isfinite(g) & np.isfinite(e)
    return float(np.linalg.norm(g[m] - e[m]) / np.linalg.norm(e[m]))


def _gemm_case(dtype, M=512, N=1152, K=1152, a_scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    A = (torch.randn(M, K, generator=g) * a_scale).to(dtype)
    W = (torch.randn(N, K, generator=g) * K ** -0.5).to(dtype)
    b = (torch.randn(N, generator=g) * 0.3).to(dtype)
    acc = cr.gemm_acc(A, W, b)                                                       # exact
    acc32 = (A.float() @ W.float().t() + b.float()).double().numpy()                # the kernel's fp32 accumulation
    nob32 = (A.float() @ W.float().t()).double().numpy()
    return A, W, b, acc, acc32, nob32


def _fails(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_correct_emulation_passes_and_truncation_fails(dtype):
    _, _, b, acc, acc32, nob32 = _gemm_case(dtype)
    pre, ref = cr.linear_ref(acc, dtype)
    rep = cr.check_contract(cr.round16(acc32, dtype), pre, ref, dtype, 1152, what="correct")
    print(f"correct emulation {dtype}: {rep}  old rel-L2 {_old_rel_l2(cr.round16(acc32, dtype), acc):.3e}")
    assert rep["allowed_frac"] < (0.04 if dtype == F16 else 0.006)      # the allowance is of the documented size
    mut = _trunc16(acc32, dtype)
    old = _old_rel_l2(mut, acc)
    msg = _fails(lambda: cr.check_contract(mut, pre, ref, dtype, 1152, what="truncation"))
    print(f"mutant truncation {dtype}: old rel-L2 {old:.3e} (passes {OLD_TOL[dtype]:.1e}: {old < OLD_TOL[dtype]}); new check: {msg}")
    assert old < OLD_TOL[dtype] and msg is not None
    # bias added after the rounding of A W^T
    mut = cr.round16(cr.round16(nob32, dtype) + b.double().numpy()[None, :], dtype)
    old = _old_rel_l2(mut, acc)
    msg = _fails(lambda: cr.check_contract(mut, pre, ref, dtype, 1152, what="bias after rounding"))
    print(f"mutant bias-after-rounding {dtype}: old rel-L2 {old:.3e} (passes: {old < OLD_TOL[dtype]}); new check: {msg}")
    assert old < OLD_TOL[dtype] and msg is not None


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_gate_residual_without_the_inner_rounding_fails(dtype):
    A, W, b, acc, acc32, _ = _gemm_case(dtype, seed=1)
    g = torch.Generator().manual_seed(2)
    gate = (torch.randn(2, 1152, generator=g) * 0.5).to(dtype).double().numpy()
    gate_rows = np.repeat(gate, 256, axis=0)
    pre, ref = cr.gate_residual_ref(acc, gate_rows, dtype)
    good = cr.round16(gate_rows * cr.round16(acc32, dtype), dtype)
    inner = np.abs(gate_rows) * cr.ulp16(acc, dtype)
    cr.check_contract(good, pre, ref, dtype, 1152, acc=acc, gain=gate_rows, inner=inner, what="gate residual")
    mut = cr.round16(gate_rows * acc32, dtype)
    old = _old_rel_l2(mut, gate_rows * cr.round16(acc, dtype))
    msg = _fails(lambda: cr.check_contract(mut, pre, ref, dtype, 1152, acc=acc, gain=gate_rows, inner=inner,
                                           what="gate residual, no inner cast16"))
    frac = float(np.mean(mut != ref))
    print(f"mutant gate-residual-no-inner-cast16 {dtype}: {frac:.1%} of the elements change; old rel-L2 {old:.3e} "
          f"(passes: {old < 2 * OLD_TOL[dtype]}); new check: {msg}")
    assert old < 2 * OLD_TOL[dtype] and msg is not None


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_layernorm_modulate_with_an_unrounded_one_plus_scale_fails(dtype):
    g = torch.Generator().manual_seed(3)
    rows, D = 512, 1152
    x = torch.randn(rows, D, generator=g) * 2.0 + 0.3
    shift = (torch.randn(2, D, generator=g) * 0.3).to(dtype).double().numpy()
    scale = (torch.randn(2, D, generator=g) * 0.3).to(dtype).double().numpy()
    sh, sc = np.repeat(shift, 256, 0), np.repeat(scale, 256, 0)
    pre, ref = cr.layernorm_modulate_ref(x, sh, sc, dtype)
    # correct emulation: fp32 statistics and arithmetic, then one rounding
    xf = x.numpy().astype(np.float32)
    mu = xf.mean(-1, keepdims=True, dtype=np.float32)
    var = ((xf - mu) ** 2).mean(-1, keepdims=True, dtype=np.float32)
    rs = (1.0 / np.sqrt(var + np.float32(1e-6))).astype(np.float32)
    m1 = cr.round16(1.0 + sc, dtype).astype(np.float32)
    good = cr.round16(((xf - mu) * rs * m1 + sh.astype(np.float32)).astype(np.float64), dtype)
    cr.check_contract(good, pre, ref, dtype, D, ew_ulps=8.0, what="layernorm_modulate")
    mut = cr.round16(((xf - mu) * rs * (1.0 + sc).astype(np.float32) + sh.astype(np.float32)).astype(np.float64), dtype)
    old = _old_rel_l2(mut, pre)
    msg = _fails(lambda: cr.check_contract(mut, pre, ref, dtype, D, ew_ulps=8.0, what="LN, (1 + scale) unrounded"))
    print(f"mutant ln-unrounded-1+scale {dtype}: old rel-L2 {old:.3e} (passes: {old < OLD_TOL[dtype]}); new check: {msg}")
    assert old < OLD_TOL[dtype] and msg is not None


def test_extra_rounding_through_fp16_on_a_bf16_output_fails():
    dtype = BF16
    _, _, _, acc, acc32, _ = _gemm_case(dtype, seed=4)
    pre, ref = cr.linear_ref(acc, dtype)
    mut = cr.round16(cr.round16(acc32, F16), BF16)
    old = _old_rel_l2(mut, acc)
    msg = _fails(lambda: cr.check_contract(mut, pre, ref, dtype, 1152, what="bf16 through fp16"))
    print(f"mutant bf16-through-fp16: old rel-L2 {old:.3e} (passes: {old < OLD_TOL[dtype]}); new check: {msg}")
    assert old < OLD_TOL[dtype] and msg is not None


def test_fp16_saturation_and_flushed_subnormals_fail():
    dtype = F16
    # outputs around the overflow threshold: scale A so that |y| spans [60000, 70000] for a good share of the elements
    _, _, _, acc, acc32, _ = _gemm_case(dtype, M=256, N=576, K=1152, seed=5)
    s = 65000.0 / np.quantile(np.abs(acc), 0.9)
    acc, acc32 = acc * s, (acc32.astype(np.float32) * np.float32(s)).astype(np.float64)
    pre, ref = cr.linear_ref(acc, dtype)
    assert np.isinf(ref).sum() > 100
    good = cr.round16(acc32, dtype)
    cr.check_contract(good, pre, ref, dtype, 1152, what="fp16 overflow band")
    mut = np.clip(good, -65504.0, 65504.0)
    old = _old_rel_l2(mut, acc)
    msg = _fails(lambda: cr.check_contract(mut, pre, ref, dtype, 1152, what="saturating fp16"))
    print(f"mutant fp16-saturates-at-65504: old rel-L2 {old:.3e} (finite elements); new check: {msg}")
    assert msg is not None
    # subnormal band: |y| < 6.1e-5
    _, _, _, acc, acc32, _ = _gemm_case(dtype, M=256, N=576, K=1152, seed=6)
    s = 3e-5 / np.quantile(np.abs(acc), 0.5)
    acc, acc32 = acc * s, (acc32.astype(np.float32) * np.float32(s)).astype(np.float64)
    pre, ref = cr.linear_ref(acc, dtype)
    assert np.mean(np.abs(ref) < 2.0 ** -14) > 0.5
    good = cr.round16(acc32, dtype)
    cr.check_contract(good, pre, ref, dtype, 1152, what="fp16 subnormal band")
    mut = np.where(np.abs(good) < 2.0 ** -14, 0.0, good)
    old = _old_rel_l2(mut, acc)
    msg = _fails(lambda: cr.check_contract(mut, pre, ref, dtype, 1152, what="flushed fp16 subnormals"))
    print(f"mutant fp16-subnormals-flushed: old rel-L2 {old:.3e}; new check: {msg}")
    assert msg is not None


def test_allowance_matches_its_derivation():
    """The allowed fraction of differing elements is the documented formula, not a number fitted to outputs: at K = 1152
    with y ~ N(0, 1) it is about 2.5 % (fp16) and 0.35 % (bf16), and it grows as sqrt(K)."""
    rng = np.random.default_rng(7)
    y = rng.standard_normal((200, 1000))
    for dt, lo, hi in ((F16, 0.015, 0.04), (BF16, 0.002, 0.006)):
        ref = cr.round16(y, dt)
        r1 = cr.contract_report(ref, y, ref, dt, 1152, ew_ulps=0.0)
        r4 = cr.contract_report(ref, y, ref, dt, 4 * 1152, ew_ulps=0.0)
        assert lo < r1["allowed_frac"] < hi, r1
        assert 1.7 < r4["allowed_frac"] / r1["allowed_frac"] < 2.1
    assert math.isclose(cr.C_ACC, 2.0)
