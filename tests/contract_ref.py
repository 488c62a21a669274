"""Rounding-contract references for the 16-bit entry points of include/primx_hip.h (CPU only: numpy + torch float64).

Every HIP entry point that writes a 16-bit result documents WHERE it rounds ("each stage rounded to the 16-bit type as
autocast does", "one rounding", "no intermediate rounding", ...).  The helpers here evaluate those formulas in float64 and
apply `round16` at exactly the documented points and nowhere else; `check_contract` then holds a kernel's output to them
ulp by ulp instead of with a rel-L2 norm.

Why float64 is the exact value here: a product of two 16-bit values has at most 2 x 11 significant bits and is exact in
float64 (53 bits); a sum of K <= 6912 such products loses at most K * 2^-53 relative to the largest partial sum, which is
below 2^-40 - about 2^-29 of a 16-bit ulp.  Rounding the float64 value is therefore the contract's rounding of the exact value.

`round16` does NOT use `tensor.to(dtype)`: torch converts float64 -> 16 bit through float32 and so rounds twice
(1 + 2^-8 + 2^-40 becomes 1.0 in bf16 instead of 1 + 2^-7).
"""
import math

import numpy as np
import torch

# (significand bits incl. the hidden one, smallest normal exponent, largest finite value)
_FMT = {torch.float16: (11, -14, 65504.0), torch.bfloat16: (8, -126, float.fromhex("0x1.fep127"))}


def _f64(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def _round_binary(x: np.ndarray, p: int, emin: int, fmax: float) -> np.ndarray:
    """Round-to-nearest-even of float64 to a binary format with p significand bits, normal exponents >= emin (gradual
    underflow below) and largest finite value fmax (overflow to +-inf from fmax + ulp/2 on), by exponent arithmetic."""
    x = np.asarray(x, dtype=np.float64)
    out = x.copy()
    fin = np.isfinite(x) & (x != 0)
    xf = x[fin]
    _, e = np.frexp(xf)                                     # |x| = m 2^e, m in [0.5, 1): binade exponent e - 1
    q = np.maximum(e - 1, emin) - (p - 1)                   # exponent of the spacing (subnormal spacing below emin)
    r = np.ldexp(np.rint(np.ldexp(xf, -q)), q)              # exact scaling; np.rint rounds half to even
    r = np.where(np.abs(r) > fmax, np.copysign(np.inf, xf), r)
    out[fin] = r
    return out


def round16(x, dtype) -> np.ndarray:
    """Correctly rounded (nearest, ties to even) float64 -> fp16 / bf16, returned as float64 values.  Subnormals are kept,
    overflow goes to +-inf, NaN stays NaN, the sign of zero is kept."""
    x = _f64(x)
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)  # numpy rounds float64 -> half directly (no float32 step)
    p, emin, fmax = _FMT[dtype]
    return _round_binary(x, p, emin, fmax)


def ulp16(x, dtype) -> np.ndarray:
    """Spacing of the 16-bit format at |x| (the gap above the binade's lower end; the subnormal spacing below the normal
    range; the top binade's spacing for |x| beyond the largest finite value, inf included)."""
    p, emin, fmax = _FMT[dtype]
    a = np.abs(_f64(x))
    a = np.where(np.isfinite(a), np.minimum(a, fmax), fmax)
    _, e = np.frexp(np.where(a > 0, a, 1.0))
    e = np.where(a > 0, np.maximum(e - 1, emin), emin)
    return np.ldexp(1.0, (e - (p - 1)).astype(np.int64))


def r16(x, dtype) -> np.ndarray:
    return round16(x, dtype)


def f32(x) -> float:
    """The float32 value of a Python scalar (what a `float` argument of the C ABI carries)."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ contract references
# Every function returns (pre, ref): pre = the float64 value in front of the LAST rounding, ref = round16(pre) (the
# contract's result).  `acc` helpers return the exact value in front of the FIRST rounding, which is where a kernel's
# fp32 accumulation error enters (check_contract's `acc=`).

def gemm_acc(A, W, bias=None) -> np.ndarray:
    """A W^T (+ bias), exact (float64)."""
    acc = _f64(A) @ _f64(W).T
    if bias is not None:
        acc = acc + _f64(bias)[None, :]
    return acc


def gelu_tanh64(y):
    return 0.5 * y * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))


def _erf64(y):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64))).numpy()


def act64(y, act):
    if act == 0:
        return y
    if act == 1:
        return gelu_tanh64(y)
    return 0.5 * y * (1.0 + _erf64(y / math.sqrt(2.0)))


def linear_ref(acc, dtype, act=0, out_scale=1.0):
    """primx_linear: out_scale * act(A W^T + bias), each stage rounded (Linear output, activation, scaled output);
    out_scale == 1 has no last stage."""
    y = r16(acc, dtype)
    if act:
        pre = act64(y, act)
        y = r16(pre, dtype)
    else:
        pre = acc
    if f32(out_scale) != 1.0:
        pre = f32(out_scale) * y
        y = r16(pre, dtype)
    return pre, y


def linear_residual_ref(acc, dtype, res=None, scale=1.0):
    """primx_linear_residual / conv3d_k3: ((A W^T + bias) + res) * scale, one rounding."""
    pre = acc + (_f64(res) if res is not None else 0.0)
    pre = pre * f32(scale)
    return pre, r16(pre, dtype)


def gate_residual_ref(acc, gate_rows, dtype):
    """primx_linear_gate_residual: the increment cast16(gate * cast16(A W^T + bias)); gate_rows = the gate of each row."""
    pre = _f64(gate_rows) * r16(acc, dtype)
    return pre, r16(pre, dtype)


def layernorm_modulate_ref(x, shift_rows, scale_rows, dtype, eps=1e-6):
    """primx_layernorm_modulate: LN(x) * cast16(1 + scale) + shift, one rounding at the end (x fp32, exact statistics)."""
    xd = _f64(x)
    mu = xd.mean(-1, keepdims=True)
    var = ((xd - mu) ** 2).mean(-1, keepdims=True)
    m1 = r16(1.0 + _f64(scale_rows), dtype)
    pre = (xd - mu) / np.sqrt(var + f32(eps)) * m1 + _f64(shift_rows)
    return pre, r16(pre, dtype)


LN_FLT_MAX = 88.72283905206835   # ln of the largest fp32 value


def silu64(x):
    """x / (1 + exp(-x)) - the formula torch (and the kernels) evaluate in fp32, whose exp(-x) overflows below
    -LN_FLT_MAX and then gives -0; primx_silu_cast documents that behaviour."""
    x = _f64(x)
    with np.errstate(over="ignore"):
        return np.where(-x > LN_FLT_MAX, -0.0, x / (1.0 + np.exp(-x)))


def silu_cast_ref(x, dtype):
    pre = silu64(x)
    return pre, r16(pre, dtype)


def cast16_ref(x, dtype):
    pre = _f64(x)
    return pre, r16(pre, dtype)


def cfg_combine_ref(cond, uncond, s, dtype):
    """primx_cfg_combine: uncond + s * (cond - uncond), every operation rounded."""
    c, u = _f64(cond), _f64(uncond)
    d = r16(c - u, dtype)
    m = r16(f32(s) * d, dtype)
    pre = u + m
    return pre, r16(pre, dtype)


def groupnorm64(x, gamma, beta, groups, eps):
    """GroupNorm of [P, V, C] channels-last blocks in float64 (statistics per primitive and group)."""
    xd = _f64(x)
    P, V, C = xd.shape
    g = xd.reshape(P, V, groups, C // groups)
    mu = g.mean(axis=(1, 3), keepdims=True)
    var = ((g - mu) ** 2).mean(axis=(1, 3), keepdims=True)
    y = ((g - mu) / np.sqrt(var + f32(eps))).reshape(P, V, C)
    return y * _f64(gamma) + _f64(beta)


def groupnorm_silu_ref(x, gamma, beta, groups, eps, silu, dtype):
    pre = groupnorm64(x, gamma, beta, groups, eps)
    if silu:
        pre = silu64(pre)
    return pre, r16(pre, dtype)


def im2col3(x, S):
    """[P, S^3, C] -> [P * S^3, 27 * C] with k = tap * C + ci (tap = (dz * 3 + dy) * 3 + dx), zero padding 1."""
    xd = _f64(x)
    P, V, C = xd.shape
    g = np.zeros((P, S + 2, S + 2, S + 2, C))
    g[:, 1:-1, 1:-1, 1:-1] = xd.reshape(P, S, S, S, C)
    cols = [g[:, dz:dz + S, dy:dy + S, dx:dx + S] for dz in range(3) for dy in range(3) for dx in range(3)]
    return np.concatenate(cols, axis=-1).reshape(P * V, 27 * C)


def conv3d_k3_acc(x, Wk, bias, S):
    """Exact 3x3x3 convolution of primx_conv3d_k3 (Wk [Cout, Kpad], k = tap * Cin + ci): [P * S^3, Cout]."""
    cols = im2col3(x, S)
    K = cols.shape[1]
    return gemm_acc(cols, _f64(Wk)[:, :K], bias)


def convtranspose_k2s2_acc(x, Wt, bias, S):
    """Exact ConvTranspose3d(k=2, s=2) of primx_convtranspose_k2s2 -> [P, (2S)^3, Cout]."""
    xd = _f64(x)
    P, V, Cin = xd.shape
    Cout = _f64(Wt).shape[0] // 8
    y = (xd.reshape(P * V, Cin) @ _f64(Wt).T).reshape(P, S, S, S, 2, 2, 2, Cout)    # row = tap * Cout + co
    y = y.transpose(0, 1, 4, 2, 5, 3, 6, 7).reshape(P, 8 * V, Cout)
    return y + _f64(bias)


def conv_in_acc(z, pq_scale, pq_bias, W, bias, S):
    """Exact conv_in: Conv3d(1 -> Cout, k3, p1) of the affine z' = a z + b (zero padding after the affine)."""
    zd = f32(pq_scale) * _f64(z) + f32(pq_bias)
    P = zd.shape[0]
    cols = im2col3(zd.reshape(P, S ** 3, 1), S)
    return gemm_acc(cols, W, bias).reshape(P, S ** 3, -1)


# ------------------------------------------------------------------------------------------------ the check
# Criterion 2's allowance.  A kernel accumulates in fp32; its value in front of the first rounding differs from the exact
# one by the accumulated fp32 rounding errors.  Each of the K additions adds an error of at most 2^-24 of the running partial
# sum, modelled as independent and uniform (standard deviation 2^-24 |s_k| / sqrt(3)); with partial sums of root-mean-square
# size at most rms(y) the total has standard deviation sigma <= 2^-24 sqrt(K / 3) rms(y) = 0.58 * 2^-24 sqrt(K) rms(y).  An
# element whose exact value lies uniformly inside its 16-bit rounding interval then changes its rounded value with
# probability E|err| / ulp16 = 0.8 sigma / ulp16 <= 0.46 * 2^-24 sqrt(K) rms(y) / ulp16.  C_ACC = 2 allows four times that
# ceiling for what the model leaves out (blocked MFMA summation orders, a few large partial sums in a skewed row):
#     allowed fraction = mean_i min(1, C_ACC * sqrt(K) * 2^-24 * rms(y) / ulp16(y_i))     (rms over the element's row)
# which is about 2.5 % for fp16 and 0.35 % for bf16 at K = 1152 with y ~ N(0, 1) (small |y_i| have small ulps).  Element-wise
# fp32 stages after the first rounding (activation, scale, LayerNorm's rsqrt) add `ew_ulps` fp32 ulps of relative error:
#     + mean_i min(1, 2 ew_ulps 2^-24 |pre_i| / ulp16(pre_i)).
# Criterion 1 ("within 1 ulp16") is measured against the larger of ulp16(ref_i) and 2 C_ACC sqrt(K) 2^-24 rms(y) gain_i: an
# element that cancels down to a few ulps of the accumulation noise cannot be held to its own, much finer, 16-bit spacing
# (gain_i: how much the operations after the accumulation scale its error - the gate of a gated residual, out_scale).  An
# inner rounding that flips by one ulp (allowed when its input lies inside that noise) moves the result by `inner_i` - e.g.
# |gate_i| ulp16(y_i) behind the inner cast16 of a gated residual - which the tolerance of criterion 1 adds.  `extra_i`: an
# expected absolute perturbation from rounding decisions made INSIDE the kernel on its inputs (the normalised activations of a
# convolution with the GroupNorm inside: sum over the taps of |w| ulp16(a) P(a flips)); it enters criterion 2's allowance.
C_ACC = 2.0
BIAS_LIMIT = 0.05


class ContractReport(dict):
    def __str__(self):
        return ", ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in self.items())


def contract_report(got, exact_pre, ref, dtype, K, acc=None, ew_ulps=0.0, c=C_ACC, gain=1.0, inner=0.0,
                    extra=0.0) -> ContractReport:
    g, pre, rf = _f64(got).ravel(), _f64(exact_pre).ravel(), _f64(ref).ravel()
    a_full = _f64(exact_pre if acc is None else acc)
    a_full = np.broadcast_to(a_full, _f64(exact_pre).shape)
    a = a_full.ravel()
    gn = np.broadcast_to(np.abs(_f64(gain)), _f64(exact_pre).shape).ravel()
    n = g.size
    fin = np.isfinite(rf)
    rep = ContractReport(n=n)
    # rms(y): over the last axis (one output row shares its A row / its input patch); per element for 1-D (element-wise) data
    af = np.where(np.isfinite(a_full), a_full, 0.0)
    rms = np.sqrt(np.mean(af ** 2, axis=-1, keepdims=True)) if af.ndim >= 2 else np.abs(af)
    noise = c * math.sqrt(K) * 2.0 ** -24 * np.broadcast_to(rms, a_full.shape).ravel()
    u = np.maximum(ulp16(rf, dtype), 2.0 * noise * gn) + np.broadcast_to(np.abs(_f64(inner)), _f64(exact_pre).shape).ravel()
    # 1. special values: the same inf / NaN in the same places with the same sign - except where the exact value lies within
    # the tolerance below of the overflow threshold (largest finite + half its ulp), a rounding boundary like any other
    _, _, fmax = _FMT[dtype]
    thr = fmax + ulp16(fmax, dtype) / 2
    mism = (np.isinf(g) != np.isinf(rf)) | (np.isnan(g) != np.isnan(rf)) | (np.isinf(rf) & (np.sign(g) != np.sign(rf)))
    with np.errstate(invalid="ignore"):
        edge = (np.abs(np.abs(pre) - thr) <= u) & np.isin(np.abs(g), (fmax, np.inf)) & np.isin(np.abs(rf), (fmax, np.inf)) & \
            (np.sign(g) == np.sign(rf))
    rep["special_mismatch"] = int(np.sum(mism & ~edge))
    rep["overflow_edge"] = int(np.sum(mism & edge))
    ok = fin & np.isfinite(g)
    with np.errstate(invalid="ignore"):
        d = np.abs(g - rf)
    rep["max_ulp"] = float(np.max(d[ok] / u[ok])) if ok.any() else 0.0
    # 2. how many differ, against the allowance derived above
    rep["differ"] = int(np.sum(ok & (g != rf))) + rep["overflow_edge"]
    p_acc = np.minimum(1.0, (noise + np.broadcast_to(np.abs(_f64(extra)), _f64(exact_pre).shape).ravel()) / ulp16(a, dtype))
    ew = np.broadcast_to(_f64(ew_ulps), _f64(exact_pre).shape).ravel()
    p_ew = np.minimum(1.0, 2.0 * ew * 2.0 ** -24 * np.abs(np.where(np.isfinite(pre), pre, 0.0)) / ulp16(pre, dtype))
    expect = float(np.sum(np.minimum(1.0, p_acc + p_ew)[fin]))
    rep["allowed"] = expect + 3.0 * math.sqrt(expect) + 3.0      # + counting noise of a sum of Bernoulli trials
    rep["differ_frac"] = rep["differ"] / max(1, n)
    rep["allowed_frac"] = rep["allowed"] / max(1, n)
    # 3. bias in units of the contract result's ulp, signed towards larger magnitude
    sel = ok & np.isfinite(pre) & (pre != 0)
    rep["bias"] = float(np.mean((g[sel] - pre[sel]) * np.sign(pre[sel]) / ulp16(pre[sel], dtype))) if sel.any() else 0.0
    rep["bias_n"] = int(sel.sum())
    return rep


def check_contract(got, exact_pre, ref, dtype, K, acc=None, ew_ulps=0.0, c=C_ACC, gain=1.0, inner=0.0, extra=0.0,
                   what="") -> ContractReport:
    """Assert that `got` keeps the rounding contract whose float64 value in front of the last rounding is `exact_pre` and
    whose correctly rounded result is `ref` (= round16(exact_pre), after any inner roundings).  K: length of the fp32
    accumulation in front of the first rounding; acc: the exact value there (default exact_pre).
      1. every element within 1 ulp16 of ref (see above for elements inside the accumulation noise); inf / NaN identical
         in position and sign;
      2. at most the allowance (C_ACC, above) of elements differ from ref at all;
      3. the mean signed error in ulps is within +-BIAS_LIMIT (truncation gives about -0.5)."""
    rep = contract_report(got, exact_pre, ref, dtype, K, acc, ew_ulps, c, gain, inner, extra)
    tag = f"{what} {dtype}: {rep}"
    assert rep["special_mismatch"] == 0, "inf / NaN differ from the contract: " + tag
    assert rep["max_ulp"] <= 1.0, "more than 1 ulp from the contract: " + tag
    assert rep["differ"] <= rep["allowed"], "too many elements differ from the contract: " + tag
    if rep["bias_n"] >= 1000:
        assert abs(rep["bias"]) <= BIAS_LIMIT, "biased rounding: " + tag
    return rep


def gemm_abs_bound(A, W, bias=None, extra_terms=0) -> np.ndarray:
    """Rigorous bound of an fp32-accumulated A W^T + bias (fp32 inputs, any summation order, FMA or not):
    gamma_n * (sum_k |a_k||w_k| + |bias|), gamma_n = n u / (1 - n u), u = 2^-24, n = K + 1 + extra_terms."""
    Ad, Wd = _f64(A), _f64(W)
    s = np.abs(Ad) @ np.abs(Wd).T
    if bias is not None:
        s = s + np.abs(_f64(bias))[None, :]
    n = Ad.shape[1] + 1 + extra_terms
    u = 2.0 ** -24
    return (n * u / (1 - n * u)) * s


# ------------------------------------------------------------------------------------------------ the LayerNorm fold
# include/primx_hip.h "The LayerNorm fold": with the row statistics mu, rho of the fp32 residual stream x, m = cast16(1 + scale),
# a centre c and a scale rho_p per row,
#     reference:  y = cast16( cast16( (x - mu) rho m + shift ) W^T + b )
#     folded:     y = cast16( (rho / rho_p) a16 W^T - rho mu' u + v ),   a16 = cast16((x - c) rho_p m),  mu' = mean(x - c),
#                 u = m W^T,  v = shift W^T + b  (fp32 rows)
# The consumer's contract takes a16, the producer's partial sums `part`, the pairs `center` and the fp32 u, v AS GIVEN: the value in
# front of its first rounding is the fold formula with float64 statistics of those partial sums and the exact a16 W^T.
U32 = 2.0 ** -24
GELU_LIPSCHITZ = 1.13      # max |d/dy gelu_tanh(y)| = 1.129 (at y = 1.5; the minimum is -0.13)


def _rel_rsqrt_err(a):
    """Largest relative change of 1 / sqrt(w) when w changes by a relative amount in [-a, a] (inf from a >= 1 on)."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a < 1.0, np.maximum(1.0 / np.sqrt(np.maximum(1.0 - a, 1e-300)) - 1.0, 1.0 - 1.0 / np.sqrt(1.0 + a)), np.inf)


def fold_partials_err(x, center, tile=144):
    """Per-row bounds (d1, d2) of the PRODUCER's fp32 error in sum_k (x_k - c) and sum_k (x_k - c)^2 (over all column tiles), for
    comparing `center_out` with the float64 statistics of x itself.  d = fl(x - c) is off by u |x - c|; a tile sums 144 terms in a
    fixed order of depth < 144 (gamma_143 of the sum of magnitudes; d^2 adds one rounding and the square doubles d's):
        d1 = gamma_145 sum_k |x_k - c|,   d2 = gamma_147 sum_k (x_k - c)^2,   gamma_n = n u / (1 - n u), u = 2^-24."""
    xd = _f64(x)
    c = _f64(center)[:, :1]
    d = np.abs(xd - c)
    g = lambda n: n * U32 / (1 - n * U32)
    return g(tile + 1) * d.sum(-1), g(tile + 3) * (d * d).sum(-1)


def fold_stats_ref(part, center, K, eps, part_err=None) -> dict:
    """float64 statistics of a folded site from the partial sums `part` [M, P, 2] and the pairs `center` [M, 2] as given (the
    consumer's input), and a bound on the CONSUMER's fp32 error in them (fold_stats_finish in csrc/gemm.hip).

    Values: s1, s2 = the sums over the P partials; mu' = s1 / K, var = max(s2 / K - mu'^2, 0), rho = 1 / sqrt(var + eps),
    center_out = (c + mu', rho).

    Error bound (u = 2^-24, first order, x 1.01 for the second-order terms).  The kernel adds the P partials in order (gamma_{P-1}
    of their magnitudes), multiplies by fl(1 / K) (two roundings), so
        e_mu  = u ((P - 1) sum |s1_i| / K + 2 |mu'|).
    E2 = s2 / K carries (P + 1) u E2 the same way; fl(mu^2) adds 2 |mu'| e_mu + u mu'^2; the difference one more u |var|:
        e_var = u ((P + 1) E2 + mu'^2 + |var|) + 2 |mu'| e_mu  =  u ((P + 2) var + (P + 2) mu'^2) + ...,
    i.e. relative to var a cancellation factor (1 + mu'^2 / var) - the price of var = E[(x - c)^2] - mu'^2 with a stale centre.
    The clamp at 0 is 1-Lipschitz; + eps adds u (var + eps); sqrtf and the reciprocal are correctly rounded (no fast-math):
        rel_rho = rsqrt_err((e_var + u (var + eps)) / (var + eps)) + 2 u       (rsqrt_err(a) ~ a / 2 for small a).
    center_out[0] = fl(c + mu'_f): e_mu + u |c + mu'|;  center_out[1] = rho_f: rel_rho rho.
    part_err = (d1, d2) per row (fold_partials_err): the producer's error in s1, s2 against x itself - then the bounds hold
    against the float64 statistics of x (e_mu += d1 / K, e_var += d2 / K + 2 |mu'| d1 / K)."""
    p = _f64(part)
    cen = _f64(center)
    P = p.shape[-2]
    s1, s2 = p[..., 0].sum(-1), p[..., 1].sum(-1)
    mu = s1 / K
    e2 = s2 / K
    raw = e2 - mu * mu
    var = np.maximum(raw, 0.0)
    epsf = f32(eps)
    rho = 1.0 / np.sqrt(var + epsf)
    e_mu = U32 * ((P - 1) * np.abs(p[..., 0]).sum(-1) / K + 2.0 * np.abs(mu))
    e_var = U32 * ((P + 1) * np.abs(e2) + mu * mu + np.abs(raw)) + 2.0 * np.abs(mu) * e_mu
    if part_err is not None:
        d1, d2 = (_f64(t) for t in part_err)
        e_mu = e_mu + d1 / K
        e_var = e_var + d2 / K + 2.0 * np.abs(mu) * d1 / K
    e_mu, e_var = 1.01 * e_mu, 1.01 * e_var
    rel_rho = _rel_rsqrt_err((e_var + U32 * (var + epsf + e_var)) / (var + epsf)) + 2.0 * U32
    c, rho_p = cen[:, 0], cen[:, 1]
    center_out = np.stack([c + mu, rho], -1)
    e_center = np.stack([e_mu + U32 * (np.abs(c + mu) + e_mu), rel_rho * rho], -1)
    return dict(mu=mu, var=var, rho=rho, c=c, rho_p=rho_p, K=K, center_out=center_out, e_mu=e_mu, e_var=e_var, rel_rho=rel_rho,
                e_center=e_center)


def check_fold_center(got, stats, what="") -> float:
    """center_out against fold_stats_ref: every pair within the derived fp32 bound.  Returns the largest fraction of it used."""
    g = _f64(got)
    assert np.all(np.isfinite(g)), f"{what}: center_out not finite"
    err = np.abs(g - stats["center_out"])
    frac = float(np.max(err / np.maximum(stats["e_center"], 1e-300)))
    assert frac <= 1.0, f"{what}: center_out off by {frac:.3g} x its bound (row {int(np.argmax(np.max(err / stats['e_center'], -1)))})"
    return frac


def fold_value(acc, stats, u, v):
    """The consumer's value in front of its first rounding: (rho / rho_p) acc - rho mu' u + v (float64; acc = exact a16 W^T)."""
    g = (stats["rho"] / stats["rho_p"])[:, None]
    return g * _f64(acc) - (stats["rho"] * stats["mu"])[:, None] * _f64(u)[None, :] + _f64(v)[None, :]


def fold_consumer_ref(acc, stats, u, v, dtype, act=0, scale0=1.0):
    """(pre, ref) of a fold consumer (primx_linear_heads_fold / primx_linear_fold): one rounding after the fold value; heads
    segment 0 with scale0 != 1: a second rounding after the scale (primx_linear_heads: "multiplied by scale0 after rounding");
    act: the activation between two roundings, as linear_ref."""
    pre = fold_value(acc, stats, u, v)
    y = r16(pre, dtype)
    if f32(scale0) != 1.0:
        pre = f32(scale0) * y
        y = r16(pre, dtype)
    if act:
        pre = act64(y, act)
        y = r16(pre, dtype)
    return pre, y


def fold_epilogue_err(y_minus_v, y, u, stats):
    """Bound of the consumer epilogue's fp32 error in its value (beyond the accumulation's): with st0 = fl(rho_p mu'_f),
    st1 = fl(rho_f / rho_p), t = fma(-st0, u, acc), y = fma(st1, t, v) and the statistics' errors of fold_stats_ref,
        |y_f - y| <= (rel_rho + 2 u) |y - v| + rho (e_mu + u |mu'|) |u| + u |y|      (x 1.01)
    because (rho / rho_p) |acc - rho_p mu' u| = |y - v|.  Arguments are magnitudes per element ([M, N]) / per column (u)."""
    rr = (stats["rel_rho"] + 2.0 * U32)[:, None]
    em = (stats["rho"] * (stats["e_mu"] + U32 * np.abs(stats["mu"])))[:, None]
    return 1.01 * (rr * np.abs(_f64(y_minus_v)) + em * np.abs(_f64(u))[None, :] + U32 * np.abs(_f64(y)))


def fold_contract_kw(acc, mag, stats, u, v, dtype, K, act=0, scale0=1.0, rms_axis=-1) -> dict:
    """check_contract's arguments for a fold consumer.  acc = the exact a16 W^T, mag = its natural size per element
    (max(sqrt(sum_k a_k^2 w_k^2), |acc|): the size of the partial sums the fp32 accumulation rounds).

    check_contract models the accumulation noise from the rms over a row of the value in front of the first rounding, y0.  Here
    the fp32 accumulation runs on a16 W^T and is scaled by the fold's gain rho / rho_p, and - mu' u cancels part of it, so the
    noise is C_ACC sqrt(K) 2^-24 (rho / rho_p) mag: `gain` carries that ratio into criterion 1, `extra` the part of it above
    check_contract's own noise into criterion 2.  The epilogue's fp32 error (fold_epilogue_err: the statistics, st0 / st1 and the
    two fused multiply-adds) is an expected perturbation of y0 (`extra`) and widens criterion 1 (`inner`).  A second stage (the
    scale0 of heads segment 0, the GELU) multiplies everything by |scale0| or GELU_LIPSCHITZ and lets y0's rounding flip by one
    ulp16(y0) (`inner`), as in linear_ref's cases; the GELU's own fp32 error is derived below (`ew_ulps`).  rms_axis = 0 for outputs
    checked column by column (check_contract on transposed arrays: the rms it bases its noise on is then a column's)."""
    y0 = fold_value(acc, stats, u, v)
    g = (stats["rho"] / stats["rho_p"])[:, None]
    rms = np.sqrt(np.mean(np.where(np.isfinite(y0), y0, 0.0) ** 2, axis=rms_axis, keepdims=True))
    scale = C_ACC * math.sqrt(K) * 2.0 ** -24
    noise_c = scale * rms
    noise_t = scale * g * _f64(mag)
    E = fold_epilogue_err(y0 - _f64(v)[None, :], y0, u, stats)
    staged = f32(scale0) != 1.0 or act != 0
    sg = abs(f32(scale0)) if f32(scale0) != 1.0 else (GELU_LIPSCHITZ if act else 1.0)
    gain = sg * noise_t / np.maximum(noise_c, 1e-300)
    inner = sg * (E + (ulp16(y0, dtype) if staged else 0.0))
    ew = 4.0 if staged else 0.0
    if act == 1:
        # GELU-tanh in fp32 is 0.5 y (1 + tanh(z)): tanh is good to a few ulps of 1, so the error is ABSOLUTE, about 0.5 |y| 4 u (+ the
        # argument's 3 u |z| through tanh' = 1 - t^2, + 3 u |gelu| for the products) - many ulps of the result where 1 + tanh(z) cancels
        # (y below -3), which the relative ew_ulps of linear_ref's cases does not cover.  In u32 units of |gelu(y)|:
        yr = r16(y0, dtype)
        z = math.sqrt(2.0 / math.pi) * (yr + 0.044715 * yr ** 3)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ga = np.abs(gelu_tanh64(yr))
            ew = np.where(ga > 0, (0.5 * np.abs(yr) * (4.0 + 3.0 * np.abs(z) * (1.0 - np.tanh(z) ** 2)) + 3.0 * ga) / ga, 4.0)
        ew = np.where(np.isfinite(ew), ew, 1e30)
    return dict(acc=y0, gain=gain, extra=np.maximum(noise_t - noise_c, 0.0) + E, inner=inner, ew_ulps=ew)


def fold_site_bound(x, center, m, shift, W, b, a16, stats, u, v, dtype, act=0, scale0=1.0, eps=1e-6, mm=None):
    """The folded output against the reference's UNFOLDED arithmetic, cast16(cast16(LN(x) m + shift) W^T + b) in float64 (LN with
    the exact statistics of the fp32 rows x), and a per-element bound of their difference.  Returns (ref_out, bound).

    From the header's identity, (rho / rho_p) a W^T - rho mu' u + v = rho (x - mu) m W^T + shift W^T + b for a = (x - c) rho_p m
    exactly.  The two pre-rounding values differ by (u16 = 2^-p, the 16-bit unit roundoff; fp16 adds 2^-25 per subnormal term):
      D1  the a16 rounding (and the three fp32 roundings in front of it): rho (u16 + 3 u) sum_k |x_k - c| |m_k| |w_k|;
      D2  the reference's own rounding of the LayerNorm output: u16 sum_k |LN_k m_k + shift_k| |w_k|;
      D3  the fp32 accumulation of a16 W^T (rigorous): (rho / rho_p) gamma_K sum_k |a16_k| |w_k|;
      D4  the statistics (stats from fold_stats_ref WITH part_err: against x itself), st0 / st1 and the fused multiply-adds:
          fold_epilogue_err with |y - v| <= |pre_ref - v| + D2;
      D5  the fp32 rows u, v (gemm_abs_bound of [m; shift] W^T): rho |mu'| du + dv.
    Both sides then round once (<= ulp16 apart beyond D); scale0 / GELU multiply by |scale0| / GELU_LIPSCHITZ and round again.
    mm(A, B) = A @ B^T in float64 (numpy by default; the GPU tests pass a device matmul)."""
    mm = mm or (lambda A_, B_: _f64(A_) @ _f64(B_).T)
    xd = _f64(x)
    c = _f64(center)[:, :1]
    md, sd, Wd = _f64(m), _f64(shift), _f64(W)
    bd = _f64(b) if b is not None else np.zeros(Wd.shape[0])
    mu = xd.mean(-1, keepdims=True)
    rho = 1.0 / np.sqrt(((xd - mu) ** 2).mean(-1, keepdims=True) + f32(eps))
    lnm = (xd - mu) * rho * md[None, :] + sd[None, :]
    pre_ref = mm(r16(lnm, dtype), Wd) + bd[None, :]
    p, _, _ = _FMT[dtype]
    u16 = 2.0 ** -p
    sub = 2.0 ** -25 if dtype == torch.float16 else 0.0
    aW = np.abs(Wd)
    colsum = aW.sum(-1)[None, :]
    g = (stats["rho"] / stats["rho_p"])[:, None]
    d1 = rho * (u16 + 3 * U32) * mm(np.abs(xd - c) * np.abs(md)[None, :], aW) + g * sub * colsum
    d2 = u16 * mm(np.abs(lnm), aW) + sub * colsum
    K = Wd.shape[1]
    d3 = g * (K * U32 / (1 - K * U32)) * mm(np.abs(_f64(a16)), aW)
    v_ex = sd @ Wd.T + bd
    u_ex = md @ Wd.T
    du = gemm_abs_bound(md[None, :], Wd)[0]
    dv = gemm_abs_bound(sd[None, :], Wd, b)[0]
    d4 = fold_epilogue_err(np.abs(pre_ref - v_ex[None, :]) + d2, np.abs(pre_ref) + d1 + d2, np.abs(u_ex) + du, stats)
    d5 = (stats["rho"] * np.abs(stats["mu"]))[:, None] * du[None, :] + dv[None, :]
    D = d1 + d2 + d3 + d4 + d5
    y_ref = r16(pre_ref, dtype)
    _, _, fmax = _FMT[dtype]
    with np.errstate(invalid="ignore", over="ignore"):
        bound = D + ulp16(np.abs(pre_ref) + D, dtype)
        edge = np.abs(np.abs(pre_ref) - (fmax + ulp16(fmax, dtype) / 2)) <= bound     # either side may overflow
        out = y_ref
        if f32(scale0) != 1.0:
            s = abs(f32(scale0))
            out = r16(f32(scale0) * y_ref, dtype)
            bound = s * bound + ulp16(s * (np.abs(y_ref) + bound), dtype)
        if act:
            out = r16(act64(y_ref, act), dtype)
            bound = GELU_LIPSCHITZ * bound + ulp16(np.abs(out) + GELU_LIPSCHITZ * bound, dtype) + 4 * U32 * np.abs(out)
    return out, 1.01 * bound, edge


def check_fold_site(got, ref_out, bound, edge, dtype, what="") -> float:
    """Every element within the site bound of fold_site_bound, except where the unfolded value in front of the first rounding lies
    within its bound of the overflow threshold (`edge`: either side may overflow there, and a GELU of -inf is NaN); elsewhere the
    same inf / NaN on both sides.  Returns the largest fraction of the bound used."""
    g, r = _f64(got), _f64(ref_out)
    both = np.isfinite(g) & np.isfinite(r) & ~edge
    frac = float(np.max(np.abs(g - r)[both] / bound[both])) if both.any() else 0.0
    one = ~edge & ((np.isfinite(g) != np.isfinite(r)) | (np.isinf(g) & np.isinf(r) & (np.sign(g) != np.sign(r))))
    assert not one.any(), f"{what}: {int(one.sum())} elements are inf / NaN on one side only, away from the overflow threshold"
    assert frac <= 1.0, f"{what}: folded output off the unfolded reference by {frac:.3g} x the site bound"
    return frac
