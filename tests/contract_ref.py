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


# ------------------------------------------------------------------------------------------------ 16-bit attention
# attn_kernel / attn64_kernel are not one-rounding operations.  csrc/attention.hip documents what they approximate:
#   dh = 72 (Q carries the mask / max columns): Q pre-scaled by c = scale log2(e) and rounded to 16 bits; the running max held
#     as two 16-bit halves; P = exp2(s - m) packed round-toward-zero (fp16) / truncated (bf16) and used for BOTH the numerator
#     and the denominator (the all-ones row of V^T);
#   dh = 32 / 64 and the 64-token kernel: logits scaled in fp32; P rounded to nearest for the numerator, the denominator summed
#     from the unrounded fp32 P;
#   fp32 O and row sum, one reciprocal, one final rounding.
# With w_j = softmax weights, out = sum_j w_j v_j, and relative weight errors eta_j, the output moves by
#   sum_j w_j eta_j (v_j - out)   when numerator and denominator carry the same eta_j (a common factor cancels), and
#   sum_j w_j eta_j v_j           when only the numerator does.
# So, per element:  bound = 0.5 ulp16(out) + ln2 sum_j w_j |v_j - out| ds_j + dP sum_j w_j A_j + floor + fp32 terms, with
#   ds_j = (u_q + (dh + 4) 2^-24) sum_d |q_d c k_jd| + 2^-22 max_j |s_j|   (exp2 units: Q's rounding u_q = 2^-11 / 2^-8 on the
#          dh = 72 path, 0 else; fp32 accumulation of dh + 3 products and of c; the max's split and the exp2 argument),
#   dP   = the pack's relative error (2^-10 / 2^-7 toward zero on the dh = 72 path, 2^-11 / 2^-8 to nearest else) + 2^-22 (v_exp),
#   A_j  = |v_j - out| (same P in both sums) or |v_j| (numerator only),
#   floor = 2^-24 sum_j A_j / L for fp16 (subnormal / flushed P below 2^-14 against the running max; L = sum_j 2^(s_j - max)),
#   fp32 = gamma_nkv (sum_j w_j |v_j| + |out|) + 2^-22 |out|   (accumulation of O and of the row sum; the reciprocal and product).
ATTN_SLACK = 2.0


def attn_bound(q, k, v, scale, dtype, same_p):
    """Exact output [B, Mq, H, dh] and the per-element bound above (float64 on q's device)."""
    B, Mq, H, dh = q.shape
    nkv = k.shape[1]
    dev = q.device
    c = f32(f32(scale) * 1.4426950408889634)
    f16 = dtype == torch.float16
    u_q = (2.0 ** -11 if f16 else 2.0 ** -8) if same_p else 0.0      # (same_p: the dh = 72 path)
    dP = ((2.0 ** -10 if f16 else 2.0 ** -7) if same_p else (2.0 ** -11 if f16 else 2.0 ** -8)) + 2.0 ** -22
    gam = nkv * 2.0 ** -24 / (1 - nkv * 2.0 ** -24)
    outs, bounds = torch.empty(B, Mq, H, dh, dtype=torch.float64, device=dev), torch.empty(B, Mq, H, dh, dtype=torch.float64, device=dev)
    for b in range(B):
        for h in range(H):
            Q, K, V = q[b, :, h].double(), k[b, :, h].double(), v[b, :, h].double()
            S2 = (Q @ K.t()) * f32(scale) * 1.4426950408889634            # exact logits, exp2 units
            m = S2.max(1, keepdim=True).values
            Pm = torch.pow(2.0, S2 - m)
            L = Pm.sum(1, keepdim=True)
            w = Pm / L
            out = w @ V
            ds = (u_q + (dh + 4) * 2.0 ** -24) * ((Q.abs() @ K.abs().t()) * c) + 2.0 ** -22 * S2.abs().max(1, keepdim=True).values
            D = (V[None] - out[:, None]).abs()                                 # [Mq, nkv, dh]
            A = D if same_p else V.abs()[None].expand_as(D)
            E = np.log(2.0) * torch.einsum("qj,qjd->qd", w * ds, D) + dP * torch.einsum("qj,qjd->qd", w, A)
            if f16:
                E = E + 2.0 ** -24 * A.sum(1) / L
            E = E + gam * (w @ V.abs() + out.abs()) + 2.0 ** -22 * out.abs()
            outs[b, :, h], bounds[b, :, h] = out, E
            del D, A
    return outs, bounds


def attn_report(got, q, k, v, scale, dtype, same_p, ref=None):
    """(ratio, signed) without an assertion: ratio = max |err| / bound (NaN when `got` holds a NaN), signed = the signed errors
    in ulps of the result, sign taken along the result, over the elements that do not cancel to near zero (the sample of the
    bias criterion below).  ref = attn_bound's (out, E) as numpy arrays when the caller holds several outputs to one input."""
    if ref is None:
        out, E = attn_bound(q, k, v, scale, dtype, same_p)
        ref = out.cpu().numpy(), E.cpu().numpy()
    out_np, E_np = ref
    bound = 0.5 * ulp16(out_np, dtype) + E_np
    g = _f64(got).reshape(out_np.shape)
    ratio = float(np.max(np.abs(g - out_np) / bound))
    rms = float(np.sqrt(np.mean(out_np ** 2)))
    sel = np.abs(out_np) >= 0.25 * rms
    signed = (g - out_np)[sel] * np.sign(out_np[sel]) / ulp16(out_np[sel], dtype)
    return ratio, signed


def attn_check(got, q, k, v, scale, dtype, same_p, what, bias=True, quiet=False):
    """bias=False: only the bound is asserted and (ratio, signed errors) come back, for a caller that pools the bias statistic
    over many cells (tests/test_hip_attention_grid.py): on one tiny cell it is taken over too few values, and under the sentinel
    patterns of attn_inputs the correctly rounded result itself is biased (the residual weight pulls every element one way)."""
    ratio, signed = attn_report(got, q, k, v, scale, dtype, same_p)
    if not quiet:
        print(f"attention {what} {dtype}: max |err| / bound = {ratio:.3f}")
    assert ratio <= ATTN_SLACK, f"attention {what} {dtype}: error {ratio:.3f} x the derived bound"
    if not bias:
        return ratio, signed
    # no bias: the mean signed error in ulps of the result, over the elements that do not cancel to near zero.  Asserted where
    # every documented approximation is unbiased (P rounded to nearest).  The dh = 72 path packs P toward zero by design: a key
    # at the running max keeps p = 1 exactly while every other key loses 2^-11 (fp16) / 2^-8 (bf16) of its weight on average,
    # which pulls the output towards the dominant key's value - inside the bound above, but a bias; it is reported only.
    mean_signed = float(np.mean(signed))
    print(f"attention {what} {dtype}: mean signed error {mean_signed:+.3f} ulp")
    if not same_p:
        assert abs(mean_signed) <= BIAS_LIMIT, f"attention {what} {dtype}: biased by {mean_signed:.3f} ulp"
    return ratio


# Inputs under which EACH KEY decides the result.  Dense random inputs give one key of nkv a weight of about 1 / nkv, which is
# inside the approximation error the bound above grants: an off-by-one in the key mask ships unnoticed (pinned by
# tests/test_attention_grid_cpu.py::test_random_inputs_alone_miss_the_unmasked_pad).  Two sentinel patterns close that:
#   lookup: k rows N(0, 1) scaled to |k_j| = sqrt(dh), q_i = 3 k_j(i) with j(i) = (nkv - 1 - i) mod nkv (query 0 looks up the LAST
#           valid key), v N(0, 1).  The chosen key's logit is 3 sqrt(dh), the others' are N(0, 9): out_i ~ v_j(i), and a dropped,
#           swapped or misplaced key, a skipped tile or a V^T tile paired with the wrong K tile moves the affected rows by O(1);
#   trap:   q, k = 0.3 N(0, 1) with q[..., 0] = c, k[..., 0] = -c, c = sqrt(17 sqrt(dh)): every real logit is about -17 nats, so a
#           pad key that reaches the softmax with score 0 takes all the weight and the row (v = 1 + 0.5 N(0, 1)) collapses from
#           about 1 to about 0.  On the dh = 72 path the first tile's max is a large NEGATIVE step from the initial m_run = 0.
# The numbers come from a CPU generator whatever the device, so the CPU proof and the GPU grid see the same tensors.
ATTN_PATTERNS = ("random", "lookup", "trap")
ATTN_SIGMAS = (0.5, 4.0, 16.0)


def attn_inputs(pattern, seed, B, Mq, Mk, H, dh, device, sigma=1.0):
    """fp32 q [B, Mq, H, dh], k, v [B, Mk, H, dh] on `device` (the caller rounds them to the 16-bit type); sigma: `random` only."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda n: torch.randn(B, n, H, dh, generator=g)
    if pattern == "random":
        q, k, v = rn(Mq) * sigma, rn(Mk), rn(Mk)
    elif pattern == "lookup":
        k = rn(Mk)
        k = k * (dh ** 0.5 / k.norm(dim=-1, keepdim=True))
        q = 3.0 * k[:, (Mk - 1 - torch.arange(Mq)) % Mk]
        v = rn(Mk)
    elif pattern == "trap":
        c = (17.0 * dh ** 0.5) ** 0.5
        q, k, v = 0.3 * rn(Mq), 0.3 * rn(Mk), 1.0 + 0.5 * rn(Mk)
        q[..., 0], k[..., 0] = c, -c
    else:
        raise ValueError(pattern)
    return q.to(device), k.to(device), v.to(device)


def trunc16(x, dtype) -> np.ndarray:
    """fp32 x >= 0 -> the 16-bit value TOWARD ZERO as fp32: v_cvt_pkrtz_f16_f32 (subnormals kept) / the upper half of the fp32 word."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == torch.bfloat16:
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    h = x.astype(np.float16)
    h = np.where(h.astype(np.float32) > x, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


# One injected bug each, for the teeth tests of tests/test_attention_grid_cpu.py; attn_fault_applies tells where it changes
# the arithmetic at all (elsewhere the faulted restatement is bit-identical to the unfaulted one, which the test asserts too).
ATTN_FAULTS = {
    "pad_last_key": "the last valid key is treated as a pad",
    "unmask_first_pad": "the first pad key is unmasked (operands laid out for nkv + 1 keys: zero K row, zero V column)",
    "skip_last_tile": "the last key tile is skipped",
    "stale_stage": "the last tile j is read from the ring stage of tile j - 3",
    "v_of_previous_tile": "V(j) is paired with K(j + 1)",
    "no_rescale": "O is not rescaled when the running max rises",
    "no_quad_order": "the V^T quad order {0, 2, 1, 3} is not applied",
    "row_from_32_above": "query rows 32 .. 63 are computed from the rows 32 above them",
    "denominator_before_mask": "overwrite path: the denominator is summed before the scores past nkv are overwritten",
}


def attn_fault_applies(fault, nq, nkv, same_p) -> bool:
    nt = (nkv + 63) // 64
    return {"pad_last_key": True, "unmask_first_pad": nkv % 64 != 0, "skip_last_tile": True, "stale_stage": nt >= 4,
            "v_of_previous_tile": nt >= 2, "no_rescale": nt >= 2, "no_quad_order": nkv > 4,
            "row_from_32_above": nq > 32 and nkv > 1, "denominator_before_mask": not same_p and nkv % 64 != 0}[fault]


def attn16_restate(q, k, v, scale, dtype, same_p, fault=None):
    """numpy restatement of the algorithm attn_kernel / attn64_kernel document (the comment block above attn_bound, the header of
    csrc/attention.hip): q [G, Mq, dh], k, v [G, nkv, dh] holding 16-bit values (G = batch x heads) -> [G, Mq, dh] float64 of 16-bit
    values.  64-key tiles; a running max that is raised - O rescaled - only when some row of a 32-row wave has a tile max more
    than 2^8 above it; fp32 O and row sum, one reciprocal, one final rounding.
      same_p (dh = 72): Q pre-scaled by c = scale log2(e) and rounded to 16 bits; the max is subtracted as two 16-bit halves inside
        the score sum; P = exp2(score) packed toward zero and used for BOTH sums (the all-ones row of V^T, valid keys only); the
        pad keys carry -30000 in the mask column of K.  m_run starts at 0 and the first tile always rescales.
      else (dh = 64 / 32, and attn64_kernel = the one-tile case): raw fp32 scores, those past nkv overwritten with -1e30;
        P = exp2(s c - m c), rounded to nearest for the numerator, summed unrounded for the denominator.
    Not bit-faithful (numpy's matmul stands for the MFMA chains, float64 for the short sum of score terms).  fault: a key of ATTN_FAULTS."""
    f4 = np.float32
    q, k, v = (np.ascontiguousarray(t, dtype=f4) for t in (q, k, v))
    G, Mq, dh = q.shape
    nkv = k.shape[1]
    c = f4(f4(scale) * f4(1.4426950408889634))
    nt = (nkv + 63) // 64
    if fault == "row_from_32_above":
        q = q.copy()
        q[:, 32:64] = q[:, :max(min(Mq, 64) - 32, 0)]
    valid = nkv - 1 if fault == "pad_last_key" else nkv + 1 if fault == "unmask_first_pad" and nkv % 64 else nkv
    Kp, Vp = np.zeros((G, 64 * nt, dh), f4), np.zeros((G, 64 * nt, dh), f4)
    Kp[:, :nkv], Vp[:, :nkv] = k, v
    key = np.arange(64 * nt)
    ones = (key < valid).astype(f4)                                            # row dh of V^T
    maskcol = np.where(key < valid, 0.0, round16(-30000.0, dtype)).astype(f4)  # column dh of K (against Q's 1)
    if fault == "no_quad_order":
        quad = (key >> 2) & 3
        Vp = Vp[:, (key & ~15) | ((((quad & 1) << 1) | (quad >> 1)) << 2) | (key & 3)]

    def wave_any(t):                                                           # __all / __any over the 32 rows of a wave
        a = np.pad(t, ((0, 0), (0, (-Mq) % 32))).reshape(G, -1, 32).any(-1)
        return np.repeat(a, 32, axis=1)[:, :Mq]

    O, l = np.zeros((G, Mq, dh), f4), np.zeros((G, Mq), f4)
    if same_p:
        qs = round16(q * c, dtype).astype(f4)
        m_run, mh, ml = np.zeros((G, Mq), f4), np.zeros((G, Mq)), np.zeros((G, Mq))   # mh, ml: -m_hi, -m_lo as Q carries them
    else:
        m_run = np.full((G, Mq), -1e30, f4)
    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        for t in range(nt - 1 if fault == "skip_last_tile" else nt):
            kt = t - 3 if fault == "stale_stage" and t == nt - 1 and t >= 3 else t
            vt = max(t - 1, 0) if fault == "v_of_previous_tile" else kt
            Kt, Vt = Kp[:, 64 * kt:64 * kt + 64], Vp[:, 64 * vt:64 * vt + 64]
            if same_p:
                s = (np.matmul(qs.astype(np.float64), Kt.transpose(0, 2, 1).astype(np.float64)) + maskcol[64 * kt:64 * kt + 64]
                     + mh[..., None] + ml[..., None]).astype(f4)
                mx = s.max(-1)
                trig = np.ones_like(mx, bool) if t == 0 else wave_any(mx > 8.0)
                delta = np.where(trig, mx if t == 0 else np.maximum(mx, 0), 0).astype(f4)
                alpha = np.exp2(-delta)
                if fault != "no_rescale":
                    O, l = O * alpha[..., None], l * alpha
                m_run = m_run + delta
                mh = round16(-m_run, dtype)
                ml = round16(-m_run.astype(np.float64) - mh, dtype)
                P = trunc16(np.exp2(s - delta[..., None]), dtype)
                l = l + np.matmul(P, ones[64 * vt:64 * vt + 64])
                O = O + np.matmul(P, Vt)
            else:
                raw = np.matmul(q, Kt.transpose(0, 2, 1))
                s = np.where(key[64 * t:64 * t + 64] >= valid, f4(-1e30), raw)
                mx = s.max(-1)
                trig = wave_any((mx - m_run) * c > 8.0)
                m_new = np.where(trig, np.maximum(m_run, mx), m_run)
                alpha = np.exp2((m_run - m_new) * c)
                l = l * alpha
                if fault != "no_rescale":
                    O = O * alpha[..., None]
                m_run = m_new
                mc = (m_run * c)[..., None]
                P = np.exp2(s * c - mc)
                l = l + (np.exp2(raw * c - mc) if fault == "denominator_before_mask" else P).sum(-1, dtype=f4)
                O = O + np.matmul(round16(P, dtype).astype(f4), Vt)
        out = O * (f4(1.0) / l)[..., None]
    return round16(out, dtype)


# ------------------------------------------------------------------------------------------------ the fp32 entry points
# csrc/fp32.hip (gemm_f32, attention_f32, layernorm_modulate_f32, silu_f32) and the fp32 front end of csrc/rowops.hip (linear_f32,
# timestep_embedding, point_features, vit_tokens, row_stats) take fp32 and give fp32: nothing is rounded to 16 bits, so the contract
# is "the float64 value, within what fp32 arithmetic in the documented order can lose".  Every helper below returns (exact, bound)
# as float64 torch tensors on the device of its inputs (the shipped shapes are too large for the CPU inside a test); `bound` is a
# worst-case bound per element from the standard model fl(a op b) = (a op b)(1 + d), |d| <= u = 2^-24, gamma_n = n u / (1 - n u)
# for n accumulated roundings in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, ch. 3), and the accuracy of
# the device math functions in ulps.  No constant in them is measured.  They are asserted without a slack factor
# (check_bound).  tests/test_fp32_contract_cpu.py proves on the CPU that numpy-fp32 restatements of the kernels' loops stay
# inside them, and that the same restatements with one fault injected do not.
#
# Device math functions (ulps of the fp32 result).  The device library is built to the OpenCL C full-profile limits (OpenCL C
# specification, "Relative error as ULPs": exp <= 3, tanh <= 5, erf <= 16, rsqrt <= 2); sinf / cosf are held to the 2 ulp this
# project has promised for them since tests/test_hip_rowops.py::test_timestep_embedding_and_mlp (the specification's limit is 4).
# v_exp_f32, the hardware exp2 behind __expf, is 1 ulp (CDNA3 / CDNA4 ISA guide).  Division and sqrtf are correctly rounded (hipcc's default
# -fhip-fp32-correctly-rounded-divide-sqrt; the build sets no fast-math flag).
EXP_ULPS, TANH_ULPS, ERF_ULPS, RSQRT_ULPS, SINCOS_ULPS = 3.0, 5.0, 16.0, 2.0, 2.0
GELU_ERF_LIPSCHITZ = 1.13  # max |d/dy (y Phi(y))| = Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 1.129 (at y = sqrt 2)
SILU_LIPSCHITZ = 1.10      # max |d/dy silu(y)| = 1.0998 (at y = 2.4)
FLT_MAX = float.fromhex("0x1.fffffep127")


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def _t64(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x.detach().double()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 at |x| (float64 tensor; the subnormal spacing 2^-149 below the normal range)."""
    _, e = torch.frexp(torch.where(x == 0, torch.ones_like(x), x.abs()))        # |x| = m 2^e, m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, -200), e)
    return torch.ldexp(torch.ones_like(x), torch.clamp(e - 24, min=-149))


def act64_t(y: torch.Tensor, act) -> torch.Tensor:
    """0 identity, 1 tanh-GELU, 2 erf-GELU, "silu" (float64 torch)."""
    if act == 1:
        return 0.5 * y * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))
    if act == 2:
        return 0.5 * y * (1.0 + torch.special.erf(y / math.sqrt(2.0)))
    if act == "silu":
        return y * torch.sigmoid(y)
    return y


def act_eval_err(ya: torch.Tensor, act) -> torch.Tensor:
    """Bound of the fp32 EVALUATION error of the activation at an argument of magnitude <= ya (non-decreasing in ya, so that it
    can be taken at |y| + the argument's own bound).
      tanh-GELU (gelu_tanh_exact, fp32.hip): z = c (x + 0.044715 x^3) carries 7 u |z| (the two rounded constants, four products,
        one sum; |0.044715 x^3| <= |x + 0.044715 x^3|); T = tanhf(z): 7 u |z| (1 - T^2) + TANH_ULPS 2 u |T|, and |z| (1 - tanh^2 z)
        <= 0.448; 1 + T one rounding of a value <= 2; 0.5 x is exact; the last product one rounding of |gelu| <= |x|:
        0.5 |x| (7 (0.448) + 2 TANH_ULPS + 2) u + u |x| = (3.6 + TANH_ULPS) u |x|.  The error is ABSOLUTE in |x|: below y = -3 the sum
        1 + T cancels and the result holds only a few of its own bits.
      erf-GELU (gelu_erf_f): w = x / sqrt 2 carries 2 u |w|, through erf' = 2 / sqrt pi exp(-w^2): 2 u (0.484); erff ERF_ULPS 2 u;
        1 + E and the product as above: 0.5 |x| (0.97 + 2 ERF_ULPS + 2) u + u |x| = (2.5 + ERF_ULPS) u |x|.
      SiLU of primx_linear_f32 (silu_f, common.h: x / (1 + __expf(-x)), __expf(a) = v_exp_f32(a log2 e)): the rounded constant and
        the product move the exp2 argument by 2 u |x| log2 e, the result by a relative 2 u |x|; v_exp_f32 2 u; so e = exp(-x) carries
        (2 |x| + 2) u, the quotient |silu| (1 - sigma) (2 |x| + 2) u + 2 u |silu| (the sum and the division).  With x^2 sigma
        (1 - sigma) <= 0.44 and |x| sigma (1 - sigma) <= 0.224: <= (1.4 + 2 |x|) u."""
    if act == 1:
        return (3.6 + TANH_ULPS) * U32 * ya
    if act == 2:
        return (2.5 + ERF_ULPS) * U32 * ya
    if act == "silu":
        return (1.4 + 2.0 * ya) * U32
    return torch.zeros_like(ya)


def gemm_f32_ref(A, W, bias=None, act=0, out_scale=1.0, gate_rows=None, x0=None):
    """primx_gemm_f32 / primx_linear_f32 -> (exact, bound).

    y = A W^T + bias is a chain of K fused multiply-adds and one addition in fp32: |y_f - y| <= gamma_(K+1) (sum |a||w| + |b|)
    (gemm_abs_bound; any order, so it holds for the MFMA chain, the fmaf tiles and the wave-per-column kernel alike).
      out = act(y) out_scale:  L |y_f - y| (L = the activation's Lipschitz constant) + act_eval_err(|y| + that bound), times
                               |out_scale|, plus one rounding u |out| of the product;
      gated, out = x0 + g y:   fl(x0 + fl(g y_f)) = two roundings (one if contracted): |g| gamma (1 + 2 u) + u (|x0| + 2 |g y|).
    act: 0, 1 (tanh-GELU), 2 (erf-GELU) or "silu" (primx_linear_f32's act_out = 1).  gate_rows: the gate of each row [M, N]."""
    Ad, Wd = _t64(A), _t64(W)
    y = Ad @ Wd.t()
    s = Ad.abs() @ Wd.abs().t()
    if bias is not None:
        y = y + _t64(bias)[None, :]
        s = s + _t64(bias).abs()[None, :]
    bnd = gamma(Ad.shape[1] + 1) * s
    if gate_rows is not None:
        g, x = _t64(gate_rows), _t64(x0)
        return x + g * y, g.abs() * bnd * (1 + 2.0 ** -22) + 1.01 * U32 * (x.abs() + 2.0 * (g * y).abs())
    L = {0: 1.0, 1: GELU_LIPSCHITZ, 2: GELU_ERF_LIPSCHITZ, "silu": SILU_LIPSCHITZ}[act]
    E = L * bnd + act_eval_err(y.abs() + bnd, act)
    sc = f32(out_scale)
    out = sc * act64_t(y, act)
    if sc != 1.0:
        E = abs(sc) * E
        E = E + U32 * (out.abs() + E)
    return out, E


def attn_f32_bound(q, k, v, scale, chunk=128):
    """primx_attention_f32 -> (exact [B, Mq, H, dh], bound), float64 on q's device; q may hold a subset of the query rows.

    attn_f32_kernel (fp32.hip): s_j = scale (q . k_j) by a chain of dh fused multiply-adds and one product; per 32-key tile the
    running max m, p_j = __expf(s_j - m), the row sum l and O rescaled by alpha = __expf(m_old - m) and accumulated by fused
    multiply-adds; out = O (1 / l).  No operand is rounded and the SAME p_j enters numerator and denominator, so with w_j the
    softmax weights and relative errors eta_j of p_j the output moves by sum_j w_j eta_j (v_j - out): a common factor (every alpha,
    the choice of m) cancels.  Natural-exp units, u = 2^-24:
        ds_j  = (dh + 4) u sum_d |q_d k_jd| scale + 2 u max_j |s_j|     (the chain, the scale; slack for the max)
        eta_j = ds_j + 4 u |s_j - m| + 4 u      (the subtraction u |s_j - m|; __expf's rounded log2 e and its product with the
                                                 argument 2 u |s_j - m|; v_exp_f32 at 1 ulp = 2 u; one u of slack in each)
        E     = sum_j w_j eta_j |v_j - out| + gamma_(nkv + tiles + 4) (sum_j w_j |v_j| + |out|) + 4 u |out|
    (accumulation of O and of l over nkv keys and `tiles` rescales; the reciprocal and the last product)."""
    B, Mq, H, dh = q.shape
    nkv = k.shape[1]
    sc = f32(scale)
    gam = gamma(nkv + (nkv + 31) // 32 + 4)
    outs = torch.empty(B, Mq, H, dh, dtype=torch.float64, device=q.device)
    bounds = torch.empty_like(outs)
    for b in range(B):
        for h in range(H):
            K, V = k[b, :, h].double(), v[b, :, h].double()
            Ka, Va = K.abs(), V.abs()
            for r0 in range(0, Mq, chunk):
                Q = q[b, r0:r0 + chunk, h].double()
                S = (Q @ K.t()) * sc
                m = S.max(1, keepdim=True).values
                P = torch.exp(S - m)
                w = P / P.sum(1, keepdim=True)
                out = w @ V
                ds = (dh + 4) * U32 * ((Q.abs() @ Ka.t()) * abs(sc)) + 2.0 * U32 * S.abs().max(1, keepdim=True).values
                eta = ds + 4.0 * U32 * (S - m).abs() + 4.0 * U32
                D = (V[None] - out[:, None]).abs()                             # [chunk, nkv, dh]
                E = torch.einsum("qj,qjd->qd", w * eta, D) + gam * (w @ Va + out.abs()) + 4.0 * U32 * out.abs()
                outs[b, r0:r0 + chunk, h], bounds[b, r0:r0 + chunk, h] = out, E
                del D
    return outs, bounds


def attn_f32_restate(q, k, v, scale, fault=None, fault_tile=-1):
    """numpy-fp32 restatement of attn_f32_kernel's loop: q [G, Mq, dh], k, v [G, Nk, dh] (G = batch x heads) -> [G, Mq, dh] fp32.
    32-key tiles, online max, fp32 exp, O and l rescaled per tile and O accumulated key by key in the kernel's order, one reciprocal.
    (numpy's matmul stands for the short q . k chains.)
    fault: None, or one injected bug for the teeth tests - "drop_last_key" (the last key of a ragged tile is masked),
    "tail_zero" (the masked tail of a ragged tile scores 0 instead of -inf), "skip_rescale" (O is not rescaled in tile
    `fault_tile`), "copy_row" (query row Mq - 1 lands in row Mq - 2 too)."""
    q, k, v = (np.ascontiguousarray(t, dtype=np.float32) for t in (q, k, v))
    G, Mq, dh = q.shape
    Nk = k.shape[1]
    sc = np.float32(scale)
    m = np.full((G, Mq), -np.inf, np.float32)
    l = np.zeros((G, Mq), np.float32)
    O = np.zeros((G, Mq, dh), np.float32)
    ntiles = (Nk + 31) // 32
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(ntiles):
            k0, k1 = 32 * t, min(32 * t + 32, Nk)
            ragged_last = k1 == Nk and Nk % 32 != 0
            if fault == "drop_last_key" and ragged_last:
                k1 -= 1
                if k1 == k0:
                    break
            Kt, Vt = k[:, k0:k1], v[:, k0:k1]
            S = np.matmul(q, Kt.transpose(0, 2, 1)) * sc
            if fault == "tail_zero" and ragged_last:
                pad = 32 - (k1 - k0)
                S = np.concatenate([S, np.zeros((G, Mq, pad), np.float32)], -1)
                Vt = np.concatenate([Vt, np.zeros((G, pad, dh), np.float32)], 1)
            m_new = np.maximum(m, S.max(-1))
            alpha = np.exp(m - m_new)
            P = np.exp(S - m_new[..., None])
            l = l * alpha + P.sum(-1, dtype=np.float32)
            if not (fault == "skip_rescale" and t == fault_tile % ntiles):
                O = O * alpha[..., None]
            for j in range(Vt.shape[1]):                    # key by key, as the kernel's chain of multiply-adds (two roundings here)
                O = O + P[..., j:j + 1] * Vt[:, None, j, :]
            m = m_new
    out = O * (np.float32(1.0) / l)[..., None]
    if fault == "copy_row" and Mq >= 2:
        out[:, Mq - 2] = out[:, Mq - 1]
    return out


def ln_stats_bound(x, eps, n_mean, n_var, rstd_u):
    """Two-pass LayerNorm statistics of fp32 rows in fp32 -> dict(mu, var, rstd, e_mu, rel_r) (float64, [rows, 1]).

    mean_f = fl(sum x / D) with n_mean roundings in any order: e_mu = gamma_(n_mean) mean |x|.  With d = mu - mean_f (one value per
    row) the centred values are c_i^ = (c_i + d)(1 + t_i), |t_i| <= u, c_i = x_i - mu, and because sum_i c_i = 0
        sum_i (c_i + d)^2 / D = var + d^2   EXACTLY  (the first-order term 2 d sum c_i vanishes: a wrong mean costs its square),
    so the computed variance is off by  e_var = e_mu^2 + (2.01 u + gamma_(n_var)) (var + e_mu^2): the roundings t_i, and the n_var
    roundings of the squares, their sum and the division (all terms non-negative, so the sum's error is relative).  Adding eps is
    one more rounding; rstd carries rstd_u (the device function's error, relative, in units of u):
        rel_r = rsqrt_err((e_var + u (var + eps + e_var)) / (var + eps)) + rstd_u u."""
    xd = _t64(x)
    D = xd.shape[-1]
    mu = xd.mean(-1, keepdim=True)
    var = ((xd - mu) ** 2).mean(-1, keepdim=True)
    e_mu = gamma(n_mean) * xd.abs().mean(-1, keepdim=True)
    e_var = e_mu ** 2 + (2.01 * U32 + gamma(n_var)) * (var + e_mu ** 2)
    epsf = f32(eps)
    a = (e_var + U32 * (var + epsf + e_var)) / (var + epsf)
    rel_r = torch.where(a < 1.0, torch.maximum(1.0 / torch.sqrt(torch.clamp(1.0 - a, min=1e-300)) - 1.0, 1.0 - 1.0 / torch.sqrt(1.0 + a)),
                        torch.full_like(a, float("inf"))) + rstd_u * U32
    return dict(mu=mu, var=var, rstd=1.0 / torch.sqrt(var + epsf), e_mu=e_mu, rel_r=rel_r, D=D)


def layernorm_modulate_f32_ref(x, shift_rows, scale_rows, eps=1e-6):
    """primx_layernorm_modulate_f32 -> (exact, bound): (x - mu) rstd (1 + scale) + shift, shift_rows / scale_rows = the
    modulation row of each x row ([rows, D]).

    ln_modulate_f32_kernel: mean = fl(sum / D) (D + 1 roundings with the division's slack), var likewise over the squares
    (n_var = D + 2), rstd = rsqrtf (RSQRT_ULPS ulp = 2 RSQRT_ULPS u).  Then per element c^ = fl(x - mean_f), off by
    e_c = e_mu + u (|c| + e_mu); P = fl(fl(c^ rstd_f) fl(1 + scale)): three roundings; out = fl(P + shift):
        |P_f - P| <= rstd |1 + scale| (e_c + (|c| + e_c) (rel_r + 3 u)),    bound = that + u (|P| + |shift| + that),   x 1.01 for
    the products of small terms."""
    st = ln_stats_bound(x, eps, x.shape[-1] + 1, x.shape[-1] + 2, 2.0 * RSQRT_ULPS)
    xd, sh, sc = _t64(x), _t64(shift_rows), _t64(scale_rows)
    c = xd - st["mu"]
    P = c * st["rstd"] * (1.0 + sc)
    e_c = st["e_mu"] + U32 * (c.abs() + st["e_mu"])
    eP = st["rstd"] * (1.0 + sc).abs() * (e_c + (c.abs() + e_c) * (st["rel_r"] + 3.0 * U32))
    return P + sh, 1.01 * (eP + U32 * (P.abs() + sh.abs() + eP))


def ln_f32_restate(x, shift_rows, scale_rows, eps=1e-6, pad_mean=False):
    """numpy-fp32 restatement of ln_modulate_f32_kernel (two-pass statistics, rsqrt as 1 / sqrt in fp32, the epilogue's operation
    order).  pad_mean: the injected fault "mean over the padded length 64 ceil(D / 64)"."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    D = x.shape[-1]
    n = np.float32(64 * ((D + 63) // 64) if pad_mean else D)
    mean = x.sum(-1, keepdims=True, dtype=np.float32) / n
    c = x - mean
    var = (c * c).sum(-1, keepdims=True, dtype=np.float32) / np.float32(D)
    rstd = np.float32(1.0) / np.sqrt(var + np.float32(eps))
    return c * rstd * (np.float32(1.0) + np.asarray(scale_rows, np.float32)) + np.asarray(shift_rows, np.float32)


def row_stats_ref(x, eps):
    """primx_row_stats -> (exact [rows, 2], bound [rows, 2]) for the pairs (mean, rstd).

    row_stats_kernel (the summation order of ln_row.h: four columns per lane and 128-column step, a 5-step half-wave tree; any
    order is covered): mean = fl(sum fl(1 / D)): D + 2 roundings; var = fl(sum of squares fl(1 / D)): D + 3; rstd = 1 / sqrtf(.):
    both correctly rounded, 2 u.  The pair's bounds: e_mu, and rel_r rstd."""
    D = x.shape[-1]
    st = ln_stats_bound(x, eps, D + 2, D + 3, 2.0)
    return torch.cat([st["mu"], st["rstd"]], -1), torch.cat([st["e_mu"], 1.01 * st["rel_r"] * st["rstd"]], -1)


def sincos_ref(arg32):
    """sinf / cosf of an fp32 argument -> (sin, cos, bound_sin, bound_cos): the float64 sine and cosine OF THE FP32 VALUE and
    SINCOS_ULPS ulps of the fp32 result.  The kernels form the argument as ONE fp32 product (t * freqs, p * freqs), which the
    caller restates exactly; nothing else is rounded."""
    a = _t64(arg32)
    s, c = torch.sin(a), torch.cos(a)
    return s, c, SINCOS_ULPS * ulp32(s), SINCOS_ULPS * ulp32(c)


def silu_f32_ref(x):
    """primx_silu_f32 on FINITE x -> (exact, bound).  x / (1 + expf(-x)): -x is exact; expf carries EXP_ULPS ulp = 2 EXP_ULPS u
    relative, which reaches the quotient through e / (1 + e) = 1 - sigma(x); the sum and the (correctly rounded) division add u
    each:   bound = |silu| u (2 EXP_ULPS (1 - sigma) + 2)  (x 1.01, + one subnormal spacing).
    Below -LN_FLT_MAX expf(-x) is +inf and the result -0 (silu64; torch's fp32 silu does the same).  Where exp(-x) lies within
    expf's error and half an ulp of the largest fp32 value - |x + LN_FLT_MAX| <= (2 EXP_ULPS + 1) u, the relative error of exp being
    the absolute one of x - either side may happen: the bound there adds the finite value's whole magnitude |x| / FLT_MAX."""
    xd = _t64(x)
    sig = torch.sigmoid(xd)
    fin = xd * sig
    over = -xd > LN_FLT_MAX
    exact = torch.where(over, torch.full_like(xd, -0.0), fin)
    bound = 1.01 * exact.abs() * U32 * (2.0 * EXP_ULPS * (1.0 - sig) + 2.0) + 2.0 ** -149
    edge = (-xd - LN_FLT_MAX).abs() <= (2.0 * EXP_ULPS + 1.0) * U32
    bound = torch.where(edge, 1.01 * xd.abs() / FLT_MAX + bound, bound)
    return exact, bound


def check_bound(got, exact, bound, what="") -> float:
    """Every element of `got` finite and within `bound` of `exact` - no slack factor.  Returns max |err| / bound."""
    g = _t64(got).to(exact.device).reshape(exact.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    err = (g - exact).abs()
    bad = err > bound
    ratio = float((err / torch.clamp(bound, min=1e-300)).max()) if err.numel() else 0.0
    if bool(bad.any()):
        idx = [tuple(int(i) for i in r) for r in torch.nonzero(bad)[:8].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements beyond the fp32 bound, worst {ratio:.3g} x, first at {idx}")
    return ratio


def rms_ratio(got, restated, exact) -> float:
    """rms |got - exact| over max(rms |restated - exact|, u rms |exact|): the kernel's error against the numpy-fp32 restatement's
    on the same inputs (the floor keeps a restatement that happens to be exact - one key, K = 4 - from being a zero)."""
    ex = _t64(exact)
    g, r = _t64(got).to(ex.device).reshape(ex.shape), _t64(restated).to(ex.device).reshape(ex.shape)
    rms = lambda t: float(torch.sqrt(torch.mean(t * t))) if t.numel() else 0.0
    floor = max(rms(r - ex), U32 * rms(ex), 1e-300)
    return rms(g - ex) / floor


RMS_MARGIN = 2.0   # NOT measured: a serial MFMA / fmaf chain against BLAS's blocked order, v_exp_f32 against libm


def check_rms(got, restated, exact, what="", margin=RMS_MARGIN) -> float:
    ratio = rms_ratio(got, restated, exact)
    assert ratio <= margin, f"{what}: rms error {ratio:.3g} x the fp32 restatement's (margin {margin})"
    return ratio


def hold_fp32(got, restated, exact, bound, what="", margin=RMS_MARGIN):
    """Both criteria of an fp32 entry point: every element inside the rigorous bound, and the rms error no more than `margin`
    times the restatement's.  Returns (max |err| / bound, rms ratio)."""
    a = check_bound(got, exact, bound, what)
    b = check_rms(got, restated, exact, what, margin)
    return a, b


def timestep_embedding_ref(t, freqs):
    """primx_timestep_embedding -> (exact [B, 2 half], bound): [cos(arg) | sin(arg)], arg = fl(float(t) * freqs) - the ONE fp32
    product of the kernel, restated exactly (an IEEE fp32 product is the same on every machine)."""
    arg = t.to(torch.float32)[:, None] * freqs.to(torch.float32)[None, :]
    s, c, bs, bc = sincos_ref(arg)
    return torch.cat([c, s], -1), torch.cat([bc, bs], -1)


def point_features_ref(x, freqs):
    """primx_point_features -> (exact [T, round_up(6 F + 3, 4)], bound): [sin(p_d f_k) (3 F) | cos (3 F) | p (3) | 0 padding], column
    d F + k, p = x[:, 1:4], arguments one fp32 product.  The pass-through columns and the padding are bit-exact: bound 0."""
    T, F = x.shape[0], freqs.shape[0]
    p = x[:, 1:4].to(torch.float32)
    arg = (p[:, :, None] * freqs.to(torch.float32)[None, None, :]).reshape(T, 3 * F)
    s, c, bs, bc = sincos_ref(arg)
    width = (6 * F + 3 + 3) // 4 * 4
    pad = torch.zeros(T, width - 6 * F - 3, dtype=torch.float64, device=x.device)
    z3 = torch.zeros(T, 3, dtype=torch.float64, device=x.device)
    return torch.cat([s, c, p.double(), pad], -1), torch.cat([bs, bc, z3, pad], -1)


def vit_tokens_ref(patches, cls, pos, reg, pos_shift=1):
    """primx_vit_tokens in torch fp32: [cls + pos[0] | reg | patches + pos[1:]] - one fp32 addition per element, so the kernel is
    held to it bit for bit.  pos_shift = 0: the injected fault pos[i] for pos[1 + i]."""
    B, n, D = patches.shape
    rows = [(cls + pos[0])[None, None].expand(B, 1, D)]
    if reg is not None and reg.shape[0]:
        rows.append(reg[None].expand(B, -1, -1))
    rows.append(patches + pos[pos_shift:pos_shift + n][None])
    return torch.cat(rows, 1)


# inputs of the fp32 contract tests (tests/test_fp32_contract_cpu.py on the CPU, tests/test_hip_fp32_contract.py on the device)
def gemm_inputs(seed, M, N, K, device):
    g = torch.Generator(device=device).manual_seed(seed)
    A = torch.randn(M, K, device=device, generator=g)
    W = torch.randn(N, K, device=device, generator=g) * K ** -0.5
    b = torch.randn(N, device=device, generator=g) * 0.1
    return A, W, b, g


def qkv_inputs(seed, B, Mq, Mk, H, dh, sigma, device):
    """Logits q . k / sqrt(dh) of standard deviation sigma."""
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randn(B, Mq, H, dh, device=device, generator=g) * sigma
    k = torch.randn(B, Mk, H, dh, device=device, generator=g)
    v = torch.randn(B, Mk, H, dh, device=device, generator=g)
    return q, k, v


LN_BANDS = [(3.0, 0.5), (1.0, 20.0), (1e-3, 1.0), (1e3, -1e4)]     # (spread, offset): the mean dwarfs the spread in three of them


def ln_inputs(seed, rows, D, spread, offset, nb, device):
    """x [rows, D] and one wide modulation buffer [nb, 3 D] whose column slices [:, :D] / [:, 2 D:] are shift / scale."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(rows, D, device=device, generator=g) * spread + offset
    mod = torch.randn(nb, 3 * D, device=device, generator=g) * 0.3
    return x, mod


def heads_of(t):
    """[B, M, H, dh] -> [B H, M, dh] numpy fp32 (attn_f32_restate's layout)."""
    B, M, H, dh = t.shape
    return t.detach().permute(0, 2, 1, 3).reshape(B * H, M, dh).cpu().numpy().astype(np.float32)


def unheads(a, B, H):
    """[B H, M, dh] numpy -> [B, M, H, dh] torch."""
    G, M, dh = a.shape
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(B, H, M, dh).permute(0, 2, 1, 3)


def chain_factor(A, W, bias=None, rows=16, cols=256) -> float:
    """How much larger the rms error of a SERIAL fp32 chain of K fused multiply-adds (what gemm_f32_kernel's MFMA chain and
    linear_f32_kernel's fmaf loop are) is than that of the BLAS product the GEMM tests use as their restatement, on a
    rows x cols block of the same operands: >= 1.  BLAS sums K in blocks and several accumulators, so its error grows with the
    block length, the chain's with sqrt(K): emulated on the CPU the ratio is 1.0 at K = 68, 1.4 - 2.4 at K = 768 / 1152 and 3.9 - 4.6
    at 4608 (it depends on the BLAS kernel the shape selects).  The rms criterion of a chain kernel is therefore RMS_MARGIN x this factor: "no worse than twice a correct chain".
    Each step is emulated as fp32(acc + a w) with the product and the sum in float64 (a double rounding happens for about one
    step in 2^29 and moves one element by half an ulp)."""
    a = _t64(A)[:rows].cpu().numpy()
    w = _t64(W)[:cols].cpu().numpy()
    b = _t64(bias)[:cols].cpu().numpy() if bias is not None else np.zeros(w.shape[0])
    exact = a @ w.T + b
    acc = np.zeros(exact.shape, np.float32)
    for k in range(a.shape[1]):
        acc = (acc.astype(np.float64) + a[:, k:k + 1] * w[None, :, k]).astype(np.float32)
    chain = (acc.astype(np.float64) + b).astype(np.float32)
    blas = (torch.from_numpy(a.astype(np.float32)) @ torch.from_numpy(w.astype(np.float32)).t() + torch.from_numpy(b.astype(np.float32))).numpy()
    rms = lambda t: float(np.sqrt(np.mean((t.astype(np.float64) - exact) ** 2)))
    return max(1.0, rms(chain) / max(rms(blas), U32 * float(np.sqrt(np.mean(exact ** 2))), 1e-300))
