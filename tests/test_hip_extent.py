"""The ADDRESS arithmetic of the VAE decoder's kernels, the elementwise kernels and the GEMM dispatch where a 32-bit index
ends: every entry point once on a batch whose largest 16-bit operand passes 2^31 elements (2^32 bytes) by a few primitives
(tests/extent.py: P = floor(2^31 / e) + 9), inside footprint.guarded(0xFF), so that an output tail no store reached is NaN.

  A. every element of the big call equals the same entry point on slices of at most 2048 primitives - bit for bit wherever the
     decoder uses the entry point (test_vae_decode_many_primitives_are_independent already demands that of the whole decoder);
  B. at the probe primitives (0, the one holding byte 2^31, the one holding element 2^31, the last) the contract check of
     tests/test_hip_contract.py for that entry point, against float64, with the arguments of its test_*_contract function.

The GEMM ring guard of csrc/gemm.hip (M K < 2^31 and N K < 2^31 for the 128-byte ring, whose byte offsets are 32-bit) is run
at the last shape below it and the first shape at it, on both sides.  No tolerance is defined here: every bound is imported
from the test of the same entry point.  Each test asserts in arithmetic on its own sizes that it passes 2^31."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth, vae_ref
from tests import contract_ref as cr
from tests import extent as ex
from tests import footprint as fp
from tests import test_hip_contract as tc
from tests.golden.make_golden import SEED, VAE_CFG
from tests.test_hip_fp32 import SILU_F32_TOL
from tests.test_hip_gemm import TOL as GEMM_TOL
from tests.test_hip_rowops import SILU_CAST_TOL
from tests.test_hip_vae import DECODE_EMU_TOL, DECODE_TOL, ROUTES_TOL
from tests.util import max_abs, rel_l2, unpack_rows, unpack_vt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
BOTH = [F16, BF16]
SKIP = 0.5 ** 0.5


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _idx(probes):
    return torch.tensor(probes, device=DEV)


def _b(what, *reps):
    """Print criterion B's margins: the largest of (error in units of the 1-ulp tolerance, elements that differ / allowance,
    |bias| / its limit) over the contract reports of one row."""
    worst = 0.0
    for r in reps:
        worst = max(worst, r["max_ulp"], r["differ"] / r["allowed"], abs(r["bias"]) / cr.BIAS_LIMIT if r["bias_n"] >= 1000 else 0.0)
    print(f"extent B: {what}: largest error / bound {worst:.3f} ({len(reps)} check(s): " +
          "; ".join(f"max_ulp {r['max_ulp']:.3f}, differ {r['differ']} / {r['allowed']:.0f}, bias {r['bias']:+.4f}" for r in reps) + ")")
    return worst


def _hold(run, P, what, gemm_form_dtype=None):
    """Criterion A.  run(lo, hi) = the entry point on primitives [lo, hi).  gemm_form_dtype: a route the decoder only takes
    with PRIMX_CONV_REG=0 - bit identity if the big and the chunked call launch the same GEMM kernel, ROUTES_TOL otherwise.
    Returns (big outputs, "bit identity" or the measured rel-L2)."""
    with fp.guarded(0xFF):
        big = run(0, P)
    tol = None
    if gemm_form_dtype is not None:
        name_big = tc._launched()
        run(0, min(P, ex.CHUNK))
        print(f"extent A: {what}: the big call launched {name_big}, a chunk {tc._launched()}")
        if tc._launched() != name_big:
            tol = ROUTES_TOL[gemm_form_dtype]
    d = ex.assert_chunks_equal(big, run, P, what=what, rel_l2=tol)
    verdict = "bit identity" if tol is None else f"rel-L2 {d:.2e} (different kernels)"
    print(f"extent A: {what}: P = {P}: {verdict}")
    return big, verdict


# ------------------------------------------------------------------------------------------------ GroupNorm
@pytest.mark.parametrize("C,V,groups,silu", [(256, 512, 32, True), (256, 64, 32, True), (32, 512, 32, True), (64, 27, 8, False)])
def test_groupnorm_silu_extent(ops, C, V, groups, silu):
    """The stream kernel (512 x 256), the register kernels (64 x 256, 512 x 32) and the generic kernel (27 x 64, no SiLU)."""
    dtype, e = F16, V * C
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "groupnorm_silu input / output")
    x = ex.randn_slabs((P, V, C), dtype, DEV, C + V, 1.3, 0.2)
    gam, bet = tc._gn_params(C, C)
    big, _ = _hold(lambda lo, hi: ops.groupnorm_silu(x[lo:hi], gam, bet, groups, 1e-5, silu), P, f"groupnorm_silu C={C} V={V}")
    i = _idx(ex.probe_primitives(P, e, 2))
    _b(f"groupnorm_silu C={C} V={V}", tc.check_groupnorm_silu(big[i], x[i], gam, bet, groups, silu, dtype))


# ------------------------------------------------------------------------------------------------ conv_in
@pytest.mark.parametrize("S,Cout", [(4, 256), (8, 32)])
def test_conv_in_extent(ops, S, Cout):
    dtype, e = F16, S ** 3 * Cout
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "conv_in output")
    g = torch.Generator(device=DEV).manual_seed(41 + S)
    z = torch.randn(P, S ** 3, device=DEV, generator=g)
    W = torch.randn(Cout, 27, device=DEV, generator=g) * 0.2
    b = torch.randn(Cout, device=DEV, generator=g) * 0.2
    big, _ = _hold(lambda lo, hi: ops.conv_in(z[lo:hi], 1.7, -0.3, W, b, S, dtype), P, f"conv_in S={S}")
    i = _idx(ex.probe_primitives(P, e, 2))
    _b(f"conv_in S={S}", tc.check_conv_in(big[i], z[i], 1.7, -0.3, W, b, S, dtype))


# ------------------------------------------------------------------------------------------------ conv3d_k3
def _conv3_extent(ops, dtype, Cin, Cout, S, packed, with_res, gn=False):
    V = S ** 3
    e = V * max(Cin, Cout)
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, f"conv3d_k3 {'input' if Cin >= Cout else 'output'}")
    x = ex.randn_slabs((P, V, Cin), dtype, DEV, Cin + S, *((1.4, 0.3) if gn else ()))
    wk, b = tc._conv_w(Cin * Cout, Cout, Cin, dtype)
    res = ex.randn_slabs((P, V, Cout), dtype, DEV, Cout) if with_res else None
    wp = None
    if packed is not None:
        wp = ops.pack_conv3(wk, Cin)
        assert wp is not None and wp.kind == packed and wp.S == S
    gam, bet = tc._gn_params(12, Cin) if gn else (None, None)
    kw = dict(gn=(gam, bet, 1e-5)) if gn else {}
    scale = SKIP if with_res else 1.0

    def run(lo, hi):
        return ops.conv3d_k3(x[lo:hi], wk, b, S, res=res[lo:hi] if with_res else None, res_scale=scale, Wp=wp, **kw)
    what = f"conv3d_k3 {packed or 'implicit GEMM'}{' gn' if gn else ''} {Cin}->{Cout} @{S} {dtype}"
    big, verdict = _hold(run, P, what, gemm_form_dtype=None if packed else dtype)
    i = _idx(ex.probe_primitives(P, e, 2))
    r = res[i] if with_res else None
    if gn:
        _, a16 = cr.groupnorm_silu_ref(x[i], gam, bet, 32, 1e-5, True, dtype)
        acc = cr.conv3d_k3_acc(a16, wk, b, S).reshape(len(i), V, Cout)
        _b(what, tc.check_conv3d_s8c32_gn(big[i], acc, a16, wk, dtype, r, scale, Cout))
    else:
        acc = cr.conv3d_k3_acc(x[i], wk, b, S).reshape(len(i), V, Cout)
        _b(what, tc.check_conv3d_k3(big[i], acc, dtype, 27 * Cin, r, scale, what))
    return verdict


def _needs_packed_kernels():
    import os
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the implicit GEMM: the activation-resident kernels do not run")


@pytest.mark.parametrize("Cin,Cout,S,packed,with_res,gn", [
    (256, 256, 4, "s4", True, False),       # input, res and output pass 2^31 together
    (256, 512, 4, "s4", True, False),       # the output (and res) pass first
    (256, 32, 8, "s8", True, False),        # conv3s8: the input passes
    (32, 32, 8, "s8c32", True, True),       # conv3s8c32 with the GroupNorm inside
    (32, 6, 8, "s8c32", False, False),      # ... the decoder's last convolution
])
def test_conv3d_k3_packed_extent(ops, Cin, Cout, S, packed, with_res, gn):
    _needs_packed_kernels()
    _conv3_extent(ops, F16, Cin, Cout, S, packed, with_res, gn)


def test_conv3d_k3_implicit_gemm_extent(ops):
    """256 -> 32 at 8^3 with Wp=None (8.4 M gathered rows).  Criterion A: the big and the chunked call launched the same
    kernel (gemm_kernel<., 3, 32, 4, 1, 1, 1, 1>), so bit identity applied."""
    verdict = _conv3_extent(ops, F16, 256, 32, 8, None, False)
    if tc._default_dispatch():
        assert verdict == "bit identity", verdict


# ------------------------------------------------------------------------------------------------ upsample and the fused front
def _upsample_operands(dtype, P):
    C = 256
    x = ex.randn_slabs((P, 64, C), dtype, DEV, 31 + C)
    g = torch.Generator(device=DEV).manual_seed(32)
    wt = (torch.randn(8 * C, C, device=DEV, generator=g) * C ** -0.5).to(dtype)
    bu = (torch.randn(C, device=DEV, generator=g) * 0.3).to(dtype)
    return x, wt, bu, g


@pytest.mark.parametrize("dtype", BOTH)
def test_convtranspose_packed_with_statistics_extent(ops, dtype):
    """4^3 x 256 -> 8^3 x 256, weight-stationary kernel with want_stats=True, then group_stats of its partial sums."""
    _needs_packed_kernels()
    e = 512 * 256
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "convtranspose_k2s2 output")
    x, wt, bu, _ = _upsample_operands(dtype, P)
    wp = ops.pack_convt_s4(wt)

    def run(lo, hi):
        out, part = ops.convtranspose_k2s2(x[lo:hi], wt, bu, 4, Wp=wp, want_stats=True)
        return out, part, ops.group_stats(part, bu, 1e-5)
    (out, part, st), _ = _hold(run, P, f"convtranspose_k2s2 packed {dtype}")
    assert bool(torch.isfinite(st).all())
    i = _idx(ex.probe_primitives(P, e, 2))
    _b(f"convtranspose_k2s2 packed {dtype}",
       tc.check_convtranspose_k2s2(out[i], cr.convtranspose_k2s2_acc(x[i], wt, bu, 4), dtype, 256, "convtranspose_k2s2 packed"))


def test_convtranspose_gemm_form_extent(ops):
    """The same upsample without Wp (1.05 M rows x N = 2048).  Criterion A: the big and the chunked call launched the same
    kernel (gemm_kernel<., 4, 32, 2, 2, 2, 2, 0>), so bit identity applied."""
    dtype, e = F16, 512 * 256
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "convtranspose_k2s2 output")
    x, wt, bu, _ = _upsample_operands(dtype, P)
    out, verdict = _hold(lambda lo, hi: ops.convtranspose_k2s2(x[lo:hi], wt, bu, 4), P, "convtranspose_k2s2 GEMM form", gemm_form_dtype=dtype)
    if tc._default_dispatch():
        assert verdict == "bit identity", verdict
    i = _idx(ex.probe_primitives(P, e, 2))
    _b("convtranspose_k2s2 GEMM form",
       tc.check_convtranspose_k2s2(out[i], cr.convtranspose_k2s2_acc(x[i], wt, bu, 4), dtype, 256, "convtranspose_k2s2 GEMM form"))


@pytest.mark.parametrize("dtype", BOTH)
def test_conv3d_s8_fused_extent(ops, dtype):
    """The upsample output (8^3 x 256, passes 2^31) and its partial statistics -> conv1 + the 1x1 shortcut in one kernel."""
    _needs_packed_kernels()
    e, C = 512 * 256, 256
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "conv3d_s8_fused input")
    x, wt, bu, g = _upsample_operands(dtype, P)
    gam, bet = tc._gn_params(23, C)
    wk, b1 = tc._conv_w(24, 32, C, dtype)
    wsc = (torch.randn(32, C, device=DEV, generator=g) * C ** -0.5).to(dtype)
    bsc = (torch.randn(32, device=DEV, generator=g) * 0.2).to(dtype)
    h8, part = ops.convtranspose_k2s2(x, wt, bu, 4, Wp=ops.pack_convt_s4(wt), want_stats=True)
    del x
    wp = ops.pack_conv3(wk, C, Wsc=wsc)
    (t, sc), _ = _hold(lambda lo, hi: ops.conv3d_s8_fused(h8[lo:hi], wp, b1, part[lo:hi], bu, gam, bet, 1e-5, bsc), P,
                       f"conv3d_s8_fused {dtype}")
    i = _idx(ex.probe_primitives(P, e, 2))
    _b(f"conv3d_s8_fused {dtype}", *tc.check_conv3d_s8_fused(t[i], sc[i], h8[i], gam, bet, wk, b1, wsc, bsc, dtype))


# ------------------------------------------------------------------------------------------------ the decoder's GEMMs and attention
@pytest.mark.parametrize("V,N,with_res", [(512, 32, False), (64, 256, True)])
def test_linear_residual_extent(ops, V, N, with_res):
    """The 1x1 shortcut of the 256 -> 32 block (M = P * 512 rows, no res) and the attention output projection (M = P * 64,
    N = 256, res = the block's input, skip scale)."""
    dtype, K = F16, 256
    e = V * K
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "linear_residual A")
    A = ex.randn_slabs((P, V, K), dtype, DEV, V + N)
    _, W, b = tc._operands(V + N, 8, N, K, dtype)
    res = ex.randn_slabs((P, V, N), dtype, DEV, N) if with_res else None
    scale = SKIP if with_res else 1.0

    def run(lo, hi):
        r = res[lo:hi].view(-1, N) if with_res else None
        return ops.linear_residual(A[lo:hi].view(-1, K), W, b, r, scale).view(hi - lo, V, N)
    big, _ = _hold(run, P, f"linear_residual M = P x {V}, N = {N}")
    i = _idx(ex.probe_primitives(P, e, 2))
    M = len(i) * V
    acc = tc._acc(A[i].view(M, K), W, b)
    _b(f"linear_residual V={V} N={N}", tc.check_linear_residual(big[i].view(M, N), acc, dtype, K, M, res[i].view(M, N) if with_res else None,
                                                                scale, f"linear_residual extent V={V} N={N}"))


def test_linear_heads_and_attention64_extent(ops):
    """The mid-block attention as vae.py runs it: q, k, V^T projection into the compact 64-token operand buffers (Q and V^T
    pass 2^31 elements, as does the A operand), then the one-wave-per-problem attention kernel."""
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    dtype, V, H, dh, C = F16, 64, 8, 32, 256
    e = V * C
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "linear_heads A")
    ex.reaches(P * H * V * dh, 2, "Q / V^T operand of attention")
    t = ex.randn_slabs((P, V, C), dtype, DEV, 77)
    _, W, _ = tc._operands(78, 8, 3 * C, C, dtype)
    kinds = [HEADS_ROWS, HEADS_KROWS, HEADS_VT]

    def run(lo, hi):
        n = hi - lo
        Q = ops.alloc_heads(n, H, V, dh, HEADS_ROWS, dtype, DEV, 64, "q")
        Kp = ops.alloc_heads(n, H, V, dh, HEADS_KROWS, dtype, DEV, 64, "k")
        Vt = ops.alloc_heads(n, H, V, dh, HEADS_VT, dtype, DEV, 64)
        ops.linear_heads(t[lo:hi].view(n * V, C), W, None, V, H, dh, kinds, [Q, Kp, Vt], Q.shape[2])
        return Q, Kp, Vt, ops.attention(Q, Kp, Vt, V, V, dh, dh ** -0.5)
    (Q, Kp, Vt, att), _ = _hold(run, P, "linear_heads + attention (64 tokens)")
    assert Q.shape[2] == 64 and Kp.shape[2] == 64                             # the compact form attn64_kernel takes
    i = _idx(ex.probe_primitives(P, e, 2))
    n = len(i)
    a5 = tc._acc(t[i].view(n * V, C), W).reshape(n, V, 3, H, dh)
    q, k, v = unpack_rows(Q[i], V, dh), unpack_rows(Kp[i], V, dh), unpack_vt(Vt[i], V, dh)
    _b("linear_heads (q, k, V^T)", *[tc.check_heads_segment(got, a5[:, :, s_], dtype, C, s_ == 0, 1.0, f"linear_heads extent segment {s_}")
                                     for s_, got in enumerate((q, k, v))])
    cr.attn_check(att[i].view(n, V, H, dh), q.contiguous(), k.contiguous(), v.contiguous(), dh ** -0.5, dtype, False, "attn64 extent")


# ------------------------------------------------------------------------------------------------ elementwise kernels
SLAB = 1 << 26


def _slabs(n):
    return [(lo, min(n, lo + SLAB)) for lo in range(0, n, SLAB)]


def test_vae_output_extent(ops):
    """[P, 512, 6] 16-bit -> [P, 6, 512] fp32, denormalize on and off: bit-exact on every element against the expression of
    test_conv_in_convtranspose_and_output (vae_ref.denormalise_decoded), slab by slab on the device."""
    dtype, e = F16, 512 * 6
    P = ex.primitives_past(e)
    ex.reaches(P * e, 2, "vae_output input")
    x = ex.randn_slabs((P, 512, 6), dtype, DEV, 91)
    # vae_ref.denormalise_decoded (channel 0 / 5, the others (v + 1) / 2) in float64 with tensor operands, rounded once to fp32.
    # (torch's own `fp32 tensor / 5.0` on the device multiplies by the rounded reciprocal and is not the CPU expression the
    # existing test compares with.  The float64 route rounds exactly as one fp32 division does: v + 1 and (v + 1) / 2 are exact
    # in float64, and k / 5 has the binary period 0011, so it never lies within 2^-29 ulp of an fp32 rounding boundary.)
    add = torch.tensor([0.0, 1, 1, 1, 1, 1], dtype=torch.float64, device=DEV).view(1, 6, 1)
    div = torch.tensor([5.0, 2, 2, 2, 2, 2], dtype=torch.float64, device=DEV).view(1, 6, 1)
    for denorm in (True, False):
        big, _ = _hold(lambda lo, hi: ops.vae_output(x[lo:hi], denorm), P, f"vae_output denormalize={denorm}")
        step = SLAB // e
        for lo in range(0, P, step):
            ref = x[lo:lo + step].double().permute(0, 2, 1)
            if denorm:
                ref = (ref + add) / div
            assert torch.equal(big[lo:lo + step], ref.float()), (denorm, lo)
        del big


def test_cast_silu_cfg_extent(ops):
    """cast16, silu_cast, silu_f32 on n = 2^31 + 257 fp32 values and cfg_combine on 2 x n 16-bit values: each slice of 2^26
    elements again on its own (criterion A) and against the torch expression of tests/test_hip_rowops.py / test_hip_fp32.py
    (cast16 and cfg_combine bit-exact).

    The values are those tests' 2 N(0, 1), clamped to |x| <= 3.9.  Their absolute bounds on silu were stated for a few
    thousand such values, of which hardly any passes 4; among 2^31 of them some reach 12.  silu_cast and torch's
    F.silu(x).to(dtype) each round a slightly different fp32 value once and may legitimately land on the two 16-bit
    neighbours of a rounding boundary: one ulp16, which is 2^-9 = 1.95e-3 <= SILU_CAST_TOL below 4 and 3.9e-3 from 4 on.  So
    the bound is a statement about one ulp exactly while |silu(x)| < 4, and the clamp keeps it that (likewise 1e-6 for the
    fp32 form: four fp32 ulps below 4).  What is under test here is where the kernels read and write, not their value range."""
    dtype = F16
    n = ex.E + 257
    ex.reaches(n, 4, "elementwise input")
    x = ex.randn_slabs((n,), torch.float32, DEV, 4, 2.0, slab_bytes=4 * SLAB).clamp_(-3.9, 3.9)

    def hold(name, op, check):
        with fp.guarded(0xFF):
            big = op(x)
        for lo, hi in _slabs(n):
            part = big[lo:hi]
            assert torch.equal(ex.bits(part), ex.bits(op(x[lo:hi]))), (name, lo)
            check(part, x[lo:hi], lo)
    hold("cast16", lambda t: ops.cast16(t, dtype), lambda got, xs, lo: _eq(got, xs.to(dtype), ("cast16", lo)))
    hold("silu_cast", lambda t: ops.silu_cast(t, dtype),
         lambda got, xs, lo: _le(float((got.float() - F.silu(xs).to(dtype).float()).abs().max()), SILU_CAST_TOL[dtype], ("silu_cast", lo)))
    hold("silu_f32", ops.silu_f32,
         lambda got, xs, lo: _lt(float((got.double() - F.silu(xs.double())).abs().max()), SILU_F32_TOL, ("silu_f32", lo)))
    del x
    mo = ex.randn_slabs((2, n), dtype, DEV, 5, slab_bytes=8 * SLAB)
    ex.reaches(n, 2, "cfg_combine half")
    with fp.guarded(0xFF):
        big = ops.cfg_combine(mo.view(2, n, 1), 6.0).view(1, n)       # (rows of one element: the guard is 256 rows per side)
    for lo, hi in _slabs(n):
        cond, unc = mo[0, lo:hi], mo[1, lo:hi]
        assert torch.equal(ex.bits(big[0, lo:hi]), ex.bits(ops.cfg_combine(torch.stack([cond, unc]), 6.0)[0])), ("cfg_combine", lo)
        _eq(big[0, lo:hi], unc + 6.0 * (cond - unc), ("cfg_combine", lo))           # torch 16-bit arithmetic rounds after every op


def _eq(a, b, what):
    assert torch.equal(a, b), what


def _le(v, tol, what):
    assert v <= tol, (what, v)


def _lt(v, tol, what):
    assert v < tol, (what, v)


def test_latent_denorm_extent(ops):
    """rows x 68 fp32 with rows * 68 > 2^31: x / nf * std + mean split into srt [rows, 4] and z [rows, 64], bit-exact (the
    expression of test_latents_to_primitives_pipeline)."""
    C = 68
    rows = ex.E // C + 9
    ex.reaches(rows * C, 4, "latent_denorm input")
    x = ex.randn_slabs((rows, C), torch.float32, DEV, 41)
    g = torch.Generator(device=DEV).manual_seed(42)
    mean = torch.randn(C, device=DEV, generator=g) * 0.5
    std = (torch.randn(C, device=DEV, generator=g) * 0.2 + 1.0).abs()
    with fp.guarded(0xFF):
        srt, z = ops.latent_denorm(x, mean, std, 1.0, 4)
    step = 1 << 20
    for lo in range(0, rows, step):
        xs = x[lo:lo + step]
        s2, z2 = ops.latent_denorm(xs, mean, std, 1.0, 4)
        assert torch.equal(ex.bits(srt[lo:lo + step]), ex.bits(s2)) and torch.equal(ex.bits(z[lo:lo + step]), ex.bits(z2)), lo
        ref = xs / 1.0 * std + mean
        assert torch.equal(srt[lo:lo + step], ref[:, :4]) and torch.equal(z[lo:lo + step], ref[:, 4:]), lo


# ------------------------------------------------------------------------------------------------ the decoder
@pytest.fixture(scope="module")
def vae(ops):
    import topia_xl_amd as pkg
    m = pkg.VAE(**VAE_CFG).eval()
    sd = synth.state_dict_like(SEED, m.state_dict())
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    return m, sd


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("P", [16384, 16393])
def test_vae_decode_extent(vae, dtype, P):
    """VAE.decode on the shipped chunk of pipeline.latents_to_primitives (8 x 2048 primitives: the [P, 512, 256] activation
    is exactly 2^31 elements, 2^32 bytes) and 9 primitives past it, against 8 (9) decodes of at most 2048 primitives, and at
    the probe primitives against oracle.vae_ref.vae_decode with the tolerances of test_vae_decode_against_reference."""
    m, sd = vae
    m.compute_dtype = dtype
    e = 512 * 256
    if P == 16384:
        assert P * e == ex.E and P * e * 2 == 1 << 32
    else:
        ex.reaches(P * e, 2, "the [P, 512, 256] activation")
    z = ex.randn_slabs((P, 1, 4, 4, 4), torch.float32, DEV, 9)
    try:
        big, _ = _hold(lambda lo, hi: m.decode(z[lo:hi]), P, f"VAE.decode {dtype}")
    finally:
        m.compute_dtype = F16
    assert big.shape == (P, 6, 8, 8, 8) and big.dtype == torch.float32
    i = _idx(ex.probe_primitives(P, e, 2))
    zp, out = z[i].cpu(), big[i].cpu()
    ref = vae_ref.vae_decode(sd, zp, VAE_CFG["up_channels"], VAE_CFG["layers_per_block"])
    rel_max = max_abs(out, ref) / float(ref.abs().max())
    print(f"extent B: VAE.decode {dtype} P = {P}: max-abs / |ref|max {rel_max:.2e} (bound {DECODE_TOL[dtype][0]:g}), rel-L2 "
          f"{rel_l2(out, ref):.2e} (bound {DECODE_TOL[dtype][1]:g})")
    assert rel_max < DECODE_TOL[dtype][0], rel_max
    assert rel_l2(out, ref) < DECODE_TOL[dtype][1], rel_l2(out, ref)
    emu = vae_ref.vae_decode(sd, zp, VAE_CFG["up_channels"], VAE_CFG["layers_per_block"], emulate=dtype)
    assert rel_l2(out, emu) < DECODE_EMU_TOL[dtype], rel_l2(out, emu)


def test_latents_to_primitives_batch_and_seam(vae):
    """An (8, 2048, 68) sample - the batch-8 shape, one decode of 16384 primitives - is bit-identical to eight batch-1 calls;
    on a 12-primitive sample max_prims_per_call=5 (three decodes and the concatenation) is bit-identical to one call."""
    from topia_xl_amd.pipeline import latents_to_primitives
    m, _ = vae
    g = torch.Generator(device=DEV).manual_seed(43)
    mean = (torch.randn(68, device=DEV, generator=g) * 0.5).tolist()
    std = (torch.randn(68, device=DEV, generator=g) * 0.2 + 1.0).abs().tolist()
    s = torch.randn(8, 2048, 68, device=DEV, generator=g)
    with fp.guarded(0xFF):
        full = latents_to_primitives(s, m, mean, std, 1.0)
    assert full.shape == (8, 2048, 4 + 6 * 512) and bool(torch.isfinite(full).all())
    for b in range(8):
        assert torch.equal(latents_to_primitives(s[b:b + 1], m, mean, std, 1.0), full[b:b + 1]), b
    small = s[:1, :12].contiguous()
    one = latents_to_primitives(small, m, mean, std, 1.0)
    assert torch.equal(latents_to_primitives(small, m, mean, std, 1.0, max_prims_per_call=5), one)
    assert torch.equal(one, full[:1, :12])


# ------------------------------------------------------------------------------------------------ the GEMM ring guard
GK = 1152
M_BELOW, M_AT = 1863936, 1864192           # 7281 and 7282 row tiles of 256: M K = 2 147 254 272 < 2^31 <= 2 147 549 184
N_BELOW, N_AT = 1863936, 1864224           # 6472 and 6473 column tiles of 288
ROWS32 = 1 << 15                           # rows per fp32 comparison slab: one wrapped 256-row tile is 12 % of its rel-L2


def _ring(below):
    return 64 if below else 32


def _assert_kernel(dtype, epi, below):
    if tc._default_dispatch():
        want = f"gemm288q_dma_kernel<{1 if dtype == F16 else 2}, {epi}, {_ring(below)}>"
        assert tc._launched() == want, (tc._launched(), want)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("M", [M_BELOW, M_AT])
@pytest.mark.parametrize("op", ["linear", "residual", "gate"])
def test_gemm_ring_guard_m_side(ops, dtype, M, op):
    """N = 288, K = 1152: the last shape of the 128-byte ring (byte offsets of A reach 4 294 508 544) and the first shape of
    the fallback, for the three dense epilogues the public ops reach through launch288q - Linear, linear_residual and the gated
    residual (EPI 0, 3, 1).  The fold epilogues need a producer's partial sums for every row and belong to
    tests/test_hip_fold_contract.py; their guard is the same expression.  check_contract against float64 on the first tile,
    the tile holding byte 2^31 of A, the last full tile and every tile from byte 2^32 - 2 MiB on; all other rows against a
    torch fp32 matmul of the same 16-bit operands, slab by slab, at the rel-L2 of tests/test_hip_gemm.py."""
    N, K = 288, GK
    below = M * K < ex.E
    assert below == (M == M_BELOW) and M % 256 == 0
    if not below:
        ex.reaches(M * K, 2, "A")
    A = ex.randn_slabs((M, K), dtype, DEV, M % 1000)
    _, W, b = tc._operands(11, 8, N, K, dtype)
    probes, rest = ex.tile_blocks(M, 2 * K, 256)
    Wf, bf = W.float(), b.float()
    if op == "linear":
        with fp.guarded(0xFF):
            out = ops.linear(A, W, b)
        _assert_kernel(dtype, 0, below)
        reps = [tc.check_linear(out[lo:hi], tc._acc(A[lo:hi], W, b), dtype, K, hi - lo, 0, 1.0, f"linear M={M} rows {lo}..{hi}")
                for lo, hi in probes]
        ref = lambda lo, hi: A[lo:hi].float() @ Wf.t() + bf
        tol = GEMM_TOL[dtype]
    elif op == "residual":
        res = ex.randn_slabs((M, N), dtype, DEV, 12, 0.3)
        with fp.guarded(0xFF):
            out = ops.linear_residual(A, W, b, res, 0.70710678)
        _assert_kernel(dtype, 3, below)
        reps = [tc.check_linear_residual(out[lo:hi], tc._acc(A[lo:hi], W, b), dtype, K, hi - lo, res[lo:hi], 0.70710678,
                                         f"residual M={M} rows {lo}..{hi}") for lo, hi in probes]
        ref = lambda lo, hi: (A[lo:hi].float() @ Wf.t() + bf + res[lo:hi].float()) * 0.70710678
        tol = GEMM_TOL[dtype]
    else:
        rpb = 2048
        nb = (M + rpb - 1) // rpb
        g = torch.Generator(device=DEV).manual_seed(13)
        gate = (torch.randn(nb, N, device=DEV, generator=g) * 0.5).to(dtype)
        out = torch.zeros(M, N, device=DEV)
        ops.linear_gate_residual(A, W, b, gate, out, rpb)
        _assert_kernel(dtype, 1, below)
        gd = gate.double().cpu().numpy()
        reps = [tc.check_gate_increment(out[lo:hi], tc._acc(A[lo:hi], W, b), gd[np.arange(lo, hi) // rpb], dtype, K, hi - lo,
                                        f"gate M={M} rows {lo}..{hi}") for lo, hi in probes]
        r16 = lambda t: t.to(dtype).float()
        ref = lambda lo, hi: r16(gate[torch.arange(lo, hi, device=DEV) // rpb].float() * r16(A[lo:hi].float() @ Wf.t() + bf))
        tol = 2 * GEMM_TOL[dtype]                          # (test_linear_gate_residual: two roundings)
    _b(f"ring guard {op} M = {M} {dtype}", *reps)
    worst = 0.0
    for lo, hi in rest:
        for a in range(lo, hi, ROWS32):
            z = min(hi, a + ROWS32)
            want = ref(a, z).double()
            d = float((out[a:z].double() - want).norm() / want.norm())
            worst = max(worst, d)
            assert d < tol, (op, M, a, z, d)
    print(f"extent ring guard: {op} M = {M} {dtype}: ring {_ring(below)}, worst slab rel-L2 against fp32 {worst:.2e} (bound {tol:g})")


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("N", [N_BELOW, N_AT])
def test_gemm_ring_guard_n_side(ops, dtype, N):
    """M = 256, K = 1152 with N K on either side of 2^31: W is the operand whose byte offsets reach 2^32."""
    M, K = 256, GK
    below = N * K < ex.E
    assert below == (N == N_BELOW) and N % 288 == 0
    if not below:
        ex.reaches(N * K, 2, "W")
    W = ex.randn_slabs((N, K), dtype, DEV, N % 1000, K ** -0.5)
    A, _, _ = tc._operands(21, M, 8, K, dtype)
    g = torch.Generator(device=DEV).manual_seed(22)
    b = (torch.randn(N, device=DEV, generator=g) * 0.3).to(dtype)
    with fp.guarded(0xFF):
        out = ops.linear(A, W, b)
    _assert_kernel(dtype, 0, below)
    probes, rest = ex.tile_blocks(N, 2 * K, 288)
    _b(f"ring guard linear N = {N} {dtype}", *[tc.check_linear(out[:, lo:hi], tc._acc(A, W[lo:hi], b[lo:hi]), dtype, K, M, 0, 1.0,
                                                               f"linear N={N} columns {lo}..{hi}") for lo, hi in probes])
    Af, worst = A.float(), 0.0
    for lo, hi in rest:
        for a in range(lo, hi, ROWS32):
            z = min(hi, a + ROWS32)
            want = (Af @ W[a:z].float().t() + b[a:z].float()).double()
            d = float((out[:, a:z].double() - want).norm() / want.norm())
            worst = max(worst, d)
            assert d < GEMM_TOL[dtype], (N, a, z, d)
    print(f"extent ring guard: linear N = {N} {dtype}: ring {_ring(below)}, worst slab rel-L2 against fp32 {worst:.2e}")


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("B", [910, 911])
def test_gemm_ring_guard_heads(ops, dtype, B):
    """primx_linear_heads, one HEADS_ROWS destination of 16 heads x 72, 2048 rows per batch entry: M = 910 x 2048 (M K =
    2 146 959 360, the heads ring of kt64_ring) and M = 911 x 2048 (2 149 318 656: the fallback).  The same row blocks against
    float64 (segment 0: scaled after its rounding), every batch entry against a torch fp32 matmul."""
    from topia_xl_amd._lib import HEADS_ROWS
    n, H, dh, K = 2048, 16, 72, GK
    M = B * n
    below = M * K < ex.E
    assert below == (B == 910)
    if not below:
        ex.reaches(M * K, 2, "A")
    A = ex.randn_slabs((M, K), dtype, DEV, B)
    _, W, b = tc._operands(31, 8, H * dh, K, dtype)
    scale0 = dh ** -0.5
    with fp.guarded(0xFF):
        dst = ops.alloc_heads(B, H, n, dh, HEADS_ROWS, dtype, DEV, 256)
        ops.linear_heads(A, W, b, n, H, dh, [HEADS_ROWS], [dst], dst.shape[2], scale0=scale0)
    _assert_kernel(dtype, 2, below)
    got = unpack_rows(dst, n, dh)                                   # [B, n, H, dh] view
    probes, _ = ex.tile_blocks(M, 2 * K, 256)
    reps = []
    for lo, hi in probes:
        for b0 in range(lo // n, (hi - 1) // n + 1):                # a merged run of late tiles can span batch entries
            r0, r1 = max(lo, b0 * n), min(hi, (b0 + 1) * n)
            acc = tc._acc(A[r0:r1], W, b).reshape(1, r1 - r0, H, dh)
            reps.append(tc.check_heads_segment(got[b0:b0 + 1, r0 - b0 * n:r1 - b0 * n], acc, dtype, K, True, scale0,
                                               f"heads B={B} rows {r0}..{r1}"))
    _b(f"ring guard heads B = {B} {dtype}", *reps)
    Wf, bf, worst, step = W.float(), b.float(), 0.0, 16
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        y16 = (A[b0 * n:b1 * n].float() @ Wf.t() + bf).to(dtype)
        want = (scale0 * y16.float()).to(dtype).view(b1 - b0, n, H, dh).double()
        d = float((got[b0:b1].double() - want).norm() / want.norm())
        worst = max(worst, d)
        assert d < 2 * GEMM_TOL[dtype], (B, b0, d)                  # (test_linear_heads_layouts: 2 x TOL behind the q scale)
    assert float(dst[:, :, :, dh:].float().abs().sum()) == 0.0      # the pad columns keep alloc_heads' zeros
    print(f"extent ring guard: heads B = {B} {dtype}: ring {_ring(below)}, worst rel-L2 against fp32 {worst:.2e}")
