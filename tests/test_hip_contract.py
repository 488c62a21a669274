"""The documented rounding contract of every 16-bit entry point (include/primx_hip.h), ulp by ulp: each kernel's output
against tests/contract_ref.py - float64 with round16 at exactly the documented points - through check_contract (within 1
ulp, only near-boundary elements differ, no bias), at shapes that reach every GEMM kernel of the default dispatch and at
values in the fp16 overflow band, the fp16 subnormal range and across many bf16 binades.  fp32-output kernels are held to
a rigorous elementwise bound instead."""
import os
import re
import zlib

import numpy as np
import pytest
import torch

from tests import contract_ref as cr
from tests.util import unpack_rows, unpack_vt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


def _default_dispatch() -> bool:
    """False when a kernel-selection switch is set (tests/test_hip_gemm.py): the arithmetic checks still run, the
    assertions on which kernel ran do not."""
    return not any(os.environ.get(v) for v in ("PRIMX_GEMM_LOADER", "PRIMX_GEMM_NOBIG", "PRIMX_GEMM_BIG_MIN",
                                               "PRIMX_GEMM_BIGHEADS_MIN", "PRIMX_GEMM_NOGEMV", "PRIMX_GEMM_PROF", "PRIMX_LIB",
                                               "PRIMX_LN_FUSE", "PRIMX_LN_FUSE_MAXGRID", "PRIMX_GEMM_KT32", "PRIMX_GEMM_KT64_MIN",
                                               "PRIMX_GEMM_HEADS_KT32"))


def _kernel_family(name: str, dtype) -> str:
    """primx_last_gemm_kernel() -> the key of KERNELS (dtype and epilogue arguments dropped where the table does not
    distinguish them)."""
    m = re.fullmatch(r"(\w+)<([^>]*)>", name)
    assert m, name
    base, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    assert int(args[0]) == (1 if dtype == F16 else 2), name
    if base == "gemv16_kernel":
        return f"gemv16_kernel<.,{args[1]}>"
    if base == "gemm_kernel":
        return f"gemm_kernel<.,{args[1]}," + ",".join(args[2:7]) + ",.>"
    return f"{base}<.," + ",".join(args[1:]) + ">"


# Every (kernel, epilogue) pair the default dispatch of csrc/gemm.hip can choose for primx_linear (EPI 0), _gate_residual[_ln] (1, 5),
# _heads (2) and _residual (3), and the case below that reaches it (epilogue = the second template argument; the fold epilogues
# are in tests/test_hip_fold_contract.py).  A pair added to the dispatch without a row here shows up as an unknown name in test_gemm_contract.
KERNELS = {
    "gemv16_kernel<.,4>": "linear M=3 (few-row GEMV)",
    "gemv16_kernel<.,8>": "linear M=7 (few-row GEMV)",
    "gemm_kernel<.,0,32,4,1,1,1,.>": "linear N=20 (N <= 32)",
    "gemm_kernel<.,3,32,4,1,1,1,.>": "residual N=32 (N <= 32)",
    "gemm_kernel<.,0,32,2,2,2,2,.>": "linear N=136 / K=200 (N % 144 or K % 64)",
    "gemm_kernel<.,1,32,2,2,2,2,.>": "gate-residual N=200",
    "gemm_kernel<.,2,32,2,2,2,2,.>": "heads K=200",
    "gemm_kernel<.,3,32,2,2,2,2,.>": "residual N=100",
    "gemm144l_dma_kernel<.,0>": "linear N=288 (loader waves)",
    "gemm144l_dma_kernel<.,1>": "gate-residual N=288 (loader waves)",
    "gemm144l_dma_kernel<.,2>": "heads, token-major segments only",
    "gemm144l_dma_kernel<.,5>": "gate-residual + LayerNorm tail N=1152",
    "gemm144_dma_kernel<.,2>": "heads with a V^T segment",
    "gemm144_dma_kernel<.,3>": "residual N=288",
    "gemm288q_dma_kernel<.,0,64>": "linear M=4096 N=4608 (256 x 288 tile, 128-byte ring)",
    "gemm288q_dma_kernel<.,1,32>": "gate-residual M=3900 (256 x 288 tile, 64-byte ring)",
    "gemm288q_dma_kernel<.,1,64>": "gate-residual M=4352 (> 256 tiles, 128-byte ring)",
    "gemm288q_dma_kernel<.,2,32>": "heads T=4096, K=64 (256 x 288 tile)",
    "gemm288q_dma_kernel<.,2,64>": "heads T=4096, K=256 (256 x 288 tile, 128-byte ring)",
    "gemm288q_dma_kernel<.,3,32>": "residual M=4096 N=4608",
    "gemm288q_dma_kernel<.,3,64>": "residual M=4352 N=4608 (> 256 tiles)",
}


def _check_rows(got, pre, ref, dtype, K, M, what, **kw):
    """check_contract over all rows, and separately over a ragged last 128-row tile (criteria 2 and 3 are statistics: a
    rounding error confined to the tail tile would vanish in the whole)."""
    rep = cr.check_contract(got, pre, ref, dtype, K, what=what, **kw)
    t0 = M - M % 128
    if M % 128 and M > 128:
        sl = lambda a: a[t0:] if np.ndim(a) == 2 else a
        kw = {k: sl(v) for k, v in kw.items()}
        cr.check_contract(cr._f64(got)[t0:], pre[t0:], ref[t0:], dtype, K, what=what + " (ragged tail tile)", **kw)
    return rep


def _operands(seed, M, N, K, dtype, band="normal", bias=True):
    """A [M, K], W [N, K], bias [N] 16-bit on the device.  band: "normal" (outputs ~ N(0, 1)), "f16_overflow" (|y| around
    65504: a good share lands in [60000, 70000]), "f16_subnormal" (|y| mostly below 6.1e-5), "bf16_binades" (rows scaled by
    2^-12 .. 2^11: outputs across 20+ binades)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    A = torch.randn(M, K, device=DEV, generator=g)
    W = torch.randn(N, K, device=DEV, generator=g) * K ** -0.5
    b = torch.randn(N, device=DEV, generator=g) * 0.3 if bias else None
    s = {"normal": 1.0, "f16_overflow": 52000.0, "f16_subnormal": 2.5e-5, "bf16_binades": 1.0}[band]
    A, W = A * s ** 0.5, W * s ** 0.5
    if b is not None:
        b = b * s
    if band == "bf16_binades":
        A = A * torch.pow(2.0, (torch.arange(M, device=DEV) % 24 - 12).float())[:, None]
        if b is not None:
            b = b * 2.0 ** -12
    return A.to(dtype), W.to(dtype), (b.to(dtype) if b is not None else None)


def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode()) % 100000


def _acc(A, W, b=None):
    """Exact A W^T + b (float64 on the device: the CPU would need seconds at the larger shapes) as numpy."""
    acc = A.double() @ W.double().t()
    if b is not None:
        acc = acc + b.double()
    return acc.cpu().numpy()


def _launched():
    from topia_xl_amd import _lib
    return _lib.load().primx_last_gemm_kernel().decode()


def check_linear(got, acc, dtype, K, M, act, scale, what):
    """The contract check of one primx_linear output `got` ([M, N]; acc = the exact A W^T + bias): the arguments
    test_gemm_contract uses (also called by tests/test_hip_extent.py on row blocks of far larger operands)."""
    pre, ref = cr.linear_ref(acc, dtype, act, scale)
    one = act == 0 and cr.f32(scale) == 1.0                 # one rounding, no element-wise stage
    return _check_rows(got, pre, ref, dtype, K, M, what, acc=acc, gain=1.2 * abs(scale),
                       inner=(0.0 if one else 1.2 * abs(cr.f32(scale)) * cr.ulp16(acc, dtype)), ew_ulps=(0.0 if one else 4.0))


def check_linear_residual(got, acc, dtype, K, M, res, scale, what):
    """The same for primx_linear_residual: ((A W^T + bias) + res) * scale with one rounding (res may be None)."""
    pre, ref = cr.linear_residual_ref(acc, dtype, res, scale)
    return _check_rows(got, pre, ref, dtype, K, M, what, acc=pre, ew_ulps=(2.0 if res is not None else 0.0))


def check_gate_increment(x, acc, gate_rows, dtype, K, M, what):
    """primx_linear_gate_residual on x_in = 0: the fp32 x holds the 16-bit increment cast16(gate * cast16(A W^T + bias))
    itself (gate_rows [M, N] = the gate of each row)."""
    pre, ref = cr.gate_residual_ref(acc, gate_rows, dtype)
    xg = cr._f64(x)
    assert np.array_equal(cr.round16(xg, dtype), xg), f"{what}: the increment is not a 16-bit value"
    return _check_rows(xg, pre, ref, dtype, K, M, f"{what} increment", acc=acc, gain=gate_rows, inner=np.abs(gate_rows) * cr.ulp16(acc, dtype))


def check_heads_segment(got, a_seg, dtype, K, first, scale0, what):
    """One segment of primx_linear_heads (got, a_seg: [B, n, H, dh]; a_seg = the exact projection): segment 0 is scaled by
    scale0 AFTER its rounding, the others are rounded once."""
    if first:
        qpre = cr.f32(scale0) * cr.round16(a_seg, dtype)
        return cr.check_contract(got, qpre, cr.round16(qpre, dtype), dtype, K, acc=a_seg, gain=scale0, ew_ulps=1.0,
                                 inner=scale0 * cr.ulp16(a_seg, dtype), what=what)
    return cr.check_contract(got, a_seg, cr.round16(a_seg, dtype), dtype, K, what=what)


def _check_gemm_case(ops, dtype, case, reached, band="normal"):
    op, M, N, K = case["op"], case["M"], case["N"], case["K"]
    seed = _seed(op, M, N, K, band)
    A, W, b = _operands(seed, M, N, K, dtype, band, bias=case.get("bias", True))
    acc = _acc(A, W, b)
    what = f"{op} {M}x{N}x{K} {band}"

    def note():
        name = _launched()
        fam = _kernel_family(name, dtype)
        if _default_dispatch():                 # (a kernel-selection switch reaches pairs the default dispatch never takes)
            assert fam in KERNELS, f"{what}: kernel {name} has no row in the contract table"
            if "expect" in case:
                assert fam == case["expect"], (what, name)
        reached.add(fam)

    if op == "linear":
        for act, scale in case.get("acts", [(0, 1.0)]):
            got = ops.linear(A, W, b, act=act, out_scale=scale)
            note()
            check_linear(got, acc, dtype, K, M, act, scale, f"{what} act={act} scale={scale}")
    elif op == "residual":
        g = torch.Generator(device=DEV).manual_seed(seed + 1)
        res = (torch.randn(M, N, device=DEV, generator=g) * 0.3 * float(np.sqrt(np.mean(acc ** 2)))).to(dtype)
        for r, sc in ((res, 0.70710678), (None, 1.0)):
            got = ops.linear_residual(A, W, b, r, sc)
            note()
            check_linear_residual(got, acc, dtype, K, M, r, sc, f"{what} res={r is not None}")
    elif op in ("gate", "gate_ln"):
        rpb = case["rpb"]
        nb = (M + rpb - 1) // rpb
        g = torch.Generator(device=DEV).manual_seed(seed + 2)
        mod = (torch.randn(nb, 3 * N, device=DEV, generator=g) * 0.5).to(dtype)
        gate, shift, scl = mod[:, :N], mod[:, N:2 * N], mod[:, 2 * N:]
        rows = np.arange(M) // rpb
        gate_rows = gate.double().cpu().numpy()[rows]
        x = torch.zeros(M, N, device=DEV)
        if op == "gate":
            ops.linear_gate_residual(A, W, b, gate, x, rpb)
            note()
        else:
            lnout = torch.empty(M, N, dtype=dtype, device=DEV)
            sync = torch.zeros(ops.ln_sync_words(M), dtype=torch.int32, device=DEV)
            ops.linear_gate_residual(A, W, b, gate, x, rpb, ln=(shift, scl, lnout, 1e-6, sync))
            note()
        # x_in = 0: the fp32 x receives the 16-bit increment itself, exactly
        check_gate_increment(x, acc, gate_rows, dtype, K, M, what)
        if op == "gate_ln":
            lpre, lref = cr.layernorm_modulate_ref(x, shift.double().cpu().numpy()[rows], scl.double().cpu().numpy()[rows], dtype)
            cr.check_contract(lnout, lpre, lref, dtype, N, ew_ulps=8.0, what=f"{what} LayerNorm tail")
        # x_in != 0: x_out = fp32(x_in + increment) with the same increment bits
        x0 = torch.randn(M, N, device=DEV, generator=g) * 4.0
        x1 = x0.clone()
        if op == "gate":
            ops.linear_gate_residual(A, W, b, gate, x1, rpb)
        else:
            ops.linear_gate_residual(A, W, b, gate, x1, rpb, ln=(shift, scl, lnout, 1e-6, sync))
        assert torch.equal(x1, x0 + x), f"{what}: x += increment is not one fp32 addition"
    elif op == "heads":
        from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
        B, n, H, dh = case["B"], case["n"], case["H"], case["dh"]
        kinds = case.get("kinds", [HEADS_ROWS, HEADS_KROWS, HEADS_VT])
        scale0 = dh ** -0.5
        pad = 256 if n % 256 == 0 else 128
        dsts = [ops.alloc_heads(B, H, n, dh, kd, dtype, DEV, pad) for kd in kinds]
        ops.linear_heads(A, W, b, n, H, dh, kinds, dsts, dsts[0].shape[2], scale0=scale0)
        note()
        a5 = acc.reshape(B, n, len(kinds), H, dh)
        for s_, (kd, dst) in enumerate(zip(kinds, dsts)):
            got = unpack_vt(dst, n, dh) if kd == HEADS_VT else unpack_rows(dst, n, dh)
            check_heads_segment(got, a5[:, :, s_], dtype, K, s_ == 0, scale0,
                                f"{what} segment 0 (scaled after rounding)" if s_ == 0 else f"{what} segment {s_} kind {kd}")
    else:
        raise AssertionError(op)


_ACTS = [(0, 1.0), (1, 1.0), (2, 1.0), (0, 72 ** -0.5), (1, 0.25)]
GEMM_CASES = [
    dict(op="linear", M=3, N=1156, K=1152, expect="gemv16_kernel<.,4>"),
    dict(op="linear", M=7, N=2308, K=264, expect="gemv16_kernel<.,8>"),
    dict(op="linear", M=3, N=1156, K=1152, acts=[(1, 1.0), (0, 0.5)]),                      # act / scale: no GEMV
    dict(op="linear", M=300, N=20, K=1160, acts=_ACTS, expect="gemm_kernel<.,0,32,4,1,1,1,.>"),
    dict(op="residual", M=700, N=32, K=256, expect="gemm_kernel<.,3,32,4,1,1,1,.>"),
    dict(op="linear", M=129, N=136, K=1152, acts=_ACTS, expect="gemm_kernel<.,0,32,2,2,2,2,.>"),
    dict(op="linear", M=257, N=288, K=200, bias=False, acts=_ACTS, expect="gemm_kernel<.,0,32,2,2,2,2,.>"),
    dict(op="gate", M=300, N=200, K=136, rpb=150, expect="gemm_kernel<.,1,32,2,2,2,2,.>"),
    dict(op="residual", M=1001, N=100, K=264, expect="gemm_kernel<.,3,32,2,2,2,2,.>"),
    dict(op="linear", M=300, N=288, K=128, acts=_ACTS, expect="gemm144l_dma_kernel<.,0>"),
    dict(op="linear", M=1370, N=288, K=1152, bias=False, expect="gemm144l_dma_kernel<.,0>"),
    dict(op="gate", M=300, N=288, K=192, rpb=150, expect="gemm144l_dma_kernel<.,1>"),
    dict(op="gate_ln", M=1024 - 77, N=1152, K=192, rpb=300, expect="gemm144l_dma_kernel<.,5>"),
    dict(op="residual", M=300, N=288, K=128, expect="gemm144_dma_kernel<.,3>"),
    dict(op="heads", M=3 * 70, N=3 * 288, K=64, B=3, n=70, H=4, dh=72, expect="gemm144_dma_kernel<.,2>"),
    dict(op="heads", M=300, N=3 * 144, K=200, B=1, n=300, H=2, dh=72, expect="gemm_kernel<.,2,32,2,2,2,2,.>"),
    dict(op="heads", M=2 * 256, N=2 * 144, K=128, B=2, n=256, H=2, dh=72, kinds=[0, 2], expect="gemm144l_dma_kernel<.,2>"),
    dict(op="heads", M=4096, N=3 * 1152, K=256, B=2, n=2048, H=16, dh=72, expect="gemm288q_dma_kernel<.,2,64>"),
    dict(op="heads", M=4096, N=3 * 1152, K=64, B=2, n=2048, H=16, dh=72, expect="gemm288q_dma_kernel<.,2,32>"),
    dict(op="gate", M=3900, N=4608, K=64, rpb=1950, expect="gemm288q_dma_kernel<.,1,32>"),
    dict(op="gate", M=4352, N=4608, K=64, rpb=1024, expect="gemm288q_dma_kernel<.,1,64>"),
    dict(op="linear", M=4096, N=4608, K=64, acts=_ACTS, expect="gemm288q_dma_kernel<.,0,64>"),
    dict(op="linear", M=3600, N=4608, K=1152, acts=[(1, 1.0)], expect="gemm288q_dma_kernel<.,0,64>"),
    dict(op="residual", M=4096, N=4608, K=128, expect="gemm288q_dma_kernel<.,3,32>"),
    dict(op="residual", M=4352 - 100, N=4608, K=64, expect="gemm288q_dma_kernel<.,3,64>"),
]
# the value bands: plain Linear / residual outputs (one rounding) on each kernel family
BAND_CASES = [c for c in GEMM_CASES if c["op"] in ("linear", "residual") and "expect" in c]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_contract(ops, dtype):
    """Linear (act 0 / 1 / 2, out_scale != 1, bias and none), linear_residual, gate-residual (+ LayerNorm tail) and the
    heads epilogue on every kernel of the default dispatch - ragged M, N and K tails included - and every kernel in
    KERNELS reached (under the default dispatch)."""
    reached = set()
    for case in GEMM_CASES:
        _check_gemm_case(ops, dtype, case, reached)
    if _default_dispatch():
        missing = sorted(set(KERNELS) - reached)
        assert not missing, f"kernels of the default dispatch without contract coverage: {missing}"
        print(f"contract coverage {dtype}: " + "; ".join(f"{k}: {v}" for k, v in KERNELS.items()))


@pytest.mark.parametrize("dtype,band", [(F16, "f16_overflow"), (F16, "f16_subnormal"), (BF16, "bf16_binades")])
def test_gemm_contract_value_bands(ops, dtype, band):
    """The same epilogues with outputs in the fp16 overflow band (65520 and above must be inf, not 65504), in the fp16
    subnormal range (not flushed) and across 20+ bf16 binades."""
    reached = set()
    for case in BAND_CASES:
        c = dict(case, acts=[(0, 1.0)])
        M = c["M"]
        _check_gemm_case(ops, dtype, c, reached, band)
        if band == "f16_overflow" and c["op"] == "linear":
            y = cr.round16(_acc(*_operands(_seed(c["op"], M, c["N"], c["K"], band), M, c["N"], c["K"], dtype, band,
                                           c.get("bias", True))), dtype)
            assert np.isinf(y).mean() > 0.05 and (np.abs(y[np.isfinite(y)]) >= 60000).mean() > 0.02, c   # the band is reached


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,rows,rpb", [(1152, 600, 256), (384, 301, 100), (256, 130, 64)])
def test_layernorm_modulate_contract(ops, dtype, D, rows, rpb):
    g = torch.Generator(device=DEV).manual_seed(D + rows)
    x = torch.randn(rows, D, device=DEV, generator=g) * 3.0 + 0.7
    nb = (rows + rpb - 1) // rpb
    mod = (torch.randn(nb, 3 * D, device=DEV, generator=g) * 0.4).to(dtype)          # [shift | scale | other] rows, stride 3 D
    shift, scale = mod[:, :D], mod[:, D:2 * D]
    out = ops.layernorm_modulate(x, shift, scale, rpb, torch.empty(rows, D, dtype=dtype, device=DEV))
    r = np.arange(rows) // rpb
    pre, ref = cr.layernorm_modulate_ref(x, shift.double().cpu().numpy()[r], scale.double().cpu().numpy()[r], dtype)
    cr.check_contract(out, pre, ref, dtype, D, ew_ulps=8.0, what=f"layernorm_modulate D={D}")


def _wide_f32(n, seed, lo=-30, hi=20):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, device=DEV, generator=g) * torch.pow(2.0, torch.randint(lo, hi, (n,), device=DEV, generator=g).float())


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast16_and_silu_cast_contract(ops, dtype):
    """cast16: correct rounding of fp32 - exact midpoints (ties to even), the fp16 overflow threshold, subnormals;
    silu_cast: one rounding of silu(x) over 50 binades."""
    x = _wide_f32(1 << 18, 5)
    p, emin, _ = cr._FMT[dtype]
    g = torch.Generator().manual_seed(6)
    e = torch.randint(emin - p + 1, 16, (1 << 14,), generator=g)
    mant = torch.randint(1 << (p - 1), 1 << p, (1 << 14,), generator=g).double() + 0.5
    ties = torch.ldexp(mant, (e - (p - 1)).double()).float().to(DEV)                       # exact midpoints (fp32-exact)
    edge = torch.tensor([65504.0, 65519.996, 65520.0, 65536.0, 1e30, -65520.0, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26,
                         2.0 ** -133, 2.0 ** -134, 0.0, -0.0, float("inf"), float("-inf")], device=DEV)
    x = torch.cat([x, ties, -ties, edge])
    got = ops.cast16(x, dtype)
    pre, ref = cr.cast16_ref(x, dtype)
    rep = cr.check_contract(got, pre, ref, dtype, 1, ew_ulps=0.0, what="cast16")
    assert rep["differ"] == 0, rep                                                         # a conversion is exact to the contract
    xs = _wide_f32(1 << 18, 7, -20, 8)
    got = ops.silu_cast(xs, dtype)
    pre, ref = cr.silu_cast_ref(xs, dtype)
    # (__expf: v_exp_f32 of x log2 e - its relative error grows with |x|, about |x| fp32 ulps)
    cr.check_contract(got, pre, ref, dtype, 1, ew_ulps=(4.0 + 2.0 * xs.abs().cpu().double().numpy()), what="silu_cast")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("s", [6.0, 4.37, 1.0])
def test_cfg_combine_contract(ops, dtype, s):
    g = torch.Generator(device=DEV).manual_seed(int(s * 100))
    base = torch.randn(2, 300, 1152, device=DEV, generator=g)
    base[1] = base[0] + 0.05 * torch.randn(300, 1152, device=DEV, generator=g)            # cond / uncond close: cancellation
    inp = base.to(dtype)
    got = ops.cfg_combine(inp, s)
    pre, ref = cr.cfg_combine_ref(inp[0], inp[1], s, dtype)
    # the differences of 16-bit values are exact in fp32; s * d is one fp32 product (24 x 11 bits) in front of its 16-bit
    # rounding, which can round twice: then m moves by one ulp16(m), and the result with it
    m = cr.round16(cr.f32(s) * cr.round16(inp[0].double().cpu().numpy() - inp[1].double().cpu().numpy(), dtype), dtype)
    cr.check_contract(got, pre, ref, dtype, 1, ew_ulps=1.0, inner=cr.ulp16(m, dtype), what=f"cfg_combine s={s}")


# ------------------------------------------------------------------------------------------------ VAE kernels
def _cl_rand(seed, P, V, C, dtype, scale=1.0, offset=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(P, V, C, device=DEV, generator=g) * scale + offset).to(dtype)


def _gn_params(seed, C):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(C, device=DEV, generator=g) * 0.2 + 1.0, torch.randn(C, device=DEV, generator=g) * 0.2


def check_groupnorm_silu(got, x, gam, bet, groups, silu, dtype):
    """The contract check of a primx_groupnorm_silu output for the operands it was computed from (x [P, V, C], eps 1e-5); the
    check functions below follow the same pattern and are also run by tests/test_hip_extent.py on single primitives of far
    larger batches."""
    _, V, C = x.shape
    pre, ref = cr.groupnorm_silu_ref(x, gam, bet, groups, 1e-5, silu, dtype)
    return cr.check_contract(got, pre, ref, dtype, V * C // groups, ew_ulps=8.0, what=f"groupnorm_silu C={C} V={V}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,V,groups,silu", [(256, 64, 32, True), (256, 512, 32, True), (32, 512, 32, True), (64, 27, 8, False)])
def test_groupnorm_silu_contract(ops, dtype, C, V, groups, silu):
    x = _cl_rand(C + V, 3, V, C, dtype, 1.3, 0.2)
    gam, bet = _gn_params(C, C)
    check_groupnorm_silu(ops.groupnorm_silu(x, gam, bet, groups, 1e-5, silu), x, gam, bet, groups, silu, dtype)


def _conv_w(seed, Cout, Cin, dtype):
    from topia_xl_amd.vae import _conv_weight_as_gemm
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(Cout, Cin, 3, 3, 3, device=DEV, generator=g) * (27 * Cin) ** -0.5
    b = (torch.randn(Cout, device=DEV, generator=g) * 0.2).to(dtype)
    return _conv_weight_as_gemm(w, dtype), b


def check_conv3d_k3(got, acc, dtype, K, res, res_scale, what):
    """conv3d_k3 (any route): ((conv + bias) + res) * res_scale with one rounding; acc [P, V, Cout] = the exact conv + bias
    (cr.conv3d_k3_acc), res None or the residual operand."""
    pre, ref = cr.linear_residual_ref(acc, dtype, res, res_scale)
    return cr.check_contract(got, pre, ref, dtype, K, what=what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cin,Cout,S,P,packed", [(256, 256, 4, 3, "s4"), (256, 512, 4, 2, "s4"), (256, 32, 8, 2, "s8"),
                                                 (32, 32, 8, 3, "s8c32"), (32, 6, 8, 3, "s8c32"), (64, 48, 4, 3, None)])
def test_conv3d_k3_contract(ops, dtype, Cin, Cout, S, P, packed):
    """((conv + bias) + res) * scale with one rounding - the implicit GEMM, and the activation-resident kernel of the shape
    held to the same contract (not just close to the implicit GEMM)."""
    V = S ** 3
    x = _cl_rand(Cin + S, P, V, Cin, dtype)
    wk, b = _conv_w(Cin * Cout, Cout, Cin, dtype)
    acc = cr.conv3d_k3_acc(x, wk, b, S).reshape(P, V, Cout)
    rms = float(np.sqrt(np.mean(acc ** 2)))
    res = _cl_rand(Cout, P, V, Cout, dtype, rms)
    K = 27 * Cin
    routes = [("implicit GEMM", None)]
    wp = ops.pack_conv3(wk, Cin)
    if packed is not None and os.environ.get("PRIMX_CONV_REG", "1") != "0":
        assert wp is not None and wp.kind == packed and wp.S == S
        routes.append((packed, wp))
    for route, w in routes:
        got = ops.conv3d_k3(x, wk, b, S, res=res, res_scale=0.5 ** 0.5, Wp=w)
        check_conv3d_k3(got, acc, dtype, K, res, 0.5 ** 0.5, f"conv3d_k3 {route} {Cin}->{Cout} @{S}")
        got = ops.conv3d_k3(x, wk, None, S, Wp=w)
        check_conv3d_k3(got, acc - b.double().cpu().numpy(), dtype, K, None, 1.0, f"conv3d_k3 {route} no bias")


def _flip_tolerance(a16, wk, dtype):
    """Criterion 1's allowance for the normalised activations the kernel forms itself.  It rounds silu(GN(x)) from fp32
    statistics that differ from the exact ones by far less than a 16-bit ulp, so only an activation whose exact value lies
    next to a rounding boundary can round the other way, and then by one ulp16(a).  Such activations are rare (a fraction of
    about 2^-24 sqrt(n) / 2^-11 of them), so an output's 27 Cin inputs hold at most a couple: each moves the output by at
    most |w| ulp16(a).  Allowance per output channel: 2 max_k |W[co, k]| max ulp16(a)."""
    wmax = np.abs(wk.double().cpu().numpy()).max(1)
    return 2.0 * wmax * float(np.max(cr.ulp16(a16, dtype)))


def check_conv3d_s8c32_gn(got, acc, a16, wk, dtype, res, res_scale, Cout):
    """The 8^3 / 32-channel kernel with the GroupNorm inside: acc = the exact convolution of a16 = round16(silu(GN(x)))."""
    pre, ref = cr.linear_residual_ref(acc, dtype, res, res_scale)
    return cr.check_contract(got, pre, ref, dtype, 27 * 32, ew_ulps=2.0, inner=_flip_tolerance(a16, wk, dtype),
                             what=f"conv3d s8c32 gn Cout={Cout}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cout,P", [(32, 3), (6, 2)])
def test_conv3d_s8c32_groupnorm_inside_contract(ops, dtype, Cout, P):
    """GroupNorm (one channel per group) + SiLU inside the 8^3 kernel: the normalised activations rounded to 16 bits,
    then ((conv + bias) + res) * scale with one rounding."""
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the implicit GEMM: no kernel takes the GroupNorm")
    S, Cin, V = 8, 32, 512
    x = _cl_rand(11, P, V, Cin, dtype, 1.4, 0.3)
    gam, bet = _gn_params(12, Cin)
    wk, b = _conv_w(13, Cout, Cin, dtype)
    wp = ops.pack_conv3(wk, Cin)
    _, a16 = cr.groupnorm_silu_ref(x, gam, bet, 32, 1e-5, True, dtype)
    acc = cr.conv3d_k3_acc(a16, wk, b, S).reshape(P, V, Cout)
    res = _cl_rand(14, P, V, Cout, dtype, float(np.sqrt(np.mean(acc ** 2))))
    got = ops.conv3d_k3(x, wk, b, S, res=res, res_scale=0.5 ** 0.5, Wp=wp, gn=(gam, bet, 1e-5))
    check_conv3d_s8c32_gn(got, acc, a16, wk, dtype, res, 0.5 ** 0.5, Cout)


def check_conv3d_s8_fused(t, sc, h8, gam, bet, wk, b1, wsc, bsc, dtype):
    """conv3d_s8_fused's two outputs for the 16-bit upsample output h8 [P, 512, 256] they were computed from."""
    P, _, C = h8.shape
    _, a16 = cr.groupnorm_silu_ref(h8, gam, bet, 32, 1e-5, True, dtype)
    acc = cr.conv3d_k3_acc(a16, wk, b1, 8).reshape(P, 512, 32)
    r1 = cr.check_contract(t, acc, cr.round16(acc, dtype), dtype, 27 * C, inner=_flip_tolerance(a16, wk, dtype),
                           what="conv3d_s8_fused conv1")
    sacc = cr.gemm_acc(h8.reshape(P * 512, C), wsc, bsc).reshape(P, 512, 32)
    return r1, cr.check_contract(sc, sacc, cr.round16(sacc, dtype), dtype, C, what="conv3d_s8_fused shortcut")


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv3d_s8_fused_contract(ops, dtype):
    """The fused front of the 256 -> 32 block: conv1(round16(silu(GN(h8)))) + bias with one rounding, and the 1x1 shortcut
    Wsc h8 + bsc with one rounding, h8 = the 16-bit upsample output."""
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the unfused kernels")
    P, C = 3, 256
    x = _cl_rand(21, P, 64, C, dtype)
    g = torch.Generator(device=DEV).manual_seed(22)
    wt = (torch.randn(8 * C, C, device=DEV, generator=g) * C ** -0.5).to(dtype)
    bu = (torch.randn(C, device=DEV, generator=g) * 0.3).to(dtype)
    gam, bet = _gn_params(23, C)
    wk, b1 = _conv_w(24, 32, C, dtype)
    wsc = (torch.randn(32, C, device=DEV, generator=g) * C ** -0.5).to(dtype)
    bsc = (torch.randn(32, device=DEV, generator=g) * 0.2).to(dtype)
    h8, part = ops.convtranspose_k2s2(x, wt, bu, 4, Wp=ops.pack_convt_s4(wt), want_stats=True)
    wp = ops.pack_conv3(wk, C, Wsc=wsc)
    t, sc = ops.conv3d_s8_fused(h8, wp, b1, part, bu, gam, bet, 1e-5, bsc)
    check_conv3d_s8_fused(t, sc, h8, gam, bet, wk, b1, wsc, bsc, dtype)


def check_convtranspose_k2s2(got, acc, dtype, Cin, what):
    """k2s2 upsample, either form: acc = cr.convtranspose_k2s2_acc of the operands, one rounding."""
    return cr.check_contract(got, acc, cr.round16(acc, dtype), dtype, Cin, what=what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P,S,Cin,Cout", [(3, 4, 256, 256), (2, 4, 64, 48)])
def test_convtranspose_k2s2_contract(ops, dtype, P, S, Cin, Cout):
    """k2s2 upsample: bias + one sum, one rounding - the GEMM form and the weight-stationary packed kernel."""
    x = _cl_rand(31 + Cin, P, S ** 3, Cin, dtype)
    g = torch.Generator(device=DEV).manual_seed(32)
    wt = (torch.randn(8 * Cout, Cin, device=DEV, generator=g) * Cin ** -0.5).to(dtype)
    b = (torch.randn(Cout, device=DEV, generator=g) * 0.3).to(dtype)
    acc = cr.convtranspose_k2s2_acc(x, wt, b, S)
    check_convtranspose_k2s2(ops.convtranspose_k2s2(x, wt, b, S), acc, dtype, Cin, "convtranspose_k2s2 GEMM form")
    wp = ops.pack_convt_s4(wt)
    if wp is not None:
        got, _ = ops.convtranspose_k2s2(x, wt, b, S, Wp=wp, want_stats=True)
        check_convtranspose_k2s2(got, acc, dtype, Cin, "convtranspose_k2s2 packed")


def check_conv_in(got, z, pq_scale, pq_bias, W, b, S, dtype):
    acc = cr.conv_in_acc(z, pq_scale, pq_bias, W, b, S)
    return cr.check_contract(got, acc, cr.round16(acc, dtype), dtype, 27, ew_ulps=8.0, what=f"conv_in S={S}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S,Cout", [(4, 256), (8, 32)])
def test_conv_in_contract(ops, dtype, S, Cout):
    P = 3
    g = torch.Generator(device=DEV).manual_seed(41 + S)
    z = torch.randn(P, S ** 3, device=DEV, generator=g)
    W = torch.randn(Cout, 27, device=DEV, generator=g) * 0.2
    b = torch.randn(Cout, device=DEV, generator=g) * 0.2
    check_conv_in(ops.conv_in(z, 1.7, -0.3, W, b, S, dtype), z, 1.7, -0.3, W, b, S, dtype)


# ------------------------------------------------------------------------------------------------ fp32 outputs
def test_gemm_f32_rigorous_bound(ops):
    """primx_gemm_f32 is EXACT fp32 arithmetic: every element within gamma_K sum|a||w| (+ the scale / gate rounding)."""
    for (M, N, K) in ((257, 384, 1152), (200, 136, 68), (2, 300, 256)):
        g = torch.Generator(device=DEV).manual_seed(M + N + K)
        A = torch.randn(M, K, device=DEV, generator=g)
        W = torch.randn(N, K, device=DEV, generator=g) * K ** -0.5
        b = torch.randn(N, device=DEV, generator=g) * 0.1
        exact = cr.gemm_acc(A, W, b)
        bound = cr.gemm_abs_bound(A, W, b)
        got = ops.gemm_f32(A, W, b).double().cpu().numpy()
        assert np.all(np.abs(got - exact) <= bound), float(np.max(np.abs(got - exact) / bound))
        s = 0.37
        got = ops.gemm_f32(A, W, b, out_scale=s).double().cpu().numpy()
        assert np.all(np.abs(got - cr.f32(s) * exact) <= cr.f32(s) * bound * (1 + 2 ** -23) + 2 ** -24 * np.abs(cr.f32(s) * exact) * 1.01)
        rpb = (M + 1) // 2
        gate = torch.randn((M + rpb - 1) // rpb, N, device=DEV, generator=g)
        x0 = torch.randn(M, N, device=DEV, generator=g)
        x = x0.clone()
        ops.gemm_f32(A, W, b, out=x, gate=gate, rows_per_batch=rpb)
        gr = gate.double().cpu().numpy()[np.arange(M) // rpb]
        want = x0.double().cpu().numpy() + gr * exact
        bnd = np.abs(gr) * bound * (1 + 2 ** -22) + 2 ** -23 * (np.abs(x0.double().cpu().numpy()) + np.abs(gr * exact)) * 1.01
        assert np.all(np.abs(x.double().cpu().numpy() - want) <= bnd)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_f32out_rigorous_bound(ops, dtype):
    """primx_linear_f32out[_group]: fp32 rows of A W^T (+ bias from bias_from_row on) from 16-bit operands: every element
    within gamma_(K+1) (sum|a||w| + |b|)."""
    M, K = 16, 1152
    problems, wants = [], []
    for i, N in enumerate((1152, 3456, 288)):
        g = torch.Generator(device=DEV).manual_seed(51 + i)
        A = torch.randn(M, K, device=DEV, generator=g).to(dtype)
        W = (torch.randn(N, K, device=DEV, generator=g) * K ** -0.5).to(dtype)
        b = (torch.randn(N, device=DEV, generator=g) * 0.3).to(dtype)
        exact = cr.gemm_acc(A, W, None)
        exact[8:] += b.double().cpu().numpy()
        bound = cr.gemm_abs_bound(A, W, b)
        out = torch.empty(M, N, device=DEV)
        ops.linear_f32out(A, W, b, out, 8)
        assert np.all(np.abs(out.double().cpu().numpy() - exact) <= bound), f"linear_f32out N={N}"
        problems.append((A, W, b, torch.empty(M, N, device=DEV)))
        wants.append((exact, bound))
    grouped = ops.linear_f32out_group(problems, 8)
    assert grouped or os.environ.get("PRIMX_UV_GROUP") == "0", "the grouped fp32-out kernel did not run"
    if grouped:
        for (_, _, _, out), (exact, bound) in zip(problems, wants):
            assert np.all(np.abs(out.double().cpu().numpy() - exact) <= bound), "linear_f32out_group"


# ------------------------------------------------------------------------------------------------ attention
# attn_kernel / attn64_kernel are not one-rounding operations: what they approximate, the per-element bound derived from it and the
# check (ATTN_SLACK, the bias criterion) live in tests/contract_ref.py next to the fp32 kernel's form of the same bound.
ATTN_SLACK = cr.ATTN_SLACK
_attn_bound = cr.attn_bound
_attn_check = cr.attn_check


def _qkv(seed, B, Mq, Mk, H, dh, sigma, dtype):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randn(B, Mq, H, dh, device=DEV, generator=g) * sigma            # logits q.k / sqrt(dh) have std sigma
    k = torch.randn(B, Mk, H, dh, device=DEV, generator=g)
    v = torch.randn(B, Mk, H, dh, device=DEV, generator=g)
    return q.to(dtype), k.to(dtype), v.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sigma", [0.5, 4.0, 16.0])
@pytest.mark.parametrize("B,Mq,Mk,H,dh", [(1, 300, 1000, 2, 72), (1, 200, 700, 2, 64), (2, 300, 500, 2, 32)])
def test_attention_bound(ops, dtype, sigma, B, Mq, Mk, H, dh):
    """attn_kernel at dh = 72 / 64 / 32 with ragged query and key counts, logit spreads sigma = 0.5, 4, 16."""
    q, k, v = _qkv(int(sigma * 10) + dh, B, Mq, Mk, H, dh, sigma, dtype)
    got = ops.memory_efficient_attention(q, k, v)
    _attn_check(got, q, k, v, dh ** -0.5, dtype, dh == 72, f"dh={dh} sigma={sigma}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sigma", [0.5, 4.0, 16.0])
def test_attention64_bound(ops, dtype, sigma):
    """attn64_kernel: the VAE mid-block shape (dh = 32, at most 64 queries and keys) in compact 64-token buffers."""
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    B, M, H, dh = 3, 64, 4, 32
    q, k, v = _qkv(int(sigma * 10) + 7, B, M, M, H, dh, sigma, dtype)
    k, v = k[:, :50].contiguous(), v[:, :50].contiguous()                      # 50 keys: a masked tail
    Qp = ops.pack_heads(q, HEADS_ROWS, 64, "q")
    Kp = ops.pack_heads(k, HEADS_KROWS, 64, "k")
    Vt = ops.pack_heads(v, HEADS_VT, 64)
    assert Qp.shape[2] == 64 and Kp.shape[2] == 64                             # the compact form attn64_kernel takes
    got = ops.attention(Qp, Kp, Vt, M, 50, dh, dh ** -0.5).view(B, M, H, dh)
    _attn_check(got, q, k, v, dh ** -0.5, dtype, False, f"attn64 sigma={sigma}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_bound_forced_rescale(ops, dtype):
    """The spike pattern of test_hip_attention.py (a key whose score dwarfs the others arrives in a late tile: the running
    max jumps and every earlier contribution is rescaled) and the ramp that keeps the kernel on a stale max for several tiles."""
    B, N, H, dh = 1, 512, 1, 72
    q, k, v = _qkv(23, B, N, N, H, dh, 1.0, dtype)
    k[0, 300, 0] = q[0, 17, 0] * 6.0
    k[0, 500, 0] = q[0, 200, 0] * 9.0
    _attn_check(ops.memory_efficient_attention(q, k, v), q, k, v, dh ** -0.5, dtype, True, "spike")
    N, H = 1024, 2
    q, k, v = _qkv(25, B, N, N, H, dh, 0.3, dtype)
    q[..., 0] = 4.0
    ramp = (torch.arange(N, device=DEV) // 64).float() * 3.0 / (4.0 * dh ** -0.5 * 1.4427)
    k[0, :, :, 0] = ramp[:, None].to(dtype)
    _attn_check(ops.memory_efficient_attention(q, k, v), q, k, v, dh ** -0.5, dtype, True, "ramp")
