"""The fp32 entry points against float64, element by element, at shipped shapes: csrc/fp32.hip (gemm_f32, attention_f32,
layernorm_modulate_f32, silu_f32 - the reference's fp32 call path) and the fp32 front end of csrc/rowops.hip that every 16-bit
forward starts with (linear_f32, timestep_embedding, point_features, vit_tokens, row_stats).

Two criteria per case (tests/contract_ref.py, "the fp32 entry points"):
  1. every element within a rigorous worst-case bound of the float64 value (u = 2^-24, gamma_n, the device functions' ulps; no
     measured constant, no slack factor) - tests/test_fp32_contract_cpu.py shows on the CPU that a correct fp32 evaluation
     stays inside and a faulty one does not;
  2. where the bound sits far above a healthy kernel (GEMMs, attention, LayerNorm): the kernel's rms error against float64 is at
     most RMS_MARGIN = 2 times that of a numpy / torch-CPU fp32 restatement of the same algorithm on the same inputs; ragged last
     tiles (rows and columns) again on their own, so that a tail cannot be averaged away.
vit_tokens and the pass-through columns of point_features are bit-exact.  Every case prints `fp32-contract | entry | case |
max err / bound | rms ratio` before it asserts.

Measured on an MI355X (max |err| / bound; rms error kernel / restatement; no case fails, no finding in a kernel):

  entry point, case                                              err/bound   rms ratio   margin
  gemm_f32 4096x1152x1152 gated (rows_per_batch 2048)              0.170       2.36       4.80
  gemm_f32 4096x4608x1152 tanh-GELU                                0.005       2.53       4.78
  gemm_f32 4096x1152x4608 gated                                    0.008       4.52       9.20
  gemm_f32 2x10368x1152 / 2740x1152x768 / 4096x136x1152         0.003-0.008  1.96-2.37  3.90-4.85
  gemm_f32 257x384xK, K = 4 / 20 / 24 / 28 / 68                  0.63 ... 0.07  0.80-1.00    2.00
  gemm_f32 1x1x4 (one element, = the emulated chain bit for bit)   0.037       3.47       6.94
  gemm_f32 129x129x16; 210x288x96 gated rpb 70; erf-GELU x 0.37  0.19; 0.46; 0.02  0.93-1.03  2.00
  attention_f32 2048x2048 / 2048x1370, sigma 0.5 / 4 / 16        0.002 / 0.020 / 0.031  0.99-1.00  2
  attention_f32 30 ragged shapes per dh (1 ... 128), pooled        <= 0.151    1.00-1.04    2
  attention_f32 spike / ramp / strided views                       <= 0.027    0.95-1.04    2
  layernorm_modulate_f32 D = 4 ... 2048, four bands                <= 0.707    0.57-1.03    2
  silu_f32 3 M values                                              0.956         -
  linear_f32 4096x1152x68 / 4096x1152x52 (+ SiLU)                  0.08-0.10     1.00       2.00
  linear_f32 2738x768x588 (+ SiLU)                                 0.009      1.73-1.84     3.54
  linear_f32 M = 1..8 (wave per column), five (N, K), pooled       <= 0.167   0.38-0.98     2
  linear_f32 M = 9 (tiled), K = 12 / 256 / 260 / 588 / 1152        <= 0.156  1.03 / 1.44 / 1.53 / 3.86 / 2.60  2 x chain factor
  linear_f32 N = 1 / 63 / 65 / 66 next to N = 4 / 64 / 68          <= 0.052   1.00-1.70     2
  timestep_embedding (2 ulp) / point_features (2 ulp)               0.754 / 0.772 (1.5 ulp)   -
  DiTAdditivePosEmb._embed_tokens                                   0.052         -
  row_stats D = 4 / 128 / 132 / 1152                             0.49 / 0.04 / 0.04 / 0.004  -

The GEMM restatement is the BLAS fp32 product, as asked; gemm_f32_kernel and linear_f32_kernel are SERIAL chains of K fused
multiply-adds, whose rounding error grows with sqrt(K) where BLAS's blocked sum does not.  That, not a defect, is every ratio
above 2: contract_ref.chain_factor emulates the chain on a 16 x 256 block of the same operands on the CPU and finds it 1.0 times
BLAS's error up to K = 132, 1.8 - 2.4 times at K = 588 / 768 / 1152 and 4.6 times at K = 4608 (it depends on the BLAS kernel the
shape selects), and the kernels sit at 0.96 - 1.06 of the emulated chain.  The margin of a chain kernel is therefore 2 x chain_factor (computed per case, from the CPU emulation, never
from the kernel); everything else keeps 2.  attention_f32's restatement accumulates P V key by key like the kernel for the same
reason.  The largest err / bound ratios (silu_f32 0.96, layernorm 0.71, gemm K = 4 0.63) are cases of two or three roundings
whose bound IS two or three half-ulps: the numpy restatement reaches the same figures on the CPU.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import contract_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


def _note(entry, case, rb, rr=None):
    print(f"fp32-contract | {entry} | {case} | {rb:.3f} | " + ("-" if rr is None else f"{rr:.2f}"))


class _Pool:
    """rms criterion over several small launches of one kind (a handful of outputs is no sample): pooled squared errors."""

    def __init__(self):
        self.g = self.r = self.e = 0.0
        self.n = 0

    def add(self, got, restated, exact):
        ex = exact.double()
        g, r = got.double().to(ex.device).reshape(ex.shape), cr._t64(restated).to(ex.device).reshape(ex.shape)
        self.g += float(((g - ex) ** 2).sum())
        self.r += float(((r - ex) ** 2).sum())
        self.e += float((ex ** 2).sum())
        self.n += ex.numel()

    def ratio(self):
        n = max(self.n, 1)
        return math.sqrt(self.g / n) / max(math.sqrt(self.r / n), cr.U32 * math.sqrt(self.e / n), 1e-300)


# ------------------------------------------------------------------------------------------------ gemm_f32
GEMM_CASES = [
    dict(M=4096, N=1152, K=1152, rpb=2048),                       # attention / cross-attention projection, gated residual
    dict(M=4096, N=4608, K=1152, act=1),                          # fc1 + tanh-GELU
    dict(M=4096, N=1152, K=4608, rpb=2048),                       # fc2, gated residual
    dict(M=2, N=10368, K=1152),                                   # adaLN modulation of one block (9 D columns)
    dict(M=2740, N=1152, K=768),                                  # condition projection (2 x 1370 DINOv2 tokens)
    dict(M=4096, N=136, K=1152),                                  # final layer
    *[dict(M=257, N=384, K=K) for K in (4, 20, 24, 28, 68)],      # K % 16 in {4, 8, 12}, K = 4
    dict(M=1, N=1, K=4),
    dict(M=129, N=129, K=16),
    dict(M=210, N=288, K=96, rpb=70),                             # rows_per_batch not a multiple of the 128-row tile
    dict(M=300, N=200, K=132, act=2, scale=0.37),                 # erf-GELU with out_scale
]


def _restate_linear(A, W, b, act=0, scale=1.0):
    y = F.linear(A.cpu(), W.cpu(), b.cpu())
    y = F.gelu(y, approximate="tanh") if act == 1 else F.gelu(y) if act == 2 else F.silu(y) if act == "silu" else y
    return y * np.float32(scale)


def _hold_with_tails(got, rest, exact, bound, M, N, tile, entry, case, margin=cr.RMS_MARGIN):
    rb, rr = cr.check_bound(got, exact, bound, f"{entry} {case}"), cr.rms_ratio(got, rest, exact)
    _note(entry, case, rb, rr)
    tails = []
    if M % tile and M > tile:
        tails.append(("last row tile", (slice(M - M % tile, M), slice(None))))
    if N % tile and N > tile:
        tails.append(("last column tile", (slice(None), slice(N - N % tile, N))))
    worst = rr
    for name, sl in tails:
        t = cr.rms_ratio(got[sl], rest[sl], exact[sl])
        _note(entry, f"{case} {name}", float((((got[sl].double() - exact[sl]).abs()) / bound[sl]).max()), t)
        worst = max(worst, t)
    assert worst <= margin, f"{entry} {case}: rms error {worst:.3g} x the fp32 restatement's (margin {margin:.2f})"
    return rb, worst


@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_gemm_f32_contract(ops, case):
    M, N, K = case["M"], case["N"], case["K"]
    act, scale, rpb = case.get("act", 0), case.get("scale", 1.0), case.get("rpb")
    A, W, b, g = cr.gemm_inputs(M + N + K, M, N, K, DEV)
    name = f"{M}x{N}x{K}" + (f" gated rpb={rpb}" if rpb else f" act={act} scale={scale}")
    margin = cr.RMS_MARGIN * cr.chain_factor(A, W, b)            # the kernel is a serial chain of K fused multiply-adds
    print(f"fp32-contract-margin | gemm_f32 | {name} | {margin:.2f}")
    if rpb:
        nb = (M + rpb - 1) // rpb
        wide = torch.randn(nb, 9 * N, device=DEV, generator=g)                     # the adaLN row: gate = chunk 2 of 9
        gate = wide[:, 2 * N:3 * N]
        x0 = torch.randn(M, N, device=DEV, generator=g)
        rows = torch.arange(M, device=DEV) // rpb
        exact, bound = cr.gemm_f32_ref(A, W, b, gate_rows=gate[rows], x0=x0)
        x = x0.clone()
        ops.gemm_f32(A, W, b, out=x, gate=gate, rows_per_batch=rpb)
        rest = x0.cpu() + gate[rows].cpu() * F.linear(A.cpu(), W.cpu(), b.cpu())
        _hold_with_tails(x, rest.to(DEV), exact, bound, M, N, 128, "gemm_f32", name, margin)
    else:
        exact, bound = cr.gemm_f32_ref(A, W, b, act, scale)
        got = ops.gemm_f32(A, W, b, act=act, out_scale=scale)
        _hold_with_tails(got, _restate_linear(A, W, b, act, scale).to(DEV), exact, bound, M, N, 128, "gemm_f32", name, margin)
        if act == 0 and M <= 300:                                                    # no bias; both GELUs at the ragged shapes
            for a2, s2 in ((1, 1.0), (2, 0.37), (0, 0.25)):
                exact, bound = cr.gemm_f32_ref(A, W, None, a2, s2)
                got = ops.gemm_f32(A, W, None, act=a2, out_scale=s2)
                rb = cr.check_bound(got, exact, bound, f"gemm_f32 {name} no bias act={a2}")
                _note("gemm_f32", f"{M}x{N}x{K} no bias act={a2} scale={s2}", rb)


# ------------------------------------------------------------------------------------------------ attention_f32
def _attn_rows(Nq):
    return sorted(set(range(0, Nq, 32)) | {0, 31, 32, 127, 128, Nq - 1})


def _attn_hold(ops, q, k, v, scale, rows=None, pool=None, what=""):
    """Launch on the full q; reference, bound and restatement on `rows` (all when None)."""
    B, Nq, H, dh = q.shape
    got = ops.attention_f32(q, k, v, scale)
    assert got.shape == (B, Nq, H, dh) and got.is_contiguous()
    s = dh ** -0.5 if scale is None else scale
    if rows is not None:
        idx = torch.tensor(rows, device=DEV)
        q, got = q[:, idx], got[:, idx]
    exact, bound = cr.attn_f32_bound(q, k, v, s)
    rest = cr.unheads(cr.attn_f32_restate(cr.heads_of(q), cr.heads_of(k), cr.heads_of(v), s), B, H).to(DEV)
    rb = cr.check_bound(got, exact, bound, f"attention_f32 {what}")
    if pool is not None:
        pool.add(got, rest, exact)
        return rb, None
    rr = cr.rms_ratio(got, rest, exact)
    _note("attention_f32", what, rb, rr)
    assert rr <= cr.RMS_MARGIN, f"attention_f32 {what}: rms error {rr:.3g} x the fp32 restatement's"
    return rb, rr


@pytest.mark.parametrize("sigma", [0.5, 4.0, 16.0])
@pytest.mark.parametrize("Nk", [2048, 1370])
def test_attention_f32_contract_shipped(ops, Nk, sigma):
    """(B, N, H, dh) = (2, 2048, 16, 72): self-attention on the unbind views of a fused qkv buffer, cross-attention on 1370 keys."""
    B, N, H, dh = 2, 2048, 16, 72
    if Nk == N:
        g = torch.Generator(device=DEV).manual_seed(int(sigma * 10))
        qkv = torch.randn(B, N, 3, H, dh, device=DEV, generator=g)
        qkv[:, :, 0] *= sigma
        q, k, v = qkv.unbind(2)
    else:
        q, k, v = cr.qkv_inputs(int(sigma * 10) + 1, B, N, Nk, H, dh, sigma, DEV)
    _attn_hold(ops, q, k, v, None, rows=_attn_rows(N), what=f"{N}x{Nk} H={H} dh={dh} sigma={sigma}")


@pytest.mark.parametrize("dh", [1, 31, 32, 33, 64, 72, 96, 97, 128])
def test_attention_f32_contract_small_shapes(ops, dh):
    """Every (Nq, Nk) of the ragged grid in full, logit spreads 0.5 / 4 / 16 in turn, default and explicit scale."""
    pool, worst, i = _Pool(), 0.0, 0
    for Nq in (1, 33, 127, 129, 300):
        for Nk in (1, 31, 32, 33, 45, 333):
            sigma = (0.5, 4.0, 16.0)[i % 3]
            scale = None if i % 2 == 0 else 1.3 * dh ** -0.5
            i += 1
            q, k, v = cr.qkv_inputs(Nq * 1000 + Nk + dh, 1, Nq, Nk, 2, dh, sigma, DEV)
            rb, _ = _attn_hold(ops, q, k, v, scale, pool=pool, what=f"{Nq}x{Nk} dh={dh} sigma={sigma}")
            worst = max(worst, rb)
    _note("attention_f32", f"small shapes dh={dh} (30 shapes pooled)", worst, pool.ratio())
    assert pool.ratio() <= cr.RMS_MARGIN, f"attention_f32 dh={dh}: pooled rms error {pool.ratio():.3g} x the restatement's"


def test_attention_f32_contract_rescale_and_strides(ops):
    """The spike (a late key dwarfs the running max: everything earlier is rescaled) and the ramp (the max rises tile after
    tile); q, k, v with three different batch / token / head strides; the refusals."""
    B, N, H, dh = 1, 512, 1, 72
    q, k, v = cr.qkv_inputs(23, B, N, N, H, dh, 1.0, DEV)
    k[0, 300, 0] = q[0, 17, 0] * 6.0
    k[0, 500, 0] = q[0, 200, 0] * 9.0
    _attn_hold(ops, q, k, v, None, what="spike")
    N, H = 1024, 2
    q, k, v = cr.qkv_inputs(25, B, N, N, H, dh, 0.3, DEV)
    q[..., 0] = 4.0
    k[0, :, :, 0] = ((torch.arange(N, device=DEV) // 64).float() * 3.0 / (4.0 * dh ** -0.5))[:, None]
    _attn_hold(ops, q, k, v, None, what="ramp")
    B, Nq, Nk, H, dh = 3, 130, 77, 4, 72
    g = torch.Generator(device=DEV).manual_seed(27)
    q = torch.randn(B, H, Nq, dh, device=DEV, generator=g).permute(0, 2, 1, 3)                # [B, H, M, dh] viewed as BMHK
    k = torch.randn(1, Nk, H, dh, device=DEV, generator=g).expand(B, Nk, H, dh)               # batch stride 0
    v = torch.randn(B, Nk, H, dh + 8, device=DEV, generator=g)[..., :dh]                      # head stride dh + 8
    assert len({q.stride()[:3], k.stride()[:3], v.stride()[:3]}) == 3 and k.stride(0) == 0
    for scale in (None, 1.0 / dh):
        _attn_hold(ops, q, k, v, scale, what=f"strided views scale={scale}")
    bad = torch.randn(1, 8, 1, 129, device=DEV)
    with pytest.raises(RuntimeError, match="dh <= 128"):
        ops.attention_f32(bad, bad, bad)
    wide = torch.randn(1, 8, 1, 64, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous last dim"):
        ops.attention_f32(wide[..., ::2], wide[..., :32], wide[..., :32])


# ------------------------------------------------------------------------------------------------ layernorm_modulate_f32
@pytest.mark.parametrize("D", [4, 63, 64, 65, 70, 384, 1152, 2048])
def test_layernorm_modulate_f32_contract(ops, D):
    for spread, offset in cr.LN_BANDS:
        pool, worst = _Pool(), 0.0
        for rows in (1, 5, 4096):
            for rpb in (1, 37, 2048):
                nb = (rows + rpb - 1) // rpb
                x, mod = cr.ln_inputs(D + rows + rpb, rows, D, spread, offset, nb, DEV)
                shift, scale = mod[:, :D], mod[:, 2 * D:]                             # column slices: row stride 3 D
                r = torch.arange(rows, device=DEV) // rpb
                exact, bound = cr.layernorm_modulate_f32_ref(x, shift[r], scale[r], 1e-6)
                got = ops.layernorm_modulate_f32(x, shift, scale, rpb, 1e-6)
                rest = cr.ln_f32_restate(x.cpu().numpy(), shift[r].cpu().numpy(), scale[r].cpu().numpy(), 1e-6)
                worst = max(worst, cr.check_bound(got, exact, bound, f"layernorm_modulate_f32 D={D} rows={rows} rpb={rpb} ({spread}, {offset})"))
                pool.add(got, rest, exact)
        _note("layernorm_modulate_f32", f"D={D} (spread, offset)=({spread}, {offset}) rows 1/5/4096 x rpb 1/37/2048", worst, pool.ratio())
        assert pool.ratio() <= cr.RMS_MARGIN, f"layernorm_modulate_f32 D={D} ({spread}, {offset}): rms {pool.ratio():.3g} x the restatement's"


def test_layernorm_modulate_f32_refuses_wide_rows(ops):
    x = torch.zeros(2, 2049, device=DEV)
    with pytest.raises(RuntimeError, match="D <= 2048"):
        ops.layernorm_modulate_f32(x, x[:1], x[:1], 2)


# ------------------------------------------------------------------------------------------------ silu_f32
def test_silu_f32_contract(ops):
    """3 M values (2048 blocks x 256 threads: the grid-stride loop runs six times) over [-100, 100], and the special values as
    torch's fp32 F.silu gives them on the CPU: -0 below -88.72, x itself where exp(-x) underflows, NaN -> NaN, +inf -> +inf and
    -inf -> NaN (-inf / (1 + inf))."""
    g = torch.Generator(device=DEV).manual_seed(31)
    n = 3 * (1 << 20)
    x = (torch.rand(n, device=DEV, generator=g) * 2 - 1) * 100.0
    x[::7] = torch.randn(x[::7].shape, device=DEV, generator=g) * 3.0
    edge = torch.tensor([-88.7, -88.72, -88.7228, -88.72284, -88.73, -103.0, 88.8, 0.0, -0.0, 1e-30, -1e-30], device=DEV)
    x[-edge.numel():] = edge                                                         # (the tail of the last grid-stride pass)
    got = ops.silu_f32(x)
    exact, bound = cr.silu_f32_ref(x)
    rb = cr.check_bound(got, exact, bound, "silu_f32")
    _note("silu_f32", "3 M values in [-100, 100]", rb)
    low = x < -88.73
    assert int(low.sum()) > 1000 and bool((got[low] == 0).all()) and bool(torch.signbit(got[low]).all())     # -0, not +0
    assert bool(torch.signbit(got[x == 0]).equal(torch.signbit(x[x == 0])))
    sp = torch.tensor([float("-inf"), float("inf"), float("nan"), -100.0, -89.0, 104.0, 120.0, 3e38, -3e38], device=DEV)
    gs, want = ops.silu_f32(sp).cpu(), F.silu(sp.cpu())
    assert torch.isnan(want[0]) and torch.isnan(want[2]) and want[1] == float("inf")
    assert torch.equal(torch.isnan(gs), torch.isnan(want)) and torch.equal(gs[~torch.isnan(gs)], want[~torch.isnan(want)])
    assert torch.equal(torch.signbit(gs[3:]), torch.signbit(want[3:])) and torch.equal(gs[5:8], sp[5:8].cpu())


# ------------------------------------------------------------------------------------------------ linear_f32
def _linear_case(ops, M, N, K, silu, pool=None, seed=0):
    A, W, b, _ = cr.gemm_inputs(seed + M * 7 + N + K, M, N, K, DEV)
    act = "silu" if silu else 0
    exact, bound = cr.gemm_f32_ref(A, W, b, act)
    got = ops.linear_f32(A, W, b, act_out=int(silu))
    rest = _restate_linear(A, W, b, act).to(DEV)
    name = f"{M}x{N}x{K}" + (" SiLU" if silu else "")
    if pool is not None:
        pool.add(got, rest, exact)
        return cr.check_bound(got, exact, bound, f"linear_f32 {name}"), (A, W, b, got)
    margin = cr.RMS_MARGIN * cr.chain_factor(A, W, b)            # (the tiled kernel: a serial fmaf chain over K)
    print(f"fp32-contract-margin | linear_f32 | {name} | {margin:.2f}")
    _hold_with_tails(got, rest, exact, bound, M, N, 64, "linear_f32", name, margin)
    return None, (A, W, b, got)


@pytest.mark.parametrize("M,N,K", [(4096, 1152, 68), (2738, 768, 588), (4096, 1152, 52)])
def test_linear_f32_contract_tiled(ops, M, N, K):
    """x-embedder (with the second destination of forward_with_cfg), ViT patch embedding (K = 588), PointEmbed (51 features
    padded to 52)."""
    for silu in (False, True):
        _, (A, W, b, got) = _linear_case(ops, M, N, K, silu)
    two = torch.full((2 * M + 1, N), 7.0, device=DEV)
    ops.linear_f32(A, W, b, act_out=1, out=two[:M], out2=two[M:2 * M])
    assert torch.equal(two[:M], got) and torch.equal(two[M:2 * M], got) and bool((two[2 * M] == 7.0).all())


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("N,K", [(1152, 256), (1152, 1152), (70, 12), (333, 260), (7, 588)])
def test_linear_f32_contract_few_rows(ops, N, K, silu):
    """M = 1..8 (one wave per column; K % 256 ragged tails, N % 4 != 0) and M = 9 (the tiled kernel) on the same operands; for
    M <= 8 a row's bits do not depend on how many rows ride along (DiT.plan_timesteps relies on it)."""
    pool, worst = _Pool(), 0.0
    A, W, b, _ = cr.gemm_inputs(N + K, 9, N, K, DEV)
    act = "silu" if silu else 0
    exact, bound = cr.gemm_f32_ref(A, W, b, act)
    rest = _restate_linear(A, W, b, act).to(DEV)
    full = ops.linear_f32(A[:8].contiguous(), W, b, act_out=int(silu))
    for M in range(1, 9):
        got = ops.linear_f32(A[:M].contiguous(), W, b, act_out=int(silu))
        worst = max(worst, cr.check_bound(got, exact[:M], bound[:M], f"linear_f32 M={M} {N}x{K} silu={silu}"))
        pool.add(got, rest[:M], exact[:M])
        assert torch.equal(got, full[:M]), f"linear_f32 M={M} {N}x{K}: a row's bits depend on the rows that ride along"
    _note("linear_f32", f"M=1..8 N={N} K={K}" + (" SiLU" if silu else ""), worst, pool.ratio())
    assert pool.ratio() <= cr.RMS_MARGIN, f"linear_f32 M<=8 {N}x{K}: rms {pool.ratio():.3g} x the restatement's"
    got9 = ops.linear_f32(A, W, b, act_out=int(silu))
    rb, rr = cr.check_bound(got9, exact, bound, f"linear_f32 M=9 {N}x{K}"), cr.rms_ratio(got9, rest, exact)
    _note("linear_f32", f"M=9 N={N} K={K}" + (" SiLU" if silu else ""), rb, rr)
    margin = cr.RMS_MARGIN * cr.chain_factor(A, W, b)            # (M = 9 is the tiled kernel: a serial fmaf chain over K)
    assert rr <= margin, f"linear_f32 M=9 {N}x{K}: rms {rr:.3g} x the restatement's (margin {margin:.2f})"


@pytest.mark.parametrize("N", [1, 63, 65, 66])
def test_linear_f32_contract_ragged_columns(ops, N):
    """N % 4 != 0 (scalar epilogue) next to the following multiple of 4 (16-byte stores), on the tiled kernel (M = 70) and the
    wave-per-column kernel (M = 3), SiLU epilogue; the four launches pooled for the rms criterion."""
    pool, worst = _Pool(), 0.0
    for M in (70, 3):
        for n in (N, (N + 3) // 4 * 4):
            rb, _ = _linear_case(ops, M, n, 68, True, pool=pool, seed=N)
            worst = max(worst, rb)
    _note("linear_f32", f"N={N} and {(N + 3) // 4 * 4}, M=70 / 3, K=68 SiLU", worst, pool.ratio())
    assert pool.ratio() <= cr.RMS_MARGIN


def test_linear_f32_refuses_misaligned_views(ops):
    """Both kernels read `in` and W with 16-byte loads and the tiled kernel stores 16 bytes when N % 4 == 0: a contiguous view
    that starts off a 16-byte boundary is an argument error before any launch (no misaligned pointer is ever launched)."""
    M, N, K = 16, 64, 32
    flat = torch.zeros(M * K + N * K + M * N + 8, device=DEV)
    x, W = flat[:M * K].view(M, K), flat[M * K:M * K + N * K].view(N, K)
    x1 = flat[1:1 + M * K].view(M, K)
    W1 = flat[M * K + 2:M * K + 2 + N * K].view(N, K)
    assert x1.is_contiguous() and x1.data_ptr() % 16 == 4 and W1.data_ptr() % 16 == 8
    for a, w, rows in ((x1, W, M), (x, W1, M), (x1[:4], W, 4), (x[:4], W1, 4)):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            ops.linear_f32(a[:rows], w, None)
    o1 = flat[M * K + N * K + 1:M * K + N * K + 1 + M * N].view(M, N)
    assert o1.is_contiguous() and o1.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.linear_f32(x, W, None, out=o1)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.linear_f32(x, W, None, out2=o1)
    ops.linear_f32(x[:4], W, None, out=o1[:4])                                       # few rows: scalar stores, any fp32 alignment
    ops.linear_f32(x, W[:63], None, out=flat[M * K + N * K + 1:M * K + N * K + 1 + M * 63].view(M, 63))   # N % 4 != 0: scalar stores
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ sin / cos kernels
@pytest.mark.parametrize("dim", [256, 2, 6, 1152])
def test_timestep_embedding_contract(ops, dim):
    """All 1000 timesteps: [cos | sin] of the ONE fp32 product t * freqs, within SINCOS_ULPS ulp of the fp32 result."""
    t = torch.arange(1000, device=DEV)
    got = ops.timestep_embedding(t, dim)
    exact, bound = cr.timestep_embedding_ref(t, ops._freq_table(dim, 10000.0, t.device))
    _note("timestep_embedding", f"t = 0..999 dim={dim} (bound = {cr.SINCOS_ULPS:g} ulp)", cr.check_bound(got, exact, bound, f"timestep_embedding dim={dim}"))


def _points(T, C, wide, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = (torch.rand(T, wide, device=DEV, generator=g) * 2 - 1) * 4.0
    buf[0, 1:4] = torch.tensor([4.0, -4.0, 0.0], device=DEV)
    return buf[:, :C]                                                                 # row stride `wide` > C channels


@pytest.mark.parametrize("F_", [1, 8])
@pytest.mark.parametrize("T", [1, 4096, 32768])
def test_point_features_contract(ops, T, F_):
    """|p| up to 4: arguments up to 2^7 pi 4 = 1.6e3, where a sine without full argument reduction is off by 1e-4; token rows at a
    stride larger than the channel count; pass-through and padding columns bit-exact."""
    x = _points(T, 7, 12, T + F_)
    assert x.stride(0) == 12 or T == 1
    freqs = (torch.pow(2, torch.arange(F_)).float() * math.pi).to(DEV)
    got = ops.point_features(x, freqs)
    exact, bound = cr.point_features_ref(x, freqs)
    assert got.shape == exact.shape and got.shape[1] % 4 == 0
    rb = cr.check_bound(got, exact, bound, f"point_features T={T} F={F_}")
    assert torch.equal(got[:, 6 * F_:6 * F_ + 3], x[:, 1:4]) and bool((got[:, 6 * F_ + 3:] == 0).all())
    _note("point_features", f"T={T} F={F_} row stride 12", rb)


def test_point_embedding_through_the_model(ops):
    """DiTAdditivePosEmb._embed_tokens = x_embedder(x) + PointEmbed(x[:, 1:4]) against float64: the two fp32 Linears' bounds
    (gemm_f32_ref; the feature columns carry their own SINCOS_ULPS ulp through |W|) and the final fp32 addition."""
    import topia_xl_amd as pkg
    T, Cin, Dh = 4096, 68, 288
    torch.manual_seed(5)
    m = pkg.DiTAdditivePosEmb(seq_length=T, in_channels=Cin, condition_channels=64, hidden_size=Dh, depth=1, num_heads=4).eval().to(DEV)
    with torch.no_grad():
        for p in (m.x_embedder.weight, m.x_embedder.bias, m.point_emb.mlp.weight, m.point_emb.mlp.bias):
            p.copy_(torch.randn(p.shape, device=DEV) * 0.2)
    xf = _points(T, Cin, Cin, 9).contiguous()
    out = torch.empty(T, Dh, device=DEV)
    m._embed_tokens(xf, out)
    n = m.point_emb.embedding_dim // 6
    feat, fb = cr.point_features_ref(xf, m.point_emb.basis[0, :n])
    feat, fb = feat[:, :6 * n + 3], fb[:, :6 * n + 3]
    Wp, bp = m.point_emb.mlp.weight.detach(), m.point_emb.mlp.bias.detach()
    e1, b1 = cr.gemm_f32_ref(xf, m.x_embedder.weight.detach(), m.x_embedder.bias.detach())
    e2, b2 = cr.gemm_f32_ref(feat, Wp, bp)                       # (K = 51 here, 52 in the kernel: one more zero term, gamma_53)
    b2 = b2 * (cr.gamma(54) / cr.gamma(52)) + (fb + cr.U32 * fb) @ Wp.double().abs().t() * (1 + cr.gamma(54))
    exact = e1 + e2
    bound = (b1 + b2) * (1 + cr.U32) + cr.U32 * (e1.abs() + e2.abs())
    _note("point_features", f"DiTAdditivePosEmb._embed_tokens T={T}", cr.check_bound(out, exact, bound, "_embed_tokens"))


# ------------------------------------------------------------------------------------------------ vit_tokens, row_stats
@pytest.mark.parametrize("B,n,R,D", [(1, 1369, 4, 768), (2, 1369, 4, 768), (3, 1369, 4, 768), (2, 16, 0, 96), (1, 1, 1, 1)])
def test_vit_tokens_bit_exact(ops, B, n, R, D):
    """One fp32 addition per element: bit-exact against torch.  8192 blocks x 256 threads cover 2.1 M elements: one image
    (1.055 M) is one pass, two and three images run the grid-stride loop."""
    g = torch.Generator(device=DEV).manual_seed(B + n + R)
    patches, cls, pos = (torch.randn(*s, device=DEV, generator=g) for s in ((B, n, D), (D,), (1 + n, D)))
    reg = torch.randn(R, D, device=DEV, generator=g) if R else None
    got = ops.vit_tokens(patches, cls, pos, reg)
    ref = cr.vit_tokens_ref(patches, cls, pos, reg)
    assert got.shape == ref.shape == (B, 1 + R + n, D)
    assert torch.equal(got, ref), f"vit_tokens {B}x{n}x{R}x{D}: {int((got != ref).sum())} elements differ"
    assert (B * (1 + R + n) * D > 8192 * 256) == (B >= 2 and n == 1369)


@pytest.mark.parametrize("D", [4, 128, 132, 1152])
def test_row_stats_contract(ops, D):
    for spread, offset in cr.LN_BANDS:
        worst = 0.0
        for rows in (1, 7, 8, 9, 4096):
            x, _ = cr.ln_inputs(D + rows, rows, D, spread, offset, 1, DEV)
            got = ops.row_stats(x, 1e-6, torch.empty(rows, 2, device=DEV))
            exact, bound = cr.row_stats_ref(x, 1e-6)
            worst = max(worst, cr.check_bound(got, exact, bound, f"row_stats D={D} rows={rows} ({spread}, {offset})"))
        _note("row_stats", f"D={D} (spread, offset)=({spread}, {offset}) rows 1/7/8/9/4096", worst)
