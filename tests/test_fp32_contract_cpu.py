"""The fp32 contract of tests/contract_ref.py, proved on the CPU (no GPU): numpy / torch fp32 restatements of the fp32 kernels
(csrc/fp32.hip, the fp32 front end of csrc/rowops.hip) stay inside the rigorous per-element bounds at every kind of case
tests/test_hip_fp32_contract.py runs (at reduced size), and the same restatements with ONE fault injected fail their check.
The first shows a bound is not too tight for a correct fp32 evaluation; the second that it is tight enough to matter."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import contract_ref as cr

CPU = "cpu"


def _fails(fn) -> bool:
    try:
        fn()
    except AssertionError:
        return True
    return False


def _act32(y, act):
    if act == 1:
        return F.gelu(y, approximate="tanh")
    if act == 2:
        return F.gelu(y)
    if act == "silu":
        return F.silu(y)
    return y


def _gemm_restate(A, W, b, act=0, out_scale=1.0, gate_rows=None, x0=None, kdrop=0):
    """fp32 on the CPU: A W^T + b, the epilogue in the kernel's order.  kdrop: the injected fault (the last columns of K dropped)."""
    K = A.shape[1] - kdrop
    y = A[:, :K] @ W[:, :K].t() + b
    if gate_rows is not None:
        return x0 + gate_rows * y
    return _act32(y, act) * np.float32(out_scale)


GEMM_CPU = [(300, 200, 132), (257, 384, 4), (257, 384, 20), (257, 384, 24), (257, 384, 28), (257, 384, 68), (1, 1, 4),
            (129, 129, 16), (2, 1000, 1152), (70, 136, 1152)]


@pytest.mark.parametrize("M,N,K", GEMM_CPU)
def test_gemm_bounds_hold_for_fp32(M, N, K):
    A, W, b, g = cr.gemm_inputs(M + N + K, M, N, K, CPU)
    worst = 0.0
    for act, s in ((0, 1.0), (1, 1.0), (2, 0.37), ("silu", 1.0)):
        exact, bound = cr.gemm_f32_ref(A, W, b, act, s)
        worst = max(worst, cr.check_bound(_gemm_restate(A, W, b, act, s), exact, bound, f"gemm {M}x{N}x{K} act={act}"))
    rpb = max(1, (M + 2) // 3)
    gate = torch.randn((M + rpb - 1) // rpb, 3 * N, generator=g)[:, N:2 * N]
    x0 = torch.randn(M, N, generator=g)
    gr = gate[torch.arange(M) // rpb]
    exact, bound = cr.gemm_f32_ref(A, W, b, gate_rows=gr, x0=x0)
    worst = max(worst, cr.check_bound(_gemm_restate(A, W, b, gate_rows=gr, x0=x0), exact, bound, f"gemm {M}x{N}x{K} gated"))
    print(f"gemm {M}x{N}x{K}: fp32 restatement max |err| / bound = {worst:.3f}")


def test_gemm_faults_fail():
    M, N, K, rpb = 210, 136, 20, 70
    A, W, b, g = cr.gemm_inputs(7, M, N, K, CPU)
    exact, bound = cr.gemm_f32_ref(A, W, b)
    good = _gemm_restate(A, W, b)
    cr.hold_fp32(good, good, exact, bound, "clean")
    assert _fails(lambda: cr.hold_fp32(_gemm_restate(A, W, b, kdrop=K % 16), good, exact, bound))      # the last K % 16 columns
    gate = torch.randn(3, N, generator=g)
    x0 = torch.randn(M, N, generator=g)
    rows = torch.arange(M)
    gr = gate[rows // rpb]
    exact, bound = cr.gemm_f32_ref(A, W, b, gate_rows=gr, x0=x0)
    good = _gemm_restate(A, W, b, gate_rows=gr, x0=x0)
    cr.hold_fp32(good, good, exact, bound, "clean gated")
    bad = _gemm_restate(A, W, b, gate_rows=gate[rows // 128 * 128 // rpb], x0=x0)                        # the tile's first row's gate
    assert _fails(lambda: cr.hold_fp32(bad, good, exact, bound))
    # a fault in ONE element of a ragged tail must not be averaged away: one output moved by 1e-4 of its size
    one = good.clone()
    one[M - 1, N - 1] *= 1.0 + 1e-4
    assert _fails(lambda: cr.hold_fp32(one, good, exact, bound))


ATTN_CPU = [(100, 333, 72), (70, 300, 72), (64, 45, 64), (33, 70, 128), (40, 1, 32), (50, 333, 33)]


def _attn_case(Nq, Nk, dh, sigma, B=1, H=2):
    q, k, v = cr.qkv_inputs(Nq + Nk + dh + int(10 * sigma), B, Nq, Nk, H, dh, sigma, CPU)
    exact, bound = cr.attn_f32_bound(q, k, v, dh ** -0.5)
    return q, k, v, exact, bound


def _restate(q, k, v, scale, **kw):
    B, _, H, _ = q.shape
    return cr.unheads(cr.attn_f32_restate(cr.heads_of(q), cr.heads_of(k), cr.heads_of(v), scale, **kw), B, H)


@pytest.mark.parametrize("sigma", [0.5, 4.0, 16.0])
@pytest.mark.parametrize("Nq,Nk,dh", ATTN_CPU)
def test_attention_bound_holds_for_fp32(Nq, Nk, dh, sigma):
    q, k, v, exact, bound = _attn_case(Nq, Nk, dh, sigma)
    r = cr.check_bound(_restate(q, k, v, dh ** -0.5), exact, bound, f"attention {Nq}x{Nk}x{dh} sigma={sigma}")
    print(f"attention {Nq}x{Nk}x{dh} sigma={sigma}: fp32 restatement max |err| / bound = {r:.3f}")


@pytest.mark.parametrize("sigma", [0.5, 4.0])
def test_attention_faults_fail(sigma):
    Nq, Nk, dh = 70, 173, 72                                  # 173 keys: the last tile holds 13
    q, k, v, _, _ = _attn_case(Nq, Nk, dh, sigma)
    k[:, 150] = 6.0 * q[:, 3]                                 # a late spike: the running max of query 3 jumps in tile 4
    s = dh ** -0.5
    exact, bound = cr.attn_f32_bound(q, k, v, s)
    good = _restate(q, k, v, s)
    cr.hold_fp32(good, good, exact, bound, "clean")
    for fault, kw in (("drop_last_key", {}), ("tail_zero", {}), ("skip_rescale", dict(fault_tile=4)), ("copy_row", {})):
        bad = _restate(q, k, v, s, fault=fault, **kw)
        assert _fails(lambda: cr.hold_fp32(bad, good, exact, bound)), fault


LN_CPU_D = [4, 63, 70, 384, 1152, 2048]


def _ln_case(D, spread, offset, rows=9, rpb=4):
    nb = (rows + rpb - 1) // rpb
    x, mod = cr.ln_inputs(D + int(spread), rows, D, spread, offset, nb, CPU)
    shift, scale = mod[:, :D], mod[:, 2 * D:]
    r = torch.arange(rows) // rpb
    return x, shift, scale, r


@pytest.mark.parametrize("spread,offset", cr.LN_BANDS)
@pytest.mark.parametrize("D", LN_CPU_D)
def test_layernorm_bounds_hold_for_fp32(D, spread, offset):
    x, shift, scale, r = _ln_case(D, spread, offset)
    exact, bound = cr.layernorm_modulate_f32_ref(x, shift[r], scale[r])
    got = cr.ln_f32_restate(x.numpy(), shift[r].numpy(), scale[r].numpy())
    a = cr.check_bound(got, exact, bound, f"layernorm D={D} ({spread}, {offset})")
    # row statistics: (mean, 1 / sqrt(var + eps)) in numpy fp32
    if D % 4 == 0:
        xn = x.numpy()
        mean = xn.sum(-1, keepdims=True, dtype=np.float32) * (np.float32(1.0) / np.float32(D))
        c = xn - mean
        rstd = np.float32(1.0) / np.sqrt((c * c).sum(-1, keepdims=True, dtype=np.float32) * (np.float32(1.0) / np.float32(D)) + np.float32(1e-6))
        se, sb = cr.row_stats_ref(x, 1e-6)
        b = cr.check_bound(np.concatenate([mean, rstd], -1), se, sb, f"row_stats D={D}")
        print(f"row_stats D={D} ({spread}, {offset}): fp32 restatement max |err| / bound = {b:.3f}")
    print(f"layernorm D={D} ({spread}, {offset}): fp32 restatement max |err| / bound = {a:.3f}")


@pytest.mark.parametrize("spread,offset", cr.LN_BANDS)
def test_layernorm_faults_fail(spread, offset):
    D = 70
    x, shift, scale, r = _ln_case(D, spread, offset)
    exact, bound = cr.layernorm_modulate_f32_ref(x, shift[r], scale[r])
    good = cr.ln_f32_restate(x.numpy(), shift[r].numpy(), scale[r].numpy())
    cr.hold_fp32(good, good, exact, bound, "clean")
    bad = cr.ln_f32_restate(x.numpy(), shift[r].numpy(), scale[r].numpy(), pad_mean=True)              # mean over 128 columns
    assert _fails(lambda: cr.hold_fp32(bad, good, exact, bound))
    r1 = torch.arange(x.shape[0]) // 5                                                                # rows_per_batch 5 for 4
    bad = cr.ln_f32_restate(x.numpy(), shift[r1].numpy(), scale[r1].numpy())
    assert _fails(lambda: cr.hold_fp32(bad, good, exact, bound))
    if offset != 0.5:       # a row statistic off by 100 ulp: what the old relative 1e-4 let through
        se, sb = cr.row_stats_ref(x[:, :68], 1e-6)
        off = se.clone()
        off[:, 1] *= 1.0 + 100 * 2.0 ** -23
        if spread == 1.0:   # (where the mean is far from zero the variance cannot be known that well in fp32, and the bound says so)
            assert _fails(lambda: cr.check_bound(off, se, sb))


def test_sincos_bounds_and_fault():
    from topia_xl_amd import ops   # the frequency table is host code
    for dim in (2, 6, 256, 1152):
        t = torch.arange(1000)
        freqs = ops._freq_table(dim, 10000.0, "cpu")
        exact, bound = cr.timestep_embedding_ref(t, freqs)
        arg = t.float()[:, None] * freqs[None]
        got = torch.cat([torch.cos(arg), torch.sin(arg)], -1)
        r = cr.check_bound(got, exact, bound, f"timestep dim={dim}")
        print(f"timestep dim={dim}: fp32 libm max |err| / bound = {r:.3f}")
        bad_arg = arg * (1.0 + 2.0 ** -11)                                                            # an argument kept to 11 bits
        bad = torch.cat([torch.cos(bad_arg), torch.sin(bad_arg)], -1)
        assert _fails(lambda: cr.check_bound(bad, exact, bound))
    g = torch.Generator().manual_seed(3)
    T, Fq = 4096, 8
    x = (torch.rand(T, 7, generator=g) * 2 - 1) * 4.0
    freqs = torch.pow(2.0, torch.arange(Fq)).float() * np.pi
    exact, bound = cr.point_features_ref(x, freqs)
    arg = (x[:, 1:4, None] * freqs[None, None]).reshape(T, 3 * Fq)
    got = torch.cat([arg.sin(), arg.cos(), x[:, 1:4], torch.zeros(T, 1)], -1)
    r = cr.check_bound(got, exact, bound, "point_features")
    print(f"point_features: fp32 libm max |err| / bound = {r:.3f}")
    barg = arg * (1.0 - 2.0 ** -11)
    assert _fails(lambda: cr.check_bound(torch.cat([barg.sin(), barg.cos(), x[:, 1:4], torch.zeros(T, 1)], -1), exact, bound))
    # a fast sine without argument reduction is off by about 2^-24 |arg| (1e-4 at |arg| = 1.6e3): sin(arg (1 + 2^-24))
    farg = arg.double() * (1.0 + 2.0 ** -24)
    assert _fails(lambda: cr.check_bound(torch.cat([farg.sin(), farg.cos(), x[:, 1:4].double(), torch.zeros(T, 1).double()], -1), exact, bound))
    moved = got.clone()
    moved[5, 6 * Fq + 1] = float(np.nextafter(np.float32(moved[5, 6 * Fq + 1]), np.float32(9.0)))             # pass-through: bit-exact
    assert _fails(lambda: cr.check_bound(moved, exact, bound))


def test_silu_bound_and_special_values():
    g = torch.Generator().manual_seed(4)
    x = torch.cat([(torch.rand(1 << 18, generator=g) * 2 - 1) * 100.0, torch.randn(1 << 16, generator=g) * 3,
                   torch.tensor([-88.7, -88.72, -88.7228, -88.72284, -88.73, -103.0, 88.8, 0.0, -0.0, 1e-30, -1e-30])])
    exact, bound = cr.silu_f32_ref(x)
    xn = x.numpy()
    with np.errstate(over="ignore"):
        got = xn / (np.float32(1.0) + np.exp(-xn))
    r = cr.check_bound(got, exact, bound, "silu")
    print(f"silu: numpy fp32 max |err| / bound = {r:.3f}")
    with np.errstate(over="ignore"):
        bad = xn / (np.float32(1.0) + np.exp(-xn) * np.float32(1.0 + 2.0 ** -19))                      # exp off by 32 ulp
    assert _fails(lambda: cr.check_bound(bad, exact, bound))
    # the special values the GPU test asserts, as torch's fp32 F.silu gives them on the CPU
    sp = F.silu(torch.tensor([float("-inf"), float("inf"), float("nan"), -100.0, -0.0, 120.0]))
    assert torch.isnan(sp[0]) and sp[1] == float("inf") and torch.isnan(sp[2])                         # -inf / inf = NaN
    assert sp[3] == 0 and torch.signbit(sp[3]) and sp[4] == 0 and torch.signbit(sp[4]) and sp[5] == 120.0


def test_vit_tokens_reference_and_fault():
    g = torch.Generator().manual_seed(5)
    B, n, R, D = 2, 16, 4, 96
    patches, cls, pos, reg = (torch.randn(*s, generator=g) for s in ((B, n, D), (D,), (1 + n, D), (R, D)))
    ref = cr.vit_tokens_ref(patches, cls, pos, reg)
    assert ref.shape == (B, 1 + R + n, D)
    assert torch.equal(ref[1, 0], cls + pos[0]) and torch.equal(ref[0, 1:1 + R], reg) and torch.equal(ref[1, 1 + R + 3], patches[1, 3] + pos[4])
    assert not torch.equal(cr.vit_tokens_ref(patches, cls, pos, reg, pos_shift=0), ref)
    assert cr.vit_tokens_ref(patches, cls, pos, None).shape == (B, 1 + n, D)
