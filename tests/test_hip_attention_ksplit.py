"""The key split of attn_kernel (csrc/attention.hip, KSPLIT = 1: 128 query rows per workgroup, the two wave groups walk the two
halves of the key tiles and merge in LDS) on the GPU: against float64 (cr.attn_bound, ATTN_SLACK as everywhere) at 16, 17 and 22
key tiles, whole and ragged, for the three head dims and both 16-bit types; against the unsplit kernel; at the 15-tile threshold;
across launches that differ only in the broadcast entries riding along; the launch rule; and the row whose second half of the keys
lies far below the first.  tests/test_attention_ksplit_cpu.py proves on the CPU that the check sees the seam between the halves.
Every launch here is a valid one.  B <= 2, H = 2, 128 / 200 / 300 query rows (one, two and three 128-row workgroups per head)."""
import pytest
import torch

from oracle import synth
from tests import contract_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
B, H = 2, 2
NQ = [128, 200, 300]
NKV = [1024, 1025, 1087, 1370]     # 16 tiles; 17 with one key / 63 keys in the last; 22 with 26 keys in the last


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


class mode:
    """primx_attention_ksplit_mode for the span of a `with` (-1 = the rule, 0 = never, 1 = wherever the kernel allows it)."""

    def __init__(self, m):
        self.m = m

    def __enter__(self):
        from topia_xl_amd import _lib
        assert _lib.attn_ksplit_available()
        self.was = _lib.load().primx_attention_ksplit_mode(self.m)

    def __exit__(self, *exc):
        from topia_xl_amd import _lib
        _lib.load().primx_attention_ksplit_mode(self.was)


def _decides(nq, nkv, b_from=B):
    from topia_xl_amd import _lib
    return _lib.load().primx_attention_ksplit(b_from, H, -(-nq // 128) * 128, nkv)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64, 32])
def test_split_against_float64(ops, dh, dtype):
    worst = 0.0
    with mode(1):
        for i, nkv in enumerate(NKV):
            for p, pattern in enumerate(("lookup", "trap")):
                nq = NQ[(i + p) % 3]
                assert _decides(nq, nkv) == 1
                q, k, v = (t.to(dtype) for t in cr.attn_inputs(pattern, 8191 * nq + 5 * nkv + dh, B, nq, nkv, H, dh, DEV))
                got = ops.memory_efficient_attention(q, k, v)
                ratio, _ = cr.attn_check(got, q, k, v, dh ** -0.5, dtype, dh == 72, f"ksplit dh={dh} {pattern} {nq}x{nkv}", bias=False, quiet=True)
                worst = max(worst, ratio)
    print(f"ksplit dh={dh} {dtype}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64, 32])
def test_split_against_unsplit(ops, dh, dtype):
    """Both are inside their own bound around the same exact value, so they differ by at most the sum of the two bounds - and they
    do differ: the split adds fp32 roundings to O, it is not the same bits."""
    for i, nkv in enumerate(NKV):
        nq = NQ[i % 3]
        for pattern in cr.ATTN_PATTERNS:
            q, k, v = (t.to(dtype) for t in cr.attn_inputs(pattern, 8191 * nq + 5 * nkv + dh, B, nq, nkv, H, dh, DEV, 4.0))
            with mode(1):
                a = ops.memory_efficient_attention(q, k, v)
            with mode(0):
                assert _decides(nq, nkv) == 0
                b = ops.memory_efficient_attention(q, k, v)
            out, E = cr.attn_bound(q, k, v, dh ** -0.5, dtype, dh == 72)
            bound = cr.ATTN_SLACK * (0.5 * torch.as_tensor(cr.ulp16(out.cpu().numpy(), dtype), device=DEV) + E)
            d = (a.double() - b.double()).abs()
            assert bool(torch.isfinite(a.float()).all()) and bool((d <= 2 * bound).all()), \
                f"dh={dh} {dtype} {pattern} {nq}x{nkv}: split and unsplit {float((d / bound).max()):.3f} bounds apart"
            if pattern == "random":
                assert not torch.equal(a, b), f"dh={dh} {dtype} {nq}x{nkv}: the split launch gave the unsplit kernel's bits - did it split?"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64])
def test_fifteen_tiles_never_split(ops, dh, dtype):
    nq, nkv = 300, 960
    q, k, v = (t.to(dtype) for t in cr.attn_inputs("random", 77 + dh, B, nq, nkv, H, dh, DEV, 4.0))
    with mode(1):
        assert _decides(nq, nkv) == 0 and _decides(nq, nkv + 1) == 1
        a = ops.memory_efficient_attention(q, k, v)
    with mode(0):
        b = ops.memory_efficient_attention(q, k, v)
    assert torch.equal(a, b)


def _value_row(dtype, dh):
    vrow = synth.tensor(25, "vrow", (1, 1, H, dh)).to(dtype).clone()
    vrow[0, 0, :, 0] = -0.0
    vrow[0, 0, H - 1, dh - 1] = -0.0
    return vrow


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,nkv", [(300, 1370), (200, 1024)])
def test_same_bits_whatever_rides_along(ops, dtype, nq, nkv):
    """The rule (mode -1) counts the entries with keys of their own: the conditional entry of a launch that carries a broadcast
    entry (B = 2, b_from = 1) is the same bits as that entry launched alone (B = b_from = 1), and the broadcast entry's rows are
    the value row, -0 as +0."""
    from topia_xl_amd import _lib
    dh = 72
    q, k, v = (t.to(dtype) for t in cr.attn_inputs("random", 13 * nq + nkv, B, nq, nkv, H, dh, DEV, 4.0))
    krow, vrow = synth.tensor(25, "krow", (1, 1, H, dh)).to(dtype), _value_row(dtype, dh)
    Qp = ops.pack_heads(q, _lib.HEADS_ROWS, ops.BQ, "q")
    nb = ops.bcast_keys(nkv)
    Kb = ops.pack_heads(krow.expand(1, nb, H, dh).contiguous().to(DEV), _lib.HEADS_KROWS, ops.BKV, "k")
    Vb = ops.pack_heads(vrow.expand(1, nb, H, dh).contiguous().to(DEV), _lib.HEADS_VT, ops.BKV)
    Kp, Vt = ops.pack_heads(k[:1].contiguous(), _lib.HEADS_KROWS, ops.BKV, "k"), ops.pack_heads(v[:1].contiguous(), _lib.HEADS_VT, ops.BKV)
    with mode(-1):
        cu = torch.cuda.get_device_properties(0).multi_processor_count
        want = int(2 * 1 * H * -(-Qp.shape[2] // 256) <= cu)
        assert _lib.load().primx_attention_ksplit(1, H, Qp.shape[2], nkv) == want
        both = ops.attention(Qp, Kp, Vt, nq, nkv, dh, dh ** -0.5, bcast=(Kb, Vb)).view(B, nq, H, dh)
        alone = ops.attention(Qp[:1].contiguous(), Kp, Vt, nq, nkv, dh, dh ** -0.5).view(1, nq, H, dh)
    assert bool(torch.isfinite(both.float()).all())
    assert torch.equal(both[:1], alone)
    bits = vrow.view(torch.int16)
    rows = torch.where(bits == -32768, torch.zeros_like(bits), bits).expand(1, nq, H, dh)
    assert torch.equal(both[1:].cpu().contiguous().view(torch.int16), rows)


def test_the_rule(ops):
    from topia_xl_amd import _lib
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the rule's cases are stated for a 256-CU device")
    f = _lib.load().primx_attention_ksplit
    with mode(-1):
        assert f(1, 16, 2048, 1370) == 1 and f(1, 16, 1408, 1370) == 1
        assert f(2, 16, 2048, 2048) == 0 and f(8, 16, 2048, 1370) == 0 and f(1, 16, 2048, 960) == 0
    with mode(0):
        assert f(1, 16, 2048, 1370) == 0
    with mode(1):
        assert f(8, 16, 2048, 1370) == 1 and f(1, 16, 2048, 960) == 0


def test_profile_tags_carry_the_split(ops):
    """ops.PROFILE's tag is the name rocprofv3 prints: at batch 1 the cross-attention launches of the depth-4 model of
    tests/test_hip_null_skip.py carry the split template argument, the self-attention launches do not."""
    from tests import test_hip_null_skip as NS
    import topia_xl_amd as pkg
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the rule's cases are stated for a 256-CU device")
    cfg = dict(in_channels=68, condition_channels=768, hidden_size=1152, depth=NS.DEPTH)
    m = pkg.DiT(seq_length=NS.N, num_heads=NS.HEADS, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    m.load_state_dict(synth.dit_state_dict(NS.SEED, **cfg))
    m.to(DEV)
    x, y = NS._inputs(1)
    ops.PROFILE = tags = []
    try:
        with mode(-1):
            NS._planned_forward(m, x, y, torch.float16)
    finally:
        ops.PROFILE = None
    names = [t[0] for t in tags if t[0].startswith("attn_kernel<")]
    cross = [n for n in names if n.endswith(f"x{NS.N}x{NS.L}x72")]
    self_ = [n for n in names if n.endswith(f"x{NS.N}x{NS.N}x72")]
    assert len(cross) == NS.DEPTH and len(self_) == NS.DEPTH, names
    assert all(n.startswith("attn_kernel<1, 5, 3, 0, 0, 1> ") for n in cross), cross
    assert all(n.startswith("attn_kernel<1, 5, 3, 0, 0, 0> ") for n in self_), self_


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nkv", [1024, 1370])
def test_far_lower_second_half_stays_finite(ops, dtype, nkv):
    """Logits of about -90 nats (-130 in the exp2 domain) in the whole second half of the keys: group 1's first tile has its row
    max below -128, where exp2(-max) is inf in fp32 - the `first` path multiplies nothing by it, and the merge's a_1 is 0."""
    dh, nq = 72, 200
    g = torch.Generator().manual_seed(5 + nkv)
    q, k = 0.3 * torch.randn(B, nq, H, dh, generator=g), 0.3 * torch.randn(B, nkv, H, dh, generator=g)
    v = 1.0 + 0.5 * torch.randn(B, nkv, H, dh, generator=g)
    c = (90.0 * dh ** 0.5) ** 0.5
    half = 64 * ((((nkv + 63) // 64) + 1) // 2)
    q[..., 0] = c
    k[:, :half, :, 0] = 0.0
    k[:, half:, :, 0] = -c
    q, k, v = (t.to(dtype).to(DEV) for t in (q, k, v))
    with mode(1):
        assert _decides(nq, nkv) == 1
        got = ops.memory_efficient_attention(q, k, v)
    assert bool(torch.isfinite(got.float()).all())
    cr.attn_check(got, q, k, v, dh ** -0.5, dtype, True, f"ksplit far-lower half {nq}x{nkv}", bias=False, quiet=True)
