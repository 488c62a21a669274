"""The premise of the null cross-attention skip (DiT.null_xattn_skip): a batch entry whose keys and values are Mk copies of ONE
row gets, from the walking kernel (attn_kernel through primx_attention_bcast), output rows that ARE the value row - bit for
bit, whatever the query - with -0 coming out as +0.  Asserted with torch.equal on the walking kernel, for both 16-bit types,
the three head dims, ragged and whole-tile key counts, and queries scaled so that the running max is large and its 16-bit
split leaves a residual."""
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


def value_row(dtype, H, dh):
    """The value row of test_broadcast_key_value_entries with a few exact -0, +0 and subnormal entries put in."""
    vrow = synth.tensor(25, "vrow", (1, 1, H, dh)).to(dtype).clone()
    tiny = torch.finfo(dtype).smallest_normal
    sub = torch.tensor([tiny / 4, -tiny / 2, tiny / 64], dtype=torch.float32).to(dtype)   # subnormal in both types
    assert bool((sub != 0).all()) and bool((sub.abs() < tiny).all())
    vrow[0, 0, :, 0] = -0.0
    vrow[0, 0, :, 5] = 0.0
    vrow[0, 0, 0, 1:4] = sub
    vrow[0, 0, H - 1, dh - 1] = -0.0
    vrow[0, 0, H - 1, dh - 2] = sub[1]
    return vrow


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("qscale", [1.0, 8.0, 32.0])
@pytest.mark.parametrize("B,b_from,Mq,Mk,H,dh", [(2, 1, 300, 1370, 4, 72), (3, 0, 256, 1370, 2, 72), (2, 1, 200, 64, 2, 72),
                                                 (2, 1, 128, 200, 2, 64), (3, 2, 64, 129, 4, 32)])
def test_broadcast_entries_return_the_value_row_bit_for_bit(ops, dtype, qscale, B, b_from, Mq, Mk, H, dh):
    from topia_xl_amd import _lib
    q = (synth.tensor(25, "q", (B, Mq, H, dh)) * qscale).to(dtype)
    k = synth.tensor(25, "k", (B, Mk, H, dh)).to(dtype)
    v = synth.tensor(25, "v", (B, Mk, H, dh)).to(dtype)
    krow = synth.tensor(25, "krow", (1, 1, H, dh)).to(dtype)
    vrow = value_row(dtype, H, dh)
    assert bool(torch.isfinite(q.float()).all())
    Qp = ops.pack_heads(q.to(DEV), _lib.HEADS_ROWS, ops.BQ, "q")
    nb = ops.bcast_keys(Mk)
    Kb = ops.pack_heads(krow.expand(1, nb, H, dh).contiguous().to(DEV), _lib.HEADS_KROWS, ops.BKV, "k")
    Vb = ops.pack_heads(vrow.expand(1, nb, H, dh).contiguous().to(DEV), _lib.HEADS_VT, ops.BKV)
    Kp = ops.pack_heads(k[:b_from].to(DEV), _lib.HEADS_KROWS, ops.BKV, "k") if b_from else None
    Vt = ops.pack_heads(v[:b_from].to(DEV), _lib.HEADS_VT, ops.BKV) if b_from else None
    got = ops.attention(Qp, Kp, Vt, Mq, Mk, dh, dh ** -0.5, bcast=(Kb, Vb)).view(B, Mq, H, dh)[b_from:].cpu()
    # -0 -> +0 on the bit pattern (0x8000 is the 16-bit integer -32768 in both types)
    bits = vrow.view(torch.int16)
    want = torch.where(bits == -32768, torch.zeros_like(bits), bits).expand(B - b_from, Mq, H, dh)
    gb = got.contiguous().view(torch.int16)
    if not torch.equal(gb, want):
        bad = gb != want
        diff = (got.double() - vrow.double().expand_as(got)).abs()[bad]
        print(f"{int(bad.sum())} of {bad.numel()} elements differ, largest difference {float(diff.max()):.3e}")
    assert torch.equal(gb, want)
