"""attn_kernel, attn64_kernel and the broadcast entries of primx_attention_bcast, element by element against float64
(cr.attn_bound, ATTN_SLACK as everywhere) at EVERY key-tile count from 1 to 8, whole and ragged by one key, and at every query
count around the 32-row wave, the 128-row operand pad and the 256-row workgroup - under dense random inputs and under the two
sentinel patterns of cr.attn_inputs, with which each single key decides the result (lookup: a dropped, swapped or misplaced key
or tile; trap: any pad key that reaches the softmax).  tests/test_attention_grid_cpu.py proves on the CPU that this check fails
for nine kinds of fault in the documented algorithm, and that random inputs alone let one of them through.
B = 2, H = 2: batch and head offsets into padded operands are part of every cell."""
import numpy as np
import pytest
import torch

from tests import contract_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
B, H = 2, 2

# key counts: tile counts 1 .. 8 (449 keys take eight 64-key tiles), whole and ragged by +-1, and the 32-key half tile
NKV = sorted({1, 31, 32, 33, 63} | {64 * t + d for t in range(1, 8) for d in (-1, 0, 1)})
# query counts: the 32-row wave, the 128-row QPAD and the 256-row workgroup, each +-1 (waves without a valid row still take
# part in every barrier); 300 = a second workgroup with a ragged first wave group
NQ = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 300]
CELLS = [(NQ[(i + s) % len(NQ)], nkv) for i, nkv in enumerate(NKV) for s in (0, 4, 8)]   # three query counts per key count
# attn64_kernel: the full cross (16-key MFMA steps and the 32-key half-wave split, each +-1)
N64 = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


def test_cells_cover_every_tile_count_and_query_class():
    tiles = lambda n: (n + 63) // 64
    for t in range(1, 8):
        assert any(tiles(n) == t and n % 64 == 0 for n in NKV), f"{t} whole tiles"
        assert any(tiles(n) == t and n % 64 == 63 for n in NKV) and any(tiles(n) == t and n % 64 == 1 for n in NKV), f"{t} tiles, ragged"
    assert max(tiles(n) for n in NKV) == 8 and {31, 32, 33} <= set(NKV)
    assert {nkv for _, nkv in CELLS} == set(NKV) and {nq for nq, _ in CELLS} == set(NQ)
    for w in (32, 128, 256):
        assert {w - 1, w, w + 1} <= set(NQ)
    assert min(NQ) == 1 and max(NQ) > 256 + 32
    for nkv in NKV:                                       # every key count meets a partial wave and more than one wave
        nqs = [nq for nq, n in CELLS if n == nkv]
        assert len(nqs) == 3 and any(nq % 32 for nq in nqs) and any(nq > 32 for nq in nqs)
    assert len(N64) == 13 and {1, 64} <= set(N64) and all({w - 1, w, w + 1} <= set(N64) for w in (16, 32, 48))


def _hold_cells(cells, run, Bn, Hn, dh, dtype, pattern, same_p, what):
    """Every cell through cr.attn_check (the bound, per cell); the bias criterion once over the pooled `random` cells of the
    paths where it is asserted today (P rounded to nearest)."""
    worst, pooled, bad = 0.0, [], []
    for i, (nq, nkv) in enumerate(cells):
        q, k, v = (t.to(dtype) for t in cr.attn_inputs(pattern, 4099 * nq + 7 * nkv + dh, Bn, nq, nkv, Hn, dh, DEV, cr.ATTN_SIGMAS[i % 3]))
        try:
            ratio, signed = cr.attn_check(run(q, k, v, nq, nkv), q, k, v, dh ** -0.5, dtype, same_p, f"{what} {pattern} {nq}x{nkv}",
                                          bias=False, quiet=True)
        except AssertionError as e:
            bad.append(str(e))
            continue
        worst = max(worst, ratio)
        pooled.append(signed)
    print(f"{what} {dtype} {pattern}: worst |err| / bound over {len(cells)} cells = {worst:.3f}")
    assert not bad, f"{len(bad)} of {len(cells)} cells: " + "; ".join(bad)
    if pattern == "random" and not same_p:
        bias = float(np.mean(np.concatenate(pooled)))
        print(f"{what} {dtype} random: pooled mean signed error {bias:+.4f} ulp")
        assert abs(bias) <= cr.BIAS_LIMIT, f"{what} {dtype}: biased by {bias:.3f} ulp over the pooled random cells"


@pytest.mark.parametrize("pattern", cr.ATTN_PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64, 32])
def test_attention_grid(ops, dh, dtype, pattern):
    """attn_kernel through memory_efficient_attention: the 3-stage ring's prologue (pairs 0 and 1, K(0) parked), its first wrap
    and the clamped tile index past the end at 1 .. 8 key tiles; the key mask in the operands (dh = 72) and in the scores (64, 32)."""
    _hold_cells(CELLS, lambda q, k, v, nq, nkv: ops.memory_efficient_attention(q, k, v), B, H, dh, dtype, pattern, dh == 72, f"attn dh={dh}")


@pytest.mark.parametrize("pattern", cr.ATTN_PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention64_grid(ops, dtype, pattern):
    """attn64_kernel on compact 64-token operands: 21 problems = five workgroups of four and a tail of one."""
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    Bn, Hn, dh = 7, 3, 32

    def run(q, k, v, nq, nkv):
        Qp, Kp, Vt = ops.pack_heads(q, HEADS_ROWS, 64, "q"), ops.pack_heads(k, HEADS_KROWS, 64, "k"), ops.pack_heads(v, HEADS_VT, 64)
        assert Qp.shape[2] == 64 and Kp.shape[2] == 64 and Vt.shape[3] == 64             # the compact form attn64_kernel takes
        return ops.attention(Qp, Kp, Vt, nq, nkv, dh, dh ** -0.5).view(Bn, nq, Hn, dh)

    _hold_cells([(nq, nkv) for nq in N64 for nkv in N64], run, Bn, Hn, dh, dtype, pattern, False, "attn64")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b_from", [0, 1])
@pytest.mark.parametrize("dh", [72, 32])
def test_broadcast_entries_grid(ops, dh, b_from, dtype):
    """primx_attention_bcast at 1 .. 5 key tiles, whole and ragged: BIT-IDENTICAL to primx_attention on the expanded operands, which
    test_attention_grid holds to float64 (the entries in front of b_from look their keys up; the others see one key / value row)."""
    from topia_xl_amd import _lib
    for i, nkv in enumerate([64, 65, 127, 128, 129, 191, 192, 193, 257]):
        nq = (33, 129, 300)[i % 3]
        q, k, v = (t.to(dtype) for t in cr.attn_inputs("lookup", 4099 * nq + 7 * nkv + dh, B, nq, nkv, H, dh, DEV))
        krow, vrow = k[-1:, :1].clone(), v[-1:, :1].clone()
        k[b_from:] = krow                                                          # the expanded form: nkv identical rows
        v[b_from:] = vrow
        Qp = ops.pack_heads(q, _lib.HEADS_ROWS, ops.BQ, "q")
        full = ops.attention(Qp, ops.pack_heads(k, _lib.HEADS_KROWS, ops.BKV, "k"), ops.pack_heads(v, _lib.HEADS_VT, ops.BKV), nq, nkv, dh, dh ** -0.5)
        nb = ops.bcast_keys(nkv)
        Kb = ops.pack_heads(krow.expand(1, nb, H, dh).contiguous(), _lib.HEADS_KROWS, ops.BKV, "k")
        Vb = ops.pack_heads(vrow.expand(1, nb, H, dh).contiguous(), _lib.HEADS_VT, ops.BKV)
        Kp = ops.pack_heads(k[:b_from].contiguous(), _lib.HEADS_KROWS, ops.BKV, "k") if b_from else None
        Vt = ops.pack_heads(v[:b_from].contiguous(), _lib.HEADS_VT, ops.BKV) if b_from else None
        got = ops.attention(Qp, Kp, Vt, nq, nkv, dh, dh ** -0.5, bcast=(Kb, Vb))
        assert torch.equal(got, full), f"broadcast entries differ from the expanded form at {nq}x{nkv} dh={dh} b_from={b_from}"
