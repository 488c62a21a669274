"""tests/extent.py proves itself without a GPU: a stand-in "kernel" on CPU tensors whose flat store index is reduced the way a
32-bit register would reduce it - at a small limit L in place of 2^31 - must fail assert_chunks_equal for each kind of wrap,
and the correct stand-in must pass; the probe primitives and the GEMM ring-guard shapes of tests/test_hip_extent.py hold as
literals."""
import pytest
import torch

from tests import extent as ex

L = 1 << 12                     # the stand-in's "2^31": an element index of this size no longer fits its (model) int
e, ITEM = 64, 2                 # elements per primitive, bytes per element
P = L // e + 9                  # the rule of extent.primitives_past at the small limit
SMALL = 16                      # chunk size: 16 * 64 elements, far below every wrap


def _signed(v, limit):
    """v as a two's-complement integer of log2(2 * limit) bits: [limit, 2 limit) maps to [-limit, 0)."""
    return (v + limit) % (2 * limit) - limit


INDEX = {
    "correct": lambda i: i,
    # an `int` element index: negative from element L on
    "int element index": lambda i: _signed(i, L),
    # an `unsigned` byte offset of log2(2 L) bits: byte 2 L is byte 0 again, i.e. element i lands at element i - L
    "unsigned byte offset": lambda i: (i * ITEM) % (2 * L) // ITEM,
    # a signed byte offset of the same width: negative from byte L, i.e. from element L / 2, on
    "signed byte offset": lambda i: torch.div(_signed(i * ITEM, L), ITEM, rounding_mode="floor"),
}


def _standin(x: torch.Tensor, index) -> torch.Tensor:
    """out[p, j] = 2 x[p, j] + 1, written through the flat index `index(i)`.  An element no store reached keeps the 0xFF
    fill of a guarded torch.empty (NaN); a store in front of the buffer is dropped (on the device the guard reports it)."""
    flat = x.reshape(-1)
    n = flat.numel()
    out = torch.full((n,), float("nan"), dtype=x.dtype)
    i = torch.arange(n)
    j = index(i)
    ok = (j >= 0) & (j < n)
    vals = (2.0 * flat.float() + 1.0).to(x.dtype)
    for lo in range(0, n, L):                       # in index order, as a grid walks it: a later store wins (j is unique within L indices)
        sel = ok[lo:lo + L]
        out[j[lo:lo + L][sel]] = vals[lo:lo + L][sel]
    return out.view(x.shape)


@pytest.fixture(scope="module")
def x():
    t = ex.randn_slabs((P, e), torch.float16, "cpu", 3, slab_bytes=4 * e * 7)      # slabs of 7 primitives: a ragged last slab
    assert len({tuple(r.tolist()) for r in t}) == P                                # every primitive has its own data
    return t


def _check(x, kind, **kw):
    big = _standin(x, INDEX[kind])
    return ex.assert_chunks_equal(big, lambda lo, hi: _standin(x[lo:hi], INDEX[kind]), P, SMALL, what=kind, **kw)


def test_correct_standin_passes(x):
    assert _check(x, "correct") == 0.0
    assert _check(x, "correct", rel_l2=1e-6) == 0.0


@pytest.mark.parametrize("kind,first_bad,fill_from", [("int element index", L // e, L // e), ("unsigned byte offset", 0, L // e),
                                                      ("signed byte offset", 0, L // 2 // e)])
def test_each_wrap_fails_the_chunk_comparison(x, kind, first_bad, fill_from):
    """A store whose index went negative lands in front of the buffer; one that came round to 0 again lands in primitives
    0 .. 8 (the byte offsets pass 2 L there: P is 9 primitives past the limit).  Either way the primitives the stores should
    have reached keep the fill, and the chunked calls, which never reach the limit, differ at both ends."""
    with pytest.raises(AssertionError, match="differs from the call on primitives") as err:
        _check(x, kind)
    assert f"first at primitive {first_bad} " in str(err.value)
    big = _standin(x, INDEX[kind])
    assert bool(torch.isnan(big[fill_from:L // e]).all()) and (kind == "signed byte offset" or bool(torch.isnan(big[L // e:]).all()))
    if first_bad == 0:
        assert torch.equal(big[:9], _standin(x[L // e:], INDEX["correct"]))           # primitives 64 .. 72 written over 0 .. 8
    with pytest.raises(AssertionError):                                            # the tolerance form sees it too (NaN or distance)
        _check(x, kind, rel_l2=2e-4)


def test_a_wrapped_read_fails_too(x):
    """A gather through a wrapped index reads primitive p - L / e: finite, plausible, wrong - only per-primitive data show it."""
    def gather(t, wrap):
        flat = t.reshape(-1)
        i = torch.arange(flat.numel())
        return (2.0 * flat[i % L if wrap else i].float() + 1.0).to(t.dtype).view(t.shape)
    big = gather(x, True)
    assert bool(torch.isfinite(big).all())
    with pytest.raises(AssertionError, match=f"first at primitive {L // e} "):
        ex.assert_chunks_equal(big, lambda lo, hi: gather(x[lo:hi], True), P, SMALL, what="wrapped read")


def test_several_outputs_and_shape_checks(x):
    big = (_standin(x, INDEX["correct"]), x.float().sum(1))
    run = lambda lo, hi: (_standin(x[lo:hi], INDEX["correct"]), x[lo:hi].float().sum(1))
    ex.assert_chunks_equal(big, run, P, SMALL)
    with pytest.raises(AssertionError):
        ex.assert_chunks_equal(big, lambda lo, hi: run(lo, hi)[:1], P, SMALL)
    with pytest.raises(AssertionError):
        ex.assert_chunks_equal(big, run, P, ex.CHUNK + 1)                          # chunks stay at a size the contract tests hold


def test_probe_primitives_by_hand():
    assert ex.E == 2147483648 and ex.CHUNK == 2048
    # e = 131072 ([512, 256]): 2^31 / 131072 = 16384 primitives hold 2^31 elements; byte 2^31 is the first byte of primitive 8192
    assert ex.primitives_past(131072) == 16393
    assert ex.probe_primitives(16393, 131072, 2) == [0, 8192, 16384, 16392]
    # e = 16384 ([64, 256], [512, 32])
    assert ex.primitives_past(16384) == 131081
    assert ex.probe_primitives(131081, 16384, 2) == [0, 65536, 131072, 131080]
    # e = 3072 ([512, 6]): 2^31 / 3072 = 699050.67, 2^31 / 6144 = 349525.33; the fp32 output passes byte 2^31 at 174762.67
    assert ex.primitives_past(3072) == 699059
    assert ex.probe_primitives(699059, 3072, 2) == [0, 349525, 699050, 699058]
    assert ex.probe_primitives(699059, 3072, 4) == [0, 174762, 699050, 699058]
    # e = 1728 ([27, 64])
    assert ex.primitives_past(1728) == 1242756 + 9 and 1242756 * 1728 <= ex.E < 1242757 * 1728
    # the shipped decode chunk: exactly 2^31 elements, 2^32 bytes - the probe at element 2^31 is past its end
    assert 16384 * 512 * 256 == ex.E and ex.probe_primitives(16384, 131072, 2) == [0, 8192, 16383]
    assert ex.reaches(16393 * 131072, 2) == 4297326592
    with pytest.raises(AssertionError):
        ex.reaches(16384 * 131072, 2)


def test_gemm_ring_guard_shapes_as_literals():
    """The guard of csrc/gemm.hip kt64_ring is M K < 2^31 and N K < 2^31, at K = 1152."""
    K = 1152
    assert 1863936 * K == 2147254272 < ex.E <= 2147549184 == 1864192 * K
    assert 1863936 == 7281 * 256 and 1864192 == 7282 * 256                         # M side: whole 256-row tiles
    assert 1863936 * K * 2 == 4294508544 < 1 << 32                                 # byte offsets of the last legal shape
    assert 1863936 == 6472 * 288 and 1864224 == 6473 * 288                         # N side: whole 288-column tiles
    assert 1863936 * K < ex.E <= 1864224 * K == 2147586048
    # heads: whole batch entries of 2048 rows
    assert 910 * 2048 == 1863680 and 1863680 * K == 2146959360 < ex.E
    assert 911 * 2048 == 1865728 and 1865728 * K == 2149318656 >= ex.E
    assert 16 * 72 == K and K % 288 == 0 and 288 % 72 == 0


def test_tile_blocks():
    probes, rest = ex.tile_blocks(1863936, 2304, 256)
    # byte 2^31 lies in row 932067 = tile 3640; 2^32 - 2 MiB in row 1863224 = tile 7278 of 7281
    assert probes == [(0, 256), (3640 * 256, 3641 * 256), (7278 * 256, 1863936)]
    assert rest == [(256, 3640 * 256), (3641 * 256, 7278 * 256)]
    assert sum(hi - lo for lo, hi in probes + rest) == 1863936
    probes, rest = ex.tile_blocks(1000, 2304, 256)                                 # a small ragged operand: first and last full tile
    assert probes == [(0, 256), (512, 768)] and rest == [(256, 512), (768, 1000)]
