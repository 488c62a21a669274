"""Helpers for the tests that hold the kernels' ADDRESS arithmetic where a 32-bit index ends (tests/test_hip_extent.py; the
mechanism proves itself on CPU tensors in tests/test_extent_cpu.py).  Importing this module needs no GPU.

Let E = 2^31.  An entry point whose largest 16-bit operand holds e elements per primitive is run once on
P = floor(E / e) + 9 primitives: the smallest batch whose operand passes E elements (2^32 bytes), plus a few primitives, so
that an access whose index wrapped lands in primitives 0 .. 8, whose data differ from the ones it should have met.  The
result is compared in FULL with the results of the same entry point on slices of at most CHUNK = 2048 primitives (a size the
contract tests already hold) and at four probe primitives against float64.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple, Union

import torch

E = 1 << 31
CHUNK = 2048
SLAB_BYTES = 256 << 20        # fp32 bytes of one generation / comparison slab: no second full-size temporary exists

Tensors = Union[torch.Tensor, Sequence[torch.Tensor]]


def primitives_past(e: int) -> int:
    """The test size for an operand of e elements per primitive: floor(E / e) + 9."""
    return E // e + 9


def reaches(numel: int, itemsize: int, what: str = "operand") -> int:
    """Assert (in arithmetic on the caller's own sizes) that an operand of `numel` elements passes 2^31 elements; returns its
    size in bytes."""
    assert numel > E, f"{what}: {numel} elements do not pass 2^31 - the test would not reach what it is there for"
    return numel * itemsize


def probe_primitives(P: int, e: int, itemsize: int) -> List[int]:
    """Primitive 0, the primitive holding byte offset 2^31, the primitive holding element 2^31 (byte 2^32 of a 16-bit
    operand) and P - 1, of an operand with e elements of `itemsize` bytes per primitive (sorted, duplicates dropped,
    primitives past the end left out)."""
    want = [0, E // (e * itemsize), E // e, P - 1]
    return sorted({p for p in want if 0 <= p < P})


def _rows_per_slab(shape: Sequence[int], slab_bytes: int = SLAB_BYTES) -> int:
    per = 1
    for s in shape[1:]:
        per *= s
    return max(1, slab_bytes // (4 * per))


def randn_slabs(shape: Sequence[int], dtype: torch.dtype, device, seed: int, scale: float = 1.0, offset: float = 0.0,
                slab_bytes: int = SLAB_BYTES) -> torch.Tensor:
    """offset + scale * N(0, 1) of `shape` in `dtype`, drawn on `device` from a seeded generator slab by slab along the first
    dimension: every primitive gets its own data, and the only temporary is one fp32 slab."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = torch.empty(tuple(shape), dtype=dtype, device=device)
    step = _rows_per_slab(shape, slab_bytes)
    for lo in range(0, shape[0], step):
        hi = min(shape[0], lo + step)
        t = torch.randn((hi - lo,) + tuple(shape[1:]), device=device, generator=g)
        if scale != 1.0:
            t.mul_(scale)
        if offset != 0.0:
            t.add_(offset)
        out[lo:hi].copy_(t)
        del t
    return out


def _as_list(x: Tensors) -> List[torch.Tensor]:
    return [x] if isinstance(x, torch.Tensor) else list(x)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes as integers of its element size (NaN payloads and signed zeros compare as bits)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def assert_chunks_equal(big_out: Tensors, run_chunk: Callable[[int, int], Tensors], P: int, chunk: int = CHUNK,
                        rel_l2: Optional[float] = None, what: str = "") -> float:
    """Compare EVERY element of `big_out` (a tensor, or several, with P entries along the first dimension) with what
    `run_chunk(lo, hi)` returns for the primitives [lo, hi) - the same entry point on slices of at most `chunk` primitives -
    on the tensors' own device, slice by slice.

    rel_l2 is None (the default): bit identity; the failure names the first differing primitive and its element count.
    rel_l2 = tol: the relative L2 distance over all elements (sums kept in float64) must stay below tol - only for routes
    whose big and chunked calls launch different kernels.  Returns the measured distance (0.0 under bit identity)."""
    assert 0 < chunk <= CHUNK, "chunks are held to a size the contract tests already cover"
    bigs = _as_list(big_out)
    for b in bigs:
        assert b.shape[0] == P, (what, tuple(b.shape), P)
    num = [0.0] * len(bigs)
    den = [0.0] * len(bigs)
    for lo in range(0, P, chunk):
        hi = min(P, lo + chunk)
        smalls = _as_list(run_chunk(lo, hi))
        assert len(smalls) == len(bigs), (what, len(smalls), len(bigs))
        for k, (b, s) in enumerate(zip(bigs, smalls)):
            part = b[lo:hi]
            assert part.shape == s.shape and part.dtype == s.dtype, (what, k, tuple(part.shape), tuple(s.shape), part.dtype, s.dtype)
            if rel_l2 is None:
                pb, sb = bits(part), bits(s)
                if not torch.equal(pb, sb):
                    bad = (pb != sb).reshape(hi - lo, -1).sum(1)
                    first = int(bad.nonzero()[0])
                    raise AssertionError(
                        f"{what}: output {k} of the call on {P} primitives differs from the call on primitives [{lo}, {hi}): first at "
                        f"primitive {lo + first} ({int(bad[first])} of {pb[0].numel()} elements), {int((bad > 0).sum())} primitives of "
                        f"this slice, {int(bad.sum())} elements")
            else:
                d = part.double() - s.double()
                num[k] += float((d * d).sum())
                den[k] += float((s.double() ** 2).sum())
                assert num[k] == num[k], f"{what}: output {k} holds NaN in primitives [{lo}, {hi})"
        del smalls
    if rel_l2 is None:
        return 0.0
    worst = max((n / (d + 1e-300)) ** 0.5 for n, d in zip(num, den))
    assert worst < rel_l2, f"{what}: rel-L2 {worst:.3e} between the call on {P} primitives and the chunked calls (tolerance {rel_l2:g})"
    return worst


def tile_blocks(rows: int, row_bytes: int, tile: int) -> Tuple[List[Tuple[int, int]], List[Tuple[int, int]]]:
    """Row (or column) blocks [lo, hi) of a GEMM operand with `rows` rows of `row_bytes` bytes, cut into tiles of `tile` rows:
    (probe blocks, the rest).  Probe blocks: the first tile, the tile holding byte offset 2^31, the last full tile and every
    tile from byte offset 2^32 - 2 MiB to the end (the ragged last one included); merged where they touch."""
    n_tiles = (rows + tile - 1) // tile
    pick = {0, (E // row_bytes) // tile, rows // tile - 1}
    first_late = max(0, ((1 << 32) - (2 << 20)) // row_bytes // tile)
    pick |= set(range(first_late, n_tiles))
    pick = sorted(t for t in pick if 0 <= t < n_tiles)
    probes: List[Tuple[int, int]] = []
    for t in pick:
        lo, hi = t * tile, min(rows, (t + 1) * tile)
        if probes and probes[-1][1] == lo:
            probes[-1] = (probes[-1][0], hi)
        else:
            probes.append((lo, hi))
    rest, at = [], 0
    for lo, hi in probes:
        if lo > at:
            rest.append((at, lo))
        at = hi
    if at < rows:
        rest.append((at, rows))
    return probes, rest
