"""The 16-bit attention check of tests/test_hip_attention_grid.py, proved on the CPU (no GPU).  cr.attn16_restate restates the
algorithm attn_kernel / attn64_kernel document; on a sub-grid of the GPU file's cells - 1 to 8 key tiles, whole and ragged, one
query row to several waves - and under the three input patterns of cr.attn_inputs
  * the unfaulted restatement passes the check the kernels get (cr.attn_bound with ATTN_SLACK, the pooled bias on `random`), so
    the bound is not too tight for a correct evaluation, and
  * the restatement with ONE fault of cr.ATTN_FAULTS fails it under at least one pattern in every cell where the fault changes
    the arithmetic (and is bit-identical to the unfaulted one in every other cell), so the check is tight enough to matter.
The last test pins why the sentinel patterns exist: on dense random inputs alone an unmasked pad key passes."""
import functools

import numpy as np
import pytest
import torch

from tests import contract_ref as cr

CPU = "cpu"
B, H = 2, 2
DTYPES = [torch.float16, torch.bfloat16]
# (nq, nkv): 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5 and 8 key tiles; 33 / 40 / 65 / 129 query rows leave partial waves
CELLS = [(1, 1), (33, 31), (40, 64), (33, 65), (65, 128), (129, 129), (33, 192), (40, 193), (65, 256), (33, 257), (40, 320), (33, 449)]


@functools.lru_cache(maxsize=None)
def _cell(dh, dtype, pattern, nq, nkv):
    """(q, k, v as [B H, M, dh] numpy, (exact, E) of cr.attn_bound) - computed once, shared by the tests below, never modified."""
    sigma = cr.ATTN_SIGMAS[CELLS.index((nq, nkv)) % 3]
    q, k, v = (t.to(dtype) for t in cr.attn_inputs(pattern, 4099 * nq + 7 * nkv + dh, B, nq, nkv, H, dh, CPU, sigma))
    out, E = cr.attn_bound(q, k, v, dh ** -0.5, dtype, dh == 72)
    return tuple(cr.heads_of(t.float()) for t in (q, k, v)), (out.numpy(), E.numpy())


def _run(dh, dtype, pattern, nq, nkv, fault=None):
    """The restatement's output [B, nq, H, dh] and its (ratio, signed errors)."""
    (q, k, v), ref = _cell(dh, dtype, pattern, nq, nkv)
    got = cr.unheads(cr.attn16_restate(q, k, v, dh ** -0.5, dtype, dh == 72, fault=fault), B, H)
    return got, cr.attn_report(got, None, None, None, None, dtype, dh == 72, ref=ref)


def test_cells_cover_the_tile_counts():
    tiles = {(nkv + 63) // 64 for _, nkv in CELLS}
    assert {1, 2, 3, 4, 5, 8} <= tiles
    for t in (1, 2, 3, 4, 5):
        assert any((nkv + 63) // 64 == t and nkv % 64 == 0 for _, nkv in CELLS) and any((nkv + 63) // 64 == t and nkv % 64 for _, nkv in CELLS), t
    assert any(nq == 1 for nq, _ in CELLS) and any(nq > 128 for nq, _ in CELLS) and all(nq == 1 or nq % 32 for nq, _ in CELLS)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64, 32])
def test_unfaulted_restatement_passes(dh, dtype):
    """What the kernels are held to is reachable: the documented algorithm, evaluated in numpy, stays inside it."""
    for pattern in cr.ATTN_PATTERNS:
        worst, pooled = 0.0, []
        for nq, nkv in CELLS:
            _, (ratio, signed) = _run(dh, dtype, pattern, nq, nkv)
            assert ratio <= cr.ATTN_SLACK, f"restatement dh={dh} {dtype} {pattern} {nq}x{nkv}: error {ratio:.3f} x the derived bound"
            worst = max(worst, ratio)
            pooled.append(signed)
        print(f"restatement dh={dh} {dtype} {pattern}: worst |err| / bound = {worst:.3f}")
        if pattern == "random" and dh != 72:
            bias = float(np.mean(np.concatenate(pooled)))
            print(f"restatement dh={dh} {dtype} random: pooled mean signed error {bias:+.4f} ulp")
            assert abs(bias) <= cr.BIAS_LIMIT, f"restatement dh={dh} {dtype}: biased by {bias:.3f} ulp"


@pytest.mark.parametrize("dtype", DTYPES)
def test_unfaulted_restatement_passes_at_64_tokens(dtype):
    """attn64_kernel is the one-tile case of the overwrite path (exact row max, P to nearest, the denominator from the unrounded
    P): the same restatement at nq, nkv <= 64, dh = 32."""
    dh, n64 = 32, (1, 17, 33, 48, 64)
    for pattern in cr.ATTN_PATTERNS:
        worst = 0.0
        for i, (nq, nkv) in enumerate((a, b) for a in n64 for b in n64):
            q, k, v = (t.to(dtype) for t in cr.attn_inputs(pattern, 4099 * nq + 7 * nkv + dh, B, nq, nkv, H, dh, CPU, cr.ATTN_SIGMAS[i % 3]))
            got = cr.unheads(cr.attn16_restate(*(cr.heads_of(t.float()) for t in (q, k, v)), dh ** -0.5, dtype, False), B, H)
            ratio, _ = cr.attn_report(got, q, k, v, dh ** -0.5, dtype, False)
            assert ratio <= cr.ATTN_SLACK, f"restatement 64-token {dtype} {pattern} {nq}x{nkv}: error {ratio:.3f} x the derived bound"
            worst = max(worst, ratio)
        print(f"restatement 64-token {dtype} {pattern}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64, 32])
def test_every_fault_fails_wherever_it_changes_the_arithmetic(dh, dtype):
    same_p = dh == 72
    for fault, text in cr.ATTN_FAULTS.items():
        caught = {p: 0 for p in cr.ATTN_PATTERNS}
        cells = 0
        for nq, nkv in CELLS:
            if not cr.attn_fault_applies(fault, nq, nkv, same_p):
                for pattern in cr.ATTN_PATTERNS:        # the predicate is right: nothing changes here
                    assert np.array_equal(_run(dh, dtype, pattern, nq, nkv, fault)[0].numpy(), _run(dh, dtype, pattern, nq, nkv)[0].numpy(),
                                          equal_nan=True), f"{fault} changes {pattern} {nq}x{nkv} dh={dh}"
                continue
            cells += 1
            hit = [p for p in cr.ATTN_PATTERNS if not _run(dh, dtype, p, nq, nkv, fault)[1][0] <= cr.ATTN_SLACK]   # (a NaN ratio fails)
            assert hit, f"dh={dh} {dtype} {nq}x{nkv}: '{text}' passes under every pattern"
            for p in hit:
                caught[p] += 1
        if not cells:
            assert fault == "denominator_before_mask" and same_p, fault
            continue
        print(f"dh={dh} {dtype} {fault}: failed in all {cells} cells it applies to - " + ", ".join(f"{p} {n}" for p, n in caught.items()))


def test_neither_sentinel_alone_catches_both_mask_faults():
    """lookup sees the dropped key, trap the unmasked pad - and not the other way round at a cell with many keys: both are needed."""
    dh, dtype, nq, nkv = 72, torch.float16, 33, 449
    fails = lambda p, f: not _run(dh, dtype, p, nq, nkv, f)[1][0] <= cr.ATTN_SLACK
    assert fails("lookup", "pad_last_key") and fails("trap", "unmask_first_pad")
    assert not fails("lookup", "unmask_first_pad") and not fails("trap", "pad_last_key")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Bn,Mq,Mk,Hn,dh,sigmas", [(1, 300, 1000, 2, 72, (0.5, 4.0, 16.0)), (1, 200, 700, 2, 64, (4.0, 16.0)),
                                                   (2, 300, 500, 2, 32, (4.0, 16.0))])
def test_random_inputs_alone_miss_the_unmasked_pad(dtype, Bn, Mq, Mk, Hn, dh, sigmas):
    """The finding behind the sentinel patterns, at the shapes of tests/test_hip_contract.py::test_attention_bound: a float64 softmax
    that lets the first pad key through (score 0, zero value), rounded once to 16 bits, PASSES the elementwise bound on the dense
    random inputs - one key of ~1000 has a weight inside the documented approximation error (at dh = 72 for every sigma; at
    dh = 64 / 32 once sigma >= 4, where a logit of 0 has no weight next to logits of +-16)."""
    for sigma in sigmas:
        q, k, v = (t.to(dtype) for t in cr.qkv_inputs(int(sigma * 10) + dh, Bn, Mq, Mk, Hn, dh, sigma, CPU))
        qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
        S = qd @ kd.transpose(-1, -2) * cr.f32(dh ** -0.5)
        w = torch.softmax(torch.cat([S, torch.zeros_like(S[..., :1])], -1), -1)[..., :Mk]      # the pad key takes its share
        bad = torch.from_numpy(cr.round16((w @ vd).permute(0, 2, 1, 3), dtype))
        ratio, _ = cr.attn_report(bad, q, k, v, dh ** -0.5, dtype, dh == 72)
        print(f"unmasked pad on random inputs dh={dh} {dtype} sigma={sigma}: |err| / bound = {ratio:.3f}")
        assert ratio <= cr.ATTN_SLACK
