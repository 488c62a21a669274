"""The key split of attn_kernel (csrc/attention.hip, KSPLIT = 1), restated in numpy and proved on the CPU (no GPU).  A split
workgroup's two wave groups walk the key tiles [0, h) and [h, ntiles), h = ceil(ntiles / 2), each with the walk cr.attn16_restate
restates - a first tile that takes the `first` path, a running max of its own, fp32 O and row sum - and group 0 merges the two:
m = max(m0, m1), a_g = exp2(m_g - m) (exp2((m_g - m) c) where the scores are raw), O = O0 a0 + O1 a1, likewise the row sum.
  * the split restatement passes the check the kernels get (cr.attn_bound with ATTN_SLACK) at 16, 17 and 22 key tiles - 1024 keys,
    1025 keys (group 1's last tile holds ONE key) and 1370 keys - under the patterns random (sigma = 4), lookup and trap;
  * the unsplit restatement passes on the same inputs, so the inputs are fair;
  * the split restatement that drops the tile on either side of the seam (h - 1 or h) fails `lookup`: the check sees the seam."""
import functools

import numpy as np
import pytest
import torch

from tests import contract_ref as cr

CPU = "cpu"
B, H = 1, 2
DTYPES = [torch.float16, torch.bfloat16]
NKV = [1024, 1025, 1370]          # 16, 17 and 22 key tiles
NQ = [128, 40]
PATTERNS = [("random", 4.0), ("lookup", 1.0), ("trap", 1.0)]


def ksplit_restate(q, k, v, scale, dtype, same_p, drop=None):
    """q [G, Mq, dh], k, v [G, nkv, dh] of 16-bit values -> [G, Mq, dh] float64 of 16-bit values: the walk of cr.attn16_restate over
    each half of the tiles, then the merge.  drop: a global tile index that its group skips (the seam test)."""
    f4 = np.float32
    q, k, v = (np.ascontiguousarray(t, dtype=f4) for t in (q, k, v))
    G, Mq, dh = q.shape
    nkv = k.shape[1]
    c = f4(f4(scale) * f4(1.4426950408889634))
    nt = (nkv + 63) // 64
    h = (nt + 1) // 2
    Kp, Vp = np.zeros((G, 64 * nt, dh), f4), np.zeros((G, 64 * nt, dh), f4)
    Kp[:, :nkv], Vp[:, :nkv] = k, v
    key = np.arange(64 * nt)
    ones = (key < nkv).astype(f4)
    maskcol = np.where(key < nkv, 0.0, cr.round16(-30000.0, dtype)).astype(f4)

    def wave_any(t):
        a = np.pad(t, ((0, 0), (0, (-Mq) % 32))).reshape(G, -1, 32).any(-1)
        return np.repeat(a, 32, axis=1)[:, :Mq]

    def walk(t0, t1):
        O, l = np.zeros((G, Mq, dh), f4), np.zeros((G, Mq), f4)
        if same_p:
            qs = cr.round16(q * c, dtype).astype(f4)
            m_run, mh, ml = np.zeros((G, Mq), f4), np.zeros((G, Mq)), np.zeros((G, Mq))
        else:
            m_run = np.full((G, Mq), -1e30, f4)
        first = True
        for t in range(t0, t1):
            if t == drop:
                continue
            Kt, Vt = Kp[:, 64 * t:64 * t + 64], Vp[:, 64 * t:64 * t + 64]
            if same_p:
                s = (np.matmul(qs.astype(np.float64), Kt.transpose(0, 2, 1).astype(np.float64)) + maskcol[64 * t:64 * t + 64]
                     + mh[..., None] + ml[..., None]).astype(f4)
                mx = s.max(-1)
                trig = np.ones_like(mx, bool) if first else wave_any(mx > 8.0)
                delta = np.where(trig, mx if first else np.maximum(mx, 0), 0).astype(f4)
                if not first:                                                  # the first tile of a group multiplies nothing
                    alpha = np.exp2(-delta)
                    O, l = O * alpha[..., None], l * alpha
                m_run = m_run + delta
                mh = cr.round16(-m_run, dtype)
                ml = cr.round16(-m_run.astype(np.float64) - mh, dtype)
                P = cr.trunc16(np.exp2(s - delta[..., None]), dtype)
                l = l + np.matmul(P, ones[64 * t:64 * t + 64])
                O = O + np.matmul(P, Vt)
            else:
                raw = np.matmul(q, Kt.transpose(0, 2, 1))
                s = np.where(key[64 * t:64 * t + 64] >= nkv, f4(-1e30), raw)
                mx = s.max(-1)
                trig = wave_any((mx - m_run) * c > 8.0)
                m_new = np.where(trig, np.maximum(m_run, mx), m_run)
                alpha = np.exp2((m_run - m_new) * c)
                l, O = l * alpha, O * alpha[..., None]
                m_run = m_new
                mc = (m_run * c)[..., None]
                P = np.exp2(s * c - mc)
                l = l + P.sum(-1, dtype=f4)
                O = O + np.matmul(cr.round16(P, dtype).astype(f4), Vt)
            first = False
        return O, l, m_run

    with np.errstate(under="ignore", over="ignore", invalid="ignore", divide="ignore"):
        (O0, l0, m0), (O1, l1, m1) = walk(0, h), walk(h, nt)
        m = np.maximum(m0, m1)
        a0 = np.exp2(m0 - m if same_p else (m0 - m) * c).astype(f4)
        a1 = np.exp2(m1 - m if same_p else (m1 - m) * c).astype(f4)
        assert (a0 <= 1).all() and (a1 <= 1).all()
        O = O0 * a0[..., None] + O1 * a1[..., None]
        l = l0 * a0 + l1 * a1
        out = O * (f4(1.0) / l)[..., None]
    return cr.round16(out, dtype)


@functools.lru_cache(maxsize=None)
def _cell(dh, dtype, pattern, sigma, nq, nkv):
    """(q, k, v as [B H, M, dh] numpy, (exact, E) of cr.attn_bound): computed once, shared, never modified."""
    q, k, v = (t.to(dtype) for t in cr.attn_inputs(pattern, 8191 * nq + 5 * nkv + dh, B, nq, nkv, H, dh, CPU, sigma))
    out, E = cr.attn_bound(q, k, v, dh ** -0.5, dtype, dh == 72)
    return tuple(cr.heads_of(t.float()) for t in (q, k, v)), (out.numpy(), E.numpy())


def _ratio(got, dtype, dh, ref):
    return cr.attn_report(cr.unheads(got, B, H), None, None, None, None, dtype, dh == 72, ref=ref)[0]


def test_the_cells_are_16_17_and_22_tiles():
    assert [(n + 63) // 64 for n in NKV] == [16, 17, 22]
    assert 1025 - 64 * 16 == 1                      # group 1's last tile holds one key
    assert [((n + 63) // 64 + 1) // 2 for n in NKV] == [8, 9, 11]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64])
@pytest.mark.parametrize("nkv", NKV)
def test_split_restatement_passes(dh, dtype, nkv):
    """The split walk and its merge stay inside the bound the kernels are held to - and so does the unsplit walk on the same
    inputs."""
    for pattern, sigma in PATTERNS:
        for nq in NQ:
            (q, k, v), ref = _cell(dh, dtype, pattern, sigma, nq, nkv)
            split = _ratio(ksplit_restate(q, k, v, dh ** -0.5, dtype, dh == 72), dtype, dh, ref)
            whole = _ratio(cr.attn16_restate(q, k, v, dh ** -0.5, dtype, dh == 72), dtype, dh, ref)
            print(f"ksplit restatement dh={dh} {dtype} {pattern} {nq}x{nkv}: split {split:.3f}, unsplit {whole:.3f} x the bound")
            assert whole <= cr.ATTN_SLACK, f"unsplit restatement dh={dh} {dtype} {pattern} {nq}x{nkv}: {whole:.3f} x the bound"
            assert split <= cr.ATTN_SLACK, f"split restatement dh={dh} {dtype} {pattern} {nq}x{nkv}: {split:.3f} x the bound"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [72, 64])
@pytest.mark.parametrize("nkv", NKV)
def test_a_dropped_seam_tile_fails_lookup(dh, dtype, nkv):
    """Query i looks up key nkv - 1 - i: with 128 queries the looked-up keys lie in the last two tiles only, so the seam is probed
    with the 128 queries that look up the keys around it."""
    nt = (nkv + 63) // 64
    h = (nt + 1) // 2
    nq = 128
    g = torch.Generator().manual_seed(977 * nkv + dh)
    k = torch.randn(B, nkv, H, dh, generator=g)
    k = k * (dh ** 0.5 / k.norm(dim=-1, keepdim=True))
    v = torch.randn(B, nkv, H, dh, generator=g)
    q = 3.0 * k[:, 64 * h - 64 + torch.arange(nq)]               # the keys of tiles h - 1 and h, one query each
    q, k, v = (t.to(dtype) for t in (q, k, v))
    out, E = cr.attn_bound(q, k, v, dh ** -0.5, dtype, dh == 72)
    ref = (out.numpy(), E.numpy())
    q, k, v = (cr.heads_of(t.float()) for t in (q, k, v))
    assert _ratio(ksplit_restate(q, k, v, dh ** -0.5, dtype, dh == 72), dtype, dh, ref) <= cr.ATTN_SLACK
    for drop in (h - 1, h):
        ratio = _ratio(ksplit_restate(q, k, v, dh ** -0.5, dtype, dh == 72, drop=drop), dtype, dh, ref)
        print(f"ksplit restatement dh={dh} {dtype} lookup 128x{nkv} without tile {drop}: {ratio:.1f} x the bound")
        assert ratio > cr.ATTN_SLACK, f"dropping tile {drop} of {nt} went unnoticed ({ratio:.3f} x the bound)"
