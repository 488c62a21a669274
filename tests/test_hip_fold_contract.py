"""The LayerNorm-fold CONSUMERS (primx_linear_heads_fold, primx_linear_heads_fold_pair, primx_linear_fold; include/primx_hip.h "The
LayerNorm fold") held to their rounding contract ulp by ulp, and their center_out to a derived fp32 bound.

Each site runs the real producer (primx_linear_gate_residual_fold) and the real u / v rows (primx_linear_f32out); the consumer's
reference is then built from the tensors it actually read - a16, part, center, u, v - so every check isolates the consumer:
  * the output against tests/contract_ref.py fold_consumer_ref under check_contract (the fold's gain and fp32 statistics through
    fold_contract_kw), a ragged last tile on its own;
  * center_out against fold_stats_ref's bound, and against the float64 statistics of the updated rows x within the bound that adds
    the producer's partial-sum error; `center` untouched; a sentinel row behind center_out untouched;
  * the output against the reference's UNFOLDED arithmetic cast16(cast16(LN(x) m + shift) W^T + b) within fold_site_bound;
  * nothing written outside the output: heads buffers (pads, the query / key-mask columns, the V^T ones row) and a linear output
    that is a view into a sentinel-filled tensor.
Every (kernel, epilogue 7 / 8) pair of the default dispatch is in FOLD_KERNELS and reached.  Regimes: ragged M and batch boundaries
inside a tile, |mu'| / sigma of 0, 2 and 20, constant rows (var = 0, stale centre), row spreads 1e-5 and 3e4 with offsets 1e4,
massive-activation channels, modulation columns with m = cast16(1 + scale) = 0, fp16 outputs across the overflow threshold and in
the subnormal band, bf16 outputs across binades, scale0 on segment 0 only, GELU-tanh and no activation."""
import os
import re

import numpy as np
import pytest
import torch

from tests import contract_ref as cr
from tests.util import unpack_rows, unpack_vt, vt_key_pos

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
EPS = 1e-6
D, H, DH = 1152, 16, 72
S0 = DH ** -0.5
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


def _default_dispatch() -> bool:
    return not any(os.environ.get(v) for v in ("PRIMX_GEMM_LOADER", "PRIMX_GEMM_NOBIG", "PRIMX_GEMM_BIG_MIN",
                                               "PRIMX_GEMM_BIGHEADS_MIN", "PRIMX_GEMM_NOGEMV", "PRIMX_GEMM_PROF", "PRIMX_LIB",
                                               "PRIMX_GEMM_KT32", "PRIMX_GEMM_KT64_MIN", "PRIMX_GEMM_HEADS_KT32"))


def _fold_kernels_selectable(ops) -> bool:
    return ops.fold_shapes_ok(4096, 2048, D, H)


# Every (kernel, epilogue) pair the default dispatch of csrc/gemm.hip launch_fold / primx_linear_heads_fold_pair chooses for a fold
# consumer (epilogue 7 = heads, 8 = linear), and the case that reaches it.  A name outside the table fails the test.
FOLD_KERNELS = {
    "gemm144l_dma_kernel<.,7>": "heads fold, token-major segments, ragged n (to_q / ROWS + KROWS)",
    "gemm144l_dma_kernel<.,8>": "linear fold below the big-tile threshold",
    "gemm288q_dma_kernel<.,7,64>": "heads fold T=4096 qkv (ROWS / KROWS / V^T), to_q T=10240",
    "gemm288q_dma_kernel<.,8,64>": "linear fold (fc1) from 224 tiles, ragged last tile",
    "gemm288q_pair_kernel<.,64>": "qkv + a to_k / to_v rider: problem 0",
}


def _family(name, dtype):
    m = re.fullmatch(r"(\w+)<([^>]*)>", name)
    assert m, name
    args = [a.strip() for a in m.group(2).split(",")]
    assert int(args[0]) == (1 if dtype == F16 else 2), name
    return f"{m.group(1)}<." + "".join("," + a for a in args[1:]) + ">"


def _launched():
    from topia_xl_amd import _lib
    return _lib.load().primx_last_gemm_kernel().decode()


def _np(t):
    return t.detach().double().cpu().numpy()


def _dev_mm(A, B):
    """A @ B^T in float64 on the device (numpy in, numpy out)."""
    return (torch.from_numpy(np.ascontiguousarray(A)).to(DEV) @ torch.from_numpy(np.ascontiguousarray(B)).to(DEV).t()).cpu().numpy()


def _band_weights(g, Nc, dtype, band):
    W = torch.randn(Nc, D, device=DEV, generator=g) * D ** -0.5
    b = torch.randn(Nc, device=DEV, generator=g) * 0.3
    if band == "f16_overflow":
        W, b = W * 52000.0, b * 52000.0
    elif band == "f16_subnormal":
        W, b = W * 2.5e-5, b * 2.5e-5
    elif band == "bf16_binades":        # output columns over 2^-12 .. 2^11
        W = W * torch.pow(2.0, (torch.arange(Nc, device=DEV) % 24 - 12).float())[:, None]
        b = b * 2.0 ** -12
    return W.to(dtype), b.to(dtype)


class Site:
    """One folded LayerNorm site: residual rows x (fp32) with the regime's statistics, the stale (c, rho_p) pairs of the previous
    site, the producer (K = 128, no bias; rows of A that are zero leave their x row as it is), the modulation of the site (shared
    by the batch: entry 0's vectors for every row, as a planned loop passes them) and the u / v rows of the consumer weights."""

    def __init__(self, ops, seed, dtype, B, n, Nc, ratio=0.3, spread=2.0, offset=0.0, const_rows=0, massive=False, neg1_cols=0,
                 band="normal", x=None, center=None):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.dtype, self.B, self.n, self.M, self.Nc = dtype, B, n, B * n, Nc
        M = self.M
        if x is None:
            x = torch.randn(M, D, device=DEV, generator=g) * spread
            if massive:
                x[:, [5, 300, 777, 1100]] += torch.tensor([4e4, -4e4, 3e4, 4e4], device=DEV)
            x = x + offset * torch.sign(torch.randn(M, 1, device=DEV, generator=g))
            const = torch.randperm(M, device=DEV, generator=g)[:const_rows]
            x[const] = (offset + spread * torch.randn(const_rows, 1, device=DEV, generator=g)).expand(-1, D)
            x = x.float()
        else:
            const = torch.zeros(0, dtype=torch.long, device=DEV)
        if center is None:
            xd = x.double()
            sd = xd.std(-1, unbiased=False)
            sgn = torch.sign(torch.randn(M, device=DEV, generator=g, dtype=torch.float64))
            c = xd.mean(-1) + ratio * sd * sgn
            c[const] = c[const] + 0.1 * spread * sgn[const]           # constant rows: the centre a tenth of the spread away
            rp = (1 + 0.1 * torch.randn(M, device=DEV, generator=g, dtype=torch.float64).clamp(-2, 2)) / torch.sqrt(sd ** 2 + EPS)
            center = torch.stack([c, rp], -1).float().contiguous()
        self.center = center
        # producer: the branch increment is small next to the row spread, so the regime survives it
        Kp = 128
        A = torch.randn(M, Kp, device=DEV, generator=g)
        A[const] = 0.0
        Wp = (torch.randn(D, Kp, device=DEV, generator=g) * Kp ** -0.5).to(dtype)
        gate = (torch.randn(B, D, device=DEV, generator=g) * 0.05 * spread).to(dtype)
        scale = torch.randn(1, D, device=DEV, generator=g) * 0.4
        scale[:, torch.randperm(D, device=DEV, generator=g)[:neg1_cols]] = -1.0      # m = cast16(1 + scale) = 0
        self.scale = scale.to(dtype)
        self.shift = (torch.randn(1, D, device=DEV, generator=g) * 0.4).to(dtype)
        self.x = x.clone()
        self.a16 = torch.full((M, D), float("nan"), dtype=dtype, device=DEV)
        self.part = torch.full((M, D // 144, 2), float("nan"), device=DEV)
        ops.linear_gate_residual_fold(A.to(dtype), Wp, None, gate, self.x, n, self.scale.expand(B, -1), self.center, self.a16, self.part)
        assert bool(torch.isfinite(self.a16.float()).all()) and bool(torch.isfinite(self.part).all())
        # consumer weights and the site's fp32 rows u = m W^T, v = shift W^T + b
        self.W, self.b = _band_weights(g, Nc, dtype, band)
        self.m = (1 + self.scale[0]).to(dtype)                                          # (1 + scale) formed in the 16-bit type
        uv = torch.full((2, Nc), float("nan"), device=DEV)
        ops.linear_f32out(torch.stack([self.m, self.shift[0]]), self.W, self.b, uv, 1)
        self.u, self.v = uv[0].clone(), uv[1].clone()
        self.center_copy = self.center.clone()
        self.cbuf = torch.full((M + 1, 2), 12345.0, device=DEV)                        # center_out + a sentinel row past M
        self.center_out = self.cbuf[:M]

    def rows(self, seed):
        """Rows the float64 reference uses: all of them below 4096; from 4096 on every row of the last tile + 512 seeded ones."""
        M = self.M
        if M < 4096:
            return np.arange(M)
        t0 = M - (M % 128 or 128)
        rng = np.random.default_rng(seed)
        return np.union1d(rng.choice(t0, 512, replace=False), np.arange(t0, M))

    def check_center(self, sel, what):
        """center_out: against fold_stats_ref of the partial sums (the consumer's bound) and against float64 statistics of x
        (+ the producer's partial-sum error); `center` and the sentinel row untouched."""
        assert torch.equal(self.center, self.center_copy), f"{what}: the consumer wrote `center`"
        assert bool((self.cbuf[self.M] == 12345.0).all()), f"{what}: center_out written past row M"
        part, cen, x = _np(self.part)[sel], _np(self.center)[sel], _np(self.x)[sel]
        cout = _np(self.center_out)[sel]
        stats = cr.fold_stats_ref(part, cen, D, EPS)
        f1 = cr.check_fold_center(cout, stats, what + " center_out vs its partial sums")
        stats_x = cr.fold_stats_ref(part, cen, D, EPS, part_err=cr.fold_partials_err(x, cen))
        want = np.stack([x.mean(-1), 1.0 / np.sqrt(x.var(-1) + cr.f32(EPS))], -1)
        f2 = cr.check_fold_center(cout, dict(stats_x, center_out=want), what + " center_out vs the statistics of x")
        return stats, stats_x, max(f1, f2)


def _contract(got, site, sel, cols, stats, act, scale0, what, transpose, stats_x):
    """Contract and site bound of the columns `cols` of a consumer output [M, Nc] (rows `sel`); the ragged last 128-row tile on
    its own as well (the contract's criteria 2 and 3 are statistics).  Returns (contract report, site-bound fraction)."""
    dt = site.dtype
    a16 = site.a16[torch.from_numpy(sel).to(DEV)]
    ci = torch.from_numpy(cols).to(DEV)
    Wc = site.W[ci]
    acc = (a16.double() @ Wc.double().t())
    mag = torch.maximum(torch.sqrt(a16.double() ** 2 @ (Wc.double() ** 2).t()), acc.abs()).cpu().numpy()
    acc = acc.cpu().numpy()
    u, v = _np(site.u)[cols], _np(site.v)[cols]
    pre, ref = cr.fold_consumer_ref(acc, stats, u, v, dt, act, scale0)
    kw = cr.fold_contract_kw(acc, mag, stats, u, v, dt, D, act, scale0, rms_axis=0 if transpose else -1)
    t = (lambda a: a.T if np.ndim(a) == 2 else a) if transpose else (lambda a: a)   # column-scaled outputs: the rms per column
    rep = cr.check_contract(t(got), t(pre), t(ref), dt, D, what=what, **{k: t(a) for k, a in kw.items()})
    t0 = site.M - site.M % 128
    tail = sel >= t0
    if site.M % 128 and site.M > 128:
        sl = lambda a: a[tail] if np.ndim(a) == 2 else a
        cr.check_contract(t(got[tail]), t(pre[tail]), t(ref[tail]), dt, D, what=what + " (ragged last tile)",
                          **{k: t(sl(a)) for k, a in kw.items()})
    ref_out, bound, edge = cr.fold_site_bound(_np(site.x)[sel], _np(site.center)[sel], _np(site.m), _np(site.shift[0]), _np(Wc),
                                        _np(site.b[ci]), _np(a16), stats_x, u, v, dt, act, scale0, EPS, mm=_dev_mm)
    frac = cr.check_fold_site(got, ref_out, bound, edge, dt, what + " site bound")
    return rep, frac


def _heads_valid_mask(buf, kind, n, dh):
    from topia_xl_amd._lib import HEADS_VT
    mask = torch.zeros_like(buf, dtype=torch.bool)
    if kind == HEADS_VT:
        pos = torch.tensor([vt_key_pos(k) for k in range(n)], device=buf.device)
        mask[:, :, :dh, pos] = True
    else:
        mask[:, :, :n, :dh] = True
    return mask


SUMMARY = {}


def _note(fam, rep, frac, cfrac):
    s = SUMMARY.setdefault(fam, dict(max_ulp=0.0, differ_over_allowed=0.0, site=0.0, center=0.0))
    s["max_ulp"] = max(s["max_ulp"], rep["max_ulp"])
    s["differ_over_allowed"] = max(s["differ_over_allowed"], rep["differ"] / rep["allowed"])
    s["site"], s["center"] = max(s["site"], frac), max(s["center"], cfrac)


def _run_case(ops, dtype, case, reached, seed):
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    form, B, n = case["form"], case["B"], case["n"]
    band = case.get("band", "normal")
    kinds = [{"q": HEADS_ROWS, "k": HEADS_KROWS, "v": HEADS_VT}[c] for c in case.get("kinds", "qkv")]   # the layouts of Q, K, V^T
    Nc = case.get("Nc", len(kinds) * H * DH if form in ("heads", "pair") else 4608)
    act, scale0 = case.get("act", 0), case.get("scale0", 1.0)
    regime = {k: case[k] for k in ("ratio", "spread", "offset", "const_rows", "massive", "neg1_cols") if k in case}
    site = Site(ops, seed, dtype, B, n, Nc, band=band, x=case.get("x"), center=case.get("center"), **regime)
    what = f"{form} B={B} n={n} {band} {regime}{' chained' if 'x' in case else ''} act={act} scale0={scale0:.3g}"
    M = site.M
    if form in ("heads", "pair"):
        pad = 256 if n % 256 == 0 else 128
        role = {HEADS_ROWS: "q", HEADS_KROWS: "k", HEADS_VT: None}
        dsts = [ops.alloc_heads(B, H, n, DH, k, dtype, DEV, pad, role[k]) for k in kinds]
        snaps = [d.clone() for d in dsts]
        fold = dict(A=site.a16, W=site.W, rows_per_batch=n, heads=H, dh=DH, kinds=kinds, dsts=dsts, n_pad=dsts[0].shape[2], part=site.part,
                    u=site.u, v=site.v, center=site.center, center_out=site.center_out, eps=EPS, scale0=scale0)
        if form == "heads":
            ops.linear_heads_fold(site.a16, site.W, n, H, DH, kinds, dsts, dsts[0].shape[2], site.part, site.u, site.v, site.center,
                                  site.center_out, EPS, scale0=scale0)
            name = _launched()
        else:
            g = torch.Generator(device=DEV).manual_seed(seed + 1)
            Lk, L, Dc = 1536, 1370, 768
            y16 = torch.zeros(Lk, Dc, device=DEV)
            y16[:L] = torch.randn(L, Dc, device=DEV, generator=g)
            y16 = y16.to(dtype)
            Wkv = (torch.randn(2 * D, Dc, device=DEV, generator=g) * Dc ** -0.5).to(dtype)
            bkv = (torch.randn(2 * D, device=DEV, generator=g) * 0.3).to(dtype)
            kv = [ops.alloc_heads(1, H, L, DH, k, dtype, DEV, 256, r) for k, r in ((HEADS_KROWS, "k"), (HEADS_VT, None))]
            ops.linear_heads_fold_pair(fold, y16, Wkv, bkv, Lk, H, DH, [HEADS_KROWS, HEADS_VT], kv, kv[0].shape[2])
            name = _launched()
            # the rider: the plain heads contract (one rounding of y16 Wkv^T + b)
            acc2 = (y16.double() @ Wkv.double().t() + bkv.double()).cpu().numpy()[:L].reshape(L, 2, H * DH)
            for s_, unpack in ((0, unpack_rows), (1, unpack_vt)):
                got2 = _np(unpack(kv[s_], L, DH)).reshape(L, H * DH)
                cr.check_contract(got2, acc2[:, s_], cr.round16(acc2[:, s_], dtype), dtype, Dc, what=f"{what} rider segment {s_}")
        for k, d, s in zip(kinds, dsts, snaps):
            outside = (d != s) & ~_heads_valid_mask(d, k, n, DH)
            assert not bool(outside.any()), f"{what}: kind {k} written outside [tok < n, d < dh] ({int(outside.sum())} elements)"
        got = np.concatenate([_np(unpack_vt(d, n, DH) if k == HEADS_VT else unpack_rows(d, n, DH)).reshape(M, H * DH)
                              for k, d in zip(kinds, dsts)], -1)
        segs = [(np.arange(s_ * H * DH, (s_ + 1) * H * DH), scale0 if s_ == 0 else 1.0) for s_ in range(len(kinds))]
    else:
        big = torch.full(((M + 2) * Nc,), SENTINEL, dtype=dtype, device=DEV)
        out = big[Nc:Nc + M * Nc].view(M, Nc)
        ops.linear_fold(site.a16, site.W, out, site.part, site.u, site.v, site.center, site.center_out, EPS, act=act)
        name = _launched()
        assert bool((big[:Nc] == SENTINEL).all()) and bool((big[Nc + M * Nc:] == SENTINEL).all()), f"{what}: written outside `out`"
        got = _np(out)
        segs = [(np.arange(Nc), 1.0)]
    fam = _family(name, dtype)
    if _default_dispatch():
        assert fam in FOLD_KERNELS, f"{what}: kernel {name} has no row in FOLD_KERNELS"
        if "expect" in case:
            assert fam == case["expect"], (what, name)
    reached.add(fam)
    sel = site.rows(seed)
    stats, stats_x, cfrac = site.check_center(sel, what)
    for s_, (cols, sc) in enumerate(segs):
        rep, frac = _contract(got[sel][:, cols], site, sel, cols, stats, act, sc, f"{what} [{name}] segment {s_}",
                              band == "bf16_binades", stats_x)
        _note(fam, rep, frac, cfrac)
        print(f"{what} [{name}] segment {s_}: {rep}; site bound used {frac:.3f}, center_out bound used {cfrac:.3f}")
    return site


CASES = [
    dict(form="heads", kinds="qk", B=2, n=300, ratio=0.0, scale0=S0, expect="gemm144l_dma_kernel<.,7>"),
    dict(form="heads", kinds="qk", B=3, n=333, ratio=2.0, spread=3e4, offset=1e4, expect="gemm144l_dma_kernel<.,7>"),
    dict(form="heads", kinds="q", B=1, n=1500, ratio=20.0, scale0=S0, expect="gemm144l_dma_kernel<.,7>"),
    dict(form="heads", kinds="qk", B=2, n=1950, massive=True, scale0=S0, expect="gemm144l_dma_kernel<.,7>"),
    dict(form="linear", act=1, B=1, n=333, const_rows=40, expect="gemm144l_dma_kernel<.,8>"),
    dict(form="linear", act=0, B=2, n=300, Nc=1152, spread=1e-5, offset=1e4, neg1_cols=37, expect="gemm144l_dma_kernel<.,8>"),
    dict(form="linear", act=0, B=1, n=1024, Nc=1152, ratio=20.0, expect="gemm144l_dma_kernel<.,8>"),
    dict(form="linear", act=1, B=3, n=1950, ratio=2.0, expect="gemm288q_dma_kernel<.,8,64>"),
    dict(form="linear", act=0, B=3, n=1500, spread=1e-5, neg1_cols=37, const_rows=64, expect="gemm288q_dma_kernel<.,8,64>"),
    dict(form="heads", B=2, n=2048, ratio=2.0, neg1_cols=37, expect="gemm288q_dma_kernel<.,7,64>"),
    dict(form="heads", kinds="q", B=5, n=2048, scale0=S0, ratio=0.0, expect="gemm288q_dma_kernel<.,7,64>"),
    dict(form="pair", B=2, n=2048, massive=True, expect="gemm288q_pair_kernel<.,64>"),
]


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_fold_consumers_meet_their_contract(ops, dtype):
    """Every fold consumer kernel of the default dispatch, in every regime above (normal-range outputs)."""
    if not _fold_kernels_selectable(ops):
        pytest.skip("a kernel-selection switch removes a tile shape of the fold kernels")
    reached = set()
    SUMMARY.clear()
    for i, case in enumerate(CASES):
        _run_case(ops, dtype, case, reached, 700 + i)
    if _default_dispatch():
        missing = sorted(set(FOLD_KERNELS) - reached)
        assert not missing, f"fold kernels of the default dispatch without contract coverage: {missing}"
    for fam, s in sorted(SUMMARY.items()):
        print(f"fold contract {dtype} {fam}: " + ", ".join(f"{k}={v:.3g}" for k, v in s.items()))
    SUMMARY.clear()


@pytest.mark.parametrize("dtype,band", [(F16, "f16_overflow"), (F16, "f16_subnormal"), (BF16, "bf16_binades")])
def test_fold_consumer_value_bands(ops, dtype, band):
    """fp16 outputs across the overflow threshold (inf from 65520 on, not 65504) and in the subnormal band (not flushed), bf16
    outputs across 24 binades - on the 128 x 144 kernel (linear, ragged) and the 256 x 288 heads kernel (scale0 on segment 0)."""
    if not _fold_kernels_selectable(ops):
        pytest.skip("a kernel-selection switch removes a tile shape of the fold kernels")
    reached = set()
    SUMMARY.clear()
    for i, case in enumerate([dict(form="linear", act=0, B=2, n=300, Nc=1152), dict(form="linear", act=1, B=1, n=333),
                              dict(form="heads", B=2, n=2048, scale0=S0)]):
        _run_case(ops, dtype, dict(case, band=band), reached, 800 + i)
    for fam, s in sorted(SUMMARY.items()):
        print(f"fold contract {dtype} {band} {fam}: " + ", ".join(f"{k}={v:.3g}" for k, v in s.items()))
    SUMMARY.clear()


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_fold_two_chained_sites(ops, dtype):
    """Block order: producer -> consumer (qkv, T = 4096) -> producer that centres and scales with THAT consumer's center_out ->
    consumer (fc1 + GELU).  The second consumer meets its contract and the site bound, its center_out its bounds."""
    from topia_xl_amd._lib import ACT_GELU_TANH
    if not _fold_kernels_selectable(ops):
        pytest.skip("a kernel-selection switch removes a tile shape of the fold kernels")
    reached = set()
    SUMMARY.clear()
    first = _run_case(ops, dtype, dict(form="heads", B=2, n=2048, ratio=0.3), reached, 900)
    _run_case(ops, dtype, dict(form="linear", act=ACT_GELU_TANH, B=2, n=2048, x=first.x, center=first.center_out), reached, 901)
    for fam, s in sorted(SUMMARY.items()):
        print(f"fold chain {dtype} {fam}: " + ", ".join(f"{k}={v:.3g}" for k, v in s.items()))
    SUMMARY.clear()
