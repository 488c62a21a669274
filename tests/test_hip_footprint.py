"""Where the kernels read and write (include/primx_hip.h "Memory contract"), held by tests/footprint.py on the MI355X.

Every case runs three times through `footprint.hold`: with every torch.empty of the package poisoned by 0xFF bytes, by 0x00
bytes, and unguarded.  It asserts (a) every guard around every buffer the package allocated - outputs, workspaces at exactly
the queried size, count-sized outputs - and around every operand of the test is intact, (b) every `const` operand still holds
its snapshot, (c) every output and documented in-place operand is bit-identical between the two fills, (d) and to the unguarded
call; the count of device allocations the guard could not wrap is 0.  Shapes are the ragged and shipped ones of the contract
tests (their tables are imported).  No case provokes a fault: the one positive control is a plain torch store inside a guarded
allocation."""
import os

import numpy as np
import pytest
import torch

from oracle import synth
from tests import footprint as fp
from tests import raymarch_scenes as sc
from tests import test_hip_contract as TC
from tests import test_hip_fold_contract as TF
from tests import test_hip_fp32_contract as T32
from tests import test_hip_mesh as TM
from tests import test_hip_mesh_scale as TS
from tests import test_primsdf_contract as TP
from tests import test_raymarch_contract as TR
from tests.golden.make_golden import SEED, VAE_CFG
from tests.golden.make_golden_xl import HEADS, L_COND, XL, XL_SEED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
DTYPES = [F16, BF16]


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


@pytest.fixture(scope="module")
def pkg(ops):
    import topia_xl_amd
    return topia_xl_amd


def I(g, t, name, const=True):
    """`t` inside a guarded allocation of the same strides (None stays None)."""
    return None if t is None else g.guard_input(t, name, const).t


def changed(t, snap):
    """Number of elements of `t` whose bits differ from `snap` (a device scalar: no synchronisation)."""
    w = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return (t.contiguous().view(w) != snap.contiguous().view(w)).sum()


def zero(plain, *keys):
    for k in keys:
        assert int(plain[k]) == 0, f"{k}: {int(plain[k])} elements changed"


def rnd(seed, *shape, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dtype)


# ------------------------------------------------------------------------------------------------ the positive control
def test_positive_control_a_store_into_a_guard_fails_the_check(ops):
    """A legal torch store (inside the guarded allocation, behind the payload) must make check() fail - with the site, the side,
    the offsets and the byte count - and a store into a const operand, and a fill-dependent result, likewise."""
    x = rnd(1, 300, 7)
    with pytest.raises(fp.FootprintError, match=r"empty allocated at .*ops\.py:\d+: back guard damaged, [12] bytes, offsets [01] \.\. [01] "):
        with fp.guarded(0xFF) as g:
            out = ops.cast16(I(g, x, "x"), F16)
            flat = out.view(-1)
            flat.as_strided((1,), (1,), flat.storage_offset() + flat.numel()).fill_(3.0)
    with pytest.raises(fp.FootprintError, match=r"front guard damaged, [1-4] bytes, offsets -[1-4] \.\. -[1-4] .*\n.*const operand 'input x'"):
        with fp.guarded(0x00) as g:
            xi = I(g, x, "x")
            ops.cast16(xi, F16)
            flat = xi.view(-1)
            flat.as_strided((1,), (1,), flat.storage_offset() - 1).fill_(3.0)
            flat[5] = 1.0
    with pytest.raises(fp.FootprintError, match="results depend on the contents of torch.empty scratch"):
        fp.hold(lambda g: g.empty(4, 4, dtype=torch.float32, device=DEV) + 1)
    with fp.guarded(0xFF) as g:                                    # and an untouched run passes, with nothing unguarded
        ops.cast16(I(g, x, "x"), F16)
        assert len(g.records) == 2 and not g.bypassed


# ------------------------------------------------------------------------------------------------ GEMM family
def _gemm_case(ops, g, dtype, case):
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    op, M, N, K = case["op"], case["M"], case["N"], case["K"]
    seed = TC._seed(op, M, N, K, "normal")
    A, W, b = TC._operands(seed, M, N, K, dtype, bias=case.get("bias", True))
    A, W, b = I(g, A, "A"), I(g, W, "W"), I(g, b, "bias")
    out = {}
    if op == "linear":
        for act, scale in case.get("acts", [(0, 1.0)]):
            out[f"act{act} x{scale}"] = ops.linear(A, W, b, act=act, out_scale=scale)
        out["out="] = ops.linear(A, W, b, out=g.empty(M, N, dtype=dtype, device=DEV))
    elif op == "residual":
        res = I(g, rnd(seed + 1, M, N, scale=0.3, dtype=dtype), "res")
        out["res"] = ops.linear_residual(A, W, b, res, 0.70710678)
        out["no res"] = ops.linear_residual(A, W, b, None, 1.0)
    elif op in ("gate", "gate_ln"):
        rpb = case["rpb"]
        nb = (M + rpb - 1) // rpb
        mod = rnd(seed + 2, nb, 3 * N, scale=0.5, dtype=dtype)
        gate, shift, scl = (I(g, mod[:, i * N:(i + 1) * N], n) for i, n in enumerate(("gate", "shift", "scale")))   # row stride 3 N
        x = I(g, rnd(seed + 3, M, N, scale=4.0), "x", const=False)
        if op == "gate":
            ops.linear_gate_residual(A, W, b, gate, x, rpb)
        else:
            lnout = g.empty(M, N, dtype=dtype, device=DEV)
            sync = I(g, torch.zeros(ops.ln_sync_words(M), dtype=torch.int32, device=DEV), "sync", const=False)
            ops.linear_gate_residual(A, W, b, gate, x, rpb, ln=(shift, scl, lnout, 1e-6, sync))
            out["ln_out"], out["sync words not zero"] = lnout, (sync != 0).sum()
            lnout2 = g.empty(M, N, dtype=dtype, device=DEV)                       # the two-launch route of the same entry point
            x2 = I(g, rnd(seed + 3, M, N, scale=4.0), "x2", const=False)
            ops.linear_gate_residual(A, W, b, gate, x2, rpb, ln=(shift, scl, lnout2, 1e-6, None))
            out["ln_out (two launches)"], out["x (two launches)"] = lnout2, x2
        out["x"] = x
    elif op == "heads":
        B, n, H, dh = case["B"], case["n"], case["H"], case["dh"]
        kinds = case.get("kinds", [HEADS_ROWS, HEADS_KROWS, HEADS_VT])
        role = {HEADS_ROWS: "q", HEADS_KROWS: "k", HEADS_VT: None}
        pad = 256 if n % 256 == 0 else 128
        dsts = [ops.alloc_heads(B, H, n, dh, kd, dtype, DEV, pad, role[kd]) for kd in kinds]
        snaps = [d.clone() for d in dsts]
        ops.linear_heads(A, W, b, n, H, dh, kinds, dsts, dsts[0].shape[2], scale0=dh ** -0.5)
        for kd, d, s in zip(kinds, dsts, snaps):
            out[f"kind {kd}"] = d
            w = d.view(torch.int16) != s.view(torch.int16)
            out[f"kind {kd} pads written"] = (w & ~TF._heads_valid_mask(d, kd, n, dh)).sum()
    else:
        raise AssertionError(op)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_family_footprint(ops, dtype):
    """Every row of test_hip_contract.GEMM_CASES - linear (every act / scale, fresh and `out=`), residual, gate, gate + LayerNorm
    (tail route with sync words, and the two-launch route), heads with the role columns and the all-ones V^T row - i.e. every
    kernel of the default dispatch with its ragged M, N and K tails.  Pads of the heads destinations keep what alloc_heads put
    there; the LayerNorm sync words are zero after the launch."""
    for case in TC.GEMM_CASES:
        plain = fp.hold(lambda g: _gemm_case(ops, g, dtype, case))
        zero(plain, *[k for k in plain if k.endswith("pads written") or k.endswith("not zero")])
        assert all(bool(torch.isfinite(v.float()).all()) for k, v in plain.items() if v.dim()), case   # nothing left unwritten


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_f32out_footprint(ops, dtype):
    """primx_linear_f32out and primx_linear_f32out_group at the shapes of test_linear_f32out_rigorous_bound."""
    M, K = 16, 1152

    def case(g):
        outs, problems = {}, []
        for i, N in enumerate((1152, 3456, 288)):
            A = I(g, rnd(51 + i, M, K, dtype=dtype), "A")
            W = I(g, rnd(61 + i, N, K, scale=K ** -0.5, dtype=dtype), "W")
            b = I(g, rnd(71 + i, N, scale=0.3, dtype=dtype), "b")
            outs[f"single N={N}"] = ops.linear_f32out(A, W, b, g.empty(M, N, dtype=torch.float32, device=DEV), 8)
            problems.append((A, W, b, g.empty(M, N, dtype=torch.float32, device=DEV)))
        outs["grouped"] = ops.linear_f32out_group(problems, 8)
        outs["group"] = [p[3] for p in problems] if outs["grouped"] else None
        return outs
    plain = fp.hold(case)
    assert plain["grouped"] or os.environ.get("PRIMX_UV_GROUP") == "0"
    if plain["grouped"]:                                           # (another kernel than the single launch: same rows within rounding)
        for i, N in enumerate((1152, 3456, 288)):
            assert torch.allclose(plain["group"][i], plain[f"single N={N}"], rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ the LayerNorm fold
_SITES = {}


def _site(ops, dtype, i, case):
    """The consumer's operands (a16, part, center, u, v, W) of fold-contract case i, made once by the real producer."""
    key = (dtype, i)
    if key not in _SITES:
        from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
        kinds = [{"q": HEADS_ROWS, "k": HEADS_KROWS, "v": HEADS_VT}[c] for c in case.get("kinds", "qkv")]
        Nc = case.get("Nc", len(kinds) * TF.H * TF.DH if case["form"] in ("heads", "pair") else 4608)
        regime = {k: case[k] for k in ("ratio", "spread", "offset", "const_rows", "massive", "neg1_cols") if k in case}
        _SITES.clear()                                             # (one site alive at a time: up to 10240 x 1152 rows)
        _SITES[key] = (TF.Site(ops, 700 + i, dtype, case["B"], case["n"], Nc, **regime), kinds)
    return _SITES[key]


def _fold_consumer_case(ops, g, dtype, i, case):
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    site, kinds = _site(ops, dtype, i, case)
    form, B, n, M, Nc = case["form"], case["B"], case["n"], site.M, site.Nc
    a16, W, part, u, v, center = (I(g, t, nm) for t, nm in ((site.a16, "a16"), (site.W, "W"), (site.part, "part"), (site.u, "u"),
                                                            (site.v, "v"), (site.center_copy, "center")))
    center_out = g.empty(M, 2, dtype=torch.float32, device=DEV)                   # the guard sits directly behind row M - 1
    out = {"center_out": center_out}
    if form == "linear":
        out["out"] = ops.linear_fold(a16, W, g.empty(M, Nc, dtype=dtype, device=DEV), part, u, v, center, center_out, TF.EPS,
                                     act=case.get("act", 0))
        return out
    pad = 256 if n % 256 == 0 else 128
    role = {HEADS_ROWS: "q", HEADS_KROWS: "k", HEADS_VT: None}
    dsts = [ops.alloc_heads(B, TF.H, n, TF.DH, k, dtype, DEV, pad, role[k]) for k in kinds]
    snaps = [d.clone() for d in dsts]
    scale0 = case.get("scale0", 1.0)
    if form == "heads":
        ops.linear_heads_fold(a16, W, n, TF.H, TF.DH, kinds, dsts, dsts[0].shape[2], part, u, v, center, center_out, TF.EPS, scale0=scale0)
    else:
        Lk, L, Dc = 1536, 1370, 768
        y16 = torch.zeros(Lk, Dc, device=DEV)
        y16[:L] = rnd(900 + i, L, Dc)
        y16 = I(g, y16.to(dtype), "y16")
        Wkv = I(g, rnd(901 + i, 2 * TF.D, Dc, scale=Dc ** -0.5, dtype=dtype), "Wkv")
        bkv = I(g, rnd(902 + i, 2 * TF.D, scale=0.3, dtype=dtype), "bkv")
        kv = [ops.alloc_heads(1, TF.H, L, TF.DH, k, dtype, DEV, 256, r) for k, r in ((HEADS_KROWS, "k"), (HEADS_VT, None))]
        kvs = [t.clone() for t in kv]
        fold = dict(A=a16, W=W, rows_per_batch=n, heads=TF.H, dh=TF.DH, kinds=kinds, dsts=dsts, n_pad=dsts[0].shape[2], part=part,
                    u=u, v=v, center=center, center_out=center_out, eps=TF.EPS, scale0=scale0)
        ops.linear_heads_fold_pair(fold, y16, Wkv, bkv, Lk, TF.H, TF.DH, [HEADS_KROWS, HEADS_VT], kv, kv[0].shape[2])
        for k, d, s in zip((HEADS_KROWS, HEADS_VT), kv, kvs):
            out[f"rider kind {k}"] = d
            # (the rider is told rows_per_batch = Lk: the zero rows L .. Lk - 1 of y16 are projected like the others, as in DiT._cond_state)
            out[f"rider kind {k} pads written"] = ((d.view(torch.int16) != s.view(torch.int16)) & ~TF._heads_valid_mask(d, k, Lk, TF.DH)).sum()
    for k, d, s in zip(kinds, dsts, snaps):
        out[f"kind {k}"] = d
        out[f"kind {k} pads written"] = ((d.view(torch.int16) != s.view(torch.int16)) & ~TF._heads_valid_mask(d, k, n, TF.DH)).sum()
    return out


def _fold_producer_case(ops, g, dtype, B, n):
    D, Kp, M = TF.D, 128, B * n
    A = I(g, rnd(11, M, Kp, dtype=dtype), "A")
    Wp = I(g, rnd(12, D, Kp, scale=Kp ** -0.5, dtype=dtype), "W")
    bias = I(g, rnd(13, D, scale=0.3, dtype=dtype), "bias")
    gate = I(g, rnd(14, B, 3 * D, scale=0.1, dtype=dtype)[:, D:2 * D], "gate")
    scale = I(g, rnd(15, 1, D, scale=0.4, dtype=dtype), "next_scale").expand(B, -1)
    x0 = rnd(16, M, D, scale=2.0)
    cen = torch.stack([x0.mean(-1), 1.0 / torch.sqrt(x0.var(-1) + 1e-6)], -1).contiguous()
    x, center = I(g, x0, "x", const=False), I(g, cen, "center")
    a16 = g.empty(M, D, dtype=dtype, device=DEV)
    part = g.empty(M, D // 144, 2, dtype=torch.float32, device=DEV)
    ops.linear_gate_residual_fold(A, Wp, bias, gate, x, n, scale, center, a16, part)
    stats = ops.row_stats(x, 1e-6, g.empty(M, 2, dtype=torch.float32, device=DEV))
    return {"x": x, "a16": a16, "part": part, "row_stats": stats}


@pytest.mark.parametrize("dtype", DTYPES)
def test_fold_producer_and_consumers_footprint(ops, dtype):
    """primx_linear_gate_residual_fold (+ primx_row_stats) at the (B, n) of the fold contract's cases, and every consumer case of
    tests/test_hip_fold_contract.py: heads, linear and the pair launch with its rider.  `center` is untouched; center_out ends at
    row M - 1; pads of every heads destination keep alloc_heads' contents."""
    if not TF._fold_kernels_selectable(ops):
        pytest.skip("a kernel-selection switch removes a tile shape of the fold kernels")
    for B, n in sorted({(c["B"], c["n"]) for c in TF.CASES}):
        plain = fp.hold(lambda g: _fold_producer_case(ops, g, dtype, B, n))
        assert all(bool(torch.isfinite(v.float()).all()) for v in plain.values()), (B, n)
    for i, case in enumerate(TF.CASES):
        plain = fp.hold(lambda g: _fold_consumer_case(ops, g, dtype, i, case))
        zero(plain, *[k for k in plain if k.endswith("pads written")])
    _SITES.clear()


# ------------------------------------------------------------------------------------------------ attention
def _packed(ops, g, q, k, v, pad_q=None, pad_k=None):
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    Qp = ops.pack_heads(I(g, q, "q"), HEADS_ROWS, pad_q or ops.BQ, "q")
    Kp = ops.pack_heads(I(g, k, "k"), HEADS_KROWS, pad_k or ops.BKV, "k")
    Vt = ops.pack_heads(I(g, v, "v"), HEADS_VT, pad_k or ops.BKV)
    return Qp, Kp, Vt


def _attn_case(ops, g, dtype, B, Mq, Mk, H, dh, pads=(None, None), strided=False):
    q, k, v = TC._qkv(dh + Mq, B, Mq, Mk, H, dh, 1.0, dtype)
    if strided:                                                    # the unbind views of a fused qkv buffer (self-attention: Mq == Mk)
        qkv = torch.stack([q, k, v], 2)
        q, k, v = qkv.unbind(2)
    Qp, Kp, Vt = _packed(ops, g, q, k, v, *pads)
    snaps = [t.clone() for t in (Qp, Kp, Vt)]
    out = ops.attention(Qp, Kp, Vt, Mq, Mk, dh, dh ** -0.5)        # [B, nq, H dh]: the guard sits directly behind row nq - 1
    res = {"out": out, "Qp": Qp, "Kp": Kp, "Vt": Vt}
    for nm, t, s in zip(("Qp", "Kp", "Vt"), (Qp, Kp, Vt), snaps):
        res[nm + " written"] = changed(t, s)
    return res


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_footprint(ops, dtype):
    """primx_pack_heads (all three kinds, plain and strided sources) and primx_attention at the ragged (nq, nkv) pairs of
    test_attention_bound for dh 72 / 64 / 32, the compact 64-token kernel with a masked tail, and a multi-tile self-attention on
    strided qkv views.  Q, K and V^T - pads included - are unchanged by the attention launch; the output has nq rows."""
    cases = [dict(B=1, Mq=300, Mk=1000, H=2, dh=72), dict(B=1, Mq=200, Mk=700, H=2, dh=64), dict(B=2, Mq=300, Mk=500, H=2, dh=32),
             dict(B=3, Mq=64, Mk=50, H=4, dh=32, pads=(64, 64)), dict(B=1, Mq=512, Mk=512, H=1, dh=72, strided=True)]
    for c in cases:
        plain = fp.hold(lambda g: _attn_case(ops, g, dtype, **c))
        zero(plain, "Qp written", "Kp written", "Vt written")
        assert plain["out"].shape == (c["B"], c["Mq"], c["H"] * c["dh"]) and bool(torch.isfinite(plain["out"].float()).all())
        if c.get("pads"):
            assert plain["Qp"].shape[2] == 64 and plain["Kp"].shape[2] == 64                 # the form attn64_kernel takes


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,b_from,Mq,Mk,H,dh", [(2, 1, 300, 1370, 4, 72), (3, 0, 256, 1370, 2, 72), (3, 2, 64, 129, 4, 32)])
def test_attention_bcast_footprint(ops, dtype, B, b_from, Mq, Mk, H, dh):
    """primx_attention_bcast with b_from = 0 and > 0 (shapes of test_broadcast_key_value_entries)."""
    from topia_xl_amd import _lib
    q = synth.tensor(25, "q", (B, Mq, H, dh)).to(dtype).to(DEV)
    k = synth.tensor(25, "k", (B, Mk, H, dh)).to(dtype).to(DEV)
    v = synth.tensor(25, "v", (B, Mk, H, dh)).to(dtype).to(DEV)
    krow, vrow = synth.tensor(25, "krow", (1, 1, H, dh)).to(dtype).to(DEV), synth.tensor(25, "vrow", (1, 1, H, dh)).to(dtype).to(DEV)
    nb = ops.bcast_keys(Mk)

    def case(g):
        Qp = ops.pack_heads(I(g, q, "q"), _lib.HEADS_ROWS, ops.BQ, "q")
        Kb = ops.pack_heads(I(g, krow.expand(1, nb, H, dh).contiguous(), "krow"), _lib.HEADS_KROWS, ops.BKV, "k")
        Vb = ops.pack_heads(I(g, vrow.expand(1, nb, H, dh).contiguous(), "vrow"), _lib.HEADS_VT, ops.BKV)
        Kp = ops.pack_heads(I(g, k[:b_from].contiguous(), "k"), _lib.HEADS_KROWS, ops.BKV, "k") if b_from else None
        Vt = ops.pack_heads(I(g, v[:b_from].contiguous(), "v"), _lib.HEADS_VT, ops.BKV) if b_from else None
        held = [t for t in (Qp, Kb, Vb, Kp, Vt) if t is not None]
        snaps = [t.clone() for t in held]
        out = ops.attention(Qp, Kp, Vt, Mq, Mk, dh, dh ** -0.5, bcast=(Kb, Vb))
        return {"out": out, "operands written": sum(changed(t, s) for t, s in zip(held, snaps))}
    plain = fp.hold(case)
    zero(plain, "operands written")
    assert plain["out"].shape == (B, Mq, H * dh)


def test_attention_f32_footprint(ops):
    """primx_attention_f32 on the three differently strided views of test_attention_f32_contract_rescale_and_strides (a [B, H, M,
    dh] tensor viewed as BMHK, batch stride 0, head stride dh + 8) and on a ragged contiguous shape."""
    B, Nq, Nk, H, dh = 3, 130, 77, 4, 72
    q0 = rnd(27, B, H, Nq, dh).permute(0, 2, 1, 3)
    k0 = rnd(28, 1, Nk, H, dh).expand(B, Nk, H, dh)
    v0 = rnd(29, B, Nk, H, dh + 8)[..., :dh]

    def case(g):
        q, k, v = I(g, q0, "q"), I(g, k0, "k"), I(g, v0, "v")
        assert q.stride() == q0.stride() and k.stride(0) == 0 and v.stride(2) == dh + 8
        qc, kc, vc = (I(g, t.contiguous(), n) for t, n in ((q0[:1, :33], "qc"), (k0[:1, :45], "kc"), (v0[:1, :45], "vc")))
        return {"strided": ops.attention_f32(q, k, v), "strided scale": ops.attention_f32(q, k, v, 1.0 / dh),
                "33 x 45": ops.attention_f32(qc, kc, vc)}
    plain = fp.hold(case)
    assert plain["strided"].shape == (B, Nq, H, dh) and plain["strided"].is_contiguous()


# ------------------------------------------------------------------------------------------------ row and fp32 kernels
VEC_SIZES = (1, 7, 255, 257, 2048 * 256 - 1, 2048 * 256 + 1)      # one element, a ragged vector, one 256-thread block and the
#                                                                   2048-block grid cap of the grid-stride loops, each +- 1


@pytest.mark.parametrize("n", VEC_SIZES)
def test_elementwise_footprint(ops, n):
    """cast16, silu_cast (fresh and `out=`), cfg_combine (fp16 / bf16 / fp32) and silu_f32 at n elements."""
    x = rnd(n, n, scale=2.0)

    def case(g):
        xi = I(g, x, "x")
        out = {"silu_f32": ops.silu_f32(xi)}
        for dt in DTYPES:
            out[f"cast16 {dt}"] = ops.cast16(xi, dt)
            out[f"silu_cast {dt}"] = ops.silu_cast(xi, dt)
            out[f"cast16 out= {dt}"] = ops.cast16(xi, dt, out=g.empty(n, dtype=dt, device=DEV))
        for dt in (F16, BF16, torch.float32):
            mo = I(g, rnd(n + 1, 2, n).to(dt), "model_out")
            out[f"cfg_combine {dt}"] = ops.cfg_combine(mo, 6.0)
        return out
    plain = fp.hold(case)
    assert torch.equal(plain[f"cast16 {F16}"], x.to(F16)) and plain[f"cfg_combine {F16}"].shape == (1, n)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_modulate_footprint(ops, dtype):
    """Both kernels of primx_layernorm_modulate (the row-in-registers kernel at D = 1152 / 384 / 256 and the general one at D = 200, the
    N of GEMM_CASES' ragged gate case)
    with ragged rows and strided shift / scale views, with prefetch ranges (a byte count that is no multiple of a line), primx_prefetch,
    primx_row_stats and primx_layernorm_modulate_f32."""
    for D, rows, rpb in ((1152, 600, 256), (384, 301, 100), (256, 130, 64), (200, 70, 35)):
        nb = (rows + rpb - 1) // rpb
        x0 = rnd(D + rows, rows, D, scale=3.0) + 0.7
        mod = rnd(D, nb, 3 * D, scale=0.4)

        def case(g):
            x = I(g, x0, "x")
            sh, sc = I(g, mod.to(dtype)[:, :D], "shift"), I(g, mod.to(dtype)[:, 2 * D:], "scale")
            w = I(g, rnd(3, 777, 64, dtype=dtype), "prefetched")
            out = {"ln": ops.layernorm_modulate(x, sh, sc, rpb, g.empty(rows, D, dtype=dtype, device=DEV)),
                   "ln + prefetch": ops.layernorm_modulate(x, sh, sc, rpb, g.empty(rows, D, dtype=dtype, device=DEV), prefetch=(w,))}
            sh32, sc32 = I(g, mod[:, :D], "shift32"), I(g, mod[:, 2 * D:], "scale32")
            out["ln_f32"] = ops.layernorm_modulate_f32(x, sh32, sc32, rpb, 1e-6)
            out["row_stats"] = ops.row_stats(x, 1e-6, g.empty(rows, 2, dtype=torch.float32, device=DEV))
            ops.prefetch(w, torch.cuda.current_stream())            # primx_prefetch: reads [ptr, ptr + bytes), writes nothing
            return out
        plain = fp.hold(case)
        assert torch.equal(plain["ln"], plain["ln + prefetch"])


def test_front_end_footprint(ops):
    """timestep_embedding, point_features (row-strided input, padded output), vit_tokens (with and without register tokens),
    pack_heads on strided sources (inside the attention cases too), latent_denorm and vae_output."""
    t = torch.tensor([0, 1, 40, 500, 960, 999, 7], device=DEV)
    xs = rnd(5, 301, 9)                                            # token rows of 9 columns, of which the kernel reads 1..3
    fr = torch.pow(2.0, torch.arange(8, device=DEV).float()) * 3.14159
    patches, cls, pos, reg = rnd(6, 2, 37, 96), rnd(7, 96), rnd(8, 38, 96), rnd(9, 4, 96)
    lat, mean, std = rnd(10, 3, 5, 68), rnd(11, 68, scale=0.5), rnd(12, 68, scale=0.2).abs() + 0.5

    def case(g):
        out = {"timestep_embedding": ops.timestep_embedding(I(g, t, "t"), 256)}
        x = I(g, xs[:, :5], "x rows")                               # row stride 9 > 5 columns
        out["point_features"] = ops.point_features(x, I(g, fr, "freqs"))
        p, c, po, r = I(g, patches, "patches"), I(g, cls, "cls"), I(g, pos, "pos"), I(g, reg, "reg")
        out["vit_tokens"], out["vit_tokens reg"] = ops.vit_tokens(p, c, po, None), ops.vit_tokens(p, c, po, r)
        out["latent_denorm"] = ops.latent_denorm(I(g, lat, "lat"), I(g, mean, "mean"), I(g, std, "std"), 1.3)
        for dt in DTYPES:
            y = I(g, rnd(13, 3, 512, 6, dtype=dt), "decoded")
            out[f"vae_output {dt}"] = [ops.vae_output(y, True), ops.vae_output(y, False)]
        return out
    plain = fp.hold(case)
    assert plain["point_features"].shape == (301, 52) and bool((plain["point_features"][:, 51] == 0).all())   # the pad column
    assert plain["vit_tokens reg"].shape == (2, 42, 96)


@pytest.mark.parametrize("out_dtype", [F16, BF16, torch.float32])
def test_diffusion_step_footprint(ops, pkg, out_dtype):
    """primx_diffusion_step: all three mean types, DDIM with and without noise, ancestral with both variance types, clipped."""
    d = pkg.create_diffusion("ddim25", noise_schedule="squaredcos_cap_v2", parameterization="v")
    coef0 = torch.from_numpy(d.step_coefficients(0.5)).to(DEV)
    x0, mo0, n0 = rnd(5, 2, 97, 68), rnd(6, 2, 97, 136).to(out_dtype), rnd(7, 2, 97, 68)

    def case(g):
        x, mo, noise, coef = I(g, x0, "x"), I(g, mo0, "model_out"), I(g, n0, "noise"), I(g, coef0, "coef")
        out = {}
        for mean_type in (0, 1, 2):
            out[f"ddim {mean_type}"] = ops.diffusion_step(x, mo, coef, 7, mean_type=mean_type, var_type=3, ancestral=False,
                                                          clip_denoised=False, noise=noise)
            out[f"ddim {mean_type} eta 0"] = ops.diffusion_step(x, mo, coef, 0, mean_type=mean_type, var_type=3, ancestral=False,
                                                                clip_denoised=True, noise=None)
            for var_type in (2, 3):
                out[f"ancestral {mean_type} {var_type}"] = ops.diffusion_step(x, mo, coef, 24, mean_type=mean_type, var_type=var_type,
                                                                              ancestral=True, clip_denoised=False, noise=noise)
        return out
    fp.hold(case)


def test_fp32_gemms_footprint(ops):
    """primx_gemm_f32 (plain / GELU / scaled / gated in place) at the ragged rows of test_hip_fp32_contract.GEMM_CASES and
    primx_linear_f32: the tiled kernel with its second destination and N % 4 != 0, and the few-row kernel at M = 1 .. 8."""
    for c in [c for c in T32.GEMM_CASES if c["M"] <= 300]:
        M, N, K = c["M"], c["N"], c["K"]
        A0, W0, b0 = rnd(M + N, M, K), rnd(N + K, N, K, scale=K ** -0.5), rnd(K, N, scale=0.1)

        def case(g):
            A, W, b = I(g, A0, "A"), I(g, W0, "W"), I(g, b0, "b")
            out = {"plain": ops.gemm_f32(A, W, b, act=c.get("act", 0), out_scale=c.get("scale", 1.0)),
                   "no bias": ops.gemm_f32(A, W, None, act=1)}
            rpb = c.get("rpb", (M + 1) // 2)
            gate = I(g, rnd(1, (M + rpb - 1) // rpb, 9 * N)[:, 2 * N:3 * N], "gate")
            out["gated"] = ops.gemm_f32(A, W, b, out=I(g, rnd(2, M, N), "x", const=False), gate=gate, rows_per_batch=rpb)
            return out
        fp.hold(case)
    for M, N, K in ((130, 70, 12), (9, 70, 260), (300, 333, 260), (1, 70, 12), (5, 333, 260), (8, 7, 588), (2, 63, 256)):
        A0, W0, b0 = rnd(M, M, K), rnd(N, N, K, scale=K ** -0.5), rnd(K, N)

        def case(g):
            A, W, b = I(g, A0, "A"), I(g, W0, "W"), I(g, b0, "b")
            out = {"plain": ops.linear_f32(A, W, b), "silu": ops.linear_f32(A, W, b, act_out=1), "no bias": ops.linear_f32(A, W, None)}
            if M > 8:
                o1, o2 = g.empty(M, N, dtype=torch.float32, device=DEV), g.empty(M, N, dtype=torch.float32, device=DEV)
                ops.linear_f32(A, W, b, out=o1, out2=o2)
                out["two destinations"] = [o1, o2]
            return out
        plain = fp.hold(case)
        if M > 8:
            assert torch.equal(plain["two destinations"][0], plain["plain"]) and torch.equal(plain["two destinations"][1], plain["plain"])


# ------------------------------------------------------------------------------------------------ VAE
def _conv_weights(Cin, Cout, dtype):
    return TC._conv_w(Cin * Cout, Cout, Cin, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [1, 3, 300])
def test_vae_kernels_footprint(ops, dtype, P):
    """groupnorm_silu, conv_in, conv3d_k3 (implicit GEMM and the three packed kernels; with and without `res`; gn= inside),
    conv3d_s8_fused, convtranspose_k2s2 (GEMM form; packed with want_stats), group_stats, and the pack routines, at P = 1, 3 and
    300 primitives (300: the persistent workgroups walk more than one primitive).  The packed images are torch.empty buffers
    between guards: the pack routines write exactly their bytes."""
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the implicit GEMM")
    for Cin, Cout, S, kind in ((256, 256, 4, "s4"), (256, 512, 4, "s4"), (256, 32, 8, "s8"), (32, 32, 8, "s8c32"), (32, 6, 8, "s8c32"),
                               (64, 48, 4, None)):
        V = S ** 3
        x0 = TC._cl_rand(Cin + S, P, V, Cin, dtype)
        wk0, b0 = _conv_weights(Cin, Cout, dtype)
        res0 = TC._cl_rand(Cout, P, V, Cout, dtype)
        gam0, bet0 = TC._gn_params(Cin, Cin)

        def case(g):
            x, wk, b, res = I(g, x0, "x"), I(g, wk0, "Wk"), I(g, b0, "bias"), I(g, res0, "res")
            out = {"implicit": ops.conv3d_k3(x, wk, b, S, res=res, res_scale=0.5 ** 0.5), "implicit plain": ops.conv3d_k3(x, wk, None, S)}
            wp = ops.pack_conv3(wk, Cin)
            assert (wp is not None and wp.kind == kind and wp.S == S) if kind else wp is None
            if wp is not None:
                out["image"] = wp.Wp
                out["packed"] = ops.conv3d_k3(x, wk, b, S, res=res, res_scale=0.5 ** 0.5, Wp=wp)
                out["packed plain"] = ops.conv3d_k3(x, wk, None, S, Wp=wp)
                if kind == "s8c32":
                    gam, bet = I(g, gam0, "gamma"), I(g, bet0, "beta")
                    out["gn inside"] = ops.conv3d_k3(x, wk, b, S, res=res, res_scale=0.5 ** 0.5, Wp=wp, gn=(gam, bet, 1e-5))
                    out["gn inside plain"] = ops.conv3d_k3(x, wk, b, S, Wp=wp, gn=(gam, bet, 1e-5))
            return out
        plain = fp.hold(case)
        assert all(bool(torch.isfinite(v.float()).all()) for v in plain.values()), (Cin, Cout)
    for C, V, groups, silu in ((256, 64, 32, True), (256, 512, 32, True), (32, 512, 32, True), (64, 27, 8, False)):
        x0 = TC._cl_rand(C + V, P, V, C, dtype, 1.3, 0.2)
        gam0, bet0 = TC._gn_params(C, C)
        fp.hold(lambda g: ops.groupnorm_silu(I(g, x0, "x"), I(g, gam0, "gamma"), I(g, bet0, "beta"), groups, 1e-5, silu))
    for S, Cout in ((4, 256), (8, 32)):
        z0, W0, b0 = rnd(41 + S, P, S ** 3), rnd(42, Cout, 27, scale=0.2), rnd(43, Cout, scale=0.2)
        fp.hold(lambda g: ops.conv_in(I(g, z0, "z"), 1.7, -0.3, I(g, W0, "W"), I(g, b0, "b"), S, dtype))
    # the k2s2 upsample (GEMM form at both contract shapes, packed with statistics), group_stats and the fused 256 -> 32 front
    for S, Cin, Cout in ((4, 256, 256), (4, 64, 48)):
        x0 = TC._cl_rand(31 + Cin, P, S ** 3, Cin, dtype)
        wt0, b0 = rnd(32, 8 * Cout, Cin, scale=Cin ** -0.5, dtype=dtype), rnd(33, Cout, scale=0.3, dtype=dtype)
        gam0, bet0 = TC._gn_params(23, 256)
        wk0, b10 = _conv_weights(256, 32, dtype)
        wsc0, bsc0 = rnd(34, 32, 256, scale=256 ** -0.5, dtype=dtype), rnd(35, 32, scale=0.2, dtype=dtype)

        def case(g):
            x, wt, b = I(g, x0, "x"), I(g, wt0, "Wt"), I(g, b0, "bias")
            out = {"gemm form": ops.convtranspose_k2s2(x, wt, b, S)}
            wp = ops.pack_convt_s4(wt)
            assert (wp is not None) == (Cin == 256)
            if wp is not None:
                h8, part = ops.convtranspose_k2s2(x, wt, b, S, Wp=wp, want_stats=True)
                out.update(image=wp, packed=h8, part=part, stats=ops.group_stats(part, b, 1e-5),
                           packed_alone=ops.convtranspose_k2s2(x, wt, b, S, Wp=wp))
                wk, wsc = I(g, wk0, "Wk"), I(g, wsc0, "Wsc")
                wp3 = ops.pack_conv3(wk, 256, Wsc=wsc)
                assert wp3.has_sc
                out["fused image"] = wp3.Wp
                out["fused"] = ops.conv3d_s8_fused(h8, wp3, I(g, b10, "b1"), part, b, I(g, gam0, "gamma"), I(g, bet0, "beta"), 1e-5,
                                                   I(g, bsc0, "bsc"))
            return out
        plain = fp.hold(case)
        if Cin == 256:
            assert torch.equal(plain["packed"], plain["packed_alone"])


def _vae(pkg, dtype):
    vae = pkg.VAE(**VAE_CFG).eval()
    vae.load_state_dict(synth.state_dict_like(SEED, vae.state_dict()), strict=True)
    vae.to(DEV)
    vae.compute_dtype = dtype
    return vae


@pytest.mark.parametrize("P", [3, 2048])
def test_vae_decode_footprint(pkg, P):
    """VAE.decode, whole, under the guard: the packed weight images, the persistent attention operands (torch.empty where the
    projection writes every element) and every intermediate are (re)allocated in each run."""
    vae = _vae(pkg, F16)
    z0 = synth.tensor(9, "z", (P, 1, 4, 4, 4)).to(DEV)

    def case(g):
        vae.repack()
        vae.__dict__.pop("_attn_ws", None)
        z = I(g, z0, "z")
        return {"decoded": vae.decode(z), "denormalized": vae.decode(z, denormalize=True)}
    plain = fp.hold(case)
    assert plain["decoded"].shape == (P, 6, 8, 8, 8) and bool(torch.isfinite(plain["decoded"]).all())


# ------------------------------------------------------------------------------------------------ DiT
@pytest.fixture(scope="module")
def dit(pkg):
    cfg = dict(depth=2, **XL)
    with torch.device(DEV):
        m = pkg.DiT(seq_length=2048, num_heads=HEADS, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    m.load_state_dict(synth.dit_state_dict(XL_SEED, **cfg), strict=True)
    return m


def _fresh(m):
    """Drop every cached workspace of the model, so that the next forward allocates all of them again (under the guard)."""
    m.repack()
    m._fold_ws, m._ln_sync = {}, {}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("planned", [True, False], ids=["planned", "unplanned"])
def test_dit_forward_and_ddim_loop_footprint(pkg, dit, dtype, planned, monkeypatch):
    """configs[1] width (d = 1152, 16 heads, 2048 tokens, 1370 x 768 condition tokens, CFG: effective batch 2, T = 4096), two
    blocks: one forward_with_cfg and a 2-step DDIM loop - planned (the LayerNorm fold through primx_dit_blocks_fold: every
    workspace of the forward and fold_workspace poisoned) and unplanned (the LayerNorm launches).  The packed blob, the heads
    workspaces, the modulation and u / v tables are allocated anew in every run; the conditioning tensors are unchanged."""
    from importlib import import_module
    sampler = import_module(pkg.__name__ + ".diffusion.sampler")
    monkeypatch.setattr(sampler, "PLAN_TIMESTEPS", planned)
    x0, y0 = synth.tensor(77, "x", (1, 2048, 68)).to(DEV), synth.tensor(77, "y", (1, L_COND, 768)).to(DEV)
    t0 = torch.tensor([520], device=DEV)
    d = pkg.create_diffusion("ddim2", noise_schedule="squaredcos_cap_v2", parameterization="v")
    folded = []

    def case(g):
        _fresh(dit)
        x, y, t = I(g, x0, "x"), I(g, y0, "y"), I(g, t0, "t")
        out = {"forward_with_cfg": dit.forward_with_cfg(x, t, y, 6.0, dtype, True)}
        kw = dict(y=y, cfg_scale=6.0, precision_dtype=dtype, enable_amp=True)
        out["ddim2"] = [o["sample"].clone() for o in d.ddim_sample_loop_progressive(dit.forward_with_cfg, tuple(x.shape), noise=x,
                                                                                   clip_denoised=False, model_kwargs=kw)]
        folded.append(bool(dit._fold_ws))
        return out
    try:
        plain = fp.hold(case)
    finally:
        _fresh(dit)
    assert len(plain["ddim2"]) == 2 and bool(torch.isfinite(plain["ddim2"][-1]).all())
    if planned and dit.fold_ln and dit.blocks_call and not os.environ.get("PRIMX_GEMM_NOBIG"):
        assert all(folded), "the planned loop did not take the LayerNorm fold"
    if not planned:
        assert not any(folded)


# ------------------------------------------------------------------------------------------------ rendering
@pytest.mark.parametrize("name,kw,fs", TR.CASES, ids=[c[0] for c in TR.CASES])
def test_raymarch_footprint(ops, name, kw, fs):
    """primx_compute_raydirs and primx_raymarch on the scenes of tests/test_raymarch_contract.py (ragged image sizes, the
    record-cache overflow, the hit-list cap, batch 2)."""
    from topia_xl_amd import raymarch as rm
    N, H, W = kw.get("N", 1), kw["H"], kw["W"]
    tpl, pos, rot, scale, cp, cr, f, pp = (t.to(DEV) for t in sc.scene(**kw))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xs, ys], -1)[None].expand(N, -1, -1, -1).contiguous().to(DEV)

    def case(g):
        rp, rd, tm = rm.compute_raydirs(I(g, cp, "campos"), I(g, cr, "camrot"), I(g, f, "focal"), I(g, pp, "princpt"),
                                        I(g, pc, "pixelcoords"), 1.0)
        img = rm.mvpraymarch(rp, rd, TR.DT, tm, (I(g, pos, "pos"), I(g, rot, "rot"), I(g, scale, "scale")), I(g, tpl, "template"),
                             fs, 8.0)
        return {"raypos": rp, "raydir": rd, "tminmax": tm, "image": img}
    plain = fp.hold(case)
    assert plain["image"].shape == (N, H, W, 4) and bool(torch.isfinite(plain["image"]).all())


@pytest.mark.parametrize("P,n", [(1, 1), (255, 255), (1023, 257), (1024, 255), (1025, 257), (3000, 257)])
@pytest.mark.parametrize("training", [False, True])
def test_primsdf_query_footprint(ops, P, n, training):
    """primx_primsdf_query at the LDS-chunk edges of test_hip_query_chunk_edges_random_features (1023 / 1024 / 1025 primitives,
    ragged point counts), eval mode (the fill of uncovered points) and training mode."""
    from topia_xl_amd.primsdf import PrimSDF
    gen = torch.Generator().manual_seed(P * 7 + n)
    srt, feat = TP._prims(gen, P, 8, lo=0.01, hi=0.03)
    x0 = (1.6 * torch.rand(n, 3, generator=gen) - 0.8).to(DEV)
    srt[P - 1, 0], srt[P - 1, 1:4] = 0.3, x0[0].cpu() + 0.05
    m = PrimSDF(num_prims=P, prim_shape=8)
    m.to(DEV).train(training)

    def case(g):
        m.srt_param.data, m.feat_param.data = I(g, srt.to(DEV), "srt"), I(g, feat.to(DEV), "feat")
        m._lin.clear()
        return m.query(I(g, x0, "x"))
    plain = fp.hold(case)
    assert plain.shape == (n, 6) and bool(torch.isfinite(plain).all())


# ------------------------------------------------------------------------------------------------ mesh export
def _mesh_outputs(m):
    return {k: getattr(m, k) for k in TS.ATTRS}


def _mesh_chain(M, g, field, R, size, target):
    """extract -> clean -> decimate + vertex normals -> bake, every stage on the previous one's output."""
    raw = M.extract_mesh(field, resolution=R)
    out = {"raw": _mesh_outputs(raw)}
    v, f = I(g, raw.v, "raw v"), I(g, raw.f, "raw f")
    st = {}
    cv, cf, cmap = M.clean_mesh(v, f, return_vmap=True, stats=st, **M.CLEAN_ARGS)
    out["clean"], out["clean stats"] = [cv, cf, cmap], sorted(st.items())
    cv, cf = I(g, cv, "clean v"), I(g, cf, "clean f")
    tgt = target if target is not None else max(cf.shape[0] * 3 // 4, 1)
    st = {}
    dv, df, dmap = M.decimate_mesh(cv, cf, tgt, return_vmap=True, stats=st)
    st["round_collapses"] = tuple(st["round_collapses"])
    out["decimate"], out["decimate stats"] = [dv, df, dmap], sorted(st.items())
    dv, df = I(g, dv, "decimated v"), I(g, df, "decimated f")
    nrm = M.vertex_normals(dv, df)
    out["normals"] = nrm
    z = torch.zeros(dv.shape[0], device=DEV)
    tm = M.bake_textures(field, M.TriMesh(dv, df, I(g, nrm, "normals"), z[:, None].expand(-1, 3), z, z), size=size[0]) \
        if size[0] == size[1] else None
    if tm is not None:
        out["bake"] = [tm.v, tm.f, tm.vt, tm.vmap, tm.albedo, tm.metallic_roughness, tm.covered]
    else:                                                          # a non-square atlas: the stages bake_textures calls, one by one
        a = M.uv_unwrap(dv, df, nrm, size)
        texel, pts = M.atlas_points(a, dv, df)
        with torch.no_grad():
            attr = field.query(pts)
        alb, mr = M.fill_textures(I(g, attr, "attr"), texel, a.face_id)
        out["bake"] = [a.vt, a.vmap, a.f, a.chart, a.face_id, a.uv_fixed, a.label, texel, pts, alb, mr]
        out["atlas"] = (a.n_charts, a.n_covered, a.doubly, a.split_rounds)
    return out


def test_marching_cubes_footprint_non_cubic(ops):
    """primx_mcubes_count / _emit on a non-cubic lattice (17 x 23 x 31 of test_exact_order_against_numpy, and the 131 x 257 x 67
    ellipsoid whose last scan block is ragged): the workspace is exactly primx_mcubes_workspace bytes between guards, v / f /
    normals have exactly nverts / ntris rows; primx_noise_filter at ragged primitive counts."""
    from topia_xl_amd import mesh as M
    vols = [(np.random.default_rng(71).standard_normal((17, 23, 31)).astype(np.float32), 0.3), (TS.ellipsoid(), 0.0137)]
    for vol, iso in vols:
        vd = torch.from_numpy(vol).to(DEV)
        plain = fp.hold(lambda g: M.marching_cubes(I(g, vd, "volume"), iso, return_normals=True))
        assert plain[0].shape[0] > 0 and plain[1].shape[0] > 0 and plain[2].shape == plain[0].shape
    for P in (1, 7, 300, 2048):
        srt = torch.cat([0.02 + 0.05 * torch.rand(P, 1), 1.6 * torch.rand(P, 3) - 0.8], 1).to(DEV)
        fp.hold(lambda g: M.noise_filter_mask(I(g, srt, "srt")))


def test_mesh_export_footprint_48(ops):
    """extract_mesh at resolution 48 on the synthetic field of tests/test_hip_mesh.py, then clean_mesh, decimate_mesh, vertex normals
    and the texture bake on a 512 x 384 atlas, each on the previous stage's output (odd V and F throughout).  Every _workspace
    buffer is exactly the queried size between guards, count-sized outputs end at their last element, the input mesh arrays are
    unchanged, results are bit-identical between fills."""
    from topia_xl_amd import mesh as M
    field = TM._synthetic_field()
    plain = fp.hold(lambda g: _mesh_chain(M, g, field, 48, (512, 384), None))
    assert plain["raw"]["f"].shape[0] > 0 and plain["clean"][1].shape[0] > 0 and plain["decimate"][1].shape[0] > 0
    assert plain["atlas"][1] > 0 and plain["atlas"][2] == 0


def test_mesh_export_footprint_sample_like_256(ops):
    """The sample-like field at 256^3 (6.9 M faces out of marching cubes), the shipped cleanup and the 100 000-face decimation on
    its output, and the bake at the shipped 2048 x 2048 size."""
    from topia_xl_amd import mesh as M
    field = synth.sample_field(DEV)
    plain = fp.hold(lambda g: _mesh_chain(M, g, field, 256, (2048, 2048), M.DECIMATE_TARGET))
    assert (plain["raw"]["v"].shape[0], plain["raw"]["f"].shape[0]) == (3517979, 6917478)        # DESIGN.md's mesh tables
    assert (plain["clean"][0].shape[0], plain["clean"][1].shape[0]) == (106412, 125061)
    assert plain["decimate"][1].shape[0] == 100191 and dict(plain["decimate stats"])["stalled"]


# ------------------------------------------------------------------------------------------------ no hidden state
def _aba(A, B):
    """A, then B, then A: both results of A are bit-identical - on the default stream and on another one."""
    streams = [torch.cuda.current_stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            first = A()
            B()
            second = A()
        s.synchronize()
        assert not fp.differences(first, second), fp.differences(first, second)
    return first


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_state_survives_between_calls(ops, dtype):
    """The library keeps no state between calls that changes what a later call does: a packed convolution, attention and a fold
    consumer, each run as A, B (another shape of the same entry point, and an entry point of another family), A."""
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    # a packed convolution
    xa, xb = TC._cl_rand(1, 3, 64, 256, dtype), TC._cl_rand(2, 300, 512, 32, dtype)
    wa, ba = _conv_weights(256, 256, dtype)
    wb, bb = _conv_weights(32, 32, dtype)
    pa, pb = ops.pack_conv3(wa, 256), ops.pack_conv3(wb, 32)
    if pa is not None:
        _aba(lambda: ops.conv3d_k3(xa, wa, ba, 4, Wp=pa), lambda: (ops.conv3d_k3(xb, wb, bb, 8, Wp=pb), ops.cast16(xb.float(), dtype)))
    # attention
    qa, ka, va = TC._qkv(3, 1, 300, 1000, 2, 72, 1.0, dtype)
    qb, kb, vb = TC._qkv(4, 2, 300, 500, 2, 32, 4.0, dtype)
    _aba(lambda: ops.memory_efficient_attention(qa, ka, va),
         lambda: (ops.memory_efficient_attention(qb, kb, vb), ops.linear(qa.view(300, 144), rnd(5, 288, 144, dtype=dtype), None)))
    # a fold consumer (the 128 x 144 and the 256 x 288 kernel)
    if TF._fold_kernels_selectable(ops):
        sa, _ = _site(ops, dtype, 4, TF.CASES[4])                  # linear, B = 1, n = 333
        sa = dict(a16=sa.a16.clone(), W=sa.W.clone(), part=sa.part.clone(), u=sa.u.clone(), v=sa.v.clone(), c=sa.center.clone(), M=sa.M)
        sb, kinds = _site(ops, dtype, 9, TF.CASES[9])              # heads, B = 2, n = 2048

        def A():
            co = torch.empty(sa["M"], 2, device=DEV)
            out = ops.linear_fold(sa["a16"], sa["W"], torch.empty(sa["M"], 4608, dtype=dtype, device=DEV), sa["part"], sa["u"], sa["v"],
                                  sa["c"], co, TF.EPS, act=1)
            return out, co

        def B():
            role = {HEADS_ROWS: "q", HEADS_KROWS: "k", HEADS_VT: None}
            dsts = [ops.alloc_heads(2, TF.H, 2048, TF.DH, k, dtype, DEV, 256, role[k]) for k in kinds]
            ops.linear_heads_fold(sb.a16, sb.W, 2048, TF.H, TF.DH, kinds, dsts, dsts[0].shape[2], sb.part, sb.u, sb.v, sb.center,
                                  sb.center_out, TF.EPS)
        _aba(A, B)
        _SITES.clear()
