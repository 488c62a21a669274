"""The stream rule of include/primx_hip.h - "Work is enqueued on `stream` and is asynchronous with respect to the host" - held
entry point by entry point with tests/streamorder.py on the MI355X.

Every case of CASES runs on ONE side stream while stream 0 and the side stream are both blocked, with operands that are
produced late, inside footprint.guarded(0xFF), and is judged for (a) order, (b) conclusiveness and (c) asynchrony as
tests/streamorder.py describes.  A case names the entry points it is there for (`declares`); while it runs the `primx_*`
functions of the loaded library are wrapped and the test asserts that each declared one was called.
tests/test_streamorder_cpu.py reads the same table without a GPU and asserts that every prototype of the header that takes a
`void* stream` is declared by some case, and nothing else.

MUST_SYNC / FIRST_CALL_MAY_SYNC are the one table of cases whose hosts synchronise by design, each with its reason; (c) is asked
of every other case, and of the second call of the FIRST_CALL_MAY_SYNC ones.
A sampling loop is probed per step (the loop itself uploads its coefficient table before the first step and reads the overflow
guard back after the last).

Streams: `S` for the cases, `S2` for the second call of the overlap pairs and the third-stream control.  With the DiT's own
side stream (`cfg_streams`) a process has three streams besides stream 0.  No case provokes a fault: the positive controls are
plain torch ops on the wrong stream, a plain synchronize and a short blocker."""
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import streamorder as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
BOTH = (F16, BF16)

Case = namedtuple("Case", "name declares build dtypes")
CASES = {}

# ---------------------------------------------------------------------------------------------- hosts that synchronise by design
_READBACK = "the C host reads the index check back (csrc/meshfield.hip read_flag) before it returns"
MUST_SYNC = {
    "mesh_field_query": _READBACK + " and before it launches the query kernel",
    "face_areas_surface_points": _READBACK,
    "mesh_to_primitives": "area_cdf sums on the host; the index checks of the three meshfield hosts; normalize_vertices reads the extent",
    "mcubes": "marching_cubes reads (nverts, ntris) back between count and emit: exact output sizes",
    "mesh_export_48": "extract_mesh, clean_mesh, decimate_mesh and the bake read their counts back after every counting stage",
    "clean_mesh_nonmanifold": "clean_mesh reads the counts of every phase back (meshclean's scan totals size the next phase's arrays)",
}
# ... and cases on a fresh module instance whose FIRST call may synchronise while it fills the instance's caches: they make a
# second call and (c) is asked of that one
FIRST_CALL_MAY_SYNC = {
    "primsdf_query": "the first query of a PrimSDF instance uploads its linspace table with a blocking copy",
    "vae_decode": "VAE.packed reads the two scalars of post_quant_conv back when it packs the instance's weights",
    "vae_encode": "the first encode of an instance packs its weights (as vae_decode)",
}


def twice(fn, probe):
    """[first call, second call] of `fn`; the probe brackets the second (FIRST_CALL_MAY_SYNC)."""
    first = fn()
    probe.step()
    second = fn()
    probe.returned()
    return [first, second]


def case(name, declares, dtypes=(None,)):
    def deco(fn):
        assert name not in CASES
        CASES[name] = Case(name, tuple(declares), fn, tuple(dtypes))
        return fn
    return deco


def declared():
    return sorted({n for c in CASES.values() for n in c.declares})


# ---------------------------------------------------------------------------------------------- fixtures and helpers
@pytest.fixture(scope="module")
def E():
    """The package, its ops, ONE side stream for every case of the module, a second one, and the calibrated blocker."""
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd
    from topia_xl_amd import _lib, ops
    env = namedtuple("Env", "pkg ops lib S S2 blocker")(topia_xl_amd, ops, _lib.load(), torch.cuda.Stream(), torch.cuda.Stream(),
                                                         so.Blocker())
    print(f"streamorder blocker: {env.blocker.cycles_per_ms:.0f} sleep cycles per ms")
    return env


@pytest.fixture
def called(E, monkeypatch):
    """Names of the primx_* functions of the loaded library that were called during the test."""
    from topia_xl_amd._lib import SIGNATURES
    seen = set()

    def wrap(name, fn):
        def wrapped(*a):
            seen.add(name)
            return fn(*a)
        return wrapped
    for name in SIGNATURES:
        if hasattr(E.lib, name):
            monkeypatch.setattr(E.lib, name, wrap(name, getattr(E.lib, name)))
    return seen


def R(k, tag, *shape, scale=1.0, offset=0.0, dtype=F32):
    """Seeded values for input `tag` of variant k (0: the measured values, 1: the warm-up's)."""
    import zlib
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(tag.encode()) % 100000 + 7919 * k)
    return (torch.randn(*shape, device=DEV, generator=g) * scale + offset).to(dtype).contiguous()


def _nan(*shape, dtype=F32, device=DEV):
    """A destination made by the test itself: NaN, like the package's own torch.empty buffers under the guard."""
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _kinds():
    from topia_xl_amd._lib import HEADS_KROWS, HEADS_ROWS, HEADS_VT
    return HEADS_ROWS, HEADS_KROWS, HEADS_VT


def _heads_dsts(ops, B, H, n, dh, kinds, dtype, pad):
    ROWS, KROWS, VT = _kinds()
    role = {ROWS: "q", KROWS: "k", VT: None}
    return [ops.alloc_heads(B, H, n, dh, k, dtype, DEV, pad, role[k]) for k in kinds]


def _fold_skip(ops):
    from tests import test_hip_fold_contract as TF
    if not TF._fold_kernels_selectable(ops):
        pytest.skip("a kernel-selection switch removes a tile shape of the fold kernels")


# ---------------------------------------------------------------------------------------------- GEMM family
LINEAR_SHAPES = [(256, 256, 64), (300, 136, 1152), (700, 288, 128), (4096, 4608, 64)]   # generic tile, loader wave, 700 rows, 256 x 288 tile


@case("linear", ["primx_linear"], BOTH)
def _linear(E, dtype):
    def make(k):
        d = {}
        for j, (M, N, K) in enumerate(LINEAR_SHAPES):
            d[f"A{j}"], d[f"W{j}"] = R(k, f"lin.A{j}", M, K, dtype=dtype), R(k, f"lin.W{j}", N, K, scale=K ** -0.5, dtype=dtype)
            d[f"b{j}"] = R(k, f"lin.b{j}", N, scale=0.3, dtype=dtype)
        return d

    def call(ctx, i, probe):
        out = {}
        for j in range(len(LINEAR_SHAPES)):
            A, W, b = i[f"A{j}"], i[f"W{j}"], i[f"b{j}"]
            out[f"{j} plain"] = E.ops.linear(A, W, b)
            out[f"{j} gelu"] = E.ops.linear(A, W, b, act=1, carry=i["W0"])          # (a carried prefetch range)
            out[f"{j} scaled"] = E.ops.linear(A, W, None, out_scale=72 ** -0.5)
        return out
    return make, call, None


@case("linear_gate_residual", ["primx_linear_gate_residual", "primx_linear_gate_residual_ln"], BOTH)
def _gate(E, dtype):
    shapes = [(300, 288, 192, 150), (947, 1152, 192, 300)]       # (M, N, K, rows per batch): plain; LayerNorm in the tail / second launch

    def make(k):
        d = {}
        for j, (M, N, K, rpb) in enumerate(shapes):
            nb = (M + rpb - 1) // rpb
            d[f"A{j}"], d[f"W{j}"] = R(k, f"g.A{j}", M, K, dtype=dtype), R(k, f"g.W{j}", N, K, scale=K ** -0.5, dtype=dtype)
            d[f"b{j}"], d[f"mod{j}"] = R(k, f"g.b{j}", N, scale=0.3, dtype=dtype), R(k, f"g.mod{j}", nb, 3 * N, scale=0.5, dtype=dtype)
            d[f"x{j}"], d[f"x{j}b"] = R(k, f"g.x{j}", M, N, scale=4.0), R(k, f"g.x{j}", M, N, scale=4.0)
        d["sync"] = torch.zeros(E.ops.ln_sync_words(shapes[1][0]), dtype=torch.int32, device=DEV)
        return d

    def call(ctx, i, probe):
        out = {}
        (M, N, K, rpb), mod = shapes[0], i["mod0"]
        E.ops.linear_gate_residual(i["A0"], i["W0"], i["b0"], mod[:, :N], i["x0"], rpb, carry=i["W1"])
        out["x plain"] = i["x0"]
        (M, N, K, rpb), mod = shapes[1], i["mod1"]
        gate, shift, scale = mod[:, :N], mod[:, N:2 * N], mod[:, 2 * N:]          # row stride 3 N
        ln1, ln2 = (_nan(M, N, dtype=dtype, device=DEV) for _ in range(2))
        E.ops.linear_gate_residual(i["A1"], i["W1"], i["b1"], gate, i["x1"], rpb, ln=(shift, scale, ln1, 1e-6, i["sync"]))
        E.ops.linear_gate_residual(i["A1"], i["W1"], i["b1"], gate, i["x1b"], rpb, ln=(shift, scale, ln2, 1e-6, None))   # two launches
        out.update({"x tail": i["x1"], "ln tail": ln1, "sync": i["sync"], "x two launches": i["x1b"], "ln two launches": ln2})
        return out
    return make, call, None


@case("linear_heads", ["primx_linear_heads"], BOTH)
def _heads(E, dtype):
    ROWS, KROWS, VT = _kinds()
    B, n, H, dh, K, n_rep = 2, 70, 4, 72, 64, 3

    def make(k):
        D = H * dh
        return {"A": R(k, "h.A", B * n, K, dtype=dtype), "W": R(k, "h.W", 3 * D, K, scale=K ** -0.5, dtype=dtype),
                "b": R(k, "h.b", 3 * D, scale=0.3, dtype=dtype),
                "Wr": R(k, "h.Wr", n_rep * 2 * D, K, scale=K ** -0.5, dtype=dtype), "br": R(k, "h.br", n_rep * 2 * D, scale=0.3, dtype=dtype)}

    def call(ctx, i, probe):
        d3 = _heads_dsts(E.ops, B, H, n, dh, [ROWS, KROWS, VT], dtype, 128)
        E.ops.linear_heads(i["A"], i["W"], i["b"], n, H, dh, [ROWS, KROWS, VT], d3, d3[0].shape[2], scale0=dh ** -0.5, carry=i["Wr"])
        dr = _heads_dsts(E.ops, n_rep * B, H, n, dh, [KROWS, VT], dtype, 64)
        E.ops.linear_heads(i["A"], i["Wr"], i["br"], n, H, dh, [KROWS, VT], dr, dr[0].shape[2], n_rep=n_rep, rep_batches=B)
        return {"three kinds": d3, "repeated": dr}
    return make, call, None


@case("linear_residual", ["primx_linear_residual"], BOTH)
def _residual(E, dtype):
    M, N, K = 300, 288, 128

    def make(k):
        return {"A": R(k, "r.A", M, K, dtype=dtype), "W": R(k, "r.W", N, K, scale=K ** -0.5, dtype=dtype),
                "b": R(k, "r.b", N, scale=0.3, dtype=dtype), "res": R(k, "r.res", M, N, scale=0.3, dtype=dtype)}

    def call(ctx, i, probe):
        return [E.ops.linear_residual(i["A"], i["W"], i["b"], i["res"], 0.70710678), E.ops.linear_residual(i["A"], i["W"], i["b"], None, 1.0)]
    return make, call, None


def _f32out_case(E, dtype, grouped):
    M, K, NS = 16, 1152, (1152, 3456, 288)

    def make(k):
        d = {}
        for j, N in enumerate(NS):
            d[f"A{j}"], d[f"W{j}"] = R(k, f"fo.A{j}", M, K, dtype=dtype), R(k, f"fo.W{j}", N, K, scale=K ** -0.5, dtype=dtype)
            d[f"b{j}"] = R(k, f"fo.b{j}", N, scale=0.3, dtype=dtype)
        return d

    def call(ctx, i, probe):
        if not grouped:
            return [E.ops.linear_f32out(i[f"A{j}"], i[f"W{j}"], i[f"b{j}"], _nan(M, N, device=DEV), 8) for j, N in enumerate(NS)]
        probs = [(i[f"A{j}"], i[f"W{j}"], i[f"b{j}"], _nan(M, N, device=DEV)) for j, N in enumerate(NS)]
        assert E.ops.linear_f32out_group(probs, 8)
        return [p[3] for p in probs]
    return make, call, None


@case("linear_f32out", ["primx_linear_f32out"], BOTH)
def _f32out(E, dtype):
    return _f32out_case(E, dtype, False)


@case("linear_f32out_group", ["primx_linear_f32out_group"], BOTH)
def _f32out_group(E, dtype):
    """The problem table goes up from pinned memory with a non-blocking copy: the host does not wait."""
    if not E.ops._lib.f32out_group_available() or os.environ.get("PRIMX_UV_GROUP") == "0":
        pytest.skip("the build or PRIMX_UV_GROUP=0 removes primx_linear_f32out_group")
    return _f32out_case(E, dtype, True)


_SITE = {}


def _site(E, dtype, idx, k):
    """The consumer operands of fold-contract case `idx`, made by the real producer on the default stream (variant k)."""
    from tests import test_hip_fold_contract as TF
    key = (dtype, idx, k)
    if key not in _SITE:
        c = TF.CASES[idx]
        kinds = c.get("kinds", "qkv")
        Nc = c.get("Nc", len(kinds) * TF.H * TF.DH if c["form"] in ("heads", "pair") else 4608)
        regime = {r: c[r] for r in ("ratio", "spread", "offset", "const_rows", "massive", "neg1_cols") if r in c}
        s = TF.Site(E.ops, 900 + idx + 50 * k, dtype, c["B"], c["n"], Nc, **regime)
        _SITE[key] = {n: getattr(s, n).contiguous().clone() for n in ("a16", "W", "part", "u", "v", "center")}
    return dict(_SITE[key])


@case("fold_producer", ["primx_linear_gate_residual_fold", "primx_row_stats"], BOTH)
def _fold_producer(E, dtype):
    from tests import test_hip_fold_contract as TF
    _fold_skip(E.ops)
    shapes = [(TF.CASES[4]["B"], TF.CASES[4]["n"]), (2, 300)]
    D, Kp = TF.D, 128

    def make(k):
        d = {}
        for j, (B, n) in enumerate(shapes):
            M = B * n
            x = R(k, f"fp.x{j}", M, D, scale=2.0)
            d[f"A{j}"], d[f"W{j}"] = R(k, f"fp.A{j}", M, Kp, dtype=dtype), R(k, f"fp.W{j}", D, Kp, scale=Kp ** -0.5, dtype=dtype)
            d[f"b{j}"], d[f"mod{j}"] = R(k, f"fp.b{j}", D, scale=0.3, dtype=dtype), R(k, f"fp.m{j}", B, 3 * D, scale=0.1, dtype=dtype)
            d[f"x{j}"], d[f"c{j}"] = x, torch.stack([x.mean(-1), 1.0 / torch.sqrt(x.var(-1) + 1e-6)], -1).contiguous()
        return d

    def call(ctx, i, probe):
        out = {}
        for j, (B, n) in enumerate(shapes):
            M, mod = B * n, i[f"mod{j}"]
            a16, part = _nan(M, D, dtype=dtype, device=DEV), _nan(M, D // 144, 2, device=DEV)
            E.ops.linear_gate_residual_fold(i[f"A{j}"], i[f"W{j}"], i[f"b{j}"], mod[:, D:2 * D], i[f"x{j}"], n, mod[:, 2 * D:], i[f"c{j}"],
                                            a16, part, carry=i["W0"])
            out[j] = [i[f"x{j}"], a16, part, E.ops.row_stats(i[f"x{j}"], 1e-6, _nan(M, 2, device=DEV))]
        return out
    return make, call, None


@case("fold_consumers", ["primx_linear_fold", "primx_linear_heads_fold", "primx_linear_heads_fold_pair"], BOTH)
def _fold_consumers(E, dtype):
    from tests import test_hip_fold_contract as TF
    _fold_skip(E.ops)
    ROWS, KROWS, VT = _kinds()
    LIN, HEADS, PAIR = 4, 0, 11                                    # TF.CASES: linear (1 x 333), heads qk (2 x 300), the pair launch (2 x 2048)
    Lk, L, Dc = 1536, 1370, 768

    def make(k):
        d = {}
        for idx in (LIN, HEADS, PAIR):
            d.update({f"{idx}.{n}": t for n, t in _site(E, dtype, idx, k).items()})
        y = torch.zeros(Lk, Dc, device=DEV)
        y[:L] = R(k, "fc.y", L, Dc)
        d["y16"], d["Wkv"] = y.to(dtype), R(k, "fc.Wkv", 2 * TF.D, Dc, scale=Dc ** -0.5, dtype=dtype)
        d["bkv"] = R(k, "fc.bkv", 2 * TF.D, scale=0.3, dtype=dtype)
        return d

    def call(ctx, i, probe):
        def site(idx):
            return [i[f"{idx}.{n}"] for n in ("a16", "W", "part", "u", "v", "center")]
        out = {}
        a16, W, part, u, v, cen = site(LIN)
        M = a16.shape[0]
        co = _nan(M, 2, device=DEV)
        out["linear"] = [E.ops.linear_fold(a16, W, _nan(M, W.shape[0], dtype=dtype, device=DEV), part, u, v, cen, co, TF.EPS, act=1,
                                           carry=i["Wkv"]), co]
        a16, W, part, u, v, cen = site(HEADS)
        c, co = TF.CASES[HEADS], _nan(a16.shape[0], 2, device=DEV)
        d = _heads_dsts(E.ops, c["B"], TF.H, c["n"], TF.DH, [ROWS, KROWS], dtype, 128)
        E.ops.linear_heads_fold(a16, W, c["n"], TF.H, TF.DH, [ROWS, KROWS], d, d[0].shape[2], part, u, v, cen, co, TF.EPS, scale0=TF.S0,
                                carry=i["Wkv"])
        out["heads"] = [d, co]
        a16, W, part, u, v, cen = site(PAIR)
        c, co = TF.CASES[PAIR], _nan(a16.shape[0], 2, device=DEV)
        d = _heads_dsts(E.ops, c["B"], TF.H, c["n"], TF.DH, [ROWS, KROWS, VT], dtype, 256)
        kv = [E.ops.alloc_heads(1, TF.H, L, TF.DH, kd, dtype, DEV, 256, r) for kd, r in ((KROWS, "k"), (VT, None))]
        fold = dict(A=a16, W=W, rows_per_batch=c["n"], heads=TF.H, dh=TF.DH, kinds=[ROWS, KROWS, VT], dsts=d, n_pad=d[0].shape[2], part=part,
                    u=u, v=v, center=cen, center_out=co, eps=TF.EPS)
        E.ops.linear_heads_fold_pair(fold, i["y16"], i["Wkv"], i["bkv"], Lk, TF.H, TF.DH, [KROWS, VT], kv, kv[0].shape[2])
        out["pair"] = [d, kv, co]
        return out
    return make, call, None


@case("fp32_gemms", ["primx_linear_f32", "primx_gemm_f32"])
def _fp32_gemms(E, dtype):
    lin = [(130, 70, 12), (1, 70, 12), (8, 7, 588)]                # the tiled kernel; the few-row kernel at M = 1 and 8
    M, N, K, rpb = 300, 96, 68, 150

    def make(k):
        d = {"A": R(k, "g32.A", M, K), "W": R(k, "g32.W", N, K, scale=K ** -0.5), "b": R(k, "g32.b", N, scale=0.1),
             "gate": R(k, "g32.gate", 2, 9 * N), "x": R(k, "g32.x", M, N)}
        for j, (m, n, kk) in enumerate(lin):
            d[f"A{j}"], d[f"W{j}"], d[f"b{j}"] = R(k, f"l32.A{j}", m, kk), R(k, f"l32.W{j}", n, kk, scale=kk ** -0.5), R(k, f"l32.b{j}", n)
        return d

    def call(ctx, i, probe):
        out = {"plain": E.ops.gemm_f32(i["A"], i["W"], i["b"], act=1, out_scale=0.5)}
        E.ops.gemm_f32(i["A"], i["W"], i["b"], out=i["x"], gate=i["gate"][:, 2 * N:3 * N], rows_per_batch=rpb)
        out["gated in place"] = i["x"]
        for j, (m, n, kk) in enumerate(lin):
            out[f"linear_f32 {m}"] = [E.ops.linear_f32(i[f"A{j}"], i[f"W{j}"], i[f"b{j}"]), E.ops.linear_f32(i[f"A{j}"], i[f"W{j}"], None, act_out=1)]
        o1, o2 = _nan(130, 70, device=DEV), _nan(130, 70, device=DEV)
        E.ops.linear_f32(i["A0"], i["W0"], i["b0"], out=o1, out2=o2)
        out["two destinations"] = [o1, o2]
        return out
    return make, call, None


# ---------------------------------------------------------------------------------------------- attention
def _qkv(k, tag, B, Mq, Mk, H, dh, dtype):
    return {"q": R(k, tag + ".q", B, Mq, 3, H, dh, dtype=dtype), "kv": R(k, tag + ".kv", B, Mk, 3, H, dh, dtype=dtype)}


@case("attention", ["primx_pack_heads", "primx_attention"], BOTH)
def _attention(E, dtype):
    ROWS, KROWS, VT = _kinds()
    shapes = [(1, 300, 1370, 2, 72, None), (1, 100, 1, 2, 72, None), (7, 37, 64, 3, 32, 64)]   # the last: 7 x 3 problems of the 64-token kernel

    def make(k):
        d = {}
        for j, (B, Mq, Mk, H, dh, pad) in enumerate(shapes):
            d.update({f"{n}{j}": t for n, t in _qkv(k, f"at{j}", B, Mq, Mk, H, dh, dtype).items()})
        return d

    def call(ctx, i, probe):
        out = {}
        for j, (B, Mq, Mk, H, dh, pad) in enumerate(shapes):
            q, kk, v = i[f"q{j}"][:, :, 0], i[f"kv{j}"][:, :, 1], i[f"kv{j}"][:, :, 2]       # strided sources: views of fused buffers
            Qp = E.ops.pack_heads(q, ROWS, pad or E.ops.BQ, "q")
            Kp = E.ops.pack_heads(kk, KROWS, pad or E.ops.BKV, "k")
            Vt = E.ops.pack_heads(v, VT, pad or E.ops.BKV)
            out[j] = [Qp, Kp, Vt, E.ops.attention(Qp, Kp, Vt, Mq, Mk, dh, dh ** -0.5)]
        assert out[2][0].shape[2] == 64 and out[2][1].shape[2] == 64                            # the form attn64_kernel takes
        return out
    return make, call, None


@case("attention_bcast", ["primx_attention_bcast"], BOTH)
def _attention_bcast(E, dtype):
    ROWS, KROWS, VT = _kinds()
    shapes = [(2, 1, 300, 1370, 4, 72), (3, 0, 256, 1370, 2, 72)]    # (B, b_from, Mq, Mk, H, dh)

    def make(k):
        d = {}
        for j, (B, b_from, Mq, Mk, H, dh) in enumerate(shapes):
            d[f"q{j}"], d[f"k{j}"] = R(k, f"ab.q{j}", B, Mq, H, dh, dtype=dtype), R(k, f"ab.k{j}", max(b_from, 1), Mk, H, dh, dtype=dtype)
            d[f"v{j}"] = R(k, f"ab.v{j}", max(b_from, 1), Mk, H, dh, dtype=dtype)
            d[f"kr{j}"], d[f"vr{j}"] = R(k, f"ab.kr{j}", 1, 1, H, dh, dtype=dtype), R(k, f"ab.vr{j}", 1, 1, H, dh, dtype=dtype)
        return d

    def call(ctx, i, probe):
        out = {}
        for j, (B, b_from, Mq, Mk, H, dh) in enumerate(shapes):
            nb = E.ops.bcast_keys(Mk)
            Qp = E.ops.pack_heads(i[f"q{j}"], ROWS, E.ops.BQ, "q")
            Kb = E.ops.pack_heads(i[f"kr{j}"].expand(1, nb, H, dh).contiguous(), KROWS, E.ops.BKV, "k")
            Vb = E.ops.pack_heads(i[f"vr{j}"].expand(1, nb, H, dh).contiguous(), VT, E.ops.BKV)
            Kp = E.ops.pack_heads(i[f"k{j}"], KROWS, E.ops.BKV, "k") if b_from else None
            Vt = E.ops.pack_heads(i[f"v{j}"], VT, E.ops.BKV) if b_from else None
            out[j] = E.ops.attention(Qp, Kp, Vt, Mq, Mk, dh, dh ** -0.5, bcast=(Kb, Vb))
        return out
    return make, call, None


@case("attention_f32", ["primx_attention_f32"])
def _attention_f32(E, dtype):
    B, Nq, Nk, H, dh = 3, 130, 77, 4, 72

    def make(k):
        return {"q": R(k, "a32.q", B, H, Nq, dh), "k": R(k, "a32.k", 1, Nk, H, dh), "v": R(k, "a32.v", B, Nk, H, dh + 8)}

    def call(ctx, i, probe):
        q, kk, v = i["q"].permute(0, 2, 1, 3), i["k"].expand(B, Nk, H, dh), i["v"][..., :dh]   # three differently strided views
        return E.ops.attention_f32(q, kk, v)
    return make, call, None


# ---------------------------------------------------------------------------------------------- row kernels
@case("layernorm_modulate", ["primx_layernorm_modulate", "primx_layernorm_modulate_f32", "primx_prefetch"], BOTH)
def _layernorm(E, dtype):
    shapes = [(1152, 600, 256), (200, 70, 35)]                     # the row-in-registers kernel and the general one

    def make(k):
        d = {"w": R(k, "ln.w", 777, 64, dtype=dtype)}
        for j, (D, rows, rpb) in enumerate(shapes):
            d[f"x{j}"], d[f"mod{j}"] = R(k, f"ln.x{j}", rows, D, scale=3.0, offset=0.7), R(k, f"ln.m{j}", (rows + rpb - 1) // rpb, 3 * D, scale=0.4)
            d[f"mod16{j}"] = d[f"mod{j}"].to(dtype)
        return d

    def call(ctx, i, probe):
        out = {}
        E.ops.prefetch(i["w"], torch.cuda.current_stream())         # an explicit stream argument: reads, writes nothing
        for j, (D, rows, rpb) in enumerate(shapes):
            m16, m32 = i[f"mod16{j}"], i[f"mod{j}"]
            out[j] = [E.ops.layernorm_modulate(i[f"x{j}"], m16[:, :D], m16[:, 2 * D:], rpb, _nan(rows, D, dtype=dtype, device=DEV),
                                               prefetch=(i["w"],)),
                      E.ops.layernorm_modulate_f32(i[f"x{j}"], m32[:, :D], m32[:, 2 * D:], rpb, 1e-6)]
        return out
    return make, call, None


@case("row_ops", ["primx_timestep_embedding", "primx_point_features", "primx_silu_cast", "primx_cast16", "primx_cfg_combine",
                  "primx_silu_f32", "primx_vit_tokens", "primx_latent_denorm", "primx_latent_norm"])
def _row_ops(E, dtype):
    n = 2048 * 256 + 1                                             # one element past the grid cap of the grid-stride loops

    def make(k):
        return {"t": torch.tensor([1, 40, 500, 960, 999, 7, 3], device=DEV) + k, "xs": R(k, "ro.xs", 301, 9),
                "fr": torch.pow(2.0, torch.arange(8, device=DEV).float()) * (3.14159 + k), "x": R(k, "ro.x", n, scale=2.0),
                "mo16": R(k, "ro.mo", 2, 4097, dtype=F16), "mo32": R(k, "ro.mo32", 2, 4097),
                "patches": R(k, "ro.p", 2, 37, 96), "cls": R(k, "ro.cls", 96), "pos": R(k, "ro.pos", 38, 96), "reg": R(k, "ro.reg", 4, 96),
                "lat": R(k, "ro.lat", 3, 5, 68), "mean": R(k, "ro.mean", 68, scale=0.5), "std": R(k, "ro.std", 68, scale=0.2).abs() + 0.5}

    def call(ctx, i, probe):
        o = E.ops
        srt, z = o.latent_denorm(i["lat"], i["mean"], i["std"], 1.3)
        return {"timestep_embedding": o.timestep_embedding(i["t"], 256), "point_features": o.point_features(i["xs"][:, :5], i["fr"]),
                "silu_cast": [o.silu_cast(i["x"], dt) for dt in BOTH], "cast16": [o.cast16(i["x"], dt) for dt in BOTH],
                "cfg_combine": [o.cfg_combine(i["mo16"], 6.0), o.cfg_combine(i["mo32"], 6.0)], "silu_f32": o.silu_f32(i["x"]),
                "vit_tokens": [o.vit_tokens(i["patches"], i["cls"], i["pos"], None), o.vit_tokens(i["patches"], i["cls"], i["pos"], i["reg"])],
                "latent_denorm": [srt, z], "latent_norm": o.latent_norm(srt, z, i["mean"], i["std"], 1.3)}
    return make, call, None


@case("diffusion_steps", ["primx_diffusion_step", "primx_q_sample", "primx_diffusion_reverse_step", "primx_diffusion_step_keep"],
      (F16, BF16, F32))
def _diffusion_steps(E, dtype):
    d = E.pkg.create_diffusion("ddim25", noise_schedule="squaredcos_cap_v2", parameterization="v")
    shape = (2, 97, 68)

    def make(k):
        keep = (R(k, "ds.keep", 2, 97) > 0).to(torch.uint8)
        return {"coef": torch.from_numpy(d.step_coefficients(0.5 + 0.1 * k)).to(DEV), "x": R(k, "ds.x", *shape),
                "mo": R(k, "ds.mo", 2, 97, 136, dtype=dtype), "noise": R(k, "ds.n", *shape), "known": R(k, "ds.kn", *shape),
                "kn": R(k, "ds.kk", *shape), "keep": keep}

    def call(ctx, i, probe):
        o, x, mo, coef, noise = E.ops, i["x"], i["mo"], i["coef"], i["noise"]
        return {"ddim": o.diffusion_step(x, mo, coef, 7, mean_type=2, var_type=3, ancestral=False, clip_denoised=False, noise=noise),
                "ancestral": o.diffusion_step(x, mo, coef, 24, mean_type=2, var_type=3, ancestral=True, clip_denoised=False, noise=noise),
                "q_sample": o.q_sample(x, noise, coef, 7), "reverse": o.diffusion_reverse_step(x, mo, coef, 7, mean_type=2, clip_denoised=True),
                "keep": o.diffusion_step_keep(x, mo, coef, 7, mean_type=2, var_type=3, ancestral=False, clip_denoised=True, noise=noise,
                                              known=i["known"], known_noise=i["kn"], keep=i["keep"])}
    return make, call, None


# ---------------------------------------------------------------------------------------------- VAE kernels
def _conv_w(k, tag, Cout, Cin, dtype):
    from topia_xl_amd.vae import _conv_weight_as_gemm
    return _conv_weight_as_gemm(R(k, tag, Cout, Cin, 3, 3, 3, scale=(27 * Cin) ** -0.5), dtype).contiguous()


@case("vae_convs", ["primx_groupnorm_silu", "primx_conv3d_k3", "primx_conv3d_s4_pack", "primx_conv3d_s4_packed", "primx_conv3d_s8_pack",
                    "primx_conv3d_s8_packed", "primx_conv3d_s8c32_pack", "primx_conv3d_s8c32_packed"], BOTH)
def _vae_convs(E, dtype):
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the implicit GEMM")
    P = 3
    convs = [(256, 256, 4, "s4"), (256, 32, 8, "s8"), (32, 32, 8, "s8c32"), (64, 48, 4, None)]

    def make(k):
        d = {"gx": R(k, "vc.gx", P, 64, 256, scale=1.3, offset=0.2, dtype=dtype), "gg": R(k, "vc.gg", 256, scale=0.2, offset=1.0),
             "gb": R(k, "vc.gb", 256, scale=0.2), "g32": R(k, "vc.g32", 32, scale=0.2, offset=1.0), "b32": R(k, "vc.b32", 32, scale=0.2)}
        for j, (Cin, Cout, S, kind) in enumerate(convs):
            d[f"x{j}"], d[f"w{j}"] = R(k, f"vc.x{j}", P, S ** 3, Cin, dtype=dtype), _conv_w(k, f"vc.w{j}", Cout, Cin, dtype)
            d[f"b{j}"], d[f"r{j}"] = R(k, f"vc.b{j}", Cout, scale=0.2, dtype=dtype), R(k, f"vc.r{j}", P, S ** 3, Cout, dtype=dtype)
        return d

    def call(ctx, i, probe):
        o = E.ops
        out = {"groupnorm_silu": o.groupnorm_silu(i["gx"], i["gg"], i["gb"], 32, 1e-5, True)}
        for j, (Cin, Cout, S, kind) in enumerate(convs):
            x, w, b, r = i[f"x{j}"], i[f"w{j}"], i[f"b{j}"], i[f"r{j}"]
            wp = o.pack_conv3(w, Cin)                                # the weight image is made on the side stream as well
            assert (wp is not None and wp.kind == kind) if kind else wp is None
            out[j] = [o.conv3d_k3(x, w, b, S, res=r, res_scale=0.5 ** 0.5, Wp=wp)]
            if kind == "s8c32":
                out[j] += [wp.Wp, o.conv3d_k3(x, w, b, S, res=r, res_scale=0.5 ** 0.5, Wp=wp, gn=(i["g32"], i["b32"], 1e-5))]
        return out
    return make, call, None


@case("vae_upsample_and_ends", ["primx_conv3d_s8_fused", "primx_convtranspose_s4_pack", "primx_convtranspose_s4_packed",
                                "primx_convtranspose_k2s2", "primx_conv_in", "primx_vae_output"], BOTH)
def _vae_up(E, dtype):
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the implicit GEMM")
    P = 3

    def make(k):
        return {"x": R(k, "vu.x", P, 64, 256, dtype=dtype), "wt": R(k, "vu.wt", 8 * 256, 256, scale=1 / 16, dtype=dtype),
                "b": R(k, "vu.b", 256, scale=0.3, dtype=dtype), "wk": _conv_w(k, "vu.wk", 32, 256, dtype), "b1": R(k, "vu.b1", 32, scale=0.2, dtype=dtype),
                "wsc": R(k, "vu.wsc", 32, 256, scale=1 / 16, dtype=dtype), "bsc": R(k, "vu.bsc", 32, scale=0.2, dtype=dtype),
                "gam": R(k, "vu.g", 256, scale=0.2, offset=1.0), "bet": R(k, "vu.be", 256, scale=0.2),
                "xs": R(k, "vu.xs", P, 64, 64, dtype=dtype), "wts": R(k, "vu.wts", 8 * 48, 64, scale=1 / 8, dtype=dtype),
                "bs": R(k, "vu.bs", 48, scale=0.3, dtype=dtype), "z": R(k, "vu.z", P, 64), "wi": R(k, "vu.wi", 256, 27, scale=0.2),
                "bi": R(k, "vu.bi", 256, scale=0.2), "y": R(k, "vu.y", P, 512, 6, dtype=dtype)}

    def call(ctx, i, probe):
        o = E.ops
        wp = o.pack_convt_s4(i["wt"])
        h8, part = o.convtranspose_k2s2(i["x"], i["wt"], i["b"], 4, Wp=wp, want_stats=True)
        wp3 = o.pack_conv3(i["wk"], 256, Wsc=i["wsc"])
        return {"packed": [wp, h8, part, o.group_stats(part, i["b"], 1e-5)],
                "fused": [wp3.Wp, o.conv3d_s8_fused(h8, wp3, i["b1"], part, i["b"], i["gam"], i["bet"], 1e-5, i["bsc"])],
                "gemm form": o.convtranspose_k2s2(i["xs"], i["wts"], i["bs"], 4), "conv_in": o.conv_in(i["z"], 1.7, -0.3, i["wi"], i["bi"], 4, dtype),
                "vae_output": [o.vae_output(i["y"], True), o.vae_output(i["y"], False)]}
    return make, call, None


@case("vae_encoder_kernels", ["primx_enc_conv_in", "primx_conv3d_down_s8c32", "primx_enc_head"], BOTH)
def _vae_enc(E, dtype):
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0: the packed weight images are switched off")
    P = 3

    def make(k):
        return {"x": R(k, "ve.x", P, 6, 8, 8, 8, scale=0.6, offset=0.3), "w": _conv_w(k, "ve.w", 32, 6, dtype), "b": R(k, "ve.b", 32, scale=0.2, dtype=dtype),
                "xd": R(k, "ve.xd", P, 512, 32, dtype=dtype), "wd": _conv_w(k, "ve.wd", 32, 32, dtype), "bd": R(k, "ve.bd", 32, scale=0.2, dtype=dtype),
                "h": R(k, "ve.h", P, 64, 256, scale=0.8, offset=0.1, dtype=dtype), "wh": _conv_w(k, "ve.wh", 2, 256, dtype),
                "bh": R(k, "ve.bh", 2, scale=0.2), "qw": R(k, "ve.qw", 2, 2, scale=0.7), "qb": R(k, "ve.qb", 2, scale=0.2)}

    def call(ctx, i, probe):
        o = E.ops
        wp = o.pack_conv3(i["wd"], 32)
        return {"enc_conv_in": [o.enc_conv_in(i["x"], i["w"], i["b"], nrm) for nrm in (False, True)],
                "down": o.conv3d_down(i["xd"], wp, i["bd"]), "head": o.enc_head(i["h"], i["wh"], i["bh"], i["qw"], i["qb"])}
    return make, call, None


_SD = {}


def _fresh_vae(E, dtype):
    from oracle import synth
    from tests.golden.make_golden import SEED, VAE_CFG
    vae = E.pkg.VAE(**VAE_CFG).eval()
    if "vae" not in _SD:
        _SD["vae"] = synth.state_dict_like(SEED, vae.state_dict())
    vae.load_state_dict(_SD["vae"], strict=True)
    vae.to(DEV)
    vae.compute_dtype = dtype
    return vae


@case("vae_decode", ["primx_conv_in", "primx_attention", "primx_vae_output"], BOTH)
def _vae_decode(E, dtype):
    def make(k):
        return {"z": R(k, "vd.z", 3, 1, 4, 4, 4)}
    return make, (lambda vae, i, probe: twice(lambda: vae.decode(i["z"]), probe)), (lambda: _fresh_vae(E, dtype))


@case("vae_encode", ["primx_enc_conv_in", "primx_conv3d_down_s8c32", "primx_enc_head"], BOTH)
def _vae_encode(E, dtype):
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0: the packed weight images are switched off")

    def make(k):
        return {"x": R(k, "vn.x", 3, 6, 8, 8, 8, scale=0.8)}
    return make, (lambda vae, i, probe: twice(lambda: vae.encode(i["x"]).parameters, probe)), (lambda: _fresh_vae(E, dtype))


# ---------------------------------------------------------------------------------------------- DiT and the sampler
def _fresh_dit(E, key, cfg, heads, N, seed, **flags):
    from oracle import synth
    if key not in _SD:
        _SD[key] = synth.dit_state_dict(seed, **cfg)
    m = E.pkg.DiT(seq_length=N, num_heads=heads, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    m.load_state_dict(_SD[key], strict=True)
    m.to(DEV)
    for name, value in flags.items():
        assert hasattr(m, name), name
        setattr(m, name, value)
    return m


def _tiny_dit(E, **flags):
    from tests.golden.make_golden import DIT_CASES, SEED
    name, cfg, heads, N, L, B = DIT_CASES[1]
    return (lambda: _fresh_dit(E, name, cfg, heads, N, SEED, **flags)), (B, N, cfg["in_channels"]), (B, L, cfg["condition_channels"])


def _dit_forward_case(E, dtype, **flags):
    setup, xs, ys = _tiny_dit(E, **flags)

    def make(k):
        return {"x": R(k, "dit.x", *xs), "y": R(k, "dit.y", *ys), "t": torch.tensor([520 + k] * xs[0], device=DEV)}
    def call(m, i, probe):
        out = m.forward_with_cfg(i["x"], i["t"], i["y"], 6.0, dtype, True)
        if flags.get("cfg_streams"):
            assert m._side, "cfg_streams is set, but the forward did not take the model's side stream"
        return out
    return make, call, setup


_DIT_FORWARD = ["primx_linear", "primx_linear_heads", "primx_attention", "primx_cfg_combine"]
for _name, _flags in (("dit_forward_with_cfg", {}), ("dit_weight_prefetch_0", dict(weight_prefetch=0)),
                      ("dit_weight_prefetch_1", dict(weight_prefetch=1)), ("dit_weight_prefetch_2", dict(weight_prefetch=2)),
                      ("dit_cfg_streams", dict(cfg_streams=True)), ("dit_collapse_null", dict(collapse_null_cross_attention=True))):
    case(_name, _DIT_FORWARD, BOTH)(lambda E, dtype, _f=_flags: _dit_forward_case(E, dtype, **_f))


def _probed_steps(d, probe):
    """Bracket every `_step` of the diffusion object with the probe: (c) at the return of each step, the first forward of a
    loop - which builds the loop's tables - included.  What a loop does outside its steps (the coefficient table and index
    uploads before the first, the fold's overflow guard after the last) is not inside a bracket."""
    real = d._step

    def stepped(*a, **kw):
        probe.step()
        out = real(*a, **kw)
        probe.returned()
        return out
    d._step = stepped


def _planned_loop_case(E, dtype, **flags):
    """3 DDIM steps, planned, at the width where every GEMM of a block has a fold kernel (d = 1152, 16 heads, 2048 tokens, 1370 x
    768 condition tokens, two blocks): the blocks of a forward go through primx_dit_blocks_fold unless `blocks_call` is off."""
    from importlib import import_module
    from tests.golden.make_golden_xl import HEADS, L_COND, XL, XL_SEED
    sampler = import_module(E.pkg.__name__ + ".diffusion.sampler")
    cfg = dict(depth=2, **XL)

    def setup():
        return (_fresh_dit(E, "xl2", cfg, HEADS, 2048, XL_SEED, **flags),
                E.pkg.create_diffusion("ddim3", noise_schedule="squaredcos_cap_v2", parameterization="v"))

    def make(k):
        return {"x": R(k, "pl.x", 1, 2048, 68), "y": R(k, "pl.y", 1, L_COND, 768)}

    def call(ctx, i, probe):
        m, d = ctx
        keep, sampler.PLAN_TIMESTEPS = sampler.PLAN_TIMESTEPS, True
        _probed_steps(d, probe)
        try:
            kw = dict(y=i["y"], cfg_scale=6.0, precision_dtype=dtype, enable_amp=True)
            out = [o["sample"] for o in d.ddim_sample_loop_progressive(m.forward_with_cfg, (1, 2048, 68), noise=i["x"], clip_denoised=False,
                                                                       model_kwargs=kw)]
        finally:
            sampler.PLAN_TIMESTEPS = keep
        folded = bool(m._fold_ws)
        if m.fold_ln and not os.environ.get("PRIMX_GEMM_NOBIG"):
            assert folded, "the planned loop did not take the LayerNorm fold"
        return out
    return make, call, setup


@case("dit_planned_loop", ["primx_dit_blocks_fold", "primx_linear_f32out_group", "primx_diffusion_step"], BOTH)
def _dit_planned(E, dtype):
    _fold_skip(E.ops)
    if not E.ops._lib.blocks_call_available() or not E.ops._lib.f32out_group_available() or os.environ.get("PRIMX_UV_GROUP") == "0":
        pytest.skip("the build lacks primx_dit_blocks_fold or the grouped u / v launch")
    return _planned_loop_case(E, dtype)


@case("dit_planned_loop_host_launches", ["primx_linear_fold", "primx_linear_gate_residual_fold", "primx_attention",
                                         "primx_diffusion_step"], BOTH)
def _dit_planned_host(E, dtype):
    _fold_skip(E.ops)
    return _planned_loop_case(E, dtype, blocks_call=False)


@case("dit_edit", ["primx_diffusion_reverse_step", "primx_diffusion_step_keep"], BOTH)
def _dit_edit(E, dtype):
    """One inversion step (level 3 -> 4) and one kept re-denoise step of the edit path on the tiny DiT, each through its loop:
    both steps are probed.  (The single-step API reads its device `t` back, _one_step_of: the loops take host step numbers.)"""
    setup_m, xs, ys = _tiny_dit(E)

    def setup():
        return setup_m(), E.pkg.create_diffusion("ddim5", noise_schedule="squaredcos_cap_v2", parameterization="v")

    def make(k):
        return {"x": R(k, "ed.x", *xs), "y": R(k, "ed.y", *ys), "known": R(k, "ed.kn", *xs), "kn": R(k, "ed.kk", *xs),
                "keep": (R(k, "ed.keep", xs[0], xs[1]) > 0).to(torch.uint8)}

    def call(ctx, i, probe):
        m, d = ctx
        _probed_steps(d, probe)
        kw = dict(y=i["y"], cfg_scale=6.0, precision_dtype=dtype, enable_amp=True)
        inv = list(d.ddim_reverse_sample_loop_progressive(m.forward_with_cfg, i["x"], clip_denoised=False, model_kwargs=kw, start_step=3,
                                                          stop_step=4))
        kept = list(d.ddim_sample_loop_progressive(m.forward_with_cfg, xs, noise=inv[0]["sample"], clip_denoised=False, model_kwargs=kw,
                                                   start_step=0, known=i["known"], known_noise=i["kn"], keep=i["keep"].bool()))
        assert len(inv) == 1 and len(kept) == 1
        return [inv[0]["sample"], inv[0]["pred_xstart"], kept[0]["sample"]]
    return make, call, setup


# ---------------------------------------------------------------------------------------------- rendering, PrimSDF, DINOv2
@case("raymarch", ["primx_compute_raydirs", "primx_raymarch"])
def _raymarch(E, dtype):
    from tests import raymarch_scenes as sc
    from tests import test_raymarch_contract as TR
    from topia_xl_amd import raymarch as rm
    name, kw, fs = next(c for c in TR.CASES if c[1]["H"] % 16 or c[1]["W"] % 16)      # a ragged image size
    N, H, W = kw.get("N", 1), kw["H"], kw["W"]
    names = ("tpl", "pos", "rot", "scale", "cp", "cr", "f", "pp")

    def make(k):
        d = {n: t.to(DEV).contiguous() for n, t in zip(names, sc.scene(**dict(kw, seed=kw.get("seed", 0) + k)))}
        ys, xs = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
        d["pc"] = torch.stack([xs, ys], -1)[None].expand(N, -1, -1, -1).contiguous().to(DEV) + 0.25 * k
        return d

    def call(ctx, i, probe):
        rp, rd, tm = rm.compute_raydirs(i["cp"], i["cr"], i["f"], i["pp"], i["pc"], 1.0)
        return [rp, rd, tm, rm.mvpraymarch(rp, rd, TR.DT, tm, (i["pos"], i["rot"], i["scale"]), i["tpl"], fs, 8.0)]
    return make, call, None


@case("primsdf_query", ["primx_primsdf_query"])
def _primsdf(E, dtype):
    from tests import test_primsdf_contract as TP
    from topia_xl_amd.primsdf import PrimSDF
    P, n = 1025, 257                                               # two LDS chunks of primitives, ragged points

    def setup():
        return PrimSDF(num_prims=P, prim_shape=8).to(DEV).eval()

    def make(k):
        gen = torch.Generator().manual_seed(P * 7 + n + k)
        srt, feat = TP._prims(gen, P, 8, lo=0.01, hi=0.03)
        x = 1.6 * torch.rand(n, 3, generator=gen) - 0.8
        srt[P - 1, 0], srt[P - 1, 1:4] = 0.3, x[0] + 0.05
        return {"srt": srt.to(DEV).contiguous(), "feat": feat.to(DEV).contiguous(), "x": x.to(DEV)}

    def call(m, i, probe):
        m.srt_param.data, m.feat_param.data = i["srt"], i["feat"]
        return twice(lambda: m.query(i["x"]), probe)
    return make, call, setup


@case("dinov2", ["primx_vit_tokens", "primx_linear_f32", "primx_linear_gate_residual", "primx_attention"], BOTH)
def _dinov2(E, dtype):
    from tests.golden.make_golden import DINO_CFG, dino_state_dict
    from topia_xl_amd import dinov2

    def setup():
        m = dinov2.DinoVisionTransformer(**DINO_CFG).eval()
        if "dino" not in _SD:
            _SD["dino"] = dino_state_dict(m.state_dict())
        m.load_state_dict(_SD["dino"], strict=True)
        return m.to(DEV)

    def make(k):
        return {"x": R(k, "dino.x", 2, 3, 84, 84)}                  # 84 != 56: the position table is interpolated
    return make, (lambda m, i, probe: m.conditioner_tokens(i["x"], precision_dtype=dtype)), setup


# ---------------------------------------------------------------------------------------------- mesh export
@case("mcubes", ["primx_mcubes_count", "primx_mcubes_emit"])
def _mcubes(E, dtype):
    from topia_xl_amd import mesh as M

    def make(k):
        return {"vol": _dev(np.random.default_rng(71 + k).standard_normal((17, 23, 31)).astype(np.float32))}
    return make, (lambda ctx, i, probe: M.marching_cubes(i["vol"], 0.3, return_normals=True)), None


@case("noise_filter", ["primx_noise_filter"])
def _noise_filter(E, dtype):
    from topia_xl_amd import mesh as M

    def make(k):
        srt = torch.cat([0.02 + 0.05 * torch.rand(300, 1, generator=torch.Generator().manual_seed(k)),
                         1.6 * torch.rand(300, 3, generator=torch.Generator().manual_seed(k + 9)) - 0.8], 1)
        return {"srt": srt.to(DEV).contiguous()}
    return make, (lambda ctx, i, probe: M.noise_filter_mask(i["srt"])), None


class _ActiveGuard:
    """The `g` the footprint case builders take: the guard streamorder.run has opened, or plain tensors on the reference run."""

    @staticmethod
    def guard_input(t, name="", const=True):
        return fp.guard_input(t, name, const) if fp._active is not None else fp.InputHandle(t, None, name)


@case("mesh_export_48", ["primx_primsdf_query", "primx_mcubes_count", "primx_mcubes_emit", "primx_noise_filter", "primx_meshclean_merge",
                         "primx_meshclean_faces", "primx_meshclean_components", "primx_meshclean_fans", "primx_meshdecim_edges",
                         "primx_meshdecim_quadrics", "primx_meshdecim_costs", "primx_meshdecim_select", "primx_meshdecim_collapse",
                         "primx_meshdecim_finish", "primx_meshdecim_normals", "primx_texbake_labels", "primx_texbake_components",
                         "primx_texbake_raster", "primx_texbake_compact", "primx_texbake_fill"])
def _mesh_export(E, dtype):
    """The chain of test_hip_footprint.test_mesh_export_footprint_48 (extract at 48^3, clean, decimate, normals, bake) with a
    256 x 256 atlas; the field's parameters are the late operands."""
    from tests import test_hip_footprint as TFP
    from tests import test_hip_mesh as TM
    from topia_xl_amd import mesh as M
    base = TM._synthetic_field()
    srt0, feat0 = base.srt_param.detach().clone(), base.feat_param.detach().clone()

    def make(k):
        f = feat0.clone()
        f[:, 512:] = f[:, 512:] * (1.0 - 0.25 * k)                  # other colours, the same surface: the same counts and sizes
        return {"srt": srt0.clone(), "feat": f.contiguous()}

    def call(field, i, probe):
        field.srt_param.data, field.feat_param.data = i["srt"], i["feat"]
        field._lin.clear()
        return TFP._mesh_chain(M, _ActiveGuard, field, 48, (256, 256), None)
    return make, call, TM._synthetic_field


@case("clean_mesh_nonmanifold", ["primx_meshclean_merge", "primx_meshclean_faces", "primx_meshclean_components", "primx_meshclean_edges",
                                 "primx_meshclean_fans"])
def _clean_nonmanifold(E, dtype):
    """The noise volume of test_hip_meshclean.test_noise_bit_exact: its merge makes non-manifold edges, so the edge pass runs."""
    from tests import mc_numpy
    from topia_xl_amd import mesh as M
    v0, _, f0 = mc_numpy.marching_cubes(np.random.default_rng(4).standard_normal((24, 24, 24)).astype(np.float32), 0.2)

    def make(k):
        return {"v": _dev(v0, F32) * (1.0 + 0.5 * k), "f": _dev(f0, torch.int32)}     # (the warm-up: the same mesh at another scale)

    def call(ctx, i, probe):
        st = {}
        v, f, vmap = M.clean_mesh(i["v"], i["f"], return_vmap=True, stats=st, v_pct=1, min_f=8, min_d=0)
        assert st["nonmanifold_candidates"] > 0
        return [v, f, vmap]
    return make, call, None


# ---------------------------------------------------------------------------------------------- fit
def _fit_mesh(F):
    from tests import meshfield_numpy as MF
    v, f = MF.mesh_with_faces(F)
    return v, f, MF.affine_attr(v)


@case("mesh_field_query", ["primx_mesh_field_query"])
def _field_query(E, dtype):
    from topia_xl_amd import fit
    v, f, attr = _fit_mesh(257)

    def make(k):
        return {"x": R(k, "fq.x", 257, 3, scale=0.5), "v": _dev(v, F32) * (1.0 + 0.1 * k), "f": _dev(f, torch.int32), "attr": _dev(attr, F32) + k}
    return make, (lambda ctx, i, probe: fit.mesh_field_query(i["x"], i["v"], i["f"], i["attr"])), None


@case("face_areas_surface_points", ["primx_mesh_face_areas", "primx_mesh_surface_points"])
def _areas_points(E, dtype):
    from tests import meshfield_numpy as MF
    from topia_xl_amd import fit
    v, f, _ = _fit_mesh(549)
    cdf = np.cumsum(MF.face_areas(v, f))

    def make(k):
        s = 1.0 + k
        return {"v": _dev(v, F32) * s, "f": _dev(f, torch.int32), "cdf": _dev(cdf * s * s, torch.float64), "u": fit.surface_uniforms(1000, 1 + k).to(DEV)}
    return make, (lambda ctx, i, probe: [fit.face_areas(i["v"], i["f"]), fit.surface_points(i["v"], i["f"], i["cdf"], i["u"])]), None


@case("fps", ["primx_fps"])
def _fps(E, dtype):
    from tests import test_hip_meshfield as TMF
    from topia_xl_amd import fit

    def make(k):
        return {"big": _dev(TMF._candidates(4097, 1 + k), F32), "two": _dev(TMF._candidates(2, 1 + k), F32) + k}
    return make, (lambda ctx, i, probe: [fit.fps(i["big"], 256, 1), fit.fps(i["two"], 2, 1)]), None    # 257 launches in five blocks; (2, 2)


@case("mesh_to_primitives", ["primx_mesh_face_areas", "primx_mesh_surface_points", "primx_fps", "primx_mesh_field_query"])
def _mesh_to_primitives(E, dtype):
    from tests import meshfield_numpy as MF
    from topia_xl_amd import fit
    v, f = MF.icosphere(1)
    attr = MF.affine_attr(v)

    def make(k):
        a = _dev(attr, F32) * (1.0 - 0.5 * k)
        return {"v": _dev(v, F32) * (1.0 + 0.3 * k), "f": _dev(f, torch.int32), "alb": a[:, :3].contiguous(), "ro": a[:, 3].contiguous(),
                "me": a[:, 4].contiguous()}

    def call(ctx, i, probe):
        recon, info = fit.mesh_to_primitives((i["v"], i["f"], i["alb"], i["ro"], i["me"]), num_prims=33, prim_shape=3, candidates=300)
        return [recon, info["candidates"], info["idx"]]
    return make, call, None


# ---------------------------------------------------------------------------------------------- the tests
PARAMS = [(c.name, dt) for c in CASES.values() for dt in c.dtypes]
LOG = []


def _id(p):
    return p if isinstance(p, str) else str(p).replace("torch.", "")


@pytest.mark.parametrize("name,dtype", PARAMS, ids=[f"{n}-{_id(dt)}" if dt is not None else n for n, dt in PARAMS])
def test_stream_order(E, called, name, dtype):
    """(a) order, (b) conclusive, (c) asynchronous unless MUST_SYNC says why not - for every case of CASES; and the entry points
    the case declares were really called.  The line printed per case holds the blocker times that were needed."""
    c = CASES[name]
    make, call, setup = c.build(E, dtype)
    rep = so.run(name, make, call, E.S, E.blocker, setup=setup, must_sync=name in MUST_SYNC)
    LOG.append(rep)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{name} declares entry points it did not call: {missing}"


# the positive controls: each a harmless torch op, reported as the kind it is
def _control(E, call, **kw):
    def make(k):
        return {"x": R(k, "ctl.x", 1 << 20)}
    return so.run("control", make, call, E.S, E.blocker, **kw)


def test_control_op_on_the_default_stream_is_an_order_violation(E):
    def call(ctx, i, probe):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return i["x"] * 2
    rep = _control(E, call)
    assert rep.verdict == so.ORDER and not rep.null_gate_done, rep.message()
    assert "(a)" in rep.message()


def test_control_output_written_from_a_third_stream_is_an_order_violation(E):
    def call(ctx, i, probe):
        with torch.cuda.stream(E.S2):
            return i["x"] * 2
    rep = _control(E, call)
    assert rep.verdict == so.ORDER and not rep.null_gate_done, rep.message()


def test_control_stream_synchronize_is_a_host_synchronisation(E):
    def call(ctx, i, probe):
        torch.cuda.current_stream().synchronize()
        return i["x"] * 2
    rep = _control(E, call)
    assert rep.verdict == so.SYNCHRONISED and rep.late_returns == [True], rep.message()
    assert "(c)" in rep.message()
    assert _control(E, call, must_sync=True).verdict == so.OK       # the same call with a documented synchronisation


def test_control_short_blocker_is_inconclusive(E):
    rep = _control(E, lambda ctx, i, probe: i["x"] * 2, null_ms=0.01)
    assert rep.verdict == so.INCONCLUSIVE and not rep.differences, rep.message()
    assert "(b)" in rep.message()
    assert _control(E, lambda ctx, i, probe: i["x"] * 2).verdict == so.OK


# ---------------------------------------------------------------------------------------------- overlap
def _pair_conv_attention(E, dtype):
    o = E.ops
    x, w, b = R(0, "ov.x", 300, 64, 256, dtype=dtype), _conv_w(0, "ov.w", 256, 256, dtype), R(0, "ov.b", 256, scale=0.2, dtype=dtype)
    wp = o.pack_conv3(w, 256)
    if wp is None:
        pytest.skip("PRIMX_CONV_REG=0 keeps the implicit GEMM: no packed convolution")
    q = _qkv(0, "ov.at", 1, 300, 1000, 2, 72, dtype)
    return (lambda: o.conv3d_k3(x, w, b, 4, Wp=wp),
            lambda: o.memory_efficient_attention(q["q"][:, :, 0], q["kv"][:, :, 1], q["kv"][:, :, 2]))


def _pair_fold_heads(E, dtype):
    from tests import test_hip_fold_contract as TF
    _fold_skip(E.ops)
    o = E.ops
    ROWS, KROWS, VT = _kinds()
    s = _site(E, dtype, 4, 0)
    M = s["a16"].shape[0]

    def consumer():
        co = _nan(M, 2)
        return o.linear_fold(s["a16"], s["W"], _nan(M, s["W"].shape[0], dtype=dtype), s["part"], s["u"], s["v"], s["center"], co, TF.EPS,
                             act=1), co
    A, W, bb = R(0, "ov.A", 4096, 256, dtype=dtype), R(0, "ov.W", 3 * 1152, 256, scale=1 / 16, dtype=dtype), R(0, "ov.bb", 3 * 1152, dtype=dtype)

    def heads():
        d = _heads_dsts(o, 2, 16, 2048, 72, [ROWS, KROWS, VT], dtype, 256)
        o.linear_heads(A, W, bb, 2048, 16, 72, [ROWS, KROWS, VT], d, d[0].shape[2], scale0=72 ** -0.5)
        return d
    return consumer, heads


def _pair_fps_query(E, dtype):
    from tests import test_hip_meshfield as TMF
    from topia_xl_amd import fit
    v, f, attr = _fit_mesh(257)
    pts, xq = _dev(TMF._candidates(4097, 1), F32), R(0, "ov.xq", 1000, 3, scale=0.5)
    vd, fd, ad = _dev(v, F32), _dev(f, torch.int32), _dev(attr, F32)
    return (lambda: fit.fps(pts, 256, 1)), (lambda: fit.mesh_field_query(xq, vd, fd, ad))       # (the synchronising host second)


PAIRS = [("conv | attention", _pair_conv_attention, F16), ("conv | attention", _pair_conv_attention, BF16),
         ("fold consumer | heads GEMM", _pair_fold_heads, F16), ("fold consumer | heads GEMM", _pair_fold_heads, BF16),
         ("fps | mesh_field_query", _pair_fps_query, None)]


@pytest.mark.parametrize("name,build,dtype", PAIRS, ids=[n.replace(" | ", "+").replace(" ", "_") + ("-" + _id(dt) if dt else "") for n, _, dt in PAIRS])
def test_pair_at_once_on_two_streams_matches_its_serial_runs(E, name, build, dtype):
    """Two calls at once on `S` and `S2`, released by one event: a packed convolution next to attention, a fold consumer next to a
    heads GEMM, fps next to mesh_field_query.  Each result is bit-identical to its serial run on the default stream."""
    a, b = build(E, dtype)
    d = so.overlap(name, a, b, (E.S, E.S2), E.blocker)
    assert not d, "\n".join(d)


# ---------------------------------------------------------------------------------------------- the repetition stays rare
MAX_REPEATED = 3


def test_few_cases_needed_the_longer_blocker():
    """streamorder.run repeats a case ONCE with a longer stream-0 blocker when (b) found the first too short.  That is calibration,
    not retry-to-pass - as long as it stays the exception: on the MI355X one case needed it (`dit_cfg_streams`, whose forward also
    waits on the model's own side stream).  More than MAX_REPEATED such cases in a run of the whole table fail here, by name."""
    if len(LOG) < len(PARAMS) // 2:
        return                                                      # (a selection of tests: the table did not run)
    repeated = sorted({r.name for r in LOG if r.attempts > 1})
    print(f"streamorder: {len(repeated)} of {len(LOG)} cases needed the longer stream-0 blocker: {repeated}")
    assert len(repeated) <= MAX_REPEATED, repeated
