"""Which kernel does each 16-bit GEMM entry point launch?  A table of (entry point, dtype, shape, environment) rows, each held to the name
primx_last_gemm_kernel() reported for it when tests/golden/gemm_dispatch.json was recorded (tools/record_gemm_dispatch.py) - or to
"the call is rejected".  The rows sit on both sides of every threshold of the dispatch in csrc/gemm.hip; operands are zero-filled,
K is as small as the route allows: the numbers are the business of the other GEMM suites.

The switches are read when the library loads, so every distinct environment runs in ONE fresh child process (this file, run as a
script), one after another; a child prints one JSON object for all rows of its environment.  tests/test_gemm_dispatch_cpu.py
holds the table itself to the kernel names and the switches that csrc/gemm.hip spells out.

Where a row names ops.fold_shapes_ok / ops.fold_pair_fits arguments, the Python restatement of the rule is held to what the
library did on that row."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.json")
F16, BF16 = "float16", "bfloat16"
ROWS_, VT, KROWS = 0, 1, 2          # _lib.HEADS_ROWS / HEADS_VT / HEADS_KROWS
QKV, QKQ, KV = (ROWS_, KROWS, VT), (ROWS_, KROWS, ROWS_), (KROWS, VT)


def _heads(M, rpb, heads, dh, kinds, K, **kw):
    return dict(M=M, rpb=rpb, heads=heads, dh=dh, kinds=kinds, K=K, **kw)


def _common(env):
    """Rows that every dispatch-moving environment repeats: both sides of each threshold the switches move."""
    return [
        # dense big tile: 16 x 14 = 224 workgroups against one tile row fewer (15 x 14 = 210), three epilogues
        ("linear_224", "linear", F16, dict(M=4096, N=4032, K=64), env),
        ("linear_210", "linear", F16, dict(M=3840, N=4032, K=64), env),
        ("linear_112", "linear", F16, dict(M=2048, N=4032, K=64), env),
        ("linear_98", "linear", F16, dict(M=1792, N=4032, K=64), env),
        ("res_224", "linear_residual", F16, dict(M=4096, N=4032, K=64), env),
        ("res_210", "linear_residual", F16, dict(M=3840, N=4032, K=64), env),
        ("res_266", "linear_residual", F16, dict(M=4864, N=4032, K=64), env),
        ("gate_224", "gate_residual", F16, dict(M=4096, N=4032, K=64, rpb=2048), env),
        ("gate_210", "gate_residual", F16, dict(M=3840, N=4032, K=64, rpb=1920), env),
        # the KT = 64 ring of the read-modify-write epilogue: 16 x 16 = 256 against 17 x 16 = 272 workgroups (threshold 257),
        # ragged M and a batch entry that is no whole number of tiles
        ("gate_256", "gate_residual", F16, dict(M=4096, N=4608, K=64, rpb=2048), env),
        ("gate_272", "gate_residual", F16, dict(M=4352, N=4608, K=64, rpb=4352), env),
        ("gate_272_ragged", "gate_residual", F16, dict(M=4344, N=4608, K=64, rpb=4344), env),
        ("gate_272_rpb2176", "gate_residual", F16, dict(M=4352, N=4608, K=64, rpb=2176), env),
        # heads: 13 x 12 = 156 against 14 x 12 = 168 workgroups of the big tile (threshold 160); K = 128 is the shortest KT = 64 ring
        ("heads_156", "heads", F16, _heads(3328, 256, 16, 72, QKV, 64), env),
        ("heads_168", "heads", F16, _heads(3584, 256, 16, 72, QKV, 64), env),
        ("heads_168_k128", "heads", F16, _heads(3584, 256, 16, 72, QKV, 128), env),
        ("heads_204", "heads", F16, _heads(4352, 256, 16, 72, QKV, 64), env),
        ("heads_168_rpb128", "heads", F16, _heads(3584, 128, 16, 72, QKV, 64), env),
        ("heads_168_dh64", "heads", F16, _heads(3584, 256, 18, 64, QKV, 64), env),           # 288 % 64 != 0
        ("heads_156_no_vt", "heads", F16, _heads(3328, 256, 16, 72, QKQ, 64), env),
        ("heads_156_rpb64", "heads", F16, _heads(3328, 64, 16, 72, QKQ, 64), env),           # rows_per_batch < 128
        # the fold: producer and both consumers on both tiles
        ("gfold_8", "gate_residual_fold", F16, dict(M=256, N=1152, K=64, rpb=256), env),
        ("gfold_224", "gate_residual_fold", F16, dict(M=14336, N=1152, K=64, rpb=2048), env),
        ("gfold_260", "gate_residual_fold", F16, dict(M=16640, N=1152, K=64, rpb=16640), env),
        ("lfold_210", "linear_fold", F16, dict(M=3840, N=4032, K=576), env),
        ("lfold_224", "linear_fold", F16, dict(M=4096, N=4032, K=576), env),
        # the qkv consumer writes a V^T segment: below the big tile's threshold the call is rejected, and ops.fold_shapes_ok says so
        ("hfold_156", "heads_fold", F16, _heads(3328, 256, 16, 72, QKV, 1152, fold_shapes_ok=(3328, 256, 1152, 16)), env),
        ("hfold_168", "heads_fold", F16, _heads(3584, 256, 16, 72, QKV, 1152, fold_shapes_ok=(3584, 256, 1152, 16)), env),
        ("hfold_204", "heads_fold", F16, _heads(4352, 256, 16, 72, QKV, 1152, fold_shapes_ok=(4352, 256, 1152, 16)), env),
        ("hfold_156_no_vt", "heads_fold", F16, _heads(3328, 256, 16, 72, QKQ, 576), env),
        ("hfold_156_rpb64", "heads_fold", F16, _heads(3328, 64, 16, 72, QKQ, 576), env),
        # the pair: problem 1 alone; 192 + 48 workgroups (one round); 192 + 96 (two launches)
        ("pair_alone", "pair", F16, dict(fold=None, kv=_heads(1536, 1536, 16, 72, KV, 128)), env),
        ("pair_alone_1408", "pair", F16, dict(fold=None, kv=_heads(1408, 1408, 16, 72, KV, 128)), env),
        ("pair_192_48", "pair", F16, dict(fold=_heads(4096, 2048, 16, 72, QKV, 1152), kv=_heads(1536, 1536, 16, 72, KV, 128),
                                          fold_pair_fits=(4096, 2048, 1152, 16, 1536, 1536, 128)), env),
        ("pair_192_96", "pair", F16, dict(fold=_heads(4096, 2048, 16, 72, QKV, 1152), kv=_heads(3072, 1536, 16, 72, KV, 128),
                                          fold_pair_fits=(4096, 2048, 1152, 16, 3072, 1536, 128)), env),
    ]


_LN = dict(M=8192, N=1152, K=64, rpb=2048)       # (a shape of tests/test_hip_gemm.py::test_gate_residual_with_layernorm_tail)

CASES = _common({}) + [
    # the narrow tile, the wide tile, the few-row kernel
    ("linear_n32", "linear", F16, dict(M=200, N=32, K=64), {}),
    ("linear_n48", "linear", F16, dict(M=200, N=48, K=64), {}),
    ("linear_n144", "linear", F16, dict(M=200, N=144, K=64), {}),
    ("linear_n144_bf16", "linear", BF16, dict(M=200, N=144, K=64), {}),
    ("linear_n144_ktail", "linear", F16, dict(M=200, N=144, K=72), {}),
    ("linear_n144_gelu", "linear", F16, dict(M=8, N=144, K=64, act=1), {}),
    ("res_n32", "linear_residual", F16, dict(M=200, N=32, K=64), {}),
    ("res_n144", "linear_residual", BF16, dict(M=200, N=144, K=64), {}),
    ("gate_n32", "gate_residual", F16, dict(M=200, N=32, K=64, rpb=100), {}),
    ("gate_n144", "gate_residual", BF16, dict(M=200, N=144, K=64, rpb=100), {}),
    ("linear_224_bf16", "linear", BF16, dict(M=4096, N=4032, K=64), {}),
    ("gate_272_bf16", "gate_residual", BF16, dict(M=4352, N=4608, K=64, rpb=4352), {}),
    ("heads_168_k128_bf16", "heads", BF16, _heads(3584, 256, 16, 72, QKV, 128), {}),
    ("heads_rep2", "heads", F16, _heads(1536, 1536, 16, 72, KV, 64, n_rep=2), {}),
    ("heads_ktail", "heads", F16, _heads(256, 256, 16, 72, QKQ, 72), {}),
    ("conv3d_n16", "conv3d_k3", F16, dict(P=1, S=4, Cin=8, Cout=16, Kpad=256), {}),
    ("conv3d_n48", "conv3d_k3", F16, dict(P=1, S=4, Cin=8, Cout=48, Kpad=256), {}),
    ("convt_n128", "convtranspose_k2s2", F16, dict(P=1, S=4, Cin=64, Cout=16), {}),
    ("f32out_n144", "f32out", F16, dict(M=50, N=144, K=64), {}),
    ("f32out_n160", "f32out", F16, dict(M=50, N=160, K=64), {}),
    ("f32out_group", "f32out_group", BF16, dict(M=50, Ns=(32, 64), K=64), {}),
    ("ln_sync", "gate_residual_ln", F16, dict(_LN, sync=True), {}),
    ("ln_no_sync", "gate_residual_ln", F16, dict(_LN, sync=False), {}),
    ("lfold_1", "linear_fold", BF16, dict(M=256, N=288, K=576), {}),
    ("lfold_n160", "linear_fold", F16, dict(M=256, N=160, K=576), {}),                       # N % 144 != 0: rejected
]
for _m in (4, 5, 8, 9):
    CASES.append((f"linear_m{_m}", "linear", F16, dict(M=_m, N=144, K=64), {}))
    CASES.append((f"linear_m{_m}", "linear", F16, dict(M=_m, N=144, K=64), {"PRIMX_GEMM_NOGEMV": "1"}))
for _env in ({"PRIMX_GEMM_BIG_MIN": "112"}, {"PRIMX_GEMM_NOBIG": "1"}, {"PRIMX_GEMM_KT32": "1"}, {"PRIMX_GEMM_KT64_MIN": "1"},
             {"PRIMX_GEMM_HEADS_KT32": "1"}, {"PRIMX_GEMM_LOADER": "0"}, {"PRIMX_GEMM_BIGHEADS_MIN": "0"},
             {"PRIMX_GEMM_BIGHEADS_MIN": "200"}):
    CASES += _common(_env)
CASES += [
    # EPI_LINEAR takes the KT = 64 ring from ONE workgroup on
    ("linear_1", "linear", F16, dict(M=256, N=288, K=64), {"PRIMX_GEMM_BIG_MIN": "1"}),
    ("gate_1", "gate_residual", F16, dict(M=256, N=288, K=64, rpb=256), {"PRIMX_GEMM_BIG_MIN": "1"}),
    ("lfold_1", "linear_fold", F16, dict(M=256, N=288, K=576), {"PRIMX_GEMM_BIG_MIN": "1"}),
    ("f32out_n144", "f32out", F16, dict(M=50, N=144, K=64), {"PRIMX_F32OUT_TILE144": "0"}),
    ("f32out_n144", "f32out", F16, dict(M=50, N=144, K=64), {"PRIMX_GEMM_LOADER": "0"}),
    ("linear_n144", "linear", F16, dict(M=200, N=144, K=64), {"PRIMX_GEMM_LOADER": "0"}),
    ("ln_sync", "gate_residual_ln", F16, dict(_LN, sync=True), {"PRIMX_GEMM_LOADER": "0"}),
    ("ln_sync", "gate_residual_ln", F16, dict(_LN, sync=True), {"PRIMX_LN_FUSE": "0"}),
    # the default protocol spelled out, a grid bound below this launch's 512 workgroups, whole tile rows per XCD in the big tile
    ("ln_sync", "gate_residual_ln", F16, dict(_LN, sync=True), {"PRIMX_LN_MODE": "41", "PRIMX_GEMM_XCD2D": "0"}),
    ("linear_224", "linear", F16, dict(M=4096, N=4032, K=64), {"PRIMX_LN_MODE": "41", "PRIMX_GEMM_XCD2D": "0"}),
    ("heads_168", "heads", F16, _heads(3584, 256, 16, 72, QKV, 64), {"PRIMX_LN_MODE": "41", "PRIMX_GEMM_XCD2D": "0"}),
    ("ln_sync", "gate_residual_ln", F16, dict(_LN, sync=True), {"PRIMX_LN_FUSE_MAXGRID": "256"}),
    # the timeline reporter (8-wave kernels): synchronous launches, never the pair kernel
    ("linear_224", "linear", F16, dict(M=4096, N=4032, K=64), {"PRIMX_GEMM_PROF": "1"}),
    ("linear_n144", "linear", F16, dict(M=200, N=144, K=64), {"PRIMX_GEMM_PROF": "1"}),
    ("pair_192_48", "pair", F16, dict(fold=_heads(4096, 2048, 16, 72, QKV, 1152), kv=_heads(1536, 1536, 16, 72, KV, 128),
                                      fold_pair_fits=(4096, 2048, 1152, 16, 1536, 1536, 128)), {"PRIMX_GEMM_PROF": "1"}),
]


def env_key(env):
    return " ".join(f"{k}={v}" for k, v in sorted(env.items())) or "default"


ENVS = []
for _c in CASES:
    if _c[4] not in ENVS:
        ENVS.append(_c[4])


def rows_of(env):
    return [c for c in CASES if c[4] == env]


# ---------------------------------------------------------------------------------------------------------------- the child process
def _run_row(ops, torch, entry, dtype, s):
    """Make the call of one row (zero-filled operands) - through ops.*, which raises _lib.PrimxError where the library rejects it."""
    dev = "cuda"
    z = lambda *shape, dt=dtype: torch.zeros(*shape, dtype=dt, device=dev)
    f32 = torch.float32

    def heads_dsts(h, n_rep=1):
        n_pad = ops.round_up(h["rpb"], 128)
        B = h["M"] // h["rpb"] * n_rep
        return [ops.alloc_heads(B, h["heads"], h["rpb"], h["dh"], k, dtype, dev, 128) for k in h["kinds"]], n_pad

    def fold_args(M, N, K):
        c = z(2, M, 2, dt=f32)
        return dict(part=z(M, K // 144, 2, dt=f32), u=z(N, dt=f32), v=z(N, dt=f32), center=c[0], center_out=c[1])

    if entry == "linear":
        ops.linear(z(s["M"], s["K"]), z(s["N"], s["K"]), z(s["N"]), act=s.get("act", 0))
    elif entry == "linear_residual":
        ops.linear_residual(z(s["M"], s["K"]), z(s["N"], s["K"]), z(s["N"]), z(s["M"], s["N"]), 1.0)
    elif entry in ("gate_residual", "gate_residual_ln"):
        M, N, K, rpb = s["M"], s["N"], s["K"], s["rpb"]
        nb = (M + rpb - 1) // rpb
        ln = None
        if entry == "gate_residual_ln":
            sync = torch.zeros(ops.ln_sync_words(M), dtype=torch.int32, device=dev) if s["sync"] else None
            ln = (z(nb, N), z(nb, N), z(M, N), 1e-6, sync)
        ops.linear_gate_residual(z(M, K), z(N, K), z(N), z(nb, N), z(M, N, dt=f32), rpb, ln=ln)
    elif entry == "heads":
        n_rep = s.get("n_rep", 1)
        N = n_rep * len(s["kinds"]) * s["heads"] * s["dh"]
        dsts, n_pad = heads_dsts(s, n_rep)
        ops.linear_heads(z(s["M"], s["K"]), z(N, s["K"]), z(N), s["rpb"], s["heads"], s["dh"], list(s["kinds"]), dsts, n_pad,
                         n_rep=n_rep, rep_batches=s["M"] // s["rpb"] if n_rep > 1 else 0)
    elif entry == "gate_residual_fold":
        M, N, K, rpb = s["M"], s["N"], s["K"], s["rpb"]
        nb = (M + rpb - 1) // rpb
        ops.linear_gate_residual_fold(z(M, K), z(N, K), z(N), z(nb, N), z(M, N, dt=f32), rpb, z(nb, N), z(M, 2, dt=f32), z(M, N),
                                      z(M, N // 144, 2, dt=f32))
    elif entry == "linear_fold":
        M, N, K = s["M"], s["N"], s["K"]
        ops.linear_fold(z(M, K), z(N, K), z(M, N), eps=1e-6, **fold_args(M, N, K))
    elif entry == "heads_fold":
        N = len(s["kinds"]) * s["heads"] * s["dh"]
        dsts, n_pad = heads_dsts(s)
        ops.linear_heads_fold(z(s["M"], s["K"]), z(N, s["K"]), s["rpb"], s["heads"], s["dh"], list(s["kinds"]), dsts, n_pad,
                              eps=1e-6, **fold_args(s["M"], N, s["K"]))
    elif entry == "pair":
        f, kv = s["fold"], s["kv"]
        fold = None
        if f is not None:
            N = len(f["kinds"]) * f["heads"] * f["dh"]
            dsts, n_pad = heads_dsts(f)
            fold = dict(A=z(f["M"], f["K"]), W=z(N, f["K"]), rows_per_batch=f["rpb"], heads=f["heads"], dh=f["dh"], kinds=list(f["kinds"]),
                        dsts=dsts, n_pad=n_pad, eps=1e-6, **fold_args(f["M"], N, f["K"]))
        N2 = len(kv["kinds"]) * kv["heads"] * kv["dh"]
        dsts2 = [ops.alloc_heads(kv["M"] // kv["rpb"], kv["heads"], kv["rpb"], kv["dh"], k, dtype, dev, 256) for k in kv["kinds"]]
        ops.linear_heads_fold_pair(fold, z(kv["M"], kv["K"]), z(N2, kv["K"]), z(N2), kv["rpb"], kv["heads"], kv["dh"], list(kv["kinds"]),
                                   dsts2, ops.round_up(kv["rpb"], 256))
    elif entry == "f32out":
        ops.linear_f32out(z(s["M"], s["K"]), z(s["N"], s["K"]), z(s["N"]), z(s["M"], s["N"], dt=f32), s["M"] // 2)
    elif entry == "f32out_group":
        ok = ops.linear_f32out_group([(z(s["M"], s["K"]), z(n, s["K"]), z(n), z(s["M"], n, dt=f32)) for n in s["Ns"]], s["M"] // 2)
        assert ok, "the grouped kernel did not apply"
    elif entry == "conv3d_k3":
        ops.conv3d_k3(z(s["P"], s["S"] ** 3, s["Cin"]), z(s["Cout"], s["Kpad"]), z(s["Cout"]), s["S"])
    elif entry == "convtranspose_k2s2":
        ops.convtranspose_k2s2(z(s["P"], s["S"] ** 3, s["Cin"]), z(8 * s["Cout"], s["Cin"]), z(s["Cout"]), s["S"])
    else:
        raise KeyError(entry)


def child(env_index):
    """All rows of ENVS[env_index] in this process (whose environment the parent has set) -> one JSON object on stdout."""
    import torch
    import topia_xl_amd  # noqa: F401
    from topia_xl_amd import _lib, ops
    out = {}
    for rid, entry, dtype, shape, _ in rows_of(ENVS[env_index]):
        rec = {}
        try:
            _run_row(ops, torch, entry, getattr(torch, dtype), shape)
            rec["kernel"] = _lib.load().primx_last_gemm_kernel().decode()
        except _lib.PrimxError:
            rec["kernel"] = None                                       # rejected
        if "fold_shapes_ok" in shape:
            rec["fold_shapes_ok"] = bool(ops.fold_shapes_ok(*shape["fold_shapes_ok"]))
        if "fold_pair_fits" in shape:
            rec["fold_pair_fits"] = bool(ops.fold_pair_fits(*shape["fold_pair_fits"]))
        out[rid] = rec
    torch.cuda.synchronize()
    print("GEMM_DISPATCH " + json.dumps(out))


def run_env(env, timeout=300):
    """One fresh child for `env` (on top of this process's environment without any PRIMX_ switch of the table)."""
    switches = {k for e in ENVS for k in e}
    base = {k: v for k, v in os.environ.items() if k not in switches}
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(ENVS.index(env))], env=dict(base, **env), cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("GEMM_DISPATCH ")][-1]
    return json.loads(line[len("GEMM_DISPATCH "):])


# ------------------------------------------------------------------------------------------------------------------------ the test
@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS, ids=env_key)
def test_dispatch_is_the_recorded_one(env):
    with open(GOLDEN) as fh:
        want = json.load(fh)["kernels"][env_key(env)]
    got = run_env(env)
    rows = rows_of(env)
    assert sorted(want) == sorted(r[0] for r in rows)
    for rid, entry, _, shape, _ in rows:
        g, w = got[rid], want[rid]
        print(env_key(env), rid, g)
        if w["kernel"] is None:
            assert g["kernel"] is None, f"{rid}: the call must raise PrimxError, it launched {g['kernel']}"
        else:
            assert g["kernel"] == w["kernel"], f"{rid}: launched {g['kernel']}, recorded {w['kernel']}"
        # The Python restatements against what the library did.  (Not under PRIMX_GEMM_LOADER=0: fold_shapes_ok speaks for ALL GEMMs of
        # a DiT block, and the consumers without a V^T segment need the loader-wave kernel - it is False there although this one
        # call lands on the big tile; fold_pair_fits follows it.  The recorded values are held in every environment.)
        restates = "PRIMX_GEMM_LOADER" not in env
        if "fold_shapes_ok" in shape:
            assert g["fold_shapes_ok"] == w["fold_shapes_ok"], (rid, g)
            assert g["kernel"] is None or g["kernel"].startswith("gemm288q_"), (rid, g)
            if restates:      # False exactly where the call raises, True where it lands on the big tile
                assert g["fold_shapes_ok"] == (g["kernel"] is not None), (rid, g)
        if "fold_pair_fits" in shape:
            assert g["fold_pair_fits"] == w["fold_pair_fits"], (rid, g)
            if restates:
                assert g["fold_pair_fits"] == (g["kernel"] or "").startswith("gemm288q_pair_kernel<"), (rid, g)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child(int(sys.argv[1]))
