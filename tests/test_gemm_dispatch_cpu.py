"""The case table of tests/test_hip_gemm_dispatch.py and its recorded golden, without a GPU: every kernel name that csrc/gemm.hip can
report (the format strings of its PRIMX_NOTE_KERNEL sites) occurs among the recorded names, every GEMM switch is set by some row,
and the golden has exactly the table's rows."""
import json
import os
import re

from tests import test_hip_gemm_dispatch as T

GEMM = os.path.join(T.ROOT, "3dtopia-xl_amd", "csrc", "gemm.hip")
SWITCHES = ["PRIMX_GEMM_NOBIG", "PRIMX_GEMM_LOADER", "PRIMX_GEMM_BIG_MIN", "PRIMX_GEMM_BIGHEADS_MIN", "PRIMX_GEMM_XCD2D", "PRIMX_LN_FUSE",
            "PRIMX_LN_MODE", "PRIMX_LN_FUSE_MAXGRID", "PRIMX_GEMM_PROF", "PRIMX_GEMM_KT32", "PRIMX_GEMM_KT64_MIN", "PRIMX_GEMM_HEADS_KT32",
            "PRIMX_GEMM_NOGEMV", "PRIMX_F32OUT_TILE144"]


def _golden():
    with open(T.GOLDEN) as fh:
        return json.load(fh)


def note_formats(text):
    """The format strings of the PRIMX_NOTE_KERNEL("...", ...) call sites (not the macro's definition)."""
    return sorted(set(re.findall(r'PRIMX_NOTE_KERNEL\(\s*"([^"]+)"', text)))


def test_parser_finds_the_format_strings():
    text = '#define PRIMX_NOTE_KERNEL(...) snprintf(x, __VA_ARGS__)\n  PRIMX_NOTE_KERNEL("a_kernel<%d, %d, 64>", DT, EPI);\nPRIMX_NOTE_KERNEL( "b<%d>", DT);'
    assert note_formats(text) == ["a_kernel<%d, %d, 64>", "b<%d>"]
    with open(GEMM) as fh:
        fmts = note_formats(fh.read())
    families = {f.split("<")[0] for f in fmts}
    assert families == {"gemm_kernel", "gemm144_dma_kernel", "gemm144l_dma_kernel", "gemm288q_dma_kernel", "gemm288q_pair_kernel",
                        "gemv16_kernel", "f32out_group_kernel"}, families


def test_every_reportable_kernel_name_is_recorded_for_some_row():
    with open(GEMM) as fh:
        fmts = note_formats(fh.read())
    names = {r["kernel"] for rows in _golden()["kernels"].values() for r in rows.values() if r["kernel"]}
    for f in fmts:      # finer than the family: each format string (tile shape, ring width) with any template arguments
        rx = re.compile("^" + re.escape(f).replace("%d", r"\d+") + "$")
        assert any(rx.match(n) for n in names), f"no row of the table lands on {f}"
    for n in names:
        assert any(re.match("^" + re.escape(f).replace("%d", r"\d+") + "$", n) for f in fmts), f"{n}: no such name in gemm.hip"


def test_every_switch_is_set_by_some_row():
    with open(GEMM) as fh:
        text = fh.read()
    used = {k for env in T.ENVS for k in env}
    for s in SWITCHES:
        assert f'"{s}"' in text, f"{s} is not read by gemm.hip"
        assert s in used, f"no row of the table sets {s}"
    assert used <= set(SWITCHES)


def test_golden_has_exactly_the_rows_of_the_table():
    g = _golden()
    assert len(g["recorded_at_commit"]) >= 7
    assert sorted(g["kernels"]) == sorted(T.env_key(e) for e in T.ENVS)
    for env in T.ENVS:
        ids = [r[0] for r in T.rows_of(env)]
        assert len(ids) == len(set(ids)), T.env_key(env)
        assert sorted(g["kernels"][T.env_key(env)]) == sorted(ids), T.env_key(env)
    rejected = [r for rows in g["kernels"].values() for r in rows.values() if r["kernel"] is None]
    assert rejected, "the table must hold rejected calls too"
