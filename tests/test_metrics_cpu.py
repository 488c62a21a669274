"""tests/metrics_numpy.py and the Python surface of the quality metrics without a GPU: the restated rules on cases with known
answers, the ABI bookkeeping of primx_nearest_points and primx_distance_stats, the closure of the stream-order table once
tests/test_hip_metrics.py has registered its case, and the wrappers' argument checks."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_numpy as MN
from tests import test_hip_metrics as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("primx_nearest_points", "primx_distance_stats")
DTYPES = (np.float32, np.float64)


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_planes_give_h_exactly(dtype):
    h = 0.125
    a, b, na, nb = MN.two_planes(8, h)
    got = MN.compare_points(a, b, na, nb, (0.0625, h, 0.25), dtype=dtype)
    assert got["accuracy"] == got["completeness"] == got["hausdorff"] == got["chamfer_l1"] == h
    assert got["chamfer_l2"] == 2 * h * h and got["normal_consistency"] == 1.0
    assert got["precision"] == got["recall"] == got["fscore"] == {0.0625: 0.0, h: 1.0, 0.25: 1.0}     # 0 below h, 1 at and above it
    d, i = MN.nearest(a, b, dtype)
    assert d.dtype == dtype and i.dtype == np.int32 and i.tolist() == list(range(64))                # each point's own partner


def test_fscore_is_zero_when_nothing_is_close():
    rows = [1.0, 1.0, 1.0, 0.0, 0.0], [1.0, 1.0, 1.0, 0.0, 3.0]
    out = MN.report(rows[0], rows[0], 4, 4, (0.5,), False)
    assert out["precision"][0.5] == out["recall"][0.5] == 0.0 and out["fscore"][0.5] == 0.0 and "normal_consistency" not in out
    one = MN.report(rows[0], rows[1], 4, 4, (0.5,), False)                                             # P = 0, R = 3 / 4
    assert one["fscore"][0.5] == 0.0 and one["recall"][0.5] == 0.75
    from topia_xl_amd import metrics
    for r in (rows[0], rows[1]):
        assert metrics._report(rows[0], r, 4, 4, (0.5,), False) == MN.report(rows[0], r, 4, 4, (0.5,), False)
    full = [3.0, 2.5, 1.5, 3.5, 2.0, 4.0], [8.0, 9.0, 2.0, 6.0, 1.0, 8.0]
    assert metrics._report(full[0], full[1], 4, 8, (0.1, 0.2), True) == MN.report(full[0], full[1], 4, 8, (0.1, 0.2), True)
    got = MN.report(full[0], full[1], 4, 8, (0.1, 0.2), True)
    assert got["accuracy"] == 0.75 and got["completeness"] == 1.0 and got["chamfer_l1"] == 0.875 and got["chamfer_l2"] == 0.625 + 1.125
    assert got["hausdorff"] == 2.0 and got["normal_consistency"] == (3.5 / 4 + 6.0 / 8) / 2
    assert got["fscore"][0.1] == 2 * 0.5 * 0.125 / 0.625 and got["fscore"][0.2] == 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_go_to_the_lowest_index_and_non_finite_pairs_never_win(dtype):
    b = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [1, 0, 0], [0, -1, 0]])
    a = np.float32([[0, 0, 0], [1, 0, 0], [0, 0.5, 0], [np.nan, 0, 0]])
    d, i = MN.nearest(a, b, dtype)
    assert i.tolist() == [0, 0, 2, 0] and d[:3].tolist() == [1.0, 0.0, 0.5] and np.isinf(d[3])
    d, i = MN.nearest(a[:3], np.float32([[np.inf, 0, 0], [0, 0, 2]]), dtype)
    assert i.tolist() == [1, 1, 1]
    d, i = MN.nearest(a[:3], np.float32([[np.inf, 0, 0]]), dtype)
    assert i.tolist() == [0, 0, 0] and bool(np.isinf(d).all())
    TM.test_the_tie_cases_have_the_ties_they_claim()


def test_stats_restatement():
    dist = np.float32([0.5, 0.25, 2.0, 0.25])
    na = np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1]])
    nb = np.float32([[0, 0, 1], [1, 0, 0]])
    out = MN.stats(dist, np.int32([1, 1, 0, 0]), na, nb, (0.25, 0.3, 2.0))
    assert out == [3.0, 0.25 + 0.0625 + 4.0 + 0.0625, 2.0, 3.0, 2.0, 2.0, 4.0]                        # <=: a tau equal to a dist counts it
    assert MN.stats(dist, thresholds=(1.0,)) == [3.0, 4.375, 2.0, 0.0, 3.0]
    assert MN.stats(np.float32([])) == [0.0, 0.0, 0.0, 0.0]
    # the fp32 compare: 0.1 as a double lies below float32(0.1), which is what the kernel is given
    assert MN.stats(np.float32([0.1]), thresholds=(0.1,))[4] == 1.0


def test_float32_restatement_is_within_the_derived_bound_of_float64():
    """The bound of tests/test_hip_metrics.py (4 x 2^-24, derived there) holds for the float32 restatement on this CPU."""
    worst = 0.0
    for scale in (1e-3, 1.0, 1e3):
        rng = np.random.default_rng(int(round(math.log10(scale))) + 20)
        a = (scale * rng.uniform(-1, 1, (600, 3))).astype(np.float32)
        b = (scale * rng.uniform(-1, 1, (577, 3))).astype(np.float32)
        d64, d32 = MN.nearest(a, b, np.float64)[0], MN.nearest(a, b, np.float32)[0].astype(np.float64)
        worst = max(worst, float((np.abs(d32 - d64) / d64).max()) / TM.U)
    print(f"float32 restatement against float64: {worst:.2f} x 2^-24")
    assert worst <= 4.0


# ------------------------------------------------------------------------------------------------ 2. ABI
HOST_FLOATS = {"tau"}                    # `const float*` arguments in HOST memory: bound as POINTER(c_float)


@pytest.mark.parametrize("name,names", [
    (NAMES[0], ["a", "n", "b", "m", "dist", "idx", "stream"]),
    (NAMES[1], ["dist", "idx", "na", "nb", "n", "tau", "T", "ws", "ws_bytes", "out", "stream"])])
def test_abi_35_declares_the_entry_points_with_the_bound_signatures(name, names):
    from topia_xl_amd import _lib
    assert _lib.ABI_VERSION == 35 and _lib._SINCE[name] == 35 and name not in _lib._FEATURES.values() and _lib._PROBE == 0
    with open(os.path.join(ROOT, "include", "primx_hip.h")) as fh:
        text = fh.read()
    assert "#define PRIMX_ABI_VERSION 35" in text
    section = text[text.index(" * Quality metrics ("):]
    assert "added to ABI 35 without a new number" in section and "24576 bytes" in section and "8-byte aligned, any contents" in section
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", section)
    assert m, "the header's section does not declare it"
    ctype = {"const float*": _lib._p, "float*": _lib._p, "const int*": _lib._p, "int*": _lib._p, "double*": _lib._p, "void*": _lib._p,
             "int": _lib._i, "int64_t": _lib._l}
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[1] for a in args] == names
    want = [_lib.C.POINTER(_lib._f) if a.rsplit(" ", 1)[1] in HOST_FLOATS else ctype[a.rsplit(" ", 1)[0]] for a in args]
    assert want == _lib.SIGNATURES[name]


def test_an_ab_build_of_version_35_from_before_the_metrics_still_loads(monkeypatch, tmp_path):
    from tests import test_lib_capabilities_cpu as TL
    from topia_xl_amd import _lib
    rest = set(_lib.SIGNATURES) - set(NAMES)
    lib = TL.StandIn(35, rest)
    assert TL._load(monkeypatch, tmp_path, lib) == TL.ALL and lib.bound() == rest
    with pytest.raises(AttributeError):                               # ... and as the package's own library it is refused
        TL._load(monkeypatch, tmp_path, lib, ab=False)
    one = TL.StandIn(35, rest | {NAMES[0]})                           # each of the two is probed on its own
    assert TL._load(monkeypatch, tmp_path, one) == TL.ALL and one.bound() == rest | {NAMES[0]}


def test_the_kernels_constants_are_the_modules():
    from topia_xl_amd import metrics
    with open(os.path.join(ROOT, "3dtopia-xl_amd", "csrc", "metrics.hip")) as fh:
        src = fh.read()
    const = {k: int(v) for k, v in re.findall(r"constexpr int (\w+) = (\d+);", src)}
    assert "#pragma clang fp contract(off)" in src and not re.search(r"\batomic[A-Z]\w*\(", src)       # no atomic call at all
    assert (const["NN_CHUNK"], const["NN_WIDE"], const["ST_MAXB"], const["ST_PER_BLOCK"], const["ST_MAXT"]) == \
        (metrics.NEAREST_CHUNK, metrics.NEAREST_WIDE, metrics.STATS_BLOCKS, metrics.STATS_PER_BLOCK, metrics.MAX_THRESHOLDS)
    assert sorted(int(p) for p in re.findall(r"nn_kernel<(\d)>", src)) == [1, 4]
    assert metrics.STATS_WS_BYTES == 24576 and (TM.C, TM.B, TM.WIDE, TM.SLICE) == \
        (metrics.NEAREST_CHUNK, metrics.NEAREST_THREADS, metrics.NEAREST_WIDE, 256 * 1024)
    with open(os.path.join(ROOT, "3dtopia-xl_amd", "csrc", "mesh_common.h")) as fh:
        assert f"constexpr int THREADS = {metrics.NEAREST_THREADS};" in fh.read()
    with open(os.path.join(ROOT, "3dtopia-xl_amd", "csrc", "build.py")) as fh:
        assert '"metrics.hip"' in fh.read()


# ------------------------------------------------------------------------------------------------ 3. stream table, validation
def test_stream_table_is_closed_with_the_metrics_case():
    from tests import test_hip_material, test_hip_normalmap, test_hip_occlusion, test_hip_primsdf_grad, test_hip_raymarch_grad  # noqa: F401  (the other registering modules)
    from tests import test_hip_streams as TS
    from tests import test_streamorder_cpu as TC
    assert TM.STREAM_CASE in TS.CASES and set(NAMES) <= set(TS.declared())
    TC.test_every_stream_taking_entry_point_is_declared_by_a_case()
    TC.test_every_declared_name_is_a_stream_taking_prototype()
    TC.test_case_table_is_well_formed()
    assert not [n for n, _ in TS.PARAMS if n == TM.STREAM_CASE]       # it runs in its own module, not twice
    assert TM.STREAM_CASE not in TS.MUST_SYNC and TM.STREAM_CASE not in TS.FIRST_CALL_MAY_SYNC       # no synchronisation is documented


def test_wrappers_refuse_cpu_tensors_and_bad_arguments():
    from topia_xl_amd import metrics, pipeline
    p, q = torch.zeros(5, 3), torch.zeros(7, 3)
    for call in (lambda: metrics.nearest_points(p, q), lambda: metrics.distance_stats(torch.zeros(5)),
                 lambda: metrics.distance_stats(torch.zeros(5), torch.zeros(5, dtype=torch.int32), p, q, (0.1,)),
                 lambda: metrics.compare_points(p, q), lambda: metrics.compare_points(p, q, p, q)):
        with pytest.raises(RuntimeError, match="HIP device"):
            call()
    for call in (lambda: metrics.nearest_points(torch.zeros(5, 2), q), lambda: metrics.nearest_points(p, torch.zeros(7)),
                 lambda: metrics.nearest_points(p, torch.zeros(0, 3)),                        # m = 0
                 lambda: metrics.distance_stats(torch.zeros(5), thresholds=[0.1] * 9),          # T > 8
                 lambda: metrics.distance_stats(torch.zeros(5, 1)),
                 lambda: metrics.distance_stats(torch.zeros(5), None, p, q),                    # normals without idx
                 lambda: metrics.distance_stats(torch.zeros(5), torch.zeros(4, dtype=torch.int32), p, q),
                 lambda: metrics.compare_points(p, torch.zeros(0, 3)), lambda: metrics.compare_points(p, q, p, p),
                 lambda: metrics.compare_points(p, q, thresholds=[0.1] * 9)):
        with pytest.raises(ValueError):
            call()
    assert metrics.DEFAULT_THRESHOLDS == (0.01, 0.02, 0.05)
    s = inspect.signature(metrics.compare_meshes).parameters
    assert (s["n"].default, s["seed"].default, s["surface"].default, s["thresholds"].default) == (100_000, 0, False, (0.01, 0.02, 0.05))
    assert inspect.signature(metrics.compare_to_field).parameters["resolution"].default == 256
    assert list(inspect.signature(pipeline.primitives_vs_mesh).parameters) == ["recon_param_b", "mesh", "resolution", "kw"]
    assert "single synchronisation" in metrics.compare_points.__doc__ and "sampling spacing" in metrics.compare_meshes.__doc__
