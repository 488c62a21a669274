"""tests/streamorder.py and the case table of tests/test_hip_streams.py, without a GPU: every prototype of include/primx_hip.h
that takes a `void* stream` is declared by some case (no exemption list), every declared name is such a prototype, and the
verdict bookkeeping classifies fabricated event outcomes as the kind they are."""
import os

from tests import streamorder as so
from tests import test_hip_streams as TS

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "primx_hip.h")


def _prototypes():
    with open(HEADER) as fh:
        return so.stream_prototypes(fh.read())


def test_header_parser_finds_the_stream_taking_prototypes():
    text = """/* int primx_in_a_comment(int a, void* stream); */
    int primx_one(const float* x, int n, void* stream);
    int primx_two(const float* x,
                  int64_t n,   // a comment with void* stream
                  void *stream);
    int primx_no_stream(int nx, int64_t* bytes);
    const char* primx_last_error(void);"""
    assert so.stream_prototypes(text) == ["primx_one", "primx_two"]
    names = _prototypes()
    assert len(names) == len(set(names)) and len(names) >= 79
    for must in ("primx_linear", "primx_dit_blocks_fold", "primx_fps", "primx_prefetch", "primx_meshdecim_collapse", "primx_raymarch"):
        assert must in names
    assert "primx_mcubes_workspace" not in names and "primx_abi_version" not in names


def test_every_stream_taking_entry_point_is_declared_by_a_case():
    missing = sorted(set(_prototypes()) - set(TS.declared()))
    assert not missing, f"no case of tests/test_hip_streams.py declares {missing}"


def test_every_declared_name_is_a_stream_taking_prototype():
    unknown = sorted(set(TS.declared()) - set(_prototypes()))
    assert not unknown, f"declared, but not a prototype with a stream of include/primx_hip.h: {unknown}"
    from topia_xl_amd._lib import SIGNATURES
    assert set(TS.declared()) <= set(SIGNATURES)


def test_case_table_is_well_formed():
    assert set(TS.MUST_SYNC) <= set(TS.CASES) and set(TS.FIRST_CALL_MAY_SYNC) <= set(TS.CASES)
    assert not set(TS.MUST_SYNC) & set(TS.FIRST_CALL_MAY_SYNC)
    for name, reason in list(TS.MUST_SYNC.items()) + list(TS.FIRST_CALL_MAY_SYNC.items()):
        assert len(reason) > 20, name                               # a reason, not a flag
    for c in TS.CASES.values():
        assert c.declares and callable(c.build) and c.dtypes, c.name


def test_classification_of_fabricated_outcomes():
    diff = ["result: 8 of 64 bytes differ"]
    # (a) a difference is an order violation whatever the events say
    for null_done in (False, True):
        for late in ([False], [True]):
            for must in (False, True):
                assert so.classify(diff, null_done, late, must) == so.ORDER
    # (b) no difference, but stream 0's blocker had ended: inconclusive - never ok
    for late in ([False], [True]):
        for must in (False, True):
            assert so.classify([], True, late, must) == so.INCONCLUSIVE
    # (c) the host waited and no synchronisation is documented
    assert so.classify([], False, [True], False) == so.SYNCHRONISED
    assert so.classify([], False, [False, False, True], False) == so.SYNCHRONISED      # one step of a loop
    assert so.classify([], False, [True], True) == so.OK                               # documented
    assert so.classify([], False, [False], False) == so.OK
    assert so.classify([], False, [False, False], False) == so.OK


def test_report_messages_are_distinct():
    kinds = {so.Report("c", ["x: differs"], False, [False], False).message(),
             so.Report("c", [], True, [False], False, null_ms=5.0).message(),
             so.Report("c", [], False, [True], False, s_ms=10.0).message(),
             so.Report("c", [], False, [False], False).message()}
    assert len(kinds) == 4
    r = so.Report("c", [], True, [False], False, s_ms=10.0, null_ms=40.0, host_ms=1.5)
    assert r.verdict == so.INCONCLUSIVE and "(b)" in r.message() and "inconclusive" in r.line() and "40 ms" in r.line()
    assert "(a)" in so.Report("c", ["x"], True, [True], True).message()
    assert "(c)" in so.Report("c", [], False, [True], False).message()
