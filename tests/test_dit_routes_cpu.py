"""Which route does a 16-bit DiT forward take?  DiT._route16 decides it from plain values - shapes, switches, the planned row, the
library's capabilities - so the table below is asked on the `meta` device, without a GPU and without loading the library.  Every row
changes ONE thing against the base case (the shipped configuration: batch 1 under CFG, N = 2048, L = 1370, planned row 0 of 25,
default switches, every capability) and states the fields that change with it."""
import functools

import pytest
import torch

import topia_xl_amd as pkg
from topia_xl_amd import _lib, ops

ALL = frozenset({"fold", "blocks_call", "kv_ride", "f32out_group", "null_skip", "attn_ksplit", "toq64"})
DEFAULTS = dict(dedup_null_kv=True, null_xattn_skip=True, null_kv_once=True, collapse_null_cross_attention=False, cfg_streams=False,
                weight_prefetch=2, fuse_ln=True, ln_in_kernel=False, fold_ln=True, fold_max_steps=128, blocks_call=True, kv_ride=True,
                reuse_cond_kv=False)
D, DC = 1152, 768


@functools.lru_cache(maxsize=None)
def _model(H, depth):
    with torch.device("meta"):
        return pkg.DiT(seq_length=2048, in_channels=68, condition_channels=DC, hidden_size=D, depth=depth, num_heads=H,
                       cond_drop_prob=0.1).eval()


@pytest.fixture(autouse=True)
def _no_library(monkeypatch):
    # ops.fold_shapes_ok asks the library for "fold": answered from here; and the switches of the dispatch rule it restates are unset
    monkeypatch.setitem(_lib._caps, _lib.LIB_PATH, ALL)
    for name in ("PRIMX_GEMM_NOBIG", "PRIMX_GEMM_LOADER", "PRIMX_GEMM_BIGHEADS_MIN", "PRIMX_GEMM_PROF"):
        monkeypatch.delenv(name, raising=False)


def route(switches=None, *, B=1, N=2048, L=1370, H=16, depth=28, cfg=True, plan=(0, 25), profiling=False, probing=False,
          kv_cached=False, vrow_cached=False, caps=ALL):
    m = _model(H, depth)
    saved = {k: getattr(m, k) for k in DEFAULTS}
    try:
        for k, v in {**DEFAULTS, **(switches or {})}.items():
            setattr(m, k, v)
        Lk = ops.round_up(L, 256) if (ops.round_up(L, 256) - L) * 8 <= L else L          # DiT._cond_state
        row, steps = plan if plan is not None else (None, None)
        return m._route16(B, N, L, Lk, D, H, depth, DC, cfg, cfg and L >= 64, row, steps, profiling, probing,
                          lambda Bkv: kv_cached and m.reuse_cond_kv, vrow_cached, m._fold_ok, ops.fold_pair_fits, caps)
    finally:
        for k, v in saved.items():
            setattr(m, k, v)


def test_base_case_takes_the_one_call_route_with_riders_and_the_null_skip():
    r = route()
    assert (r.dedup, r.skip, r.fuse, r.fold, r.one_call, r.ride, r.need_kv, r.reads_null) == (True,) * 8
    assert (r.two_streams, r.ln_tail, r.collapse, r.ride_in_python) == (False,) * 4
    assert r.Bkv == 1 and r.wpf == 2
    assert all(type(v) is bool for k, v in r._asdict().items() if k not in ("Bkv", "wpf"))


T, F = True, False
ROWS = [
    ("vrow_cached", {}, dict(vrow_cached=True), dict(reads_null=F)),
    ("vrow_cached_null_kv_once_off", dict(null_kv_once=False), dict(vrow_cached=True), dict(reads_null=T)),
    ("blocks_call_off", dict(blocks_call=False), {}, dict(one_call=F, ride=T, ride_in_python=T)),
    ("kv_ride_off", dict(kv_ride=False), {}, dict(ride=F, one_call=T)),
    ("unplanned", {}, dict(plan=None), dict(fold=F, one_call=F, ride=F, skip=T, fuse=T)),
    ("weight_prefetch_1", dict(weight_prefetch=1), {}, dict(fuse=F, fold=F, one_call=F, wpf=1)),
    ("fuse_ln_off", dict(fuse_ln=False), {}, dict(fuse=F, fold=F, one_call=F)),
    ("fold_ln_off", dict(fold_ln=False), {}, dict(fold=F, one_call=F, ride=F, skip=T)),
    ("ln_in_kernel", dict(ln_in_kernel=True), {}, dict(ln_tail=T, fold=T, one_call=F, ride_in_python=T)),
    ("cfg_streams", dict(cfg_streams=True), {}, dict(two_streams=T, skip=F, fold=F, one_call=F, ride=F, dedup=T)),
    ("cfg_streams_profiling", dict(cfg_streams=True), dict(profiling=True), dict(two_streams=F, fold=T, skip=T, one_call=F)),
    ("profiling", {}, dict(profiling=True), dict(one_call=F, ride_in_python=T)),
    ("probing", {}, dict(probing=True), dict(one_call=F)),
    ("plan_of_129_steps", {}, dict(plan=(0, 129)), dict(fold=F)),
    ("null_xattn_skip_off", dict(null_xattn_skip=False), {}, dict(skip=F, reads_null=T)),
    ("dedup_null_kv_off", dict(dedup_null_kv=False), {}, dict(dedup=F, skip=F, Bkv=2)),
    ("collapse_under_the_skip", dict(collapse_null_cross_attention=True), {}, dict(collapse=F)),
    ("collapse_unplanned_without_skip", dict(collapse_null_cross_attention=True, null_xattn_skip=False), dict(plan=None), dict(collapse=T)),
    ("head_dim_144", {}, dict(H=8), dict(skip=F, fold=T)),
    ("L_32_no_broadcast_entry", {}, dict(L=32), dict(dedup=F, skip=F)),
    ("caps_without_null_skip", {}, dict(caps=ALL - {"null_skip"}), dict(skip=F)),
    ("caps_without_blocks_call", {}, dict(caps=ALL - {"blocks_call"}), dict(one_call=F)),
    ("caps_without_kv_ride", {}, dict(caps=ALL - {"kv_ride"}), dict(ride=F)),
    ("no_cfg_batch_2", {}, dict(cfg=False, B=2), dict(dedup=F, skip=F, fold=T, one_call=T, ride=F)),     # 192 + 96 tiles > 256
    ("no_cfg_batch_1", {}, dict(cfg=False), dict(fold=F)),                                                # 96 tiles < 160
    ("cfg_batch_8", {}, dict(B=8), dict(fold=T, skip=T, one_call=T, ride=F)),
    ("kv_cached_with_reuse_cond_kv", dict(reuse_cond_kv=True), dict(kv_cached=True), dict(need_kv=F, ride=F)),
    ("depth_0", {}, dict(depth=0), dict(dedup=F, two_streams=F, fold=F, need_kv=F)),
]


@pytest.mark.parametrize("switches, shape, expect", [pytest.param(*row[1:], id=row[0]) for row in ROWS])
def test_one_change_against_the_base_case(switches, shape, expect):
    got = route(switches, **shape)._asdict()
    assert {k: got[k] for k in expect} == expect
    # what holds on every route
    assert got["ride_in_python"] == (got["ride"] and not got["one_call"])
    assert got["Bkv"] == shape.get("B", 1) * (1 if got["dedup"] or not shape.get("cfg", True) else 2)
    assert not (got["collapse"] and got["skip"]) and not (got["one_call"] and got["two_streams"])
    assert got["ln_tail"] <= got["fuse"] and got["fold"] <= got["fuse"] and got["one_call"] <= got["fold"] and got["ride"] <= got["need_kv"]


def test_kv_cached_is_only_asked_with_blocks_to_project_for():
    asked = []
    m = _model(16, 0)
    m._route16(1, 2048, 1370, 1536, D, 16, 0, DC, True, True, 0, 25, False, False, lambda Bkv: asked.append(Bkv) or False, False,
               m._fold_ok, ops.fold_pair_fits, ALL)
    assert asked == []
    m = _model(16, 28)
    r = m._route16(1, 2048, 1370, 1536, D, 16, 28, DC, True, True, 0, 25, False, False, lambda Bkv: asked.append(Bkv) or False, False,
                   m._fold_ok, ops.fold_pair_fits, ALL)
    assert asked == [r.Bkv]
