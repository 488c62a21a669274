"""The routes of DiT._forward16 held to each other on ONE small model: full width (1152, 16 heads, 68 in, 768 conditioning channels),
depth 4, N = 2048, L = 1370, batch 1, fp16 - a configuration on which a planned loop folds, takes the one-call route and carries the
K / V riders (tests/test_dit_routes_cpu.py states which switch moves which field of the route).  Depth 4, not 2: the batched K / V
projection that `kv_ride` off issues is 6 x 8 x depth tiles and takes the riders' 256 x 288 tile from 160 tiles on; at depth 2 it
runs on the 128 x 144 kernel and the operands differ at rounding level (tests/test_hip_fold.py, the same note).

  * planned forward_with_cfg: the default, `blocks_call` / `kv_ride` / `null_xattn_skip` / `null_kv_once` off give the same bits;
  * unplanned forward_with_cfg: the default, `fuse_ln` off, `weight_prefetch` 0 and 1 give the same bits.  (`cfg_streams` is not
    among them: it launches half-size GEMMs, which take other tiles and sum in another order - tests/test_hip_dit.py holds it to 2e-3
    of the default and to itself across `fuse_ln` - and a side stream made here would move tests/test_hip_streams.py's two streams
    onto other hardware queues: that module counts on three streams besides stream 0 in the process);
  * with ops.PROFILE on, a planned forward emits the same tag list twice in a row;
  * primx_dit_blocks_fold is called for a whole forward once per forward on the default route and never with `blocks_call` off
    (there the null skip's two single launches per block go through it, PrimxDitForwardFold::only_launch, and nothing else does)."""
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEPTH, N, L, SEED = 4, 2048, 1370, 97
F16 = torch.float16
STEPS = (900, 520)          # two planned rows on one conditioning state: the second forward finds the value rows cached


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd
    return topia_xl_amd


@pytest.fixture(scope="module")
def model(pkg):
    cfg = dict(in_channels=68, condition_channels=768, hidden_size=1152, depth=DEPTH)
    m = pkg.DiT(seq_length=N, num_heads=16, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    m.load_state_dict(synth.dit_state_dict(SEED, **cfg))
    m.to(DEV)
    assert (m.null_xattn_skip and m.dedup_null_kv and m.null_kv_once and m.blocks_call and m.kv_ride and m.fuse_ln and m.fold_ln
            and m.weight_prefetch == 2 and not m.cfg_streams and not m.ln_in_kernel), "the suite runs with the default switches"
    return m


@pytest.fixture(scope="module")
def data():
    return synth.tensor(SEED, "x", (1, N, 68)).to(DEV), synth.tensor(SEED, "y", (1, L, 768)).to(DEV)


def _planned(m, x, y):
    """forward_with_cfg at every planned row, on a new conditioning state (the first forward projects the broadcast entry)."""
    m._cond = None
    ts = torch.tensor(STEPS, dtype=torch.int64, device=DEV)
    m.plan_timesteps(ts)
    try:
        outs = []
        for i in range(len(STEPS)):
            m.select_planned_timestep(i)
            outs.append(m.forward_with_cfg(x, ts[i:i + 1], y, 6.0, F16, True).clone())
        return outs
    finally:
        m.clear_timestep_plan()


def _unplanned(m, x, y):
    m._cond = None
    return [m.forward_with_cfg(x, torch.tensor([t], device=DEV), y, 6.0, F16, True).clone() for t in STEPS]


@pytest.fixture(scope="module")
def planned_default(model, data):
    return _planned(model, *data)


@pytest.fixture(scope="module")
def unplanned_default(model, data):
    return _unplanned(model, *data)


def _with(m, run, data, **switches):
    saved = {k: getattr(m, k) for k in switches}
    try:
        for k, v in switches.items():
            setattr(m, k, v)
        return run(m, *data)
    finally:
        for k, v in saved.items():
            setattr(m, k, v)


@pytest.mark.parametrize("switch", [dict(blocks_call=False), dict(kv_ride=False), dict(null_xattn_skip=False), dict(null_kv_once=False)],
                         ids=lambda s: "-".join(f"{k}={v}" for k, v in s.items()))
def test_planned_routes_give_the_same_bits(model, data, planned_default, switch):
    assert model._fold_ok(2 * N, N), "the planned forwards of this file fold"
    got = _with(model, _planned, data, **switch)
    for a, b in zip(got, planned_default):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("switch", [dict(fuse_ln=False), dict(weight_prefetch=0), dict(weight_prefetch=1)],
                         ids=lambda s: "-".join(f"{k}={v}" for k, v in s.items()))
def test_unplanned_routes_give_the_same_bits(model, data, unplanned_default, switch):
    got = _with(model, _unplanned, data, **switch)
    for a, b in zip(got, unplanned_default):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_profiled_planned_forward_emits_the_same_tags_twice(model, data, planned_default):
    from topia_xl_amd import ops
    x, y = data
    m = model
    ts = torch.tensor(STEPS, dtype=torch.int64, device=DEV)
    m.plan_timesteps(ts)
    try:
        m.select_planned_timestep(0)
        m.forward_with_cfg(x, ts[:1], y, 6.0, F16, True)          # (the loop's tables and the value rows exist from here on)
        lists = []
        for _ in range(2):
            ops.PROFILE = tags = []
            try:
                out = m.forward_with_cfg(x, ts[:1], y, 6.0, F16, True)
            finally:
                ops.PROFILE = None
            lists.append([t[0] for t in tags])
    finally:
        m.clear_timestep_plan()
    assert lists[0] == lists[1] and len(lists[0]) >= 8 * DEPTH
    assert torch.equal(out, planned_default[0])                  # (per-launch timing issues the same launches from Python)


def test_whole_forward_calls_of_primx_dit_blocks_fold(model, data, planned_default):
    from topia_xl_amd import _lib
    lib = _lib.load()
    calls = []
    real = lib.primx_dit_blocks_fold

    class Spy:          # (ctypes function objects cannot be monkeypatched in place: wrap the attribute)
        def __call__(self, f, *a):
            calls.append(f._obj.only_launch)
            return real(f, *a)
    lib.primx_dit_blocks_fold = Spy()
    try:
        _planned(model, *data)
        default, calls[:] = list(calls), []
        _with(model, _planned, data, blocks_call=False)
        python_loop, calls[:] = list(calls), []
        _with(model, _planned, data, blocks_call=False, null_xattn_skip=False)
        python_loop_walk = list(calls)
    finally:
        lib.primx_dit_blocks_fold = real
    assert default == [0] * len(STEPS)                                           # one call per forward, for the whole forward
    # never for a whole forward; under the null skip block i's to_q (i >= 1) and cross proj have no entry point of their own
    assert python_loop == ([2] + [1, 2] * (DEPTH - 1)) * len(STEPS)
    assert python_loop_walk == []
