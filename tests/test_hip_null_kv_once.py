"""`DiT.null_kv_once` (default on): the broadcast K / V entry of the unconditional half (Kn / Vn) depends on the null embedding and
the packed weights only, and a forward that takes the null cross-attention skip reads nothing of it once its conditioning state
holds the value rows - so it is projected ONCE per conditioning state, not in every forward.

  * by ops.PROFILE tags: the first forward of a conditioning state launches the null projection, the second and third do not
    (with null_kv_once = False every forward does);
  * a planned loop's samples equal those of a model that re-projects in every forward, bit for bit;
  * a forward that READS Kn / Vn after skipped forwards - skip switched off on the live model, after repack(), with a second
    conditioning tensor - equals a fresh model's."""
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, HEADS, DEPTH, N, L, DC, SEED = 576, 8, 3, 256, 129, 768, 91
F16 = torch.float16


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd
    return topia_xl_amd


def _model(pkg):
    cfg = dict(in_channels=68, condition_channels=DC, hidden_size=D, depth=DEPTH)
    m = pkg.DiT(seq_length=N, num_heads=HEADS, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    m.load_state_dict(synth.dit_state_dict(SEED, **cfg))
    m.to(DEV)
    assert m.null_xattn_skip and m.dedup_null_kv and m.null_kv_once and not m.cfg_streams, "the suite runs with the default switches"
    return m


@pytest.fixture(scope="module")
def data():
    x = synth.tensor(SEED, "x", (1, N, 68)).to(DEV)
    return x, synth.tensor(SEED, "y", (1, L, DC)).to(DEV), synth.tensor(SEED + 1, "y", (1, L, DC)).to(DEV)


def _fwd(m, x, y, t=520):
    return m.forward_with_cfg(x, torch.tensor([t] * x.shape[0], device=DEV), y, 6.0, F16, True).clone()


def _null_projections(pkg, m, x, y):
    """The null projection's launches in one profiled forward: the heads GEMM over ops.bcast_keys(L) rows, all blocks' [to_k; to_v]."""
    from topia_xl_amd import ops
    ops.PROFILE = tags = []
    try:
        _fwd(m, x, y)
    finally:
        ops.PROFILE = None
    return sum(1 for t in tags if t[0].endswith(f" {ops.bcast_keys(L)}x{DEPTH * 2 * D}x{DC}"))


def test_projected_once_per_conditioning_state(pkg, data):
    x, y, y2 = data
    m = _model(pkg)
    assert [_null_projections(pkg, m, x, y) for _ in range(3)] == [1, 0, 0]
    assert [_null_projections(pkg, m, x, y2) for _ in range(2)] == [1, 0]       # another conditioning tensor: its first forward projects
    m.null_xattn_skip = False                                                  # the broadcast attention reads the entry: every forward
    assert [_null_projections(pkg, m, x, y2) for _ in range(2)] == [1, 1]
    m.null_xattn_skip, m.null_kv_once = True, False                            # the switch off: every forward, as before
    assert [_null_projections(pkg, m, x, y.clone()) for _ in range(1)] == [1]
    yc = y.clone()
    assert [_null_projections(pkg, m, x, yc) for _ in range(3)] == [1, 1, 1]


def test_outputs_equal_a_model_that_projects_every_forward(pkg, data):
    from tests.test_hip_null_skip import _loop, _same
    x, y, _ = data
    once, every = _model(pkg), _model(pkg)
    every.null_kv_once = False
    _same(_loop(pkg, once, x, y, F16), _loop(pkg, every, x, y, F16))            # a planned 3-step loop, every step's sample
    _same([_fwd(once, x, y, t) for t in (900, 520, 33)], [_fwd(every, x, y, t) for t in (900, 520, 33)])   # unplanned forwards, one state


def test_readers_after_skipped_forwards_see_a_fresh_model_s_bytes(pkg, data):
    from tests.test_hip_null_skip import _same
    x, y, y2 = data
    live, fresh_off = _model(pkg), _model(pkg)
    fresh_off.null_xattn_skip = False
    want_off, want_off2 = _fwd(fresh_off, x, y), _fwd(fresh_off, x, y2)
    fresh_on = _model(pkg)
    want_on2 = _fwd(fresh_on, x, y2)

    _fwd(live, x, y), _fwd(live, x, y)                                          # two forwards that skip (the second projects nothing)
    live.null_xattn_skip = False
    _same(_fwd(live, x, y), want_off)                                           # the broadcast attention reads Kn / Vn
    live.null_xattn_skip = True
    _fwd(live, x, y), _fwd(live, x, y)
    live.repack()                                                               # new buffers, new conditioning state
    live.null_xattn_skip = False
    _same(_fwd(live, x, y), want_off)
    live.null_xattn_skip = True
    _fwd(live, x, y), _fwd(live, x, y)
    _same(_fwd(live, x, y2), want_on2)                                          # a second conditioning tensor: its value rows come from Vn
    _fwd(live, x, y2)
    live.null_xattn_skip = False
    _same(_fwd(live, x, y2), want_off2)
    live.null_xattn_skip = True
