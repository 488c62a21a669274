"""`DiT.null_xattn_skip` (default on): under classifier-free guidance the unconditional entries' to_q and cross-attention walk are
not run - their only possible result is the value row (tests/test_hip_null_identity.py) - and the cross proj reads that row as
every unconditional row of its A operand.  The samples of a planned DDIM loop and a single forward_with_cfg must be the same to the
last bit with the skip on and off: on the one-call route with the K / V riders (the default), on the Python block loop, without
the riders, and in an unplanned (unfolded) forward; with the skip on the cross-attention launch covers B x H problems."""
import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, HEADS, DEPTH, SEED = 2048, 1370, 16, 4, 91


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd
    return topia_xl_amd


@pytest.fixture(scope="module")
def model(pkg):
    """Depth 4 at full width, as tests/test_hip_fold.py builds it: the smallest configuration on which the planned loop folds, takes
    the one-call route and the riders' bit-identity with the batched projection holds."""
    cfg = dict(in_channels=68, condition_channels=768, hidden_size=1152, depth=DEPTH)
    m = pkg.DiT(seq_length=N, num_heads=HEADS, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    m.load_state_dict(synth.dit_state_dict(SEED, **cfg))
    m.to(DEV)
    assert m.null_xattn_skip and m.dedup_null_kv and not m.cfg_streams, "the suite runs with the default switches"
    return m


def _inputs(batch):
    return synth.tensor(SEED, "x", (batch, N, 68)).to(DEV), synth.tensor(SEED, "y", (batch, L, 768)).to(DEV)


def _loop(pkg, m, x, y, dtype):
    d = pkg.create_diffusion("ddim3", noise_schedule="squaredcos_cap_v2", parameterization="v")
    kw = dict(y=y, cfg_scale=6.0, precision_dtype=dtype, enable_amp=True)
    return [o["sample"].clone() for o in d.ddim_sample_loop_progressive(m.forward_with_cfg, tuple(x.shape), noise=x, clip_denoised=False,
                                                                        model_kwargs=kw)]


def _planned_forward(m, x, y, dtype):
    t = torch.tensor([520] * x.shape[0], device=DEV)
    m.plan_timesteps(t[:1])
    m.select_planned_timestep(0)
    try:
        return m.forward_with_cfg(x, t, y, 6.0, dtype, True).clone()
    finally:
        m.clear_timestep_plan()


def _on_and_off(m, fn):
    out = {}
    for on in (False, True):
        m.null_xattn_skip = on
        try:
            out[on] = fn()
        finally:
            m.null_xattn_skip = True
    return out[False], out[True]


def _same(a, b):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            _same(u, v)
    else:
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ, largest difference {float((a.float() - b.float()).abs().max()):.3e}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("batch", [1, 2])
def test_skip_is_bit_identical_on_the_default_route(pkg, model, dtype, batch):
    x, y = _inputs(batch)
    _same(*_on_and_off(model, lambda: _loop(pkg, model, x, y, dtype)))                  # every step's sample, the final one included
    _same(*_on_and_off(model, lambda: _planned_forward(model, x, y, dtype)))            # forward_with_cfg, planned (folded)
    t = torch.tensor([520] * batch, device=DEV)
    _same(*_on_and_off(model, lambda: model.forward_with_cfg(x, t, y, 6.0, dtype, True).clone()))   # unplanned (LayerNorm launches)


@pytest.mark.parametrize("flag", ["blocks_call", "kv_ride"])
def test_skip_is_bit_identical_without_the_one_call_route_or_the_riders(pkg, model, flag):
    """PRIMX_DIT_BLOCKS_CALL=0 / PRIMX_DIT_KV_RIDE=0 set these attributes at construction."""
    x, y = _inputs(1)
    assert getattr(model, flag) is True
    setattr(model, flag, False)
    try:
        off, on = _on_and_off(model, lambda: _loop(pkg, model, x, y, torch.float16))
    finally:
        setattr(model, flag, True)
    _same(off, on)
    _same(on, _loop(pkg, model, x, y, torch.float16))                                   # ... and the same as the default route's


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_skip_is_bit_identical_on_the_big_tiles(pkg, model, dtype):
    """Batch 8 (T = 32768 token rows): to_q over the 16384 conditional rows and the cross proj over all rows both take the 256 x 288
    kernel - its form of the mirrored statistics and of the one-row A source; batch 1 and 2 above run both on the 128 x 144 kernel."""
    from topia_xl_amd import ops
    x, y = _inputs(8)
    _same(*_on_and_off(model, lambda: _planned_forward(model, x, y, dtype)))
    ops.PROFILE = tags = []
    try:
        _planned_forward(model, x, y, dtype)
    finally:
        ops.PROFILE = None
    names = [t[0] for t in tags]
    code = ops.dtype_code(dtype)
    assert sum(1 for n in names if n.startswith(f"gemm288q_dma_kernel<{code}, 7,") and n.endswith(f" {8 * N}x1152x1152")) == DEPTH - 1, names
    assert sum(1 for n in names if n.startswith(f"gemm288q_dma_kernel<{code}, 6,") and n.endswith(f" {16 * N}x1152x1152")) >= DEPTH, names


@pytest.mark.parametrize("batch", [1, 2])
def test_skip_halves_the_cross_attention_launch(pkg, model, batch):
    """ops.PROFILE tags an attention launch `<kernel> <problems>x<nq>x<nkv>x<dh>`: the cross-attention (nkv = L) covers B x H problems
    with the skip, 2 B x H without; the self-attention (nkv = N) always 2 B x H.  to_q multiplies half the rows."""
    from topia_xl_amd import ops
    x, y = _inputs(batch)
    seen = {}
    for on in (False, True):
        model.null_xattn_skip = on
        ops.PROFILE = tags = []
        try:
            _planned_forward(model, x, y, torch.float16)
        finally:
            ops.PROFILE = None
            model.null_xattn_skip = True
        seen[on] = [t[0] for t in tags]
    def problems(names, nkv):
        return [int(n.split(" ")[-1].split("x")[0]) for n in names if n.startswith("attn_kernel<") and n.endswith(f"x{N}x{nkv}x72")]
    assert problems(seen[False], L) == [2 * batch * HEADS] * DEPTH and problems(seen[True], L) == [batch * HEADS] * DEPTH
    assert problems(seen[False], N) == problems(seen[True], N) == [2 * batch * HEADS] * DEPTH
    to_q = lambda names, rows: sum(1 for n in names if n.endswith(f" {rows}x1152x1152") and ", 7>" in n)   # the heads-fold consumer, K = N = D
    assert to_q(seen[True], batch * N) == DEPTH - 1 and to_q(seen[False], batch * N) == 0
