"""to_q under the null cross-attention skip on 64 x 144 tiles (csrc/gemm.hip gemm144l64_dma_kernel, primx_gemm_toq64_mode).

The skip's to_q launch multiplies the attending entries' rows only (and finishes the other rows' statistics: GemmArgs::fold_mirror);
at batch 1 its 128-row tiles cover half of the CUs.  The 64-row kernel runs the same body on half the rows per workgroup: the same
MFMA chain per output element, so everything it writes must equal the 128-row kernel's BIT FOR BIT.

Operator level: ONE to_q launch through primx_dit_blocks_fold (only_launch = 1, as DiT._forward16's single_launch issues it), mode on
against mode off - Qc and both row ranges of center_out (own, mirrored) equal; pads, the other batch entry, and the words around
center_out and part untouched; the recorded kernel name tells which kernel ran.  Then the rule, and a model-level loop."""
import ctypes as C

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
EPS = 1e-6
SENT = 12345.0


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd
    return topia_xl_amd


@pytest.fixture()
def mode(pkg):
    """Sets the switch for the test and restores what it found."""
    from topia_xl_amd import ops
    first = ops.gemm_toq64_mode(1)
    try:
        yield ops.gemm_toq64_mode
    finally:
        ops.gemm_toq64_mode(first)


def _launched():
    from topia_xl_amd import _lib
    return _lib.load().primx_last_gemm_kernel().decode()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class ToQ:
    """The operands of one skip-form to_q launch: B attending entries of n rows (+ B unconditional ones), width D = K = N."""

    def __init__(self, seed, dtype, B, n, D, H, dh):
        from topia_xl_amd import ops
        from topia_xl_amd._lib import HEADS_ROWS
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.dtype, self.B, self.n, self.D, self.H, self.dh = dtype, B, n, D, H, dh
        Be, T, Tc, nt = 2 * B, 2 * B * n, B * n, D // 144
        self.T, self.Tc = T, Tc
        x = torch.randn(T, D, device=DEV, generator=g) * 2.0 + torch.randn(T, 1, device=DEV, generator=g)
        c = x.mean(-1) + 0.3 * x.std(-1) * torch.sign(torch.randn(T, device=DEV, generator=g))
        rp = (1 + 0.1 * torch.randn(T, device=DEV, generator=g).clamp(-2, 2)) / torch.sqrt(x.var(-1, unbiased=False) + EPS)
        m = (1 + 0.4 * torch.randn(D, device=DEV, generator=g)).to(dtype)
        d = x - c[:, None]
        self.a16 = (d * rp[:, None] * m.float()).to(dtype).contiguous()
        # the producer's partial sums of (x - c), (x - c)^2 per 144 columns, between two guard rows
        part = torch.stack([d.view(T, nt, 144).sum(-1), (d * d).view(T, nt, 144).sum(-1)], -1).float()
        self.pbuf = torch.full((T + 2, nt, 2), SENT, device=DEV)
        self.pbuf[1:T + 1] = part
        self.part = self.pbuf[1:T + 1]
        self.center = torch.stack([c, rp], -1).float().contiguous()
        self.W = (torch.randn(D, D, device=DEV, generator=g) * D ** -0.5).to(dtype)
        self.uv = torch.randn(2, 1, D, device=DEV, generator=g).float().contiguous()          # [u; v] of ONE planned timestep
        self.vrow = torch.zeros(2, D, dtype=dtype, device=DEV)
        self.Qc0 = ops.alloc_heads(Be, H, n, dh, HEADS_ROWS, dtype, DEV, ops.BQ, "q")
        if not bool(torch.isfinite(self.Qc0.float()).all()):                                # (a buffer without pads is not zero-filled)
            self.Qc0.zero_()
        self.valid = torch.zeros_like(self.Qc0, dtype=torch.bool)
        self.valid[:B, :, :n, :dh] = True                                                    # what the launch may write: the attending entries
        self.dummy = torch.zeros(64, dtype=torch.float32, device=DEV)                        # workspaces the to_q launch never touches
        self.copies = (self.a16.clone(), self.pbuf.clone(), self.center.clone(), self.W.clone(), self.uv.clone())

    def launch(self):
        """-> (kernel name, Qc, center_out [T, 2]); checks everything that must stay untouched."""
        from topia_xl_amd import _lib, ops
        T, D = self.T, self.D
        Qc = self.Qc0.clone()
        cbuf = torch.full((T + 2, 2), SENT, device=DEV)
        cout = cbuf[1:T + 1]
        blocks = (_lib.DitBlockFold * 2)()
        blocks[1].w_q, blocks[1].uv_q = self.W.data_ptr(), self.uv.data_ptr()
        dp = self.dummy.data_ptr()
        f = _lib.DitForwardFold(
            dtype=ops.dtype_code(self.dtype), Be=2 * self.B, N=self.n, D=D, H=self.H, dh=self.dh, hidden=4 * D, depth=2, L=64,
            nq_pad=Qc.shape[2], nkv_pad_c=64, nkv_pad_b=64, b_from=self.B, step=0, n_steps=1, ln_eps=EPS, scale=self.dh ** -0.5,
            h=dp, xn=self.a16.data_ptr(), att=dp, hid=dp, Qc=Qc.data_ptr(), Qs=dp, Ks=dp, Vs=dp, mod=dp,
            center0=self.center.data_ptr(), center1=cout.data_ptr(), part=self.part.data_ptr())
        f.null_vrow = self.vrow.data_ptr()
        f.only_block, f.only_launch, f.side = 1, 1, 0
        ops._dev(self.a16, "A")
        _lib.check(_lib.load().primx_dit_blocks_fold(C.byref(f), blocks, ops._stream()), "primx_dit_blocks_fold")
        name = _launched()
        torch.cuda.synchronize()
        for t, c, what in zip((self.a16, self.pbuf, self.center, self.W, self.uv), self.copies, ("A", "part and its guard rows", "center", "W", "u / v")):
            assert torch.equal(_bits(t), _bits(c)), f"{name}: the launch wrote {what}"
        assert bool((cbuf[0] == SENT).all()) and bool((cbuf[T + 1] == SENT).all()), f"{name}: center_out written outside its rows"
        outside = (_bits(Qc) != _bits(self.Qc0)) & ~self.valid
        assert not bool(outside.any()), f"{name}: Qc written outside the attending entries' [tok < n, d < dh] ({int(outside.sum())} elements)"
        assert bool(torch.isfinite(Qc.float()).all()) and bool(torch.isfinite(cout).all())
        assert not bool((cout == SENT).any()), f"{name}: rows of center_out (own or mirrored) not written"
        return name, Qc, cout.clone()


def _code(dtype):
    return 1 if dtype == F16 else 2


# (D = K, heads, head dim): 9 k-tiles (odd: the loop's tail step) x 4 column tiles, tiles that straddle heads of 64; 18 k-tiles x 8
SHAPES = [(576, 8, 72), (576, 9, 64), (1152, 16, 72)]


@pytest.mark.parametrize("dtype", [F16, BF16])
@pytest.mark.parametrize("D,H,dh", SHAPES)
def test_64_row_tile_writes_the_128_row_tile_s_bits(pkg, mode, dtype, D, H, dh):
    """B = 1, n = 256: four 64-row tiles against two 128-row tiles per column tile."""
    case = ToQ(40 + D + dh, dtype, 1, 256, D, H, dh)
    mode(1)
    n64, q64, c64 = case.launch()
    mode(0)
    n128, q128, c128 = case.launch()
    assert n64 == f"gemm144l64_dma_kernel<{_code(dtype)}, 7>", n64
    assert n128 == f"gemm144l_dma_kernel<{_code(dtype)}, 7>", n128
    Tc = case.Tc
    assert torch.equal(_bits(q64), _bits(q128)), f"Q: {int((_bits(q64) != _bits(q128)).sum())} of {q64.numel()} elements differ"
    assert torch.equal(_bits(c64[:Tc]), _bits(c128[:Tc])), "center_out of the tile's own rows differs"
    assert torch.equal(_bits(c64[Tc:]), _bits(c128[Tc:])), "center_out of the mirrored rows differs"
    # ... and the values are the site's statistics, not merely equal: mean and rstd of x = c + (x - c) from the partial sums
    s = case.part.double().sum(1) / D
    mean = case.center[:, 0].double() + s[:, 0]
    rstd = 1.0 / torch.sqrt((s[:, 1] - s[:, 0] ** 2).clamp_min(0) + EPS)
    assert torch.allclose(c64[:, 0].double(), mean, rtol=1e-5, atol=1e-5) and torch.allclose(c64[:, 1].double(), rstd, rtol=1e-4)


def test_rule(pkg, mode):
    """Taken by the headline's launch (M = 2048, N = 1152: 256 workgroups of 64 rows); not at M = 4096 (the 128-row tiles already
    cover every CU), not without the mirrored rows, not with the switch off."""
    from topia_xl_amd import ops
    from topia_xl_amd._lib import HEADS_ROWS
    D, H, dh = 1152, 16, 72
    mode(1)
    head = ToQ(7, F16, 1, 2048, D, H, dh)
    n_on, q_on, c_on = head.launch()
    assert n_on == "gemm144l64_dma_kernel<1, 7>", n_on
    assert ToQ(8, F16, 2, 2048, D, H, dh).launch()[0] == "gemm144l_dma_kernel<1, 7>"
    # mirror == 0: the plain consumer entry point at M = 1500 (its 12 x 8 tiles of 128 rows would pass the rule's count)
    c = ToQ(9, F16, 1, 1500, D, H, dh)
    dst = ops.alloc_heads(1, H, 1500, dh, HEADS_ROWS, F16, DEV, ops.BQ, "q")
    cout = torch.empty(1500, 2, device=DEV)
    ops.linear_heads_fold(c.a16[:1500], c.W, 1500, H, dh, [HEADS_ROWS], [dst], dst.shape[2], c.part[:1500], c.uv[0, 0], c.uv[1, 0],
                          c.center[:1500], cout, EPS)
    assert _launched() == "gemm144l_dma_kernel<1, 7>", _launched()
    mode(0)
    n_off, q_off, c_off = head.launch()
    assert n_off == "gemm144l_dma_kernel<1, 7>", n_off
    assert torch.equal(_bits(q_on), _bits(q_off)) and torch.equal(_bits(c_on), _bits(c_off))   # the headline shape, 256 workgroups
    assert mode(1) == 0 and mode(1) == 1                                                        # the setter returns what it replaces


def _model(pkg, D, heads, depth, N):
    cfg = dict(in_channels=68, condition_channels=768, hidden_size=D, depth=depth)
    m = pkg.DiT(seq_length=N, num_heads=heads, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    m.load_state_dict(synth.dit_state_dict(91, **cfg))
    return m.to(DEV)


def _loop_on_and_off(pkg, mode, m, N, L):
    from tests.test_hip_null_skip import _loop, _same
    x, y = synth.tensor(91, "x", (1, N, 68)).to(DEV), synth.tensor(91, "y", (1, L, 768)).to(DEV)
    mode(1)
    on = _loop(pkg, m, x, y, F16)
    mode(0)
    off = _loop(pkg, m, x, y, F16)
    assert len(on) == 3
    _same(on, off)
    return x, y


def test_small_model_loop_is_bit_identical(pkg, mode):
    """Depth 3, D = 576, N = 256, L = 129: a planned 3-step loop of forward_with_cfg, every step's sample."""
    _loop_on_and_off(pkg, mode, _model(pkg, 576, 8, 3, 256), 256, 129)


def test_folded_loop_runs_the_64_row_tile_and_is_bit_identical(pkg, mode):
    """Full width, depth 2, N = 2048 (the smallest rows at which the planned loop folds, so that to_q IS the fold consumer): the
    loop's samples with the switch on and off, and - by the tags of a profiled forward - the kernel each setting runs."""
    from topia_xl_amd import ops
    from tests.test_hip_null_skip import _planned_forward
    m = _model(pkg, 1152, 16, 2, 2048)
    x, y = _loop_on_and_off(pkg, mode, m, 2048, 129)
    seen = {}
    for on in (1, 0):
        mode(on)
        ops.PROFILE = tags = []
        try:
            _planned_forward(m, x, y, F16)
        finally:
            ops.PROFILE = None
        seen[on] = [t[0] for t in tags if t[0].endswith(" 2048x1152x1152") and ", 7>" in t[0]]
    assert seen[1] == ["gemm144l64_dma_kernel<1, 7> 2048x1152x1152"], seen[1]
    assert seen[0] == ["gemm144l_dma_kernel<1, 7> 2048x1152x1152"], seen[0]
