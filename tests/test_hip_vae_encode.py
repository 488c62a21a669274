"""GPU tests of the VAE encoder: the three kernels of csrc/vaeenc.hip and primx_latent_norm against float64 / torch, and
VAE.encode / VAE.forward / pipeline.primitives_to_latents against the reference's recorded output
(tests/golden/vae_encode.npz) and the restatement tests/vae_encode_ref.py.

Every comparison prints its measured figure; those of an MI355X run are in the docstring of test_vae_encode_against_reference
and in DESIGN.md "VAE encode".
"""
import gc
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth
from tests import extent as ex
from tests import footprint as fp
from tests import vae_encode_ref as er
from tests.golden import make_golden_vae_encode as mg
from tests.golden.make_golden import SEED, VAE_CFG
from tests.test_hip_vae import DECODE_EMU_TOL
from tests.util import max_abs, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, BF16 = torch.float16, torch.bfloat16
BOTH = [F16, BF16]
CONV_TOL = {F16: 1.5e-3, BF16: 1.2e-2}     # the project's bound for a 16-bit convolution against float64 (tests/test_hip_vae.py)
INPUTS = {"a": mg.input_a, "b": mg.input_b}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import ops
    return ops


@pytest.fixture(scope="module")
def vae(ops):
    import topia_xl_amd as pkg
    m = pkg.VAE(**VAE_CFG).eval()
    sd = synth.state_dict_like(SEED, m.state_dict())
    m.load_state_dict(sd, strict=True)
    m.to(DEV)
    return m, sd


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _gemm_form(w, dtype):
    from topia_xl_amd.vae import _conv_weight_as_gemm
    return _conv_weight_as_gemm(w, dtype)


def _cf(x, S):  # [P, V, C] -> [P, C, S, S, S]
    P, V, C = x.shape
    return x.permute(0, 2, 1).reshape(P, C, S, S, S)


def _cl(x):     # [P, C, S, S, S] -> [P, V, C]
    P, C = x.shape[:2]
    return x.reshape(P, C, -1).permute(0, 2, 1).contiguous()


def _I(g, t, name):
    return g.guard_input(t, name).t


# ------------------------------------------------------------------------------------------------ conv_in
def _conv_in_operands(P, dtype, seed=51):
    x = synth.tensor(seed, "ci.x", (P, 6, 8, 8, 8), 0.6, 0.3)
    w = synth.tensor(seed, "ci.w", (32, 6, 3, 3, 3), 162 ** -0.5).to(dtype)
    b = synth.tensor(seed, "ci.b", (32,), 0.2).to(dtype)
    return x, w, b


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("P", [1, 3, 300])
def test_enc_conv_in(ops, dtype, normalize, P):
    """Against float64 F.conv3d of the rounded operands (the rounded, normalised input included)."""
    x, w, b = _conv_in_operands(P, dtype)
    xn = er.normalise_payload(x) if normalize else x
    ref = F.conv3d(xn.to(dtype).double(), w.double(), b.double(), padding=1)
    got = ops.enc_conv_in(x.to(DEV), _gemm_form(w, dtype).to(DEV), b.to(DEV), normalize)
    assert got.shape == (P, 512, 32) and got.dtype == dtype
    d = rel_l2(_cf(got, 8), ref)
    print(f"enc_conv_in {dtype} P={P} normalize={normalize}: rel-L2 vs float64 {d:.2e} (bound {CONV_TOL[dtype]:g})")
    assert d < CONV_TOL[dtype], d


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("normalize", [False, True])
def test_enc_conv_in_rounds_the_normalised_input_as_torch_does(ops, dtype, normalize):
    """With a weight that copies input channel c to output channel c (1 at the centre tap) and no bias, the output IS the
    kernel's rounded input: bit-equal to (x * 5 | x * 2 - 1).to(dtype); the other 26 output channels are exactly 0."""
    x = synth.tensor(52, "ci.x", (3, 6, 8, 8, 8), 0.7, 0.2)
    w = torch.zeros(32, 6, 3, 3, 3)
    for c in range(6):
        w[c, c, 1, 1, 1] = 1.0
    got = ops.enc_conv_in(x.to(DEV), _gemm_form(w.to(dtype), dtype).to(DEV), torch.zeros(32, dtype=dtype, device=DEV), normalize)
    want = (er.normalise_payload(x) if normalize else x).to(dtype)
    assert fp.same_bits(_cf(got, 8)[:, :6].cpu(), want)
    assert int(got[:, :, 6:].ne(0).sum()) == 0


# ------------------------------------------------------------------------------------------------ downsample
def _down_operands(P, dtype, seed=53):
    x = synth.tensor(seed, "dn.x", (P, 32, 8, 8, 8)).to(dtype)
    w = synth.tensor(seed, "dn.w", (32, 32, 3, 3, 3), 864 ** -0.5).to(dtype)
    b = synth.tensor(seed, "dn.b", (32,), 0.2).to(dtype)
    return x, w, b


def _needs_packed_kernels():
    """The only skip of this file, decided by the switch and before any work: with PRIMX_CONV_REG=0 no packed weight image is
    made and the stride-2 kernel, which has no other form, cannot run (VAE.encode raises)."""
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0: the packed weight images are switched off")


def _pack_down(ops, w, dtype):
    wp = ops.pack_conv3(_gemm_form(w, dtype).to(DEV), 32)
    assert wp is not None and wp.kind == "s8c32"
    return wp


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("P", [1, 3, 300])
def test_conv3d_down(ops, dtype, P):
    _needs_packed_kernels()
    x, w, b = _down_operands(P, dtype)
    ref = F.conv3d(x.double(), w.double(), b.double(), stride=2, padding=1)
    got = ops.conv3d_down(_cl(x).to(DEV), _pack_down(ops, w, dtype), b.to(DEV))
    assert got.shape == (P, 64, 32) and got.dtype == dtype
    d = rel_l2(_cf(got, 4), ref)
    print(f"conv3d_down {dtype} P={P}: rel-L2 vs float64 {d:.2e} (bound {CONV_TOL[dtype]:g})")
    assert d < CONV_TOL[dtype], d


@pytest.mark.parametrize("dtype", BOTH)
def test_conv3d_down_impulses(ops, dtype):
    """One-hot inputs at the 8 corner voxels, (3,3,3) and (4,4,4), each in one channel; integer weights and bias.  Every
    output is one product plus the bias: bit-equal to F.conv3d.  Catches the one-sided padding (output o reads 2 o - 1 ..
    2 o + 1) and any tap-order error.

    The weights: n = tap * 32 + cout (864 values) + 864 for odd classes of cin, negated for classes 2 and 3, class =
    (cin + cin // 4) % 4 (so cin + 1, + 4 and + 8 all change the class; the ten impulse channels meet all four).  fp16: the
    integer n + 1 itself (|w| <= 1728, every w + bias exact in fp16).  bf16 holds no 1728 distinct small integers, so there
    w is the n-th bf16 value from 128.0 upwards (integers, spaced 1, 2, 4 ...).  All 27 * 32 * 32 weights cannot be
    distinct in 16 bits; within one cin (all that one impulse meets) and across the four classes they are."""
    _needs_packed_kernels()
    vox = [(z, y, x) for z in (0, 7) for y in (0, 7) for x in (0, 7)] + [(3, 3, 3), (4, 4, 4)]
    tap = torch.arange(27).view(1, 1, 27)
    ci = torch.arange(32).view(1, 32, 1)
    co = torch.arange(32).view(32, 1, 1)
    cls = (ci + ci // 4) % 4
    n = tap * 32 + co + 864 * (cls % 2)                                              # [0, 1728)
    if dtype == F16:
        mag = (n + 1).float()
    else:
        mag = (n + int(torch.tensor(128.0, dtype=BF16).view(torch.int16))).to(torch.int16).view(BF16).float()
    w = (mag * (1 - 2 * (cls // 2))).view(32, 32, 3, 3, 3).contiguous()
    b = (torch.arange(32) % 17 - 8).float()
    assert torch.equal(w.to(dtype).float(), w) and torch.equal(w, w.round())
    assert w.permute(1, 0, 2, 3, 4).reshape(8, 4, -1)[0].unique().numel() == 4 * 864     # cin 0..3: four classes, all distinct
    x = torch.zeros(len(vox), 32, 8, 8, 8)
    for i, (z, y, xx) in enumerate(vox):
        x[i, (5 * i + 2) % 32, z, y, xx] = 1.0
    want = F.conv3d(x, w, b, stride=2, padding=1).to(dtype)
    got = ops.conv3d_down(_cl(x.to(dtype)).to(DEV), _pack_down(ops, w.to(dtype), dtype), b.to(dtype).to(DEV))
    assert fp.same_bits(_cf(got, 4).cpu().contiguous(), want)


# ------------------------------------------------------------------------------------------------ head
def _head_operands(P, dtype, seed=54):
    h = synth.tensor(seed, "hd.h", (P, 256, 4, 4, 4), 0.8, 0.1).to(dtype)
    w = synth.tensor(seed, "hd.w", (2, 256, 3, 3, 3), 6912 ** -0.5).to(dtype)
    b = synth.tensor(seed, "hd.b", (2,), 0.2).to(dtype).float()
    qw = synth.tensor(seed, "hd.qw", (2, 2), 0.7)
    qb = synth.tensor(seed, "hd.qb", (2,), 0.2)
    return h, w, b, qw, qb


def _ulp32(x):
    """One fp32 unit in the last place at |x| (float64 tensor)."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x), e - 24)


def _head_check(got, h, w, b, qw, qb, what):
    """|got - ref64| <= (6912 + 8) * 2^-24 * S_abs + one fp32 ulp of |ref64|, elementwise; S_abs = the same expression on
    absolute values: the worst case of an fp32 sum of K products in any order."""
    def expr(h_, w_, b_, qw_, qb_):
        y = F.conv3d(h_, w_, b_, padding=1)
        return F.conv3d(y, qw_.view(2, 2, 1, 1, 1), qb_)
    d = lambda t: t.double()
    ref = expr(d(h), d(w), d(b), d(qw), d(qb))
    s_abs = expr(d(h).abs(), d(w).abs(), d(b).abs(), d(qw).abs(), d(qb).abs())
    bound = (6912 + 8) * 2.0 ** -24 * s_abs + _ulp32(ref)
    err = (got.double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print(f"enc_head {what}: largest error / bound {worst:.2e}, max-abs error {float(err.max()):.2e}")
    assert bool((err <= bound).all()), worst
    return ref


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("P", [1, 5, 300])
def test_enc_head(ops, dtype, P):
    h, w, b, qw, qb = _head_operands(P, dtype)
    got = ops.enc_head(_cl(h).to(DEV), _gemm_form(w, dtype).to(DEV), b.to(DEV), qw.to(DEV), qb.to(DEV))
    assert got.shape == (P, 2, 4, 4, 4) and got.dtype == torch.float32
    _head_check(got, h, w, b, qw, qb, f"{dtype} P={P}")


@pytest.mark.parametrize("dtype", BOTH)
def test_enc_head_beyond_the_logvar_clamp(ops, dtype):
    """conv_out / quant_conv biases that push the log-variance past +20 and below -30: `parameters` come out unclamped (and
    within the head's bound), the posterior's logvar is clamped."""
    from topia_xl_amd.vae import DiagonalGaussianDistribution
    h, w, b, qw, qb = _head_operands(5, dtype)
    qw = torch.tensor([[0.9, 0.1], [0.2, 1.1]])
    for sign, end in ((1.0, 20.0), (-1.0, -30.0)):
        b2 = torch.tensor([0.1, sign * 40.0]).to(dtype).float()
        qb2 = torch.tensor([-0.2, sign * 15.0])
        got = ops.enc_head(_cl(h).to(DEV), _gemm_form(w, dtype).to(DEV), b2.to(DEV), qw.to(DEV), qb2.to(DEV))
        ref = _head_check(got, h, w, b2, qw, qb2, f"{dtype} logvar {'+' if sign > 0 else '-'}")
        assert bool((ref[:, 1] * sign > 50).all()) and bool((got[:, 1] * sign > 50).all())
        post = DiagonalGaussianDistribution(got)
        assert post.parameters is got and bool((post.logvar == end).all())
        assert torch.equal(post.mean, got[:, :1]) and bool(torch.isfinite(post.std).all())


# ------------------------------------------------------------------------------------------------ latent_norm
@pytest.mark.parametrize("rows", [1, 5, 2048])
def test_latent_norm(ops, rows):
    """Bit-equal to the fp32 torch expression (nf = 1.3).  With nf = 1 (the shipped value: the scalings by nf are exact)
    latent_denorm(latent_norm(v)) reproduces v to within 2 ulp: two fp32 roundings each way - the subtraction and the
    division, then the multiplication by the same std and the addition - of half an ulp each, where the ulp is that of the
    larger of |v| and |v - mean|, the magnitudes at which those four roundings happen (in ulps of v alone the bound cannot
    hold: v - mean carries an error of the size of an ulp of mean back into a v that may be far smaller).  With nf = 1.3 the
    two scalings round as well: six roundings of relative error <= 2^-24 each, five of them on values of the size of
    |v - mean| and the last on v, so |back - v| <= (5 |v - mean| + |v|) * 2^-24 to first order, asserted elementwise."""
    v = synth.tensor(55, "ln.v", (rows, 68), 1.5, 0.2)
    mean = synth.tensor(55, "ln.mean", (68,), 0.5)
    std = synth.tensor(55, "ln.std", (68,), 0.2, 1.0).abs()
    md, sd_ = mean.to(DEV), std.to(DEV)
    s0, z0 = v[:, :4].contiguous().to(DEV), v[:, 4:].contiguous().to(DEV)
    got = ops.latent_norm(s0, z0, md, sd_, 1.3)
    assert got.shape == (rows, 68) and fp.same_bits(got.cpu(), (v - mean[None]) / std[None] * 1.3)
    one = ops.latent_norm(s0, z0, md, sd_, 1.0)
    assert fp.same_bits(one.cpu(), (v - mean[None]) / std[None])
    srt, z = ops.latent_denorm(one, md, sd_, 1.0, 4)
    back = torch.cat([srt, z], dim=1).cpu()
    scale = torch.maximum(v.abs(), (v - mean[None]).abs()).double()
    ulps = ((back.double() - v.double()).abs() / _ulp32(scale)).max()
    print(f"latent_norm rows={rows}: round trip through latent_denorm within {float(ulps):.2f} ulp (bound 2)")
    assert float(ulps) <= 2.0
    srt, z = ops.latent_denorm(got, md, sd_, 1.3, 4)
    err = (torch.cat([srt, z], dim=1).cpu().double() - v.double()).abs()
    bound = (5 * (v.double() - mean.double()[None]).abs() + v.double().abs()) * 2.0 ** -24 * (1 + 2.0 ** -20)
    print(f"latent_norm rows={rows}: nf = 1.3 round trip: largest error / bound {float((err / bound).max()):.2f}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ VAE.encode
_FLOORS = {}


def _floor(sd, which, dtype):
    """(rel-L2, max-abs / max|ref|) of the 16-bit restatement against the golden, and the restatement itself: computed once."""
    key = (which, dtype)
    if key not in _FLOORS:
        ref = torch.from_numpy(np.load(os.path.join(mg.HERE, "vae_encode.npz"), allow_pickle=False)["parameters_" + which])
        emu = er.vae_encode(sd, INPUTS[which](), dtype)
        _FLOORS[key] = (rel_l2(emu, ref), max_abs(emu, ref) / float(ref.abs().max()), emu, ref)
    return _FLOORS[key]


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("which", ["a", "b"])
def test_vae_encode_against_reference(vae, dtype, which):
    """VAE.encode(x).parameters against the reference's recorded fp32 output: rel-L2 and max-abs / max|ref| within 2 x the
    floor of the 16-bit restatement on the same input (the floor is what rounding at the ~20 stored stages costs with the
    reference's own summation order; the kernels' order flips roundings at each of those stages, an error of the floor's
    own size - hence 2).  Against the restatement: DECODE_EMU_TOL, the decoder's bound at the same depth.

    Measured on an MI355X (rel-L2 vs reference (floor); max-abs / max|ref| (floor); rel-L2 vs restatement), also in DESIGN.md
    "VAE encode":
        fp16 A  1.40e-3 (1.47e-3)   1.15e-3 (1.44e-3)   1.43e-3
        fp16 B  1.62e-3 (1.77e-3)   1.71e-3 (1.77e-3)   1.63e-3
        bf16 A  1.18e-2 (1.22e-2)   1.08e-2 (1.09e-2)   1.12e-2
        bf16 B  1.38e-2 (1.35e-2)   1.20e-2 (1.48e-2)   1.08e-2"""
    m, sd = vae
    f_l2, f_mx, emu, ref = _floor(sd, which, dtype)
    m.compute_dtype = dtype
    try:
        post = m.encode(INPUTS[which]().to(DEV))
    finally:
        m.compute_dtype = F16
    got = post.parameters.cpu()
    assert got.shape == (3, 2, 4, 4, 4) and got.dtype == torch.float32
    l2, mx, e2 = rel_l2(got, ref), max_abs(got, ref) / float(ref.abs().max()), rel_l2(got, emu)
    print(f"VAE.encode {dtype} input {which.upper()}: rel-L2 vs reference {l2:.2e} (floor {f_l2:.2e}), max-abs / max|ref| {mx:.2e} "
          f"(floor {f_mx:.2e}), rel-L2 vs restatement {e2:.2e} (bound {DECODE_EMU_TOL[dtype]:g})")
    assert l2 <= 2 * f_l2, (l2, f_l2)
    assert mx <= 2 * f_mx, (mx, f_mx)
    assert e2 < DECODE_EMU_TOL[dtype], e2
    assert torch.equal(post.mode().cpu(), got[:, :1]) and torch.equal(post.logvar.cpu(), got[:, 1:].clamp(-30.0, 20.0))


def test_vae_encode_normalize_and_refusals(vae):
    """normalize=True == encode of the host-normalised payload, bit for bit (x * 5 and x * 2 - 1 are the same fp32 operations);
    configurations the kernels do not cover are refused by name."""
    import topia_xl_amd as pkg
    m, _ = vae
    x = (mg.input_b() / 5.0).to(DEV)
    assert torch.equal(m.encode(x, normalize=True).parameters, m.encode(er.normalise_payload(x)).parameters)
    with pytest.raises(NotImplementedError, match="shipped"):
        m.encode(torch.zeros(2, 6, 4, 4, 4, device=DEV))
    other = pkg.VAE(**dict(VAE_CFG, down_channels=[32, 64, 256])).to(DEV)
    with pytest.raises(NotImplementedError, match="shipped"):
        other.encode(torch.zeros(2, 6, 8, 8, 8, device=DEV))


def test_vae_encode_many_primitives_are_independent(vae):
    """P = 2048: primitives never interact, so encode(x)[i] is bit-equal to encode(x[i:i+1])."""
    m, _ = vae
    x = synth.tensor(9, "enc.many", (2048, 6, 8, 8, 8), 0.8).to(DEV)
    full = m.encode(x).parameters
    assert bool(torch.isfinite(full).all())
    for i in (0, 1, 777, 2047):
        assert torch.equal(m.encode(x[i:i + 1].contiguous()).parameters, full[i:i + 1]), i


def test_vae_encode_one_full_chunk(vae):
    """P = 8 * 2048, the default max_prims_per_call of primitives_to_latents, in fp16 and bf16: the [P * 64, 32] operand of
    the 32 -> 256 shortcut (K = 32 < the GEMM's k-tile of 64) is then 64 MB and ends where its allocation ends, so a K-tail
    load issued past the row would leave the allocation (csrc/gemm.hip, load_tile).  Bit-equal to encodes of 2048."""
    m, _ = vae
    P = 8 * 2048
    x = synth.tensor(9, "enc.chunk", (P, 6, 8, 8, 8), 0.8).to(DEV)
    for dtype in BOTH:
        m.compute_dtype = dtype
        try:
            full = m.encode(x, normalize=True).parameters
            parts = torch.cat([m.encode(x[lo:lo + 2048], normalize=True).parameters for lo in range(0, P, 2048)], dim=0)
        finally:
            m.compute_dtype = F16
        assert full.shape == (P, 2, 4, 4, 4) and bool(torch.isfinite(full).all())
        assert torch.equal(full, parts), dtype


def test_vae_forward(vae):
    m, _ = vae
    x = mg.input_a().to(DEV)
    rec, post = m(x, sample=False)
    assert torch.equal(rec, m.decode(m.encode(x).mode())) and rec.shape == x.shape
    g = torch.Generator(device=DEV).manual_seed(11)
    rec_s, post_s = m(x, sample=True, generator=g)
    noise = torch.randn(post_s.mean.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    assert torch.equal(post_s.parameters, post.parameters)
    assert torch.equal(rec_s, m.decode(post_s.mean + post_s.std * noise))
    assert not torch.equal(rec_s, rec)


def test_primitives_to_latents(vae):
    """B = 2, N = 5 against the restatement composed on the CPU: srt columns bit-exact (fp32 elementwise), z columns within
    the fp16 bounds of test_vae_encode_against_reference (2 x the restatement's floor against the fp32 restatement,
    DECODE_EMU_TOL against the rounding one); max_prims_per_call=4 (three encodes) is bit-equal to one call."""
    from topia_xl_amd.pipeline import latents_to_primitives, primitives_to_latents
    m, sd = vae
    B, N = 2, 5
    mean = synth.tensor(41, "mean", (68,), 0.5)
    std = synth.tensor(41, "std", (68,), 0.2, 1.0).abs()
    nf = 1.1
    srt = synth.tensor(42, "p2l.srt", (B, N, 4), 0.4)
    payload = torch.from_numpy(np.load(os.path.join(mg.HERE, "vae_decode.npz"), allow_pickle=False)["decoded"]).float()
    payload = torch.cat([payload, synth.tensor(42, "p2l.x", (B * N - payload.shape[0], 6, 8, 8, 8), 0.8)], dim=0)
    den = torch.cat([payload[:, :1] / 5.0, (payload[:, 1:] + 1.0) / 2.0], dim=1)             # what latents_to_primitives emits
    rp = torch.cat([srt, den.reshape(B, N, -1)], dim=-1)
    got = primitives_to_latents(rp.to(DEV), m, mean.tolist(), std.tolist(), nf)
    assert got.shape == (B, N, 68) and got.dtype == torch.float32
    assert torch.equal(primitives_to_latents(rp.to(DEV), m, mean.tolist(), std.tolist(), nf, max_prims_per_call=4), got)

    def compose(emulate):
        z = er.vae_encode(sd, den, emulate, normalize=True)[:, :1].reshape(B, N, 64)
        return (torch.cat([srt, z], dim=-1) - mean) / std * nf
    ref, emu = compose(None), compose(F16)
    assert fp.same_bits(got[..., :4].cpu(), ref[..., :4].contiguous())
    gz, rz, ez = got[..., 4:].cpu(), ref[..., 4:], emu[..., 4:]
    f_l2, f_mx = rel_l2(ez, rz), max_abs(ez, rz) / float(rz.abs().max())
    l2, mx, e2 = rel_l2(gz, rz), max_abs(gz, rz) / float(rz.abs().max()), rel_l2(gz, ez)
    print(f"primitives_to_latents z columns: rel-L2 {l2:.2e} (floor {f_l2:.2e}), max-abs / max|ref| {mx:.2e} (floor {f_mx:.2e}), "
          f"vs restatement {e2:.2e}")
    assert l2 <= 2 * f_l2 and mx <= 2 * f_mx and e2 < DECODE_EMU_TOL[F16]
    # and it inverts latents_to_primitives on the srt columns to within the round trip of test_latent_norm
    tokens = synth.tensor(43, "p2l.tok", (B, N, 68)).to(DEV)
    back = primitives_to_latents(latents_to_primitives(tokens, m, mean.tolist(), std.tolist(), nf), m, mean.tolist(), std.tolist(), nf)
    assert float((back[..., :4] - tokens[..., :4]).abs().max()) < 1e-5
    # a sample instead of the mode: mean + std * randn of the generator passed, normalised
    g = torch.Generator(device=DEV).manual_seed(3)
    smp = primitives_to_latents(rp.to(DEV), m, mean.tolist(), std.tolist(), nf, sample=True, generator=g)
    assert torch.equal(smp[..., :4], got[..., :4]) and not torch.equal(smp[..., 4:], got[..., 4:])
    # the noise is drawn once for all B * N primitives: the same generator state gives the same sample under any chunking,
    # and that sample is mean + std * randn of one draw
    smp4 = primitives_to_latents(rp.to(DEV), m, mean.tolist(), std.tolist(), nf, sample=True,
                                 generator=torch.Generator(device=DEV).manual_seed(3), max_prims_per_call=4)
    assert torch.equal(smp4, smp)
    post = m.encode(den.to(DEV), normalize=True)
    noise = torch.randn(post.mean.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    zs = (post.mean + post.std * noise).reshape(B * N, 64)
    from topia_xl_amd import ops
    want = ops.latent_norm(rp.to(DEV).reshape(B * N, -1)[:, :4].contiguous(), zs.contiguous(), mean.to(DEV), std.to(DEV), nf)
    assert torch.equal(smp, want.view(B, N, 68))


# ------------------------------------------------------------------------------------------------ footprint
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("P", [1, 3, 300])
def test_encoder_kernels_footprint(ops, dtype, P):
    """enc_conv_in (both normalisations), conv3d_down with its image, enc_head and latent_norm between guards, under both
    fills (tests/footprint.py)."""
    _needs_packed_kernels()
    x0, w0, b0 = _conv_in_operands(P, dtype)
    x0, wk0, b0 = x0.to(DEV), _gemm_form(w0, dtype).to(DEV), b0.to(DEV)
    fp.hold(lambda g: {n: ops.enc_conv_in(_I(g, x0, "x"), _I(g, wk0, "Wk"), _I(g, b0, "bias"), n) for n in (False, True)})
    xd, wd, bd = _down_operands(P, dtype)
    xd, wkd, bd = _cl(xd).to(DEV), _gemm_form(wd, dtype).to(DEV), bd.to(DEV)

    def down(g):
        wp = ops.pack_conv3(_I(g, wkd, "Wk"), 32)
        assert wp is not None
        return {"image": wp.Wp, "out": ops.conv3d_down(_I(g, xd, "x"), wp, _I(g, bd, "bias"))}
    fp.hold(down)
    h, w, b, qw, qb = _head_operands(P, dtype)
    h, wk, b, qw, qb = _cl(h).to(DEV), _gemm_form(w, dtype).to(DEV), b.to(DEV), qw.to(DEV), qb.to(DEV)
    fp.hold(lambda g: ops.enc_head(_I(g, h, "h"), _I(g, wk, "Wk"), _I(g, b, "bias"), _I(g, qw, "qw"), _I(g, qb, "qb")))
    v = synth.tensor(55, "ln.v", (P, 68), 1.5, 0.2).to(DEV)
    mean, std = synth.tensor(55, "ln.mean", (68,), 0.5).to(DEV), synth.tensor(55, "ln.std", (68,), 0.2, 1.0).abs().to(DEV)
    s0, z0 = v[:, :4].contiguous(), v[:, 4:].contiguous()
    fp.hold(lambda g: ops.latent_norm(_I(g, s0, "srt"), _I(g, z0, "z"), _I(g, mean, "mean"), _I(g, std, "std"), 1.3))


@pytest.mark.parametrize("P", [1, 3, 300])
def test_vae_encode_footprint(vae, P):
    """VAE.encode, whole, under the guard: packed weights, attention operands and every intermediate are (re)allocated in each run."""
    m, _ = vae
    x0 = synth.tensor(9, "enc.fp", (P, 6, 8, 8, 8), 0.8).to(DEV)

    def case(g):
        m.repack()
        m.__dict__.pop("_attn_ws", None)
        x = _I(g, x0, "x")
        return {"plain": m.encode(x).parameters, "normalized": m.encode(x, normalize=True).parameters}
    plain = fp.hold(case)
    assert plain["plain"].shape == (P, 2, 4, 4, 4) and bool(torch.isfinite(plain["plain"]).all())


# ------------------------------------------------------------------------------------------------ extent
P_BIG = ex.primitives_past(16384)      # 131081: the [P, 512, 32] and [P, 64, 256] operands pass 2^31 elements


def _hold_extent(run, P, what):
    with fp.guarded(0xFF):
        big = run(0, P)
    ex.assert_chunks_equal(big, run, P, what=what)
    print(f"extent: {what}: P = {P}: bit identity with the calls on 2048 primitives")
    return big


def test_enc_conv_in_extent(ops):
    dtype, e = F16, 512 * 32
    ex.reaches(P_BIG * e, 2, "enc_conv_in output")
    x = ex.randn_slabs((P_BIG, 6, 8, 8, 8), torch.float32, DEV, 61, 0.6, 0.3)
    _, w, b = _conv_in_operands(1, dtype)
    wk, bd = _gemm_form(w, dtype).to(DEV), b.to(DEV)
    big = _hold_extent(lambda lo, hi: ops.enc_conv_in(x[lo:hi], wk, bd, True), P_BIG, "enc_conv_in")
    i = ex.probe_primitives(P_BIG, e, 2)
    xi = x[torch.tensor(i, device=DEV)].cpu()
    ref = F.conv3d(er.normalise_payload(xi).to(dtype).double(), w.double(), b.double(), padding=1)
    d = rel_l2(_cf(big[torch.tensor(i, device=DEV)], 8), ref)
    print(f"extent: enc_conv_in probes {i}: rel-L2 vs float64 {d:.2e}")
    assert d < CONV_TOL[dtype]


def test_conv3d_down_extent(ops):
    _needs_packed_kernels()
    dtype, e = F16, 512 * 32
    ex.reaches(P_BIG * e, 2, "conv3d_down input")
    x = ex.randn_slabs((P_BIG, 512, 32), dtype, DEV, 62)
    _, w, b = _down_operands(1, dtype)
    wp, bd = _pack_down(ops, w, dtype), b.to(DEV)
    big = _hold_extent(lambda lo, hi: ops.conv3d_down(x[lo:hi], wp, bd), P_BIG, "conv3d_down")
    i = ex.probe_primitives(P_BIG, e, 2)
    xi = _cf(x[torch.tensor(i, device=DEV)], 8).cpu()
    ref = F.conv3d(xi.double(), w.double(), b.double(), stride=2, padding=1)
    d = rel_l2(_cf(big[torch.tensor(i, device=DEV)], 4), ref)
    print(f"extent: conv3d_down probes {i}: rel-L2 vs float64 {d:.2e}")
    assert d < CONV_TOL[dtype]


def test_enc_head_extent(ops):
    dtype, e = F16, 64 * 256
    ex.reaches(P_BIG * e, 2, "enc_head input")
    x = ex.randn_slabs((P_BIG, 64, 256), dtype, DEV, 63, 0.8, 0.1)
    _, w, b, qw, qb = _head_operands(1, dtype)
    wk = _gemm_form(w, dtype).to(DEV)
    bd, qwd, qbd = b.to(DEV), qw.to(DEV), qb.to(DEV)
    big = _hold_extent(lambda lo, hi: ops.enc_head(x[lo:hi], wk, bd, qwd, qbd), P_BIG, "enc_head")
    i = ex.probe_primitives(P_BIG, e, 2)
    hi_ = _cf(x[torch.tensor(i, device=DEV)], 4).cpu()
    _head_check(big[torch.tensor(i, device=DEV)], hi_, w, b, qw, qb, f"extent probes {i}")


def test_vae_encode_extent(vae):
    """VAE.encode once on 131081 primitives against encodes of at most 2048."""
    m, _ = vae
    ex.reaches(P_BIG * 512 * 32, 2, "the [P, 512, 32] activation")
    x = ex.randn_slabs((P_BIG, 6, 8, 8, 8), torch.float32, DEV, 64, 0.8)
    big = _hold_extent(lambda lo, hi: m.encode(x[lo:hi]).parameters, P_BIG, "VAE.encode")
    assert big.shape == (P_BIG, 2, 4, 4, 4) and bool(torch.isfinite(big).all())
