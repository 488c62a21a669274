"""GPU parity of the VAE decoder kernels and of VAE.decode against the oracle and the REAL
reference's output (tests/golden/vae_decode.npz, fp32)."""
import os

import pytest
import torch
import torch.nn.functional as F

from oracle import synth, vae_ref
from tests.golden.make_golden import SEED, VAE_CFG
from tests.util import max_abs, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# rel-L2 between two routes of one operation that round the same fp32 sums once, in a different summation order (a packed
# kernel and the GEMM form)
ROUTES_TOL = {torch.float16: 2e-4, torch.bfloat16: 2e-3}
# VAE.decode against the fp32 reference: (max-abs relative to the reference's largest magnitude, rel-L2), and rel-L2 against the
# oracle that rounds where the decoder does (test_vae_decode_against_reference states why)
DECODE_TOL = {torch.float16: (6e-3, 5e-3), torch.bfloat16: (4e-2, 3e-2)}
DECODE_EMU_TOL = {torch.float16: 3e-3, torch.bfloat16: 2e-2}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__
    __graft_entry__.build()
    import topia_xl_amd
    return topia_xl_amd


def _cl(x):   # [P, C, S, S, S] -> channels-last [P, V, C]
    P, C = x.shape[:2]
    return x.reshape(P, C, -1).permute(0, 2, 1).contiguous()


def _cf(x, S):  # [P, V, C] -> [P, C, S, S, S]
    P, V, C = x.shape
    return x.permute(0, 2, 1).reshape(P, C, S, S, S)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,S,groups,silu", [(256, 4, 32, True), (32, 8, 32, True), (256, 8, 32, False)])
def test_groupnorm_silu(pkg, dtype, C, S, groups, silu):
    from topia_xl_amd import ops
    x = synth.tensor(31, "gn.x", (5, C, S, S, S), 1.3, 0.2).to(dtype)
    g, b = synth.tensor(31, "gn.g", (C,), 0.2, 1.0), synth.tensor(31, "gn.b", (C,), 0.2)
    ref = F.group_norm(x.float(), groups, g, b, 1e-5)
    ref = F.silu(ref) if silu else ref
    got = ops.groupnorm_silu(_cl(x).to(DEV), g.to(DEV), b.to(DEV), groups, 1e-5, silu)
    assert rel_l2(_cf(got, S), ref) < (1e-3 if dtype == torch.float16 else 6e-3)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Cin,Cout,S,P", [(256, 256, 4, 5), (256, 512, 4, 4), (256, 32, 8, 2), (32, 32, 8, 3), (32, 6, 8, 3)])
def test_conv3d_k3_and_residual(pkg, dtype, Cin, Cout, S, P):
    from topia_xl_amd import ops
    from topia_xl_amd.vae import _conv_weight_as_gemm
    x = synth.tensor(32, "cv.x", (P, Cin, S, S, S)).to(dtype)
    w = synth.tensor(32, "cv.w", (Cout, Cin, 3, 3, 3), (27 * Cin) ** -0.5).to(dtype)
    b = synth.tensor(32, "cv.b", (Cout,), 0.2).to(dtype)
    res = synth.tensor(32, "cv.r", (P, Cout, S, S, S)).to(dtype)
    ref = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    wk = _conv_weight_as_gemm(w, dtype).to(DEV)
    tol = 1.5e-3 if dtype == torch.float16 else 1.2e-2
    got = ops.conv3d_k3(_cl(x).to(DEV), wk, b.to(DEV), S)
    assert rel_l2(_cf(got, S), ref) < tol, rel_l2(_cf(got, S), ref)
    got = ops.conv3d_k3(_cl(x).to(DEV), wk, b.to(DEV), S, res=_cl(res).to(DEV), res_scale=0.5 ** 0.5)
    assert rel_l2(_cf(got, S), (ref + res.double()) * 0.5 ** 0.5) < tol
    wp = ops.pack_conv3(wk, Cin)
    covered = (Cin == 256 and (Cout % 256 == 0 or Cout == 32)) or (Cin == 32 and (Cout == 32 or Cout <= 16))
    assert (wp is not None) == (covered and os.environ.get("PRIMX_CONV_REG", "1") != "0")
    if wp is not None and wp.S == S:
        # the activation-resident kernels (4^3: csrc/conv3.hip, 8^3: csrc/conv3s8.hip, conv3s8c32.hip): same sums in a different order -
        # against fp64, and within accumulation-order noise of the implicit GEMM (both round the fp32 result once)
        got_p = ops.conv3d_k3(_cl(x).to(DEV), wk, b.to(DEV), S, res=_cl(res).to(DEV), res_scale=0.5 ** 0.5, Wp=wp)
        assert rel_l2(_cf(got_p, S), (ref + res.double()) * 0.5 ** 0.5) < tol
        assert rel_l2(got_p, got) < ROUTES_TOL[dtype], rel_l2(got_p, got)
        got_p = ops.conv3d_k3(_cl(x).to(DEV), wk, None, S, Wp=wp)
        assert rel_l2(_cf(got_p, S), ref - b.double().view(1, -1, 1, 1, 1)) < tol


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("Cout,P", [(32, 3), (6, 2), (32, 300)])
def test_conv3d_with_groupnorm_silu_inside(pkg, dtype, Cout, P):
    """csrc/conv3s8c32.hip: GroupNorm(32 groups of one channel) + SiLU applied inside the 8^3 convolution kernel ==
    groupnorm_silu followed by the convolution (the normalised activations are rounded to 16 bits in both), and both
    against fp64.  P = 300 makes the persistent workgroups walk more than one primitive."""
    from topia_xl_amd import ops
    from topia_xl_amd.vae import _conv_weight_as_gemm
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the implicit GEMM: no kernel takes the GroupNorm")
    S, Cin = 8, 32
    x = synth.tensor(35, "cg.x", (P, Cin, S, S, S), 1.4, 0.3).to(dtype)
    w = synth.tensor(35, "cg.w", (Cout, Cin, 3, 3, 3), (27 * Cin) ** -0.5).to(dtype)
    b = synth.tensor(35, "cg.b", (Cout,), 0.2).to(dtype)
    g, be = synth.tensor(35, "cg.g", (Cin,), 0.2, 1.0), synth.tensor(35, "cg.be", (Cin,), 0.2)
    res = synth.tensor(35, "cg.r", (P, Cout, S, S, S)).to(dtype)
    wk = _conv_weight_as_gemm(w, dtype).to(DEV)
    wp = ops.pack_conv3(wk, Cin)
    assert ops.conv3_takes_groupnorm(wp, S, 32) and not ops.conv3_takes_groupnorm(wp, S, 8)
    xd = _cl(x).to(DEV)
    n16 = ops.groupnorm_silu(xd, g.to(DEV), be.to(DEV), 32, 1e-5, True)
    two = ops.conv3d_k3(n16, wk, b.to(DEV), S, res=_cl(res).to(DEV), res_scale=0.5 ** 0.5)          # implicit GEMM on the 16-bit GN output
    got = ops.conv3d_k3(xd, wk, b.to(DEV), S, res=_cl(res).to(DEV), res_scale=0.5 ** 0.5, Wp=wp, gn=(g.to(DEV), be.to(DEV), 1e-5))
    assert rel_l2(got, two) < (3e-4 if dtype == torch.float16 else 3e-3), rel_l2(got, two)
    ref = F.conv3d(F.silu(F.group_norm(x.double(), 32, g.double(), be.double(), 1e-5)), w.double(), b.double(), padding=1)
    ref = (ref + res.double()) * 0.5 ** 0.5
    assert rel_l2(_cf(got, S), ref) < (1.5e-3 if dtype == torch.float16 else 1.2e-2)
    with pytest.raises(ValueError):
        ops.conv3d_k3(xd, wk, b.to(DEV), S, gn=(g.to(DEV), be.to(DEV), 1e-5))                        # gn needs the packed kernel


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("P", [3, 37])
def test_convtranspose_s4_with_group_statistics(pkg, dtype, P):
    """csrc/convt.hip: the activation-resident k2s2 upsample == the GEMM form (same rounding: one per output), against
    fp64, and its per-(primitive, group) statistics == mean / rstd of the 16-bit output it wrote."""
    from topia_xl_amd import ops
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the GEMM form")
    S, C = 4, 256
    x = synth.tensor(36, "ct.x", (P, C, S, S, S)).to(dtype)
    w = synth.tensor(36, "ct.w", (C, C, 2, 2, 2), C ** -0.5).to(dtype)            # ConvTranspose3d weight [Cin, Cout, 2, 2, 2]
    b = synth.tensor(36, "ct.b", (C,), 0.3).to(dtype)
    wt = w.permute(2, 3, 4, 1, 0).reshape(8 * C, C).contiguous().to(DEV)
    wp = ops.pack_convt_s4(wt)
    assert wp is not None
    xd = _cl(x).to(DEV)
    gemm = ops.convtranspose_k2s2(xd, wt, b.to(DEV), S)
    got, part = ops.convtranspose_k2s2(xd, wt, b.to(DEV), S, Wp=wp, want_stats=True)
    st = ops.group_stats(part, b.to(DEV), 1e-5)
    assert rel_l2(got, gemm) < ROUTES_TOL[dtype], rel_l2(got, gemm)
    ref = F.conv_transpose3d(x.double(), w.double(), b.double(), stride=2)
    assert rel_l2(_cf(got, 2 * S), ref) < (1e-3 if dtype == torch.float16 else 8e-3)
    g = got.float().cpu().view(P, 512, 32, 8).permute(0, 2, 1, 3).reshape(P, 32, -1).double()   # [P, group, voxels x 8 channels]
    mean, var = g.mean(-1), g.var(-1, unbiased=False)
    assert float((st[..., 0].cpu().double() - mean).abs().max()) < 2e-5
    assert float((st[..., 1].cpu().double() * (var + 1e-5).sqrt() - 1).abs().max()) < 1e-4
    assert isinstance(ops.convtranspose_k2s2(xd, wt, b.to(DEV), S, Wp=wp), torch.Tensor)              # without statistics: the tensor alone


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_fused_front_of_the_256_to_32_block(pkg, dtype):
    """upsample (with partial statistics) -> ONE kernel for GroupNorm(32) + SiLU + conv1 + 1x1 shortcut == the unfused chain
    groupnorm_silu -> conv3d_k3 and linear_residual on the same upsample output, and both against fp64."""
    from topia_xl_amd import ops
    from topia_xl_amd.vae import _conv_weight_as_gemm
    if os.environ.get("PRIMX_CONV_REG", "1") == "0":
        pytest.skip("PRIMX_CONV_REG=0 keeps the unfused kernels")
    P, C = 5, 256
    x = synth.tensor(37, "ff.x", (P, C, 4, 4, 4)).to(dtype)
    wu = synth.tensor(37, "ff.wu", (C, C, 2, 2, 2), C ** -0.5).to(dtype)
    bu = synth.tensor(37, "ff.bu", (C,), 0.3).to(dtype)
    g, be = synth.tensor(37, "ff.g", (C,), 0.2, 1.0), synth.tensor(37, "ff.be", (C,), 0.2)
    w1 = synth.tensor(37, "ff.w1", (32, C, 3, 3, 3), (27 * C) ** -0.5).to(dtype)
    b1 = synth.tensor(37, "ff.b1", (32,), 0.2).to(dtype)
    wsc = synth.tensor(37, "ff.wsc", (32, C), C ** -0.5).to(dtype)
    bsc = synth.tensor(37, "ff.bsc", (32,), 0.2).to(dtype)
    wt = wu.permute(2, 3, 4, 1, 0).reshape(8 * C, C).contiguous().to(DEV)
    h8, part = ops.convtranspose_k2s2(_cl(x).to(DEV), wt, bu.to(DEV), 4, Wp=ops.pack_convt_s4(wt), want_stats=True)
    wk = _conv_weight_as_gemm(w1, dtype).to(DEV)
    wp = ops.pack_conv3(wk, C, Wsc=wsc.to(DEV))
    assert wp.has_sc
    t_f, sc_f = ops.conv3d_s8_fused(h8, wp, b1.to(DEV), part, bu.to(DEV), g.to(DEV), be.to(DEV), 1e-5, bsc.to(DEV))
    n16 = ops.groupnorm_silu(h8, g.to(DEV), be.to(DEV), 32, 1e-5, True)
    t_u = ops.conv3d_k3(n16, wk, b1.to(DEV), 8, Wp=ops.pack_conv3(wk, C))
    sc_u = ops.linear_residual(h8.view(P * 512, C), wsc.to(DEV), bsc.to(DEV), None, 1.0).view(P, 512, 32)
    tol = 1e-3 if dtype == torch.float16 else 8e-3
    assert rel_l2(sc_f, sc_u) < 1e-6 + (0 if dtype == torch.float16 else 0), rel_l2(sc_f, sc_u)   # same sums, same rounding
    assert rel_l2(t_f, t_u) < tol, rel_l2(t_f, t_u)
    hd = _cf(h8, 8).double().cpu()                                                                  # fp64 from the 16-bit upsample output
    ref = F.conv3d(F.silu(F.group_norm(hd, 32, g.double(), be.double(), 1e-5)), w1.double(), b1.double(), padding=1)
    assert rel_l2(_cf(t_f, 8), ref) < (1.5e-3 if dtype == torch.float16 else 1.2e-2)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_conv_in_convtranspose_and_output(pkg, dtype):
    from topia_xl_amd import ops
    P, S = 4, 4
    z = synth.tensor(33, "z", (P, 1, S, S, S))
    w = synth.tensor(33, "w", (256, 1, 3, 3, 3), 0.2)
    b = synth.tensor(33, "b", (256,), 0.2)
    a_, b_ = 1.7, -0.3
    ref = F.conv3d(a_ * z + b_, w, b, padding=1)          # zero padding AFTER the affine (vae3d_dib.py:438,373)
    got = ops.conv_in(z.reshape(P, -1).to(DEV), a_, b_, w.reshape(256, 27).to(DEV), b.to(DEV), S, dtype)
    assert rel_l2(_cf(got, S), ref) < (1e-3 if dtype == torch.float16 else 6e-3)
    # ConvTranspose3d(k2, s2)
    x = synth.tensor(33, "x", (P, 256, S, S, S)).to(dtype)
    wt = synth.tensor(33, "wt", (256, 256, 2, 2, 2), 256 ** -0.5).to(dtype)
    bt = synth.tensor(33, "bt", (256,), 0.2).to(dtype)
    ref = F.conv_transpose3d(x.double(), wt.double(), bt.double(), stride=2)
    wg = wt.permute(2, 3, 4, 1, 0).reshape(8 * 256, 256).contiguous()
    got = ops.convtranspose_k2s2(_cl(x).to(DEV), wg.to(DEV), bt.to(DEV), S)
    assert rel_l2(_cf(got, 2 * S), ref) < (1.5e-3 if dtype == torch.float16 else 1.2e-2)
    # output layout change + inverse normalisation (inference.py:345-346)
    y = synth.tensor(33, "y", (P, 6, 8, 8, 8)).to(dtype)
    got = ops.vae_output(_cl(y).to(DEV), True).view(P, 6, 8, 8, 8)
    assert torch.equal(got.cpu(), vae_ref.denormalise_decoded(y.float()))
    assert torch.equal(ops.vae_output(_cl(y).to(DEV), False).view(P, 6, 8, 8, 8).cpu(), y.float())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_vae_decode_against_reference(pkg, golden, dtype):
    """Stated tolerance, RELATIVE to the output range (the decoded grids reach |x| ~ 7-8, so an absolute bound says little):
    max-abs error <= 6e-3 (fp16) / 4e-2 (bf16, 8-bit mantissa through ~20 layers) of the reference's largest magnitude, and
    rel-L2 <= 5e-3 / 3e-2, vs the fp32 reference; fp16 is the decoder's default compute type.  (Round 2 asserted an absolute
    2e-2 and measured 1.2e-2 .. 1.95e-2 depending on the primitives drawn: the error follows the 16-bit rounding of the
    (P, 256, 8^3) intermediates, i.e. it scales with the activations.)"""
    g = golden("vae_decode")
    vae = pkg.VAE(**VAE_CFG).eval()
    sd = synth.state_dict_like(SEED, vae.state_dict())
    vae.load_state_dict(sd, strict=True)
    vae.to(DEV)
    vae.compute_dtype = dtype
    z = synth.tensor(SEED, "vae.z", (3, 1, 4, 4, 4))
    out = vae.decode(z.to(DEV))
    assert out.shape == (3, 6, 8, 8, 8) and out.dtype == torch.float32
    ref = torch.as_tensor(g["decoded"])
    rel_max = max_abs(out, ref) / float(ref.abs().max())
    print(f"VAE.decode {dtype}: max-abs {max_abs(out, ref):.3e} on |ref| <= {float(ref.abs().max()):.2f} (relative {rel_max:.2e}), "
          f"rel-L2 {rel_l2(out, ref):.2e}")
    assert rel_max < DECODE_TOL[dtype][0], rel_max
    assert rel_l2(out, ref) < DECODE_TOL[dtype][1], rel_l2(out, ref)
    emu = vae_ref.vae_decode(sd, z, VAE_CFG["up_channels"], VAE_CFG["layers_per_block"], emulate=dtype)
    assert rel_l2(out, emu) < DECODE_EMU_TOL[dtype]
    den = vae.decode(z.to(DEV), denormalize=True)
    assert rel_l2(den, vae_ref.denormalise_decoded(ref)) < (5e-3 if dtype == torch.float16 else 3e-2)


def test_vae_decode_many_primitives_are_independent(pkg):
    """2048-primitive batch (one sample): primitives never interact, so decode(batch)[i] == decode(batch[i:i+1])."""
    vae = pkg.VAE(**VAE_CFG).eval()
    vae.load_state_dict(synth.state_dict_like(SEED, vae.state_dict()))
    vae.to(DEV)
    z = synth.tensor(9, "z", (2048, 1, 4, 4, 4)).to(DEV)
    full = vae.decode(z)
    assert torch.isfinite(full).all()
    for i in (0, 1, 777, 2047):
        assert torch.equal(vae.decode(z[i:i + 1].contiguous()), full[i:i + 1])


def test_latents_to_primitives_pipeline(pkg, golden):
    """inference.py:326-348 as one call: de-normalise + split -> decode ALL primitives -> inverse normalisation -> concat,
    against the oracle restatement of the same lines (per-sample loop, fp32)."""
    import numpy as np
    from topia_xl_amd.pipeline import latents_to_primitives
    vae = pkg.VAE(**VAE_CFG).eval()
    sd = synth.state_dict_like(SEED, vae.state_dict())
    vae.load_state_dict(sd)
    vae.to(DEV)
    B, N = 2, 5
    samples = synth.tensor(41, "samples", (B, N, 68))
    mean = synth.tensor(41, "mean", (68,), 0.5)
    std = synth.tensor(41, "std", (68,), 0.2, 1.0).abs()
    got = latents_to_primitives(samples.to(DEV), vae, mean.tolist(), std.tolist(), 1.0)
    assert got.shape == (B, N, 4 + 6 * 512)
    # oracle: the reference's driver lines, sample by sample
    rp = samples / 1.0 * std[None, None] + mean[None, None]
    assert torch.equal(got[..., :4].cpu(), rp[..., :4])                 # srt: pure fp32 elementwise -> bit-exact
    ref = []
    for b in range(B):
        dec = vae_ref.vae_decode(sd, rp[b, :, 4:].reshape(N, 1, 4, 4, 4), VAE_CFG["up_channels"], VAE_CFG["layers_per_block"])
        ref.append(vae_ref.denormalise_decoded(dec).reshape(N, -1))
    ref = torch.stack(ref)
    assert max_abs(got[..., 4:], ref) < 2e-2 and rel_l2(got[..., 4:], ref) < 5e-3
