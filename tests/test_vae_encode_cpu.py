"""CPU checks of the VAE encoder's test infrastructure and host code (no GPU): the restatement tests/vae_encode_ref.py
against the recorded reference (tests/golden/vae_encode.npz, made by tests/golden/make_golden_vae_encode.py), the port of
DiagonalGaussianDistribution against the recorded reference class, and the host semantics of the new entry points."""
import numpy as np
import pytest
import torch

from oracle import synth
from tests import vae_encode_ref as er
from tests.golden import make_golden_vae_encode as mg
from tests.golden.make_golden import SEED, VAE_CFG
from tests.util import max_abs, rel_l2

INPUTS = {"a": mg.input_a, "b": mg.input_b}


@pytest.fixture(scope="module")
def sd(pkg):
    vae = pkg.VAE(**VAE_CFG)
    return synth.state_dict_like(SEED, vae.state_dict())


@pytest.mark.parametrize("which", ["a", "b"])
def test_restatement_equals_the_reference(sd, golden, which):
    """The fp32 restatement against the reference module's recorded output.  Measured: max-abs difference 0.0 on both
    inputs.  The bound 5e-5 * max|ref| covers the fp32-vs-fp64 spread (1.3e-5) should a thread count reorder the sums."""
    ref = torch.from_numpy(golden("vae_encode")["parameters_" + which])
    got = er.vae_encode(sd, INPUTS[which](), None, False, VAE_CFG["down_channels"], VAE_CFG["layers_per_block"])
    d = max_abs(got, ref)
    print(f"vae_encode restatement, input {which.upper()}: max-abs vs reference {d:.3e} (max|ref| {float(ref.abs().max()):.3f})")
    assert got.shape == ref.shape == (3, 2, 4, 4, 4)
    assert d <= 5e-5 * float(ref.abs().max())


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_rounding_floor_is_reported(sd, golden, which, dtype):
    """The emulated 16-bit floors against the golden, printed (measured: fp16 rel-L2 1.5e-3 / 1.8e-3, max-abs / max|ref|
    1.4e-3 / 1.7e-3 on A / B; bf16 1.2e-2 / 1.5e-2 and 1.1e-2 / 1.9e-2).  tests/test_hip_vae_encode.py bounds the kernels by
    twice these, computed there; here only their order of magnitude is held: 16-bit rounding through ~20 stored stages
    cannot come out above 100 units in the last place of the format (2^-11 fp16, 2^-8 bf16) or the restatement is broken."""
    ref = torch.from_numpy(golden("vae_encode")["parameters_" + which])
    emu = er.vae_encode(sd, INPUTS[which](), dtype)
    l2, mx = rel_l2(emu, ref), max_abs(emu, ref) / float(ref.abs().max())
    print(f"vae_encode floor, input {which.upper()}, {dtype}: rel-L2 {l2:.2e}, max-abs / max|ref| {mx:.2e}")
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    assert 0.0 < l2 < 100 * u and mx < 100 * u


def test_distribution_matches_the_reference_class(pkg, golden):
    from topia_xl_amd.vae import DiagonalGaussianDistribution
    g = golden("vae_encode")
    p, q, s = mg.dist_inputs()
    assert float(p[:, 1].min()) < -30.0 and float(p[:, 1].max()) > 20.0, "the parameters must pass both clamp ends"
    d, o = DiagonalGaussianDistribution(p), DiagonalGaussianDistribution(q)
    assert d.parameters is p
    assert float(d.logvar.min()) == -30.0 and float(d.logvar.max()) == 20.0
    got = {"mean": d.mean, "logvar": d.logvar, "std": d.std, "var": d.var, "mode": d.mode(), "kl": d.kl(), "kl_other": d.kl(o),
           "nll": d.nll(s)}
    for k, v in got.items():
        ref = torch.from_numpy(g["dist_" + k])
        assert v.shape == ref.shape, k
        # the same torch expressions: a few fp32 ulp (another CPU's exp), and the reduction order of mean / sum on top
        assert torch.allclose(v, ref, rtol=1e-5 if k in ("kl", "kl_other", "nll") else 1e-6, atol=0.0), k
    det = DiagonalGaussianDistribution(p, deterministic=True)
    assert torch.equal(det.std, torch.from_numpy(g["dist_det_std"])) and torch.equal(det.var, det.std)
    assert torch.equal(det.kl(), torch.from_numpy(g["dist_det_kl"])) and torch.equal(det.nll(s), torch.Tensor([0.0]))
    # sample = mean + std * randn of the generator passed
    gen = torch.Generator().manual_seed(5)
    smp = d.sample(gen)
    noise = torch.randn(d.mean.shape, generator=torch.Generator().manual_seed(5))
    assert torch.equal(smp, d.mean + d.std * noise)


def test_host_semantics_on_cpu_tensors(pkg):
    from topia_xl_amd.pipeline import primitives_to_latents
    vae = pkg.VAE(**VAE_CFG).eval()
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae.encode(torch.zeros(2, 6, 8, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae(torch.zeros(2, 6, 8, 8, 8), sample=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        primitives_to_latents(torch.zeros(1, 3, 4 + 6 * 512), vae, [0.0] * 68, [1.0] * 68)
    # a new state_dict, a repack and a move drop the packed encoder weights together with the decoder's
    vae._enc_pack["x"] = vae._pack["x"] = 1
    vae.load_state_dict(vae.state_dict())
    assert vae._enc_pack == {} and vae._pack == {}
    vae._enc_pack["x"] = vae._pack["x"] = 1
    vae.float()
    assert vae._enc_pack == {} and vae._pack == {}
