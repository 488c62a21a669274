"""Generate tests/golden/vae_encode.npz: the REFERENCE VAE encoder's posterior parameters (fp32, CPU).

    python tests/golden/make_golden_vae_encode.py

Same mechanism as make_golden.py: the unmodified reference ``models.vae3d_dib.VAE`` through oracle/ref_import.py, the shipped
configuration (VAE_CFG), the suite's synthetic weights (``synth.state_dict_like(SEED, ...)``), 8 threads.  The file holds no
weights - the tests regenerate them from the seed - only recorded results:

* ``parameters_a`` / ``parameters_b``: ``quant_conv(encoder(x))`` [3, 2, 4, 4, 4] for input A = ``synth.tensor(77, "enc.x",
  (3, 6, 8, 8, 8))`` and input B = the ``decoded`` array of vae_decode.npz (a realistic range, |x| <= 6);
* ``dist_*``: what the reference's ``DiagonalGaussianDistribution`` makes of ``dist_parameters`` (random values, some beyond
  both clamp ends of the log-variance) and of ``dist_other`` / ``dist_sample``: every field and method the port restates.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import, synth  # noqa: E402
from tests.golden.make_golden import SEED, VAE_CFG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ENC_SEED = 77


def input_a() -> torch.Tensor:
    return synth.tensor(ENC_SEED, "enc.x", (3, 6, 8, 8, 8))


def input_b() -> torch.Tensor:
    return torch.from_numpy(np.load(os.path.join(HERE, "vae_decode.npz"), allow_pickle=False)["decoded"]).float()


def dist_inputs():
    """(parameters, other, sample) of the distribution check: logvar spans [-45, 35], i.e. both clamp ends are passed."""
    p = synth.tensor(ENC_SEED, "dist.p", (5, 2, 4, 4, 4))
    p[:, 1] = p[:, 1] * 20.0
    p[0, 1, 0, 0, :2] = torch.tensor([-45.0, 35.0])
    q = synth.tensor(ENC_SEED, "dist.q", (5, 2, 4, 4, 4))
    s = synth.tensor(ENC_SEED, "dist.s", (5, 1, 4, 4, 4))
    return p, q, s


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _, vae_mod, _, _ = ref_import.load()
    vae = vae_mod.VAE(**VAE_CFG).eval()
    vae.load_state_dict(synth.state_dict_like(SEED, vae.state_dict()), strict=True)
    out = {"seed": np.int64(SEED)}
    with torch.no_grad():
        out["parameters_a"] = vae.encode(input_a()).parameters.numpy()
        out["parameters_b"] = vae.encode(input_b()).parameters.numpy()
        p, q, s = dist_inputs()
        d, o = vae_mod.DiagonalGaussianDistribution(p), vae_mod.DiagonalGaussianDistribution(q)
        for name in ("mean", "logvar", "std", "var"):
            out["dist_" + name] = getattr(d, name).numpy()
        out["dist_mode"] = d.mode().numpy()
        out["dist_kl"] = d.kl().numpy()
        out["dist_kl_other"] = d.kl(o).numpy()
        out["dist_nll"] = d.nll(s).numpy()
        det = vae_mod.DiagonalGaussianDistribution(p, deterministic=True)
        out["dist_det_std"] = det.std.numpy()
        out["dist_det_kl"] = det.kl().numpy()
    np.savez_compressed(os.path.join(HERE, "vae_encode.npz"), **out)
    for k, v in out.items():
        print(k, getattr(v, "shape", v))


if __name__ == "__main__":
    main()
