"""Golden vectors of the editing steps from the REAL reference (run in the build container only):

    python tests/golden/make_golden_edit.py

`q_sample` and `ddim_reverse_sample` of the unmodified reference (gaussian_diffusion.py:216-231, 580-616; imported through
oracle/ref_import.py) in fp32 on the CPU, on oracle.synth tensors, stored in tests/golden/edit.npz:

  * with a stand-in model that returns a stored tensor: ddim5, every step, v / eps / xstart, clip on and off, at (2, 12, 68);
    ddim25, every step, v, unclipped, at (1, 8, 68).  Only `sample` is stored (pred_xstart is the forward step's, held
    elsewhere);
  * on the `dit_dh72` case of make_golden.py (the real reference DiT, forward_with_cfg, ddim5): the inversion trajectory level
    0 -> 4 at cfg 1, the re-denoised trajectory 4 -> clean at cfg 6 from that inversion's end (the reference has no partial
    loop: ddim_sample step by step), and a q_sample at step 2 followed by the steps 2, 1, 0.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_import, synth  # noqa: E402
from tests.golden.make_golden import DIT_CASES, SEED  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
STEP_CASES = [(5, (2, 12, 68), ("v", "eps", "xstart"), (False, True)), (25, (1, 8, 68), ("v",), (False,))]


def step_inputs(n: int, shape):
    """x (a level / a clean sample), the stand-in model's output (2C channels: learned-range variance) and q_sample's noise."""
    B, N, C = shape
    return (synth.tensor(SEED, f"edit{n}.x", shape), synth.tensor(SEED, f"edit{n}.mo", (B, N, 2 * C)),
            synth.tensor(SEED, f"edit{n}.noise", shape))


def dit_noise(shape):
    return synth.tensor(SEED, "edit.dit.noise", shape)


def gen_steps(diffusion_pkg, out):
    for n, shape, pars, clips in STEP_CASES:
        x, mo, noise = step_inputs(n, shape)
        for par in pars:
            d = diffusion_pkg.create_diffusion(timestep_respacing=f"ddim{n}", noise_schedule="squaredcos_cap_v2",
                                               parameterization=par, diffusion_steps=1000)
            if par == pars[0]:
                out[f"q{n}"] = np.stack([d.q_sample(x, torch.full((shape[0],), i, dtype=torch.int64), noise).numpy()
                                         for i in range(n)])
            for clip in clips:
                out[f"rev{n}_{par}_clip{int(clip)}"] = np.stack([
                    d.ddim_reverse_sample(lambda x_, t_, **kw: mo, x, torch.full((shape[0],), i, dtype=torch.int64),
                                          clip_denoised=clip)["sample"].numpy() for i in range(n)])


def gen_dit(dit_mod, diffusion_pkg, out):
    name, cfg, heads, N, L, B = DIT_CASES[1]
    model = dit_mod.DiT(seq_length=N, num_heads=heads, attn_proj_bias=True, cond_drop_prob=0.1, **cfg).eval()
    model.load_state_dict(synth.dit_state_dict(SEED, **cfg), strict=True)
    x = synth.tensor(SEED, name + ".x", (B, N, cfg["in_channels"]))
    y = synth.tensor(SEED, name + ".y", (B, L, cfg["condition_channels"]))
    d = diffusion_pkg.create_diffusion(timestep_respacing="ddim5", noise_schedule="squaredcos_cap_v2",
                                       parameterization="v", diffusion_steps=1000)

    def t(i):
        return torch.full((B,), i, dtype=torch.int64)

    with torch.no_grad():
        inv, lvl = [], x
        for i in range(4):                                            # level 0 -> 4 under cfg 1
            lvl = d.ddim_reverse_sample(model.forward_with_cfg, lvl, t(i), clip_denoised=False,
                                        model_kwargs=dict(y=y, cfg_scale=1.0))["sample"]
            inv.append(lvl.numpy())
        out["dit_invert"] = np.stack(inv)
        red = []
        for i in range(4, -1, -1):                                    # level 4 -> clean under cfg 6
            lvl = d.ddim_sample(model.forward_with_cfg, lvl, t(i), clip_denoised=False, model_kwargs=dict(y=y, cfg_scale=6.0))["sample"]
            red.append(lvl.numpy())
        out["dit_redenoise"] = np.stack(red)
        lvl = d.q_sample(x, t(2), dit_noise(x.shape))
        out["dit_q2"] = lvl.numpy()
        part = []
        for i in range(2, -1, -1):
            lvl = d.ddim_sample(model.forward_with_cfg, lvl, t(i), clip_denoised=False, model_kwargs=dict(y=y, cfg_scale=6.0))["sample"]
            part.append(lvl.numpy())
        out["dit_partial2"] = np.stack(part)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    dit_mod, _, diffusion_pkg, _ = ref_import.load()
    out = {"seed": np.int64(SEED)}
    gen_steps(diffusion_pkg, out)
    gen_dit(dit_mod, diffusion_pkg, out)
    path = os.path.join(HERE, "edit.npz")
    np.savez_compressed(path, **out)
    print("edit.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
