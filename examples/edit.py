"""Edit a stored asset: regenerate the primitives on one side of a plane, keep everything else.

  denoised.pt (or a freshly generated asset) -> recon_param -> VAE encode -> tokens -> q_sample to level --start-step
        -> DDIM from there with the kept primitives held on their own trajectory -> VAE decode -> new denoised.pt

The primitives whose centres lie in the half-space  normal . xyz > offset  are regenerated under the conditioning image; the
others come out as the encode -> decode round trip of the input, bit for bit.  Without --dit / --vae checkpoints every network
carries random weights (as examples/generate.py): the outputs are noise, the point is the data flow and the per-stage timing.

    python examples/edit.py [--denoised IN.pt] [--out OUT.pt] [--steps 25] [--start-step 12] [--normal 1 0 0] [--offset 0]
                            [--mode noise|invert] [--sampler ddim|dpm] [--dit DIT.pt] [--vae VAE.pt] [--small]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--denoised", default=None, help="the asset to edit (a denoised.pt); generated first when absent")
    ap.add_argument("--out", default="denoised_edited.pt")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--start-step", type=int, default=12, help="the level the asset is taken to (0 .. steps - 1): higher = freer")
    ap.add_argument("--normal", type=float, nargs=3, default=[1.0, 0.0, 0.0])
    ap.add_argument("--offset", type=float, default=0.0)
    ap.add_argument("--mode", choices=["noise", "invert"], default="noise", help="invert: DDIM inversion, regenerates everything")
    ap.add_argument("--sampler", choices=["ddim", "dpm"], default="ddim", help="dpm: generate and re-denoise with DPM-Solver++(2M) "
                    "over the same ddim<steps> grid (e.g. --steps 12 --start-step 6)")
    ap.add_argument("--dit", default=None, help="DiT checkpoint (.pt with 'ema'); synthetic weights when absent")
    ap.add_argument("--vae", default=None, help="VAE checkpoint (.pt with 'model_state_dict'); synthetic weights when absent")
    ap.add_argument("--small", action="store_true", help="tiny networks (smoke run)")
    a = ap.parse_args()
    __graft_entry__.build()
    import topia_xl_amd as pkg
    from topia_xl_amd import dinov2, pipeline

    dev = "cuda:0"
    torch.manual_seed(42)
    if a.small:
        cond = dinov2.DinoVisionTransformer(img_size=56, embed_dim=96, depth=2, num_heads=3)
        dit = pkg.DiT(seq_length=64, in_channels=68, condition_channels=96, hidden_size=288, depth=2, num_heads=4,
                      attn_proj_bias=True, cond_drop_prob=0.1)
        n_prims, img = 64, 56
    else:
        cond = dinov2.vit_base(img_size=518, init_values=1.0)
        dit = pkg.DiT(seq_length=2048, in_channels=68, condition_channels=768, hidden_size=1152, depth=28, num_heads=16,
                      attn_proj_bias=True, cond_drop_prob=0.1)
        n_prims, img = 2048, 518
    vae = pkg.VAE(in_channels=6, latent_channels=1, out_channels=6, down_channels=[32, 256], mid_attention=True,
                  up_channels=[256, 32], layers_per_block=2)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():   # trained-network-like magnitudes for whatever has no checkpoint (examples/generate.py)
        for m, ckpt in ((cond, None), (dit, a.dit), (vae, a.vae)):
            if ckpt is None:
                for name, p in m.named_parameters():
                    if p.dim() > 1 and "token" not in name and "pos_embed" not in name:
                        p.copy_(torch.randn(p.shape, generator=g) * (0.6 if "adaLN" in name else 1.0) * p[0].numel() ** -0.5)
                    elif "norm" in name and name.endswith("weight") or name.endswith("gamma"):
                        p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
                    else:
                        p.copy_(0.05 * torch.randn(p.shape, generator=g))
    pipeline.load_checkpoints(dit, vae, a.dit, a.vae)
    for m in (cond, dit, vae):
        m.eval().to(dev)
    diffusion = pkg.create_diffusion(f"ddim{a.steps}", noise_schedule="squaredcos_cap_v2", parameterization="v")
    mean, std = [0.0] * 68, [1.0] * 68      # the shipped configuration carries its own per-channel statistics (configs/inference_dit.yml:64-65)

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        print(f"{name:52s} {1e3 * (time.perf_counter() - t0):9.2f} ms", flush=True)
        return r

    image = torch.rand(1, 3, img, img, device=dev)
    y = timed("DINOv2 conditioner tokens", lambda: cond.conditioner_tokens(image))
    kw = dict(y=y, cfg_scale=6.0, precision_dtype=torch.float16, enable_amp=True)
    if a.denoised:
        sd = torch.load(a.denoised, map_location="cpu")["model_state_dict"]
        recon = torch.cat([sd["srt_param"], sd["feat_param"]], dim=-1)[None].float().to(dev)
    else:
        x = torch.randn(1, n_prims, 68).to(dev)
        loop, label = {"ddim": (diffusion.ddim_sample_loop, "DDIM"), "dpm": (diffusion.dpm_solver_sample_loop, "DPM-Solver++(2M)")}[a.sampler]
        samples = timed(f"{label} loop, {a.steps} steps, CFG 6 (first call)",
                        lambda: loop(dit.forward_with_cfg, x.shape, noise=x, clip_denoised=False, model_kwargs=kw))
        recon = timed("de-normalise + VAE decode", lambda: pipeline.latents_to_primitives(samples, vae, mean, std))
        recon[:, :, 1:4] = 1.2 * torch.rand_like(recon[:, :, 1:4]) - 0.6      # random networks: give the primitives a plausible layout
    normal = torch.tensor(a.normal, device=dev)
    regenerate = (recon[:, :, 1:4] @ normal) > a.offset                        # [1, N]: centres in the half-space
    keep = None if a.mode == "invert" else ~regenerate
    print(f"{int(regenerate.sum())} of {recon.shape[1]} primitives lie in the half-space"
          + (" (mode invert regenerates all of them)" if keep is None else " and are regenerated"))

    tokens = timed("VAE encode + normalise (stage alone)", lambda: pipeline.primitives_to_latents(recon, vae, mean, std))
    trip = timed("de-normalise + VAE decode (stage alone)", lambda: pipeline.latents_to_primitives(tokens, vae, mean, std))

    def edit():
        return pipeline.redenoise_primitives(recon, vae, dit, diffusion, y, start_step=a.start_step, mode=a.mode, keep=keep,
                                             generator=torch.Generator(device=dev).manual_seed(11), latent_mean=mean, latent_std=std,
                                             sampler=a.sampler)
    edit_steps = a.start_step + 1 + (a.start_step if a.mode == "invert" else 0)
    timed(f"redenoise_primitives, {a.sampler}, {edit_steps} DiT steps (first call)", edit)
    out = timed(f"redenoise_primitives, {a.sampler}, {edit_steps} DiT steps", edit)
    if keep is not None:
        same = bool(torch.equal(out[keep], trip[keep]))
        moved = int((out[~keep] != trip[~keep]).any(-1).sum())
        print(f"kept primitives bit-identical to the encode -> decode round trip: {same}; regenerated primitives that changed: "
              f"{moved} of {int((~keep).sum())}")
    pipeline.save_denoised(a.out, out)
    print("recon_param", tuple(out.shape), "->", a.out)


if __name__ == "__main__":
    main()
