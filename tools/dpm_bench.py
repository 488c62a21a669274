"""Timing of few-step sampling on one box, in one run: whole jobs - the sampling loop with CFG, then de-normalisation + VAE
decode - for 25 DDIM steps next to DPM-Solver++(2M) at 10, 12 and 15 steps (diffusion/sampler.py), at batch 1 and batch 8.
DiT-XL and the VAE with synthetic weights, 2048 primitives, fp16, CFG 6; host clock around a device synchronise, the four
jobs alternating, min and median.  The loop alone is timed the same way, next to K / 25 of the ddim25 loop: what is left is
the per-loop work that does not shrink with K (timestep planning, table upload).

Synthetic weights: the times are real, the samples are noise - this says nothing about quality at 10 to 15 steps.

    python tools/dpm_bench.py [--jobs 5] [--batches 1 8] [--small]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

CASES = (("ddim", 25), ("dpm", 10), ("dpm", 12), ("dpm", 15))


def networks(pkg, small, dev):
    if small:
        dit = pkg.DiT(seq_length=64, in_channels=68, condition_channels=96, hidden_size=288, depth=2, num_heads=4,
                      attn_proj_bias=True, cond_drop_prob=0.1)
        N, L, Dc = 64, 21, 96
    else:
        dit = pkg.DiT(seq_length=2048, in_channels=68, condition_channels=768, hidden_size=1152, depth=28, num_heads=16,
                      attn_proj_bias=True, cond_drop_prob=0.1)
        N, L, Dc = 2048, 1374, 768
    vae = pkg.VAE(in_channels=6, latent_channels=1, out_channels=6, down_channels=[32, 256], mid_attention=True,
                  up_channels=[256, 32], layers_per_block=2)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():   # trained-network-like magnitudes, as examples/generate.py
        for m in (dit, vae):
            for name, p in m.named_parameters():
                if p.dim() > 1 and "token" not in name and "pos_embed" not in name:
                    p.copy_(torch.randn(p.shape, generator=g) * (0.6 if "adaLN" in name else 1.0) * p[0].numel() ** -0.5)
                elif "norm" in name and name.endswith("weight") or name.endswith("gamma"):
                    p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
            m.eval().to(dev)
    return dit, vae, N, L, Dc


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=5, help="timed runs of each job; the jobs alternate")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--small", action="store_true", help="tiny networks (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dpm_bench needs a HIP device: there is nothing to time without one")
    __graft_entry__.build()
    import topia_xl_amd as pkg
    from topia_xl_amd import pipeline
    dev = "cuda:0"
    dit, vae, N, L, Dc = networks(pkg, a.small, dev)
    procs = {k: pkg.create_diffusion(f"ddim{k}", noise_schedule="squaredcos_cap_v2", parameterization="v") for _, k in CASES}
    mean, std = [0.0] * 68, [1.0] * 68
    gd = torch.Generator(device=dev).manual_seed(3)
    for B in a.batches:
        y = torch.randn(B, L, Dc, device=dev, generator=gd)
        x = torch.randn(B, N, 68, device=dev, generator=gd)
        kw = dict(y=y, cfg_scale=6.0, precision_dtype=torch.float16, enable_amp=True)

        def loop(kind, k):
            d = procs[k]
            fn = d.ddim_sample_loop if kind == "ddim" else d.dpm_solver_sample_loop
            return fn(dit.forward_with_cfg, x.shape, noise=x, clip_denoised=False, model_kwargs=kw)

        def job(kind, k):
            return pipeline.latents_to_primitives(loop(kind, k), vae, mean, std)

        for case in CASES:
            job(*case)                                        # warm-up: code objects, packed weights, workspaces, tables
        t_job, t_loop = {c: [] for c in CASES}, {c: [] for c in CASES}
        for _ in range(a.jobs):
            for case in CASES:
                t_job[case].append(clock(lambda: job(*case)))
            for case in CASES:
                t_loop[case].append(clock(lambda: loop(*case)))
        base = min(t_loop[CASES[0]])
        print(f"{N} primitives, batch {B}, fp16, CFG 6, {a.jobs} alternating runs each:")
        for kind, k in CASES:
            j, l = t_job[kind, k], t_loop[kind, k]
            name = f"{'DDIM' if kind == 'ddim' else 'DPM-Solver++(2M)'} {k} steps"
            print(f"    {name:26s} job (loop + decode) min {min(j):8.2f} ms  median {statistics.median(j):8.2f} ms   "
                  f"loop min {min(l):8.2f} ms  median {statistics.median(l):8.2f} ms   {k}/25 of the ddim25 loop {base * k / 25:8.2f} ms   "
                  f"samples/s {1e3 * B / min(j):6.2f}", flush=True)


if __name__ == "__main__":
    main()
