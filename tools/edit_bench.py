"""Timing of the editing path on one box, in one run:

  * the three editing kernels next to primx_diffusion_step at (1, 2048, 68) and (8, 2048, 68) with fp16 model output
    (event-timed windows of --launches launches each, the four kernels alternating over --rounds rounds: min / median);
  * a whole pipeline.redenoise_primitives (start_step = 12 of ddim25, half of the primitives kept: encode, q_sample,
    13 masked DDIM steps with CFG, decode) next to the plain job (25 DDIM steps with CFG + decode), DiT-XL and the VAE
    with synthetic weights, host clock around a device synchronise, the two jobs alternating.

    python tools/edit_bench.py [--launches 2000] [--rounds 5] [--jobs 5] [--small]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402


def window(fn, launches):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / launches          # microseconds per launch


def kernels(pkg, ops, a):
    dev = "cuda:0"
    d = pkg.create_diffusion("ddim25", noise_schedule="squaredcos_cap_v2", parameterization="v")
    coef = torch.from_numpy(d.step_coefficients(0.0)).to(dev)
    g = torch.Generator(device=dev).manual_seed(1)
    for B in (1, 8):
        shape = (B, 2048, 68)
        x, noise, known = (torch.randn(shape, device=dev, generator=g) for _ in range(3))
        mo = torch.randn(B, 2048, 136, device=dev, generator=g).half()
        keep = (torch.rand(B, 2048, device=dev, generator=g) < 0.5).view(torch.uint8)
        keep_el = (torch.rand(shape, device=dev, generator=g) < 0.5).view(torch.uint8)
        kw = dict(mean_type=2, var_type=3, ancestral=False, clip_denoised=False, noise=None)
        fns = {
            "primx_diffusion_step": lambda: ops.diffusion_step(x, mo, coef, 12, **kw),
            "primx_diffusion_step_keep (rows)": lambda: ops.diffusion_step_keep(x, mo, coef, 12, known=known, known_noise=noise,
                                                                                keep=keep, **kw),
            "primx_diffusion_step_keep (elements)": lambda: ops.diffusion_step_keep(x, mo, coef, 12, known=known, known_noise=noise,
                                                                                    keep=keep_el, **kw),
            "primx_diffusion_reverse_step": lambda: ops.diffusion_reverse_step(x, mo, coef, 12, mean_type=2, clip_denoised=False),
            "primx_q_sample": lambda: ops.q_sample(x, noise, coef, 12),
        }
        times = {k: [] for k in fns}
        for fn in fns.values():
            window(fn, 50)                                # warm-up of every shape the timed windows use
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(window(fn, a.launches))
        print(f"shape {shape}, fp16 model output, {a.rounds} windows of {a.launches} launches (host call + kernel, back to back):")
        for k, v in times.items():
            print(f"    {k:38s} min {min(v):7.2f} us   median {statistics.median(v):7.2f} us", flush=True)


def jobs(pkg, a):
    from topia_xl_amd import pipeline
    dev = "cuda:0"
    if a.small:
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
    d = pkg.create_diffusion("ddim25", noise_schedule="squaredcos_cap_v2", parameterization="v")
    gd = torch.Generator(device=dev).manual_seed(3)
    y = torch.randn(1, L, Dc, device=dev, generator=gd)
    x = torch.randn(1, N, 68, device=dev, generator=gd)
    mean, std = [0.0] * 68, [1.0] * 68
    kw = dict(y=y, cfg_scale=6.0, precision_dtype=torch.float16, enable_amp=True)

    def plain():
        s = d.ddim_sample_loop(dit.forward_with_cfg, x.shape, noise=x, clip_denoised=False, model_kwargs=kw)
        return pipeline.latents_to_primitives(s, vae, mean, std)

    recon = plain()
    keep = torch.rand(1, N, device=dev, generator=gd) < 0.5
    noise = torch.randn(1, N, 68, device=dev, generator=gd)

    def edit():
        return pipeline.redenoise_primitives(recon, vae, dit, d, y, start_step=12, keep=keep, noise=noise, latent_mean=mean,
                                             latent_std=std)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for fn in (plain, edit, plain, edit):
        fn()                                              # warm-up: code objects, packed weights, workspaces
    t = {"plain": [], "edit": []}
    for _ in range(a.jobs):
        t["plain"].append(clock(plain))
        t["edit"].append(clock(edit))
    print(f"whole jobs, {N} primitives, batch 1, fp16, CFG 6, {a.jobs} alternating runs each:")
    print(f"    25 DDIM steps + decode                                    min {min(t['plain']):8.2f} ms   median "
          f"{statistics.median(t['plain']):8.2f} ms")
    print(f"    redenoise_primitives (encode, q_sample, 13 kept steps, decode) min {min(t['edit']):8.2f} ms   median "
          f"{statistics.median(t['edit']):8.2f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="tiny DiT for the whole-job part (a rehearsal, not a measurement)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edit_bench needs a HIP device: there is nothing to time without one")
    __graft_entry__.build()
    import topia_xl_amd as pkg
    from topia_xl_amd import ops
    kernels(pkg, ops, a)
    jobs(pkg, a)


if __name__ == "__main__":
    main()
