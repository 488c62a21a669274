"""Timing of VAE.encode (csrc/vaeenc.hip + the decoder's kernels) next to VAE.decode on the same box: P = 2048 (one sample)
and 8 x 2048 primitives (the chunk of pipeline.primitives_to_latents), fp16 and bf16, and the per-launch split of the three
encoder kernels (ops.PROFILE: HIP events around every timed launch).  Event-timed after warm-up, synthetic weights.

    python tools/vae_encode_bench.py [--reps 20]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    __graft_entry__.build()
    import topia_xl_amd as pkg
    from oracle import synth
    from topia_xl_amd import ops

    dev = "cuda:0"
    cfg = dict(in_channels=6, latent_channels=1, out_channels=6, down_channels=[32, 256], mid_attention=True,
               up_channels=[256, 32], layers_per_block=2, gradient_checkpointing=False)
    vae = pkg.VAE(**cfg).eval()
    vae.load_state_dict(synth.state_dict_like(1234, vae.state_dict()), strict=True)
    vae.to(dev)
    gen = torch.Generator(device=dev).manual_seed(5)
    for dtype in (torch.float16, torch.bfloat16):
        vae.compute_dtype = dtype
        for P in (2048, 8 * 2048):
            x = torch.randn(P, 6, 8, 8, 8, device=dev, generator=gen) * 0.8
            z = torch.randn(P, 1, 4, 4, 4, device=dev, generator=gen)
            enc, _ = timed(lambda: vae.encode(x, normalize=True).parameters, a.reps)
            dec, _ = timed(lambda: vae.decode(z, denormalize=True), a.reps)
            print(f"{str(dtype)[6:]:9s} P = {P:6d}: VAE.encode {enc:8.3f} ms  ({P / enc / 1e3:7.2f} M primitives/s)   "
                  f"VAE.decode {dec:8.3f} ms", flush=True)
            # the per-launch split: every timed launch of one encode, summed by kernel
            ops.PROFILE = []
            try:
                for _ in range(a.reps):
                    vae.encode(x, normalize=True)
                torch.cuda.synchronize()
                split = {}
                for tag, flops, s, e in ops.PROFILE:
                    name = tag.split(" ")[0].split("<")[0]
                    t, f = split.get(name, (0.0, 0.0))
                    split[name] = (t + s.elapsed_time(e) / a.reps, f + flops / a.reps)
            finally:
                ops.PROFILE = None
            for name in ("enc_conv_in_kernel", "conv3_down_kernel", "enc_head_kernel"):
                t, f = split.pop(name)
                print(f"    {name:22s} {t * 1e3:8.1f} us  {f / t / 1e9:7.1f} TFLOP/s", flush=True)
            rest = sum(t for t, _ in split.values())
            print(f"    {'the decoder kernels':22s} {rest * 1e3:8.1f} us  ({len(split)} kinds of timed launches)", flush=True)
            del x, z


if __name__ == "__main__":
    main()
