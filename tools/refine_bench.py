"""Timing and effect of primitive refinement (fit.refine_primitives; csrc/primsdf.hip, csrc/rowops.hip) on the example torus of
examples/tokenize_mesh.py at P = 2048 primitives of 8^3 voxels, 256 training points per primitive (n = 524288, the default):

* per kernel, event-timed after a warm-up: the training-mode `primx_primsdf_query`, `primx_primsdf_query_backward` at the same n
  (with the atomic bytes it adds per step and their share of the chip-wide float-atomic rate), `primx_adam_step` on the payload
  and on srt; and a whole refinement step inside the loop;
* the whole fit with and without refinement;
* the field error before and after: |sdf| at the 65536 surface candidates (where the mesh's SDF is 0) and the error against
  the mesh's own field at held-out points of the primitives' boxes (another seed than the training set);
* with --sweep: the same errors for a grid of (samples per primitive, lr, lr_srt, steps), the measurement behind the defaults.

    python tools/refine_bench.py [--steps 20] [--spp 256] [--reps 5] [--sweep]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

ATOMIC_RATE = 1.3e12       # bytes of fp32 atomic adds per second, chip-wide (contiguous 256-byte wave instructions)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps, out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=256, help="training points per primitive")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--prims", type=int, default=2048)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    __graft_entry__.build()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from tokenize_mesh import torus
    from topia_xl_amd import fit, ops, primsdf

    dev = "cuda:0"
    P, S, spp = a.prims, 8, a.spp
    v, f, _, alb, ro, me = (t.to(dev) for t in torus())
    mesh = (v, f, alb, ro, me)
    fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S)
    t_fit, (recon, info) = wall(lambda: fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S))
    field = fit.MeshField(info["v"], info["f"], info["attr"])
    cand = info["candidates"]
    lin = torch.linspace(-1, 1, S).to(dev)
    held = fit.refine_points(recon[:, :4], 16, seed=12345)
    q = field.query(held)
    held_t = torch.cat([q["sdf"], q["tex"], q["mat"]], 1)

    def errors(r):
        srt, feat = r[:, :4].contiguous(), r[:, 4:].contiguous()
        m = primsdf.PrimSDF(num_prims=P, prim_shape=S).to(dev).eval()
        m.srt_param.data, m.feat_param.data = srt, feat
        s = m.query(cand)[:, 0].abs()
        d = (m.query(held) - held_t).abs()
        return (f"|sdf| at the {cand.shape[0]} candidates mean {float(s.mean()):.3e} max {float(s.max()):.3e}; held-out points: "
                f"sdf mean {float(d[:, 0].mean()):.3e} max {float(d[:, 0].max()):.3e}, tex mean {float(d[:, 1:4].mean()):.3e}, "
                f"mat mean {float(d[:, 4:].mean()):.3e}")

    print(f"--- torus, P = {P}, S = {S}, {spp} training points per primitive", flush=True)
    print(f"initialisation                    {errors(recon)}")

    # per kernel
    srt, feat = recon[:, :4].clone().contiguous(), recon[:, 4:].clone().contiguous()
    pts = fit.refine_points(srt, spp, 0)
    n = pts.shape[0]
    gout = torch.randn(n, 6, device=dev) / n
    gs, gf = torch.zeros_like(srt), torch.zeros_like(feat)
    ms_f, _ = timed(lambda: primsdf._query_train(pts, srt, feat, lin, S), a.reps)
    ms_b, _ = timed(lambda: primsdf.query_backward(pts, srt, feat, gout, S, gsrt=gs, gfeat=gf), a.reps)
    ms_bf, _ = timed(lambda: primsdf.query_backward(pts, srt, feat, gout, S, gfeat=gf, want_srt=False), a.reps)
    cover = float((primsdf._query_train(pts, srt, torch.ones_like(feat), lin, S)[:, 0] > 0).float().mean())
    pairs = _pairs(pts, srt)            # (point, covering primitive) pairs: each adds 8 x 6 payload floats and 4 srt floats
    bytes_step = pairs * (48 + 4) * 4
    print(f"primx_primsdf_query (training)    {ms_f:10.3f} ms   n = {n}, {100 * cover:.1f} % covered, {pairs / n:.2f} covering primitives per point")
    print(f"primx_primsdf_query_backward      {ms_b:10.3f} ms   = {ms_b / ms_f:.2f} x the forward; payload only {ms_bf:.3f} ms")
    print(f"  atomic adds per step            {bytes_step / 1e6:10.1f} MB  = {1e3 * bytes_step / ATOMIC_RATE:.3f} ms at {ATOMIC_RATE / 1e12:.1f} TB/s; "
          f"the kernel runs at {bytes_step / (ms_b * 1e-3) / 1e12:.3f} TB/s of added bytes")
    mf, vf = torch.zeros_like(feat), torch.zeros_like(feat)
    ms_a, _ = timed(lambda: ops.adam_step(feat, gf, mf, vf, 1, 1e-9, zero_grad=True), a.reps)
    ms_s, _ = timed(lambda: ops.adam_step(srt, gs, torch.zeros_like(srt), torch.zeros_like(srt), 1, 1e-9, zero_grad=True), a.reps)
    print(f"primx_adam_step, payload          {ms_a:10.3f} ms   {feat.numel()} elements, {feat.numel() * 28 / (ms_a * 1e-3) / 1e12:.2f} TB/s")
    print(f"primx_adam_step, srt              {ms_s:10.3f} ms   {srt.numel()} elements")

    # the loop and the whole fit
    fit.refine_primitives(recon, field, 2, samples_per_prim=spp)
    t_1, _ = wall(lambda: fit.refine_primitives(recon, field, 1, samples_per_prim=spp))
    t_n, (out, rinfo) = wall(lambda: fit.refine_primitives(recon, field, a.steps, samples_per_prim=spp))
    print(f"refine_primitives, {a.steps} steps        {t_n:10.2f} ms   = targets and set-up {t_1:.2f} ms (1 step) + {(t_n - t_1) / max(a.steps - 1, 1):.3f} ms per step")
    print(f"  loss {rinfo['loss'][0]:.4e} -> {rinfo['loss'][-1]:.4e}")
    t_ref, _ = wall(lambda: fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S, refine=a.steps, refine_kw={"samples_per_prim": spp}))
    print(f"mesh_to_primitives                {t_fit:10.2f} ms   with refine={a.steps}: {t_ref:.2f} ms")
    print(f"after {a.steps} steps                    {errors(out)}")
    if a.sweep:
        for spp_s in (64, 256, 512):
            for lr in (1e-3, 2e-3, 5e-3):
                for srt_on, ratio in ((False, 0.0), (True, 0.1), (True, 0.01), (True, 0.001)):
                    for steps in (20, 50, 100):
                        if spp_s != 64 and (srt_on or lr > 2e-3):
                            continue
                        o, ri = fit.refine_primitives(recon, field, steps, lr=lr, samples_per_prim=spp_s, refine_srt=srt_on, lr_srt=lr * ratio)
                        print(f"spp {spp_s:3d} lr {lr:.0e} lr_srt {lr * ratio:.0e} steps {steps:3d}: loss {ri['loss'][0]:.3e} -> {ri['loss'][-1]:.3e} "
                              f"(max {max(ri['loss']):.3e}); {errors(o)}", flush=True)


def _pairs(pts, srt):
    """Number of (point, covering primitive) pairs, by torch in chunks (the forward's cull: max |d| < |s|)."""
    total = 0
    for lo in range(0, pts.shape[0], 8192):
        d = (pts[lo:lo + 8192, None, :] - srt[None, :, 1:4]).abs().amax(-1)
        total += int((d < srt[None, :, 0].abs()).sum())
    return total


if __name__ == "__main__":
    main()
