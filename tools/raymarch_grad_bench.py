"""Timing of the differentiable ray marcher: forward, backward and one Adam step on the template, on the synthetic scene of
tools/raymarch_bench.py (2048 primitives with 8^3 RGBA payloads, the shipped step: volradius 10000, dt 1.0 -> 1e-4 of the
normalised volume per step), and the number of fp32 atomic adds one backward issues.

    python tools/raymarch_grad_bench.py            # RES=256 rays per side by default; REPS=5 timed launches per stage

The image is RES x RES (default 256: the whole run, counting pass included, stays well under a minute); the gradient of the image is
seeded normal, all four gradients are computed.  The stages are timed with events on the current stream, REPS launches each, in
alternating order (forward, backward, Adam, forward, ...), and the median is printed.  The atomic adds are counted by a second
process with PRIMX_RAYMARCH_STATS=1 (csrc/raymarch.hip: device counters and a synchronising read-back, so never in the timed
process)."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import __graft_entry__  # noqa: E402


def scene(R, dev):
    from topia_xl_amd import raymarch as rm
    g = torch.Generator().manual_seed(11)
    K, S, volradius = 2048, 8, 10000.0
    half = 0.03 + 0.05 * torch.rand(1, K, 1, generator=g)                      # half extents in the [-1, 1] volume
    pos = 1.2 * torch.rand(1, K, 3, generator=g) - 0.6
    rot = torch.eye(3).expand(1, K, 3, 3).contiguous()
    scale = (1.0 / half).expand(-1, -1, 3).contiguous()
    tpl = torch.rand(1, K, S, S, S, 4, generator=g)
    tpl[..., 3] *= 40.0
    gout = torch.randn(1, R, R, 4, generator=g)
    Rt = torch.tensor([[[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 5 * volradius]]])
    Kc = torch.tensor([[[2084.95 * R / 1024, 0, R / 2], [0, 2084.95 * R / 1024, R / 2], [0, 0, 1]]])
    cam = rm.convert_camera_parameters(Rt, Kc)
    focal = torch.diagonal(cam["focal"], dim1=1, dim2=2).contiguous()
    rp, rd, tm = rm.compute_raydirs(cam["campos"].to(dev), cam["camrot"].to(dev), focal.to(dev), cam["princpt"].to(dev),
                                    rm.base_pixel_coords(R, R, dev)[None].contiguous(), volradius)
    return dict(rp=rp, rd=rd, tm=tm, dt=1.0 / volradius, prim=(pos.to(dev), rot.to(dev), scale.to(dev)), tpl=tpl.to(dev), gout=gout.to(dev))


def main():
    __graft_entry__.build()
    from topia_xl_amd import ops
    from topia_xl_amd import raymarch as rm
    dev = "cuda:0"
    R, reps = int(os.environ.get("RES", "256")), int(os.environ.get("REPS", "5"))
    s = scene(R, dev)
    fwd = lambda: rm.mvpraymarch(s["rp"], s["rd"], s["dt"], s["tm"], s["prim"], s["tpl"])
    bwd = lambda: rm.raymarch_backward(s["rp"], s["rd"], s["dt"], s["tm"], s["prim"], s["tpl"], s["gout"])
    if "--count" in sys.argv:                                                   # the child: one backward, counters to stderr
        bwd()
        torch.cuda.synchronize()
        return
    img, grads = fwd(), bwd()
    param, m, v = s["tpl"].clone(), torch.zeros_like(s["tpl"]), torch.zeros_like(s["tpl"])
    adam = lambda: ops.adam_step(param, grads[0], m, v, 1, lr=1e-3)
    adam()
    torch.cuda.synchronize()
    times = {"forward": [], "backward": [], "adam": []}
    for _ in range(reps):
        for name, fn in (("forward", fwd), ("backward", bwd), ("adam", adam)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    alpha = img[..., 3]
    print(f"raymarch grad bench {R}x{R}, K=2048, 8^3 template, dt/volradius=1e-4, {reps} launches per stage (median, min .. max ms): "
          f"coverage {float((alpha > 0).float().mean()):.2f}, saturated {float((alpha >= 0.999).float().mean()):.2f}")
    for name, ts in times.items():
        print(f"  {name:9s} {statistics.median(ts):10.3f} ms   ({min(ts):.3f} .. {max(ts):.3f})")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--count"], env=dict(os.environ, PRIMX_RAYMARCH_STATS="1"),
                           capture_output=True, text=True, timeout=300)
    lines = [ln for ln in child.stderr.splitlines() if ln.startswith("raymarch backward stats")]
    print("  " + (lines[-1] if lines else f"atomic adds: not counted (the counting process ended with status {child.returncode})"))


if __name__ == "__main__":
    main()
