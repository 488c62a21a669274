"""Timing of mesh export (csrc/mcubes.hip, mesh.py): marching_cubes at 128^3 / 256^3 / 512^3 on the PrimSDF lattice of
2048 synthetic primitives (the primsdf_bench.py set), each call including its one count readback and the output
allocation, and the whole extract_mesh (noise filter + 256^3 lattice query + marching cubes + attribute query) at 256^3.
Event-timed after warm-up.  Effective GB/s = the lattice bytes (4 R^3) over the call time.

    python tools/mesh_bench.py [--reps 20]
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
    from topia_xl_amd.mesh import extract_mesh, lattice_points, marching_cubes
    from topia_xl_amd.primsdf import PrimSDF

    dev = "cuda:0"
    gen = torch.Generator().manual_seed(5)
    P, S = 2048, 8
    m = PrimSDF(num_prims=P, prim_shape=S).eval()
    m.srt_param.data = torch.cat([0.03 + 0.05 * torch.rand(P, 1, generator=gen), 1.6 * torch.rand(P, 3, generator=gen) - 0.8], dim=1)
    m.feat_param.data = torch.randn(P, 6 * S ** 3, generator=gen) * 0.5 + 0.3
    m.to(dev)
    for R in (128, 256, 512):
        pts = lattice_points(R, dev)
        grid = torch.empty(pts.shape[0], device=dev)
        for lo in range(0, pts.shape[0], 1 << 21):
            grid[lo:lo + (1 << 21)] = m.query(pts[lo:lo + (1 << 21)])[:, 0]
        del pts
        grid = grid.reshape(R, R, R)
        ms, (v, f) = timed(lambda: marching_cubes(grid, 0.0), a.reps)
        msn, _ = timed(lambda: marching_cubes(grid, 0.0, return_normals=True), a.reps)
        print(f"marching_cubes {R}^3: {ms:8.3f} ms ({msn:8.3f} ms with normals)  V = {v.shape[0]:9d}  F = {f.shape[0]:9d}  "
              f"lattice {4 * R ** 3 / ms / 1e6:7.1f} GB/s", flush=True)
        del grid
    ms, mesh = timed(lambda: extract_mesh(m, resolution=256), max(3, a.reps // 4))
    print(f"extract_mesh 256^3 (filter + lattice query + marching cubes + attributes): {ms:8.2f} ms  V = {mesh.v.shape[0]}  "
          f"F = {mesh.f.shape[0]}", flush=True)


if __name__ == "__main__":
    main()
