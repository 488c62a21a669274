"""Timing of primitive fitting (csrc/meshfield.hip, fit.py) at P = 2048 primitives of 8^3 voxels from 65536 candidates, on the
two meshes of tools/meshdecim_bench.py: the sphere field extracted at 256^3 (about 154 k faces) and the cleaned sample-like
mesh (about 125 k faces).  Per kernel (event-timed after a warm-up call; every call includes its own index-check readback):
primx_mesh_face_areas, the host-side float64 inclusive sum, primx_mesh_surface_points, primx_fps, primx_mesh_field_query at the
2048 x 512 voxel positions; and the whole mesh_to_primitives.  The query line also gives the point-triangle pairs per second
and the share of DESIGN.md's arithmetic floor.

    python tools/fit_bench.py [--reps 3] [--only sphere sample]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402
from oracle.synth import sample_field, sphere_field  # noqa: E402  (the fields of the mesh benchmarks and tests)

LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9      # 256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", nargs="+", default=["sphere", "sample"])
    ap.add_argument("--valu-per-pair", type=float, default=270.0,
                    help="VALU instructions per point-triangle pair (counted in the kernel's ISA: DESIGN.md) for the floor")
    a = ap.parse_args()
    __graft_entry__.build()
    from topia_xl_amd import fit
    from topia_xl_amd import mesh as M

    dev = "cuda:0"
    P, S, N = 2048, 8, 65536
    for name in a.only:
        field = {"sphere": sphere_field, "sample": sample_field}[name](dev)
        m = M.extract_mesh(field, resolution=256)
        if name == "sample":
            m = M.clean_trimesh(m, **M.CLEAN_ARGS)
        V, F = m.v.shape[0], m.f.shape[0]
        print(f"--- {name}: V = {V}  F = {F}", flush=True)
        v, _, _ = fit.normalize_vertices(m.v.float())
        f = m.f.int().contiguous()
        attr = torch.cat([m.albedo, m.roughness[:, None], m.metallic[:, None]], 1).float().contiguous()
        ms, area = timed(lambda: fit.face_areas(v, f), a.reps)
        print(f"primx_mesh_face_areas            {ms:10.3f} ms")
        t0 = time.perf_counter()
        cdf = fit.area_cdf(area)
        torch.cuda.synchronize()
        print(f"float64 inclusive sum on the host {1e3 * (time.perf_counter() - t0):9.3f} ms (with both copies)")
        u = fit.surface_uniforms(N, 0).to(dev)
        ms, (cand, _) = timed(lambda: fit.surface_points(v, f, cdf, u), a.reps)
        print(f"primx_mesh_surface_points N={N} {ms:10.3f} ms")
        ms, (idx, nn) = timed(lambda: fit.fps(cand, P, 0), a.reps)
        print(f"primx_fps {P} of {N}           {ms:10.3f} ms  ({1e3 * ms / P:.2f} us per centre)")
        x = (cand[idx.long()][:, None, :] + nn[:, None, None] * fit._local_grid(S, dev)[None]).reshape(-1, 3).contiguous()
        ms, _ = timed(lambda: fit.mesh_field_query(x, v, f, attr), a.reps)
        pairs = x.shape[0] * F
        line = f"primx_mesh_field_query n={x.shape[0]} {ms:10.2f} ms  {pairs / ms / 1e6:8.1f} G pairs/s"
        if a.valu_per_pair > 0:
            floor = pairs * a.valu_per_pair / LANE_OPS_PER_S * 1e3
            line += f"  floor {floor:.1f} ms at {a.valu_per_pair:.0f} VALU/pair and 2.4 GHz = {100 * floor / ms:.0f} % of it"
        print(line, flush=True)
        mesh = (m.v, m.f, m.albedo, m.roughness, m.metallic)
        ms, (recon, _) = timed(lambda: fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S), max(1, a.reps - 1))
        print(f"mesh_to_primitives (whole call)  {ms:10.2f} ms  recon_param {tuple(recon.shape)}", flush=True)


if __name__ == "__main__":
    main()
