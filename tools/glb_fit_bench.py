"""Timing of a textured fit (csrc/material.hip, fit.py, gltf.py): P = 2048 primitives of 8^3 voxels fitted to a textured mesh with
2048^2 textures - the sphere field of the mesh benchmarks extracted at 256^3 (about 154 k faces), baked by `extract_texmesh`,
written with `TexturedMesh.write_glb` and read back with `read_glb`.

Reported: the host side (`read_glb` with both PNGs decoded, the construction of `MeshField(..., material=)` = the one upload of the
tables and the texel blob), then `primx_mesh_field_query` (C = 8: [vt | color | rm]) and `primx_material_sample` at the 2048 x 512
= 1048576 voxel positions, event-timed in ALTERNATING launches after a warm-up of both (every call includes its own index-check
read-back), with the spread over the repetitions; the sampler's minimum traffic (56 bytes per point plus 8 texels of 4 bytes for the
two LINEAR lookups) over its time; and the whole `mesh_to_primitives`.

    python tools/glb_fit_bench.py [--reps 5] [--texture-size 2048] [--resolution 256]
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402
from oracle.synth import sphere_field  # noqa: E402  (the field of the mesh benchmarks and tests)


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e), out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def spread(xs):
    xs = sorted(xs)
    return f"median {xs[len(xs) // 2]:10.3f} ms  (min {xs[0]:.3f}, max {xs[-1]:.3f}, {len(xs)} runs)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--texture-size", type=int, default=2048)
    ap.add_argument("--resolution", type=int, default=256)
    a = ap.parse_args()
    __graft_entry__.build()
    from topia_xl_amd import fit
    from topia_xl_amd import mesh as M

    dev = "cuda:0"
    P, S, N = 2048, 8, 65536
    tex = M.extract_texmesh(sphere_field(dev), a.resolution, a.texture_size)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.glb")
        tex.write_glb(path)
        size = os.path.getsize(path)
        ms, mm = host_ms(lambda: M.read_glb(path, device=dev))
    print(f"--- textured sphere: V = {mm.v.shape[0]}  F = {mm.f.shape[0]}  images "
          + ", ".join(f"{i.shape[1]}x{i.shape[0]}" for i in mm.images) + f"  ({size / 2 ** 20:.1f} MiB GLB)", flush=True)
    print(f"read_glb (host: parse, inflate, unfilter, upload) {ms:10.1f} ms")
    v, _, _ = fit.normalize_vertices(mm.v.float())
    f = mm.f.int().contiguous()
    ms, field = host_ms(lambda: fit.MeshField(v, f, material=mm))
    print(f"MeshField(..., material=): tables and texel blob   {ms:10.1f} ms  ({field.material[4].numel() / 2 ** 20:.0f} MiB of texels)")
    cdf = fit.area_cdf(fit.face_areas(v, f))
    cand, _ = fit.surface_points(v, f, cdf, fit.surface_uniforms(N, 0).to(dev))
    idx, nn = fit.fps(cand, P, 0)
    x = (cand[idx.long()][:, None, :] + nn[:, None, None] * fit._local_grid(S, dev)[None]).reshape(-1, 3).contiguous()
    n = x.shape[0]
    _, _, _, at = fit.mesh_field_query(x, field.v, field.f, field.attr)                       # warm-up of both kernels
    _, face, _, at = fit.mesh_field_query(x, field.v, field.f, field.attr)
    uv, va = at[:, 0:2].contiguous(), at[:, 2:8].contiguous()
    fit.material_sample(uv, va, face, *field.material)
    tq, ts = [], []
    for _ in range(a.reps):                                                                     # alternating launches
        tq.append(event_ms(lambda: fit.mesh_field_query(x, field.v, field.f, field.attr))[0])
        ts.append(event_ms(lambda: fit.material_sample(uv, va, face, *field.material))[0])
    mid = sorted(ts)[len(ts) // 2]
    traffic = n * (56 + 2 * 4 * 4)
    print(f"primx_mesh_field_query  n={n} F={f.shape[0]} C=8   {spread(tq)}")
    print(f"primx_material_sample   n={n}                 {spread(ts)}  >= {traffic / 2 ** 20:.0f} MiB moved = "
          f"{traffic / (mid * 1e-3) / 1e12:.2f} TB/s; {100 * mid / sorted(tq)[len(tq) // 2]:.3f} % of the query")
    tw = [host_ms(lambda: fit.mesh_to_primitives(mm, num_prims=P, prim_shape=S))[0] for _ in range(max(2, a.reps - 2))]
    print(f"mesh_to_primitives(MaterialMesh), whole call       {spread(tw)}", flush=True)


if __name__ == "__main__":
    main()
