"""The mesh BVH (csrc/meshbvh.hip, fit.MeshBVH) against the brute-force field query in the same run on the same box, at the shapes
of tools/fit_bench.py: the sphere field extracted at 256^3 (about 154 k faces) and the cleaned sample-like mesh (about 125 k
faces).  Event-timed, the mean of `--reps` calls after a warm-up call.  Per mesh: the build (both passes and torch's sort), the
query at the 2048 x 512 voxel positions of a fit (brute force, tree, tree with sorted points; the outputs are compared bit for
bit, the signs counted), the whole mesh_to_primitives, 20 refinement steps, compare_meshes(surface=True).  Then one query of 10^5
surface samples of the sphere against the raw 6.9 M-face export of the sample-like field (`--no-raw` skips it).

    python tools/meshbvh_bench.py [--reps 3] [--only sphere sample] [--no-raw] [--beta 2.0]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402
from oracle.synth import sample_field, sphere_field  # noqa: E402  (the fields of the mesh benchmarks and tests)


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


def both(label, brute, fast, reps):
    """-> (brute result, fast result); prints both times and the factor."""
    tb, rb = timed(brute, reps)
    tf, rf = timed(fast, reps)
    print(f"{label:44s} brute force {tb:10.2f} ms   bvh {tf:9.2f} ms   x{tb / tf:7.1f}", flush=True)
    return rb, rf


def same(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", nargs="+", default=["sphere", "sample"])
    ap.add_argument("--no-raw", action="store_true")
    ap.add_argument("--beta", type=float, default=2.0)
    a = ap.parse_args()
    __graft_entry__.build()
    from topia_xl_amd import fit, metrics
    from topia_xl_amd import mesh as M

    dev = "cuda:0"
    P, S, N = 2048, 8, 65536
    sphere_samples = None
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
        ms, bvh = timed(lambda: fit.MeshBVH(v, f), a.reps)
        print(f"MeshBVH(v, f): both passes and the sort          {ms:10.3f} ms   ({bvh.ws.numel() / F:.0f} bytes per face)", flush=True)
        cdf = fit.area_cdf(fit.face_areas(v, f))
        cand, _ = fit.surface_points(v, f, cdf, fit.surface_uniforms(N, 0).to(dev))
        idx, nn = fit.fps(cand, P, 0)
        x = (cand[idx.long()][:, None, :] + nn[:, None, None] * fit._local_grid(S, dev)[None]).reshape(-1, 3).contiguous()
        rb, rf = both(f"query, n = {x.shape[0]}, C = 5", lambda: fit.mesh_field_query(x, v, f, attr),
                      lambda: bvh.query(x, attr, a.beta), a.reps)
        ts, rs = timed(lambda: bvh.query(x, attr, a.beta, sort_points=True), a.reps)
        print(f"{'  the same with sort_points=True':44s} {'':25s} bvh {ts:9.2f} ms", flush=True)
        flips = int(((rb[2].abs() >= 0.5) != (rf[2].abs() >= 0.5)).sum())
        print(f"  dist / face / attr bit-identical: {same(rb[0], rf[0])} / {same(rb[1], rf[1])} / {same(rb[3], rf[3])}; sorted: "
              f"{all(same(p, q) for p, q in zip(rf, rs))}; max |wn - brute force wn| {float((rb[2] - rf[2]).abs().max()):.4f}; "
              f"{flips} of {x.shape[0]} signs differ", flush=True)
        mesh = (m.v, m.f, m.albedo, m.roughness, m.metallic)
        (recon, _), (recon_f, _) = both(f"mesh_to_primitives, {P} x {S}^3",
                                        lambda: fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S),
                                        lambda: fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S, accel="bvh", beta=a.beta),
                                        max(1, a.reps - 1))
        print(f"  recon_param bit-identical: {same(recon, recon_f)}", flush=True)
        fields = fit.MeshField(v, f, attr), fit.MeshField(v, f, attr, accel="bvh", beta=a.beta)
        both("refine_primitives, 20 steps", lambda: fit.refine_primitives(recon, fields[0], 20),
             lambda: fit.refine_primitives(recon, fields[1], 20), max(1, a.reps - 1))
        other = (v * 1.01, f)
        db, df = both("compare_meshes(surface=True), 10^5 samples", lambda: metrics.compare_meshes((v, f), other, surface=True),
                      lambda: metrics.compare_meshes((v, f), other, surface=True, accel="bvh"), a.reps)
        print(f"  the same dict: {db == df}", flush=True)
        if name == "sphere":
            sphere_samples = metrics.sample_surface((v, f), 100_000, 0)[0]
        del bvh, fields
    if not a.no_raw:
        m = M.extract_mesh(sample_field(dev), resolution=256)
        v, _, _ = fit.normalize_vertices(m.v.float())
        f = m.f.int().contiguous()
        print(f"--- raw export of the sample-like field: V = {v.shape[0]}  F = {f.shape[0]}", flush=True)
        x = sphere_samples if sphere_samples is not None else metrics.sample_surface((v, f), 100_000, 0)[0]
        ms, bvh = timed(lambda: fit.MeshBVH(v, f), 1)
        print(f"MeshBVH(v, f): both passes and the sort          {ms:10.3f} ms", flush=True)
        rb, rf = both("query, n = 100000, C = 0", lambda: fit.mesh_field_query(x, v, f), lambda: bvh.query(x, None, a.beta, sort_points=True), 1)
        print(f"  dist / face bit-identical: {same(rb[0], rf[0])} / {same(rb[1], rf[1])}", flush=True)


if __name__ == "__main__":
    main()
