"""The mesh ray queries (the ray kernels of csrc/meshbvh.hip; fit.MeshBVH.raycast / .visibility, MeshField(sign="visibility")) in one
run on one box, at the shapes of tools/meshbvh_bench.py: the sphere field extracted at 256^3 (about 154 k faces) and the raw
6.9 M-face export of the sample-like field (`--no-raw` skips it).  Event-timed, the mean of `--reps` calls after a warm-up call.
Per mesh: closest-hit rays per second for a 256 x 256 `compute_raydirs` camera (coherent rays) and for 10^6 incoherent rays (seeded
origins on a sphere about the mesh, aimed at seeded points inside its box), the same with any_hit.  On the sphere also: `visibility`
at a fit's 2048 x 512 voxel positions with limit = 1 and limit = 0 (64 directions), and the whole mesh_to_primitives(accel="bvh")
with sign="winding" against sign="visibility" - the comparison is the winding fit of this run, not a number from another box.

    python tools/meshray_bench.py [--reps 3] [--no-raw] [--directions 64]
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


def camera_rays(rm, R, dev):
    """The 256 x 256 camera of tools/raymarch_grad_bench.py, five volume radii away -> (origins, dirs) [R * R, 3]."""
    volradius = 1.0
    Rt = torch.tensor([[[1.0, 0, 0, 0], [0, -1.0, 0, 0], [0, 0, -1.0, 5 * volradius]]])
    Kc = torch.tensor([[[2084.95 * R / 1024, 0, R / 2], [0, 2084.95 * R / 1024, R / 2], [0, 0, 1]]])
    cam = rm.convert_camera_parameters(Rt, Kc)
    focal = torch.diagonal(cam["focal"], dim1=1, dim2=2).contiguous()
    _, rd, _ = rm.compute_raydirs(cam["campos"].to(dev), cam["camrot"].to(dev), focal.to(dev), cam["princpt"].to(dev),
                                  rm.base_pixel_coords(R, R, dev)[None].contiguous(), volradius)
    rd = rd.reshape(-1, 3).contiguous()
    return cam["campos"].to(dev).expand(rd.shape[0], 3).contiguous(), rd


def incoherent_rays(n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g)
    o = 3.0 * o / o.norm(dim=1, keepdim=True)
    target = torch.rand(n, 3, generator=g) * 1.8 - 0.9
    return o.to(dev).contiguous(), (target - o).to(dev).contiguous()


def rays(label, bvh, o, d, reps):
    n = o.shape[0]
    ms, (t, face, _, _) = timed(lambda: bvh.raycast(o, d), reps)
    ma, (_, fa, _, _) = timed(lambda: bvh.raycast(o, d, any_hit=True), reps)
    hits = int((face >= 0).sum())
    print(f"{label:44s} closest {ms:9.3f} ms  {n / ms / 1e3:8.1f} M rays/s   any_hit {ma:9.3f} ms  {n / ma / 1e3:8.1f} M rays/s   "
          f"{hits} of {n} hit, any_hit agrees: {bool(((fa >= 0) == (face >= 0)).all())}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-raw", action="store_true")
    ap.add_argument("--directions", type=int, default=64)
    a = ap.parse_args()
    __graft_entry__.build()
    from topia_xl_amd import fit
    from topia_xl_amd import mesh as M
    from topia_xl_amd import raymarch as rm

    dev = "cuda:0"
    P, S, N = 2048, 8, 65536
    cam_o, cam_d = camera_rays(rm, 256, dev)
    inc_o, inc_d = incoherent_rays(1_000_000, dev)

    m = M.extract_mesh(sphere_field(dev), resolution=256)
    v, _, _ = fit.normalize_vertices(m.v.float())
    f = m.f.int().contiguous()
    print(f"--- sphere: V = {v.shape[0]}  F = {f.shape[0]}", flush=True)
    bvh = fit.MeshBVH(v, f)
    rays("256 x 256 camera", bvh, cam_o, cam_d, a.reps)
    rays("10^6 incoherent rays", bvh, inc_o, inc_d, a.reps)
    cdf = fit.area_cdf(fit.face_areas(v, f))
    cand, _ = fit.surface_points(v, f, cdf, fit.surface_uniforms(N, 0).to(dev))
    idx, nn = fit.fps(cand, P, 0)
    x = (cand[idx.long()][:, None, :] + nn[:, None, None] * fit._local_grid(S, dev)[None]).reshape(-1, 3).contiguous()
    attr = torch.cat([m.albedo, m.roughness[:, None], m.metallic[:, None]], 1).float().contiguous()
    mq, q = timed(lambda: bvh.query(x, attr), a.reps)
    m1, e1 = timed(lambda: bvh.visibility(x, a.directions, limit=1), a.reps)
    m0, e0 = timed(lambda: bvh.visibility(x, a.directions), a.reps)
    inside_w, inside_v = q[2].abs() >= 0.5, e1 < 1
    print(f"query (dist, face, wn, C = 5), n = {x.shape[0]:9d} {mq:9.3f} ms", flush=True)
    print(f"visibility, {a.directions} directions, limit = 1             {m1:9.3f} ms", flush=True)
    print(f"visibility, {a.directions} directions, limit = 0             {m0:9.3f} ms   limit 1 == min(limit 0, 1): {bool((e0.clamp(max=1) == e1).all())}",
          flush=True)
    print(f"  inside by winding {int(inside_w.sum())}, by visibility {int(inside_v.sum())}, {int((inside_w != inside_v).sum())} of {x.shape[0]} signs "
          f"differ (|sdf| there at most {float(q[0][inside_w != inside_v].max()) if bool((inside_w != inside_v).any()) else 0.0:.2e})", flush=True)
    mesh = (m.v, m.f, m.albedo, m.roughness, m.metallic)
    reps = max(1, a.reps - 1)
    tw, (rw, _) = timed(lambda: fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S, accel="bvh"), reps)
    tv, (rv, _) = timed(lambda: fit.mesh_to_primitives(mesh, num_prims=P, prim_shape=S, accel="bvh", sign="visibility",
                                                       sign_directions=a.directions), reps)
    differ = int((rw[:, 4:4 + S ** 3] != rv[:, 4:4 + S ** 3]).sum())
    print(f"mesh_to_primitives(accel='bvh'), {P} x {S}^3      sign='winding' {tw:9.2f} ms   sign='visibility' {tv:9.2f} ms   x{tv / tw:5.2f}   "
          f"{differ} of {P * S ** 3} SDF values differ", flush=True)
    del bvh
    if not a.no_raw:
        m = M.extract_mesh(sample_field(dev), resolution=256)
        v, _, _ = fit.normalize_vertices(m.v.float())
        f = m.f.int().contiguous()
        print(f"--- raw export of the sample-like field: V = {v.shape[0]}  F = {f.shape[0]}", flush=True)
        bvh = fit.MeshBVH(v, f)
        rays("256 x 256 camera", bvh, cam_o, cam_d, a.reps)
        rays("10^6 incoherent rays", bvh, inc_o, inc_d, a.reps)


if __name__ == "__main__":
    main()
