"""Per-stage timing of the texture bake (csrc/texbake.hip, mesh.py) on the marching-cubes mesh of a 256^3 lattice, with
1024^2 and 2048^2 textures: labels + charts, host packing (+ the atlas arrays), the raster, compaction of the covered
texels, the fp32 field query, the quantize + fill, and the PNG / GLB write.  Two fields: a sphere of 96 primitives
(radius 0.5, the mesh tests' synthetic field) and a sample-like set of 2048 primitives posed the way
examples/generate.py poses a random-weight sample (scale 0.05-0.08, centres in [-0.6, 0.6]^3, random payload).  Each
stage is timed with a device synchronisation around it, median of --reps runs after one warm-up.

    python tools/texbake_bench.py [--reps 5] [--sizes 1024 2048] [--normal-map] [--occlusion]

--normal-map adds the rows of the tangent-space normal map (mesh.bake_normal_map, stage by stage): the field's gradient query
at the texel points, the tangents, the texel normals, the second fill, the GLB write with the third PNG, and the total of
`bake_textures(normal_map=True)` next to the plain one.  --occlusion adds the rows of the ambient occlusion, each on its own:
the SDF lattice (`field_lattice`; `extract_texmesh` reuses the one marching cubes read instead), the field normals, the
occlusion kernel (`texel_occlusion`, default arguments), the extra fill that carries it into R, and the totals of
`bake_textures(occlusion=True)` with the lattice handed over and computed.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402
from oracle.synth import sample_field, sphere_field  # noqa: E402,F401  (the mesh tests use the same two)


def stage(name, fn, times):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    times.setdefault(name, []).append((time.perf_counter() - t) * 1e3)
    return out


def bake_stages(M, field, mesh, size, times, normal_map=False, occlusion=False, resolution=256):
    """mesh.bake_textures, stage by stage (the same calls)."""
    v, f, n = mesh.v, mesh.f, mesh.normals
    nv, nf = v.shape[0], f.shape[0]

    def charts():
        lab = M.face_labels(v, f, n)
        return lab, M.face_components((f.long() * 6 + lab[:, None].long()).int(), 6 * nv)

    lab, (chart, nc) = stage("labels + charts", charts, times)
    atlas = stage("unwrap total (charts + pack + raster)", lambda: M.uv_unwrap(v, f, n, (size, size)), times)
    fid, cover, covered, doubly, _ = stage("raster", lambda: M.atlas_raster(atlas.uv_fixed, atlas.f, size, size), times)
    texel, pts = stage("compact", lambda: M.atlas_points(atlas, v, f), times)

    def query():
        attr = torch.empty(pts.shape[0], 6, device=v.device)
        for lo in range(0, pts.shape[0], 1 << 21):
            attr[lo:lo + (1 << 21)] = field.query(pts[lo:lo + (1 << 21)])
        return attr

    attr = stage("query", query, times)
    albedo, mr = stage("quantize + fill", lambda: M.fill_textures(attr, texel, atlas.face_id), times)
    tm = M.TexturedMesh(v=v[atlas.vmap], f=atlas.f, normals=n[atlas.vmap], vt=atlas.vt, vmap=atlas.vmap, albedo=albedo,
                        metallic_roughness=mr, covered=atlas.face_id >= 0)
    with tempfile.TemporaryDirectory() as d:
        stage("PNG + GLB write", lambda: tm.write_glb(os.path.join(d, "m.glb")), times)
    stage("bake_textures total", lambda: M.bake_textures(field, mesh, size), times)
    if normal_map:
        nv_ = n[atlas.vmap].contiguous()
        g = stage("normal map: gradient query", lambda: M.field_normals(field, pts), times)
        tan = stage("normal map: tangents", lambda: M.atlas_tangents(atlas, nv_), times)
        _, nattr = stage("normal map: texel normals", lambda: M.texel_normals(atlas, texel, nv_, tan, g, with_attr=True), times)
        nmap, _ = stage("normal map: fill", lambda: M.fill_textures(nattr, texel, atlas.face_id), times)
        tm.tangents, tm.normal_map = tan, nmap
        with tempfile.TemporaryDirectory() as d:
            stage("normal map: GLB write with 3 PNGs", lambda: tm.write_glb(os.path.join(d, "m.glb")), times)
        stage("bake_textures(normal_map=True) total", lambda: M.bake_textures(field, mesh, size, normal_map=True), times)
    if occlusion:
        lattice = stage("occlusion: lattice (reused by extract_texmesh)", lambda: M.field_lattice(field, resolution), times)
        g = stage("occlusion: field normals", lambda: M.field_normals(field, pts), times)
        dirs = M.occlusion_directions().to(v.device)
        ao = stage("occlusion: kernel", lambda: M.texel_occlusion(lattice, pts, g, dirs), times)
        stage("occlusion: quantize + fill with the extra fill", lambda: M.fill_textures(attr, texel, atlas.face_id, occlusion=ao), times)
        stage("bake_textures(occlusion=True, lattice=) total", lambda: M.bake_textures(field, mesh, size, occlusion=True, lattice=lattice),
              times)
        stage("bake_textures(occlusion=True) total, own lattice",
              lambda: M.bake_textures(field, mesh, size, occlusion=True, occlusion_resolution=resolution), times)
    return atlas, nc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--normal-map", action="store_true", help="also time the stages of the tangent-space normal map")
    ap.add_argument("--occlusion", action="store_true", help="also time the stages of the ambient occlusion bake")
    a = ap.parse_args()
    __graft_entry__.build()
    from topia_xl_amd import mesh as M

    dev = "cuda:0"
    for fname, make in (("sphere", sphere_field), ("sample", sample_field)):
        field = make(dev)
        mesh = M.extract_mesh(field, resolution=a.resolution)
        for size in a.sizes:
            times = {}
            try:
                M.uv_unwrap(mesh.v, mesh.f, mesh.normals, (size, size))
            except ValueError as e:   # more charts than minimum-size rectangles fit the atlas
                lab = M.face_labels(mesh.v, mesh.f, mesh.normals)
                nc = M.face_components((mesh.f.long() * 6 + lab[:, None].long()).int(), 6 * mesh.v.shape[0])[1]
                print(f"{fname} {a.resolution}^3 -> {size}^2: F = {mesh.f.shape[0]}, charts {nc}: not baked ({e})", flush=True)
                continue
            for rep in range(a.reps + 1):
                t = {}
                atlas, nc = bake_stages(M, field, mesh, size, t, a.normal_map, a.occlusion, a.resolution)
                if rep:
                    for k, x in t.items():
                        times.setdefault(k, []).extend(x)
            med = {k: statistics.median(x) for k, x in times.items()}
            pack = med["unwrap total (charts + pack + raster)"] - med["labels + charts"] - med["raster"] * (1 + atlas.split_rounds)
            sizes = np.sort(np.bincount(atlas.chart.cpu().numpy()))[::-1]
            print(f"{fname} {a.resolution}^3 -> {size}^2: F = {mesh.f.shape[0]}, V' = {atlas.vt.shape[0]}, charts {nc} "
                  f"(largest six hold {sizes[:6].sum() / max(1, sizes.sum()):.4f} of the faces), final charts {atlas.n_charts}, "
                  f"split rounds {atlas.split_rounds}, covered texels {atlas.n_covered} ({atlas.coverage:.3f}), "
                  f"scale {atlas.scale:.1f} texels / unit", flush=True)
            for k, x in med.items():
                print(f"    {k:48s} {x:9.2f} ms", flush=True)
            print(f"    {'host packing + atlas arrays (derived)':48s} {pack:9.2f} ms", flush=True)


if __name__ == "__main__":
    main()
