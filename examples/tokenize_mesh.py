"""Turn a mesh into PrimX primitives (and, with checkpoints, into the DiT's tokens), then back into a mesh.

  PLY (as TriMesh.write_ply writes it) -> read_ply -> mesh_to_primitives (surface samples, farthest point sampling,
        scale = nearest-centre distance, payload = the mesh's signed distance / colour / material per voxel)
        -> PrimSDF -> extract_mesh -> PLY            [-> primitives_to_latents with --vae: the 68-channel tokens]

--mesh takes a .ply or a .glb (glTF 2.0 binary: UVs, textures, material factors, several materials, node transforms - what
`mesh.read_glb` documents); a GLB is fitted from its textures (`primx_material_sample` at the closest surface point of every
voxel) and comes back as a textured GLB: `extract_texmesh` -> `TexturedMesh.write_glb`.  Without --mesh a coloured torus is
written first and read back, so the run is end to end on a written PLY, and the loop is then closed on a GLB as well: the fitted
torus is extracted as a textured GLB, that file is read back with `read_glb` and fitted again.  The fit is the
initialisation the 3DTopia-XL paper describes; --refine N follows it with N steps of gradient refinement against the mesh's own
field and reports the field error at the surface candidates before and after; --metrics prints the round trip's Chamfer distance, F-score, Hausdorff
distance and normal consistency (`metrics.compare_to_field`: the mesh extracted from the fitted field against the input's exact
surface).  Without --vae the encoder carries
random weights (the tokens are then noise: the point is the data flow and the per-stage timing).  (The file is not called
tokenize.py: a script directory is searched for modules first, and that name would replace the standard library's `tokenize`
for every script in examples/.)

    python examples/tokenize_mesh.py [--mesh IN.ply | IN.glb] [--out OUT.ply] [--prims 2048] [--refine N] [--resolution 256] [--normal-map] [--occlusion] [--metrics] [--vae VAE.pt] [--denoised OUT.pt]
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402


def torus(nu=192, nv=96, R=0.6, r=0.25):
    """A closed, outward-oriented torus with smooth vertex colours: (v, f, normals, albedo, roughness, metallic), CPU tensors."""
    u = torch.arange(nu, dtype=torch.float32) * (2 * math.pi / nu)
    w = torch.arange(nv, dtype=torch.float32) * (2 * math.pi / nv)
    uu, ww = torch.meshgrid(u, w, indexing="ij")
    n = torch.stack([ww.cos() * uu.cos(), ww.cos() * uu.sin(), ww.sin()], -1).reshape(-1, 3)
    c = torch.stack([R * uu.cos(), R * uu.sin(), torch.zeros_like(uu)], -1).reshape(-1, 3)
    v = c + r * n
    i, j = torch.meshgrid(torch.arange(nu), torch.arange(nv), indexing="ij")
    a, b, cc, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
    f = torch.cat([torch.stack([a, b, cc], -1).reshape(-1, 3), torch.stack([a, cc, d], -1).reshape(-1, 3)]).int()
    alb = torch.stack([0.5 + 0.5 * uu.cos(), 0.5 + 0.5 * ww.sin(), 0.5 + 0.5 * (uu + ww).sin()], -1).reshape(-1, 3)
    return v, f, n, (alb * 255).round() / 255, (0.3 + 0.4 * ww.cos().abs()).reshape(-1), (0.5 + 0.5 * uu.sin()).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", "--ply", dest="ply", default=None,
                    help="input mesh: a binary PLY as TriMesh.write_ply writes it, or a glTF 2.0 .glb; a torus when absent")
    ap.add_argument("--texture-size", type=int, default=1024, help="texture size of the GLBs written")
    ap.add_argument("--normal-map", action="store_true", help="bake a tangent-space normal map of the field into the GLBs written")
    ap.add_argument("--occlusion", action="store_true", help="bake ambient occlusion from the SDF lattice into R of the metallic-roughness "
                    "image of the GLBs written (occlusionTexture)")
    ap.add_argument("--metrics", action="store_true", help="print the round trip's quality metrics (metrics.compare_to_field, surface=True)")
    ap.add_argument("--out", default="tokenized.ply", help="the mesh extracted from the fitted primitives")
    ap.add_argument("--denoised", default=None, help="also save the primitives as a denoised.pt")
    ap.add_argument("--prims", type=int, default=2048)
    ap.add_argument("--refine", type=int, default=0, help="refinement steps after the initialisation (fit.refine_primitives)")
    ap.add_argument("--accel", choices=["bvh"], default=None,
                    help="answer the mesh's field queries through a BVH (fit.MeshBVH) instead of brute force over the faces")
    ap.add_argument("--sign", choices=["winding", "visibility"], default="winding",
                    help="inside / outside from the winding number, or (with --accel bvh) from rays through the BVH: for meshes "
                    "whose faces are not oriented consistently (fit.MeshField)")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--vae", default=None, help="VAE checkpoint (.pt with 'model_state_dict'); random weights when absent")
    ap.add_argument("--no-encode", action="store_true", help="skip primitives_to_latents")
    a = ap.parse_args()
    __graft_entry__.build()
    import topia_xl_amd as pkg
    from topia_xl_amd import mesh as M
    from topia_xl_amd import pipeline
    from topia_xl_amd.primsdf import PrimSDF

    dev = "cuda:0"

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        print(f"{name:52s} {1e3 * (time.perf_counter() - t0):9.2f} ms", flush=True)
        return r

    path = a.ply
    if path is None:
        path = os.path.splitext(a.out)[0] + "_input.ply"
        M.TriMesh(*torus()).write_ply(path)
        print("wrote the input torus ->", path)
    is_glb = path.lower().endswith(".glb")
    if is_glb:
        mesh = timed("read_glb", lambda: pipeline.read_glb(path, device=dev))
        print(f"  {mesh.mat_factor.shape[0]} materials, {mesh.tex_image.shape[0]} textures, images "
              + ", ".join(f"{i.shape[1]}x{i.shape[0]}" for i in mesh.images))
    else:
        mesh = timed("read_ply", lambda: pipeline.read_ply(path, device=dev))
    print(f"  V = {mesh.v.shape[0]}  F = {mesh.f.shape[0]}")
    timed("mesh_to_primitives (first call)", lambda: pipeline.mesh_to_primitives(mesh, num_prims=a.prims, seed=a.seed, accel=a.accel, sign=a.sign))
    recon, info = timed("mesh_to_primitives" + (f" (accel={a.accel})" if a.accel else ""),
                        lambda: pipeline.mesh_to_primitives(mesh, num_prims=a.prims, seed=a.seed, accel=a.accel, sign=a.sign))
    print(f"  recon_param {tuple(recon.shape)}  scale {float(recon[:, 0].min()):.4f} .. {float(recon[:, 0].max()):.4f}  "
          f"normalised by x{float(info['scale']):.4f}")

    def as_field(r):
        m = PrimSDF(num_prims=r.shape[0], dim_feat=6, prim_shape=8)
        m.srt_param = torch.nn.Parameter(r[:, :4].contiguous(), requires_grad=False)
        m.feat_param = torch.nn.Parameter(r[:, 4:].contiguous(), requires_grad=False)
        return m.to(dev).eval()

    def report(m, what):
        # how well the primitives hold the mesh: the fitted field at the surface candidates, where the mesh's own SDF is 0
        with torch.no_grad():
            s = m(info["candidates"])["sdf"][:, 0]
        print(f"  {what} |sdf| at the {s.shape[0]} surface candidates: mean {float(s.abs().mean()):.2e}  max {float(s.abs().max()):.2e}")

    field = as_field(recon)
    report(field, "fitted")
    if a.refine > 0:
        from topia_xl_amd import fit
        target = fit.MeshField(info["v"], info["f"], material=mesh, accel=a.accel, sign=a.sign) if is_glb else \
            fit.MeshField(info["v"], info["f"], info["attr"], accel=a.accel, sign=a.sign)
        fit.refine_primitives(recon, target, 1)                                       # (first call: loads the kernels)
        recon, rinfo = timed(f"refine_primitives, {a.refine} steps", lambda: fit.refine_primitives(recon, target, a.refine))
        print(f"  loss {rinfo['loss'][0]:.3e} -> {rinfo['loss'][-1]:.3e}")
        field = as_field(recon)
        report(field, "refined")
    glb_out = os.path.splitext(a.out)[0] + ".glb"
    if is_glb:
        tex = timed(f"extract_texmesh {a.resolution}^3, {a.texture_size}^2", lambda: M.extract_texmesh(field, a.resolution, a.texture_size, normal_map=a.normal_map, occlusion=a.occlusion))
        print(f"  V = {tex.v.shape[0]}  F = {tex.f.shape[0]}")
        tex.write_glb(glb_out)
        print("extracted textured mesh ->", glb_out)
    else:
        out = timed(f"extract_mesh {a.resolution}^3", lambda: M.extract_mesh(field, resolution=a.resolution))
        print(f"  V = {out.v.shape[0]}  F = {out.f.shape[0]}")
        out.write_ply(a.out)
        print("extracted mesh ->", a.out)
    if a.metrics:
        from topia_xl_amd import metrics
        rt = timed(f"compare_to_field {a.resolution}^3, surface=True", lambda: metrics.compare_to_field((info["v"], info["f"]), field, a.resolution, surface=True))
        print("  round trip:", rt)
    if a.ply is None:
        # close the loop on this project's own textured GLB: tokens -> GLB -> read_glb -> tokens
        tex = timed(f"extract_texmesh {a.resolution}^3, {a.texture_size}^2", lambda: M.extract_texmesh(field, a.resolution, a.texture_size, normal_map=a.normal_map, occlusion=a.occlusion))
        tex.write_glb(glb_out)
        back = timed("read_glb (the GLB just written)", lambda: pipeline.read_glb(glb_out, device=dev))
        print(f"  V = {back.v.shape[0]}  F = {back.f.shape[0]}  images " + ", ".join(f"{i.shape[1]}x{i.shape[0]}" for i in back.images))
        recon2, info2 = timed("mesh_to_primitives (textured GLB)",
                              lambda: pipeline.mesh_to_primitives(back, num_prims=a.prims, seed=a.seed))
        info = info2
        report(as_field(recon2), "refitted from the GLB:")
        with torch.no_grad():
            q = field(info2["candidates"] / info2["scale"] + info2["center"])
            c2 = as_field(recon2)(info2["candidates"])
        d = (torch.cat([c2["tex"], c2["mat"]], 1) - torch.cat([q["tex"], q["mat"]], 1)).abs()
        print(f"  colour / material of the refit against the first fit at its surface candidates: mean {float(d.mean()):.3e}  max {float(d.max()):.3e}")
    if not a.no_encode:
        vae = pkg.VAE(in_channels=6, latent_channels=1, out_channels=6, down_channels=[32, 256], mid_attention=True,
                      up_channels=[256, 32], layers_per_block=2)
        if a.vae is None:
            g = torch.Generator().manual_seed(7)
            with torch.no_grad():
                for name, p in vae.named_parameters():
                    if p.dim() > 1:
                        p.copy_(torch.randn(p.shape, generator=g) * p[0].numel() ** -0.5)
                    elif "norm" in name and name.endswith("weight"):
                        p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
                    else:
                        p.copy_(0.05 * torch.randn(p.shape, generator=g))
        pipeline.load_checkpoints(None, vae, None, a.vae)
        vae.eval().to(dev)
        mean, std = [0.0] * 68, [1.0] * 68      # the shipped configuration carries its own per-channel statistics
        timed("primitives_to_latents (first call)", lambda: pipeline.primitives_to_latents(recon[None], vae, mean, std))
        tokens = timed("primitives_to_latents", lambda: pipeline.primitives_to_latents(recon[None], vae, mean, std))
        print(f"  tokens {tuple(tokens.shape)}" + ("" if a.vae else "  (random encoder weights)"))
    if a.denoised:
        pipeline.save_denoised(a.denoised, recon[None])
        print("primitives ->", a.denoised)


if __name__ == "__main__":
    main()
