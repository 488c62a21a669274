"""What the README called unmeasured, measured with metrics.py on the synthetic assets the other tools use: Chamfer distance,
F-score and Hausdorff distance (each side's 100 000 samples against the other mesh's exact surface, `surface=True`) of

  * the round trip mesh -> primitives -> mesh of examples/tokenize_mesh.py's torus (36864 faces, 2048 primitives of 8^3 voxels,
    extracted at 256^3) at refine = 0 and refine = 20;
  * the decimation of the sphere field's 256^3 mesh (about 154 k faces) to 100 000 faces, against the undecimated mesh;
  * `clean=True` on the same mesh, against the uncleaned one.

Units: PrimSDF's [-1, 1]^3 domain (one cell of the 256^3 lattice is 2 / 255 = 7.8e-3).  One line per case, then one JSON line.

    python tools/quality_report.py [--samples 100000] [--resolution 256] [--refine 0 20]
"""
import argparse
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import __graft_entry__  # noqa: E402


def _torus():
    spec = importlib.util.spec_from_file_location("tokenize_mesh_example", os.path.join(ROOT, "examples", "tokenize_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.torus()


def line(name, r):
    f = "  ".join(f"F[{t:g}] {v:.4f}" for t, v in r["fscore"].items())
    print(f"{name:46s} chamfer_l1 {r['chamfer_l1']:.3e}  chamfer_l2 {r['chamfer_l2']:.3e}  accuracy {r['accuracy']:.3e}  completeness "
          f"{r['completeness']:.3e}  hausdorff {r['hausdorff']:.3e}  {f}  normal_consistency {r['normal_consistency']:.5f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--refine", type=int, nargs="+", default=[0, 20])
    a = ap.parse_args()
    __graft_entry__.build()
    from oracle.synth import sphere_field
    from topia_xl_amd import mesh as M
    from topia_xl_amd import metrics, pipeline

    dev = "cuda:0"
    kw = dict(n=a.samples, surface=True)
    out = {}
    v, f, _, alb, rough, metal = (t.to(dev) for t in _torus())
    for steps in a.refine:
        recon, info = pipeline.mesh_to_primitives((v, f, alb, rough, metal), num_prims=2048, refine=steps)
        name = f"torus round trip, refine={steps}"
        out[name] = pipeline.primitives_vs_mesh(recon, (info["v"], info["f"]), a.resolution, **kw)
        line(name, out[name])
    field = sphere_field(dev)
    full = M.extract_mesh(field, a.resolution)
    for name, opt in (("decimated to 100000 faces", dict(decimate=100_000)), ("clean=True", dict(clean=True))):
        m = M.extract_mesh(field, a.resolution, **opt)
        name = f"sphere {full.f.shape[0]} faces, {name} ({m.f.shape[0]})"
        out[name] = metrics.compare_meshes(full, m, **kw)
        line(name, out[name])
    print(json.dumps({k: {**r, **{q: {str(t): x for t, x in r[q].items()} for q in ("precision", "recall", "fscore")}} for k, r in out.items()}))


if __name__ == "__main__":
    main()
