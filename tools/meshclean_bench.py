"""Mesh cleanup (csrc/meshclean.hip, mesh.clean_mesh) with inference.py:126's arguments on the marching-cubes meshes of
tools/texbake_bench.py's two fields (a sphere of 96 primitives and a sample-like set of 2048) at 128^3 and 256^3 (and
512^3 with --resolutions): V and F before and after, the components removed, the non-manifold edges and vertices
repaired, the merge rounds, and the time of clean_mesh (HIP events around the call, readbacks included; median of
--reps runs after one warm-up).  For the sample-like field also the chart count before and after, and whether the
texture bake at --size^2 now succeeds.  Per-kernel times: run this under rocprofv3 --kernel-trace --stats.

    python tools/meshclean_bench.py [--reps 5] [--resolutions 128 256] [--size 1024]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402
from texbake_bench import sample_field, sphere_field  # noqa: E402

KW = dict(v_pct=1.0, min_f=8, min_d=5, repair=True)


def charts(M, v, f, n):
    lab = M.face_labels(v, f, n)
    return M.face_components((f.long() * 6 + lab[:, None].long()).int(), 6 * v.shape[0])[1] if f.shape[0] else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--size", type=int, default=1024)
    a = ap.parse_args()
    __graft_entry__.build()
    from topia_xl_amd import mesh as M

    dev = "cuda:0"
    for fname, make in (("sphere", sphere_field), ("sample", sample_field)):
        field = make(dev)
        for R in a.resolutions:
            raw = M.extract_mesh(field, resolution=R)
            times, st = [], {}
            for rep in range(a.reps + 1):
                st = {}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                v, f, vmap = M.clean_mesh(raw.v, raw.f, return_vmap=True, stats=st, **KW)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times.append(e0.elapsed_time(e1))
            print(f"{fname} {R}^3: V {raw.v.shape[0]} -> {v.shape[0]}, F {raw.f.shape[0]} -> {f.shape[0]}; "
                  f"r = {st['radius']:.5f}, merge rounds {st['merge_rounds']}, faces after merge {st['faces_after_merge']}, "
                  f"components {st['components']} (removed {st['components_removed']}), non-manifold candidates "
                  f"{st['nonmanifold_candidates']} (faces removed {st['nonmanifold_faces_removed']}), vertices split "
                  f"{st['vertices_split']}; clean_mesh {statistics.median(times):.2f} ms (median of {len(times)}, "
                  f"min {min(times):.2f})", flush=True)
            if fname == "sample":
                c0 = charts(M, raw.v, raw.f, raw.normals)
                c1 = charts(M, v, f, raw.normals[vmap])
                try:
                    M.uv_unwrap(v, f, raw.normals[vmap], (a.size, a.size))
                    ok = "bakes"
                except ValueError as e:
                    ok = f"not baked ({e})"
                print(f"    charts {c0} -> {c1}; cleaned mesh at {a.size}^2: {ok}", flush=True)


if __name__ == "__main__":
    main()
