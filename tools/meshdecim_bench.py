"""Mesh decimation (csrc/meshdecim.hip, mesh.decimate_mesh) to the reference's 100 000 faces on the three meshes of
tools/meshclean_bench.py (a sphere of 96 primitives at 256^3 and a sample-like set of 2048 at 128^3 and 256^3), raw and
cleaned: V and F before and after, rounds, `stalled`, for the cleaned meshes the chart count before and after
(uv_unwrap's n_charts, or its ValueError), and the time of decimate_mesh (HIP events around the call, readbacks included; median of --reps runs after
one warm-up).  Per-kernel times: run one case under rocprofv3 --kernel-trace --stats (--only picks the cases).

    python tools/meshdecim_bench.py [--reps 5] [--target 100000] [--size 1024] [--only sphere:256 sample:128 sample:256]
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


def charts(M, mesh, size):
    try:
        return str(M.uv_unwrap(mesh.v, mesh.f, mesh.normals, (size, size)).n_charts)
    except ValueError as e:
        return f"refused ({e})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--target", type=int, default=100000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--only", nargs="+", default=["sphere:256", "sample:128", "sample:256"])
    ap.add_argument("--no-charts", action="store_true", help="skip the uv_unwrap of the meshes (host packing dominates it)")
    a = ap.parse_args()
    __graft_entry__.build()
    from topia_xl_amd import mesh as M

    dev = "cuda:0"
    fields = {"sphere": sphere_field, "sample": sample_field}
    for case in a.only:
        fname, R = case.split(":")
        field = fields[fname](dev)
        raw = M.extract_mesh(field, resolution=int(R))
        for kind, mesh in (("raw", raw), ("cleaned", M.clean_trimesh(raw, **M.CLEAN_ARGS))):
            if mesh.f.shape[0] <= a.target:
                print(f"{fname} {R}^3 {kind}: F {mesh.f.shape[0]} <= {a.target}: not decimated", flush=True)
                continue
            times, st = [], {}
            for rep in range(a.reps + 1):
                st = {}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                v, f = M.decimate_mesh(mesh.v, mesh.f, a.target, stats=st)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times.append(e0.elapsed_time(e1))
            print(f"{fname} {R}^3 {kind}: V {mesh.v.shape[0]} -> {v.shape[0]}, F {mesh.f.shape[0]} -> {f.shape[0]}; rounds "
                  f"{st['rounds']}, stalled {st['stalled']}; decimate_mesh {statistics.median(times):.2f} ms (median of "
                  f"{len(times)}, min {min(times):.2f})", flush=True)
            if not a.no_charts and kind == "cleaned":
                dec = M.decimate_trimesh(mesh, a.target)
                print(f"    charts at {a.size}^2: {charts(M, mesh, a.size)} -> {charts(M, dec, a.size)}", flush=True)


if __name__ == "__main__":
    main()
