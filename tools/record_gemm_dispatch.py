#!/usr/bin/env python3
"""Record tests/golden/gemm_dispatch.json: for every row of the case table of tests/test_hip_gemm_dispatch.py, the kernel name
primx_last_gemm_kernel() reports after the call (null: the call is rejected) and what ops.fold_shapes_ok / ops.fold_pair_fits
say on the rows that name them.  One fresh child process per environment, as in the test.

The file states what the dispatch of csrc/gemm.hip DID at the commit named in it; it is recorded BEFORE a change to that dispatch
and never regenerated from the changed code - a refactor is held to it.

    python tools/record_gemm_dispatch.py --commit <hash of the commit the library was built from> [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_hip_gemm_dispatch as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit csrc/gemm.hip was built from")
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    kernels = {}
    for env in T.ENVS:
        kernels[T.env_key(env)] = T.run_env(env)
        print(T.env_key(env), len(kernels[T.env_key(env)]), "rows", flush=True)
    with open(a.out, "w") as fh:
        json.dump({"recorded_at_commit": a.commit, "kernels": kernels}, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
