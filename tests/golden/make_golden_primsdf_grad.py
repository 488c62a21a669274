"""Generate tests/golden/primsdf_grad.npz from the REAL reference (run in the build container only):

    python tests/golden/make_golden_primsdf_grad.py

`srt_param.grad` / `feat_param.grad` of the unmodified models/primsdf.py:PrimSDF in `.train()`, `.double()`, for the parameters
and points of make_golden.primsdf_params() and loss = sum(cat(sdf, tex, mat) * gout) with a seeded gout.  trimesh, imported at
the reference module's top and unused by forward, is stubbed as make_golden.py stubs it.  Stored: gout (float64), the whole
srt gradient, the payload gradient of every second primitive (the whole one would pass the size limit of a committed file) and
the row sums of all of them.  Data only.
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import ref_import  # noqa: E402
from tests.golden.make_golden import PRIMSDF_CFG, SEED, primsdf_params  # noqa: E402

GOUT_SEED = SEED + 34


def gout_for(n: int) -> torch.Tensor:
    return torch.randn(n, 6, generator=torch.Generator().manual_seed(GOUT_SEED), dtype=torch.float64)


def main():
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
    mod = importlib.import_module("models.primsdf")
    m = mod.PrimSDF(**PRIMSDF_CFG).double().train()
    srt, feat, pts = primsdf_params()
    m.srt_param.data, m.feat_param.data = srt.double(), feat.double()
    gout = gout_for(pts.shape[0])
    pr = m(pts.double())
    (torch.cat([pr["sdf"], pr["tex"], pr["mat"]], 1) * gout).sum().backward()
    gs, gf = m.srt_param.grad.numpy(), m.feat_param.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "primsdf_grad.npz"), seed=np.int64(SEED), gout_seed=np.int64(GOUT_SEED), gout=gout.numpy(),
                        srt_grad=gs, feat_grad_even=gf[::2], feat_grad_rowsum=gf.sum(1))
    print("srt_grad", gs.shape, float(np.abs(gs).max()), "feat_grad", gf.shape, float(np.abs(gf).max()))


if __name__ == "__main__":
    main()
