"""Pin the ray marcher's BACKWARD to the reference's own executable PyTorch formulation (build container only):

    python tests/golden/make_golden_raymarch_grad.py

The route of make_golden_raymarch.py: the "run pytorch version" lines of the reference's `gradcheck()`
(dva/mvp/extensions/mvpraymarch/mvpraymarch.py:391-467) are executed unmodified at generation time, with M = 8, this time through
`sample0.backward(torch.ones_like(sample0))`.  The marcher's four inputs - the post-softplus template, primpos, primrot and
primscale as the march loop receives them - are intermediate tensors of those lines; between the loop and the backward line this
script asks autograd to retain their gradients (`retain_grad()`, which changes no value).  Stored: those four gradients of the
first batch item, fp32, compressed (tests/golden/raymarch_grad.npz).  The inputs are the ones of tests/golden/raymarch.npz (the
script asserts it), so they are not stored twice - except primrot and raydir, whose last bits depend on the torch build that evaluates
Rodrigues' formula and the normalisation: the values these gradients belong to are stored next to them.  Nothing of the reference is copied into the repository.
"""
from __future__ import annotations

import inspect
import os

import numpy as np

from make_golden_raymarch import HERE, REF, _load, _pytorch_section

NAMES = ("template", "primpos", "primrot", "primscale")


def main():
    mod = _load(os.path.join(REF, "mvpraymarch", "mvpraymarch.py"), "mvpraymarchlib")
    env = {k: v.default for k, v in inspect.signature(mod.gradcheck).parameters.items()}
    env.update(vars(mod))
    fwd = _pytorch_section(mod.gradcheck, "sample0 = rayrgba", patches=[(r"M = 32", "M = 8")])
    both = _pytorch_section(mod.gradcheck, "sample0.backward(torch.ones_like(sample0))", patches=[(r"M = 32", "M = 8")])
    assert both.startswith(fwd)
    exec(compile(fwd, "<reference gradcheck: pytorch version>", "exec"), env)
    for k in NAMES:
        env[k].retain_grad()
    exec(compile(both[len(fwd):], "<reference gradcheck: pytorch version, backward>", "exec"), env)
    old = np.load(os.path.join(HERE, "raymarch.npz"))
    for k in NAMES + ("_raypos", "_raydir", "_tminmax"):
        d = float(np.abs(env[k].detach().float().numpy() - old["march_" + k.lstrip("_")]).max())
        print(f"{k}: differs from raymarch.npz by at most {d:.3e}")
        assert d == 0.0 or (k in ("primrot", "_raydir") and d < 1e-6), k     # sin / cos / sqrt may round differently from one torch build to the next
    out = {"grad_" + k: env[k].grad[:1].detach().float().contiguous().numpy() for k in NAMES}     # template: [1, K, 4, M, M, M]
    out["primrot"] = env["primrot"][:1].detach().float().contiguous().numpy()                       # the operands these gradients belong to
    out["raydir"] = env["_raydir"][:1].detach().float().contiguous().numpy()
    path = os.path.join(HERE, "raymarch_grad.npz")
    np.savez_compressed(path, **out)
    print("raymarch_grad.npz", os.path.getsize(path), {k: float(np.abs(v).max()) for k, v in out.items()})
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "raymarch.npz"))


if __name__ == "__main__":
    main()
