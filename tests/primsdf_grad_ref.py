"""Restatement of the differentiable PrimSDF and of the refinement loop, written from the rules of include/primx_hip.h
("PrimSDF field query": the forward, its backward `primx_primsdf_query_backward`, `primx_adam_step`) and of fit.refine_primitives.

* `field(x, srt, feat, S)`: the training-mode query in torch, in the dtype of its arguments (float64 or float32), built from
  differentiable torch operations so that autograd gives d loss / d srt and d loss / d feat.  No eval fill.
* `grads(x, srt, feat, gout, S)`: (gsrt, gfeat) of loss = sum(out * gout).
* `kinks(x, srt, feat, S, delta)`: the points within `delta` of a place where the field is not differentiable.
* `adam_step(...)`: one step of Adam in numpy, every expression as the header writes it, in `dtype`.
* `refine(...)`: fit.refine_primitives' loop on the CPU in `dtype`: same point set, same loss, same schedule.
"""
from __future__ import annotations

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ the field
def _pairs(x, srt):
    """-> (d [n, P, 3], w [n, P]) with w = relu(1 - max_a |d_a| / |s|)."""
    d = x[:, None, :] - srt[None, :, 1:4]
    m = d.abs().max(dim=-1).values                       # (autograd sends the gradient to ONE axis of the maximum)
    w = torch.relu(1 - m / srt[None, :, 0].abs())
    return d, w


def field(x, srt, feat, S: int, clip: bool = True):
    """x [n, 3], srt [P, 4] = (scale, pos), feat [P, C S^3] ([C][z][y][x]) -> out [n, C]: o_c = inv sum_k w_k sigma_kc with
    inv = 1 / (sum_k w_k + 1e-6), sigma the trilinear sample in the cell min(floor(f), S - 2) clamped at 0,
    f = ((x - pos) / s + 1) (S - 1) / 2; channels >= 1 clipped to [0, 1]."""
    n, P = x.shape[0], srt.shape[0]
    C = feat.shape[1] // S ** 3
    d, w = _pairs(x, srt)
    ib, ik = torch.where(w.detach() > 0)
    wk = w[ib, ik]
    f = (d[ib, ik] / srt[ik, 0:1] + 1) * (0.5 * (S - 1))
    cell = f.detach().floor().clamp(0, S - 2)
    t = f - cell
    cell = cell.long()
    ix, iy, iz = cell[:, 0], cell[:, 1], cell[:, 2]
    vol = feat.reshape(P, C, S, S, S)
    tx, ty, tz = t[:, 0:1], t[:, 1:2], t[:, 2:3]

    def at(dz, dy, dx):
        return vol[ik, :, iz + dz, iy + dy, ix + dx]                                        # [pairs, C]
    c00 = at(0, 0, 0) * (1 - tx) + at(0, 0, 1) * tx
    c01 = at(0, 1, 0) * (1 - tx) + at(0, 1, 1) * tx
    c10 = at(1, 0, 0) * (1 - tx) + at(1, 0, 1) * tx
    c11 = at(1, 1, 0) * (1 - tx) + at(1, 1, 1) * tx
    sigma = (c00 * (1 - ty) + c01 * ty) * (1 - tz) + (c10 * (1 - ty) + c11 * ty) * tz
    acc = torch.zeros(n, C, dtype=x.dtype).index_add(0, ib, sigma * wk[:, None])
    out = acc / (w.sum(1, keepdim=True) + 1e-6)
    if not clip:
        return out
    return torch.cat([out[:, :1], out[:, 1:].clip(0, 1)], 1)


def grads(x, srt, feat, gout, S: int):
    """(gsrt, gfeat) of sum(field(x, srt, feat) * gout) by autograd, in the dtype of the arguments."""
    srt, feat = srt.detach().clone().requires_grad_(True), feat.detach().clone().requires_grad_(True)
    (field(x, srt, feat, S) * gout).sum().backward()
    return srt.grad, feat.grad


def kinks(x, srt, feat, S: int, delta: float = 1e-5):
    """bool [n]: the point lies within `delta` (in float64) of a weight boundary max|u| = 1 of any primitive, of a tie of the two
    largest |u_a| of a covering primitive, of a cell boundary of a covering primitive, or a clipped channel of a covered point
    lies within `delta` of 0 or 1."""
    x, srt, feat = x.double(), srt.double(), feat.double()
    u = (x[:, None, :] - srt[None, :, 1:4]) / srt[None, :, 0:1]
    au = u.abs().sort(dim=-1, descending=True).values
    bad = ((au[..., 0] - 1).abs() < delta).any(1)
    cov = au[..., 0] < 1
    bad |= (cov & ((au[..., 0] - au[..., 1]) < delta)).any(1)
    f = (u + 1) * (0.5 * (S - 1))
    bad |= (cov & ((f - f.round()).abs() < delta).any(-1)).any(1)
    o = field(x, srt, feat, S, clip=False)[:, 1:]
    bad |= cov.any(1) & ((o.abs() < delta) | ((o - 1).abs() < delta)).any(1)
    return bad


# ------------------------------------------------------------------------------------------------ Adam
def adam_step(p, g, m, v, t: int, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, dtype=np.float32):
    """Step t (1, 2, ...) -> (p, m, v), every operation rounded to `dtype`, as written in the header:
    m = m + w1 (g - m); v = v beta2 + (w2 g) g; p = p - ((lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps); w = 1 - beta and
    bc = 1 - beta^t in double, then rounded."""
    f = dtype
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b2 = f(beta2)
    w1, w2 = f(1.0 - float(beta1)), f(1.0 - float(beta2))
    bc1, bc2 = f(1.0 - float(beta1) ** t), f(1.0 - float(beta2) ** t)
    step, rbc2 = f(lr) / bc1, np.sqrt(bc2)
    m = m + w1 * (g - m)
    v = v * b2 + (w2 * g) * g
    p = p - (step * m) / (np.sqrt(v) / rbc2 + f(eps))
    return p.astype(f), m.astype(f), v.astype(f)


# ------------------------------------------------------------------------------------------------ the refine loop
SCALE_FLOOR = 1e-4


def refine_points(srt32: torch.Tensor, samples_per_prim: int, seed: int = 0) -> torch.Tensor:
    """fp32 [P * samples_per_prim, 3]: pos + scale * (2 rand - 1), the uniforms from a CPU generator seeded with `seed`."""
    P = srt32.shape[0]
    u = torch.rand(P, samples_per_prim, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float32) * 2 - 1
    return (srt32[:, None, 1:4] + srt32[:, None, 0:1] * u).reshape(-1, 3)


def refine(recon, target, pts, steps: int, S: int, lr=1e-3, lr_srt=None, refine_srt=True, weights=(1.0, 1.0, 1.0),
           dtype=torch.float64):
    """recon [P, 4 + 6 S^3], target [n, 6] and pts [n, 3] (the fixed training set) -> (recon', [loss before each step]) in `dtype`:
    loss = sum(diff^2 coef / 2), coef = 2 w / (n channels) per group; Adam (betas 0.9 / 0.999, eps 1e-8) on the payload with
    `lr` and on srt with `lr_srt` (lr / 100 by default); the scale clamped to SCALE_FLOOR after each step."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    lr_srt = 0.01 * lr if lr_srt is None else lr_srt
    recon, target, pts = (torch.as_tensor(a).to(dtype) for a in (recon, target, pts))
    srt, feat = recon[:, :4].clone(), recon[:, 4:].clone()
    n = pts.shape[0]
    ws, wt, wm = weights
    coef = torch.tensor([2 * ws / n] + [2 * wt / (3 * n)] * 3 + [2 * wm / (2 * n)] * 2, dtype=dtype)
    state = {k: np.zeros(a.shape, npdt) for k, a in (("ms", srt), ("vs", srt), ("mf", feat), ("vf", feat))}
    losses = []
    for t in range(1, steps + 1):
        srt.requires_grad_(True), feat.requires_grad_(True)
        diff = field(pts, srt, feat, S) - target
        loss = (diff * diff * (coef * 0.5)).sum()
        gs, gf = torch.autograd.grad(loss, (srt, feat))
        losses.append(float(loss.detach()))
        srt, feat = srt.detach(), feat.detach()
        f, state["mf"], state["vf"] = adam_step(feat.numpy(), gf.numpy(), state["mf"], state["vf"], t, lr, dtype=npdt)
        feat = torch.from_numpy(f)
        if refine_srt:
            s, state["ms"], state["vs"] = adam_step(srt.numpy(), gs.numpy(), state["ms"], state["vs"], t, lr_srt, dtype=npdt)
            s[:, 0] = np.maximum(s[:, 0], npdt(SCALE_FLOOR))
            srt = torch.from_numpy(s)
    return torch.cat([srt, feat], 1), losses


def icosphere_problem(samples_per_prim: int = 64, seed: int = 0):
    """The refinement problem of the tests on the CPU: meshfield_numpy's fit of icosphere(1) with 33 primitives of 3^3 voxels from
    300 candidates (float32 recon), the fixed point set and the mesh's own field there -> (recon [33, 166], target [n, 6],
    pts [n, 3]), float32 numpy / torch."""
    from tests import meshfield_numpy as MF
    v, f = MF.icosphere(1)
    attr = MF.affine_attr(v)
    u = torch.rand(300, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float32).numpy()
    lin = torch.linspace(-1, 1, 3).numpy()
    recon, info = MF.mesh_to_primitives(v, f, attr, u, lin, 33, 3)
    recon = torch.from_numpy(recon.astype(np.float32))
    pts = refine_points(recon[:, :4], samples_per_prim, seed)
    q = MF.query(pts.numpy(), info["v"], f, attr, np.float64, keep_d2=False)
    target = np.concatenate([MF.sdf_of(q)[:, None], np.clip(q["attr"], 0, 1)], 1).astype(np.float32)
    return recon, torch.from_numpy(target), pts
