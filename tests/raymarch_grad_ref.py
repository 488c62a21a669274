"""TEST INFRASTRUCTURE ONLY: a float64 restatement of the ray march that torch.autograd differentiates - the reference of
`primx_raymarch_backward` (include/primx_hip.h, ABI 35).

Every ray runs against the primitives of its tile's hit list (8 x 8 pixels, index order, 512 cap), out of place.  The sample
POSITIONS are the fp32 trajectory the kernel walks, emulated with the helpers of tests/raymarch_replay.py (`f32`, `fma`,
`_slab`; the start and step rules of its docstring), and enter as constants.  The local position y = ((x - pos) rot) scale, the
fade exp(-fs sum |y_d|^fe), the trilinear sample and the accumulation are functions of the four differentiable inputs
(template, primpos, primrot, primscale) in `dtype`.  WHICH samples are taken - strict |y| < 1, t < rtmax + 1e-5, not after the
saturating sample - is decided from the float64 y and enters as a constant; so is the cell of the trilinear sample.

The accumulation is the closed form of the sequential rule (as in the replay): over a ray's taken samples in (step, index)
order, cum_i = sum_{j <= i} a_j dt;  alpha = min(1, cum_last);  rgb = sum_i rgb_i (min(1, cum_i) - min(1, cum_{i-1})).  For a_j >= 0
this is newalpha = A + a dt, contrib = min(newalpha, 1) - A with A = min(1, cum_{i-1}), and nothing after newalpha >= 1.  Its
autograd is primaccum.h:81-98: weight = contrib for rgb, dt ((rgb_i - S) . dL.rgb + (saturates ? 0 : dL.a)) for an unsaturated
sample's alpha, 0 for the saturating one (the clamp's derivative).

`march` also returns the smallest margin of any decision of the scene: | |y|_inf - 1 | over listed samples of live rays before
rtmax + 1e-5 (a sample further than a step from a box has a margin of a step or more, so taking all of them changes nothing),
|t - (rtmax + 1e-5)| over the steps of live rays, and |newalpha - 1| over taken samples.
"""
from __future__ import annotations

import math

import torch

from tests import raymarch_replay as rr
from tests.raymarch_replay import f32, fma

PAIR_BUDGET = 1 << 22          # (ray, step, primitive) candidates per float64 pass


def _decisions(ro, rd, tmin0, tmax0, dt, pos, rot, scl, H, W):
    """Constants of one batch item, from fp32 values held in float64: the listed mask [R, K], the live mask [R], the fp32
    trajectory T [R, J], P [R, J, 3], the threshold thr = fl(rtmax + 1e-5) [R] and the taken samples (ray, step, primitive) in
    (ray, step, index) order before saturation is applied, with the face / t margins."""
    R, K = ro.shape[0], pos.shape[0]
    dt_t = torch.tensor(dt, dtype=torch.float64)
    trmin, trmax = rr._slab(ro, rd, pos, rot, scl)
    hit = trmin <= trmax
    inf = torch.tensor(math.inf, dtype=torch.float64)
    rtmin = torch.fmax(torch.where(hit, trmin, inf).amin(1), tmin0)
    rtmax = torch.fmin(torch.where(hit, trmax, -inf).amax(1), tmax0)
    hh = torch.arange(H)[:, None].expand(H, W).reshape(-1)
    ww = torch.arange(W)[None, :].expand(H, W).reshape(-1)
    tiles_w = (W + rr.TILE - 1) // rr.TILE
    tile = (hh // rr.TILE) * tiles_w + ww // rr.TILE
    tany = torch.zeros(((H + rr.TILE - 1) // rr.TILE) * tiles_w, K, dtype=torch.long).index_add_(0, tile, hit.long()) > 0
    listed = (tany & (torch.cumsum(tany.long(), 1) <= rr.MAXHIT))[tile]
    # start and steps (fp32, as the ISA; tests/raymarch_replay.py)
    live = torch.isfinite(rtmin) & (rtmin <= rtmax + 1e-5)
    incs = torch.floor(f32(f32(torch.where(live, rtmin, tmin0) - tmin0) / dt_t))
    incs = torch.where(live, incs, torch.zeros_like(incs))
    t = fma(incs, dt_t, tmin0)
    p = fma(f32(rd * incs[:, None]), dt_t, fma(rd, tmin0[:, None], ro))
    thr = f32(rtmax + f32(torch.tensor(1e-5, dtype=torch.float64)))
    step = f32(rd * dt_t)
    ts, ps = [t], [p]
    while bool(((t < thr) & live).any()):
        t, p = f32(t + dt_t), f32(p + step)
        ts.append(t)
        ps.append(p)
    T, P = torch.stack(ts, 1), torch.stack(ps, 1)
    J = T.shape[1]
    tok = (T < thr[:, None]) & live[:, None]
    m_t = float((T - thr[:, None]).abs()[live].min()) if bool(live.any()) else math.inf
    # float64 inside test of every listed (ray, step, primitive), a block of steps at a time
    found = []
    face_prim, face_ray = torch.full((K,), math.inf, dtype=torch.float64), torch.full((R,), math.inf, dtype=torch.float64)
    jc = max(1, PAIR_BUDGET // max(1, R * K))
    for j0 in range(0, J, jc):
        x = P[:, j0:j0 + jc]                                                        # [R, j, 3]
        y = torch.einsum("rjkc,kcd->rjkd", x[:, :, None, :] - pos[None, None], rot) * scl[None, None]
        top = y.abs().amax(-1)
        cand = listed[:, None, :] & tok[:, j0:j0 + jc, None]
        m = torch.where(cand, (top - 1.0).abs(), inf)
        face_prim, face_ray = torch.minimum(face_prim, m.amin((0, 1))), torch.minimum(face_ray, m.amin((1, 2)))
        r, j, k = (cand & (top < 1.0)).nonzero(as_tuple=True)
        found.append(torch.stack([r, j + j0, k], 1))
    e = torch.cat(found)
    e = e[torch.argsort((e[:, 0] * J + e[:, 1]) * K + e[:, 2])]
    return dict(listed=listed, live=live, T=T, P=P, thr=thr, e=e, face_prim=face_prim, face_ray=face_ray, m_t=m_t, steps=J)


def _values(x, ek, pos, rot, scl, tpl, fs, fe):
    """(rgb [E, 3], a [E]) of samples at constant positions x [E, 3] inside primitives ek [E]: functions of pos, rot, scl, tpl."""
    dt = pos.dtype
    y = torch.einsum("ec,ecd->ed", x.to(dt) - pos[ek], rot[ek]) * scl[ek]
    fade = torch.exp(-fs * (y.abs() ** fe).sum(-1))
    K, D, Hh, Ww, _ = tpl.shape
    size = torch.tensor([Ww - 1, Hh - 1, D - 1], dtype=dt)
    g = (y + 1.0) * 0.5 * size
    i0 = torch.minimum(torch.clamp(torch.floor(g.detach()).long(), min=0), torch.tensor([Ww - 2, Hh - 2, D - 2]))
    f = g - i0
    raw = torch.zeros(x.shape[0], 4, dtype=dt)
    for c in range(8):
        bx, by, bz = c & 1, (c >> 1) & 1, c >> 2
        w = (f[:, 0] if bx else 1 - f[:, 0]) * (f[:, 1] if by else 1 - f[:, 1]) * (f[:, 2] if bz else 1 - f[:, 2])
        raw = raw + tpl[ek, i0[:, 2] + bz, i0[:, 1] + by, i0[:, 0] + bx] * w[:, None]
    return raw[:, :3], raw[:, 3] * fade


def march(raypos, raydir, tminmax, stepsize, primpos, primrot, primscale, template, fadescale, fadeexp, dtype=torch.float64):
    """raypos / raydir [N,H,W,3], tminmax [N,H,W,2] (fp32, constants); primpos [N,K,3], primrot [N,K,3,3], primscale [N,K,3],
    template [N,K,TD,TH,TW,4] channels-last, of `dtype` (they may require grad; their values are fp32 values).
    -> (image [N,H,W,4] of `dtype`, info): info["margin"] = {"face", "t", "alpha"}, info["samples"] = the largest number of taken
    samples of a ray, info["taken"] = all of them, info["hit"] / info["saturated"] = rays with a sample / saturated rays,
    info["steps"]; info["face_prim"] [K] / info["face_ray"] [H W] per batch item = the face margin by primitive / by ray."""
    N, H, W, _ = raypos.shape
    dt = float(torch.tensor(stepsize, dtype=torch.float32))
    D = lambda v: v.detach().to(torch.float64)
    out = []
    info = dict(margin=dict(face=math.inf, t=math.inf, alpha=math.inf), samples=0, taken=0, hit=0, saturated=0, steps=0, face_prim=[],
                face_ray=[])
    for n in range(N):
        ro, rd = D(raypos[n]).reshape(-1, 3), D(raydir[n]).reshape(-1, 3)
        tmin0, tmax0 = D(tminmax[n]).reshape(-1, 2).unbind(-1)
        c = _decisions(ro, rd, tmin0, tmax0, dt, D(primpos[n]), D(primrot[n]), D(primscale[n]), H, W)
        er, ej, ek = c["e"].unbind(1)
        R, E = ro.shape[0], er.shape[0]
        rgb, a = _values(c["P"][er, ej], ek, primpos[n], primrot[n], primscale[n], template[n], fadescale, fadeexp)
        assert E == 0 or float(a.detach().min()) >= 0.0, "the closed-form accumulation needs alpha >= 0"
        # rows = rays, columns = the ray's samples in order
        first = torch.ones(E, dtype=torch.bool)
        first[1:] = er[1:] != er[:-1]
        start = torch.cummax(torch.where(first, torch.arange(E), torch.zeros(E, dtype=torch.long)), 0)[0]
        rank = torch.arange(E) - start
        S = int(rank.max()) + 1 if E else 1
        adt = torch.zeros(R, S, dtype=dtype).index_put((er, rank), a * dt)
        col = torch.zeros(R, S, 3, dtype=dtype).index_put((er, rank), rgb)
        cum = torch.cumsum(adt, 1)
        prev = cum - adt
        contrib = torch.clamp(cum, max=1.0) - torch.clamp(prev, max=1.0)
        img = torch.cat([(col * contrib[..., None]).sum(1), contrib.sum(1, keepdim=True)], 1)
        out.append(img.reshape(H, W, 4))
        if E:
            used = torch.zeros(R, S, dtype=torch.bool).index_put((er, rank), torch.ones(E, dtype=torch.bool)) & (prev.detach() < 1.0)
            info["margin"]["alpha"] = min(info["margin"]["alpha"], float((cum.detach().double() - 1.0).abs()[used].min()))
            info["samples"] = max(info["samples"], int(used.sum(1).max()))
            info["taken"] += int(used.sum())
            info["hit"] += int(used.any(1).sum())
            info["saturated"] += int((cum.detach()[:, -1] >= 1.0).sum())
        info["margin"]["face"] = min(info["margin"]["face"], float(c["face_prim"].min()))
        info["face_prim"].append(c["face_prim"])
        info["face_ray"].append(c["face_ray"])
        info["margin"]["t"] = min(info["margin"]["t"], c["m_t"])
        info["steps"] = max(info["steps"], c["steps"])
    return torch.stack(out), info


def grads(raypos, raydir, tminmax, stepsize, primpos, primrot, primscale, template, gout, fadescale, fadeexp, dtype=torch.float64):
    """-> ((gtemplate, gpos, grot, gscale), image, info): autograd of <gout, image> through `march` in `dtype`."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (template, primpos, primrot, primscale)]
    img, info = march(raypos, raydir, tminmax, stepsize, leaves[1], leaves[2], leaves[3], leaves[0], fadescale, fadeexp, dtype)
    (img * gout.to(dtype)).sum().backward()
    return tuple(torch.zeros_like(t) if t.grad is None else t.grad for t in leaves), img.detach(), info
