"""TEST INFRASTRUCTURE ONLY: an unfiltered replay of csrc/raymarch.hip's raymarch_kernel with a derived per-pixel bound.

What the kernel header documents as semantics is restated without its optimizations (no chunks, no step windows, no
record cache): the per-tile (8 x 8 pixels, index order) hit list with its 512 cap, each ray's own [rtmin, rtmax], the
`incs` start step, the strict |y| < 1 inside test, `t < rtmax + 1e-5` and saturation.

Everything that decides WHICH samples are taken is replayed in fp32 as the gfx950 code does it (hipcc -S of raymarch.hip):
  start     rp = fma(rd, tmin, ro);  t = fma(incs, dt, tmin);  rp = fma(rd * incs, dt, rp)
  step      t += dt;  rp += fl(rd * dt)          (the product is hoisted out of the loop: an add, not an fma)
  slab / y  the clang contraction of the sources (fma(a, b, c * d) + ...); the compiler reorders these sums, so the
            inside test, the slab intervals and `t` vs `rtmax + 1e-5` are decided with a band of DELTA_Y / DELTA_T
fma(a, b, c) is emulated as fl32(a * b + c) in float64 (the product is exact; the double rounding is harmless here).
What only moves the value - the trilinear sample, exp(-fs sum |y|^fe) and the accumulation - is evaluated in float64.

A march of ~2 x 10^4 steps per ray is replayed without a step loop per primitive: the fp32 trajectory (t_j, rp_j) of every
ray is scanned once; a (ray, primitive) pair is only tested at the steps j whose line point p0 + j dt rd lies in the
primitive's box grown by the trajectory's measured deviation from that line (max_j |rp_j - p0 - j dt rd|) - a provable
superset of the steps whose rp_j can be inside.  The taken samples are then accumulated in closed form:
acc.a = min(1, cumsum(alpha dt)), acc.rgb = sum rgb * (min(1, cum_i) - min(1, cum_{i-1})).

Bound per pixel and channel (fp32 value error + decisions near their thresholds):
  fade     v_log_f32 / v_exp_f32 each 2^-22 relative (+ 2^-22 absolute for log2 near 1) through fast_pow / fast_exp
  sample   fp32 grid coordinate (3 roundings of a value <= S - 1) and 8 weights of 3 products, 8 fma accumulations
  position the sample's local coordinate to DELTA_Y (fp32 transform): |d sample / d y| DELTA_Y, incl. the fade's slope
  accum    per taken sample 3 fp32 roundings of acc.a and 2 of acc.rgb; an error E_a of acc.a moves the saturating
           sample by E_a (|rgb| E_a) and may admit one more sample's E_a worth
  decision every sample within DELTA_Y of a face or DELTA_T of rtmax + 1e-5 (taken or not) adds its contribution
           alpha dt (|rgb_i| + max rgb of the ray), as long as the ray is not saturated before it
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
DELTA_Y = 1e-6          # band of the inside test in local units (|y| ~ 1: ~16 fp32 ulps)
DELTA_T = 2e-6          # band of t vs rtmax + 1e-5 (relative to max(1, |t|))
MAXHIT = 512
TILE = 8


def f32(x):
    return x.to(torch.float32).to(torch.float64)


def fma(a, b, c):
    return f32(a * b + c)


def _local(x, pos, rot, scl):
    """fp32 R^T-row transform of [.., 3] points: y_i = (r0i x + r1i y + r2i z) * s_i, contracted as clang does."""
    xm = f32(x - pos)
    out = []
    for i in range(3):
        a = fma(rot[..., 0, i], xm[..., 0], f32(rot[..., 1, i] * xm[..., 1]))
        a = fma(rot[..., 2, i], xm[..., 2], a)
        out.append(f32(a * scl[..., i]))
    return torch.stack(out, -1)


def _slab(ro, rd, pos, rot, scl):
    """fp32 slab interval of rays [R, 3] against primitives [K, ..] -> trmin, trmax [R, K] (kernel formulas)."""
    r0 = _local(ro[:, None, :], pos[None], rot[None], scl[None])
    r1 = []
    for i in range(3):
        a = fma(rot[None, :, 0, i], rd[:, None, 0], f32(rot[None, :, 1, i] * rd[:, None, 1]))
        a = fma(rot[None, :, 2, i], rd[:, None, 2], a)
        r1.append(f32(a * scl[None, :, i]))
    r1 = torch.stack(r1, -1)
    with np.errstate(all="ignore"):
        ix = f32(1.0 / r1)
        a, b = f32((-1.0 - r0) * ix), f32((1.0 - r0) * ix)
    lo, hi = torch.fmin(a, b), torch.fmax(a, b)
    trmin = torch.fmax(torch.fmax(lo[..., 0], lo[..., 1]), lo[..., 2])
    trmax = torch.fmin(torch.fmin(hi[..., 0], hi[..., 1]), hi[..., 2])
    return trmin, trmax


def _trilinear(tpl, k, y):
    """float64 trilinear sample of channels-last templates tpl [K, D, H, W, 4] at local y [E, 3] of primitives k [E]."""
    K, D, Hh, Ww, _ = tpl.shape
    g = (y + 1.0) * 0.5 * torch.tensor([Ww - 1, Hh - 1, D - 1], dtype=torch.float64, device=y.device)
    i0 = torch.floor(g).long()
    i0 = torch.minimum(torch.clamp(i0, min=0), torch.tensor([Ww - 2, Hh - 2, D - 2], device=y.device))
    f = g - i0
    s = torch.zeros(y.shape[0], 4, dtype=torch.float64, device=y.device)
    qabs = torch.zeros(y.shape[0], 4, dtype=torch.float64, device=y.device)
    qs = []
    for c in range(8):
        bx, by, bz = c & 1, (c >> 1) & 1, c >> 2
        w = (f[:, 0] if bx else 1 - f[:, 0]) * (f[:, 1] if by else 1 - f[:, 1]) * (f[:, 2] if bz else 1 - f[:, 2])
        q = tpl[k, i0[:, 2] + bz, i0[:, 1] + by, i0[:, 0] + bx]
        s = s + q * w[:, None]
        qabs = qabs + q.abs() * w[:, None]
        qs.append(q)
    qs = torch.stack(qs)
    qdiff = qs.amax(0) - qs.amin(0)
    return s, qabs, qdiff


def replay(raypos, raydir, tminmax, stepsize, primpos, primrot, primscale, template, fadescale, fadeexp, device="cpu",
           with_stats=False):
    """raypos / raydir [N,H,W,3], tminmax [N,H,W,2], prim* [N,K,..], template [N,K,TD,TH,TW,4] channels-last (fp32).
    Returns (exact [N,H,W,4] float64, bound [N,H,W,4] float64, stats): stats counts samples, ambiguous decisions and
    steps; with_stats=True adds per batch entry the taken samples and the fp32 trajectories (stats["windows"]) that
    window_misses() and chunk_sublists() read."""
    N, H, W, _ = raypos.shape
    K = primpos.shape[1]
    dt = float(np.float32(stepsize))
    dt_t = torch.tensor(dt, dtype=torch.float64, device=device)
    exact = torch.zeros(N, H, W, 4, dtype=torch.float64)
    bound = torch.zeros(N, H, W, 4, dtype=torch.float64)
    stats = dict(samples=0, ambiguous=0, steps=0, windows=[])
    D = lambda x: x.to(device=device, dtype=torch.float64)
    for n in range(N):
        ro, rd = D(raypos[n]).reshape(-1, 3), D(raydir[n]).reshape(-1, 3)
        tmin0, tmax0 = D(tminmax[n]).reshape(-1, 2).unbind(-1)
        pos, rot, scl = D(primpos[n]), D(primrot[n]), D(primscale[n])
        tpl = D(template[n])
        R = ro.shape[0]
        # ---- hit list per tile (index order, capped) and each ray's own [rtmin, rtmax]
        trmin, trmax = _slab(ro, rd, pos, rot, scl)
        hit = trmin <= trmax
        inf = torch.tensor(math.inf, dtype=torch.float64, device=device)
        rtmin = torch.where(hit, trmin, inf).amin(1)
        rtmax = torch.where(hit, trmax, -inf).amax(1)
        rtmin, rtmax = torch.fmax(rtmin, tmin0), torch.fmin(rtmax, tmax0)
        hh = torch.arange(H, device=device)[:, None].expand(H, W).reshape(-1)
        ww = torch.arange(W, device=device)[None, :].expand(H, W).reshape(-1)
        tiles_w = (W + TILE - 1) // TILE
        tile = (hh // TILE) * tiles_w + ww // TILE
        ntile = ((H + TILE - 1) // TILE) * tiles_w
        tany = torch.zeros(ntile, K, dtype=torch.long, device=device).index_add_(0, tile, hit.long()) > 0
        listed_t = tany & (torch.cumsum(tany.long(), 1) <= MAXHIT)
        listed = listed_t[tile]                                                       # [R, K]
        # ---- start (fp32, as the ISA)
        live = torch.isfinite(rtmin) & (rtmin <= rtmax + 1e-5)
        rtmin_s = torch.where(live, rtmin, tmin0)
        incs = torch.floor(f32((f32(rtmin_s - tmin0)) / dt_t))
        incs = torch.where(live, incs, torch.zeros_like(incs))
        t0 = fma(incs, dt_t, tmin0)
        p = fma(rd, tmin0[:, None], ro)
        p = fma(f32(rd * incs[:, None]), dt_t, p)
        thr = f32(rtmax + f32(torch.tensor(1e-5, dtype=torch.float64)))
        # ---- fp32 trajectory scan until every live ray is past its rtmax + 1e-5
        step = f32(rd * dt_t)
        ts, ps = [t0], [p]
        t, pp = t0, p
        while bool(((t < thr) & live).any()):
            t = f32(t + dt_t)
            pp = f32(pp + step)
            ts.append(t)
            ps.append(pp)
        T = torch.stack(ts, 1).float()                                               # [R, J] (fp32 values)
        P = torch.stack(ps, 1).float()                                               # [R, J, 3]
        J = T.shape[1]
        stats["steps"] = max(stats["steps"], J)
        nsteps = ((T.double() < thr[:, None]) & live[:, None]).sum(1)                # taken steps: a prefix
        line = p[:, None, :] + torch.arange(J, dtype=torch.float64, device=device)[None, :, None] * dt_t * rd[:, None, :]
        dev_max = (P.double() - line).norm(dim=-1).amax(1)                           # [R]
        del line
        # ---- candidate steps per listed pair: line point inside the box grown by the deviation (float64)
        rr, kk = (listed & live[:, None] & (nsteps[:, None] > 0)).nonzero(as_tuple=True)
        grow = 1.0 + 2.0 * DELTA_Y + math.sqrt(3.0) * dev_max[rr] * scl[kk].abs().amax(-1) * rot[kk].abs().amax((-1, -2)) * 3.0
        o = p[rr]
        y0 = torch.einsum("ei,eij->ej", o - pos[kk], rot[kk]) * scl[kk]
        y1 = torch.einsum("ei,eij->ej", rd[rr], rot[kk]) * scl[kk]
        with np.errstate(all="ignore"):
            a = (-grow[:, None] - y0) / y1
            b = (grow[:, None] - y0) / y1
        lo = torch.fmax(torch.fmax(torch.fmin(a, b)[:, 0], torch.fmin(a, b)[:, 1]), torch.fmin(a, b)[:, 2])
        hi = torch.fmin(torch.fmin(torch.fmax(a, b)[:, 0], torch.fmax(a, b)[:, 1]), torch.fmax(a, b)[:, 2])
        # parallel axes (y1 = 0) give +-inf / nan: inside along that axis iff |y0| < grow
        par = (y1 == 0)
        outside_par = (par & (y0.abs() >= grow[:, None])).any(-1)
        lo = torch.where(torch.isnan(lo), torch.zeros_like(lo), lo)
        hi = torch.where(torch.isnan(hi), torch.full_like(hi, 1e30), hi)
        j0 = torch.clamp(torch.ceil(lo / dt) - 1, min=0)
        j1 = torch.minimum(torch.floor(hi / dt) + 1, (nsteps[rr] - 1).double())
        ok = (j1 >= j0) & ~outside_par
        rr, kk, j0, j1 = rr[ok], kk[ok], j0[ok].long(), j1[ok].long()
        cnt = j1 - j0 + 1
        e_pair = torch.repeat_interleave(torch.arange(rr.shape[0], device=device), cnt)
        off = torch.arange(e_pair.shape[0], device=device) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        er, ek, ej = rr[e_pair], kk[e_pair], j0[e_pair] + off
        # ---- exact fp32 inside decision (+ band) and t decision at every candidate
        x = P[er, ej].double()
        y = _local(x, pos[ek], rot[ek], scl[ek])
        ay = y.abs()
        inside = (ay < 1.0).all(-1)
        near_face = ((ay < 1.0 + DELTA_Y).all(-1)) & ((ay > 1.0 - DELTA_Y).any(-1))
        tj = T[er, ej].double()
        tok = tj < thr[er]
        near_t = (tj - thr[er]).abs() <= DELTA_T * torch.clamp(tj.abs(), min=1.0)
        keep = inside | near_face
        er, ek, ej, y, inside, near_face, tok, near_t = (v[keep] for v in (er, ek, ej, y, inside, near_face, tok, near_t))
        take = inside & tok
        amb = (near_face & (tok | near_t)) | (inside & near_t)
        # order of accumulation: ray, step, list (index) order
        order = torch.argsort((er * J + ej) * K + ek)
        er, ek, ej, y, take, amb = er[order], ek[order], ej[order], y[order], take[order], amb[order]
        # ---- float64 values
        s, qabs, qdiff = _trilinear(tpl, ek, y)
        ay = y.abs()
        L = torch.log2(ay)
        pw = torch.exp2(fadeexp * L)
        ssum = pw.sum(-1)
        fade = torch.exp(-fadescale * ssum)
        alpha = s[:, 3] * fade
        adt = alpha * dt
        # fade relative error (v_log / v_exp 2^-22 each, fp32 products / sums 2^-24)
        # |y_d| = 0: v_log gives -inf and v_exp 0, exactly the value - no error (and no inf * 0 in the bound)
        Lf = torch.where(ay > 0, L, torch.zeros_like(L))
        e_arg = fadeexp * (2.0 ** -22) * (Lf.abs() + 1.0) + U * (fadeexp * Lf).abs()
        e_pw = torch.where(ay > 0, pw * (math.log(2.0) * e_arg + 2.0 ** -22), torch.zeros_like(pw))
        e_sum = e_pw.sum(-1) + 2 * U * ssum
        arg = fadescale * ssum * 1.4426950408889634
        e_fade = math.log(2.0) * (fadescale * 1.4426950408889634 * e_sum + 3 * U * arg) + 2.0 ** -22
        TWm1 = max(tpl.shape[1:4]) - 1
        e_s = U * (12.0 * qabs + 6.0 * TWm1 * qdiff)                                    # [E, 4]
        # position: d sample / d y <= 1.5 (S - 1) qdiff per axis; d fade / d y_d = fade fs fe |y_d|^(fe-1)
        slope = 1.5 * TWm1 * qdiff + s.abs() * (fadescale * fadeexp * ay.clamp(max=1.0) ** max(fadeexp - 1.0, 0.0)).sum(-1, keepdim=True)
        e_pos = DELTA_Y * slope
        # ---- closed-form accumulation per ray over the taken samples
        a_take = torch.where(take, adt, torch.zeros_like(adt))
        cum = torch.cumsum(a_take, 0)
        first = torch.ones_like(er, dtype=torch.bool)
        first[1:] = er[1:] != er[:-1]
        seg_start = torch.cummax(torch.where(first, torch.arange(er.shape[0], device=device), torch.zeros_like(er)), 0)[0]
        base = (cum - a_take)[seg_start]
        cum = cum - base
        prev = cum - a_take
        contrib = torch.clamp(cum, max=1.0) - torch.clamp(prev, max=1.0)
        rgba = torch.cat([s[:, :3], torch.ones_like(s[:, :1])], 1)
        acc_vals = torch.zeros(R, 4, dtype=torch.float64, device=device).index_add_(0, er, rgba * contrib[:, None])
        # value error: alpha's relative error (fade + sample's own), sample error, accumulation roundings
        rel_a = e_fade + e_s[:, 3] / s[:, 3].abs().clamp(min=1e-30) + e_pos[:, 3] / s[:, 3].abs().clamp(min=1e-30)
        e_contrib = contrib * rel_a
        cum_c = torch.clamp(cum, max=1.0)
        Ew_terms = torch.where(take, e_contrib + 3 * U * cum_c, torch.zeros_like(cum))
        Ew = torch.zeros(R, dtype=torch.float64, device=device).index_add_(0, er, Ew_terms)
        e_rgb = contrib[:, None] * (s[:, :3].abs() * (rel_a[:, None] + 2 * U) + e_s[:, :3] + e_pos[:, :3])
        e_rgb = torch.where(take[:, None], e_rgb, torch.zeros_like(e_rgb))
        Erg = torch.zeros(R, 3, dtype=torch.float64, device=device).index_add_(0, er, e_rgb)
        Erg = Erg + 2 * U * acc_vals[:, :3].abs() * torch.zeros(R, 1, dtype=torch.float64, device=device).index_add_(
            0, er, take.double()[:, None])
        smax = torch.zeros(R, 3, dtype=torch.float64, device=device).scatter_reduce_(
            0, er[:, None].expand(-1, 3), torch.where(take[:, None], s[:, :3].abs(), torch.zeros_like(s[:, :3])), "amax")
        # decisions near a threshold (before saturation)
        a_amb = torch.where(amb & (prev < 1.0 + 1e-6), torch.clamp(adt, min=0.0), torch.zeros_like(adt))
        dec = torch.zeros(R, 4, dtype=torch.float64, device=device).index_add_(
            0, er, torch.cat([a_amb[:, None] * (s[:, :3].abs() + smax[er]), a_amb[:, None]], 1))
        bnd = torch.cat([Erg + 2 * smax * Ew[:, None], 2 * Ew[:, None]], 1) + dec
        exact[n] = acc_vals.reshape(H, W, 4).cpu()
        bound[n] = bnd.reshape(H, W, 4).cpu()
        stats["samples"] += int(take.sum())
        stats["ambiguous"] += int(amb.sum())
        if with_stats:
            stats["windows"].append(dict(er=er[take].cpu(), ek=ek[take].cpu(), ej=ej[take].cpu(), T=T.cpu(), P=P.cpu(),
                                         ro=ro.cpu(), rd=rd.cpu(), pos=pos.cpu(), rot=rot.cpu(), scl=scl.cpu(),
                                         thr=thr.cpu(), live=live.cpu(), listed=listed.cpu(), tile=tile.cpu()))
    return exact, bound, stats


def window_misses(st, stepsize, chunk=96, margin=2.0, from_rp=False):
    """How many taken samples of a replay fall outside the kernel's per-chunk step window [e0, e1] for their primitive.
    from_rp=False: the window as written before the fix - slab interval from the ray origin, minus t at the chunk start;
    from_rp=True: slab interval from the sample position rp at the chunk start.  Returns (misses, largest gap in steps)."""
    dt = float(np.float32(stepsize))
    er, ek, ej = st["er"], st["ek"], st["ej"]
    c0 = (ej // chunk) * chunk
    if from_rp:
        org = st["P"][er, c0].double()
        tc = torch.zeros_like(er, dtype=torch.float64)
    else:
        org = st["ro"][er]
        tc = st["T"][er, c0].double()
    trmin, trmax = [], []
    for i in range(0, er.shape[0], 1 << 16):
        sl = slice(i, i + (1 << 16))
        a, b = _slab_pairs(org[sl], st["rd"][er[sl]], st["pos"][ek[sl]], st["rot"][ek[sl]], st["scl"][ek[sl]])
        trmin.append(a)
        trmax.append(b)
    trmin, trmax = torch.cat(trmin), torch.cat(trmax)
    e0 = torch.floor(f32(f32(trmin - tc) / dt)) - margin
    e1 = torch.ceil(f32(f32(trmax - tc) / dt)) + margin
    local = (ej - c0).double()
    miss = (local < e0) | (local > e1)
    gap = torch.maximum(e0 - local, local - e1).clamp(min=0)
    return int(miss.sum()), float(gap.max()) if gap.numel() else 0.0


def _slab_pairs(o, rd, pos, rot, scl):
    r0 = _local(o, pos, rot, scl)
    r1 = []
    for i in range(3):
        a = fma(rot[:, 0, i], rd[:, 0], f32(rot[:, 1, i] * rd[:, 1]))
        a = fma(rot[:, 2, i], rd[:, 2], a)
        r1.append(f32(a * scl[:, i]))
    r1 = torch.stack(r1, -1)
    ix = f32(1.0 / r1)
    a, b = f32((-1.0 - r0) * ix), f32((1.0 - r0) * ix)
    lo, hi = torch.fmin(a, b), torch.fmax(a, b)
    return torch.fmax(torch.fmax(lo[:, 0], lo[:, 1]), lo[:, 2]), torch.fmin(torch.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])


def chunk_sublists(st, stepsize, chunk=96):
    """The size of every chunk sub-list the kernel builds, per 8 x 8 tile and 96-step chunk: the tile's listed primitives
    that some live ray of the tile does not skip, with the skip test measured from the ray's rp at the chunk start
    (raymarch.hip: trmax < -2 dt, trmin > 96 dt + 2 dt or trmin > trmax + 4 dt).  A ray is live while t <= rtmax + 1e-5;
    saturation, which also ends a ray, is not modelled, so use it on scenes without saturated rays.  -> [tiles, chunks]."""
    dt = float(np.float32(stepsize))
    c_end = float(np.float32(chunk * dt))
    T, P, thr, live, listed, tile = st["T"], st["P"], st["thr"], st["live"], st["listed"], st["tile"]
    J = T.shape[1]
    cs = torch.arange(0, J, chunk)
    out = torch.zeros(int(tile.max()) + 1, cs.shape[0], dtype=torch.long)
    for tl in range(out.shape[0]):
        rays = (tile == tl).nonzero()[:, 0]
        ks = listed[rays[0]].nonzero()[:, 0] if rays.numel() else rays
        if ks.numel() == 0:
            continue
        r = rays[:, None, None].expand(-1, cs.shape[0], ks.shape[0]).reshape(-1)
        c = cs[None, :, None].expand(rays.shape[0], -1, ks.shape[0]).reshape(-1)
        k = ks[None, None, :].expand(rays.shape[0], cs.shape[0], -1).reshape(-1)
        trmin, trmax = _slab_pairs(P[r, c].double(), st["rd"][r], st["pos"][k], st["rot"][k], st["scl"][k])
        skip = (trmax < -2.0 * dt) | (trmin > c_end + 2.0 * dt) | (trmin > trmax + 4.0 * dt)
        alive = live[r] & (T[r, c].double() <= thr[r])
        keep = (alive & ~skip).reshape(rays.shape[0], cs.shape[0], ks.shape[0]).any(0)
        out[tl] = keep.sum(-1)
    return out
