"""Ray marcher at the shipped step (1e-4 of the volume: RayMarcher(volradius=10000, dt=1)) against an unfiltered float64
replay of its semantics with a derived per-pixel bound (tests/raymarch_replay.py).  At that step a ray takes ~10^4
steps and the kernel's chunk filter, per-ray step windows, LDS record cache and hit-list cap are all in play; the replay
has none of them, so every pixel within its bound means the filters drop nothing the unfiltered loop takes."""
import numpy as np
import pytest
import torch

from oracle import raymarch_ref
from tests import raymarch_replay as rr
from tests import raymarch_scenes as sc

DEV = "cuda:0"
DT = 1e-4


def test_replay_matches_reference_pytorch_loop(golden):
    """The replay == the reference's own torch march loop (tests/golden/raymarch.npz, 18 steps, 64 primitives)."""
    g = golden("raymarch")
    T = lambda k: torch.from_numpy(g[k])[:1]
    tpl = T("march_template").permute(0, 1, 3, 4, 5, 2).contiguous()
    ex, bd, st = rr.replay(T("march_raypos"), T("march_raydir"), T("march_tminmax"), float(g["march_stepsize"]),
                           T("march_primpos"), T("march_primrot"), T("march_primscale"), tpl,
                           float(g["march_fadescale"]), float(g["march_fadeexp"]))
    ref = T("march_rgba").double()
    assert float(ref[..., 3].min()) > 0.5
    assert float((ex - ref).abs().max()) < 1e-5, float((ex - ref).abs().max())
    assert float(bd.max()) < 2e-3                      # the bound stays far below a visible difference


def test_replay_matches_oracle_loop():
    """The replay == oracle/raymarch_ref (the dense torch restatement) on the dt = 0.02 scene of test_raymarch.py."""
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(seed=3, N=1, K=24, H=20, W=18, dist=3.0)
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, 20, 18)
    ex, bd, _ = rr.replay(rp, rd, tm, 0.02, pos, rot, scale, tpl, 8.0, 8.0)
    ref = raymarch_ref.raymarch(rp, rd, tm, 0.02, pos, rot, scale, tpl, 8.0, 8.0).double()
    assert float(ref[..., 3].max()) > 0.99 and float((ref[..., 3] > 0).float().mean()) > 0.2
    err = (ex - ref).abs()
    # the oracle steps rp with fl(rp + rd dt) and tests |y| < 1 without a band: it may differ where the replay's bound says
    assert bool((err <= bd + 1e-6).all()), float((err - bd).max())


def test_window_from_t_misses_samples_at_shipped_step():
    """The hazard without a GPU: t and rp are accumulated separately in fp32; with t in [2, 4) (camera 3 volume radii
    away) t += 1e-4 advances 419 ulps instead of 419.43, so a step window placed with ro + t rd falls behind the actual
    samples rp by more than its 2-step margin within ~8000 steps, while a window measured from rp keeps them all."""
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(seed=1, N=1, K=16, H=10, W=12, dist=3.0)
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, 10, 12)
    _, _, st = rr.replay(rp, rd, tm, DT, pos, rot, scale, tpl, 0.0, 8.0, with_stats=True)
    w = st["windows"][0]
    miss_t, gap_t = rr.window_misses(w, DT)
    miss_rp, gap_rp = rr.window_misses(w, DT, from_rp=True)
    print(f"window from t: {miss_t} samples missed (largest gap {gap_t:.0f} steps); from rp: {miss_rp}")
    assert miss_t > 0 and miss_rp == 0


# (name, scene kwargs, fadescale): each aims at one part of the kernel
CASES = [
    ("far_t_lags_fade8", dict(seed=11, K=40, H=24, W=20, dist=3.0), 8.0),
    ("far_t_lags_hard", dict(seed=12, K=40, H=24, W=20, dist=3.0), 0.0),
    ("near_t_leads_hard", dict(seed=13, K=40, H=20, W=21, dist=1.5), 0.0),
    ("inside_volume_const", dict(seed=14, K=40, H=19, W=22, dist=0.9, const=True, opacity=20.0), 0.0),
    ("cache_overflow", dict(seed=15, K=90, H=8, W=8, dist=3.0, spread=0.004, half=(0.2, 0.3), rotate=False, thin=0.004,
                            opacity=0.5), 0.0),
    ("hitlist_cap", dict(seed=16, K=900, H=8, W=8, dist=3.0, spread=0.35, half=(0.2, 0.35), opacity=0.5, focal=0.6,
                         rotate=False, thin=0.004), 8.0),
    ("ragged_sparse", dict(seed=17, K=6, H=13, W=27, dist=3.0, spread=0.5, half=(0.04, 0.1)), 0.0),
    ("axis_aligned", dict(seed=18, K=30, H=17, W=17, dist=3.0, rotate=False, axis=True, face_on_axis=True), 0.0),
    ("batch2", dict(seed=19, N=2, K=30, H=16, W=18, dist=2.5, yaw=(0.4, -1.1)), 0.0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,fs", CASES, ids=[c[0] for c in CASES])
def test_hip_march_within_bound_at_shipped_step(name, kw, fs):
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import raymarch as rm
    kw = dict(kw)
    N, H, W = kw.get("N", 1), kw["H"], kw["W"]
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(**kw)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xs, ys], -1)[None].expand(N, -1, -1, -1).contiguous()
    rp, rd, tm = rm.compute_raydirs(cp.to(DEV), cr.to(DEV), f.to(DEV), pp.to(DEV), pc.to(DEV), 1.0)
    img = rm.mvpraymarch(rp, rd, DT, tm, (pos.to(DEV), rot.to(DEV), scale.to(DEV)), tpl.to(DEV), fs, 8.0).cpu().double()
    # the replay marches the DEVICE's rays, so what is compared is the march, not the ray generator
    ex, bd, st = rr.replay(rp.cpu(), rd.cpu(), tm.cpu(), DT, pos, rot, scale, tpl, fs, 8.0, device=DEV)
    err = (img - ex).abs()
    share = float((err / bd.clamp(min=1e-30)).max())
    bad = err > bd
    a = ex[..., 3]
    print(f"{name}: {st['samples']} samples, {st['steps']} steps, coverage {float((a > 0).float().mean()):.2f}, "
          f"saturated {float((a >= 1 - 1e-6).float().mean()):.2f}; max err {float(err.max()):.3e}, largest bound share "
          f"{share:.3f}, pixels over bound {int(bad.any(-1).sum())}")
    assert torch.isfinite(img).all() and torch.isfinite(ex).all() and torch.isfinite(bd).all()
    assert float((a > 0).float().mean()) > 0.02
    assert not bool(bad.any()), (int(bad.any(-1).sum()), float(err.max()), share)


def test_scenes_reach_their_targets():
    """Guards of the GPU scenes (CPU only, geometry): the far camera puts t in [2, 4), the near one in [1, 2), the inside
    one clamps tmin to 0; the cap scene hits > 512 primitives from one tile; the ragged scene has rays without hits in
    tiles with hits; the axis-aligned scene has zero components in r1 and rays lying exactly in a face plane."""
    def geo(name):
        kw = dict(next(c[1] for c in CASES if c[0] == name))
        tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(**kw)
        _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, kw["H"], kw["W"])
        trmin, trmax = rr._slab(rp[0].reshape(-1, 3).double(), rd[0].reshape(-1, 3).double(), pos[0].double(),
                                rot[0].double(), scale[0].double())
        return tm[0].reshape(-1, 2), trmin, trmax, rd[0].reshape(-1, 3)
    tm, trmin, trmax, _ = geo("far_t_lags_hard")
    hit = trmin <= trmax
    first = torch.where(hit, trmin, torch.full_like(trmin, float("inf"))).amin(1)
    assert float(first[torch.isfinite(first)].min()) >= 2.0
    tm, trmin, trmax, _ = geo("near_t_leads_hard")
    first = torch.where(trmin <= trmax, trmin, torch.full_like(trmin, float("inf"))).amin(1)
    assert float(first[torch.isfinite(first)].max()) < 2.0 and float(first[torch.isfinite(first)].min()) >= 0.5
    tm, _, _, _ = geo("inside_volume_const")
    assert bool((tm[:, 0] == 0).all())
    _, trmin, trmax, _ = geo("hitlist_cap")
    assert int((trmin <= trmax).any(0).sum()) > 512
    _, trmin, trmax, _ = geo("ragged_sparse")
    hit = trmin <= trmax
    assert bool(hit.any()) and not bool(hit.any(1).all())
    _, trmin, trmax, rd = geo("axis_aligned")
    assert bool((rd == 0).any())


def test_cache_overflow_scene_overflows_the_record_cache():
    """The chunk sub-list of one tile holds more than NREC = 64 primitives in some 96-step chunk, counted as the kernel
    builds it (skip test from rp at the chunk start, union over the tile's live rays), so the uncached fallback runs."""
    kw = dict(next(c[1] for c in CASES if c[0] == "cache_overflow"))
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(**kw)
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, kw["H"], kw["W"])
    ex, _, st = rr.replay(rp, rd, tm, DT, pos, rot, scale, tpl, 0.0, 8.0, with_stats=True)
    assert float(ex[..., 3].max()) < 0.99                     # no saturated ray: chunk_sublists' liveness is exact
    subs = rr.chunk_sublists(st["windows"][0], DT)
    print(f"largest chunk sub-list {int(subs.max())}, chunks over 64: {int((subs > 64).sum())}")
    assert int(subs.max()) > 64


def test_rays_in_a_face_plane_never_reach_the_unordered_window():
    """The axis-aligned scene's centre column lies exactly in a face plane of primitives 0 and 1 (r1.x = 0, r0.x = -1 /
    +1).  One slab bound is then 0 * inf = NaN, but fminf / fmaxf drop a lone NaN and the other bound is +-inf, so trmin /
    trmax come out ordered: such a ray misses the box (it is not strictly inside), and the kernel's 0xff00 'always'
    window, kept for non-finite inputs, is not reached by finite ones."""
    kw = dict(next(c[1] for c in CASES if c[0] == "axis_aligned"))
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(**kw)
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, kw["H"], kw["W"])
    ro, d = rp[0].reshape(-1, 3).double(), rd[0].reshape(-1, 3).double()
    on = (d[:, 0] == 0) & (ro[:, 0] == 0)
    assert int(on.sum()) == kw["H"]
    r0 = rr._local(ro[on][:, None, :], pos[0, :2].double()[None], rot[0, :2].double()[None], scale[0, :2].double()[None])
    assert bool((r0[..., 0].abs() == 1).all())
    trmin, trmax = rr._slab(ro[on], d[on], pos[0, :2].double(), rot[0, :2].double(), scale[0, :2].double())
    assert not bool(torch.isnan(trmin).any() or torch.isnan(trmax).any())
    assert not bool((trmin <= trmax).any())
    # the replay of this scene (samples in the face plane, local coordinates exactly 0) has a finite value and bound
    ex, bd, st = rr.replay(rp, rd, tm, DT, pos, rot, scale, tpl, 0.0, 8.0)
    assert bool(torch.isfinite(ex).all() and torch.isfinite(bd).all()) and st["ambiguous"] > 0
