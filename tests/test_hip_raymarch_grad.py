"""The differentiable ray marcher on the MI355X: `primx_raymarch_backward` against the float64 autograd of
tests/raymarch_grad_ref.py, the autograd surface of `mvpraymarch` / `RayMarcher.train()`, the adjoint identity at the shipped
step, a descent run with `ops.adam_step`, and the footprint and stream-order cases of the entry point.

The backward adds with fp32 atomics, so its sums are not bitwise reproducible in general; each gradient is compared per tensor,
relative to the tensor's largest entry, with 4 x the distance of the SAME restatement run in float32 on the CPU from the float64
one (the fp32 floor of this arithmetic; the margin covers the arrival order of the atomics and the 2^-22 fast exp2 / log2).
tests/test_raymarch_grad_cpu.py asserts, without a GPU, that every scene here keeps every decision at least 1e-5 from its
threshold, so no comparison can hide a flipped sample.  The rays are the CPU oracle's (tests/raymarch_scenes.rays), uploaded:
the device marches exactly the rays the margins were checked on.

The module imports without a GPU: it registers its stream-order case in the table of tests/test_hip_streams.py at import (that
file stays as it is) and runs it here, like tests/test_hip_primsdf_grad.py does.
"""
import functools

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import raymarch_grad_ref as G
from tests import raymarch_scenes as sc
from tests import streamorder as so
from tests import test_hip_streams as TS
from tests.test_hip_primsdf_grad import E  # noqa: F401  (one side stream of its own, destroyed at teardown: see that module)
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-5                  # 10 x DELTA_Y of tests/raymarch_replay.py
NAMES = ("gtemplate", "gpos", "grot", "gscale")

# name -> (scene kwargs, step, fadescale, template extent (TD, TH, TW) cut out of the S^3 one or None).  The seeds were chosen so that
# every decision of the scene keeps MARGIN (tests/test_raymarch_grad_cpu.py::test_gpu_scenes_keep_their_decision_margins).
SCENES = {
    "rotated_sat": (dict(seed=5, K=24, H=20, W=18, dist=3.0, half=(0.08, 0.2), opacity=60.0), 0.02, 8.0, None),
    "rotated_sat_hard": (dict(seed=5, K=24, H=20, W=18, dist=3.0, half=(0.08, 0.2), opacity=60.0), 0.02, 0.0, None),
    "unsaturated": (dict(seed=2, K=24, H=12, W=10, dist=3.0, opacity=0.5), 0.02, 8.0, None),
    "ragged_batch2": (dict(seed=5, N=2, K=6, H=13, W=27, dist=3.0, spread=0.5, half=(0.04, 0.1)), 0.02, 8.0, None),
    "noncubic": (dict(seed=1, K=12, S=5, H=9, W=11, dist=3.0, half=(0.1, 0.25)), 0.02, 8.0, (3, 4, 5)),
    "cache_overflow": (dict(seed=16, K=90, H=8, W=8, dist=3.0, spread=0.004, half=(0.2, 0.3), rotate=False, thin=0.004, opacity=0.5,
                            focal=5.0), 0.004, 0.0, None),
    "hitlist_cap": (dict(seed=16, K=900, H=8, W=8, dist=3.0, spread=0.35, half=(0.2, 0.35), opacity=0.5, focal=0.6, rotate=False,
                         thin=0.004), 0.01, 8.0, None),
}


def build_scene(name):
    """-> dict of CPU fp32 tensors: the rays of the CPU oracle, the primitives, the template, the seeded normal gout."""
    kw, dt, fs, cut = SCENES[name]
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(**kw)
    if cut is not None:
        tpl = tpl[:, :, :cut[0], :cut[1], :cut[2]].contiguous()
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, kw["H"], kw["W"])
    gout = torch.randn(rp.shape[0], kw["H"], kw["W"], 4, generator=torch.Generator().manual_seed(1000 + kw["seed"]))
    return dict(rp=rp, rd=rd, tm=tm, dt=dt, pos=pos, rot=rot, scale=scale, tpl=tpl, gout=gout, fs=fs, fe=8.0)


def reference(s, gout=None):
    """float64 autograd, and per tensor (4 x the fp32 restatement's distance from it, largest entry)."""
    gout = s["gout"] if gout is None else gout
    args = (s["rp"], s["rd"], s["tm"], s["dt"], s["pos"], s["rot"], s["scale"], s["tpl"], gout, s["fs"], s["fe"])
    g64, img, info = G.grads(*args, dtype=torch.float64)
    g32, _, _ = G.grads(*args, dtype=torch.float32)
    tol = {}
    for name, a64, a32 in zip(NAMES, g64, g32):
        top = float(a64.abs().max())
        tol[name] = (4 * float((a32.double() - a64).abs().max()), top)
    return dict(zip(NAMES, g64), tol=tol, img=img, info=info)


@functools.lru_cache(maxsize=None)
def _case(name):
    s = build_scene(name)
    return s, reference(s)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import _lib, ops, raymarch
    return type("Mods", (), dict(lib=_lib.load(), ops=ops, rm=raymarch))


def _gpu(mods, s, gout=None, **kw):
    d = lambda t: t.to(DEV)
    return mods.rm.raymarch_backward(d(s["rp"]), d(s["rd"]), s["dt"], d(s["tm"]), (d(s["pos"]), d(s["rot"]), d(s["scale"])), d(s["tpl"]),
                                     d(s["gout"] if gout is None else gout), s["fs"], s["fe"], **kw)


def _compare(tag, r, got, scale=1.0):
    worst = 0.0
    for name, g in zip(NAMES, got):
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), (tag, name)
        tol, top = r["tol"][name]
        err = float((g.cpu().double() - scale * r[name]).abs().max())
        ratio = err / max(scale * tol, 1e-300)
        worst = max(worst, ratio)
        print(f"{tag} {name}: max-abs error {err:.3e} = {err / max(scale * top, 1e-300):.2e} of the largest entry {scale * top:.3e}; "
              f"fp32 floor {tol / 4 / max(top, 1e-300):.2e} of it; error / (4 x floor) = {ratio:.3f}")
        assert top > 0 and err <= scale * tol, (tag, name, err, scale * tol)
    return worst


# ------------------------------------------------------------------------------------------------ 1. kernel vs float64 autograd
@pytest.mark.parametrize("name", list(SCENES))
def test_backward_matches_float64_autograd(mods, name):
    s, r = _case(name)
    i = r["info"]
    print(f"{name}: {i['taken']} samples (at most {i['samples']} per ray), {i['hit']} rays with samples, {i['saturated']} saturated, "
          f"margins {i['margin']}")
    assert min(i["margin"].values()) >= MARGIN
    _compare(name, r, _gpu(mods, s))


# ------------------------------------------------------------------------------------------------ 2. the autograd surface
def _dev_scene(s, grad=()):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in s.items()}
    for k in grad:
        d[k] = d[k].clone().requires_grad_(True)
    return d


def _march(mods, d):
    return mods.rm.mvpraymarch(d["rp"], d["rd"], d["dt"], d["tm"], (d["pos"], d["rot"], d["scale"]), d["tpl"], d["fs"], d["fe"])


def test_mvpraymarch_under_grad_is_the_same_image_and_fills_exactly_the_wanted_grads(mods):
    s, r = _case("rotated_sat")
    with torch.no_grad():
        plain = _march(mods, _dev_scene(s, grad=("tpl", "pos")))
    assert plain.grad_fn is None and not plain.requires_grad
    assert _march(mods, _dev_scene(s)).grad_fn is None                  # nothing requires a gradient: today's path
    d = _dev_scene(s, grad=("tpl", "pos", "rot", "scale"))
    img = _march(mods, d)
    assert img.grad_fn is not None and torch.equal(img.detach(), plain)
    (img * d["gout"]).sum().backward()
    _compare("autograd, all four", r, (d["tpl"].grad, d["pos"].grad, d["rot"].grad, d["scale"].grad))
    d = _dev_scene(s, grad=("pos", "scale"))
    img = _march(mods, d)
    assert torch.equal(img.detach(), plain)
    (img * d["gout"]).sum().backward()
    assert d["tpl"].grad is None and d["rot"].grad is None
    _compare("autograd, pos and scale", r, (None, d["pos"].grad, None, d["scale"].grad))


def test_want_and_accumulators(mods):
    s, r = _case("unsaturated")
    gt, gp, gr, gs = _gpu(mods, s, want=(True, False, False, True))
    assert gp is None and gr is None
    _compare("want template, scale", r, (gt, None, None, gs))
    own = torch.full_like(s["rot"], 0.5).to(DEV)
    sentinel = torch.full_like(s["pos"], 7.0).to(DEV)                   # not wanted: must stay untouched even when passed
    gt, gp, gr, gs = _gpu(mods, s, want=(False, False, True, False), grot=own, gpos=sentinel)
    assert gt is None and gp is None and gs is None and gr is own and bool((sentinel == 7.0).all())
    shifted = dict(r, grot=r["grot"] + 0.5)
    ulp = float(np.finfo(np.float32).eps)
    shifted["tol"] = dict(r["tol"], grot=(r["tol"]["grot"][0] + ulp * (r["tol"]["grot"][1] + 0.5), r["tol"]["grot"][1]))
    _compare("pre-filled grot", shifted, (None, None, own, None))
    # a second call into the caller's accumulators: the sum of the two
    acc = _gpu(mods, s)
    again = _gpu(mods, s, gtemplate=acc[0], gpos=acc[1], grot=acc[2], gscale=acc[3])
    assert all(a is b for a, b in zip(acc, again))
    _compare("two calls", r, again, scale=2.0)
    with pytest.raises(RuntimeError, match="no gradient is wanted"):
        _gpu(mods, s, want=(False, False, False, False))


def test_zero_gout_leaves_exact_zeros(mods):
    s, _ = _case("rotated_sat")
    for g in _gpu(mods, s, gout=torch.zeros_like(s["gout"])):
        assert int((g != 0).sum()) == 0
    half = s["gout"].clone()
    half[:, :, 9:] = 0                                                  # whole tiles and part of a tile without a gradient
    r = reference(s, half)
    _compare("gout zero right of column 9", r, _gpu(mods, s, gout=half))


def test_raymarcher_trains_with_ray_subsampling(mods):
    """RayMarcher(...).train() with ray_subsample_factor = 2: runs, renders the subsampled rays and back-propagates to prim_rgba and
    prim_pos through the permute to channels-last and the division by volradius."""
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(seed=21, N=2, K=8, H=16, W=16, dist=3.0)
    vr = 100.0
    Rt = torch.cat([cr, -torch.einsum("nij,nj->ni", cr, cp * vr)[..., None]], -1)          # c = -R^T t
    Kmat = torch.zeros(2, 3, 3)
    Kmat[:, 0, 0], Kmat[:, 1, 1], Kmat[:, :2, 2], Kmat[:, 2, 2] = f[:, 0], f[:, 1], pp, 1.0
    m = mods.rm.RayMarcher(16, 16, vr, dt=2.0, ray_subsample_factor=2).train()
    rgba = tpl.permute(0, 1, 5, 2, 3, 4).contiguous().to(DEV).requires_grad_(True)           # [B, K, 4, S, S, S]
    ppos = (pos * vr).to(DEV).requires_grad_(True)
    torch.manual_seed(3)
    out = m(rgba, ppos, rot.to(DEV), scale.to(DEV), Kmat.to(DEV), Rt.to(DEV))
    img = out["rgba_image"]
    assert tuple(img.shape) == (2, 4, 8, 8) and tuple(out["pixel_coords"].shape) == (2, 8, 8, 2) and img.grad_fn is not None
    assert float(img.detach()[:, 3].max()) > 0
    gout = torch.randn(img.shape, generator=torch.Generator().manual_seed(4)).to(DEV)
    (img * gout).sum().backward()
    assert rgba.grad.shape == rgba.shape and ppos.grad.shape == ppos.shape
    assert bool(torch.isfinite(rgba.grad).all()) and bool(torch.isfinite(ppos.grad).all())
    assert float(rgba.grad.abs().max()) > 0 and float(ppos.grad.abs().max()) > 0
    # the same through raymarch_backward on the marcher's own operands: channels-last gradient permuted back, gpos / volradius
    rp, rd, tm = mods.rm.compute_raydirs(cp.to(DEV) * vr, cr.to(DEV), f.to(DEV), pp.to(DEV), out["pixel_coords"], vr)
    gt, gp, _, _ = mods.rm.raymarch_backward(rp, rd, 2.0 / vr, tm, (ppos.detach() / vr, rot.to(DEV), scale.to(DEV)),
                                             rgba.detach().permute(0, 1, 3, 4, 5, 2), gout.permute(0, 2, 3, 1), want=(True, True, False, False))
    top_t, top_p = float(gt.abs().max()), float(gp.abs().max())
    assert float((rgba.grad - gt.permute(0, 1, 5, 2, 3, 4)).abs().max()) <= 1e-4 * top_t       # two atomic-order runs of one sum
    assert float((ppos.grad * vr - gp).abs().max()) <= 1e-4 * top_p
    m.eval()
    with torch.no_grad():
        assert tuple(m(rgba, ppos, rot.to(DEV), scale.to(DEV), Kmat.to(DEV), Rt.to(DEV))["rgba_image"].shape) == (2, 4, 8, 8)


# ------------------------------------------------------------------------------------------------ 3. the shipped step
def test_adjoint_identity_at_the_shipped_step(mods):
    """dt = 1e-4 (chunks, step windows and the record cache all in play).  With gout.a = 0 and fixed decisions the image's rgb is
    linear in the template's rgb: image.rgb = sum over taken samples of weight_i w_c tpl.rgb_c, and gtemplate.rgb_c = sum weight_i w_c
    gout.rgb, so <gout.rgb, image.rgb> = <gtemplate.rgb, template.rgb>.  Both sides are fp32 sums of the same products, each rounded
    a few times and accumulated along a ray's n taken samples: |difference| <= n 2^-23 (sum |gout.rgb image.rgb| + sum |gtemplate.rgb
    template.rgb|), n = the largest number of taken samples of a ray (counted by the replay)."""
    from tests import raymarch_replay as rr
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(seed=1, N=1, K=16, H=10, W=12, dist=3.0)
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, 10, 12)
    gout = torch.randn(1, 10, 12, 4, generator=torch.Generator().manual_seed(8))
    gout[..., 3] = 0
    s = dict(rp=rp, rd=rd, tm=tm, dt=1e-4, pos=pos, rot=rot, scale=scale, tpl=tpl, gout=gout, fs=8.0, fe=8.0)
    img = _march(mods, _dev_scene(s)).cpu().double()
    grads = _gpu(mods, s)
    for g in grads:
        assert bool(torch.isfinite(g).all())
    _, _, st = rr.replay(rp, rd, tm, 1e-4, pos, rot, scale, tpl, 8.0, 8.0, device=DEV, with_stats=True)
    n = int(torch.bincount(st["windows"][0]["er"]).max())
    lhs_terms = gout[..., :3].double() * img[..., :3]
    rhs_terms = grads[0].cpu().double()[..., :3] * tpl[..., :3].double()
    lhs, rhs = float(lhs_terms.sum()), float(rhs_terms.sum())
    bound = n * 2.0 ** -23 * (float(lhs_terms.abs().sum()) + float(rhs_terms.abs().sum()))
    print(f"shipped step: {st['samples']} samples, at most {n} per ray; <gout, image> = {lhs:.9e}, <gtemplate, template> = {rhs:.9e}, "
          f"|difference| / bound = {abs(lhs - rhs) / bound:.4f}")
    assert n > 1000 and abs(lhs) > 0 and abs(lhs - rhs) <= bound


# ------------------------------------------------------------------------------------------------ 4. descent
def test_adam_descends_on_a_perturbed_template(mods):
    tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(seed=9, N=1, K=8, H=16, W=16, dist=3.0)
    _, (rp, rd, tm) = sc.rays(cp, cr, f, pp, 16, 16)
    d = _dev_scene(dict(rp=rp, rd=rd, tm=tm, dt=0.02, pos=pos, rot=rot, scale=scale, tpl=tpl, fs=8.0, fe=8.0))
    target = _march(mods, d)
    param = (d["tpl"] + 0.3 * torch.randn(tpl.shape, generator=torch.Generator().manual_seed(10)).to(DEV)).clamp(min=0).contiguous()
    m, v = torch.zeros_like(param), torch.zeros_like(param)
    losses = []
    for t in range(1, 11):
        p = param.detach().requires_grad_(True)
        loss = (_march(mods, dict(d, tpl=p)) - target).pow(2).mean()
        loss.backward()
        losses.append(float(loss.detach()))
        mods.ops.adam_step(param, p.grad.contiguous(), m, v, t, lr=2e-2)
    with torch.no_grad():
        losses.append(float((_march(mods, dict(d, tpl=param)) - target).pow(2).mean()))
    print("descent, loss per step:", " ".join(f"{x:.4e}" for x in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 5. footprint and stream order
def test_footprint_of_the_backward(mods):
    """Inside footprint.guarded under both fills: nothing is written outside the four gradient arrays (their guards, and the guards
    and contents of every const operand, are intact), nothing bypasses the wrapper, and the results do not depend on the fill -
    within the gradient tolerance, since the sums are atomic."""
    s, r = _case("ragged_batch2")
    for fill in fp.FILLS:
        with fp.guarded(fill) as g:
            d = {k: (g.guard_input(v.to(DEV), k).t if torch.is_tensor(v) else v) for k, v in s.items()}
            got = mods.rm.raymarch_backward(d["rp"], d["rd"], d["dt"], d["tm"], (d["pos"], d["rot"], d["scale"]), d["tpl"], d["gout"],
                                            d["fs"], d["fe"])                                   # (zeros_like inside the package: guarded)
            own = g.guard_input(torch.zeros_like(s["pos"]).to(DEV), "gpos", const=False).t       # a caller's own accumulator
            mods.rm.raymarch_backward(d["rp"], d["rd"], d["dt"], d["tm"], (d["pos"], d["rot"], d["scale"]), d["tpl"], d["gout"],
                                      d["fs"], d["fe"], gpos=own, want=(False, True, False, False))
            assert len(g.records) >= 13 and not g.bypassed
        _compare(f"fill {fill:#04x}", r, got)
        _compare(f"fill {fill:#04x}, own gpos", r, (None, own, None, None))


@TS.case("raymarch_backward", ["primx_raymarch_backward"])
def _stream_raymarch_backward(E, dtype):  # noqa: F811
    """The stream check compares bit for bit, so the scene is reproducible: an N x 1 x 1 image, N = 3 - one valid ray per batch item
    (the other 63 lanes of its 8 x 8 tile are shadow lanes and add nothing) marching a few hundred samples at dt = 0.002.  Every
    gradient address then receives its adds from a single lane in program order (the template's from the ray's lane, the SRT's from
    lane 0), and the wave sums in front of the SRT adds have a fixed order."""
    from topia_xl_amd import raymarch

    def make(k):
        tpl, pos, rot, scale, cp, cr, f, _ = sc.scene(seed=40 + k, N=3, K=24, H=1, W=1, dist=3.0, spread=0.3, half=(0.15, 0.3), yaw=(0.3, -0.8, 1.9))
        _, (rp, rd, tm) = sc.rays(cp, cr, f, torch.zeros(3, 2), 1, 1)                        # pixel (0, 0) is the principal point
        gout = torch.randn(3, 1, 1, 4, generator=torch.Generator().manual_seed(50 + k))
        return {n: t.to(DEV).contiguous() for n, t in dict(rp=rp, rd=rd, tm=tm, pos=pos, rot=rot, scale=scale, tpl=tpl, gout=gout).items()}

    def call(ctx, i, probe):
        return list(raymarch.raymarch_backward(i["rp"], i["rd"], 0.002, i["tm"], (i["pos"], i["rot"], i["scale"]), i["tpl"], i["gout"]))
    return make, call, None


STREAM_CASES = ("raymarch_backward",)


@pytest.mark.parametrize("name", STREAM_CASES)
def test_stream_order_of_the_backward(E, called, name):  # noqa: F811  (`E`, `called` are the imported fixtures)
    """The body of tests/test_hip_streams.py::test_stream_order for the case registered above; no host synchronisation is documented."""
    c = TS.CASES[name]
    make, call, setup = c.build(E, None)
    rep = so.run(name, make, call, E.S, E.blocker, setup=setup, must_sync=False)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{name} declares entry points it did not call: {missing}"
