"""`primx_compute_raydirs` on the MI355X against tests/raydirs_ref.py: every element inside the rigorous enclosure of a correct fp32
evaluation, the exact classes of the slab test with no tolerance, the null-`pixelcoords` path of the C ABI, and the generator's rays
handed to the marcher without a mask.  tests/test_raydirs_cpu.py proves the yardstick, the cameras' guards and the injected faults
without a GPU.  Finite cameras only; the rays of the face camera (`axis_on_face`: tmax = -inf or tmin = +inf) are never marched.

Not repeated here: the memory footprint of the entry point (tests/test_hip_footprint.py::test_raymarch_footprint runs
`compute_raydirs` under both fills with guarded operands on nine scenes, ragged 13 x 27 and batch 2 among them) and its stream order
(the `raymarch` case of tests/test_hip_streams.py declares `primx_compute_raydirs`).
"""
import functools

import numpy as np
import pytest
import torch

from tests import raydirs_ref as rr
from tests import raymarch_replay as replay
from tests import raymarch_scenes as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = 1e-4                      # the shipped step (tests/test_raymarch_contract.py)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import _lib, ops, raymarch
    return type("Mods", (), dict(lib=_lib.load(), ops=ops, rm=raymarch))


@functools.lru_cache(maxsize=None)
def _yard(name):
    c = rr.case(name)
    ops = rr.operands(c)
    return c, ops, rr.bound(*ops), rr.classes(*ops)


def _device_rays(mods, c, pixelcoords=None):
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pc = c["pixelcoords"] if pixelcoords is None else pixelcoords
    return mods.rm.compute_raydirs(D(c["viewpos"]), D(c["viewrot"]), D(c["focal"]), D(c["princpt"]), D(pc), c["volradius"])


# ------------------------------------------------------------------------------------------------ 1. the kernel inside the enclosure
@pytest.mark.parametrize("name", list(rr.CASES))
def test_kernel_inside_the_enclosure_and_the_exact_classes(mods, name):
    c, ops, B, C = _yard(name)
    rp, rd, tm = (t.cpu().numpy() for t in _device_rays(mods, c))
    v, cv = rr.violations(B, rp, rd, tm), rr.class_violations(B, C, rp, rd, tm)
    unit = float(np.abs((rd.astype(np.float64) ** 2).sum(-1) - 1.0).max())
    same = rr.trange_of(rp, rd)
    moved = int((same != tm).any(-1).sum())
    print(f"{name} {tuple(tm.shape[:3])}: max |value - centre| / half-width {rr.share(B, rd, tm):.3f}; unit-length residual "
          f"{unit / rr.UNIT_RESIDUAL:.3f} of its bound; classes {rr.population(C)}; non-finite t values {int((~np.isfinite(tm)).sum())}, "
          f"NaN {int(np.isnan(tm).sum())}; outside {({k: int(m.sum()) for k, m in v.items()})}, classes broken "
          f"{({k: int(m.sum()) for k, m in cv.items()})}; pixels whose t-range is not the one of the kernel's own direction {moved}")
    assert not v["raypos"].any(), "raypos is not bit-exact"
    assert not v["raydir"].any(), int(v["raydir"].sum())
    assert not v["tminmax"].any(), int(v["tminmax"].sum())
    assert not v["unit"].any(), unit
    for k, m in cv.items():
        assert not m.any(), (k, int(m.sum()))
    assert not np.isnan(tm).any() and not np.isnan(rd).any()
    # finite for every pixel that is not of class (b) or (c)
    assert np.isfinite(tm[~(C["b"] | C["c"]).any(-1)]).all()
    # one correctly rounded division per candidate, of two fp32 values the test holds: the same VALUES (either zero for tmin)
    assert moved == 0, moved


# ------------------------------------------------------------------------------------------------ 2. the null pixelcoords pointer
def test_null_pixelcoords_is_the_integer_grid(mods):
    """The kernel takes px = w, py = h when `pixelcoords` is null - reachable through the C ABI only.  N = 2, 13 x 27 with two
    different cameras: bit-identical to the explicit grid, and nothing written past the three outputs."""
    c = rr.case("generic_batch3")
    N, H, W = 2, 13, 27
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    vp, rot, f, pp = D(c["viewpos"][:N]), D(c["viewrot"][:N]), D(c["focal"][:N]), D(c["princpt"][:N])
    n, pad, mark = N * H * W, 64, 12345.0
    outs = {}
    for tag, pc in (("null", None), ("grid", D(rr.pixel_grid(N, H, W)))):
        bufs = [torch.full((n * k + pad,), mark, dtype=torch.float32, device=DEV) for k in (3, 3, 2)]
        st = mods.lib.primx_compute_raydirs(vp.data_ptr(), rot.data_ptr(), f.data_ptr(), pp.data_ptr(), None if pc is None else pc.data_ptr(),
                                            float(c["volradius"]), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), N, H, W,
                                            mods.ops._stream())
        assert st == 0, mods.lib.primx_last_error()
        outs[tag] = [b.cpu().numpy() for b in bufs]
        for b, k in zip(outs[tag], (3, 3, 2)):
            assert (b[n * k:] == mark).all() and not (b[:n * k] == mark).any()
    for a, b in zip(outs["null"], outs["grid"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and it is the yardstick's grid: inside the enclosure of pixelcoords = None
    ops = (c["viewpos"][:N], c["viewrot"][:N], c["focal"][:N], c["princpt"][:N], None, c["volradius"])
    B = rr.bound(*ops, hw=(H, W))
    rp, rd, tm = (outs["null"][i][:n * k].reshape(N, H, W, k) for i, k in enumerate((3, 3, 2)))
    v = rr.violations(B, rp, rd, tm)
    assert not any(m.any() for m in v.values()), {k: int(m.sum()) for k, m in v.items()}
    via_host = [t.cpu().numpy() for t in _device_rays(mods, dict(c, viewpos=c["viewpos"][:N], viewrot=c["viewrot"][:N], focal=c["focal"][:N],
                                                                 princpt=c["princpt"][:N]), rr.pixel_grid(N, H, W))]
    for a, b in zip((rp, rd, tm), via_host):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. generator into marcher, no mask
def _prims(N, H, W, **kw):
    tpl, pos, rot, scale, *_ = sc.scene(N=N, K=16, H=H, W=W, **kw)
    return tpl, pos, rot, scale


@pytest.mark.parametrize("name", ["looking_away", "grazing"])
def test_missing_rays_march_to_exact_zeros_forward_and_backward(mods, name):
    """The generator's rays go to the marcher as they are.  A ray that misses the volume by more than the marcher's 1e-5 (every
    missing ray here, asserted) takes no sample: its pixel is an exact zero, and a loss that looks at such pixels only leaves exact
    zeros in all four gradients."""
    c, ops, B, C = _yard(name)
    N, H, W = c["pixelcoords"].shape[:3]
    rp, rd, tm = _device_rays(mods, c)
    t = tm.cpu()
    assert bool(torch.isfinite(t).all())
    miss = (t[..., 0] > t[..., 1]) | (t[..., 1] < 0)
    assert bool(((t[..., 0] - t[..., 1])[miss] > 1e-3).all())
    assert int(miss.sum()) >= 16 and (name == "looking_away") == bool(miss.all())
    tpl, pos, rot, scale = _prims(N, H, W, seed=21, spread=0.7, half=(0.15, 0.3), opacity=20.0)
    d = lambda x: x.to(DEV)
    img = mods.rm.mvpraymarch(rp, rd, DT, tm, (d(pos), d(rot), d(scale)), d(tpl), 8.0, 8.0).cpu()
    assert bool(torch.isfinite(img).all())
    assert bool((img[miss] == 0).all()), int((img[miss] != 0).any(-1).sum())
    if name == "grazing":
        assert float((img[~miss][..., 3] > 0).float().mean()) > 0.2          # the hitting rays of the same block do march
    gout = torch.randn(N, H, W, 4, generator=torch.Generator().manual_seed(5))
    gout[~miss] = 0.0
    grads = mods.rm.raymarch_backward(rp, rd, DT, tm, (d(pos), d(rot), d(scale)), d(tpl), d(gout), 8.0, 8.0)
    assert len(grads) == 4
    for nm, g in zip(("gtemplate", "gpos", "grot", "gscale"), grads):
        assert bool((g == 0).all()), (nm, int((g != 0).sum()))
    print(f"{name}: {int(miss.sum())} of {miss.numel()} rays miss; image and the four gradients exact zeros there")


MARCHED = [("inside", dict(seed=14, const=True, opacity=20.0), 0.0), ("principal_cross", dict(seed=18, rotate=False), 0.0)]


@pytest.mark.parametrize("name,kw,fs", MARCHED, ids=[m[0] for m in MARCHED])
def test_generated_rays_march_within_the_replay_bound(mods, name, kw, fs):
    """The check of test_hip_march_within_bound_at_shipped_step with THIS file's cameras on a 16 x 16 image, K = 16: the camera
    inside the volume (tmin = 0 exactly) and the cameras whose principal row and column hold exact-zero components (slab times of
    +-inf inside the marcher's own per-primitive test).  The replay marches the device's rays; no pixel may exceed its bound."""
    c, ops, B, C = _yard(name)
    N, H, W = c["pixelcoords"].shape[0], 16, 16
    pc = np.ascontiguousarray(c["pixelcoords"][:, :H, :W])
    assert pc.shape == (N, H, W, 2)
    rp, rd, tm = _device_rays(mods, c, pc)
    assert bool(torch.isfinite(tm).all()) and bool(torch.isfinite(rd).all())
    if name == "principal_cross":
        assert int((rd == 0).sum()) >= 16 * 4
    tpl, pos, rot, scale = _prims(N, H, W, **kw)
    d = lambda x: x.to(DEV)
    img = mods.rm.mvpraymarch(rp, rd, DT, tm, (d(pos), d(rot), d(scale)), d(tpl), fs, 8.0).cpu().double()
    ex, bd, st = replay.replay(rp.cpu(), rd.cpu(), tm.cpu(), DT, pos, rot, scale, tpl, fs, 8.0, device=DEV)
    err = (img - ex).abs()
    bad = err > bd
    a = ex[..., 3]
    print(f"{name}: {st['samples']} samples, {st['steps']} steps, coverage {float((a > 0).float().mean()):.2f}; max err "
          f"{float(err.max()):.3e}, largest bound share {float((err / bd.clamp(min=1e-30)).max()):.3f}, pixels over bound "
          f"{int(bad.any(-1).sum())}")
    assert torch.isfinite(img).all() and torch.isfinite(ex).all() and torch.isfinite(bd).all()
    assert float((a > 0).float().mean()) > 0.02
    assert not bool(bad.any()), (int(bad.any(-1).sum()), float(err.max()))
