"""The yardstick of tests/test_hip_raydirs.py, proved without a GPU: the numpy restatement of the ray generator and its enclosure
(tests/raydirs_ref.py) against each other, against the reference's own PyTorch outputs (tests/golden/raymarch.npz), against every
injected fault and against oracle/raymarch_ref.compute_raydirs; the guards of the cameras; and the host plumbing in front of the
kernel (RayMarcher._pixel_coords, training_pixel_coords, convert_camera_parameters) on CPU tensors."""
import functools

import numpy as np
import pytest
import torch

from oracle import raymarch_ref
from tests import raydirs_ref as rr

NAMES = list(rr.CASES)


@functools.lru_cache(maxsize=None)
def _case(name):
    c = rr.case(name)
    ops = rr.operands(c)
    return c, ops, rr.bound(*ops), rr.classes(*ops), rr.rays(*ops, dtype=np.float64), rr.rays(*ops, dtype=np.float32)


def _count(masks):
    return {k: int(v.sum()) for k, v in masks.items()}


def _failures(name, fault):
    """-> (number of elements outside the enclosure, number of pixels breaking a class, tminmax mask) of the faulty fp32 restatement."""
    c, ops, B, C, _, _ = _case(name)
    got = rr.rays(*ops, dtype=np.float32, fault=fault)
    v, cv = rr.violations(B, *got), rr.class_violations(B, C, *got)
    return sum(_count(v).values()), sum(_count(cv).values()), v


# ------------------------------------------------------------------------------------------------ restatement inside its bound
@pytest.mark.parametrize("name", NAMES)
def test_fp32_restatement_lies_inside_the_bound_of_the_float64_one(name):
    c, ops, B, C, r64, r32 = _case(name)
    for tag, (rp, rd, tm) in (("fp32", r32), ("float64", r64)):
        v = rr.violations(B, r32[0], rd, tm)                      # raypos is fp32 by contract (class e)
        cv = rr.class_violations(B, C, r32[0], rd, tm)
        assert not any(_count(v).values()), (name, tag, _count(v))
        assert not any(_count(cv).values()), (name, tag, _count(cv))
    print(f"{name}: fp32 restatement at {rr.share(B, r32[1], r32[2]):.3f} of the half-width; classes {rr.population(C)}; "
          f"{B.tlo.shape[0]} sign scenario(s)")
    # the enclosure is tight where it matters: a few fp32 ulps on the direction, on the t-range of rays that hit the volume
    w = (B.dhi - B.dlo) / 2
    assert float(w.max()) <= 8 * rr.U
    tm = r64[2]
    hit = (tm[..., 0] <= tm[..., 1]) & (tm[..., 1] >= 0) & np.isfinite(tm).all(-1)
    if hit.any():
        with np.errstate(invalid="ignore"):                       # inf - inf on the missing rays, which `hit` leaves out
            wt = ((B.thi - B.tlo) / 2)[:, hit]
        assert np.isfinite(wt).all()
        scale = np.maximum(np.abs(tm[hit]).max(-1, keepdims=True), 1.0)
        # (a / d): the direction's relative width carries over, times |d t / d d| <= |t| / |d_i|: bounded by the grazing factor
        assert float((wt / scale).max()) < 1e-3, float((wt / scale).max())


def test_restatement_reproduces_the_reference_pytorch_rays(golden):
    """The `rays_*` arrays of the committed golden are the outputs of the reference's own torch ray-direction code.  Tolerances: the
    existing test's (1e-6 directions, 1e-5 t-range) for the fp32 restatement; the float64 one is held tighter - the golden's own
    fp32 rounding: 2 ulp of a direction component (2^-22), 8 ulp of a t of up to 8 (8 * 2^-21)."""
    g = golden("raymarch")
    ops = (g["rays_viewpos"], g["rays_viewrot"], g["rays_focal"], g["rays_princpt"], g["rays_pixelcoords"], float(g["rays_volradius"]))
    for dtype, td, tt in ((np.float32, 1e-6, 1e-5), (np.float64, 2.0 ** -22, 2.0 ** -18)):
        rp, rd, tm = rr.rays(*ops, dtype=dtype)
        ed, et = float(np.abs(rd - g["rays_raydir"]).max()), float(np.abs(tm - g["rays_tminmax"]).max())
        print(f"{np.dtype(dtype).name} restatement vs the reference's torch rays: directions {ed:.2e}, t-range {et:.2e}")
        assert ed < td and et < tt, (ed, et)
    # ... and the golden itself lies inside the enclosure, but for the reference's different normalisation (v / |v|: a square root
    # and a division instead of rsqrt and a product) nothing says it must: reported, not asserted
    B = rr.bound(*ops)
    rp32 = rr.rays(*ops, dtype=np.float32)[0]
    v = _count(rr.violations(B, rp32, g["rays_raydir"], g["rays_tminmax"]))
    print(f"golden rays outside the kernel's enclosure (a different normalisation): {v}")
    assert v["raypos"] == 0
    assert np.isfinite(g["rays_tminmax"]).all()


# ------------------------------------------------------------------------------------------------ guards
def test_cases_reach_what_they_are_there_for():
    """In arithmetic on the operands (as test_scenes_reach_their_targets does for the marcher's scenes)."""
    pop = {n: rr.population(_case(n)[3]) for n in NAMES}
    hits = {}
    for n in NAMES:
        tm = _case(n)[4][2]
        hits[n] = (tm[..., 0] <= tm[..., 1]) & (tm[..., 1] >= 0)
    # exact-zero components: one row (yaw only), one row and one column (no rotation), and negative zeros
    c, ops, B, C, r64, r32 = _case("principal_cross")
    z = C["zero"]
    assert z[0, 8, :, 1].all() and not z[0, :, :, 0].any() and int(z[0].sum()) == 17
    assert z[1, 8, :, 1].all() and z[1, :, 8, 0].all() and int(z[1].sum()) == 34
    assert bool(np.signbit(r32[1][2][z[2]]).any()) and not bool(np.signbit(r32[1][1][z[1]]).any())
    assert pop["principal_cross"]["a"] == 17 + 33 + 33 and pop["principal_cross"]["b"] == pop["principal_cross"]["c"] == 0
    # the face camera: class (c) with +0 (tmax = -inf) and with -0 (tmin = +inf); the camera beside the volume: class (b)
    c, ops, B, C, r64, r32 = _case("axis_on_face")
    assert (c["viewpos"][0] == [0, 1, -3]).all() and (c["viewpos"][1] == [2, 0, -3]).all()
    assert pop["axis_on_face"]["b"] == 17 and pop["axis_on_face"]["c"] == 3 * 17
    assert C["c"][0, 8, :, 1].all() and C["b"][1, :, 8, 0].all() and C["c"][2, 8, :, 1].all() and C["c"][3, :, 8, 0].all()
    tm = r32[2]
    assert np.isneginf(tm[0, 8, :, 1]).all() and np.isfinite(tm[0, 8, :, 0]).all()
    assert np.isposinf(tm[2, 8, :, 0]).any() and not np.isnan(tm).any()
    assert hits["axis_on_face"][0].any() and not hits["axis_on_face"][0].all()          # the rest of that image is ordinary
    # hits and misses in one image, within one 256-thread block
    assert _case("grazing")[0]["pixelcoords"].shape[:3] == (1, 8, 31)
    assert 16 <= int(hits["grazing"].sum()) <= 248 - 16
    assert not hits["looking_away"].any() and bool((_case("looking_away")[4][2][..., 1] < 0).all())
    # a batch item with tmin == 0 everywhere: both cameras of `inside`, at 0.9 radii and at the exact centre
    c, ops, B, C, r64, r32 = _case("inside")
    assert C["d"].all() and (c["viewpos"][1] == 0).all() and 0.85 < float(np.linalg.norm(c["viewpos"][0])) < 0.95
    assert (r64[2][..., 0] == 0).all() and (r64[2][..., 1] > 0).all()
    assert not any(pop[n]["d"] for n in NAMES if n != "inside")
    # ragged against the 256-thread block, every batch stride in play, per-item cameras that all differ
    c = _case("generic_batch3")[0]
    N, H, W = c["pixelcoords"].shape[:3]
    assert (N, H, W) == (3, 13, 27) and (N * H * W) % 256 != 0 and N * H * W > 4 * 256
    assert (c["focal"][:, 0] != c["focal"][:, 1]).all() and len({tuple(r) for r in c["focal"].tolist()}) == 3
    assert len({tuple(r) for r in c["princpt"].tolist()}) == 3 and (c["princpt"] % 1 != 0).all()
    assert _case("one_pixel")[0]["pixelcoords"].shape == (1, 1, 1, 2)
    # the subsampled coordinates are not the integer grid of their own size, and the training draw differs between items
    for n in ("subsampled_eval", "subsampled_train"):
        pc = _case(n)[0]["pixelcoords"]
        assert not np.array_equal(pc, rr.pixel_grid(*pc.shape[:3]))
    pc = _case("subsampled_train")[0]["pixelcoords"]
    assert len({tuple(pc[b, 0, 0].tolist()) for b in range(pc.shape[0])}) > 1
    # world units: the origin is not the camera position
    for n, vr in (("volradius_100", 100.0), ("volradius_10000", 10000.0)):
        c, ops, B = _case(n)[:3]
        assert c["volradius"] == vr and float(np.abs(c["viewpos"]).max()) > 2 * vr and float(np.abs(B.o).max()) < 6
    # every case is a finite camera with a non-zero focal length
    for n in NAMES:
        c = _case(n)[0]
        assert all(np.isfinite(c[k]).all() for k in ("viewpos", "viewrot", "focal", "princpt", "pixelcoords")) and (c["focal"] != 0).all()
        assert max(c["pixelcoords"].shape[1:3]) <= 32


# ------------------------------------------------------------------------------------------------ injected faults
# fault -> the cases it must fail on (each is aimed at one of them; it may fail on others as well)
AIMED = {
    "rot_transposed": ["generic_batch3", "principal_cross"],
    "focal_swapped": ["generic_batch3", "one_pixel"],
    "princpt_swapped": ["generic_batch3", "one_pixel"],
    "hw_swapped": ["generic_batch3", "subsampled_eval"],
    "camera0": ["generic_batch3", "subsampled_train", "inside"],
    "no_volradius": ["volradius_100", "volradius_10000"],
    "no_normalise": NAMES,
    "tmin_unclamped": ["inside"],
    "tmax_clamped": ["looking_away"],              # (the misses of `grazing` lie in front of the camera: tmax > 0 there)
    "nan_propagating": ["axis_on_face"],
    "rsqrt11": NAMES,
}


@pytest.mark.parametrize("fault", rr.FAULTS)
def test_every_injected_fault_fails(fault):
    assert set(AIMED) == set(rr.FAULTS)
    for name in AIMED[fault]:
        nb, nc, _ = _failures(name, fault)
        print(f"{fault} on {name}: {nb} elements outside the enclosure, {nc} class violations")
        assert nb > 0, (fault, name)


def test_nan_propagation_fails_on_class_c_and_only_there():
    """np.minimum / np.maximum in place of np.fmin / np.fmax: every pixel of class (c) fails (both of its values are NaN), no other
    pixel of any case changes by a bit."""
    total = 0
    for name in NAMES:
        c, ops, B, C, _, r32 = _case(name)
        got = rr.rays(*ops, dtype=np.float32, fault="nan_propagating")
        in_c = C["c"].any(-1)
        v, cv = rr.violations(B, *got), rr.class_violations(B, C, *got)
        assert np.array_equal(v["tminmax"], in_c), name
        assert np.array_equal(np.isnan(got[2]).all(-1), in_c) and np.array_equal(np.isnan(got[2]).any(-1), in_c)
        assert np.array_equal(cv["c"], in_c) and not any(int(m.sum()) for k, m in cv.items() if k != "c")
        assert np.array_equal(got[2][~in_c].view(np.uint32), r32[2][~in_c].view(np.uint32))
        assert not v["raydir"].any() and not v["raypos"].any()
        total += int(in_c.sum())
    assert total == 3 * 17


# ------------------------------------------------------------------------------------------------ the oracle
def _propagating_oracle(viewpos, viewrot, focal, princpt, pixelcoords, volradius):
    """oracle/raymarch_ref.compute_raydirs as it was before it took the reference CUDA's fminf / fmaxf."""
    raypos = (viewpos / volradius)[:, None, None, :].expand(-1, pixelcoords.shape[1], pixelcoords.shape[2], -1)
    pc = (pixelcoords - princpt[:, None, None, :]) / focal[:, None, None, :]
    d = torch.cat([pc, torch.ones_like(pc[..., :1])], dim=-1)
    d = torch.einsum("nhwi,nij->nhwj", d, viewrot)
    d = d / d.norm(dim=-1, keepdim=True)
    t1, t2 = (-1.0 - raypos) / d, (1.0 - raypos) / d
    return torch.stack([torch.minimum(t1, t2).amax(-1).clamp(min=0.0), torch.maximum(t1, t2).amin(-1)], dim=-1)


def test_oracle_drops_the_nan_as_the_reference_cuda_does():
    """The discrepancy, recorded: with torch.minimum / maximum the oracle returned NaN on the rays of class (c) - a camera on a face
    plane of the volume looking along it - where the reference CUDA's fminf / fmaxf, the kernel and the restatement return an ordered
    pair without a NaN (tmax = -inf or tmin = +inf: a miss).  The oracle now uses torch.fmin / fmax; on every case here its t-range
    has no NaN, lies inside the enclosure and keeps every exact class."""
    c, ops, B, C, r64, r32 = _case("axis_on_face")
    T = [torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x for x in ops]
    in_c = C["c"].any(-1)
    old = _propagating_oracle(*T).numpy()
    assert np.array_equal(np.isnan(old).all(-1), in_c) and int(in_c.sum()) == 51
    assert not np.isnan(r32[2]).any() and not np.isnan(r64[2]).any()
    for name in NAMES:
        c, ops, B, C, r64, r32 = _case(name)
        T = [torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x for x in ops]
        rp, rd, tm = (x.numpy() for x in raymarch_ref.compute_raydirs(*T))
        assert not np.isnan(tm).any(), name
        # the oracle normalises with v / |v| (a correctly rounded square root and division: 2 u, inside the 5 u the enclosure grants
        # rsqrt and the product) and may hold the other zero (its sums run in another order): inside the enclosure, every class holds
        v, cv = rr.violations(B, rp, rd, tm), rr.class_violations(B, C, rp, rd, tm)
        assert not any(_count(v).values()), (name, _count(v))
        assert not any(_count(cv).values()), (name, _count(cv))


def test_marcher_scenes_have_no_ray_the_oracle_change_moves():
    """tests/raymarch_scenes.rays feeds the CPU tests of the marcher and the decision margins of the backward scenes.  None of those
    scenes has a ray of class (c) - the only rays the oracle's change touches - so their rays, and with them the margins, are
    bit for bit what they were: asserted here by running the former formulation next to the present one on every scene."""
    from tests import raymarch_scenes as sc
    from tests.test_hip_raymarch_grad import SCENES
    from tests.test_raymarch_contract import CASES
    kws = [dict(kw) for _, kw, _ in CASES] + [dict(v[0]) for v in SCENES.values()]
    assert len(kws) == len(CASES) + len(SCENES)
    for kw in kws:
        tpl, pos, rot, scale, cp, cr, f, pp = sc.scene(**kw)
        pc, (rp, rd, tm) = sc.rays(cp, cr, f, pp, kw["H"], kw["W"])
        old = _propagating_oracle(cp, cr, f, pp, pc, 1.0)
        assert not bool(torch.isnan(old).any())
        assert torch.equal(old.view(torch.int32), tm.view(torch.int32))


# ------------------------------------------------------------------------------------------------ host plumbing (CPU tensors)
def _resize_pixel_coords(H, W, factor):
    """The reference's resize_pixel_coords (dva/ray_marcher.py:57-76), restated in numpy: the (x, y) grid, for factor > 1 sampled
    with stride `factor` from the offset factor // 2, cut to H // factor x W // factor."""
    base = rr.pixel_grid(1, H, W)[0]
    if factor == 1:
        return base
    o = factor // 2
    return base[o:o + factor * (H // factor):factor, o:o + factor * (W // factor):factor]


def test_pixel_coords_factors_cache_and_resize():
    from topia_xl_amd import raymarch as rm
    m = rm.RayMarcher(13, 27, 1.0).eval()
    for f in (1, 2, 3, 2, 1):                       # the one-entry cache is replaced, then replaced back
        want = _resize_pixel_coords(13, 27, f)
        for B in (1, 3):
            got = m._pixel_coords(B, f, "cpu")
            assert got.shape == (B, 13 // f, 27 // f, 2) and got.dtype == torch.float32 and got.is_contiguous()
            assert all(np.array_equal(got[b].numpy(), want) for b in range(B)), f
    assert m._pixel_coords(1, 2, "cpu")[0, 0, 0].tolist() == [1.0, 1.0] and m._pixel_coords(1, 3, "cpu")[0, -1, -1].tolist() == [25.0, 10.0]
    first = m._pixel_coords(2, 2, "cpu").clone()
    m.resize(9, 31)
    got = m._pixel_coords(2, 2, "cpu")              # the new size's coordinates, not the cached ones
    assert got.shape == (2, 4, 15, 2) and np.array_equal(got[1].numpy(), _resize_pixel_coords(9, 31, 2))
    m.resize(27, 13)                                # H and W exchanged: same element count as the first size
    got = m._pixel_coords(2, 2, "cpu")
    assert got.shape == (2, 13, 6, 2) and np.array_equal(got[0].numpy(), _resize_pixel_coords(27, 13, 2))
    m.resize(13, 27)
    assert torch.equal(m._pixel_coords(2, 2, "cpu"), first)
    got[...] = -1.0                                 # the returned tensor is the caller's: writing to it leaves the cache alone
    back = m._pixel_coords(2, 2, "cpu")
    back[...] = -1.0
    assert torch.equal(m._pixel_coords(2, 2, "cpu"), first)


def test_training_pixel_coords_draw_order_and_range():
    from topia_xl_amd import raymarch as rm
    H, W, B = 13, 27, 4
    base = rm.base_pixel_coords(H, W)
    assert np.array_equal(base.numpy(), rr.pixel_grid(1, H, W)[0])
    for f in (2, 3, 4):
        gen_state = torch.random.get_rng_state()
        try:
            torch.manual_seed(7 + f)
            got = rm.training_pixel_coords(base, B, f)
            torch.manual_seed(7 + f)
            draws = [int(torch.randint(0, f - 1, size=())) for _ in range(2 * B)]
        finally:
            torch.random.set_rng_state(gen_state)
        assert got.shape == (B, H // f, W // f, 2) and got.is_contiguous()
        assert min(draws) >= 0 and max(draws) <= f - 2
        for b in range(B):
            x0, y0 = draws[2 * b], draws[2 * b + 1]                      # x0 is drawn before y0, per batch item
            want = base[y0::f, x0::f][:H // f, :W // f]
            assert torch.equal(got[b], want), (f, b)
            assert got[b, 0, 0].tolist() == [float(x0), float(y0)]
        if f > 2:
            assert len({(draws[2 * b], draws[2 * b + 1]) for b in range(B)}) > 1 and any(draws[2 * b] != draws[2 * b + 1] for b in range(B))


def test_convert_camera_parameters_is_minus_rt_t():
    """c = -R^T t in float64 for non-symmetric rotations (R != R^T: a transposed product gives another point)."""
    from topia_xl_amd import raymarch as rm
    Rs = np.stack([rr._rot(0.7, -0.4), rr._rot(-2.0, 0.9)]).astype(np.float64)
    assert float(np.abs(Rs - Rs.transpose(0, 2, 1)).max()) > 0.3
    t = np.array([[0.3, -1.2, 4.0], [-2.5, 0.4, 3.0]])
    Rt = np.concatenate([Rs, t[..., None]], -1)
    K = np.array([[[38.0, 0, 13.3], [0, 41.0, 6.7], [0, 0, 1]], [[30.0, 0, 12.1], [0, 36.5, 5.9], [0, 0, 1]]])
    for dtype, tol in ((torch.float64, 1e-15), (torch.float32, 4 * 2.0 ** -24)):
        cam = rm.convert_camera_parameters(torch.from_numpy(Rt).to(dtype), torch.from_numpy(K).to(dtype))
        want = -np.einsum("nji,nj->ni", Rs, t)
        wrong = -np.einsum("nij,nj->ni", Rs, t)
        err = float(np.abs(cam["campos"].double().numpy() - want).max())
        assert err <= tol * 8.0 and float(np.abs(want - wrong).max()) > 0.5, err          # |t| < 8; the transposed product is far off
        assert torch.equal(cam["camrot"], torch.from_numpy(Rs).to(dtype))
        assert cam["focal"].shape == (2, 2, 2) and torch.equal(torch.diagonal(cam["focal"], dim1=1, dim2=2),
                                                               torch.from_numpy(K[:, [0, 1], [0, 1]]).to(dtype))
        assert torch.equal(cam["princpt"], torch.from_numpy(K[:, :2, 2]).to(dtype))
        oc = raymarch_ref.convert_camera(torch.from_numpy(Rt).to(dtype), torch.from_numpy(K).to(dtype))
        assert float((oc[0] - cam["campos"]).abs().max()) <= tol * 8.0
