"""Ambient occlusion of the SDF lattice on the MI355X: `primx_texbake_occlusion` against the float64 restatement of rules A1-A4
(tests/occlusion_numpy.py), its determinism, the R channel `fill_textures(occlusion=)` writes, the small export with and without
the option, and the footprint and stream-order case of the entry point.

Tolerance: 4 x the distance of the SAME restatement run in float32 on the CPU from the float64 one, pooled over all cases of the
kernel test (the project's convention).  The estimator is continuous in its operands, so no texel is left out.

The module imports without a GPU: it registers its stream-order case in the table of tests/test_hip_streams.py at import (that
file stays as it is) and runs it here; the lattices below are numpy and serve tests/test_occlusion_cpu.py too.
"""
import functools

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import occlusion_numpy as ON
from tests import streamorder as so
from tests import test_hip_streams as TS
from tests.test_hip_normalmap import E, mods  # noqa: F401  (fixtures: the built package; one side stream of this module's own)
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES, ATLAS, RADIUS = 48, 128, 4                                          # the small export: 48^3 lattice, 128^2 atlas, fill radius 4
STREAM_CASE = "texbake_occlusion"


# ------------------------------------------------------------------------------------------------ lattices and points (numpy)
def _axes(R):
    lin = np.linspace(-1, 1, R, dtype=np.float32).astype(np.float64)
    return np.meshgrid(lin, lin, lin, indexing="ij")


def plane_lattice(R):
    return (_axes(R)[2] - 0.1).astype(np.float32)


def sphere_lattice(R, r=0.5):
    X, Y, Z = _axes(R)
    return (np.sqrt(X * X + Y * Y + Z * Z) - r).astype(np.float32)


def two_spheres_lattice(R, r=0.35, c=0.3):
    X, Y, Z = _axes(R)
    return (np.minimum(np.sqrt((X - c) ** 2 + Y * Y + Z * Z), np.sqrt((X + c) ** 2 + Y * Y + Z * Z)) - r).astype(np.float32)


def hollow_lattice(R, r=0.6):
    X, Y, Z = _axes(R)
    return (r - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)


def smooth_lattice(R, seed):
    """A seeded sum of eight low-frequency waves (|wave vector| <= 4 per axis), amplitude about 1: no distance function at all."""
    rng = np.random.default_rng(seed)
    X, Y, Z = _axes(R)
    out = np.zeros_like(X)
    for _ in range(8):
        w, ph, a = rng.uniform(-4, 4, 3), rng.uniform(0, 2 * np.pi), rng.uniform(0.2, 0.5)
        out += a * np.sin(w[0] * X + w[1] * Y + w[2] * Z + ph)
    return out.astype(np.float32)


def unit_vectors(n, seed):
    u = np.random.default_rng(seed).standard_normal((n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> dict(lat, pts, nrm, K, steps, radius, bias, iso, open): every R of {2, 33, 65}, n of {1, 257, 4099}, K of
    {1, 64, 256} and steps of {1, 8}; an isovalue, bias = 0, points on and beyond the cube's faces and zero normals."""
    out = {}

    def add(name, lat, pts, nrm, K=64, steps=8, radius=0.25, bias=None, iso=0.0, open_=False):
        out[name] = dict(lat=lat, pts=_f32(pts), nrm=_f32(nrm), K=K, steps=steps, radius=radius, bias=bias, iso=iso, open=open_)

    rng = np.random.default_rng(7)
    xy = rng.uniform(-0.8, 0.8, (257, 2))
    add("plane", plane_lattice(65), np.concatenate([xy, np.full((257, 1), 0.1)], 1), np.tile([0.0, 0.0, 1.0], (257, 1)), open_=True)
    u = unit_vectors(4099, 1)
    add("sphere exterior", sphere_lattice(65), 0.5 * u, u, open_=True)
    # (at R = 33 the first sample lies half a cell out and the interpolation error outweighs the sphere's curvature: the float64
    # estimator itself is 2e-7 short of 1 at six of these texels, so the exactly-open cases stay at R = 65)
    add("sphere exterior, isovalue", sphere_lattice(65, 0.4), 0.5 * u[:257], u[:257], K=256, iso=0.1, open_=True)
    add("sphere exterior, coarse", sphere_lattice(33, 0.4), 0.5 * u[:257], u[:257], K=256, iso=0.1)
    c = np.array([0.3, 0.0, 0.0])
    add("two spheres", two_spheres_lattice(65), c + 0.35 * u, u)
    add("two spheres, one direction", two_spheres_lattice(33), 0.35 * u - c, u, K=1)        # d_0 = +x: towards the other sphere
    add("hollow sphere", hollow_lattice(33), 0.6 * u[:257], -u[:257], K=256)
    # no distance field; points in [-1.3, 1.3]^3, every 7th on a face of the cube, every 5th normal zero; one sample per ray, no bias
    p = rng.uniform(-1.3, 1.3, (4099, 3))
    p[::7, rng.integers(0, 3)] = 1.0
    p[3::7, rng.integers(0, 3)] = -1.0
    nz = unit_vectors(4099, 2)
    nz[::5] = 0
    add("waves, one step, no bias", smooth_lattice(33, 11), p, nz, steps=1, bias=0.0, iso=0.05)
    add("waves, isovalue", smooth_lattice(65, 12), p[:257], nz[:257], K=256, radius=0.4, iso=-0.2)
    add("two cells, one texel", smooth_lattice(2, 13), [[0.2, -0.4, 0.1]], [[0.6, 0.0, 0.8]], K=1, steps=1)
    add("two cells", smooth_lattice(2, 13), p[:257], unit_vectors(257, 3), radius=1.0, iso=0.1)
    return out


@functools.lru_cache(maxsize=None)
def _pool():
    """-> ({name: (ao64, ao32)}, bound): the float64 truth, the float32 yardstick and 4 x the yardstick's largest error over ALL
    cases.  Computed once."""
    ref, floor = {}, 0.0
    for name, c in _cases().items():
        a = [ON.occlusion(c["lat"], c["pts"], c["nrm"], ON.directions(c["K"]), c["steps"], c["radius"], c["bias"], c["iso"], dt)
             for dt in (np.float64, np.float32)]
        ref[name] = a
        floor = max(floor, float(np.abs(a[1].astype(np.float64) - a[0]).max()))
    return ref, 4.0 * floor


def _run(M, c):
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    return M.texel_occlusion(t(c["lat"]), t(c["pts"]), t(c["nrm"]), M.occlusion_directions(c["K"]), c["steps"], c["radius"],
                             c["bias"], c["iso"])


# ------------------------------------------------------------------------------------------------ 1. kernel vs float64
def test_kernel_matches_the_float64_restatement(mods):
    """Measured on the MI355X (largest kernel error over the pooled bound): see DESIGN.md "Ambient occlusion"."""
    ref, bound = _pool()
    occluded = sum(int((r[0] < 1).sum()) for r in ref.values())
    print(f"pooled bound 4 x {bound / 4:.3e} = {bound:.3e}; {occluded} occluded texels in the pool")
    assert bound > 0 and occluded > 1000
    worst, failed = 0.0, []
    for name, c in _cases().items():
        ao = _run(mods.M, c).cpu().numpy()
        assert ao.dtype == np.float32 and ao.shape == (len(c["pts"]),)
        err = float(np.abs(ao.astype(np.float64) - ref[name][0]).max())
        worst = max(worst, err)
        print(f"{name}: R = {c['lat'].shape[0]}, n = {len(ao)}, K = {c['K']}, steps = {c['steps']}; ao in [{ao.min():.4f}, {ao.max():.4f}], "
              f"{int((ao < 1).sum())} occluded; max-abs error {err:.3e} (fp32 restatement's own {np.abs(ref[name][1] - ref[name][0]).max():.3e})")
        if c["open"]:
            assert bool((ao == 1.0).all()), name                      # plane and convex: bit-exactly open
        zero = ~c["nrm"].any(1)
        assert bool((ao[zero] == 1.0).all()), name                    # a zero normal
        assert float(ao.min()) >= 0 and float(ao.max()) <= 1, name
        if err > bound:
            failed.append((name, err))
    print(f"largest kernel error {worst:.3e} = {worst / bound:.3f} of the pooled bound {bound:.3e}")
    assert not failed, (failed, bound)


def test_arguments_are_checked(mods):
    M = mods.M
    c = _cases()["two cells"]
    t = lambda a: torch.from_numpy(a).to(DEV)   # noqa: E731
    lat, pts, nrm = t(c["lat"]), t(c["pts"]), t(c["nrm"])
    assert tuple(M.texel_occlusion(lat, pts[:0], nrm[:0]).shape) == (0,)
    for kw in (dict(steps=0), dict(steps=65), dict(radius=0.0), dict(bias=-1.0), dict(directions=torch.zeros(257, 3))):
        with pytest.raises(RuntimeError, match="primx_texbake_occlusion"):
            M.texel_occlusion(lat, pts, nrm, **kw)
    with pytest.raises(RuntimeError, match="primx_texbake_occlusion"):
        M.texel_occlusion(lat[:1, :1, :1], pts, nrm)
    with pytest.raises(ValueError):
        M.texel_occlusion(lat[:, :, :1], pts, nrm)
    with pytest.raises(RuntimeError, match="HIP device"):
        M.texel_occlusion(lat.cpu(), pts.cpu(), nrm.cpu())


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_two_runs_and_both_fills_give_equal_bits(mods):
    c = _cases()["two spheres"]
    a, b = _run(mods.M, c), _run(mods.M, c)
    assert fp.same_bits(a, b)
    for fill in fp.FILLS:                                             # torch.empty's contents
        with fp.Guard(fill):
            assert fp.same_bits(_run(mods.M, c), a), fill


# ------------------------------------------------------------------------------------------------ the small export
def _crease_field(S=8, seed=31):
    """A PrimSDF on DEV (eval mode) whose payload is the SDF of the union of two spheres (radius 0.35, centres +-0.3 on x) sampled
    at the primitives' grid points: centres on a Fibonacci lattice of each sphere where it lies outside the other, scales
    0.16 .. 0.2 and colours / materials in [0.2, 0.8] from a seeded generator.  The crease between the spheres is the concavity."""
    from topia_xl_amd.primsdf import PrimSDF
    gen = torch.Generator().manual_seed(seed)
    d = torch.from_numpy(ON.directions(72)).double()
    cs = torch.tensor([[0.3, 0.0, 0.0], [-0.3, 0.0, 0.0]], dtype=torch.float64)
    pos = torch.cat([cs[k] + 0.35 * d for k in range(2)])
    pos = pos[torch.cat([(pos[:72] - cs[1]).norm(dim=1), (pos[72:] - cs[0]).norm(dim=1)]) > 0.35].float()
    P = pos.shape[0]
    scale = 0.16 + 0.04 * torch.rand(P, 1, generator=gen)
    lin = torch.linspace(-1, 1, S)
    Zg, Yg, Xg = torch.meshgrid(lin, lin, lin, indexing="ij")                 # [z][y][x] payload layout
    grid = pos[:, None, :] + scale[:, None, :] * torch.stack([Xg, Yg, Zg], -1).reshape(1, -1, 3)
    sdf = torch.minimum((grid - cs[0].float()).norm(dim=-1), (grid - cs[1].float()).norm(dim=-1)) - 0.35
    m = PrimSDF(num_prims=P, prim_shape=S)
    m.srt_param.data = torch.cat([scale, pos], 1)
    m.feat_param.data = torch.cat([sdf, 0.2 + 0.6 * torch.rand(P, 5 * S ** 3, generator=gen)], 1)
    return m.eval().to(DEV)


class _Export:
    """The stages of mesh.extract_texmesh(occlusion=True) on the crease field, kept for the tests below (computed once)."""

    def __init__(self, M):
        field = _crease_field()
        self.raw = field
        self.field = M._filtered_copy(field, M.noise_filter_mask(field.srt_param.detach()))     # as extract_texmesh filters it
        self.lattice = M.field_lattice(self.field, RES)
        self.mesh = M.extract_mesh(self.field, RES, filter_noise=False)
        self.atlas = M.uv_unwrap(self.mesh.v, self.mesh.f, self.mesh.normals, (ATLAS, ATLAS))
        self.texel, self.pts = M.atlas_points(self.atlas, self.mesh.v, self.mesh.f)
        self.g = M.field_normals(self.field, self.pts)
        self.attr = self.field.query(self.pts)
        self.dirs = M.occlusion_directions().to(DEV)
        self.ao = M.texel_occlusion(self.lattice, self.pts, self.g, self.dirs)


@functools.lru_cache(maxsize=None)
def _export(M):
    return _Export(M)


# ------------------------------------------------------------------------------------------------ 3. the fill's R channel
def test_fill_copies_r_from_the_texel_g_and_b_come_from(mods):
    """With the roughness column set to the same ao, R equals G at EVERY texel of the image: the covered ones quantise the same
    number, the filled ones copy the same band texel, the rest are 0.  G, B and the albedo keep the bits they have without it."""
    M = mods.M
    x = _export(M)
    attr = x.attr.clone()
    attr[:, 4] = x.ao
    albedo0, mr0 = M.fill_textures(attr, x.texel, x.atlas.face_id, RADIUS)
    albedo1, mr1 = M.fill_textures(attr, x.texel, x.atlas.face_id, RADIUS, occlusion=x.ao)
    assert fp.same_bits(albedo0, albedo1) and fp.same_bits(mr0[..., 1:].contiguous(), mr1[..., 1:].contiguous())
    assert int(mr0[..., 0].max()) == 0
    assert torch.equal(mr1[..., 0], mr1[..., 1])
    cov = x.atlas.face_id >= 0
    filled = ~cov & (mr1[..., 1] > 0)
    assert int(filled.sum()) > 100 and int((~cov & (mr1[..., 1] == 0)).sum()) > 100
    with pytest.raises(ValueError):
        M.fill_textures(attr, x.texel, x.atlas.face_id, RADIUS, occlusion=x.ao[:-1])


# ------------------------------------------------------------------------------------------------ 4. end to end
def test_extract_texmesh_with_occlusion(mods, tmp_path):
    from topia_xl_amd import pipeline
    M = mods.M
    x = _export(M)
    off = M.extract_texmesh(x.raw, RES, ATLAS, fill_radius=RADIUS)
    on = M.extract_texmesh(x.raw, RES, ATLAS, fill_radius=RADIUS, occlusion=True)
    assert on.occlusion is True and off.occlusion is False and on.normal_map is None and on.tangents is None
    for name in ("v", "f", "normals", "vt", "vmap", "albedo", "covered"):
        assert fp.same_bits(getattr(off, name), getattr(on, name)), name
    assert torch.equal(off.metallic_roughness[..., 1:], on.metallic_roughness[..., 1:]) and int(off.metallic_roughness[..., 0].max()) == 0
    # the covered bytes are the quantised kernel output of the same operands
    assert torch.equal(on.covered, x.atlas.face_id >= 0)
    r = on.metallic_roughness[..., 0].reshape(-1)[x.texel.long()].cpu().numpy()
    ao = x.ao.cpu().numpy()
    assert np.array_equal(r, ON.quantize(ao))
    # ... and within one byte step plus the kernel's bound of the float64 estimator
    _, bound = _pool()
    ao64 = ON.occlusion(x.lattice.cpu().numpy(), x.pts.cpu().numpy(), x.g.cpu().numpy(), ON.directions(64))
    err = float(np.abs(r.astype(np.float64) - 255.0 * ao64).max())
    print(f"{len(r)} covered texels: ao in [{ao.min():.4f}, {ao.max():.4f}], {int((r < 255).sum())} below 255, {int((r == 255).sum())} at 255; "
          f"|byte - 255 ao64| <= {err:.4f} (bound 1 + 255 x {bound:.3e}); kernel vs float64 {np.abs(ao - ao64).max():.3e}")
    assert err <= 1.0 + 255.0 * bound
    assert int((r < 255).sum()) > 0 and int((r == 255).sum()) > 0
    # with the normal map: the field normals are shared, both maps keep their bits
    both = M.extract_texmesh(x.raw, RES, ATLAS, fill_radius=RADIUS, occlusion=True, normal_map=True)
    nm = M.extract_texmesh(x.raw, RES, ATLAS, fill_radius=RADIUS, normal_map=True)
    assert fp.same_bits(both.metallic_roughness, on.metallic_roughness) and fp.same_bits(both.normal_map, nm.normal_map)
    # bake_textures on its own computes the lattice itself
    own = M.bake_textures(x.field, x.mesh, ATLAS, fill_radius=RADIUS, occlusion=True, occlusion_resolution=RES)
    assert fp.same_bits(own.metallic_roughness, on.metallic_roughness)
    # the pipeline's pass-through
    recon = torch.cat([x.raw.srt_param.detach(), x.raw.feat_param.detach()], 1)
    via = pipeline.primitives_to_texmesh(recon, RES, ATLAS, fill_radius=RADIUS, occlusion=True)
    assert via.occlusion and fp.same_bits(via.metallic_roughness, on.metallic_roughness) and fp.same_bits(via.albedo, on.albedo)
    # the GLB names the image and still reads back
    path = str(tmp_path / "ao.glb")
    on.write_glb(path)
    off.write_glb(str(tmp_path / "plain.glb"))
    assert b'"occlusionTexture":{"index":1,"strength":1.0}' in open(path, "rb").read()
    assert b"occlusionTexture" not in open(str(tmp_path / "plain.glb"), "rb").read()
    back = M.read_glb(path)
    assert tuple(back.f.shape) == tuple(on.f.shape) and len(back.images) == 2
    assert np.array_equal(np.asarray(back.images[1])[..., :3], on.metallic_roughness.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 5. footprint
def test_footprint_of_the_entry_point(mods):
    """Inside footprint.hold: intact guards around the output, untouched const operands, no allocation past the wrapper, and a
    result that depends neither on the fill of torch.empty nor on the guard (bit for bit: nothing here is atomic)."""
    M = mods.M
    x = _export(M)

    def case(g):
        gi = lambda t, name: g.guard_input(t, name).t   # noqa: E731
        lat, pts, nrm, dirs = gi(x.lattice, "lattice"), gi(x.pts, "pts"), gi(x.g, "normals"), gi(x.dirs, "directions")
        ao = M.texel_occlusion(lat, pts, nrm, dirs)
        return [ao, M.fill_textures(x.attr, x.texel, x.atlas.face_id, RADIUS, occlusion=ao)]

    out = fp.hold(case)
    assert fp.same_bits(out[0], x.ao)


# ------------------------------------------------------------------------------------------------ 6. stream order
@TS.case(STREAM_CASE, ["primx_texbake_occlusion"])
def _stream_occlusion(E, dtype):  # noqa: F811
    """The two-spheres lattice at 33^3 and 4099 texels; the lattice, the points, the normals and the table are all late operands
    (their poison is NaN: the position clamp keeps every index inside the lattice)."""
    from topia_xl_amd import mesh as M
    c = _cases()["two spheres, one direction"]

    def make(k):
        rot = np.roll(c["nrm"], k, 1) if k else c["nrm"]
        return {"lattice": torch.from_numpy(c["lat"] + np.float32(0.02 * k)).to(DEV), "pts": torch.from_numpy(c["pts"]).to(DEV) + 0.01 * k,
                "nrm": torch.from_numpy(_f32(rot)).to(DEV), "dirs": M.occlusion_directions(64).roll(k, 1).contiguous().to(DEV)}

    def call(ctx, i, probe):
        return [M.texel_occlusion(i["lattice"], i["pts"], i["nrm"], i["dirs"])]
    return make, call, None


def test_stream_order_of_the_occlusion_entry_point(E, called):  # noqa: F811  (`called` is the imported fixture)
    """The body of tests/test_hip_streams.py::test_stream_order for the case registered above; no host synchronisation is documented."""
    c = TS.CASES[STREAM_CASE]
    make, call, setup = c.build(E, None)
    rep = so.run(STREAM_CASE, make, call, E.S, E.blocker, setup=setup, must_sync=False)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{STREAM_CASE} declares entry points it did not call: {missing}"
