"""The tangent-space normal map on the MI355X: `primx_primsdf_query_grad` against the float64 autograd of the restated field
(tests/normalmap_numpy.py through tests/primsdf_grad_ref.field), `primx_texbake_tangents` and `primx_texbake_normal_texels`
against their float64 restatements and the glTF 2.0 handedness, the baked bytes, the unchanged default path, the decimated
pipeline, and the footprint and stream-order cases of the three entry points.

Tolerances follow tests/test_hip_primsdf_grad.py: 4 x the distance of the SAME restatement run in float32 on the CPU from the
float64 one, plus one fp32 ulp of the largest entry.  Points within DELTA of a kink of the field are dropped before either side
is compared (the share is printed and capped).  The `_inputs` generator is that module's, copied.

The module imports without a GPU: it registers its stream-order cases in the table of tests/test_hip_streams.py at import (that
file stays as it is) and runs them here.  The side stream is this module's own, created and destroyed here, for the reason given
in tests/test_hip_primsdf_grad.py.
"""
import dataclasses
import functools
import json
import struct

import numpy as np
import pytest
import torch

from tests import footprint as fp
from tests import normalmap_numpy as NM
from tests import primsdf_grad_ref as G
from tests import streamorder as so
from tests import test_hip_streams as TS
from tests import texbake_numpy as tb
from tests.test_hip_streams import called  # noqa: F401  (the stream table's fixture: which primx_* functions a case called)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = 1e-5
MAX_DROPPED = 0.02
ULP = float(np.finfo(np.float32).eps)
CASES = [(1, 2, 257), (33, 3, 4099), (33, 8, 4099), (1025, 8, 4099)]    # one block plus a lane; overlaps; across the 1024-primitive chunk
RES, ATLAS, RADIUS = 48, 128, 4                                          # the small export: 48^3 lattice, 128^2 atlas, fill radius 4
QUANT = 1.0 / 255.0                                                      # half a quantisation step of the map, in normal units


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__
    __graft_entry__.build()
    from oracle import synth
    from topia_xl_amd import _lib, mesh, ops, primsdf
    return type("Mods", (), dict(lib=_lib.load(), M=mesh, ops=ops, primsdf=primsdf, synth=synth, check=staticmethod(_lib.check)))


@pytest.fixture(scope="module")
def E(mods):
    """The Env of tests/test_hip_streams.py::E with ONE side stream of this module's own, non-blocking with respect to stream 0,
    destroyed at teardown (tests/test_hip_primsdf_grad.py explains why)."""
    import ctypes
    import os
    from collections import namedtuple

    import topia_xl_amd
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))    # the runtime torch has mapped
    hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamDestroy.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], [ctypes.c_void_p]
    torch.cuda.init()
    with torch.cuda.device(0):
        raw = ctypes.c_void_p()
        assert hip.hipStreamCreateWithFlags(ctypes.byref(raw), 1) == 0 and raw.value                 # 1 = hipStreamNonBlocking
        env = namedtuple("Env", "pkg ops lib S S2 blocker")(topia_xl_amd, mods.ops, mods.lib, torch.cuda.ExternalStream(raw.value), None,
                                                             so.Blocker())
        yield env
        torch.cuda.synchronize()
        assert hip.hipStreamDestroy(raw) == 0


# ------------------------------------------------------------------------------------------------ inputs and references
def _inputs(P, S, n, seed=0):
    """tests/test_hip_primsdf_grad.py::_inputs, copied: -> (x [n, 3], srt [P, 4], feat [P, 6 S^3], gout [n, 6])."""
    g = torch.Generator().manual_seed(1000 * P + 10 * S + seed)
    pos = 1.2 * torch.rand(P, 3, generator=g) - 0.6
    scale = 0.15 + 0.2 * torch.rand(P, 1, generator=g)
    feat = 0.5 * torch.randn(P, 6, S ** 3, generator=g)
    feat[:, 1:] += 0.5                                               # tex / mat around 0.5: a share of the outputs clips
    n0 = n // 2
    k = torch.randint(P, (n - n0,), generator=g)
    x = torch.cat([1.8 * torch.rand(n0, 3, generator=g) - 0.9, pos[k] + scale[k] * (2 * torch.rand(n - n0, 3, generator=g) - 1)])
    return x, torch.cat([scale, pos], 1), feat.reshape(P, -1).contiguous(), torch.randn(n, 6, generator=g)


def _reference(x, srt, feat, S):
    """Flag the kinks, then float64 autograd of the training-mode field and the tolerance from the fp32 restatement's own error."""
    bad = G.kinks(x, srt, feat, S, DELTA)
    keep = ~bad
    _, g64 = NM.point_grad(x[keep], srt, feat, S, torch.float64)
    _, g32 = NM.point_grad(x[keep], srt, feat, S, torch.float32)
    top = float(g64.abs().max())
    floor = float((g32.double() - g64).abs().max())
    return dict(x=x, srt=srt, feat=feat, S=S, keep=keep, grad=g64, tol=4 * floor + ULP * top, floor=floor, top=top,
                dropped=float(bad.float().mean()))


@functools.lru_cache(maxsize=None)
def _case(P, S, n):
    x, srt, feat, _ = _inputs(P, S, n)
    return _reference(x, srt, feat, S)


def _shell_field(P=96, S=8, seed=29):
    """A PrimSDF on DEV (eval mode) whose payload is the SDF of the sphere of radius 0.5 sampled at the primitives' grid points:
    centres on a Fibonacci lattice of that sphere, scales 0.16 .. 0.2 from a seeded generator - every point within 0.03 of the
    sphere is covered with sum w > 0.8 - and seeded colours / materials in [0.2, 0.8] (no clipped channel)."""
    from topia_xl_amd.primsdf import PrimSDF
    gen = torch.Generator().manual_seed(seed)
    k = torch.arange(P, dtype=torch.float64) + 0.5
    z = 1 - 2 * k / P
    phi = k * (np.pi * (3 - 5 ** 0.5))
    r = (1 - z * z).sqrt()
    pos = (0.5 * torch.stack([r * phi.cos(), r * phi.sin(), z], 1)).float()
    scale = 0.16 + 0.04 * torch.rand(P, 1, generator=gen)
    lin = torch.linspace(-1, 1, S)
    Zg, Yg, Xg = torch.meshgrid(lin, lin, lin, indexing="ij")                 # [z][y][x] payload layout
    grid = pos[:, None, :] + scale[:, None, :] * torch.stack([Xg, Yg, Zg], -1).reshape(1, -1, 3)
    m = PrimSDF(num_prims=P, prim_shape=S)
    m.srt_param.data = torch.cat([scale, pos], 1)
    m.feat_param.data = torch.cat([grid.norm(dim=-1) - 0.5, 0.2 + 0.6 * torch.rand(P, 5 * S ** 3, generator=gen)], 1)
    return m.eval().to(DEV)


def _module(mods, srt, feat, S, training):
    m = mods.primsdf.PrimSDF(num_prims=srt.shape[0], prim_shape=S).to(DEV)
    m.srt_param.data, m.feat_param.data = srt.to(DEV).contiguous(), feat.to(DEV).contiguous()
    return m.train(training)


def _plain_query(mods, m, x, eval_fill):
    out = torch.empty(x.shape[0], 6, device=DEV)
    mods.check(mods.lib.primx_primsdf_query(x.data_ptr(), m.srt_param.data_ptr(), m.feat_param.data_ptr(), m._linspace(x.device).data_ptr(),
                                            out.data_ptr(), x.shape[0], m.srt_param.shape[0], m.prim_shape, 6, eval_fill,
                                            torch.cuda.current_stream().cuda_stream), "primx_primsdf_query")
    return out


def _compare(tag, r, grad):
    assert bool(torch.isfinite(grad).all()), tag
    err = float((grad.cpu().double()[r["keep"]] - r["grad"]).abs().max())
    print(f"{tag}: max-abs error {err:.3e}, tolerance {r['tol']:.3e} (fp32 restatement's own error {r['floor']:.3e}), largest entry "
          f"{r['top']:.3e} (error / largest {err / max(r['top'], 1e-300):.2e}); {100 * r['dropped']:.3f} % of the points dropped as kinks")
    assert r["dropped"] <= MAX_DROPPED, (tag, r["dropped"])
    assert err <= r["tol"], (tag, err, r["tol"])


# ------------------------------------------------------------------------------------------------ 1. kernel vs float64 autograd
@pytest.mark.parametrize("P,S,n", CASES)
def test_gradient_matches_float64_autograd_and_out_keeps_the_query_bits(mods, P, S, n):
    """Measured on the MI355X (error / tolerance): see DESIGN.md "Normal map"."""
    r = _case(P, S, n)
    assert r["top"] > 0
    x = r["x"].to(DEV)
    for training in (True, False):
        m = _module(mods, r["srt"], r["feat"], S, training)
        out, grad = m.query_grad(x)
        assert torch.equal(out, _plain_query(mods, m, x, 0 if training else 1)) and torch.equal(out, m.query(x))
        if training:                                                 # the restated field has no fill: eval_fill = 0 is its twin
            _compare(f"({P}, {S}, {n})", r, grad)
        else:                                                        # covered points do not feel the fill
            cov = NM.covered(r["x"], r["srt"]) & r["keep"]
            assert torch.equal(grad.cpu()[cov], train_grad.cpu()[cov])
        train_grad = grad


# ------------------------------------------------------------------------------------------------ 2. special cases
def test_negative_scale(mods):
    x, srt, feat, _ = _inputs(33, 3, 1025, seed=1)
    srt[::2, 0] *= -1
    r = _reference(x, srt, feat, 3)
    assert r["top"] > 0
    _compare("negative scale", r, _module(mods, srt, feat, 3, True).query_grad(x.to(DEV))[1])


def test_zero_scale_covers_nothing(mods):
    """A zero scale weighs nothing (the forward's rule): the field with such a primitive is the field without it, also for the
    point at its very centre (where the reference's own weight is NaN)."""
    x, srt, feat, _ = _inputs(33, 3, 1025, seed=2)
    x[0] = srt[7, 1:4]
    r = _reference(x, torch.cat([srt[:7], srt[8:]]), torch.cat([feat[:7], feat[8:]]), 3)     # the field without primitive 7
    srt[7, 0] = 0.0
    out, grad = _module(mods, srt, feat, 3, True).query_grad(x.to(DEV))
    assert bool(torch.isfinite(out).all())
    _compare("zero scale", r, grad)


def test_point_exactly_at_a_centre(mods):
    """d = 0: every |d_a| ties at 0, the x axis is chosen and sign(0) = 0, so the weight path adds nothing - as torch's abs and
    max differentiate it.  One primitive of 2^3 voxels: the centre lies in the middle of its only cell."""
    x, srt, feat, _ = _inputs(1, 2, 257)
    x = srt[:1, 1:4].clone()
    _, g64 = NM.point_grad(x, srt, feat, 2, torch.float64)
    _, g32 = NM.point_grad(x, srt, feat, 2, torch.float32)
    tol = 4 * float((g32.double() - g64).abs().max()) + ULP * float(g64.abs().max())
    out, grad = _module(mods, srt, feat, 2, True).query_grad(x.to(DEV))
    err = float((grad.cpu().double() - g64).abs().max())
    print(f"centre: gradient {grad.cpu().tolist()}, error {err:.3e}, tolerance {tol:.3e}")
    assert float(g64.abs().max()) > 0 and err <= tol


def test_uncovered_points_without_the_fill_have_exactly_zero_gradient(mods):
    x, srt, feat, _ = _inputs(33, 3, 300)
    x = x * 0.01 + 5.0                                                # far from every primitive
    out, grad = _module(mods, srt, feat, 3, True).query_grad(x.to(DEV))
    assert int((grad != 0).sum()) == 0 and int((out != 0).sum()) == 0


def test_uncovered_points_with_the_fill_follow_the_written_out_gradient(mods):
    x, srt, feat, _ = _inputs(33, 3, 4099)
    x = torch.cat([x, x[:300] * 0.01 + 5.0])                          # ... and some far from every primitive
    unc = ~NM.covered(x, srt)
    v64, g64, margin = NM.fill_value_grad(x, srt, feat, 3, np.float64)
    v32, g32, _ = NM.fill_value_grad(x, srt, feat, 3, np.float32)
    bad = (torch.from_numpy(margin < DELTA) | G.kinks(x, srt, feat, 3, DELTA)) & unc
    keep = (unc & ~bad).numpy()
    dropped = float(bad.sum()) / float(unc.sum())
    tol_g = 4 * float(np.abs(g32.astype(np.float64) - g64)[keep].max()) + ULP * float(np.abs(g64[keep]).max())
    tol_v = 4 * float(np.abs(v32.astype(np.float64) - v64)[keep].max()) + ULP * float(np.abs(v64[keep]).max())
    out, grad = _module(mods, srt, feat, 3, False).query_grad(x.to(DEV))
    err_g = float(np.abs(grad.cpu().double().numpy() - g64)[keep].max())
    err_v = float(np.abs(out[:, 0].cpu().double().numpy() - v64)[keep].max())
    print(f"fill: {int(keep.sum())} uncovered points of {x.shape[0]}, {100 * dropped:.3f} % dropped near a tie; gradient error {err_g:.3e} "
          f"(tolerance {tol_g:.3e}), value error {err_v:.3e} (tolerance {tol_v:.3e})")
    assert keep.sum() > 500 and dropped <= MAX_DROPPED
    assert err_g <= tol_g and err_v <= tol_v
    length = np.linalg.norm(grad.cpu().double().numpy()[keep], axis=1)
    assert float(np.abs(length - 1).max()) < 1e-5                     # a distance field: unit gradient (no stored sdf is 0 here)


def test_two_runs_give_equal_bits(mods):
    r = _case(1025, 8, 4099)
    x = r["x"].to(DEV)
    for training in (True, False):
        m = _module(mods, r["srt"], r["feat"], 8, training)
        a, b = m.query_grad(x), m.query_grad(x)
        assert fp.same_bits(a[0], b[0]) and fp.same_bits(a[1], b[1])


def test_normals_are_unit_or_zero_and_point_outward(mods):
    field = _shell_field()
    mesh = mods.M.extract_mesh(field, RES)
    nrm = mods.M.field_normals(field, mesh.v, chunk=1000)             # several chunks
    assert torch.equal(nrm, field.normals(mesh.v))
    length = nrm.norm(dim=1)
    assert bool((((length - 1).abs() < 1e-5) | (length == 0)).all())
    assert bool(NM.covered(mesh.v.cpu(), field.srt_param.detach().cpu()).all())     # the layout covers the surface
    along = (nrm * mesh.normals).sum(1)
    print(f"field normals . marching cubes' lattice normals at {mesh.v.shape[0]} vertices: min {float(along.min()):.4f}, "
          f"mean {float(along.mean()):.4f}")
    assert float(along.min()) > 0                                     # the orientation of marching_cubes(return_normals=True)
    assert float((nrm * torch.nn.functional.normalize(mesh.v, dim=1)).sum(1).min()) > 0       # outward, towards higher sdf
    far = torch.full((3, 3), 5.0, device=DEV)
    assert int((field.train().normals(far) != 0).sum()) == 0
    with pytest.raises(RuntimeError, match="HIP device"):
        field.query_grad(torch.zeros(2, 3))


# ------------------------------------------------------------------------------------------------ the small export
class _Bake:
    """The stages of mesh.bake_textures(normal_map=True) on a small field, kept for the tests below (computed once)."""

    def __init__(self, mods, noise):
        M = mods.M
        field = mods.synth.sphere_field(DEV, 96, 8, noise) if noise else _shell_field()
        self.field = M._filtered_copy(field, M.noise_filter_mask(field.srt_param.detach()))     # as extract_texmesh filters it
        self.mesh = M.extract_mesh(self.field, RES, filter_noise=False, clean=bool(noise))
        self.atlas = M.uv_unwrap(self.mesh.v, self.mesh.f, self.mesh.normals, (ATLAS, ATLAS))
        self.normals = self.mesh.normals[self.atlas.vmap].contiguous()
        self.tangents = M.atlas_tangents(self.atlas, self.normals)
        self.texel, self.pts = M.atlas_points(self.atlas, self.mesh.v, self.mesh.f)
        self.g = M.field_normals(self.field, self.pts)
        self.nts, self.attr = M.texel_normals(self.atlas, self.texel, self.normals, self.tangents, self.g, with_attr=True)
        c = lambda t: t.cpu().numpy()   # noqa: E731
        self.h = dict(nrm=c(self.normals), tan=c(self.tangents), ft=c(self.atlas.f), label=c(self.atlas.label), fid=c(self.atlas.face_id),
                      uv=c(self.atlas.uv_fixed), vt=c(self.atlas.vt), v=c(self.mesh.v)[c(self.atlas.vmap)], texel=c(self.texel),
                      pts=c(self.pts), g=c(self.g), nts=c(self.nts))


@functools.lru_cache(maxsize=None)
def _bake(mods, noise):
    return _Bake(mods, noise)


# ------------------------------------------------------------------------------------------------ 3. tangents
def test_tangents_on_the_atlas_of_a_small_mesh(mods):
    """Unit, orthogonal to the normal, w = +-1, T along every face's d pos / d u and w cross(N, T) along its -d pos / d v (up the
    image), and the restated rule within fp32 rounding.  A face's UV derivatives are only as good as its snapped corners: each
    coordinate carries up to 1/512 texel, so faces whose UV height (twice the area over the longest edge) is under 1/16 texel - a
    few dozen times that error - are left out as degenerate."""
    b = _bake(mods, 6)
    h = b.h
    T, w, N = h["tan"][:, :3].astype(np.float64), h["tan"][:, 3], h["nrm"].astype(np.float64)
    assert T.shape[0] == h["vt"].shape[0] > 0 and set(np.unique(w)) <= {-1.0, 1.0}
    assert float(np.abs(np.linalg.norm(T, axis=1) - 1).max()) <= 1e-5
    assert float(np.abs((T * N).sum(1)).max()) <= 1e-5
    ft = h["ft"].astype(np.int64)
    texels = h["vt"].astype(np.float64) * ATLAS
    dpdu, dpdv, det = NM.uv_derivatives(h["v"][ft], texels[ft])
    edge = np.stack([np.linalg.norm(texels[ft][:, (k + 1) % 3] - texels[ft][:, k], axis=1) for k in range(3)], 1).max(1)
    good = np.abs(det) >= edge / 16.0
    print(f"tangents: {T.shape[0]} split vertices, {ft.shape[0]} faces, {int((~good).sum())} of degenerate UV area, "
          f"w = +1 at {int((w > 0).sum())} vertices")
    assert good.mean() > 0.9 and bool((det[good] > 0).all())         # charts keep their faces' orientation
    B = w[:, None] * np.cross(N, T)
    for k in range(3):
        vi = ft[good, k]
        assert bool(((T[vi] * dpdu[good]).sum(1) > 0).all())
        assert bool(((B[vi] * -dpdv[good]).sum(1) > 0).all())
    t64 = NM.tangents(h["nrm"], h["ft"], h["label"], np.float64)
    t32 = NM.tangents(h["nrm"], h["ft"], h["label"], np.float32)
    floor = float(np.abs(t32.astype(np.float64) - t64).max())
    tol = 4 * floor + ULP
    err = float(np.abs(h["tan"].astype(np.float64) - t64).max())
    print(f"tangents vs the restated rule: max-abs error {err:.3e}, tolerance {tol:.3e} (fp32 restatement's own error {floor:.3e})")
    assert err <= tol
    assert fp.same_bits(b.tangents, mods.M.atlas_tangents(b.atlas, b.normals))


# ------------------------------------------------------------------------------------------------ 4. texel normals and bytes
def test_texel_normals_and_the_baked_bytes(mods):
    """Bounds.  eps = 1 / 255 + tol: a decoded byte is within half a quantisation step (1 / 255 in normal units) of the fp32 value
    it encodes, and that is within tol of the float64 one.  The frame (T_i, B, N_i) is orthonormal, so the rebuilt world normal
    differs from the field normal g by the Euclidean distance of the renormalised decoded vector from n_ts: at most sqrt(3) eps
    for the decoded vector, and renormalising a vector within r of a unit vector moves it by at most r again: 2 sqrt(3) eps."""
    M = mods.M
    b = _bake(mods, 0)
    h = b.h
    lam, face = NM.barycentrics(h["texel"], h["fid"], h["uv"], h["ft"])
    # (a) the kernel against its restatement, on the kernel's own operands
    r64, _, ok = NM.texel_normals(lam, face, h["ft"], h["nrm"], h["tan"], h["g"], np.float64)
    r32, _, _ = NM.texel_normals(lam, face, h["ft"], h["nrm"], h["tan"], h["g"], np.float32)
    floor = float(np.abs(r32.astype(np.float64) - r64).max())
    err = float(np.abs(h["nts"].astype(np.float64) - r64).max())
    print(f"texel normals: {len(face)} covered texels; max-abs error {err:.3e}, tolerance {4 * floor + ULP:.3e} (fp32 restatement's own "
          f"error {floor:.3e})")
    assert ok.all() and err <= 4 * floor + ULP
    assert float(np.abs(np.linalg.norm(h["nts"], axis=1) - 1).max()) < 1e-5 and float(h["nts"][:, 2].min()) > 0.5
    # (b) the baked map against the float64 chain: float64 field normal at the texel point, float64 transform
    tm = M.bake_textures(b.field, b.mesh, ATLAS, fill_radius=RADIUS, normal_map=True)
    assert fp.same_bits(tm.tangents, b.tangents) and tm.normal_map.dtype == torch.uint8 and tuple(tm.normal_map.shape) == (ATLAS, ATLAS, 3)
    srt, feat, pts = b.field.srt_param.detach().cpu(), b.field.feat_param.detach().cpu(), b.pts.cpu()
    keep = (~G.kinks(pts, srt, feat, 8, DELTA) & NM.covered(pts, srt)).numpy()
    g64 = NM.unit(NM.point_grad(pts, srt, feat, 8, torch.float64)[1].numpy())
    g32 = NM.unit(NM.point_grad(pts, srt, feat, 8, torch.float32)[1].numpy(), np.float32)
    n64, (Ti, Bi, Ni), _ = NM.texel_normals(lam, face, h["ft"], h["nrm"], h["tan"], g64, np.float64)
    n32, _, _ = NM.texel_normals(lam, face, h["ft"], h["nrm"], h["tan"], g32, np.float32)
    tol = 4 * float(np.abs(n32.astype(np.float64) - n64)[keep].max()) + ULP
    eps = QUANT + tol
    nmap = tm.normal_map.cpu().numpy()
    dec = NM.decode(nmap.reshape(-1, 3)[h["texel"]])
    err_b = float(np.abs(dec - n64)[keep].max())
    print(f"baked bytes: {100 * (1 - keep.mean()):.3f} % of the texel points dropped (kinks, uncovered); decoded vs float64 {err_b:.3e}, bound "
          f"1 / 255 + {tol:.3e} = {eps:.3e}")
    assert 1 - keep.mean() <= MAX_DROPPED and err_b <= eps
    # (c) the world normal rebuilt by the glTF rule from the map, TANGENT and NORMAL
    nd = NM.unit(dec)
    world = nd[:, 0:1] * Ti + nd[:, 1:2] * Bi + nd[:, 2:3] * Ni
    bound = 2 * np.sqrt(3.0) * eps
    err_c = float(np.linalg.norm(world - g64, axis=1)[keep].max())
    print(f"rebuilt world normal vs the float64 field normal: {err_c:.3e}, bound 2 sqrt(3) (1 / 255 + tol) = {bound:.3e}")
    assert err_c <= bound
    # (d) ... and against the analytic radial direction of the sphere
    radial = NM.unit(h["pts"].astype(np.float64))
    own = float(np.linalg.norm(g64 - radial, axis=1)[keep].max())
    err_d = float(np.linalg.norm(world - radial, axis=1)[keep].max())
    print(f"rebuilt world normal vs radial: {err_d:.3e}; the float64 field normal's own deviation {own:.3e} + the bound above")
    assert own < 0.5 and err_d <= own + bound
    # (e) the fill: primx_texbake_fill's own, on the encoded bytes; texels beyond its radius are flat
    cov = h["fid"] >= 0
    assert np.array_equal(nmap.reshape(-1, 3)[h["texel"]], NM.encode(h["nts"], np.float32))
    like = np.zeros((len(face), 6), np.float32)
    like[:, 1:4] = (NM.encode(h["nts"], np.float32).astype(np.float32) + np.float32(0.5)) / np.float32(255)
    assert np.array_equal(b.attr.cpu().numpy(), like)
    want, _ = tb.fill(like, h["texel"], cov, RADIUS, 3)
    inpaint, _ = tb.fill_regions(cov, RADIUS, 3)
    beyond = ~cov & ~inpaint
    want[beyond] = (128, 128, 255)
    assert beyond.sum() > 100 and inpaint.sum() > 100 and np.array_equal(nmap, want)
    assert np.array_equal(tm.covered.cpu().numpy(), cov)


# ------------------------------------------------------------------------------------------------ 5. the default path
def _glb_json(path):
    with open(path, "rb") as fh:
        data = fh.read()
    magic, version, total = struct.unpack_from("<III", data, 0)
    n, kind = struct.unpack_from("<II", data, 12)
    assert magic == 0x46546C67 and version == 2 and total == len(data) and kind == 0x4E4F534A
    return json.loads(data[20:20 + n]), data


def test_default_path_is_unchanged(mods, tmp_path):
    M = mods.M
    b = _bake(mods, 0)
    plain = M.bake_textures(b.field, b.mesh, ATLAS, fill_radius=RADIUS)
    withmap = M.bake_textures(b.field, b.mesh, ATLAS, fill_radius=RADIUS, normal_map=True)
    assert plain.tangents is None and plain.normal_map is None and withmap.normal_map is not None
    for name in ("v", "f", "normals", "vt", "vmap", "albedo", "metallic_roughness", "covered"):
        assert fp.same_bits(getattr(plain, name), getattr(withmap, name)), name
    plain.write_glb(str(tmp_path / "plain.glb"))
    dataclasses.replace(withmap, tangents=None, normal_map=None).write_glb(str(tmp_path / "stripped.glb"))
    js, data = _glb_json(str(tmp_path / "plain.glb"))
    assert len(js["images"]) == 2 and len(js["textures"]) == 2 and "normalTexture" not in js["materials"][0]
    assert "TANGENT" not in js["meshes"][0]["primitives"][0]["attributes"]
    assert data == open(str(tmp_path / "stripped.glb"), "rb").read()


# ------------------------------------------------------------------------------------------------ 6. the decimated pipeline
def test_extract_texmesh_with_decimation_and_a_normal_map(mods, tmp_path):
    from topia_xl_amd import pipeline
    M = mods.M
    field = mods.synth.sphere_field(DEV, 96, 8, 6)
    full = M.extract_mesh(field, RES)
    target = full.f.shape[0] // 3
    stats = {}
    tm = M.extract_texmesh(field, RES, ATLAS, decimate=target, normal_map=True, stats=stats)
    print(f"decimated {stats['faces_before']} -> {stats['faces_after']} faces; {tm.v.shape[0]} split vertices")
    nv, nf = tm.v.shape[0], tm.f.shape[0]
    assert 0 < nf <= target * 1.05 and stats["faces_after"] == nf
    assert tuple(tm.tangents.shape) == (nv, 4) and tuple(tm.normals.shape) == (nv, 3) and int(tm.f.max()) == nv - 1
    t = tm.tangents.cpu().double()
    assert float((t[:, :3].norm(dim=1) - 1).abs().max()) <= 1e-5 and bool((t[:, 3].abs() == 1).all())
    assert float((t[:, :3] * tm.normals.cpu().double()).sum(1).abs().max()) <= 1e-5
    path = str(tmp_path / "decimated.glb")
    tm.write_glb(path)
    js, _ = _glb_json(path)
    prim = js["meshes"][0]["primitives"][0]
    acc = js["accessors"]
    for name, typ in (("POSITION", "VEC3"), ("NORMAL", "VEC3"), ("TEXCOORD_0", "VEC2"), ("TANGENT", "VEC4")):
        a = acc[prim["attributes"][name]]
        assert a["count"] == nv and a["type"] == typ and a["componentType"] == 5126, name
    assert acc[prim["indices"]]["count"] == 3 * nf and len(js["images"]) == 3
    assert js["materials"][0]["normalTexture"] == {"index": 2, "scale": 1.0}
    view = js["bufferViews"][js["images"][2]["bufferView"]]
    with open(path, "rb") as fh:
        blob = fh.read()
    start = 20 + struct.unpack_from("<I", blob, 12)[0] + 8 + view["byteOffset"]
    assert np.array_equal(M.decode_png(blob[start:start + view["byteLength"]])[..., :3], tm.normal_map.cpu().numpy())
    # the pipeline's pass-through
    recon = torch.cat([field.srt_param.detach(), field.feat_param.detach()], 1)
    via = pipeline.primitives_to_texmesh(recon, RES, ATLAS, decimate=target, normal_map=True)
    assert fp.same_bits(via.normal_map, tm.normal_map) and fp.same_bits(via.tangents, tm.tangents)
    tm.write_textures(str(tmp_path / "tex"))
    assert np.array_equal(M.decode_png(open(str(tmp_path / "tex" / "normal.png"), "rb").read())[..., :3], tm.normal_map.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 7. footprint and stream order
def test_footprint_of_the_three_entry_points(mods):
    """Inside footprint.hold: intact guards around every output, untouched const operands, no allocation past the wrapper, and
    results that depend neither on the fill of torch.empty nor on the guard (bit for bit: nothing here is atomic)."""
    M = mods.M
    b = _bake(mods, 0)
    r = _case(1025, 8, 4099)

    def case(g):
        x, srt, feat = (g.guard_input(r[k].to(DEV).contiguous(), k).t for k in ("x", "srt", "feat"))
        outs = []
        for training in (True, False):
            m = mods.primsdf.PrimSDF(num_prims=1025, prim_shape=8).to(DEV).train(training)
            m.srt_param.data, m.feat_param.data = srt, feat
            outs.append(m.query_grad(x))
        gi = lambda t, name: g.guard_input(t, name).t   # noqa: E731
        atlas = dataclasses.replace(b.atlas, f=gi(b.atlas.f, "ft"), label=gi(b.atlas.label, "label"), uv_fixed=gi(b.atlas.uv_fixed, "uv"),
                                    face_id=gi(b.atlas.face_id, "face_id"))
        nrm, texel, gn = gi(b.normals, "normals"), gi(b.texel, "texel"), gi(b.g, "g")
        tan = M.atlas_tangents(atlas, nrm)
        outs.append([tan, M.texel_normals(atlas, texel, nrm, tan, gn, with_attr=True), M.texel_normals(atlas, texel, nrm, tan, gn)])
        return outs

    out = fp.hold(case)
    assert fp.same_bits(out[2][0], b.tangents) and fp.same_bits(out[2][1][0], b.nts) and fp.same_bits(out[2][2], b.nts)


@TS.case("primsdf_query_grad", ["primx_primsdf_query_grad"])
def _stream_query_grad(E, dtype):  # noqa: F811
    from topia_xl_amd.primsdf import PrimSDF

    def setup():
        return PrimSDF(num_prims=1025, prim_shape=8).to(DEV).eval()  # two LDS chunks of primitives, the fill on

    def make(k):
        x, srt, feat, _ = _inputs(1025, 8, 257, seed=k)
        return {"srt": srt.to(DEV).contiguous(), "feat": feat.to(DEV).contiguous(), "x": x.to(DEV).contiguous()}

    def call(m, i, probe):
        m.srt_param.data, m.feat_param.data = i["srt"], i["feat"]
        return TS.twice(lambda: list(m.query_grad(i["x"])) + [m.normals(i["x"])], probe)
    return make, call, setup


@TS.case("normal_map_texels", ["primx_texbake_tangents", "primx_texbake_normal_texels"])
def _stream_normal_map(E, dtype):  # noqa: F811
    """The atlas of the small export; the split vertices' normals and the field normals at the texels are the late operands, and so
    are the index arrays (their poison is 0: a wrong but addressable value)."""
    from topia_xl_amd import mesh as M
    field = _shell_field()
    mesh = M.extract_mesh(field, RES)
    atlas = M.uv_unwrap(mesh.v, mesh.f, mesh.normals, (ATLAS, ATLAS))
    texel, pts = M.atlas_points(atlas, mesh.v, mesh.f)
    normals, g = mesh.normals[atlas.vmap].contiguous(), M.field_normals(field, pts)

    def make(k):
        turn = lambda t: torch.nn.functional.normalize(t + 0.2 * k * t.roll(1, 1), dim=1).contiguous()   # noqa: E731
        return {"normals": turn(normals), "g": turn(g), "texel": texel.clone(), "ft": atlas.f.clone(), "label": atlas.label.clone(),
                "uv": atlas.uv_fixed.clone(), "fid": atlas.face_id.clone()}

    def call(ctx, i, probe):
        a = dataclasses.replace(atlas, f=i["ft"], label=i["label"], uv_fixed=i["uv"], face_id=i["fid"])
        tan = M.atlas_tangents(a, i["normals"])
        return [tan] + list(M.texel_normals(a, i["texel"], i["normals"], tan, i["g"], with_attr=True))
    return make, call, None


STREAM_CASES = ("primsdf_query_grad", "normal_map_texels")


@pytest.mark.parametrize("name", STREAM_CASES)
def test_stream_order_of_the_normal_map_entry_points(E, called, name):  # noqa: F811  (`called` is the imported fixture)
    """The body of tests/test_hip_streams.py::test_stream_order for the cases registered above; no host synchronisation is documented."""
    c = TS.CASES[name]
    make, call, setup = c.build(E, None)
    rep = so.run(name, make, call, E.S, E.blocker, setup=setup, must_sync=False)
    print(rep.line())
    assert rep.verdict == so.OK, rep.message()
    missing = sorted(set(c.declares) - called)
    assert not missing, f"{name} declares entry points it did not call: {missing}"
