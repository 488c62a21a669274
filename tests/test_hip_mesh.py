"""Mesh export on the MI355X (csrc/mcubes.hip, mesh.py): marching cubes against the numpy restatement in exact output
order, topology on analytic level sets, edge cases, the noise filter against the reference's torch code on the CPU
(inference.py:89-103), and extract_mesh against the field query and the PrimSDF oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import primsdf_ref, synth
from tests import mc_numpy
from tests.test_mesh_cpu import parse_glb

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mesh():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import mesh as M
    return M


def _mc(M, vol, iso=0.0):
    v, f, n = M.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(DEV), iso,
                               return_normals=True)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    return v.cpu().numpy(), n.cpu().numpy(), f.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("shape", [(17, 23, 31), (64, 64, 64)])
@pytest.mark.parametrize("iso", [0.0, 0.3])
def test_exact_order_against_numpy(mesh, shape, iso):
    vol = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    v, n, f = _mc(mesh, vol, iso)
    rv, rn, rf = mc_numpy.marching_cubes(vol, iso)
    assert v.shape == rv.shape and f.shape == rf.shape and len(f) > 0
    np.testing.assert_allclose(v, rv, rtol=0, atol=1e-6)
    np.testing.assert_allclose(n, rn, rtol=0, atol=1e-5)
    np.testing.assert_array_equal(f, rf)


@pytest.mark.parametrize("n", [64, 96])
def test_topology_on_analytic_fields(mesh, n):
    for name, (vol, va, chi, grad) in mc_numpy.analytic_fields(n).items():
        assert mc_numpy.ambiguous_faces(vol) == 0, name          # no choice left to the table on these level sets
        v, nrm, f = _mc(mesh, vol)
        euler, volume = mc_numpy.mesh_checks(v, f)              # watertight, oriented, no repeated index in a triangle
        assert volume > 0, name
        if chi is not None:
            assert euler == chi, (name, euler)
        if va is not None:
            assert abs(volume / va - 1) < 0.01, (name, volume, va)
        if grad is not None:
            dots = np.einsum("ij,ij->i", nrm.astype(np.float64), grad(v.astype(np.float64)))
            assert dots.min() > 0.999, (name, dots.min())


def test_vertex_count_at_256(mesh):
    x = np.linspace(0, 6 * np.pi, 256, dtype=np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    vol = (np.sin(X) * np.cos(Y) + np.sin(Y) * np.cos(Z) + np.sin(Z) * np.cos(X)).astype(np.float32)   # a gyroid
    v, f = mesh.marching_cubes(torch.from_numpy(vol).to(DEV))
    assert v.shape[0] == mc_numpy.sign_changing_edges(vol) and f.shape[0] > v.shape[0]


def test_bitwise_deterministic(mesh):
    vol = torch.randn(96, 80, 72, generator=torch.Generator().manual_seed(3)).to(DEV)
    a = mesh.marching_cubes(vol, 0.1, return_normals=True)
    b = mesh.marching_cubes(vol, 0.1, return_normals=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_edge_cases(mesh):
    for fill in (1.0, -1.0):                                      # all outside / all inside: nothing to emit
        v, f = mesh.marching_cubes(torch.full((9, 10, 11), fill, device=DEV))
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3)
        vn, fn = mesh.marching_cubes(np.full((9, 10, 11), fill, dtype=np.float32))
        assert vn.shape == (0, 3) and fn.shape == (0, 3) and vn.dtype == np.float64 and fn.dtype == np.int64
    # values exactly at the iso level: inside is value < iso, so they are outside and t may be 0 or 1
    vol = np.random.default_rng(1).integers(-1, 2, size=(12, 13, 14)).astype(np.float32)
    v, n, f = _mc(mesh, vol, 0.0)
    rv, rn, rf = mc_numpy.marching_cubes(vol, 0.0)
    np.testing.assert_allclose(v, rv, rtol=0, atol=1e-6)
    np.testing.assert_array_equal(f, rf)
    assert np.isfinite(n).all()
    # the smallest lattice, every one of the 256 cases
    for case in range(256):
        vol = np.array([(-1.0 if case >> b & 1 else 1.0) for b in range(8)], dtype=np.float32)
        vol = vol.reshape(2, 2, 2).transpose(2, 1, 0).copy()   # corner b at (b & 1, b >> 1 & 1, b >> 2 & 1)
        v, n, f = _mc(mesh, vol)
        rv, rn, rf = mc_numpy.marching_cubes(vol)
        np.testing.assert_allclose(v, rv, rtol=0, atol=1e-6)
        np.testing.assert_array_equal(f, rf)
        assert len(f) == len(mc_numpy.TRI[case]) // 3
    # an oversized request is refused before any launch
    from topia_xl_amd import _lib
    h = _lib.load()
    small = torch.zeros(8, device=DEV)
    tot = torch.zeros(2, dtype=torch.int64, device=DEV)
    assert h.primx_mcubes_count(small.data_ptr(), 2048, 1024, 512, 0.0, small.data_ptr(), 1 << 40, tot.data_ptr(),
                                None) == -1
    assert b"2^31" in h.primx_last_error()
    ws = C.c_int64(0)
    assert h.primx_mcubes_workspace(1024, 1024, 1024, C.byref(ws)) == -1


def _reference_mask(srt):
    """inference.py:89-103 as the reference runs it, on the CPU."""
    prim_position = srt[:, 1:4]
    prim_scale = srt[:, 0:1]
    dist = torch.sqrt(torch.sum((prim_position[:, None, :] - prim_position[None, :, :]) ** 2, dim=-1))
    dist += torch.eye(prim_position.shape[0]).to(srt)
    min_dist, min_indices = dist.min(1)
    dst_prim_scale = prim_scale[min_indices, :]
    min_scale_converage = prim_scale * 1. + dst_prim_scale * 1.
    return min_dist < min_scale_converage[:, 0]


def test_noise_filter_bit_exact(mesh):
    gen = torch.Generator().manual_seed(11)
    for P in (1, 7, 300, 2048):
        srt = torch.cat([0.02 + 0.06 * torch.rand(P, 1, generator=gen), 1.6 * torch.rand(P, 3, generator=gen) - 0.8], 1)
        if P >= 7:
            srt[0, 1:] = torch.tensor([5.0, 5.0, 5.0])                      # no neighbour within 1
            srt[1, 1:], srt[2, 1:], srt[3, 1:] = 0.0, 0.0, 0.0              # exact ties: 2 and 3 both at distance 0 of 1
            srt[2, 0], srt[3, 0] = 0.5, 0.001
            # an exact tie at a distance where the scale of the arg-min decides: 5 and 6 both 0.25 from 4 (first wins)
            srt[4, 1:], srt[5, 1:], srt[6, 1:] = torch.tensor([3.0, 3.0, 3.0]), torch.tensor([3.25, 3.0, 3.0]), torch.tensor([2.75, 3.0, 3.0])
            srt[4, 0], srt[5, 0], srt[6, 0] = 0.05, 0.5, 0.01
        got = mesh.noise_filter_mask(srt.to(DEV)).cpu()
        ref = _reference_mask(srt)
        assert got.dtype == torch.bool and torch.equal(got, ref), (P, (got != ref).nonzero())
        if P >= 7:
            assert not bool(got[0]) and bool(got[4])


def _synthetic_field(P=96, S=8, noise=6):
    """oracle.synth.sphere_field with a few isolated noise primitives, on the test device."""
    return synth.sphere_field(DEV, P, S, noise)


def test_extract_mesh(mesh, tmp_path):
    field = _synthetic_field()
    srt0, feat0 = field.srt_param.detach().cpu(), field.feat_param.detach().cpu()
    R = 48
    out = mesh.extract_mesh(field, resolution=R, filter_noise=False)
    # = marching cubes of the lattice the existing query produces
    pts = mesh.lattice_points(R, DEV)
    grid = field.query(pts)[:, 0].reshape(R, R, R)
    v, f, n = mesh.marching_cubes(grid, 0.0, return_normals=True)
    assert torch.equal(out.v, v / (R - 1.0) * 2.0 - 1.0) and torch.equal(out.f, f) and torch.equal(out.normals, n)
    assert out.f.shape[0] > 1000
    # attributes = the field query at the returned vertices, and the oracle within 2e-5
    q = field.query(out.v)
    assert torch.equal(out.albedo, q[:, 1:4]) and torch.equal(out.roughness, q[:, 4]) and torch.equal(out.metallic, q[:, 5])
    idx = torch.randperm(out.v.shape[0], generator=torch.Generator().manual_seed(0))[:2000]
    ref = primsdf_ref.primsdf_forward(srt0, feat0, out.v.cpu()[idx], field.prim_shape, training=False)
    assert (out.albedo.cpu()[idx] - ref["tex"]).abs().max() < 2e-5
    assert (torch.stack([out.roughness, out.metallic], 1).cpu()[idx] - ref["mat"]).abs().max() < 2e-5
    # the vertices lie on the level set, up to the field's jumps where primitive coverage starts / ends (~1 % here)
    assert float((ref["sdf"][:, 0].abs() < 2.0 / (R - 1)).float().mean()) > 0.97
    # with the filter: exactly the masked primitives, and the caller's field untouched
    mask = _reference_mask(srt0)
    assert not bool(mask[96:].any())
    filt = mesh.extract_mesh(field, resolution=R, filter_noise=True)
    from topia_xl_amd.primsdf import PrimSDF
    kept = PrimSDF(num_prims=int(mask.sum()), prim_shape=field.prim_shape)
    kept.srt_param.data, kept.feat_param.data = srt0[mask].clone(), feat0[mask].clone()
    exp = mesh.extract_mesh(kept.eval().to(DEV), resolution=R, filter_noise=False)
    for k in ("v", "f", "normals", "albedo", "roughness", "metallic"):
        assert torch.equal(getattr(filt, k), getattr(exp, k)), k
    assert filt.v.shape[0] < out.v.shape[0]                                  # the noise blobs' surfaces are gone
    assert torch.equal(field.srt_param.detach().cpu(), srt0) and torch.equal(field.feat_param.detach().cpu(), feat0)
    # the GLB parses back
    path = str(tmp_path / "mesh.glb")
    filt.write_glb(path)
    gltf, arrays = parse_glb(path)
    prim = gltf["meshes"][0]["primitives"][0]
    np.testing.assert_array_equal(arrays[prim["attributes"]["POSITION"]], filt.v.cpu().numpy())
    np.testing.assert_array_equal(arrays[prim["indices"]].reshape(-1, 3), filt.f.cpu().numpy())


def test_primitives_to_mesh(mesh):
    from topia_xl_amd import pipeline
    field = _synthetic_field()
    recon = torch.cat([field.srt_param.detach(), field.feat_param.detach()], 1)
    a = pipeline.primitives_to_mesh(recon, resolution=40)
    b = mesh.extract_mesh(field, resolution=40)
    assert torch.equal(a.v, b.v) and torch.equal(a.f, b.f) and torch.equal(a.albedo, b.albedo)
