"""Forward ray marcher.  Parity is PINNED to the reference's own executable PyTorch statement
of the kernels: tests/golden/raymarch.npz holds the seeded scene and the outputs of the torch march loop
(dva/mvp/extensions/mvpraymarch/mvpraymarch.py:301-461, seed 1112) and of the torch ray-direction code
(dva/mvp/extensions/utils/utils.py:73-148, seed 1113), produced by tests/golden/make_golden_raymarch.py running those
lines unmodified.  CPU: the oracle restatement against that golden; GPU: the HIP kernels against the same golden and,
on a camera-driven scene with sub-volume primitives, against the (now pinned) oracle."""
import math

import numpy as np
import pytest
import torch

from oracle import raymarch_ref

DEV = "cuda:0"


def _golden_march(golden):
    g = golden("raymarch")
    T = lambda k: torch.from_numpy(g[k])
    return g, T


def test_oracle_march_loop_matches_reference_pytorch_loop(golden):
    """oracle/raymarch_ref.raymarch (restated from the CUDA kernels) == the reference's torch loop on its own seeded
    scene: 2 x 65 x 65 rays, 64 overlapping unit-scale primitives, 18 marching steps, all rays partly opaque."""
    g, T = _golden_march(golden)
    n = slice(0, 1)                                   # one of the two batch entries keeps the CPU suite quick
    tpl = T("march_template").permute(0, 1, 3, 4, 5, 2).contiguous()
    out = raymarch_ref.raymarch(T("march_raypos")[n], T("march_raydir")[n], T("march_tminmax")[n], float(g["march_stepsize"]),
                                T("march_primpos")[n], T("march_primrot")[n], T("march_primscale")[n], tpl[n],
                                float(g["march_fadescale"]), float(g["march_fadeexp"]))
    ref = T("march_rgba")[n]
    assert float(ref[..., 3].min()) > 0.5 and float(ref.abs().mean()) > 0.5          # a non-trivial image
    assert float((out - ref).abs().max()) < 1e-5, float((out - ref).abs().max())


def test_oracle_raydirs_match_reference_pytorch(golden):
    g, T = _golden_march(golden)
    rp, rd, tm = raymarch_ref.compute_raydirs(T("rays_viewpos"), T("rays_viewrot"), T("rays_focal"), T("rays_princpt"),
                                              T("rays_pixelcoords"), float(g["rays_volradius"]))
    assert float((rd - T("rays_raydir")).abs().max()) < 1e-6
    assert float((tm - T("rays_tminmax")).abs().max()) < 1e-5


@pytest.mark.gpu
def test_hip_kernels_match_reference_pytorch_golden(golden):
    """The HIP ray generator and marcher against the outputs of the reference's own PyTorch code (same seeded inputs).
    Stated tolerance: directions 1e-6, t-range 1e-5; image max-abs 2e-3, mean-abs 2e-5 (hardware exp2/log2 in the fade,
    fp32 re-association of the SRT transform), no pixel off by more than 2e-3."""
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import raymarch as rm
    g, T = _golden_march(golden)
    D = lambda k: T(k).to(DEV)
    rp, rd, tm = rm.compute_raydirs(D("rays_viewpos"), D("rays_viewrot"), D("rays_focal"), D("rays_princpt"),
                                    D("rays_pixelcoords"), float(g["rays_volradius"]))
    assert float((rd.cpu() - T("rays_raydir")).abs().max()) < 1e-6
    assert float((tm.cpu() - T("rays_tminmax")).abs().max()) < 1e-5
    tpl = D("march_template").permute(0, 1, 3, 4, 5, 2).contiguous()                  # channels-last, as the product path holds it
    img = rm.mvpraymarch(D("march_raypos"), D("march_raydir"), float(g["march_stepsize"]), D("march_tminmax"),
                         (D("march_primpos"), D("march_primrot"), D("march_primscale")), tpl,
                         float(g["march_fadescale"]), float(g["march_fadeexp"])).cpu()
    err = (img - T("march_rgba")).abs()
    print(f"HIP march vs reference torch loop: max {float(err.max()):.2e} mean {float(err.mean()):.2e}")
    assert float(err.max()) < 2e-3 and float(err.mean()) < 2e-5, (float(err.max()), float(err.mean()))


def _scene(seed=3, N=2, K=24, S=8, H=40, W=36):
    g = torch.Generator().manual_seed(seed)
    pos = 0.55 * (2 * torch.rand(N, K, 3, generator=g) - 1)
    rv = torch.randn(N, K, 3, generator=g)
    th = rv.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    ax = rv / th
    Kx = torch.zeros(N, K, 3, 3)
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -ax[..., 2], ax[..., 1], ax[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -ax[..., 0], -ax[..., 1], ax[..., 0]
    rot = torch.eye(3) + torch.sin(th)[..., None] * Kx + (1 - torch.cos(th))[..., None] * (Kx @ Kx)
    scale = 1.0 / (0.12 + 0.2 * torch.rand(N, K, 3, generator=g))          # inverse half extents
    rgba = torch.rand(N, K, 4, S, S, S, generator=g)
    rgba[:, :, 3] = 6.0 * rgba[:, :, 3] ** 2                                # opacities large enough to saturate some rays
    ang = torch.tensor([0.3, -0.8])[:N]
    R = torch.stack([torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) for a in ang])
    campos = torch.stack([R[i].t() @ torch.tensor([0.0, 0.1, -3.0]) for i in range(N)])
    RT = torch.cat([R, (-R @ campos[..., None])], dim=-1)
    Kc = torch.tensor([[[1.4 * W, 0, W / 2], [0, 1.4 * W, H / 2], [0, 0, 1]]]).repeat(N, 1, 1)
    return rgba, pos, rot, scale, Kc, RT, H, W


@pytest.mark.gpu
def test_raydirs_and_march_against_oracle():
    import __graft_entry__
    __graft_entry__.build()
    from topia_xl_amd import raymarch as rm
    rgba, pos, rot, scale, Kc, RT, H, W = _scene()
    volradius, dt = 1.0, 0.02
    m = rm.RayMarcher(H, W, volradius, dt=dt).eval()
    out = m(rgba.to(DEV), pos.to(DEV), rot.to(DEV), scale.to(DEV), Kc.to(DEV), RT.to(DEV))
    img = out["rgba_image"].cpu()
    assert img.shape == (2, 4, H, W) and out["pixel_coords"].shape == (2, H, W, 2)
    # rays
    campos, camrot, focal, princpt = raymarch_ref.convert_camera(RT, Kc)
    pc = out["pixel_coords"].cpu()
    rp, rd, tmm = raymarch_ref.compute_raydirs(campos, camrot, focal, princpt, pc, volradius)
    grp, grd, gtm = rm.compute_raydirs(campos.to(DEV), camrot.to(DEV), focal.to(DEV), princpt.to(DEV), pc.to(DEV), volradius)
    assert (grp.cpu() - rp).abs().max() < 1e-6 and (grd.cpu() - rd).abs().max() < 1e-5
    # a generic camera: every t is finite on both sides, so ALL of the t-range is compared (tests/test_hip_raydirs.py holds the
    # cameras whose rays have exact zeros and infinities, element by element)
    assert bool(torch.isfinite(tmm).all()) and bool(torch.isfinite(gtm).all())
    assert (gtm.cpu() - tmm).abs().max() < 1e-4
    # image: march the oracle on the DEVICE's rays (so that step alignment is compared, not ray rounding)
    ref = raymarch_ref.raymarch(grp.cpu(), grd.cpu(), gtm.cpu(), dt / volradius, pos / volradius, rot, scale,
                                rgba.permute(0, 1, 3, 4, 5, 2).contiguous(), 8.0, 8.0)
    ref = ref.permute(0, 3, 1, 2)
    err = (img - ref).abs()
    assert float(ref[:, 3].max()) > 0.99 and float((ref[:, 3] > 0).float().mean()) > 0.2    # saturated and empty rays both present
    # fast-math exp/pow in the fade and one-ulp step-boundary decisions: a handful of pixels may differ visibly
    assert float(err.mean()) < 2e-4, float(err.mean())
    assert float((err > 5e-3).float().mean()) < 2e-3, float((err > 5e-3).float().mean())


def test_cpu_tensors_are_refused():
    from topia_xl_amd import raymarch as rm
    rgba, pos, rot, scale, Kc, RT, H, W = _scene(N=1, K=2, H=8, W=8)
    with pytest.raises(RuntimeError):
        rm.RayMarcher(H, W, 1.0).eval()(rgba, pos, rot, scale, Kc, RT)
