"""TEST INFRASTRUCTURE ONLY: seeded marcher scenes at the shipped step (RayMarcher(volradius=10000, dt=1): 1e-4 of the
volume per step), each aimed at one part of csrc/raymarch.hip (see tests/test_raymarch_contract.py)."""
from __future__ import annotations

import math

import torch


def _rotations(g, N, K):
    rv = torch.randn(N, K, 3, generator=g)
    th = rv.norm(dim=-1, keepdim=True).clamp(min=1e-6)
    ax = rv / th
    Kx = torch.zeros(N, K, 3, 3)
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0] = -ax[..., 2], ax[..., 1], ax[..., 2]
    Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -ax[..., 0], -ax[..., 1], ax[..., 0]
    return torch.eye(3) + torch.sin(th)[..., None] * Kx + (1 - torch.cos(th))[..., None] * (Kx @ Kx)


def scene(seed=0, N=1, K=24, S=8, H=16, W=16, dist=3.0, spread=0.55, half=(0.08, 0.2), rotate=True, const=False,
          opacity=6.0, axis=False, focal=1.4, yaw=(0.3, -0.8), thin=None, face_on_axis=False):
    """-> (template [N,K,TD,TH,TW,4] channels-last, pos [N,K,3], rot [N,K,3,3], scale [N,K,3], campos [N,3],
    camrot [N,3,3], focal [N,2], princpt [N,2]) in the normalised volume (volradius 1).  `dist` is the camera's distance
    from the centre in volume radii (< 1: inside the volume); axis=True looks straight down -z with unrotated primitives;
    face_on_axis=True (with axis and rotate=False) puts a face of primitives 0 and 1 exactly on the plane x = 0 that the
    centre column's rays lie in (ray direction x = 0, origin x = 0: r1.x = 0 and r0.x = -1 / +1 exactly)."""
    g = torch.Generator().manual_seed(seed)
    pos = spread * (2 * torch.rand(N, K, 3, generator=g) - 1)
    rot = _rotations(g, N, K) if rotate else torch.eye(3).expand(N, K, 3, 3).contiguous()
    scale = 1.0 / (half[0] + (half[1] - half[0]) * torch.rand(N, K, 3, generator=g))
    if thin is not None:
        scale[..., 2] = 1.0 / thin                  # slabs across the view direction: few steps per crossing
    if face_on_axis:
        scale[:, :2, 0] = 8.0                       # half extent 0.125 along x, centred at x = +-0.125
        pos[:, 0, :2] = torch.tensor([0.125, 0.0])
        pos[:, 1, :2] = torch.tensor([-0.125, 0.0])
    rgba = torch.rand(N, K, 4, S, S, S, generator=g)
    if const:
        rgba = rgba[..., :1, :1, :1].expand(-1, -1, -1, S, S, S).contiguous()
    rgba[:, :, 3] = opacity * rgba[:, :, 3] ** 2
    tpl = rgba.permute(0, 1, 3, 4, 5, 2).contiguous()
    Rs, cps = [], []
    for i in range(N):
        a = 0.0 if axis else yaw[i % len(yaw)]
        R = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        c = torch.tensor([0.0, 0.0 if axis else 0.1, -dist])
        Rs.append(R)
        cps.append(R.t() @ c)
    camrot, campos = torch.stack(Rs), torch.stack(cps)
    f = torch.tensor([[focal * W, focal * W]]).repeat(N, 1)
    pp = torch.tensor([[W / 2, H / 2]]).repeat(N, 1)
    if axis:
        pp = pp - 0.5   # the centre pixel's ray is exactly +z
    return tpl, pos, rot, scale, campos, camrot, f, pp


def rays(campos, camrot, focal, princpt, H, W):
    from oracle import raymarch_ref
    N = campos.shape[0]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    pc = torch.stack([xs, ys], -1)[None].expand(N, -1, -1, -1).contiguous()
    return pc, raymarch_ref.compute_raydirs(campos, camrot, focal, princpt, pc, 1.0)
