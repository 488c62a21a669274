"""Forward volumetric ray marcher - SURVEY.md section 8(f) row N2 (dva/ray_marcher.py:RayMarcher and the CUDA extension
behind it).  `RayMarcher` keeps the reference's constructor and `forward(prim_rgba, prim_pos, prim_rot, prim_scale, K, RT)`
-> {"rgba_image": [B, 4, H, W], "pixel_coords"}; the kernels are `primx_compute_raydirs`, `primx_raymarch` and, since ABI 35,
`primx_raymarch_backward` (csrc/raymarch.hip).  `mvpraymarch` is differentiable with respect to the template and the three
primitive transforms (mvpraymarch.py:162-213; rays get no gradient, as in the reference): under grad mode with an input that
requires a gradient it goes through a torch.autograd.Function whose forward is the same `primx_raymarch` call, so the image has
the same bits either way; `raymarch_backward` is the backward on its own.  In `.train()` with `ray_subsample_factor > 1`
`RayMarcher.forward` draws the reference's random ray subsample (ray_marcher.py:33-52)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _lib, ops


def convert_camera_parameters(Rt: torch.Tensor, K: torch.Tensor):
    """World-to-camera [R | t] and pinhole K -> the quantities the ray generator consumes (dva/ray_marcher.py:22-30):
    camera centre c = -R^T t, the rotation itself, the 2 x 2 focal block and the principal point.  (Two tiny batched
    products on a handful of floats: plumbing.)"""
    rot = Rt[:, :3, :3]
    centre = -torch.einsum("nji,nj->ni", rot, Rt[:, :3, 3])
    return {"campos": centre, "camrot": rot, "focal": K[:, :2, :2], "princpt": K[:, :2, 2]}


@ops.on_input_device
def compute_raydirs(viewpos, viewrot, focal, princpt, pixelcoords, volradius):
    N, H, W = pixelcoords.shape[0], pixelcoords.shape[1], pixelcoords.shape[2]
    dev = viewpos.device
    raypos = torch.empty(N, H, W, 3, dtype=torch.float32, device=dev)
    raydir = torch.empty_like(raypos)
    tminmax = torch.empty(N, H, W, 2, dtype=torch.float32, device=dev)
    # the dense fp32 copies must stay referenced until the launch is enqueued: a temporary dropped earlier returns its
    # block to the caching allocator, and the NEXT temporary's copy kernel would overwrite it ahead of our kernel
    keep = [t.float().contiguous() for t in (viewpos, viewrot, focal, princpt, pixelcoords)]
    ptrs = [ops._dev(t, name, torch.float32) for t, name in zip(keep, ("viewpos", "viewrot", "focal", "princpt", "pixelcoords"))]
    _lib.check(_lib.load().primx_compute_raydirs(*ptrs, float(volradius), raypos.data_ptr(), raydir.data_ptr(),
                                                 tminmax.data_ptr(), N, H, W, ops._stream()), "primx_compute_raydirs")
    del keep
    return raypos, raydir, tminmax


def _march_operands(raypos, primtransf, template):
    primpos, primrot, primscale = (t.float().contiguous() for t in primtransf)
    template = template.float().contiguous()
    if template.shape[-1] != 4:
        raise RuntimeError("mvpraymarch: the template must be channels-last RGBA")
    return primpos, primrot, primscale, template, tuple(raypos.shape[:3]), tuple(template.shape[1:5])


def _raymarch_forward(raypos, raydir, stepsize, tminmax, primpos, primrot, primscale, template, fadescale, fadeexp):
    (N, H, W), (K, TD, TH, TW) = tuple(raypos.shape[:3]), tuple(template.shape[1:5])
    out = torch.empty(N, H, W, 4, dtype=torch.float32, device=raypos.device)
    _lib.check(_lib.load().primx_raymarch(
        ops._dev(raypos, "raypos", torch.float32), ops._dev(raydir, "raydir", torch.float32),
        ops._dev(tminmax, "tminmax", torch.float32), float(stepsize), ops._dev(primpos, "primpos", torch.float32),
        ops._dev(primrot, "primrot", torch.float32), ops._dev(primscale, "primscale", torch.float32),
        ops._dev(template, "template", torch.float32), out.data_ptr(), N, H, W, K, TD, TH, TW, float(fadescale),
        float(fadeexp), ops._stream()), "primx_raymarch")
    return out


@ops.on_input_device
def raymarch_backward(raypos, raydir, stepsize, tminmax, primtransf, template, grad_rgba, fadescale=8.0, fadeexp=8.0, *,
                      gtemplate=None, gpos=None, grot=None, gscale=None, want=(True, True, True, True)):
    """primx_raymarch_backward: the gradients of a scalar loss with respect to (template, primpos, primrot, primscale), given
    grad_rgba [N, H, W, 4] = its gradient with respect to the image of `mvpraymarch` on the same operands.  The march is
    repeated inside the kernel; no forward output is needed.  -> (gtemplate, gpos, grot, gscale), fp32, shaped like the
    operands, None where `want` is False.  A caller's own accumulator (fp32, contiguous) is ADDED into and returned; otherwise the
    array starts from zeros.  The sums are fp32 atomics: not bitwise reproducible in general."""
    primpos, primrot, primscale, template, (N, H, W), (K, TD, TH, TW) = _march_operands(raypos, primtransf, template)
    grad_rgba = grad_rgba.float().contiguous()
    if tuple(grad_rgba.shape) != (N, H, W, 4):
        raise RuntimeError(f"raymarch_backward: grad_rgba must be [N, H, W, 4] = {(N, H, W, 4)}, got {tuple(grad_rgba.shape)}")
    if not any(want):
        raise RuntimeError("raymarch_backward: no gradient is wanted")
    outs = []
    for w, own, like, name in zip(want, (gtemplate, gpos, grot, gscale), (template, primpos, primrot, primscale),
                                  ("gtemplate", "gpos", "grot", "gscale")):
        if not w:
            outs.append(None)
            continue
        if own is None:
            own = torch.zeros_like(like)
        elif own.shape != like.shape or own.dtype != torch.float32 or not own.is_contiguous():
            raise RuntimeError(f"raymarch_backward: {name} must be a contiguous fp32 tensor of shape {tuple(like.shape)}")
        outs.append(own)
    ptr = lambda t, name: None if t is None else ops._dev(t, name, torch.float32)
    _lib.check(_lib.load().primx_raymarch_backward(
        ops._dev(raypos, "raypos", torch.float32), ops._dev(raydir, "raydir", torch.float32),
        ops._dev(tminmax, "tminmax", torch.float32), float(stepsize), ops._dev(primpos, "primpos", torch.float32),
        ops._dev(primrot, "primrot", torch.float32), ops._dev(primscale, "primscale", torch.float32),
        ops._dev(template, "template", torch.float32), ops._dev(grad_rgba, "grad_rgba", torch.float32),
        ptr(outs[0], "gtemplate"), ptr(outs[1], "gpos"), ptr(outs[2], "grot"), ptr(outs[3], "gscale"),
        N, H, W, K, TD, TH, TW, float(fadescale), float(fadeexp), ops._stream()), "primx_raymarch_backward")
    return tuple(outs)


class _RayMarch(torch.autograd.Function):
    """out = primx_raymarch; backward = primx_raymarch_backward for the inputs that need a gradient (none for the rays)."""

    @staticmethod
    def forward(ctx, template, primpos, primrot, primscale, raypos, raydir, tminmax, stepsize, fadescale, fadeexp):
        ctx.save_for_backward(template, primpos, primrot, primscale, raypos, raydir, tminmax)
        ctx.consts = (stepsize, fadescale, fadeexp)
        return _raymarch_forward(raypos, raydir, stepsize, tminmax, primpos, primrot, primscale, template, fadescale, fadeexp)

    @staticmethod
    def backward(ctx, grad_rgba):
        template, primpos, primrot, primscale, raypos, raydir, tminmax = ctx.saved_tensors
        stepsize, fadescale, fadeexp = ctx.consts
        want = tuple(ctx.needs_input_grad[:4])
        grads = raymarch_backward(raypos, raydir, stepsize, tminmax, (primpos, primrot, primscale), template, grad_rgba,
                                  fadescale, fadeexp, want=want)
        return (*grads, None, None, None, None, None, None)


def mvpraymarch(raypos, raydir, stepsize, tminmax, primtransf, template, fadescale=8.0, fadeexp=8.0):
    """template: [N, K, TD, TH, TW, 4] channels-last RGBA; primtransf = (pos [N,K,3], rot [N,K,3,3], scale [N,K,3]).
    Differentiable with respect to the template and the three transforms (see the module docstring)."""
    needs_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (template, *primtransf))
    primpos, primrot, primscale, template, _, _ = _march_operands(raypos, primtransf, template)
    if needs_grad:
        return _RayMarch.apply(template, primpos, primrot, primscale, raypos, raydir, tminmax, float(stepsize), float(fadescale),
                               float(fadeexp))
    return _raymarch_forward(raypos, raydir, stepsize, tminmax, primpos, primrot, primscale, template, fadescale, fadeexp)


def training_pixel_coords(base: torch.Tensor, batch_size: int, factor: int) -> torch.Tensor:
    """The reference's training-time random ray subsample (ray_marcher.py:33-52) of base [H, W, 2] -> [B, H // f, W // f, 2]: per
    batch item x0 then y0 are drawn with torch.randint(0, f - 1, size=()) from the global CPU generator - the exclusive upper
    bound is the reference's, so the offsets lie in [0, f - 2] - and the strided slice base[y0::f, x0::f] of SH x SW is taken.
    Works on tensors of any device (the draws are CPU scalars)."""
    H, W = base.shape[:2]
    sw, sh = W // factor, H // factor
    out = []
    for _ in range(batch_size):
        x0 = int(torch.randint(0, factor - 1, size=()))
        y0 = int(torch.randint(0, factor - 1, size=()))
        out.append(base[y0:y0 + factor * sh:factor, x0:x0 + factor * sw:factor, :])
    return torch.stack(out, dim=0).contiguous()


def base_pixel_coords(height: int, width: int, device="cpu") -> torch.Tensor:
    """[H, W, 2] (x, y) pixel centres, fp32."""
    ys, xs = torch.meshgrid(torch.arange(height, dtype=torch.float32, device=device),
                            torch.arange(width, dtype=torch.float32, device=device), indexing="ij")
    return torch.stack([xs, ys], dim=-1)


class RayMarcher(nn.Module):
    def __init__(self, image_height, image_width, volradius, fadescale=8.0, fadeexp=8.0, dt=1.0, ray_subsample_factor=1,
                 accum=2, termthresh=0.99, blocksize=None, with_t_img=True, chlast=False, assets=None):
        super().__init__()
        self.image_height, self.image_width = image_height, image_width
        self.volradius, self.dt = volradius, dt
        self.fadescale, self.fadeexp = fadescale, fadeexp
        self.accum, self.termthresh = accum, termthresh          # carried; the forward path uses additive accumulation
        self.ray_subsample_factor = ray_subsample_factor
        self.__dict__["_coords"] = {}

    def resize(self, h: int, w: int):
        self.image_height, self.image_width = h, w

    def _pixel_coords(self, B: int, factor: int, device) -> torch.Tensor:
        key = (self.image_height, self.image_width, factor, str(device))
        c = self._coords.get(key)
        if c is None:
            ys, xs = torch.meshgrid(torch.arange(self.image_height, dtype=torch.float32, device=device),
                                    torch.arange(self.image_width, dtype=torch.float32, device=device), indexing="ij")
            c = torch.stack([xs, ys], dim=-1)
            if factor > 1:   # resize_pixel_coords (ray_marcher.py:57-76)
                sw, sh = self.image_width // factor, self.image_height // factor
                x0 = y0 = factor // 2
                c = c[y0:y0 + factor * sh:factor, x0:x0 + factor * sw:factor, :]
            self.__dict__["_coords"] = {key: c.contiguous()}
        return c[None].expand(B, -1, -1, -1).contiguous()

    @ops.on_input_device
    def forward(self, prim_rgba, prim_pos, prim_rot, prim_scale, K, RT, ray_subsample_factor: Optional[int] = None):
        if not prim_rgba.is_cuda:
            raise RuntimeError("RayMarcher.forward needs HIP device tensors; there is no CPU path")
        B = prim_rgba.shape[0]
        cam = convert_camera_parameters(RT.float(), K.float())
        factor = self.ray_subsample_factor if ray_subsample_factor is None else ray_subsample_factor
        if self.training and factor > 1:
            pixel_coords = training_pixel_coords(base_pixel_coords(self.image_height, self.image_width, prim_rgba.device), B, factor)
        else:
            pixel_coords = self._pixel_coords(B, factor, prim_rgba.device)
        focal = torch.diagonal(cam["focal"], dim1=1, dim2=2).contiguous()
        raypos, raydir, tminmax = compute_raydirs(cam["campos"], cam["camrot"], focal, cam["princpt"], pixel_coords,
                                                  self.volradius)
        rgba = mvpraymarch(raypos, raydir, self.dt / self.volradius, tminmax,
                           (prim_pos / self.volradius, prim_rot, prim_scale),
                           prim_rgba.permute(0, 1, 3, 4, 5, 2), self.fadescale, self.fadeexp)
        return {"rgba_image": rgba.permute(0, 3, 1, 2), "pixel_coords": pixel_coords}


def generate_colored_boxes(template: torch.Tensor, prim_rot: torch.Tensor, alpha: float = 10000.0, seed: int = 123456):
    """Debug templates for the bounding-box preview (dva/ray_marcher.py:232-279, used by dva/visualize.py:26): every
    primitive becomes an opaque box of one random colour, shaded by the face its voxel is nearest to.  template:
    [B, K, 4, S, S, S] -> same shape.  Elementwise preparation of a marcher input (plumbing, plain torch); colours follow
    the reference's `np.random.seed(seed)` stream so previews look the same."""
    import numpy as np

    B, K, S = template.shape[0], template.shape[1], template.shape[-1]
    dev = template.device
    lin = torch.linspace(-1.0, 1.0, S, device=dev)
    zz, yy, xx = torch.meshgrid(lin, lin, lin, indexing="ij")
    ax, ay, az = xx.abs(), yy.abs(), zz.abs()
    # outward unit normal of the dominant face(s), in the marcher's (x, -y, -z) convention; ties share the normal
    n = torch.stack([torch.where((ax >= ay) & (ax >= az), xx.sign(), torch.zeros_like(xx)),
                     -torch.where((ay >= ax) & (ay >= az), yy.sign(), torch.zeros_like(xx)),
                     -torch.where((az >= ax) & (az >= ay), zz.sign(), torch.zeros_like(xx))], dim=-1)
    n = n / n.pow(2).sum(-1, keepdim=True).sqrt()
    light = torch.full((3,), -3.0, device=dev)
    light = light / light.norm()
    shade = 1.4 * (n * light).sum(-1).clamp(min=0.2)                                   # [S, S, S]
    colours = torch.as_tensor(np.random.RandomState(seed).rand(K, 3) * 255.0, dtype=template.dtype, device=dev)
    out = template.clone()
    out[:, :, :3] = colours[None, :, :, None, None, None] * shade[None, None, None]
    out[:, :, 3] = alpha
    return out
