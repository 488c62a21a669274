"""PrimSDF field query on MI355X - SURVEY.md section 8(f) row N3 (models/primsdf.py, queried by the mesh / texture
extraction of inference.py:106-116, 180-193).

`PrimSDF` mirrors the reference module's parameters (`srt_param` [P, 1 + 3] = scale + translation, `feat_param`
[P, 6 * S^3]), its properties (`pos`, `scale`, `feat`, `feat_geo`, `feat_tex`, `feat_mat`) and `forward(x) ->
{'sdf', 'tex', 'mat'}` including the inference-time fill of uncovered points; the evaluation itself is one HIP kernel
(`primx_primsdf_query`).  The reference's fitting path (`_init_param`, an empty `pass` in its tree) is not mirrored: the
constructor still refuses `f_sdf` / `geo_fn` / `asset_list`.  `PrimSDF.from_mesh` fits primitives to a triangle mesh instead
(fit.py: the initialisation the paper describes and, with `refine=N`, N steps of its gradient refinement).

Like the reference's module in `.train()`, a `PrimSDF(differentiable=True)` in training mode is differentiable in `srt_param`
and `feat_param`: `primx_primsdf_query_backward` (`query_backward` below) is the backward of the training-mode query.  There is
no gradient with respect to the points under autograd; `PrimSDF.query_grad` / `normals` return the analytic gradient of the sdf
with respect to the points as plain tensors (`primx_primsdf_query_grad`), which the normal-map bake of mesh.py reads.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _lib, ops


def _query_train(x, srt, feat, lin, S: int) -> torch.Tensor:
    """The training-mode query (eval_fill = 0) of detached, contiguous fp32 device tensors -> [n, C]."""
    n, C = x.shape[0], feat.shape[1] // S ** 3
    out = torch.empty(n, C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().primx_primsdf_query(
        ops._dev(x, "x", torch.float32), ops._dev(srt, "srt", torch.float32), ops._dev(feat, "feat", torch.float32),
        ops._dev(lin, "lin", torch.float32), out.data_ptr(), n, srt.shape[0], S, C, 0, ops._stream()), "primx_primsdf_query")
    return out


def query_backward(x, srt, feat, gout, prim_shape: int, gsrt=None, gfeat=None, want_srt: bool = True, want_feat: bool = True):
    """primx_primsdf_query_backward: x [n, 3], srt [P, 4], feat [P, C S^3], gout [n, C] (the gradient with respect to the
    training-mode query's clipped output) -> (gsrt [P, 4] or None, gfeat [P, C S^3] or None), fp32.  The kernel ADDS: given
    `gsrt` / `gfeat` are accumulated into, missing ones start from zero (`want_*` = False skips that gradient).  Atomic adds: the
    last bits depend on the arrival order."""
    S = int(prim_shape)
    x, srt, feat, gout = (t.detach().float().contiguous() for t in (x, srt, feat, gout))
    n, P = x.shape[0], srt.shape[0]
    C = feat.shape[1] // S ** 3
    if tuple(gout.shape) != (n, C) or tuple(srt.shape) != (P, 4) or feat.shape[0] != P or feat.shape[1] != C * S ** 3:
        raise ValueError(f"x [n, 3], srt [P, 4], feat [P, C S^3], gout [n, C] expected, got {tuple(x.shape)}, {tuple(srt.shape)}, "
                         f"{tuple(feat.shape)}, {tuple(gout.shape)}")
    if gsrt is None and want_srt:
        gsrt = torch.zeros_like(srt)
    if gfeat is None and want_feat:
        gfeat = torch.zeros_like(feat)
    if n == 0 or (gsrt is None and gfeat is None):
        return gsrt, gfeat
    _lib.check(_lib.load().primx_primsdf_query_backward(
        ops._dev(x, "x", torch.float32), ops._dev(srt, "srt", torch.float32), ops._dev(feat, "feat", torch.float32),
        ops._dev(gout, "gout", torch.float32), None if gsrt is None else ops._dev(gsrt, "gsrt", torch.float32),
        None if gfeat is None else ops._dev(gfeat, "gfeat", torch.float32), n, P, S, C, ops._stream()),
        "primx_primsdf_query_backward")
    return gsrt, gfeat


class _TrainQuery(torch.autograd.Function):
    """out = the training-mode query; backward = primx_primsdf_query_backward (no gradient for the points)."""

    @staticmethod
    def forward(ctx, x, srt, feat, lin, S):
        srt_c, feat_c = srt.detach().float().contiguous(), feat.detach().float().contiguous()
        ctx.save_for_backward(x, srt_c, feat_c)
        ctx.S = S
        return _query_train(x, srt_c, feat_c, lin, S)

    @staticmethod
    def backward(ctx, gout):
        x, srt, feat = ctx.saved_tensors
        gsrt, gfeat = query_backward(x, srt, feat, gout, ctx.S, want_srt=ctx.needs_input_grad[1],
                                     want_feat=ctx.needs_input_grad[2])
        return None, gsrt, gfeat, None, None


class PrimSDF(nn.Module):
    def __init__(self, mesh_obj=None, f_sdf=None, geo_fn=None, asset_list=None, num_prims=1024, dim_feat=6, prim_shape=8,
                 init_scale=0.05, sdf2alpha_var=0.005, auto_scale_init=True, init_sampling="uniform", differentiable=False):
        super().__init__()
        self.differentiable = bool(differentiable)
        if f_sdf is not None or geo_fn is not None or asset_list is not None:
            raise NotImplementedError("primitive fitting (PrimSDF._init_param) is training-side; load fitted parameters")
        self.num_prims, self.dim_feat, self.prim_shape = num_prims, dim_feat, prim_shape
        self.sdf2alpha_var = sdf2alpha_var
        self.srt_param = nn.Parameter(torch.zeros(num_prims, 1 + 3))
        self.feat_param = nn.Parameter(torch.zeros(num_prims, dim_feat * prim_shape ** 3))
        s3 = prim_shape ** 3
        self.geo_start_index, self.geo_end_index = 0, s3
        self.tex_start_index, self.tex_end_index = s3, 4 * s3
        self.mat_start_index, self.mat_end_index = 4 * s3, 6 * s3
        xx = torch.linspace(-1, 1, prim_shape)
        meshx, meshy, meshz = torch.meshgrid(xx, xx, xx, indexing="ij")
        self.local_grid = torch.stack((meshz, meshy, meshx), dim=-1).reshape(-1, 3)   # (primsdf.py:35-41)
        self.__dict__["_lin"] = {}

    # reference properties (primsdf.py:112-137)
    pos = property(lambda self: self.srt_param[:, 1:4])
    scale = property(lambda self: self.srt_param[:, 0:1])
    feat = property(lambda self: self.feat_param)
    feat_geo = property(lambda self: self.feat_param[:, self.geo_start_index:self.geo_end_index])
    feat_tex = property(lambda self: self.feat_param[:, self.tex_start_index:self.tex_end_index])
    feat_mat = property(lambda self: self.feat_param[:, self.mat_start_index:self.mat_end_index])

    @classmethod
    def from_mesh(cls, mesh, num_prims=2048, prim_shape=8, **kw):
        """A module holding `fit.mesh_to_primitives(mesh, num_prims, prim_shape, **kw)`, in eval mode on the HIP device: ready
        for `query`, `mesh.extract_mesh` and (as `torch.cat([srt_param, feat_param], 1)[None]`) `primitives_to_latents`.
        `refine=N` runs N refinement steps (`fit.refine_primitives`); `return_info=True` also returns the fit's `info`."""
        from . import fit
        return fit.primsdf_from_mesh(cls, mesh, num_prims=num_prims, prim_shape=prim_shape, **kw)

    def sdf2alpha(self, sdf):
        return torch.exp(-(sdf / self.sdf2alpha_var) ** 2)

    def _linspace(self, device) -> torch.Tensor:
        key = (str(device), self.prim_shape)
        if key not in self._lin:
            self._lin[key] = torch.linspace(-1, 1, self.prim_shape).to(device)   # the reference's own table (primsdf.py:35)
        return self._lin[key]

    def _differentiates(self) -> bool:
        return (getattr(self, "differentiable", False) and self.training and torch.is_grad_enabled()
                and (self.srt_param.requires_grad or self.feat_param.requires_grad))

    def query(self, x: torch.Tensor) -> torch.Tensor:
        """x: [n, 3] fp32 on the HIP device -> [n, dim_feat] = [sdf, clipped tex (3), clipped mat (2)].  With
        `differentiable=True`, in `.train()`, under grad mode and with a parameter that requires grad, the result carries a
        `grad_fn` (gradients for `srt_param` / `feat_param`, none for `x`: an `x` that requires grad raises); in every other
        state the parameters are detached as before."""
        if not x.is_cuda:
            raise RuntimeError("PrimSDF.query needs HIP device tensors; there is no CPU path")
        if self.dim_feat != 6 or self.srt_param.shape[0] == 0:
            raise NotImplementedError("the query kernel covers the 6-channel PrimX payload")
        if self._differentiates():
            if x.requires_grad:
                raise RuntimeError("PrimSDF is differentiable in srt_param and feat_param only: no gradient with respect to "
                                   "the query points is built (pass x.detach())")
            x = x.float().contiguous()
            if x.shape[0] == 0:
                return torch.empty(0, self.dim_feat, dtype=torch.float32, device=x.device)
            return _TrainQuery.apply(x, self.srt_param, self.feat_param, self._linspace(x.device), self.prim_shape)
        x = x.float().contiguous()
        n = x.shape[0]
        out = torch.empty(n, self.dim_feat, dtype=torch.float32, device=x.device)
        if n == 0:
            return out
        srt = self.srt_param.detach().float().contiguous()
        feat = self.feat_param.detach().float().contiguous()
        _lib.check(_lib.load().primx_primsdf_query(
            ops._dev(x, "x", torch.float32), ops._dev(srt, "srt", torch.float32), ops._dev(feat, "feat", torch.float32),
            ops._dev(self._linspace(x.device), "lin", torch.float32), out.data_ptr(), n, srt.shape[0], self.prim_shape,
            self.dim_feat, 0 if self.training else 1, ops._stream()), "primx_primsdf_query")
        return out

    def query_grad(self, x: torch.Tensor):
        """x: [n, 3] fp32 on the HIP device -> (out [n, dim_feat], grad [n, 3]): `query`'s columns (the same bits, with the fill
        of uncovered points in eval mode and without it in `.train()`, as `query` chooses) and the analytic gradient of the sdf
        column with respect to the point (`primx_primsdf_query_grad`, rules in include/primx_hip.h).  The parameters are
        detached and nothing here is recorded by autograd."""
        if not x.is_cuda:
            raise RuntimeError("PrimSDF.query_grad needs HIP device tensors; there is no CPU path")
        if self.dim_feat != 6 or self.srt_param.shape[0] == 0:
            raise NotImplementedError("the query kernel covers the 6-channel PrimX payload")
        x = x.detach().float().contiguous()
        n = x.shape[0]
        out = torch.empty(n, self.dim_feat, dtype=torch.float32, device=x.device)
        grad = torch.empty(n, 3, dtype=torch.float32, device=x.device)
        if n == 0:
            return out, grad
        srt = self.srt_param.detach().float().contiguous()
        feat = self.feat_param.detach().float().contiguous()
        _lib.check(_lib.load().primx_primsdf_query_grad(
            ops._dev(x, "x", torch.float32), ops._dev(srt, "srt", torch.float32), ops._dev(feat, "feat", torch.float32),
            ops._dev(self._linspace(x.device), "lin", torch.float32), out.data_ptr(), grad.data_ptr(), n, srt.shape[0],
            self.prim_shape, self.dim_feat, 0 if self.training else 1, ops._stream()), "primx_primsdf_query_grad")
        return out, grad

    def normals(self, x: torch.Tensor) -> torch.Tensor:
        """x: [n, 3] -> [n, 3] unit field normals grad / |grad| of `query_grad`, (0, 0, 0) where the gradient is zero.  They point
        towards higher sdf values, outward, like the lattice normals of `mesh.marching_cubes(return_normals=True)`."""
        grad = self.query_grad(x)[1]
        length = grad.norm(dim=1, keepdim=True)
        return torch.where(length > 0, grad / length.clamp_min(1e-38), torch.zeros_like(grad))

    @ops.on_input_device
    def forward(self, x: torch.Tensor):
        out = self.query(x)
        return {"sdf": out[:, 0:1], "tex": out[:, 1:4], "mat": out[:, 4:6]}
