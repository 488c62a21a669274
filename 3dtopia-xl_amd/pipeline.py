"""Post-sampling driver of the hot path: denoised latents -> per-primitive PBR voxel payload, and back (`primitives_to_latents`,
`redenoise_primitives`: edit a stored asset and re-denoise it).

Mirrors what the reference's CLI / app do between the sampler and the ray-marcher / mesh export
(inference.py:326-348, app.py:117-139):  de-normalise with the per-channel latent statistics, split
(scale + xyz | 4^3 VAE latent), decode every sample's primitives, apply the decoder's inverse normalisation
(SDF / 5, colour+material (v + 1) / 2) and concatenate to ``[B, N_prim, 4 + 6 * 8^3]`` - the ``recon_param``
tensor the renderer and ``PrimSDF`` consume (``srt_param`` = [:, :, :4], ``feat_param`` = [:, :, 4:]).

MI355X-first differences: the reference decodes one sample at a time "to avoid oom" (inference.py:334-340) and
runs four full-tensor elementwise passes afterwards; here all B * N_prim primitives go through ONE decoder call
(288 GB of HBM: 8 samples x 2048 primitives peak at ~9 GB of 16-bit activations), the inverse normalisation is
fused into the decoder's output kernel and the latent de-normalisation + split is one kernel.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .fit import mesh_field, mesh_to_primitives, refine_primitives  # noqa: F401  (fitting a user's mesh: fit.py)
from .mesh import read_glb, read_ply                     # noqa: F401


_STATS_CACHE: dict = {}


def _latent_stats(latent_mean, latent_std, dev):
    """fp32 device tensors of the per-channel statistics.  The reference re-uploads them with every call
    (inference.py:328-332); here a Python list / tuple is uploaded once per device (two pageable host-to-device copies and
    their synchronisation per decode otherwise), tensors are used as they are."""
    def one(v):
        if isinstance(v, torch.Tensor):
            return v.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        key = (tuple(float(a) for a in v), str(dev))
        t = _STATS_CACHE.get(key)
        if t is None:
            if len(_STATS_CACHE) > 16:
                _STATS_CACHE.clear()
            t = _STATS_CACHE[key] = torch.tensor(key[0], dtype=torch.float32, device=dev)
        return t
    return one(latent_mean), one(latent_std)


@ops.on_input_device
def latents_to_primitives(samples: torch.Tensor, vae, latent_mean: Optional[Sequence[float]] = None,
                          latent_std: Optional[Sequence[float]] = None, latent_nf: float = 1.0,
                          max_prims_per_call: int = 8 * 2048) -> torch.Tensor:
    """samples: (B, N_prim, 68) fp32 sampler output -> recon_param (B, N_prim, 4 + C_out * (2S)^3) fp32."""
    if not samples.is_cuda:
        raise RuntimeError("latents_to_primitives needs HIP device tensors; there is no CPU path")
    B, N, C = samples.shape
    dev = samples.device
    if latent_mean is None:
        # the reference's non-per-channel branch (inference.py:336-344) is dead for the shipped config (yml:64-65)
        raise NotImplementedError("per-channel latent_mean / latent_std are required (configs/inference_dit.yml:64-65)")
    mean, std = _latent_stats(latent_mean, latent_std, dev)      # device copies are made once per (values, device)
    if mean.numel() != C or std.numel() != C:
        raise AssertionError("latent_mean / latent_std must have one entry per latent channel")
    srt, z = ops.latent_denorm(samples.float().contiguous(), mean, std, latent_nf, 4)
    S = round((C - 4) ** (1.0 / 3.0))
    if S ** 3 != C - 4:
        raise AssertionError("latent channels minus 4 must be a cube")
    z = z.reshape(B * N, 1, S, S, S)
    outs = []
    for lo in range(0, B * N, max_prims_per_call):
        outs.append(vae.decode(z[lo:lo + max_prims_per_call].contiguous(), denormalize=True))
    dec = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
    feat = dec.reshape(B, N, -1)
    return torch.cat([srt, feat], dim=-1)


@ops.on_input_device
def primitives_to_latents(recon_param: torch.Tensor, vae, latent_mean: Optional[Sequence[float]] = None,
                          latent_std: Optional[Sequence[float]] = None, latent_nf: float = 1.0, sample: bool = False,
                          generator=None, max_prims_per_call: int = 8 * 2048) -> torch.Tensor:
    """recon_param (B, N_prim, 4 + 6 * 8^3) fp32 -> (B, N_prim, 68) fp32 tokens in the DiT's normalised space: the inverse of
    latents_to_primitives.  The payload goes through ``vae.encode(normalize=True)`` in chunks of max_prims_per_call
    primitives; the posterior's mode (``sample=True``: a sample, its noise drawn once with ``generator`` for all B * N primitives,
    so it does not depend on the chunking) and the srt columns are normalised
    with the per-channel statistics and joined by one kernel (primx_latent_norm)."""
    if not recon_param.is_cuda:
        raise RuntimeError("primitives_to_latents needs HIP device tensors; there is no CPU path")
    B, N, C = recon_param.shape
    if latent_mean is None:
        raise NotImplementedError("per-channel latent_mean / latent_std are required (configs/inference_dit.yml:64-65)")
    S2 = round(((C - 4) / 6) ** (1.0 / 3.0))
    if 6 * S2 ** 3 != C - 4:
        raise AssertionError("recon_param must have 4 + 6 * (2S)^3 channels")
    mean, std = _latent_stats(latent_mean, latent_std, recon_param.device)
    rp = recon_param.float().reshape(B * N, C)
    zs, noise = [], None
    for lo in range(0, B * N, max_prims_per_call):
        post = vae.encode(rp[lo:lo + max_prims_per_call, 4:].reshape(-1, 6, S2, S2, S2), normalize=True)
        z = post.mode()
        if sample:
            if noise is None:      # one draw for all B * N primitives: a sample does not depend on max_prims_per_call
                noise = torch.randn((B * N,) + tuple(z.shape[1:]), device=z.device, dtype=z.dtype, generator=generator)
            z = post.mean + post.std * noise[lo:lo + z.shape[0]]
        zs.append(z.reshape(z.shape[0], -1))
    z = (zs[0] if len(zs) == 1 else torch.cat(zs, dim=0)).contiguous()
    if mean.numel() != 4 + z.shape[1] or std.numel() != mean.numel():
        raise AssertionError("latent_mean / latent_std must have one entry per latent channel")
    return ops.latent_norm(rp[:, :4].contiguous(), z, mean, std, latent_nf).view(B, N, -1)


# ---------------------------------------------------------------------------------------------------------------------
# Editing a stored asset: encode -> noise or invert to a level -> re-denoise from there, with part
# of the tokens optionally held -> decode.  DESIGN.md "Editing" has the level convention and the kept-token contract.
def keep_mask(n_prim_mask: torch.Tensor, channels: str = "all", n_channels: int = 68) -> torch.Tensor:
    """A per-primitive bool mask (B, N) -> the (B, N, n_channels) element mask `redenoise_primitives(keep=...)` and
    `ddim_sample_loop(keep=...)` take: of the flagged primitives keep every channel ("all"), only scale + xyz ("srt",
    channels 0..3: keep the layout, regenerate the appearance) or only the appearance latents ("latent", channels 4..)."""
    if n_prim_mask.dtype != torch.bool or n_prim_mask.dim() != 2:
        raise ValueError("n_prim_mask must be a bool tensor of shape (B, N_prim)")
    if channels not in ("all", "srt", "latent"):
        raise ValueError(f'channels must be "all", "srt" or "latent", got {channels!r}')
    ch = torch.zeros(n_channels, dtype=torch.bool, device=n_prim_mask.device)
    ch[{"all": slice(None), "srt": slice(0, 4), "latent": slice(4, None)}[channels]] = True
    return n_prim_mask[:, :, None] & ch


def redenoise_primitives(recon_param: torch.Tensor, vae, model, diffusion, y: torch.Tensor, *, start_step: int,
                         mode: str = "noise", keep: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                         generator=None, cfg_scale: float = 6.0, invert_cfg_scale: float = 1.0,
                         precision_dtype: torch.dtype = torch.float16, enable_amp: bool = True,
                         latent_mean: Optional[Sequence[float]] = None, latent_std: Optional[Sequence[float]] = None,
                         latent_nf: float = 1.0, sampler: str = "ddim") -> torch.Tensor:
    """recon_param (B, N_prim, 4 + 6 * 8^3) -> recon_param of the edited asset: `primitives_to_latents`, then the tokens are
    taken to level `start_step` of `diffusion` - mode "noise": `q_sample` with `noise` (drawn once with `generator` when None);
    mode "invert": `ddim_reverse_sample_loop(stop_step=start_step)` under `model.forward_with_cfg` at `invert_cfg_scale` - and
    `ddim_sample_loop(start_step=start_step)` re-denoises them under the conditioning `y` at `cfg_scale`; `latents_to_primitives`
    decodes.  `keep` (bool; (B, N_prim) keeps whole primitives, (B, N_prim, 68) elements, see `keep_mask`) holds those tokens
    on the input asset's own trajectory: they come out as the encode -> decode round trip of the input, bit for bit.  `keep`
    needs mode "noise": the kept rows of an inversion would need the inversion's own implied noise.  `sampler` "dpm" re-denoises
    with `dpm_solver_sample_loop` (DPM-Solver++(2M), for processes of 10 to 15 steps) in place of `ddim_sample_loop`: the same
    `start_step` and `keep`, nothing drawn differently, the same contract for the kept tokens."""
    if mode not in ("noise", "invert"):
        raise ValueError(f'mode must be "noise" or "invert", got {mode!r}')
    if sampler not in ("ddim", "dpm"):
        raise ValueError(f'sampler must be "ddim" or "dpm", got {sampler!r}')
    if keep is not None and mode == "invert":
        raise ValueError('keep needs mode="noise": an inverted trajectory has no noise tensor to hold the kept tokens on')
    if not (0 <= int(start_step) < diffusion.num_timesteps):
        raise ValueError(f"start_step must lie in 0 .. {diffusion.num_timesteps - 1}, got {start_step}")
    start_step = int(start_step)
    tokens = primitives_to_latents(recon_param, vae, latent_mean, latent_std, latent_nf)
    with ops.device_of(tokens):
        kw = dict(y=y, cfg_scale=cfg_scale, precision_dtype=precision_dtype, enable_amp=enable_amp)
        if mode == "noise":
            if noise is None:
                noise = torch.randn(tokens.shape, device=tokens.device, dtype=torch.float32, generator=generator)
            t = torch.full((tokens.shape[0],), start_step, dtype=torch.int64, device=tokens.device)
            level = diffusion.q_sample(tokens, t, noise)
        elif start_step == 0:
            level = tokens                      # level 0 is what the inversion starts from
        else:
            level = diffusion.ddim_reverse_sample_loop(model.forward_with_cfg, tokens, clip_denoised=False,
                                                       model_kwargs=dict(kw, cfg_scale=invert_cfg_scale), stop_step=start_step)
        held = {} if keep is None else dict(known=tokens, keep=keep, known_noise=noise)
        loop = diffusion.ddim_sample_loop if sampler == "ddim" else diffusion.dpm_solver_sample_loop
        samples = loop(model.forward_with_cfg, tuple(tokens.shape), noise=level, clip_denoised=False, model_kwargs=kw,
                       start_step=start_step, **held)
    return latents_to_primitives(samples, vae, latent_mean, latent_std, latent_nf)


# ---------------------------------------------------------------------------------------------------------------------
# On-disk formats of the hot path: the two checkpoints the CLI loads and the `denoised.pt`
# it writes between sampling and mesh extraction.
def load_checkpoints(model=None, vae=None, dit_checkpoint_path: Optional[str] = None,
                     vae_checkpoint_path: Optional[str] = None, packed_dtype: Optional[torch.dtype] = None) -> None:
    """`model.load_state_dict(torch.load(p)['ema'])` / `vae.load_state_dict(torch.load(p)['model_state_dict'])`, strict,
    as inference.py:257-262 does (fp16 `.pt` files load into the fp32 parameters; the packed 16-bit copies the kernels
    read are rebuilt lazily on the first forward).

    `packed_dtype` (torch.float16 / torch.bfloat16) takes the direct route for the DiT instead: the checkpoint is memory-
    mapped and its tensors are copied straight into the packed 16-bit blob on the model's device (`DiT.pack_from_state_dict`)
    - no 3.6 GB of fp32 parameters, no repack on the first forward; the model is then packed-only (its fp32 route raises).
    A path ending in `.primxpk` is a `DiT.save_packed` file and is mapped as is (`DiT.load_packed`)."""
    if model is not None and dit_checkpoint_path:
        if dit_checkpoint_path.endswith(".primxpk"):
            model.load_packed(dit_checkpoint_path)
        elif packed_dtype is not None:
            model.pack_from_state_dict(torch.load(dit_checkpoint_path, map_location="cpu", mmap=True)["ema"], packed_dtype)
        else:
            model.load_state_dict(torch.load(dit_checkpoint_path, map_location="cpu")["ema"], strict=True)
    if vae is not None and vae_checkpoint_path:
        vae.load_state_dict(torch.load(vae_checkpoint_path, map_location="cpu")["model_state_dict"], strict=True)


def save_denoised(path: str, recon_param: torch.Tensor, index: int = 0) -> None:
    """`{'model_state_dict': {'srt_param': [N, 4], 'feat_param': [N, 6 * 8^3]}}` of sample `index` (inference.py:351-352):
    the file PrimSDF (mesh extraction) and the viewer load."""
    p = recon_param[index].detach().cpu()
    torch.save({"model_state_dict": {"srt_param": p[:, :4].contiguous(), "feat_param": p[:, 4:].contiguous()}}, path)


def primsdf_from_denoised(path: str, device=None):
    """A `PrimSDF` holding the primitives of a `denoised.pt` (what the GLB export builds before querying the field)."""
    from .primsdf import PrimSDF
    sd = torch.load(path, map_location="cpu")["model_state_dict"]
    n, s3 = sd["srt_param"].shape[0], sd["feat_param"].shape[1] // 6
    m = PrimSDF(num_prims=n, dim_feat=6, prim_shape=round(s3 ** (1.0 / 3.0)))
    m.load_state_dict(sd, strict=True)
    return m.to(device).eval() if device is not None else m.eval()


def primitives_to_mesh(recon_param_b: torch.Tensor, resolution: int = 256, **kw):
    """recon_param[b] [N, 4 + 6 S^3] (srt = [:, :4], feat = [:, 4:]) -> `mesh.TriMesh`: a `PrimSDF` of the sample's
    primitives (eval mode, on recon_param's device) through `mesh.extract_mesh(field, resolution, **kw)` - the GLB
    export of inference.py:86-125 without the UV / texture bake; `clean=True` adds the reference's `clean_mesh` step and
    `decimate=N` its `decimate_mesh` step (to at most N faces)."""
    from .mesh import extract_mesh
    from .primsdf import PrimSDF
    if recon_param_b.dim() != 2:
        raise ValueError(f"recon_param_b must be one sample [N, 4 + 6 S^3], got {tuple(recon_param_b.shape)}")
    n, c = recon_param_b.shape
    S = round(((c - 4) / 6) ** (1.0 / 3.0))
    if 6 * S ** 3 != c - 4:
        raise ValueError(f"recon_param_b has {c} channels, not 4 + 6 S^3")
    m = PrimSDF(num_prims=n, dim_feat=6, prim_shape=S)
    m.srt_param = torch.nn.Parameter(recon_param_b[:, :4].detach().float().contiguous(), requires_grad=False)
    m.feat_param = torch.nn.Parameter(recon_param_b[:, 4:].detach().float().contiguous(), requires_grad=False)
    return extract_mesh(m.eval(), resolution, **kw)


def primitives_vs_mesh(recon_param_b: torch.Tensor, mesh, resolution: int = 256, **kw) -> dict:
    """recon_param[b] [N, 4 + 6 S^3] and a mesh in the primitives' coordinates (`info['v']`, `info['f']` of `mesh_to_primitives`)
    -> `metrics.compare_meshes(mesh, primitives_to_mesh(recon_param_b, resolution), **kw)`: Chamfer distance, F-score, Hausdorff
    distance and normal consistency of the round trip mesh -> primitives -> mesh (metrics.py states the definitions)."""
    from .metrics import compare_meshes
    return compare_meshes(mesh, primitives_to_mesh(recon_param_b, resolution), **kw)


def primitives_to_texmesh(recon_param_b: torch.Tensor, resolution: int = 256, texture_size: int = 1024, **kw):
    """recon_param[b] [N, 4 + 6 S^3] -> `mesh.TexturedMesh`: the sample's primitives (as `primitives_to_mesh` builds them)
    through `mesh.extract_texmesh(field, resolution, texture_size, **kw)` - the UV-mapped PBR GLB of inference.py:86-225
    `clean=True` adds the reference's `clean_mesh` step and `decimate=N` its `decimate_mesh` step (`mesh.DECIMATE_TARGET`
    = 100000 in its configuration) before the bake; `normal_map=True` also bakes the field's normals into a tangent-space
    normal map (TANGENT + normalTexture in the GLB); `occlusion=True` bakes ambient occlusion from the SDF lattice into R of
    the metallic-roughness image (occlusionTexture in the GLB)."""
    from .mesh import extract_texmesh
    from .primsdf import PrimSDF
    if recon_param_b.dim() != 2:
        raise ValueError(f"recon_param_b must be one sample [N, 4 + 6 S^3], got {tuple(recon_param_b.shape)}")
    n, c = recon_param_b.shape
    S = round(((c - 4) / 6) ** (1.0 / 3.0))
    if 6 * S ** 3 != c - 4:
        raise ValueError(f"recon_param_b has {c} channels, not 4 + 6 S^3")
    m = PrimSDF(num_prims=n, dim_feat=6, prim_shape=S)
    m.srt_param = torch.nn.Parameter(recon_param_b[:, :4].detach().float().contiguous(), requires_grad=False)
    m.feat_param = torch.nn.Parameter(recon_param_b[:, 4:].detach().float().contiguous(), requires_grad=False)
    return extract_texmesh(m.eval(), resolution, texture_size, **kw)


def primitives_to_marcher_inputs(recon_param: torch.Tensor, volradius: float, sdf2alpha_var: float = 0.005):
    """recon_param [B, N, 4 + 6 S^3] -> (prim_rgba [B,N,4,S,S,S] in 0..255, prim_pos, prim_rot, prim_scale) exactly as the
    preview renderer prepares them (dva/visualize.py:215-239): alpha = 255 exp(-(sdf / 0.005)^2), rgb = 255 tex, identity
    rotations, inverse scales.  Elementwise tensor preparation around the marcher (plumbing)."""
    B, N, C = recon_param.shape
    S = round(((C - 4) / 6) ** (1.0 / 3.0))
    s3 = S ** 3
    geo = recon_param[:, :, 4:4 + s3]
    tex = recon_param[:, :, 4 + s3:4 + 4 * s3]
    alpha = torch.exp(-(geo / sdf2alpha_var) ** 2).reshape(B, N, 1, S, S, S) * 255
    rgb = tex.reshape(B, N, 3, S, S, S) * 255
    pos = recon_param[:, :, 1:4].reshape(B, N, 3) * volradius
    rot = torch.eye(3, device=recon_param.device, dtype=recon_param.dtype)[None, None].repeat(B, N, 1, 1)
    scale = 1.0 / recon_param[:, :, 0:1].reshape(B, N, 1).repeat(1, 1, 3)
    return torch.cat([rgb, alpha], dim=2), pos, rot, scale


def preview_camera(volradius: float, height: int, width: int, device):
    """The fixed preview camera of dva/visualize.py:240-285 (looking down -z from 5 volume radii, 1024-pixel intrinsics
    rescaled to the image size)."""
    Rt = torch.tensor([[[1.0, 0.0, 0.0, 0.0], [0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 5.0 * volradius]]], device=device)
    K = torch.tensor([[[2084.9526697685183, 0.0, 512.0], [0.0, 2084.9526697685183, 512.0], [0.0, 0.0, 1.0]]], device=device)
    K[:, 0:1, :] *= height / 1024.0
    K[:, 1:2, :] *= width / 1024.0
    return K, Rt
