"""ctypes binding of ``libprimx_hip.so`` (the C ABI declared in ``include/primx_hip.h``).

There is exactly one compute backend.  If the library has not been built (``__graft_entry__.build()``
or ``python 3dtopia-xl_amd/csrc/build.py``) every op raises - nothing falls back to PyTorch or the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRIMX_LIB") or os.path.join(_HERE, "csrc", "libprimx_hip.so")  # PRIMX_LIB: A/B builds

F32, F16, BF16 = 0, 1, 2
ACT_NONE, ACT_GELU_TANH, ACT_GELU_ERF = 0, 1, 2
HEADS_ROWS, HEADS_VT, HEADS_KROWS = 0, 1, 2
ABI_VERSION = 35

_p, _i, _l, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double



class DitBlockFold(C.Structure):
    """PrimxDitBlockFold (include/primx_hip.h): weights, cross-attention operands, fold tables and prefetch ranges of one DiT block."""
    _fields_ = [(n, _p) for n in ("w_q", "b_q", "w_cproj", "b_cproj", "w_qkv", "w_proj", "b_proj", "w_fc1", "w_fc2", "b_fc2",
                                  "Kc", "Vc", "Kb", "Vb", "uv_q", "uv_qkv", "uv_fc1",
                                  "carry_q", "carry_cproj", "carry_fc1", "carry_fc2")] + \
               [(n, _l) for n in ("carry_q_bytes", "carry_cproj_bytes", "carry_fc1_bytes", "carry_fc2_bytes")]


class F32outProblem(C.Structure):
    """PrimxF32outProblem (include/primx_hip.h, ABI 26): one problem of primx_linear_f32out_group; the array lives in DEVICE memory (40 bytes each)."""
    _fields_ = [("A", _p), ("W", _p), ("bias", _p), ("out", _p), ("N", _i), ("first_wg", _i)]


class DitForwardFold(C.Structure):
    """PrimxDitForwardFold (include/primx_hip.h): one forward's shapes, workspaces and tables."""
    _fields_ = [(n, _i) for n in ("dtype", "Be", "N", "D", "H", "dh", "hidden", "depth", "L", "nq_pad", "nkv_pad_c", "nkv_pad_b",
                                  "b_from", "step", "n_steps")] + \
               [("ln_eps", _f), ("scale", _f)] + \
               [(n, _p) for n in ("h", "xn", "att", "hid", "Qc", "Qs", "Ks", "Vs", "mod", "center0", "center1", "part")] + \
               [(n, _p) for n in ("kv_A", "kv_W", "kv_bias")] + [(n, _i) for n in ("kv_rows", "kv_rows_per_batch", "kv_K")] + \
               [("null_vrow", _p)] + [(n, _i) for n in ("only_block", "only_launch", "side")]   # ABI 25; the null cross-attention skip's tail


# name -> argument ctypes (return type is always int unless listed in _RESTYPES)
SIGNATURES = {
    "primx_dit_blocks_fold": [C.POINTER(DitForwardFold), C.POINTER(DitBlockFold), _p],
    "primx_abi_version": [],
    "primx_dit_blocks_fold_features": [],
    "primx_last_error": [],
    "primx_last_gemm_kernel": [],
    "primx_padded_head_dim": [_i],
    "primx_layernorm_modulate": [_p, _p, _p, _l, _p, _i, _i, _i, _i, _f, _p, _l, _p, _l, _p],
    "primx_timestep_embedding": [_p, _p, _p, _i, _i, _p],
    "primx_compute_raydirs": [_p, _p, _p, _p, _p, _f, _p, _p, _p, _i, _i, _i, _p],
    "primx_raymarch": [_p, _p, _p, _f, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _p],
    "primx_primsdf_query": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    "primx_vit_tokens": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p],
    "primx_point_features": [_p, _l, _p, _p, _l, _i, _i, _p],
    "primx_prefetch": [_p, _l, _p],
    "primx_silu_cast": [_p, _p, _i, _l, _p],
    "primx_cast16": [_p, _p, _i, _l, _p],
    "primx_linear_f32": [_p, _p, _p, _p, _p, _i, _i, _i, _i, _p],
    "primx_linear": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _f, _p, _l, _p],
    "primx_linear_gate_residual": [_p, _p, _p, _p, _l, _p, _i, _i, _i, _i, _i, _p, _l, _p],
    "primx_linear_gate_residual_ln": [_p, _p, _p, _p, _l, _p, _i, _i, _i, _i, _p, _p, _l, _p, _f, _p, _l, _i, _p, _l, _p],
    "primx_ln_sync_timeouts": [],
    "primx_linear_f32out": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    "primx_row_stats": [_p, _i, _i, _f, _p, _p],
    "primx_linear_gate_residual_fold": [_p, _p, _p, _p, _l, _p, _i, _i, _i, _i, _p, _l, _p, _p, _p, _i, _p, _l, _p],
    "primx_linear_heads_fold": [_p, _p, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_p), _i, _f, _p, _p, _p, _p, _p, _f,
                                _i, _p, _l, _p],
    "primx_linear_heads_fold_pair": [_p, _p, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_p), _i, _f, _p, _p, _p, _p, _p, _f,
                                     _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_p), _i, _f, _i, _p],
    "primx_linear_f32out_group": [_p, _i, _i, _i, _i, _i, _i, _p],
    "primx_linear_fold": [_p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p, _p, _f, _i, _p, _l, _p],
    "primx_linear_heads": [_p, _p, _p, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i), C.POINTER(_p), _i, _i, _i, _f, _i, _p, _l, _p],
    "primx_attention": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _i, _p],
    "primx_attention_bcast": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _p, _p, _i, _i, _i, _p],
    "primx_attention_ksplit_mode": [_i],
    "primx_attention_ksplit": [_i, _i, _i, _i],
    "primx_gemm_toq64_mode": [_i],
    "primx_pack_heads": [_p, _l, _l, _l, _p, _i, _i, _i, _i, _i, _i, _i, _p],
    "primx_cfg_combine": [_p, _p, _i, _l, _f, _p],
    "primx_diffusion_step": [_p, _p, _i, _l, _i, _i, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p],
    "primx_q_sample": [_p, _p, _l, _p, _i, _p, _p],
    "primx_diffusion_reverse_step": [_p, _p, _i, _l, _i, _i, _p, _i, _i, _i, _p, _p, _p],
    "primx_diffusion_step_keep": [_p, _p, _i, _l, _i, _i, _p, _i, _i, _i, _i, _i, _p, _p, _p, _p, _i, _p, _p, _p],
    "primx_groupnorm_silu": [_p, _p, _p, _p, _i, _i, _i, _i, _f, _i, _i, _p],
    "primx_conv3d_k3": [_p, _p, _p, _p, _f, _p, _i, _i, _i, _i, _i, _i, _p],
    "primx_conv3d_s4_pack": [_p, _p, _i, _i, _p],
    "primx_conv3d_s4_packed": [_p, _p, _p, _p, _f, _p, _i, _i, _i, _p],
    "primx_conv3d_s8_pack": [_p, _p, _p, _i, _p],
    "primx_conv3d_s8_fused": [_p, _p, _p, _p, _p, _p, _p, _f, _p, _p, _p, _i, _i, _p],
    "primx_conv3d_s8_packed": [_p, _p, _p, _p, _f, _p, _i, _i, _p],
    "primx_convtranspose_s4_pack": [_p, _p, _i, _p],
    "primx_convtranspose_s4_packed": [_p, _p, _p, _p, _p, _i, _i, _p],
    "primx_conv3d_s8c32_pack": [_p, _p, _i, _i, _i, _p],
    "primx_conv3d_s8c32_packed": [_p, _p, _p, _p, _p, _f, _p, _f, _p, _i, _i, _i, _p],
    "primx_linear_residual": [_p, _p, _p, _p, _f, _p, _i, _i, _i, _i, _p],
    "primx_conv_in": [_p, _f, _f, _p, _p, _p, _i, _i, _i, _i, _p],
    "primx_convtranspose_k2s2": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    "primx_vae_output": [_p, _p, _i, _i, _i, _i, _f, _i, _p],
    "primx_latent_denorm": [_p, _p, _p, _f, _p, _p, _l, _i, _i, _p],
    "primx_latent_norm": [_p, _p, _p, _p, _f, _p, _l, _i, _i, _p],
    "primx_enc_conv_in": [_p, _p, _i, _p, _p, _i, _i, _i, _p],
    "primx_conv3d_down_s8c32": [_p, _p, _p, _p, _i, _i, _p],
    "primx_enc_head": [_p, _p, _i, _p, _p, _p, _p, _i, _i, _p],
    "primx_gemm_f32": [_p, _p, _p, _p, _i, _i, _i, _i, _f, _p, _l, _i, _p],
    "primx_attention_f32": [_p, _p, _p, _p, _i, _i, _i, _i, _i, C.POINTER(_l), C.POINTER(_l), C.POINTER(_l), _f, _p],
    "primx_layernorm_modulate_f32": [_p, _p, _p, _l, _p, _i, _i, _i, _f, _p],
    "primx_silu_f32": [_p, _p, _l, _p],
    "primx_mcubes_workspace": [_i, _i, _i, C.POINTER(_l)],
    "primx_mcubes_count": [_p, _i, _i, _i, _f, _p, _l, _p, _p],
    "primx_mcubes_emit": [_p, _i, _i, _i, _f, _p, _l, _l, _l, _p, _p, _p, _p],
    "primx_noise_filter": [_p, _i, _p, _p],
    "primx_texbake_labels": [_p, _p, _p, _i, _i, _p, _p],
    "primx_texbake_components_workspace": [_i, _i, C.POINTER(_l)],
    "primx_texbake_components": [_p, _i, _i, _p, _l, _p, C.POINTER(_l), _p],
    "primx_texbake_raster_workspace": [_i, _i, C.POINTER(_l)],
    "primx_texbake_raster": [_p, _p, _i, _i, _i, _i, _p, _p, _p, _l, _p, _p],
    "primx_texbake_compact": [_p, _i, _i, _p, _l, _p, _p, _i, _p, _p, _i, _i, _l, _p, _p, _p],
    "primx_texbake_fill_workspace": [_i, _i, C.POINTER(_l)],
    "primx_texbake_fill": [_p, _p, _l, _p, _i, _i, _i, _i, _p, _l, _p, _p, _p],
    "primx_meshclean_workspace": [_i, _i, C.POINTER(_l)],
    "primx_meshclean_merge": [_p, _p, _i, _i, _d, _p, _l, _p, C.POINTER(_l), C.POINTER(_f), _p],
    "primx_meshclean_faces": [_p, _p, _p, _i, _i, _p, _l, _p, C.POINTER(_l), _p],
    "primx_meshclean_components": [_p, _p, _p, _p, _i, _i, _i, _i, _i, _d, _i, _p, _l, _p, _p, _p, C.POINTER(_l), _p],
    "primx_meshclean_edges": [_p, _p, _i, _i, _p, _l, _p, _l, _p, C.POINTER(_l), _p],
    "primx_meshclean_fans": [_p, _p, _i, _i, _i, _p, _l, _p, _p, C.POINTER(_l), _p],
    "primx_meshdecim_workspace": [_i, _i, C.POINTER(_l)],
    "primx_meshdecim_edges": [_p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p],
    "primx_meshdecim_quadrics": [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p],
    "primx_meshdecim_costs": [_p, _p, _p, _p, _p, _i, _i, _i, _p, _p, _p, _p, _p],
    "primx_meshdecim_select": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p, _p, _p, _p],
    "primx_meshdecim_collapse": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p, _l, _p, C.POINTER(_l), _p],
    "primx_meshdecim_finish": [_p, _p, _i, _i, _p, _l, _p, _p, _p, C.POINTER(_l), _p],
    "primx_meshdecim_normals": [_p, _p, _p, _p, _i, _i, _p, _l, _p, _p],
    "primx_mesh_field_query": [_p, _l, _p, _p, _i, _i, _p, _i, _p, _l, _p, _p, _p, _p, _p],
    "primx_mesh_face_areas": [_p, _p, _i, _i, _p, _p, _p],
    "primx_mesh_surface_points": [_p, _p, _i, _i, _p, _p, _l, _p, _p, _p, _p],
    "primx_fps": [_p, _i, _i, _i, _p, _l, _p, _p, _p],
    "primx_primsdf_query_backward": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _p],
    "primx_adam_step": [_p, _p, _p, _p, _l, _f, _d, _d, _f, _f, _f, _i, _p],
    "primx_raymarch_backward": [_p, _p, _p, _f, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _f, _p],
    "primx_material_sample": [_p, _p, _p, _l, _p, _i, _p, _p, _i, _p, _i, _p, _l, _p, _p, _p],
    "primx_primsdf_query_grad": [_p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p],
    "primx_texbake_tangents": [_p, _p, _p, _i, _i, _p, _p],
    "primx_texbake_normal_texels": [_p, _l, _p, _i, _i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p],
    "primx_texbake_occlusion": [_p, _i, _p, _p, _l, _p, _i, _i, _f, _f, _f, _p, _p],
    "primx_nearest_points": [_p, _l, _p, _i, _p, _p, _p],
    "primx_distance_stats": [_p, _p, _p, _p, _l, C.POINTER(_f), _i, _p, _l, _p, _p],     # tau: T floats in host memory
    "primx_mesh_bvh_workspace": [_i, C.POINTER(_l)],
    "primx_mesh_bvh_build": [_p, _p, _i, _i, _p, _p, _p, _l, _p],
    "primx_mesh_bvh_query": [_p, _l, _p, _i, _p, _i, _p, _l, _f, _p, _p, _p, _p, _p],
    "primx_mesh_bvh_raycast": [_p, _p, _l, _f, _f, _i, _p, _i, _p, _l, _p, _p, _p, _p],
    "primx_mesh_bvh_visibility": [_p, _l, _p, _i, _f, _i, _p, _i, _p, _l, _p, _p],
}
_RESTYPES = {"primx_last_error": C.c_char_p, "primx_last_gemm_kernel": C.c_char_p}
# An alternate build named by PRIMX_LIB (same-box A/B against another build) must speak the same ABI.  Version 21 changed the argument
# lists of the GEMM / LayerNorm entry points (explicit prefetch ranges), so older libraries cannot be bound any more; every later
# version only ADDED entry points (23 also re-typed the fold's: an older build's are not bound), so an older build serves everything
# but what it lacks.  _SINCE: entry point -> the first ABI version that has it (not listed: 21).  _PROBE marks those that joined
# version 35 without a new number, because they change no existing call: an A/B build of version 35 from before them lacks the
# symbol, which `load` finds out with hasattr.  A version-24 build ignores the kv_* tail of PrimxDitForwardFold that came with
# primx_linear_heads_fold_pair (the host then projects K / V itself).  The normal map's three entry points joined version 35 the same
# way but are listed with the number 35: under PRIMX_LIB an absent entry point of 35 is skipped like a probed one.  So did the ambient
# occlusion's primx_texbake_occlusion, the two entry points of the quality metrics (metrics.py), the three of the mesh BVH (fit.MeshBVH)
# and the two of its ray queries (MeshBVH.raycast, MeshBVH.visibility).
_PROBE = 0
_SINCE: dict = {
    **dict.fromkeys(("primx_linear_f32out", "primx_row_stats", "primx_linear_gate_residual_fold", "primx_linear_heads_fold",
                     "primx_linear_fold"), 23),                                                  # the LayerNorm fold
    "primx_dit_blocks_fold": 24,                                                                 # one foreign call for a forward's blocks
    "primx_linear_heads_fold_pair": 25,                                                          # the K / V riders
    "primx_linear_f32out_group": 26,                                                             # the fold's u / v rows in one launch
    **dict.fromkeys(("primx_mcubes_workspace", "primx_mcubes_count", "primx_mcubes_emit", "primx_noise_filter"), 27),   # mesh.py
    **dict.fromkeys(("primx_texbake_labels", "primx_texbake_components_workspace", "primx_texbake_components",
                     "primx_texbake_raster_workspace", "primx_texbake_raster", "primx_texbake_compact",
                     "primx_texbake_fill_workspace", "primx_texbake_fill"), 28),                 # mesh.py's texture bake
    **dict.fromkeys(("primx_meshclean_workspace", "primx_meshclean_merge", "primx_meshclean_faces", "primx_meshclean_components",
                     "primx_meshclean_edges", "primx_meshclean_fans"), 29),                      # mesh.clean_mesh
    **dict.fromkeys(("primx_meshdecim_workspace", "primx_meshdecim_edges", "primx_meshdecim_quadrics", "primx_meshdecim_costs",
                     "primx_meshdecim_select", "primx_meshdecim_collapse", "primx_meshdecim_finish",
                     "primx_meshdecim_normals"), 30),                                            # mesh.decimate_mesh
    **dict.fromkeys(("primx_latent_norm", "primx_enc_conv_in", "primx_conv3d_down_s8c32", "primx_enc_head"), 31),   # VAE.encode
    **dict.fromkeys(("primx_q_sample", "primx_diffusion_reverse_step", "primx_diffusion_step_keep"), 32),             # editing
    **dict.fromkeys(("primx_mesh_field_query", "primx_mesh_face_areas", "primx_mesh_surface_points", "primx_fps"), 33),  # fit.py
    **dict.fromkeys(("primx_primsdf_query_backward", "primx_adam_step"), 34),                    # differentiable PrimSDF, refine=
    "primx_raymarch_backward": 35,                                                               # the marcher's backward
    **dict.fromkeys(("primx_primsdf_query_grad", "primx_texbake_tangents", "primx_texbake_normal_texels"), 35),   # the normal map
    "primx_texbake_occlusion": 35,                                                               # ambient occlusion, the same way
    **dict.fromkeys(("primx_nearest_points", "primx_distance_stats"), 35),                       # metrics.py, the same way
    **dict.fromkeys(("primx_mesh_bvh_workspace", "primx_mesh_bvh_build", "primx_mesh_bvh_query"), 35),   # fit.MeshBVH, the same way
    **dict.fromkeys(("primx_mesh_bvh_raycast", "primx_mesh_bvh_visibility"), 35),                # its ray queries, the same way
    **dict.fromkeys(("primx_material_sample",                                                    # a MeshField with a material
                     "primx_attention_ksplit_mode", "primx_attention_ksplit",                    # without them: attention never splits its keys
                     "primx_gemm_toq64_mode",                                                    # without it: to_q under the null skip on the 128-row tile
                     "primx_dit_blocks_fold_features"), _PROBE),                                 # bit 0: the null skip's tail of PrimxDitForwardFold is read
}
# what the DiT's route asks of the library (`capabilities`): feature -> the entry point whose presence tells
_FEATURES: dict = {"fold": "primx_linear_fold", "blocks_call": "primx_dit_blocks_fold", "kv_ride": "primx_linear_heads_fold_pair",
                   "f32out_group": "primx_linear_f32out_group", "null_skip": "primx_dit_blocks_fold_features",
                   "attn_ksplit": "primx_attention_ksplit", "toq64": "primx_gemm_toq64_mode"}
_AB_ABI_VERSIONS: tuple = (21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34)
_caps: dict = {}        # library path -> frozenset of feature names

_lib: Optional[C.CDLL] = None


class PrimxError(RuntimeError):
    """A C-ABI entry point returned a non-zero status."""


def load(path: Optional[str] = None) -> C.CDLL:
    """dlopen the library and attach prototypes.  Raises if it is missing or ABI-mismatched."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP library is not built. Run `python __graft_entry__.py` "
            "(build()) first - there is no PyTorch/CPU fallback for this path."
        )
    if path == LIB_PATH and not os.environ.get("PRIMX_LIB") and not os.environ.get("PRIMX_SKIP_FRESH_CHECK"):
        # the binary must have been built from exactly the sources next to it (content hashes, csrc/build.py): a
        # stale shipped .so is an error, never silently benchmarked
        import importlib.util
        spec = importlib.util.spec_from_file_location("primx_build", os.path.join(_HERE, "csrc", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if not mod.check_fresh():
            raise RuntimeError(f"{path} does not match the sources in {os.path.dirname(path)} (build_manifest.json): "
                               "run `python __graft_entry__.py` (build()) to rebuild it")
    # make sure the HIP runtime PyTorch uses is the one already mapped (same SONAME libamdhip64.so.7)
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - symbol-table checks work without torch
        pass
    lib = C.CDLL(path)
    ab = bool(os.environ.get("PRIMX_LIB"))
    lib.primx_abi_version.restype = C.c_int
    got = lib.primx_abi_version()
    if got != ABI_VERSION and not (ab and got in _AB_ABI_VERSIONS):
        raise RuntimeError(f"libprimx_hip.so ABI {got} != expected {ABI_VERSION}; rebuild it")
    bound = set()
    for name, argtypes in SIGNATURES.items():
        since = _SINCE.get(name, 21)
        if got < since or (since in (_PROBE, 35) and ab and not hasattr(lib, name)):
            continue                # an older A/B build: it lacks the entry point (or, before 23, has it with another argument list)
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, C.c_int)
        bound.add(name)
    _caps[path] = frozenset(f for f, name in _FEATURES.items() if name in bound
                            and (f != "null_skip" or (got >= 35 and lib.primx_dit_blocks_fold_features() & 1)))
    if path == LIB_PATH:
        _lib = lib
    return lib


def capabilities(path: Optional[str] = None) -> frozenset:
    """What the library at `path` (default: the loaded one) can do, as feature names: "fold" (the LayerNorm-fold entry points, ABI 23),
    "blocks_call" (primx_dit_blocks_fold, 24), "kv_ride" (it projects the conditioning K / V itself, on the qkv launches, 25),
    "f32out_group" (primx_linear_f32out_group, 26), "null_skip" (primx_dit_blocks_fold reads the null cross-attention skip's tail),
    "attn_ksplit" (the attention key split and its switch), "toq64" (to_q's 64-row tile under the null skip and its switch).  Only an
    older PRIMX_LIB A/B build lacks any of them."""
    path = path or LIB_PATH
    if path not in _caps:
        load(path)
    return _caps[path]


def fold_available() -> bool:
    return "fold" in capabilities()


def blocks_call_available() -> bool:
    return "blocks_call" in capabilities()


def kv_ride_available() -> bool:
    return "kv_ride" in capabilities()


def f32out_group_available() -> bool:
    return "f32out_group" in capabilities()


def null_skip_available() -> bool:
    return "null_skip" in capabilities()


def attn_ksplit_available() -> bool:
    return "attn_ksplit" in capabilities()


def toq64_available() -> bool:
    return "toq64" in capabilities()


def check(status: int, name: str) -> None:
    if status != 0:
        msg = load().primx_last_error()
        raise PrimxError(f"{name} failed ({status}): {msg.decode() if msg else '?'}")
