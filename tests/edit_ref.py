"""CPU restatement of the editing steps and loops (TEST INFRASTRUCTURE): q_sample, the DDIM step run towards noise, the
kept-token DDIM step and the loops over them, in torch-CPU fp32 tensor ops in the reference's operation order
(gaussian_diffusion.py:216-231, 580-616).  Built from oracle/diffusion_ref.py's pieces - `_ex` (a float64 table value cast
to fp32), `_sqrt32` (a correctly rounded fp32 square root), `predict_xstart`, `ddim_step` - and held bit for bit to the REAL
reference by tests/golden/edit.npz (tests/test_edit_cpu.py).

Levels: level i is what `ddim_step` at i accepts; `ddim_step` at i maps level i to level i - 1 (step 0: the clean sample);
`reverse_step` at i maps level i to level i + 1."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from oracle.diffusion_ref import Tables, _ex, _sqrt32, ddim_step, predict_xstart


def q_sample(tab: Tables, i: int, x_start: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """gaussian_diffusion.py:216-231."""
    return _ex(tab.sqrt_acp, i, x_start) * x_start + _ex(tab.sqrt_1m_acp, i, x_start) * noise


def reverse_step(tab: Tables, i: int, x: torch.Tensor, model_out: torch.Tensor, parameterization: str = "v",
                 clip: bool = False) -> Dict[str, torch.Tensor]:
    """ddim_reverse_sample (gaussian_diffusion.py:580-616); alphas_cumprod_next = append(acp[1:], 0) (:163)."""
    C = x.shape[-1]
    x0 = predict_xstart(tab, i, x, model_out[..., :C], parameterization)
    if clip:
        x0 = x0.clamp(-1, 1)
    eps = (_ex(tab.sqrt_recip_acp, i, x) * x - x0) / _ex(tab.sqrt_recipm1_acp, i, x)
    abar_next = _ex(np.append(tab.acp[1:], 0.0), i, x)
    return {"sample": x0 * _sqrt32(abar_next) + _sqrt32(1 - abar_next) * eps, "pred_xstart": x0}


def keep_step(tab: Tables, i: int, x: torch.Tensor, model_out: torch.Tensor, known: torch.Tensor, known_noise: torch.Tensor,
              keep: torch.Tensor, parameterization: str = "v", eta: float = 0.0, clip: bool = False,
              noise: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """ddim_step where `keep` (bool, broadcastable to x) is False; where it is True pred_xstart = known and the sample is
    q_sample(known, known_noise) at level i - 1 (`known` itself at step 0), whatever the model returned there."""
    keep = keep.expand_as(x) if keep.dim() == x.dim() else keep[..., None].expand_as(x)
    free = ddim_step(tab, i, x, model_out, parameterization, eta, clip, noise)
    held = q_sample(tab, i - 1, known, known_noise) if i > 0 else known
    return {"sample": torch.where(keep, held, free["sample"]), "pred_xstart": torch.where(keep, known, free["pred_xstart"].float())}


def _t(x: torch.Tensor, tmap: List[int], i: int) -> torch.Tensor:
    return torch.full((x.shape[0],), tmap[i], dtype=torch.int64)


def reverse_loop(model: Callable, x: torch.Tensor, tab: Tables, tmap: List[int], parameterization: str = "v", clip: bool = False,
                 start_step: int = 0, stop_step: Optional[int] = None, **model_kwargs) -> List[Dict[str, torch.Tensor]]:
    """Steps start_step .. stop_step - 1 ascending from level start_step; the last sample is level stop_step (default n - 1)."""
    outs = []
    for i in range(start_step, tab.n - 1 if stop_step is None else stop_step):
        out = reverse_step(tab, i, x, model(x, _t(x, tmap, i), **model_kwargs), parameterization, clip)
        outs.append(out)
        x = out["sample"]
    return outs


def partial_loop(model: Callable, x: torch.Tensor, tab: Tables, tmap: List[int], parameterization: str = "v", eta: float = 0.0,
                 clip: bool = False, start_step: Optional[int] = None, known: Optional[torch.Tensor] = None,
                 keep: Optional[torch.Tensor] = None, known_noise: Optional[torch.Tensor] = None,
                 **model_kwargs) -> List[Dict[str, torch.Tensor]]:
    """Steps start_step .. 0 descending from level start_step (default n - 1), every step a keep_step when `keep` is given."""
    outs = []
    for i in range(tab.n - 1 if start_step is None else start_step, -1, -1):
        mo = model(x, _t(x, tmap, i), **model_kwargs)
        if keep is None:
            out = ddim_step(tab, i, x, mo, parameterization, eta, clip)
        else:
            out = keep_step(tab, i, x, mo, known, known_noise, keep, parameterization, eta, clip)
        outs.append(out)
        x = out["sample"]
    return outs
