"""DDIM / ancestral sampling loops over a denoiser callable.

Host-side mirror of the reference's ``GaussianDiffusion`` / ``SpacedDiffusion`` /
``_WrappedModel`` (models/diffusion/gaussian_diffusion.py:145-698,
models/diffusion/respace.py:65-129): same constructor arguments, same method
names and generator protocol (each step yields ``{"sample", "pred_xstart"}``),
same assertions.

What is different by design (MI355X-first):

* The reference re-uploads ~10 one-element tables and materialises ~10
  full-size temporaries per step (``_extract_into_tensor``,
  gaussian_diffusion.py:880-892).  Here every per-step scalar is computed ONCE
  on the host in float32 - following the reference's float32 operation order
  exactly - uploaded as one ``[n_steps, 16]`` table at loop start, and the whole
  update ``x_t, model_out -> x_{t-1}, pred_xstart`` is ONE fused HIP kernel
  (``primx_diffusion_step``) that indexes the table by the step number carried
  as a kernel argument.  No host<->device traffic inside the loop.
* The spaced->original timestep map (respace.py:124-129) lives on the device
  as an int64 vector; step ``i`` hands the model ``map[i].expand(B)``.
* There is no CPU arithmetic path: tensors must live on a HIP device and the
  HIP library must be built, otherwise the loop raises.

Editing (DESIGN.md "Editing").  *Level i* is what
``ddim_sample`` at ``t = i`` accepts; ``ddim_sample`` at step ``i`` maps level
``i`` to level ``i - 1`` and step 0 produces the clean sample.

* ``q_sample`` (gaussian_diffusion.py:216-231) takes a clean sample to level
  ``t`` (``primx_q_sample``) and ``ddim_reverse_sample``
  (gaussian_diffusion.py:580-616) takes level ``t`` to level ``t + 1``
  (``primx_diffusion_reverse_step``); both have the reference's signatures.
* New API in the reference's naming style - the reference has no loop over the
  reverse step, no partial loop and no masked loop:
  ``ddim_reverse_sample_loop[_progressive]`` (steps ``start_step .. stop_step - 1``
  ascending), ``ddim_sample_loop*(start_step=k)`` (``noise`` is level ``k``, steps
  ``k .. 0``) and ``ddim_sample_loop*(known=, keep=, known_noise=)``: every step is
  ``primx_diffusion_step_keep``, which holds the flagged elements on the
  trajectory ``q_sample(known, known_noise, level)`` - one noise tensor per loop.
* Every loop is ``_loop`` over an index sequence.  A loop that is not the full
  descending one announces only the rows it will use
  (``plan_timesteps(tmap[indices])``, selected by position).

Few-step sampling (DESIGN.md "Few-step sampling").
``dpm_solver_sample_loop[_progressive]`` is DPM-Solver++(2M) (Lu et al. 2022,
arXiv:2211.01095): a second-order multistep solver of the same probability-flow
ODE the DDIM loop (eta = 0) integrates to first order, over the same ``ddimK``
index sequences - no new timestep grid.  The reference has no counterpart.

* With ``lambda = 0.5 * log(acp / (1 - acp))``, ``h_i = lambda(acp_prev[i]) -
  lambda(acp[i])`` and ``r_i = h_{i+1} / h_i``, the 2M step from level ``i`` to
  level ``i - 1`` is, in exact arithmetic, ``DDIM(x, x0_i) + k_i * (x0_i -
  x0_prev)`` with ``k_i = sqrt(acp_prev[i]) * (1 - exp(-h_i)) / (2 r_i)`` and
  ``x0_prev`` the previous (noisier) step's ``pred_xstart``.
* The table trick: the fused step computes ``x0 * col9 + col10 * eps +
  (col12 * col11) * noise``.  ``dpm_solver_coefficients`` is the DDIM table with
  ``col9 + k_i`` and ``col11 = -k_i``; the loop passes ``noise := x0_prev``.  The
  same two kernels (``primx_diffusion_step`` / ``primx_diffusion_step_keep``)
  then perform the 2M step: no new kernel, no new entry point, nothing drawn.
* ``k_i = 0`` - the row IS the DDIM row and no history is passed - at the loop's
  first step (no history yet), at step 0 (``acp_prev = 1``) and at every step
  below ``lower_order_final``.  Defaults: ``order = 2``, ``lower_order_final = 2``
  (the last TWO steps are first-order: on a grid uniform in t the final step's
  ``h`` is several times its predecessor's and the extrapolation overshoots).
  ``order = 1`` is the DDIM loop, bit for bit.
* ``clip_denoised`` clips ``x0`` as DDIM does; the history holds the clipped
  values.  Partial (``start_step``) and masked (``known`` / ``keep`` /
  ``known_noise``) loops work as in DDIM.

Out of scope (no caller on the inference path):
``training_losses``, VLB terms, ``cond_fn`` / ``denoised_fn`` hooks
(NotImplementedError when passed), RePaint-style resampling jumps, masked
ancestral sampling, differing timesteps within a batch; for the few-step solver
order 3, SDE variants, UniPC correctors and other timestep grids.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterator, Optional, Sequence

import numpy as np
import torch

from .schedule import (
    DiffusionTables,
    LossType,
    ModelMeanType,
    ModelVarType,
    respaced_betas,
)

COEF_STRIDE = 16  # floats per step in the device coefficient table (see include/primx_hip.h)

# column indices of the coefficient table - keep in sync with csrc/rowops.hip (diffusion_step_kernel)
C_SQRT_ACP, C_SQRT_1M_ACP, C_SQRT_RECIP_ACP, C_SQRT_RECIPM1_ACP = 0, 1, 2, 3
C_POST_MEAN1, C_POST_MEAN2, C_MIN_LOG, C_MAX_LOG, C_FIXED_LOGVAR = 4, 5, 6, 7, 8
C_DDIM_X0, C_DDIM_EPS, C_DDIM_SIGMA, C_NONZERO, C_FIXED_VAR = 9, 10, 11, 12, 13
C_REV_X0, C_REV_EPS = 14, 15    # the reverse (towards noise) DDIM step: sqrt(acp_next), sqrt(1 - acp_next) (diffusion_reverse_step_kernel)

# PRIMX_PLAN_TIMESTEPS=0: the sampling loops do not announce their timesteps to the model (A/B of DiT.plan_timesteps)
PLAN_TIMESTEPS = __import__("os").environ.get("PRIMX_PLAN_TIMESTEPS", "1") != "0"
# Longest loop that is planned.  Device memory per planned step for DiT-XL: 0.6 MB of 16-bit modulation rows (n x (depth * 9 + 2) * D)
# + 2.1 MB of fp32 u / v rows when the LayerNorm fold applies (2 x 9216 columns x depth; DiT._fold_tables) + their 16-bit A operands
# (0.4 MB): ~0.8 GB at 256 steps, freed when the loop ends (clear_timestep_plan drops the plan).  The fold's share is capped separately:
# loops longer than DiT.fold_max_steps (128: BASELINE configs[3]'s 100 steps fold, 0.33 GB) are planned WITHOUT the fold.
PLAN_MAX_STEPS = 256
_MEAN_CODE = {ModelMeanType.EPSILON: 0, ModelMeanType.START_X: 1, ModelMeanType.VELOCITY: 2}
_VAR_CODE = {
    ModelVarType.FIXED_SMALL: 0,
    ModelVarType.FIXED_LARGE: 1,
    ModelVarType.LEARNED: 2,
    ModelVarType.LEARNED_RANGE: 3,
}


def _f32(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64).astype(np.float32)


class GaussianDiffusion(DiffusionTables):
    """Sampling half of the reference's ``GaussianDiffusion`` (gaussian_diffusion.py:145-698)."""

    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type):
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        super().__init__(betas)
        self._dev_cache: Dict = {}

    # ------------------------------------------------------------------ tables
    def step_coefficients(self, eta: float = 0.0) -> np.ndarray:
        """float32 ``[num_timesteps, 16]`` table of every scalar one sampling step needs.

        Each entry reproduces what the reference computes on the fly:
        ``_extract_into_tensor`` = float64 table value cast to float32
        (gaussian_diffusion.py:889); the DDIM scalars follow
        gaussian_diffusion.py:561-573 with every intermediate rounded to float32
        as torch does (``eta`` is a Python float multiplied into a float32 tensor).
        """
        n = self.num_timesteps
        tab = np.zeros((n, COEF_STRIDE), dtype=np.float32)
        tab[:, C_SQRT_ACP] = _f32(self.sqrt_alphas_cumprod)
        tab[:, C_SQRT_1M_ACP] = _f32(self.sqrt_one_minus_alphas_cumprod)
        tab[:, C_SQRT_RECIP_ACP] = _f32(self.sqrt_recip_alphas_cumprod)
        tab[:, C_SQRT_RECIPM1_ACP] = _f32(self.sqrt_recipm1_alphas_cumprod)
        tab[:, C_POST_MEAN1] = _f32(self.posterior_mean_coef1)
        tab[:, C_POST_MEAN2] = _f32(self.posterior_mean_coef2)
        if n > 1:
            tab[:, C_MIN_LOG] = _f32(self.posterior_log_variance_clipped)
        tab[:, C_MAX_LOG] = _f32(np.log(self.betas))
        if self.model_var_type == ModelVarType.FIXED_LARGE and n > 1:
            var = np.append(self.posterior_variance[1], self.betas[1:])
            tab[:, C_FIXED_VAR] = _f32(var)
            tab[:, C_FIXED_LOGVAR] = _f32(np.log(var))
        elif self.model_var_type == ModelVarType.FIXED_SMALL and n > 1:
            tab[:, C_FIXED_VAR] = _f32(self.posterior_variance)
            tab[:, C_FIXED_LOGVAR] = _f32(self.posterior_log_variance_clipped)

        one = np.float32(1.0)
        abar = _f32(self.alphas_cumprod)
        abar_prev = _f32(self.alphas_cumprod_prev)
        abar_next = _f32(self.alphas_cumprod_next)     # gaussian_diffusion.py:611-614; 0 at the last step
        eta32 = np.float32(eta)
        with np.errstate(divide="ignore", invalid="ignore"):
            sigma = (eta32 * np.sqrt((one - abar_prev) / (one - abar))) * np.sqrt(one - abar / abar_prev)
            sigma = sigma.astype(np.float32)
            tab[:, C_DDIM_X0] = np.sqrt(abar_prev)
            tab[:, C_DDIM_EPS] = np.sqrt((one - abar_prev) - sigma * sigma)
        tab[:, C_DDIM_SIGMA] = sigma
        tab[:, C_NONZERO] = (np.arange(n) != 0).astype(np.float32)
        tab[:, C_REV_X0] = np.sqrt(abar_next)
        tab[:, C_REV_EPS] = np.sqrt(one - abar_next)
        return tab

    def dpm_solver_k(self, order: int = 2, lower_order_final: int = 2, first_step: Optional[int] = None) -> np.ndarray:
        """float64 ``[num_timesteps]``: the history weight ``k_i`` of DPM-Solver++(2M) per step (0 where the step is first-order).
        See ``dpm_solver_coefficients``."""
        n = self.num_timesteps
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order!r}")
        if int(lower_order_final) < 1:
            raise ValueError(f"lower_order_final must be at least 1, got {lower_order_final!r}")
        first_step = n - 1 if first_step is None else int(first_step)
        if not (0 <= first_step < n):
            raise ValueError(f"first_step must lie in 0 .. {n - 1}, got {first_step}")
        k = np.zeros(n, dtype=np.float64)
        if order == 1:
            return k
        acp = np.asarray(self.alphas_cumprod, dtype=np.float64)
        acp_prev = np.asarray(self.alphas_cumprod_prev, dtype=np.float64)
        lam = lambda a: 0.5 * np.log(a / (1.0 - a))
        # i = n - 1 has no noisier level before it: first-order whatever first_step says
        for i in range(max(1, int(lower_order_final)), n - 1):
            if i == first_step:
                continue
            h = lam(acp_prev[i]) - lam(acp[i])
            h_before = lam(acp_prev[i + 1]) - lam(acp[i + 1])       # the previous (noisier) step's
            k[i] = np.sqrt(acp_prev[i]) * -np.expm1(-h) / (2.0 * (h_before / h))
        return k

    def dpm_solver_coefficients(self, order: int = 2, lower_order_final: int = 2, first_step: Optional[int] = None) -> np.ndarray:
        """The coefficient table under which the fused DDIM step performs DPM-Solver++(2M): ``step_coefficients(0.0)`` with
        column 9 = ``float32(float64(col 9) + k_i)`` and column 11 = ``float32(-k_i)`` where ``k_i != 0``; every other entry,
        and every row with ``k_i = 0``, is the DDIM table bit for bit.  The loop passes the previous step's ``pred_xstart``
        where the kernel takes ``noise``: ``x0 * (c_x0 + k) + c_eps * eps + (nonzero * -k) * x0_prev``
        = ``DDIM + k * (x0 - x0_prev)``.

        ``k_i = alpha_next * (1 - exp(-h_i)) / (2 r_i)`` in float64 from ``alphas_cumprod`` / ``alphas_cumprod_prev``, with
        ``lambda = 0.5 * log(acp / (1 - acp))``, ``h_i = lambda(acp_prev[i]) - lambda(acp[i])``, ``r_i = h_{i+1} / h_i``,
        ``alpha_next = sqrt(acp_prev[i])``.  ``k_i = 0`` when ``order == 1``; at ``i == 0`` (``acp_prev = 1``: the step returns
        ``pred_xstart`` as DDIM does); at ``i < lower_order_final``; at ``i == first_step``, the loop's first step, which has
        no history (default ``num_timesteps - 1``; the last row has no noisier level before it and is first-order always).

        ``lower_order_final`` defaults to 2.  On a grid uniform in t the step into timestep 0 spans several times the previous
        step's ``h`` (ddim10, linear schedule: 3.5 against 0.75), the linear extrapolation of ``x0`` overshoots there, and on the
        closed-form Gaussian denoiser (DESIGN.md "Few-step sampling") ``lower_order_final = 1`` ends at an RMS error of 0.22
        where DDIM itself ends at 0.136.  With the last two steps first-order 2M ends at 0.082."""
        k = self.dpm_solver_k(order, lower_order_final, first_step)
        tab = self.step_coefficients(0.0)
        on = k != 0.0
        tab[on, C_DDIM_X0] = (tab[on, C_DDIM_X0].astype(np.float64) + k[on]).astype(np.float32)
        tab[on, C_DDIM_SIGMA] = (-k[on]).astype(np.float32)
        return tab

    # ------------------------------------------------------------------ device state
    def _timestep_ids(self) -> Sequence[int]:
        """Values handed to the model for spaced step i (identity for an un-spaced process)."""
        return list(range(self.num_timesteps))

    def _device_state(self, device: torch.device, eta: float, solver: Optional[tuple] = None):
        """(coef, tmap) of the DDIM / ancestral table at `eta`, or - `solver` = (order, lower_order_final, first_step) - (coef,
        tmap, uses_history) of the 2M table, uses_history[i] saying whether row i has k_i != 0.  One entry per family is kept
        (the latest (device, eta) and the latest (device, solver)), so alternating DDIM and 2M loops rebuild neither."""
        key = (str(device), float(eta)) if solver is None else (str(device), "dpm") + tuple(solver)
        st = self._dev_cache.get(key)
        if st is None:
            tmap = torch.tensor(list(self._timestep_ids()), dtype=torch.int64, device=device)
            if solver is None:
                st = (torch.from_numpy(self.step_coefficients(eta)).to(device), tmap)
            else:
                tab = self.dpm_solver_coefficients(*solver)
                st = (torch.from_numpy(tab).to(device), tmap, (tab[:, C_DDIM_SIGMA] != 0).tolist())
            other = {k: v for k, v in self._dev_cache.items() if (k[1] == "dpm") != (solver is not None)}
            self._dev_cache = {**other, key: st}  # keep only the latest of each family
        return st

    # ------------------------------------------------------------------ one step
    def _step(self, kind: str, model: Callable, x: torch.Tensor, i: int, **kw):
        from .. import ops  # deferred: importing the sampler must not need the HIP library
        with ops.device_of(x):   # launches go to the current device's stream: make x's device current for the step
            return self._step_on_device(kind, model, x, i, **kw)

    def _step_on_device(self, kind: str, model: Callable, x: torch.Tensor, i: int, *, clip_denoised: bool,
                        model_kwargs: Optional[dict], eta: float, coef: torch.Tensor, tmap: torch.Tensor, planner=None,
                        row: Optional[int] = None, keep_args: Optional[dict] = None, history: Optional[torch.Tensor] = None):
        """`row`: the planner's row of this step (its position in the announced sequence; None: the step index, the full
        loop's convention).  `keep_args`: known / known_noise / keep of a masked DDIM loop.  `history` (kind "dpm"): the
        previous step's pred_xstart where `coef`'s row has k != 0, else None - it goes where the kernel takes noise."""
        from .. import ops

        if x.dim() != 3:
            raise AssertionError("x must be (B, n_tokens, C)")
        B, nt, C = x.shape
        # (B,) int64 timesteps of the ORIGINAL process (respace.py:124-129): a row of the per-loop [n, B] table (contiguous,
        # so nothing downstream has to copy it), or a broadcast view for the single-step API.  No allocation, no H2D.
        t_model = tmap[i] if tmap.dim() == 2 else tmap[i].expand(B)
        if planner is not None:
            planner.select_planned_timestep(i if row is None else row)        # the row announced in _loop
        try:
            model_output = model(x, t_model, **(model_kwargs or {}))
        finally:
            if planner is not None:
                planner.select_planned_timestep(None)
        if isinstance(model_output, tuple):
            model_output = model_output[0]
        learned = self.model_var_type in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE)
        want = (B, nt, C * 2) if learned else (B, nt, C)
        if tuple(model_output.shape) != want:
            raise AssertionError(f"model output shape {tuple(model_output.shape)} != {want}")
        # eta == 0: the reference still draws `th.randn_like(x)` every DDIM step and multiplies it by sigma = 0
        # (gaussian_diffusion.py:569-579).  The sample is identical without the draw; what differs is the process-global
        # RNG position afterwards, so a LATER seeded draw in the same process (the next sample's initial noise when no
        # generator is passed) does not replay a reference run.  Callers that need that pass explicit noise / a generator.
        if kind == "reverse":
            sample, pred_xstart = ops.diffusion_reverse_step(x, model_output, coef, i, mean_type=_MEAN_CODE[self.model_mean_type],
                                                             clip_denoised=clip_denoised)
            return {"sample": sample, "pred_xstart": pred_xstart}
        if kind == "dpm":
            noise = history                     # nothing is drawn: the 2M table's column 11 is -k, the "noise" is x0_prev
        else:
            need_noise = (kind == "ancestral") or (eta != 0.0)
            noise = torch.randn_like(x) if need_noise else None
        step_fn, extra = (ops.diffusion_step, {}) if keep_args is None else (ops.diffusion_step_keep, keep_args)
        sample, pred_xstart = step_fn(
            x, model_output, coef, i,
            mean_type=_MEAN_CODE[self.model_mean_type],
            var_type=_VAR_CODE[self.model_var_type],
            ancestral=(kind == "ancestral"),
            clip_denoised=clip_denoised,
            noise=noise,
            **extra,
        )
        return {"sample": sample, "pred_xstart": pred_xstart}

    def _keep_args(self, img: torch.Tensor, known, keep, known_noise) -> Optional[dict]:
        """The operands of a masked loop as primx_diffusion_step_keep takes them (fp32 known / known_noise of the sample's shape;
        keep bool (B, N), (B, N, 1) or (B, N, C) -> uint8 per row or per element), made once per loop."""
        if keep is None:
            return None
        B, N, C = img.shape
        if keep.dtype != torch.bool or tuple(keep.shape) not in ((B, N), (B, N, 1), (B, N, C)):
            raise ValueError(f"keep must be a bool tensor of shape (B, N), (B, N, 1) or (B, N, C) = {(B, N, C)}, got "
                             f"{keep.dtype} {tuple(keep.shape)}")
        for name, a in (("known", known), ("known_noise", known_noise)):
            if tuple(a.shape) != (B, N, C):
                raise ValueError(f"{name} must have the sample's shape {(B, N, C)}, got {tuple(a.shape)}")
        dev = img.device
        if keep.dim() == 3 and keep.shape[2] == 1 and C != 1:
            keep = keep[:, :, 0]
        return dict(known=known.to(dev, torch.float32).contiguous(), known_noise=known_noise.to(dev, torch.float32).contiguous(),
                    keep=keep.to(dev).contiguous().view(torch.uint8))

    def _loop(self, kind: str, model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs,
              device, progress, eta, indices: Optional[Sequence[int]] = None, known=None, keep=None,
              known_noise=None, solver: Optional[tuple] = None) -> Iterator[dict]:
        """Every sampling loop: the steps `indices` in order, each fed the previous one's sample.  None is the full descending loop
        n - 1 .. 0 on its own code path (the planner is handed every row and selects by step index).  `solver` (kind "dpm"):
        (order, lower_order_final) of DPM-Solver++; the loop then carries the previous step's pred_xstart."""
        if denoised_fn is not None or cond_fn is not None:
            raise NotImplementedError("denoised_fn / cond_fn hooks are outside the accelerated path")
        if self.model_mean_type not in _MEAN_CODE:
            raise NotImplementedError(f"Model Mean type {self.model_mean_type} is not supported!")
        if len({a is None for a in (known, keep, known_noise)}) != 1:
            raise ValueError("known, keep and known_noise are given together or not at all")
        if device is None:
            device = noise.device if noise is not None else next(model.parameters()).device
        device = torch.device(device)
        if not isinstance(shape, (tuple, list)):
            raise AssertionError("shape must be a tuple or list")
        img = noise if noise is not None else torch.randn(*shape, device=device)
        if img.device.type != "cuda":
            raise RuntimeError(
                "the sampler runs on a HIP device only (there is no CPU arithmetic path); "
                f"got a tensor on {img.device}"
            )
        img = img.float().contiguous()
        keep_args = self._keep_args(img, known, keep, known_noise)
        if kind == "dpm":
            first = self.num_timesteps - 1 if indices is None else int(indices[0])
            coef, tmap1, uses_history = self._device_state(img.device, 0.0, tuple(solver) + (first,))
        else:
            coef, tmap1 = self._device_state(img.device, eta)
        tmap = tmap1[:, None].expand(-1, img.shape[0]).contiguous()     # [n_steps, B], built once per loop
        # The loop knows every timestep it will ask the model for.  A model that can use that (DiT.plan_timesteps: the
        # timestep-only adaLN modulation of all steps is computed once per loop, several rows per pass over the weights,
        # instead of one row per step) is told; the rows are selected by step index, no device read-back.  `model` is the
        # reference's call convention: a module or a bound method such as `model.forward_with_cfg` (inference.py:306-311).
        owner = getattr(model, "__self__", model)
        if indices is None:
            steps = list(range(self.num_timesteps - 1, -1, -1))
            rows = steps                                                # every row is announced: row = step index
        else:
            steps = [int(i) for i in indices]
            rows = list(range(len(steps)))                              # only the loop's rows, in loop order: row = position
        planner = owner if (callable(getattr(owner, "plan_timesteps", None)) and PLAN_TIMESTEPS
                            and len(steps) <= PLAN_MAX_STEPS) else None
        if planner is not None:
            planner.plan_timesteps(tmap1 if indices is None
                                   else tmap1[torch.tensor(steps, dtype=torch.int64, device=tmap1.device)])
        todo = list(zip(steps, rows))
        shown = todo
        if progress:
            from tqdm.auto import tqdm
            shown = tqdm(todo)
        img0 = img
        hist = [None]       # kind "dpm": the previous step's pred_xstart (clipped if the loop clips); part of what a repeat resets

        def step(x, i, row):
            with torch.no_grad():   # scoped to the step: a generator must not hold the grad-mode context across yields
                h = hist[0] if kind == "dpm" and uses_history[i] else None
                out = self._step(kind, model, x, i, clip_denoised=clip_denoised, model_kwargs=model_kwargs, eta=eta, coef=coef,
                                 tmap=tmap, planner=planner, row=row, keep_args=keep_args, history=h)
                if kind == "dpm":
                    hist[0] = out["pred_xstart"]
                return out

        def restart():
            hist[0] = None
        try:
            for pos, (i, row) in enumerate(shown):
                out = step(img, i, row)
                if pos == len(todo) - 1:
                    out = self._fold_guard(planner, out, img0, step, todo, restart)   # BEFORE the final yield: consumers stop at the last item
                yield out
                img = out["sample"]
        finally:
            if planner is not None:
                planner.clear_timestep_plan()

    def _fold_guard(self, planner, out: dict, img0: torch.Tensor, step: Callable, todo: Sequence,
                    restart: Optional[Callable] = None) -> dict:
        """A model that folded its LayerNorms in fp16 (DiT.fold_ln) has the FINAL sample of the loop checked once (one reduction +
        one read-back per loop; NaN / inf propagate through the diffusion update, clipped or not).  The folded operand is
        normalised with the previous site's statistics, so it leaves the fp16 range only if ONE gated branch multiplies a row's
        spread by > 1e3 - no model of the suite comes near.  If it ever happens the loop is run again with the LayerNorm launches
        (whose operand cannot overflow, as in the reference) and THAT result is returned: same contract as the reference, which
        returns whatever its fp16 arithmetic gives.

        What a caller sees on that (never observed) path: `*_sample_loop` return the second loop's sample.  A consumer of the
        `*_progressive` generators has already been handed the FIRST loop's intermediate items - a generator cannot take them back - and
        gets the second loop's final item last: the trajectory it saw is not one loop's (a RuntimeWarning says so).  The second loop
        draws its own noise where the sampler is stochastic (ancestral steps, DDIM with eta > 0): it is a new sample of the same
        distribution, not a replay.  A NaN that does not come from the fold (bad weights or conditioning) survives the second loop and
        is returned as it is, after the same warning.

        `todo`: the loop's (step, planner row) sequence - the SAME loop is repeated (a partial, reverse or masked one as it was:
        `step` carries the keep operands).  `restart` drops what `step` carries from one step to the next (the 2M solver's
        history), so the repeated loop starts as a fresh one does."""
        over = getattr(planner, "fold_overflowed", None) if planner is not None else None
        if not callable(over) or not over(out["sample"]):
            return out
        import warnings
        warnings.warn("non-finite sample after a sampling loop with the fp16 LayerNorm fold: running the loop again with "
                      "LayerNorm launches (PRIMX_DIT_FOLD=0 / model.fold_ln = False avoids the first attempt); items already "
                      "yielded by a *_progressive generator belong to the first loop", RuntimeWarning)
        keep, planner.fold_ln = planner.fold_ln, False
        try:
            img = img0
            if restart is not None:
                restart()
            for i, row in todo:
                out = step(img, i, row)
                img = out["sample"]
        finally:
            planner.fold_ln = keep
        return out

    # ------------------------------------------------------------------ public API (reference names)
    def p_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                  cond_fn=None, model_kwargs=None, device=None, progress=False):
        """Ancestral sampling generator (gaussian_diffusion.py:476-529)."""
        return self._loop("ancestral", model, shape, noise, clip_denoised, denoised_fn, cond_fn,
                          model_kwargs, device, progress, 0.0)

    def p_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                      model_kwargs=None, device=None, progress=False):
        """gaussian_diffusion.py:437-474."""
        final = None
        for final in self.p_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                    denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                    model_kwargs=model_kwargs, device=device,
                                                    progress=progress):
            pass
        return final["sample"]

    def _descending(self, start_step: Optional[int]) -> Optional[Sequence[int]]:
        """Steps of a DDIM loop whose input is level `start_step`: start_step .. 0 (None: the full loop on its own path)."""
        if start_step is None:
            return None
        if not (0 <= int(start_step) < self.num_timesteps):
            raise ValueError(f"start_step must lie in 0 .. {self.num_timesteps - 1}, got {start_step}")
        return range(int(start_step), -1, -1)

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                     cond_fn=None, model_kwargs=None, device=None, progress=False, eta=0.0,
                                     start_step=None, known=None, keep=None, known_noise=None):
        """DDIM generator (gaussian_diffusion.py:651-698).  Beyond the reference: `start_step = k` treats `noise` as level k and
        runs steps k .. 0; `known` / `keep` / `known_noise` (together) hold the elements flagged by the bool `keep` - (B, N),
        (B, N, 1) or (B, N, C) - on the trajectory q_sample(known, known_noise, level) at every step and end them at `known`."""
        return self._loop("ddim", model, shape, noise, clip_denoised, denoised_fn, cond_fn,
                          model_kwargs, device, progress, float(eta), self._descending(start_step), known, keep, known_noise)

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0,
                         start_step=None, known=None, keep=None, known_noise=None):
        """gaussian_diffusion.py:618-649; the trailing keywords as in ddim_sample_loop_progressive."""
        final = None
        for final in self.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                       denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                       model_kwargs=model_kwargs, device=device,
                                                       progress=progress, eta=eta, start_step=start_step,
                                                       known=known, keep=keep, known_noise=known_noise):
            pass
        return final["sample"]

    def dpm_solver_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                           cond_fn=None, model_kwargs=None, device=None, progress=False, order=2,
                                           lower_order_final=2, start_step=None, known=None, keep=None, known_noise=None):
        """DPM-Solver++(2M) generator over the DDIM loop's steps (no counterpart in the reference; the module docstring has the
        method): each step yields {"sample", "pred_xstart"} and is the fused DDIM step under `dpm_solver_coefficients(order,
        lower_order_final, first step of the loop)`, handed the previous step's pred_xstart where its k is non-zero.  Deterministic:
        nothing is drawn and there is no eta.  `order = 1` is `ddim_sample_loop_progressive(eta=0)` bit for bit.  `start_step`,
        `known` / `keep` / `known_noise` as in ddim_sample_loop_progressive; the first step of a partial loop has no history and is
        the DDIM step.  A yielded `pred_xstart` is the next step's history (held by reference): do not write into it."""
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order!r}")
        if int(lower_order_final) < 1:
            raise ValueError(f"lower_order_final must be at least 1, got {lower_order_final!r}")
        return self._loop("dpm", model, shape, noise, clip_denoised, denoised_fn, cond_fn, model_kwargs, device, progress, 0.0,
                          self._descending(start_step), known, keep, known_noise, solver=(int(order), int(lower_order_final)))

    def dpm_solver_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                               model_kwargs=None, device=None, progress=False, order=2, lower_order_final=2,
                               start_step=None, known=None, keep=None, known_noise=None):
        """The final sample of dpm_solver_sample_loop_progressive."""
        final = None
        for final in self.dpm_solver_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                             denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                             model_kwargs=model_kwargs, device=device, progress=progress,
                                                             order=order, lower_order_final=lower_order_final,
                                                             start_step=start_step, known=known, keep=keep,
                                                             known_noise=known_noise):
            pass
        return final["sample"]

    def ddim_reverse_sample_loop_progressive(self, model, x, clip_denoised=True, model_kwargs=None, device=None,
                                             progress=False, start_step=0, stop_step=None):
        """The DDIM ODE run towards noise (no counterpart loop in the reference): `x` is level `start_step`; steps
        start_step .. stop_step - 1 ascending, each yielding {"sample", "pred_xstart"}; the last sample is level `stop_step`.
        stop_step defaults to n - 1, the level ddim_sample_loop accepts as `noise`; n is allowed (alphas_cumprod_next = 0 there)."""
        n = self.num_timesteps
        stop_step = n - 1 if stop_step is None else int(stop_step)
        start_step = int(start_step)
        if not (0 <= start_step < stop_step <= n):
            raise ValueError(f"need 0 <= start_step < stop_step <= {n}, got start_step = {start_step}, stop_step = {stop_step}")
        return self._loop("reverse", model, tuple(x.shape), x, clip_denoised, None, None, model_kwargs, device, progress, 0.0,
                          range(start_step, stop_step))

    def ddim_reverse_sample_loop(self, model, x, clip_denoised=True, model_kwargs=None, device=None, progress=False,
                                 start_step=0, stop_step=None):
        """Level `stop_step` of ddim_reverse_sample_loop_progressive."""
        final = None
        for final in self.ddim_reverse_sample_loop_progressive(model, x, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                                               device=device, progress=progress, start_step=start_step,
                                                               stop_step=stop_step):
            pass
        return final["sample"]

    def _single(self, kind, model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, eta):
        if denoised_fn is not None or cond_fn is not None:
            raise NotImplementedError("denoised_fn / cond_fn hooks are outside the accelerated path")
        step = self._one_step_of(t, x.shape[0])
        if x.device.type != "cuda":
            raise RuntimeError("the sampler runs on a HIP device only (there is no CPU arithmetic path); "
                               f"got a tensor on {x.device}")
        coef, tmap = self._device_state(x.device, eta)
        with torch.no_grad():
            return self._step(kind, model, x.float().contiguous(), step, clip_denoised=clip_denoised,
                              model_kwargs=model_kwargs, eta=eta, coef=coef, tmap=tmap)

    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None,
                    model_kwargs=None, eta=0.0):
        """One DDIM step at spaced timestep ``t`` (gaussian_diffusion.py:531-578)."""
        return self._single("ddim", model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, float(eta))

    def ddim_reverse_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None,
                            model_kwargs=None, eta=0.0):
        """One step of the DDIM ODE towards noise: level ``t`` -> level ``t + 1`` (gaussian_diffusion.py:580-616)."""
        assert eta == 0.0, "Reverse ODE only for deterministic path"
        return self._single("reverse", model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, 0.0)

    def _one_step_of(self, t: torch.Tensor, B: int) -> int:
        if tuple(t.shape) != (B,):
            raise AssertionError("t must have shape (B,)")
        steps = torch.unique(t).tolist()
        if len(steps) != 1:
            raise NotImplementedError("one fused step handles a single timestep per batch")
        if not (0 <= int(steps[0]) < self.num_timesteps):
            raise ValueError(f"t must lie in 0 .. {self.num_timesteps - 1}, got {int(steps[0])}")
        return int(steps[0])

    def q_sample(self, x_start, t, noise=None):
        """Diffuse clean data to level ``t``: sample from q(x_t | x_0) (gaussian_diffusion.py:216-231).  ``t``: (B,) device
        tensor holding one value, as the other single-step APIs require."""
        from .. import ops
        if x_start.device.type != "cuda":
            raise RuntimeError("the sampler runs on a HIP device only (there is no CPU arithmetic path); "
                               f"got a tensor on {x_start.device}")
        if noise is None:
            noise = torch.randn_like(x_start)
        assert noise.shape == x_start.shape
        step = self._one_step_of(t, x_start.shape[0])
        coef, _ = self._device_state(x_start.device, 0.0)
        with ops.device_of(x_start):
            return ops.q_sample(x_start.float().contiguous(), noise.to(x_start.device, torch.float32).contiguous(), coef, step)

    def p_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None):
        """One ancestral step (gaussian_diffusion.py:394-435)."""
        return self._single("ancestral", model, x, t, clip_denoised, denoised_fn, cond_fn, model_kwargs, 0.0)


class SpacedDiffusion(GaussianDiffusion):
    """A process that keeps only ``use_timesteps`` of a base process (respace.py:65-114)."""

    def __init__(self, use_timesteps, **kwargs):
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(kwargs["betas"])
        base = DiffusionTables(kwargs["betas"])
        new_betas, self.timestep_map = respaced_betas(base.alphas_cumprod, self.use_timesteps)
        kwargs["betas"] = new_betas
        super().__init__(**kwargs)

    def _timestep_ids(self):
        return self.timestep_map

    def _scale_timesteps(self, t):
        return t


def create_diffusion(timestep_respacing, noise_schedule="linear", use_kl=False, sigma_small=False,
                     parameterization="eps", learn_sigma=True, rescale_learned_sigmas=False,
                     diffusion_steps=1000) -> SpacedDiffusion:
    """Factory with the reference's signature (models/diffusion/__init__.py:10-52)."""
    from .schedule import get_named_beta_schedule, space_timesteps

    betas = get_named_beta_schedule(noise_schedule, diffusion_steps)
    if use_kl:
        loss_type = LossType.RESCALED_KL
    elif rescale_learned_sigmas:
        loss_type = LossType.RESCALED_MSE
    else:
        loss_type = LossType.MSE
    if timestep_respacing is None or timestep_respacing == "":
        timestep_respacing = [diffusion_steps]
    try:
        mean_type = {"eps": ModelMeanType.EPSILON, "xstart": ModelMeanType.START_X,
                     "v": ModelMeanType.VELOCITY}[parameterization]
    except KeyError:
        raise NotImplementedError("Model Mean Type {} is not supported!".format(parameterization)) from None
    if learn_sigma:
        var_type = ModelVarType.LEARNED_RANGE
    else:
        var_type = ModelVarType.FIXED_SMALL if sigma_small else ModelVarType.FIXED_LARGE
    return SpacedDiffusion(
        use_timesteps=space_timesteps(diffusion_steps, timestep_respacing),
        betas=betas, model_mean_type=mean_type, model_var_type=var_type, loss_type=loss_type,
    )
