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

Out of scope (no caller on the inference path):
``training_losses``, VLB terms, ``cond_fn`` / ``denoised_fn`` hooks
(NotImplementedError when passed), RePaint-style resampling jumps, masked
ancestral sampling, differing timesteps within a batch.
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

    # ------------------------------------------------------------------ device state
    def _timestep_ids(self) -> Sequence[int]:
        """Values handed to the model for spaced step i (identity for an un-spaced process)."""
        return list(range(self.num_timesteps))

    def _device_state(self, device: torch.device, eta: float):
        key = (str(device), float(eta))
        st = self._dev_cache.get(key)
        if st is None:
            coef = torch.from_numpy(self.step_coefficients(eta)).to(device)
            tmap = torch.tensor(list(self._timestep_ids()), dtype=torch.int64, device=device)
            st = (coef, tmap)
            self._dev_cache = {key: st}  # keep only the latest (eta, device)
        return st

    # ------------------------------------------------------------------ one step
    def _step(self, kind: str, model: Callable, x: torch.Tensor, i: int, **kw):
        from .. import ops  # deferred: importing the sampler must not need the HIP library
        with ops.device_of(x):   # launches go to the current device's stream: make x's device current for the step
            return self._step_on_device(kind, model, x, i, **kw)

    def _step_on_device(self, kind: str, model: Callable, x: torch.Tensor, i: int, *, clip_denoised: bool,
                        model_kwargs: Optional[dict], eta: float, coef: torch.Tensor, tmap: torch.Tensor, planner=None,
                        row: Optional[int] = None, keep_args: Optional[dict] = None):
        """`row`: the planner's row of this step (its position in the announced sequence; None: the step index, the full
        loop's convention).  `keep_args`: known / known_noise / keep of a masked DDIM loop."""
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
              known_noise=None) -> Iterator[dict]:
        """Every sampling loop: the steps `indices` in order, each fed the previous one's sample.  None is the full descending loop
        n - 1 .. 0 on its own code path (the planner is handed every row and selects by step index)."""
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

        def step(x, i, row):
            with torch.no_grad():   # scoped to the step: a generator must not hold the grad-mode context across yields
                return self._step(kind, model, x, i, clip_denoised=clip_denoised, model_kwargs=model_kwargs, eta=eta, coef=coef,
                                  tmap=tmap, planner=planner, row=row, keep_args=keep_args)
        try:
            for pos, (i, row) in enumerate(shown):
                out = step(img, i, row)
                if pos == len(todo) - 1:
                    out = self._fold_guard(planner, out, img0, step, todo)     # BEFORE the final yield: consumers stop at the last item
                yield out
                img = out["sample"]
        finally:
            if planner is not None:
                planner.clear_timestep_plan()

    def _fold_guard(self, planner, out: dict, img0: torch.Tensor, step: Callable, todo: Sequence) -> dict:
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
        `step` carries the keep operands)."""
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
