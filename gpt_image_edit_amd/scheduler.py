"""FlowMatchEulerDiscreteScheduler as the reference pipeline drives it (host logic + one HIP kernel).

Interface used by ``univa/utils/flux_pipeline.py``: ``config.get(...)`` (:994-999),
``set_timesteps(sigmas=, mu=, device=)`` via ``retrieve_timesteps`` (:1000-1006), ``timesteps``,
``order``, ``set_begin_index(0)`` (:1052), ``step(noise_pred, t, latents, return_dict=False)[0]`` (:1099).
Masked edits and ``strength`` (diffusers' inpaint pipeline of this model family) add ``scale_noise`` and a begin index
other than 0.
The sigma schedule is host arithmetic in float32 (28 numbers); the update itself is
``fk_euler_step_bf16`` with the reference's rounding (bf16(dsigma) * v in bf16, sum in fp32 -> bf16).
``FlowMatchMultistepScheduler`` is the opt-in second-order (Adams-Bashforth 2) rule on the same schedule: ``fk_ab2_step_bf16``.
The pipeline's ``latent_state="fp32"`` runs either rule on a float32 state (``fk_solver_step_f32``) with this module's ``dsigma``
/ ``coefficients``; the ``step()`` methods here, the hand-driven out-of-place forms, stay bf16.
"""
import math

import numpy as np
import torch

from . import flux_spec, ops


class FlowMatchEulerDiscreteScheduler:
    order = 1

    def __init__(self, **config):
        self.config = dict(flux_spec.SCHEDULER_CONFIG)
        self.config.update(config)
        self.timesteps = None
        self.sigmas = None
        self._sigmas_host = None
        self._step_index = None
        self._begin_index = None

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index=0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps=None, device=None, sigmas=None, mu=None):
        cfg = self.config
        if cfg["use_dynamic_shifting"] and mu is None:
            raise ValueError(" you have a pass a value for `mu` when `use_dynamic_shifting` is set to be `True`")
        if sigmas is None:
            ts = np.linspace(cfg["num_train_timesteps"], 1, num_inference_steps)
            sigmas = ts / cfg["num_train_timesteps"]
        s = np.array(sigmas).astype(np.float32)
        if cfg["use_dynamic_shifting"]:
            s = math.exp(mu) / (math.exp(mu) + (1 / s - 1) ** 1.0)
        else:
            s = cfg["shift"] * s / (1 + (cfg["shift"] - 1) * s)
        s = np.asarray(s, dtype=np.float32)
        self.num_inference_steps = len(s)
        self._sigmas_host = np.concatenate([s, np.zeros(1, dtype=np.float32)])
        self.timesteps = torch.from_numpy(s * np.float32(cfg["num_train_timesteps"])).to(device=device)
        self.sigmas = torch.from_numpy(self._sigmas_host.copy()).to(device=device)
        self._step_index = None
        self._begin_index = None

    def dsigma(self, i):
        """sigma[i+1] - sigma[i] in float32, as the reference forms it on the device."""
        return float(np.float32(self._sigmas_host[i + 1]) - np.float32(self._sigmas_host[i]))

    def sigma_next(self, i):
        """sigma[i+1] in float32: the noise level after step i (0 after the last one), which the keep region of a masked
        edit is re-noised to."""
        return float(np.float32(self._sigmas_host[i + 1]))

    def index_for_timestep(self, timestep):
        idx = (self.timesteps.cpu() == float(timestep)).nonzero()
        return int(idx[1 if len(idx) > 1 else 0])

    def scale_noise(self, sample, timestep, noise):
        """sigma * noise + (1 - sigma) * sample at the sigma of ``timestep`` (looked up like ``_init_step_index`` does, or
        the begin index when one is set), in bf16 with one rounding per tensor op: ``fk_scale_noise_bf16``."""
        if sample.dtype != torch.bfloat16 or noise.dtype != torch.bfloat16:
            raise TypeError("the HIP scale_noise works on bf16 latents")
        i = self.index_for_timestep(timestep) if self._begin_index is None else self._begin_index
        return ops.scale_noise(sample.contiguous(), noise.contiguous(), float(self._sigmas_host[i]))

    def _init_step_index(self, timestep):
        if self._begin_index is None:
            self._step_index = self.index_for_timestep(timestep)
        else:
            self._step_index = self._begin_index

    def step(self, model_output, timestep, sample, return_dict=True, **unused):
        """x <- x.float() + (sigma_next - sigma) * v, cast to v.dtype (out of place, like the reference)."""
        if self._step_index is None:
            self._init_step_index(timestep)
        if model_output.dtype != torch.bfloat16 or sample.dtype != torch.bfloat16:
            raise TypeError("the HIP scheduler step works on bf16 latents")
        prev = sample.contiguous().clone()
        B, S, _ = prev.shape
        ops.euler_step(prev, model_output.contiguous(), S, self.dsigma(self._step_index))
        self._step_index += 1
        if not return_dict:
            return (prev,)
        return {"prev_sample": prev}


class FlowMatchMultistepScheduler(FlowMatchEulerDiscreteScheduler):
    """Second-order Adams-Bashforth rule on the parent's (non-uniform) sigma grid: one model call per step, the previous
    velocity as the only state.  With d_i = sigma[i+1] - sigma[i] and r = d_i / d_{i-1} the update is
    ``x + d_i (1 + r/2) v_i - d_i (r/2) v_{i-1}``; the first executed step (no history yet) and, with ``lower_order_final``,
    the last step of the schedule are first-order steps ``x + d_i v_i``.  The sum is formed in float32 with float32
    coefficients and rounded to bf16 once (``fk_ab2_step_bf16``) -- unlike the parent's step, which mirrors the reference's
    bf16 scheduler arithmetic.  Timesteps, sigmas, ``scale_noise`` and the begin index are the parent's."""
    order = 1               # model calls per step
    solver_order = 2

    def __init__(self, lower_order_final=True, **config):
        super().__init__(**config)
        self.lower_order_final = bool(lower_order_final)
        self._hist = None

    def set_timesteps(self, num_inference_steps=None, device=None, sigmas=None, mu=None):
        super().set_timesteps(num_inference_steps=num_inference_steps, device=device, sigmas=sigmas, mu=mu)
        self._hist = None
        if not (np.diff(self._sigmas_host.astype(np.float64)) < 0).all():     # a NaN fails this too
            self.timesteps = self.sigmas = self._sigmas_host = None
            raise ValueError("the multistep rule divides by the step size: the sigmas (with the final 0) must be strictly "
                             "decreasing")

    def coefficients(self, i, have_history):
        """(c_v, c_h, use_hist) of step ``i``: the float32 values ``fk_ab2_step_bf16`` receives, computed in float64 from the
        float32 sigmas.  ``have_history``: a velocity of step ``i - 1`` exists (False at the first executed step, which sits at
        the begin index when the loop starts inside the schedule; step 0 has no predecessor whatever is passed)."""
        s = self._sigmas_host.astype(np.float64)
        d = s[i + 1] - s[i]
        last = i == len(s) - 2
        if not have_history or i == 0 or (last and self.lower_order_final):
            return float(np.float32(d)), 0.0, 0
        r = d / (s[i] - s[i - 1])
        return float(np.float32(d * (1 + r / 2))), float(np.float32(-d * r / 2)), 1

    def step(self, model_output, timestep, sample, return_dict=True, **unused):
        """The rule out of place, for callers that drive the scheduler themselves; the history tensor is allocated at the
        first step of a run and dropped by ``set_timesteps``."""
        first = self._step_index is None
        if first:
            self._init_step_index(timestep)
        if model_output.dtype != torch.bfloat16 or sample.dtype != torch.bfloat16:
            raise TypeError("the HIP scheduler step works on bf16 latents")
        prev = sample.contiguous().clone()
        B, S, _ = prev.shape
        if first or self._hist is None or self._hist.shape != prev.shape or self._hist.device != prev.device:
            self._hist, first = torch.empty_like(prev), True
        c_v, c_h, use_hist = self.coefficients(self._step_index, not first)
        ops.ab2_step(prev, model_output.contiguous(), self._hist, S, c_v, c_h, use_hist)
        self._step_index += 1
        if not return_dict:
            return (prev,)
        return {"prev_sample": prev}
