"""The second-order multistep (Adams-Bashforth 2) step restated outside the package -- the reference both the CPU tests (which
pin its identities, its order and its rounding bound) and the GPU tests (which hold ``fk_ab2_step_bf16`` and the pipeline to it
at 0 ulp) use.

* ``coefficients``: the rule in float64 from the float32 sigmas, returned as the float32 values the kernel receives.
* ``step``: the op-by-op float32 torch expression, one rounding per op and one rounding to bf16 -- what the kernel computes.
* ``step64``: the same sum in float64, unrounded: what the expression is measured against.
* ``integrate`` / ``test_equation_error``: the scalar test equation dx/dsigma = 1.5 cos(3 sigma) x on the shifted schedule.
Runs on any device."""
import math

import numpy as np
import torch

import inpaint_ref

BF = torch.bfloat16


def schedule(n, s_tgt):
    """The pipeline's float32 sigmas for ``n`` steps at ``s_tgt`` target tokens: linspace(1, 1/n, n) shifted by
    mu = calculate_shift(s_tgt), with the final 0 appended (scheduler.py: set_timesteps, restated)."""
    from gpt_image_edit_amd import helpers
    mu = helpers.calculate_shift(s_tgt)
    s = np.linspace(1.0, 1 / n, n).astype(np.float32)
    s = np.asarray(math.exp(mu) / (math.exp(mu) + (1 / s - 1) ** 1.0), dtype=np.float32)
    return np.concatenate([s, np.zeros(1, dtype=np.float32)])


def coefficients64(sig, i, have_history, lower_order_final=True):
    """(c_v, c_h, use_hist) in float64.  d_i = sigma[i+1] - sigma[i], r = d_i / d_{i-1}:
    c_v = d_i (1 + r/2), c_h = -d_i r/2; first order (d_i, 0, 0) without history and, by default, at the last step."""
    s = np.asarray(sig, dtype=np.float32).astype(np.float64)
    d = s[i + 1] - s[i]
    if not have_history or i == 0 or (lower_order_final and i == len(s) - 2):
        return d, 0.0, 0
    r = d / (s[i] - s[i - 1])
    return d * (1 + r / 2), -d * r / 2, 1


def coefficients(sig, i, have_history, lower_order_final=True):
    c_v, c_h, use = coefficients64(sig, i, have_history, lower_order_final)
    return float(np.float32(c_v)), float(np.float32(c_h)), use


def f32_scalar(v, device="cpu"):
    return torch.tensor(float(v), dtype=torch.float32, device=device)


def update(x, v, h, c_v, c_h, use_hist):
    """bf16(x + c_v * v [+ c_h * h]): float32 tensor ops, each rounded once, the coefficients 0-dim float32 tensors."""
    s = x.float() + f32_scalar(c_v, x.device) * v.float()
    if use_hist:
        s = s + f32_scalar(c_h, x.device) * h.float()
    return s.to(BF)


def step(x, v, h, c_v, c_h, use_hist, sigma_next=0.0, x0=None, noise=None, m=None):
    """The new x.  ``m``: [1 or B, S, C] bf16 (already expanded) or None; the blend is ``inpaint_ref``'s with this update."""
    p = update(x, v, h, c_v, c_h, use_hist)
    if m is None:
        return p
    k = inpaint_ref.keep(x0, noise, sigma_next)
    return (1 - m) * k + m * p


def step64(x, v, h, c_v, c_h, use_hist):
    """The update's sum in float64 from the float32 coefficients, and the magnitude its rounding bound scales with."""
    x, v, h = x.double(), v.double(), h.double()
    cv, ch = float(np.float32(c_v)), float(np.float32(c_h)) if use_hist else 0.0
    return x + cv * v + ch * h, x.abs() + (cv * v).abs() + (ch * h).abs()


def rounding_bound(ref, mag):
    """One bf16 rounding of the result plus three float32 roundings (two products feed two sums; the products' own roundings
    are within the same 2^-24 of terms no larger than ``mag``)."""
    return 2.0 ** -8 * ref.abs() + 3 * 2.0 ** -24 * mag


# ---- the test equation ---------------------------------------------------------------------------------------------------------
def f_test(sigma, x):
    return 1.5 * math.cos(3 * sigma) * x


EXACT = math.exp(-0.5 * math.sin(3.0))        # x(0) of dx/dsigma = 1.5 cos(3 sigma) x, x(1) = 1


def integrate(sig, solver, lower_order_final=True):
    """x(sigma = 0) in float64 from x(1) = 1 along ``sig`` with 'euler' or 'ab2' (float64 coefficients: the rule, not its
    float32 storage)."""
    s = np.asarray(sig, dtype=np.float32).astype(np.float64)
    x, h = 1.0, None
    for i in range(len(s) - 1):
        v = f_test(s[i], x)
        if solver == "euler":
            x = x + (s[i + 1] - s[i]) * v
        else:
            c_v, c_h, use = coefficients64(sig, i, h is not None, lower_order_final)
            x = x + c_v * v + (c_h * h if use else 0.0)
        h = v
    return x


def test_equation_error(n, s_tgt, solver, lower_order_final=True):
    return abs(integrate(schedule(n, s_tgt), solver, lower_order_final) - EXACT)


test_equation_error.__test__ = False      # a helper, not a test
