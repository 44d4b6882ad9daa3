"""The denoise loop's step on a float32 latent state (``fk_solver_step_f32``) restated outside the package -- the reference of the
CPU tests (which pin its rounding bound, the mistakes that bound has to catch and what the float32 state buys on a test equation)
and of the GPU tests (which hold the kernel and the pipeline to it at 0 ulp).

* ``step``: the op-by-op float32 torch expression -- ``torch.mul`` then ``torch.add``, never ``addcmul`` -- on a float32 state.
* ``step64``: the same recurrence in float64 on the same bf16 inputs and the same float32 scalars, with the magnitudes the bound
  scales with.
* ``step_bound``: the rounding bound of one step, derived below; ``run64`` sums it over a run.
* ``ode_error``: ``solver_ref``'s test equation through the project's schedule with a bf16 model input and a bf16 velocity, the
  state in bf16 or in float32.
Runs on any device.

The bound.  u = 2^-24 is the relative error of one float32 rounding.  The unmasked step is
    p1 = fl(c_v * v);  s1 = fl(xs + p1);  p2 = fl(c_h * h);  s = fl(s1 + p2)
four roundings, each of a value no larger than mag = |xs| + |c_v v| + |c_h h| (to first order: |p1| + |p2| <= mag, |s1| <= mag,
|s| <= mag, so the sum of the four errors is even below 3 u mag); the state enters with gain 1.  Hence
    |s - s64| <= E + 4 u mag                       E: the error the state carried in.
The masked step adds  q1 = fl(sn * noise), q2 = fl(om * x0), k = fl(q1 + q2), w = fl(1 - m), a = fl(w * k), b = fl(m * s),
out = fl(a + b).  om is ONE float32 number formed on the host and shared with the float64 recurrence, and w is exact for every
bf16 m in {0} or [2^-17, 1] (1 - m then needs no more than 24 bits), which ``step_bound`` asserts.  With magk = |sn noise| + |om x0|
and M = (1 - m) magk + m mag:  k is off by at most u (|q1| + |q2| + |k|) <= 2 u magk, which the blend scales by (1 - m);  a adds
u (1 - m) |k| <= u (1 - m) magk, b adds u m |s| <= u m mag, and the sum adds u |out| <= u M: together at most 4 u M, below the
five roundings of size u M the bound allows for "k and the blend".  Hence
    |out - out64| <= m (E + 4 u mag) + 5 u M.
Second-order terms (products of two roundings, the magnitudes taken from the float64 run instead of the float32 one) are below
2^-20 of the bound; ``SLACK`` covers them."""
import math

import numpy as np
import torch

import inpaint_ref
import solver_ref

BF = torch.bfloat16
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20


def f32(v, device="cpu"):
    return torch.tensor(float(v), dtype=torch.float32, device=device)


def one_minus(sigma_next):
    """float32(1 - sigma_next), formed once on the host."""
    return float(np.float32(1.0) - np.float32(sigma_next))


def step(xs, v, h, c_v, c_h, use_hist, sigma_next=0.0, x0=None, noise=None, m=None):
    """The new float32 state from the float32 ``xs`` (``x.float()`` at a seeding step); the token rows are ``.to(bfloat16)`` of
    it.  ``v``, ``h``, ``x0``, ``noise``: bf16; ``m``: [1 or B, S, C] bf16 (already expanded) or None."""
    d = xs.device
    assert xs.dtype == torch.float32
    s = torch.add(xs, torch.mul(f32(c_v, d), v.float()))
    if use_hist:
        s = torch.add(s, torch.mul(f32(c_h, d), h.float()))
    if m is None:
        return s
    k = torch.add(torch.mul(f32(sigma_next, d), noise.float()), torch.mul(f32(one_minus(sigma_next), d), x0.float()))
    mf = m.float()
    return torch.add(torch.mul(torch.sub(f32(1.0, d), mf), k), torch.mul(mf, s))


def step64(xs, v, h, c_v, c_h, use_hist, sigma_next=0.0, x0=None, noise=None, m=None):
    """(out, mag, magk) in float64: the same expression, unrounded, from the float32 scalars the kernel receives."""
    cv, ch = float(np.float32(c_v)), float(np.float32(c_h)) if use_hist else 0.0
    xs, v = xs.double(), v.double()
    hh = h.double() if use_hist else torch.zeros_like(v)
    s = xs + cv * v + ch * hh
    mag = xs.abs() + (cv * v).abs() + (ch * hh).abs()
    if m is None:
        return s, mag, None
    sn, om = float(np.float32(sigma_next)), one_minus(sigma_next)
    k = sn * noise.double() + om * x0.double()
    magk = (sn * noise.double()).abs() + (om * x0.double()).abs()
    md = m.double()
    return (1 - md) * k + md * s, mag, magk


def step_bound(err_in, mag, magk=None, m=None):
    """The error bound of one step's state against ``step64`` (module docstring), from the bound ``err_in`` carried in."""
    if m is None:
        return (err_in + 4 * U * mag) * SLACK
    md = m.double()
    assert bool(((md == 0) | ((md >= 2.0 ** -17) & (md <= 1))).all()), "1 - m must be exact in float32"
    return (md * (err_in + 4 * U * mag) + 5 * U * ((1 - md) * magk + md * mag)) * SLACK


def run64(x, vs, coef, sigma_next=None, x0=None, noise=None, m=None):
    """The float64 recurrence over a run from the bf16 ``x`` with the velocities ``vs`` (bf16, one per step) and the per-step
    ``coef`` (c_v, c_h, use_hist): (final state in float64, the summed bound on a float32 run's state)."""
    ref, err, h = x.double(), torch.zeros_like(x, dtype=torch.float64), None
    for i, (v, c) in enumerate(zip(vs, coef)):
        sn = 0.0 if sigma_next is None else sigma_next[i]
        ref, mag, magk = step64(ref, v, h if c[2] else v, *c, sn, x0, noise, m)
        err = step_bound(err, mag, magk, m)
        h = v
    return ref, err


def run32(x, vs, coef, sigma_next=None, x0=None, noise=None, m=None, one_step=step):
    """The float32 run: the state seeded from the bf16 ``x`` (exact), ``one_step`` per step, the history the previous velocity."""
    s, h = x.float(), None
    for i, (v, c) in enumerate(zip(vs, coef)):
        sn = 0.0 if sigma_next is None else sigma_next[i]
        s = one_step(s, v, h, *c, sn, x0, noise, m)
        h = v
    return s


# ---- the test equation with a bf16 model input and a bf16 velocity ------------------------------------------------------------------
def ode_error(n, s_tgt, solver, state, x1):
    """RMS relative error at sigma = 0 of dx/dsigma = 1.5 cos(3 sigma) x (``solver_ref``) from the bf16 start values ``x1``, along
    the project's schedule.  Both arms evaluate the velocity on bf16(x) and round it to bf16.  ``state`` "fp32": this file's
    ``step`` on a float32 state, with the unrounded float32 step size for Euler.  ``state`` "bf16": the loop as it is today --
    ``inpaint_ref.euler`` (the reference's bf16 arithmetic) for Euler, ``solver_ref.update`` for AB2.  Returns (error of the carried
    state, error of its final bf16 rounding -- the returned latents); they coincide for the bf16 state."""
    sig = solver_ref.schedule(n, s_tgt)
    assert x1.dtype == BF
    x, h = (x1.float() if state == "fp32" else x1.clone()), None
    for i in range(n):
        xin = x.to(BF)                                                               # what the model reads
        v = (1.5 * math.cos(3.0 * float(sig[i])) * xin.double()).to(BF)              # what the model returns
        if solver == "euler":
            c = (float(np.float32(sig[i + 1]) - np.float32(sig[i])), 0.0, 0)
        else:
            c = solver_ref.coefficients(sig, i, i > 0)
        if state == "fp32":
            x = step(x, v, h, *c)
        elif solver == "euler":
            x = inpaint_ref.euler(x, v, c[0])
        else:
            x = solver_ref.update(x, v, h, *c)
        h = v
    exact = solver_ref.EXACT * x1.double()

    def rms(t):
        return float((((t.double() - exact) / exact) ** 2).mean().sqrt())
    return rms(x), rms(x.to(BF))
