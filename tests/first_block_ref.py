"""Host reference for the first-block measure kernel (plain module: tests/test_first_block_ref.py checks it on the CPU,
tests/test_hip_first_block_kernels.py holds ``ops.residual_absdiff_sums`` to it).

The kernel forms r = bf16(float(h1) - float(h0)) -- an exactly defined bf16 tensor, ``residual`` below -- and sums
|r - ref| and |ref| with csrc/step_cache.hip's decomposition and order.  So the truth is ``step_cache_ref.sums64(r, ref)`` and
the error bound ``step_cache_ref.bound(r, ref)``: the derivation in that module's docstring carries over unchanged (a term is
still one fp32 subtraction of two bf16 numbers and passes the same additions), and ``step_cache_ref.emulate(r, ref)`` is the
kernel's order.  Nothing here comes from a kernel's output.
"""
import torch

import step_cache_ref as R

BF = torch.bfloat16


def residual(h1, h0):
    """r = bf16(float(h1) - float(h0)): fk_residual_save_bf16's value."""
    return (h1.float() - h0.float()).to(BF)


def sums64(h1, h0, ref):
    return R.sums64(residual(h1, h0), ref)


def bound(h1, h0, ref):
    return R.bound(residual(h1, h0), ref)


def emulate(h1, h0, ref, **kw):
    return R.emulate(residual(h1, h0), ref, **kw)


def check(name, got, h1, h0, ref):
    return R.check(name, got, residual(h1, h0), ref)


def inside(got, h1, h0, ref):
    """Whether a pair of sums lies inside the derived bound of fp64 (both of them)."""
    s, b = sums64(h1, h0, ref), bound(h1, h0, ref)
    return all(abs(float(g) - t) <= e for g, t, e in zip(got, s, b))


def data(shape, seed, spread=0.05):
    """(h1, h0, ref) bf16, a fit model of a step: the stream h0 ~ N(0, 1) in front of block 0, what the block adds
    r ~ 0.5 N(0, 1), h1 = h0 + r, and the last computed step's residual ref = r + spread * 0.5 N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    h0 = torch.randn(shape, generator=g)
    r = 0.5 * torch.randn(shape, generator=g)
    ref = r + spread * 0.5 * torch.randn(shape, generator=g)
    return (h0 + r).to(BF), h0.to(BF), ref.to(BF)
