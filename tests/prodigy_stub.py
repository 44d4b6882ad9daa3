"""Torch stand-ins (CPU) for ``ops.sumsq`` and the four Prodigy kernels, with the kernels' signatures and operation order (fp32
elements, fp64 scalars and sums): what the host tests monkeypatch into ``ops`` and the gloo tests hand to
``zero.ShardedAdamW(kernels=...)``.  ``calls`` records the order of the calls."""
import math

import numpy as np
import torch

SLOTS = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "dlr", "k", "skipped", "sum_dot", "sum_abs")
I = {n: i for i, n in enumerate(SLOTS)}
calls = []


def _f32(x):
    return float(np.float32(x))


def _beta3(betas, beta3):
    return _f32(math.sqrt(float(betas[1])) if beta3 is None else beta3)


def sumsq(tensors, out=None):
    tensors = [tensors] if isinstance(tensors, torch.Tensor) else list(tensors)
    calls.append(("sumsq", len(tensors)))
    return torch.stack([t.double().pow(2).sum() for t in tensors]).sum().reshape(1)


def prodigy_ws(device):
    return torch.empty(0, dtype=torch.float64, device=device)


def prodigy_init_state(d0=1e-6, device="cpu"):
    buf = torch.zeros(len(SLOTS), dtype=torch.float64)
    buf[0] = buf[1] = float(d0)
    return buf.to(device)


def prodigy_begin(state, lr=1.0, betas=(0.9, 0.99), beta3=None, use_bias_correction=True):
    calls.append(("begin",))
    b1, b2, k1 = _f32(betas[0]), _f32(betas[1]), state[I["k"]].item() + 1
    bc = math.sqrt(1.0 - b2 ** k1) / (1.0 - b1 ** k1) if use_bias_correction else 1.0
    state[I["dlr"]] = state[I["d"]].item() * float(lr) * bc
    state[I["d_numerator"]] *= _beta3(betas, beta3)
    state[I["sum_dot"]] = state[I["sum_abs"]] = state[I["skipped"]] = 0.0
    return state


def prodigy_moments(master, p0, grad, m, v, s, state, betas=(0.9, 0.99), beta3=None, weight_decay=0.0, d0=1e-6, decouple=True,
                    safeguard_warmup=True, grad_sumsq=None, max_grad_norm=1.0, grad_scale=1.0, ws=None):
    calls.append(("moments", master.numel()))
    F = torch.float32
    coef = torch.tensor(grad_scale, dtype=F)
    if grad_sumsq is not None:
        total = grad_sumsq[0].sqrt().to(F) * coef
        coef = torch.minimum(torch.tensor(max_grad_norm, dtype=F) / (total + 1e-6), torch.tensor(1.0, dtype=F)) * coef
    d, dlr = state[I["d"]].item(), state[I["dlr"]].item()
    b1, b2, b3 = _f32(betas[0]), _f32(betas[1]), _beta3(betas, beta3)
    cm, cv, cs = _f32(d * (1.0 - b1)), _f32(d * d * (1.0 - b2)), _f32((d / d0) * (d if safeguard_warmup else dlr))
    g = grad.to(F).reshape(master.shape) * coef
    if not decouple:
        g = g + _f32(weight_decay) * master
    state[I["sum_dot"]] += (g.double() * (p0 - master).double()).sum()
    m.copy_(b1 * m + cm * g)
    v.copy_(b2 * v + (cv * g) * g)
    s.copy_(b3 * s + cs * g)
    state[I["sum_abs"]] += s.double().abs().sum()
    return state


def prodigy_update_d(state, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
    calls.append(("update_d",))
    d = state[I["d"]].item()
    num = state[I["d_numerator"]].item() + (d / d0) * state[I["dlr"]].item() * state[I["sum_dot"]].item()
    den = state[I["sum_abs"]].item()
    state[I["d_numerator"]], state[I["d_denom"]] = num, den
    if den == 0.0:
        state[I["skipped"]] = 1.0
        return state
    d_hat = d_coef * num / den
    if d == d0:
        d = max(d, d_hat)
    d_max = max(state[I["d_max"]].item(), d_hat)
    state[I["d_hat"]], state[I["d_max"]], state[I["d"]] = d_hat, d_max, min(d_max, d * growth_rate)
    state[I["k"]] += 1.0
    return state


def prodigy_apply(master, m, v, state, eps=1e-8, weight_decay=0.0, decouple=True, param_bf16=None):
    calls.append(("apply", master.numel()))
    if state[I["skipped"]].item() != 0.0:
        return master
    dlr = state[I["dlr"]].item()
    p = master
    if decouple:
        p = p + p * _f32(-_f32(weight_decay) * dlr)
    p = p - _f32(dlr) * (m / (v.sqrt() + _f32(state[I["d"]].item() * _f32(eps))))
    master.copy_(p)
    if param_bf16 is not None:
        param_bf16.copy_(master.reshape(param_bf16.shape))
    return master


def prodigy_state(buf):
    out = dict(zip(SLOTS, buf.detach().cpu().tolist()))
    out["k"], out["skipped"] = int(out["k"]), bool(out["skipped"])
    return out


def install(monkeypatch, ops):
    for name in ("sumsq", "prodigy_ws", "prodigy_init_state", "prodigy_begin", "prodigy_moments", "prodigy_update_d", "prodigy_apply",
                 "prodigy_state"):
        monkeypatch.setattr(ops, name, globals()[name])
    del calls[:]
