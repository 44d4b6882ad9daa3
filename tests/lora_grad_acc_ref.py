"""Host reference for the ACCUMULATE form of the LoRA gradient projection (``fk_lora_grad_acc_bf16``, ``ops.lora_grad(...,
accumulate=True)``); extends tests/lora_grad_ref.py by import.  tests/test_lora_grad_acc_ref.py checks it on the CPU,
tests/test_hip_lora_grad_acc_kernel.py and tests/test_hip_lora_dp_train_step.py hold the HIP kernel to it.

The kernel forms ``out = old + scale * sum`` where it forms ``scale * sum`` in the overwrite form: ``old`` (fp32, whatever the
output held) is read once and added once.  Against ref = old + ref_projection in fp64 (``old``'s fp32 value is the truth):

  * the projection ``p = scale * sum`` is within ``bound_p = lora_grad_ref.bounds(...)`` of its fp64 value ``ref_p``;
  * the add rounds once more: u * |old + p| <= u * (|old| + |ref_p| + bound_p), u = 2^-24.  When the compiler contracts the
    multiply and the add into one fma the product is NOT rounded, which removes one u * |ref_p| that ``bound_p`` counts: the
    bound holds for both.

    |out - (old + ref_p)| <= bound_p + 2^-24 * (|old| + |ref_p| + bound_p)

Nothing in it comes from the kernel's output.  Exact cases: ``lora_grad_ref.exact_data`` with an integer ``old`` in [-64, 64] --
the projection is a multiple of 1/4 below 2^18 (an fp32 number, lora_grad_ref), old + it likewise: 0 ulp.
"""
import torch

import lora_grad_ref as R

U32 = R.U32


def old_like(N, K, r, seed, device="cpu"):
    """(old_up [N, r], old_down [r, K]) fp32 of the projection's own magnitude: the projection of other operands."""
    dw, up, down, s = R.data(N, K, r, seed=seed + 4099)
    (ru, _), (rd, _) = R.grads64(dw, up, down, s)
    return ru.to(torch.float32).to(device), rd.to(torch.float32).to(device)


def exact_old(N, K, r, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed + 4099)
    return (torch.randint(-64, 65, (N, r), generator=g).float().to(device), torch.randint(-64, 65, (r, K), generator=g).float().to(device))


def bounds(old_up, old_down, dw, up, down, s):
    """(ref_up, bound_up), (ref_down, bound_down) of one accumulating call onto (old_up, old_down)."""
    out = []
    for old, (ref, b) in zip((old_up, old_down), R.bounds(dw, up, down, s)):
        o = old.to(torch.float64)
        out.append((o + ref, b + U32 * (o.abs() + ref.abs() + b)))
    return tuple(out)


def emulate(old_up, old_down, dw, up, down, s):
    """``lora_grad_ref.emulate`` followed by the fp32 add."""
    du, dd = R.emulate(dw, up, down, s)
    return old_up + du, old_down + dd


def ratios(d_up, d_down, old_up, old_down, dw, up, down, s):
    (ru, bu), (rd, bd) = bounds(old_up, old_down, dw, up, down, s)
    return R.worst_ratio(d_up, ru, bu), R.worst_ratio(d_down, rd, bd)


def check(name, d_up, d_down, old_up, old_down, dw, up, down, s):
    a, b = ratios(d_up, d_down, old_up, old_down, dw, up, down, s)
    N, K = dw.shape
    print(f"[parity] lora_grad_acc {name}: N={N} K={K} r={up.shape[1]} observed/bound d_up={a:.4f} d_down={b:.4f}", flush=True)
    assert a <= 1.0 and b <= 1.0, f"{name}: the worst element is {a:.3f} (d_up) / {b:.3f} (d_down) x the derived bound"
    return a, b


def exact(old_up, old_down, dw, up, down, s):
    """The fp32 results of an exact case: old + the exact projection, itself an fp32 number."""
    fu, fd = R.exact_grads(dw, up, down, s)
    ru, rd = old_up.double() + fu.double(), old_down.double() + fd.double()
    assert torch.equal(ru.float().double(), ru) and torch.equal(rd.float().double(), rd), "not an exact case"
    return ru.float(), rd.float()
