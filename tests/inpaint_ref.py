"""The masked-edit step restated in torch bf16 tensor ops, one rounding per op -- the reference both the host test
(which pins its identities on the CPU) and the GPU tests (which hold the HIP kernels and the pipeline to it at 0 ulp) use.
Runs on any device: torch evaluates a bf16 tensor op in fp32 and rounds once, on the CPU and on the GPU alike."""
import torch

BF = torch.bfloat16


def bf_scalar(v, device="cpu"):
    """A host float32 scalar as the 0-dim bf16 tensor it becomes when it is multiplied into a bf16 tensor."""
    return torch.tensor(float(v), dtype=torch.float32, device=device).to(BF)


def euler(x, v, dsigma):
    return x + bf_scalar(dsigma, x.device) * v


def keep(x0, noise, sigma):
    sb = bf_scalar(sigma, x0.device)
    return sb * noise + (1 - sb) * x0


def expand_mask(m, C):
    """Compact [Bm, S, 4] -> [Bm, S, C]: element j of a token lies on sub-pixel j % 4."""
    return m.repeat(1, 1, C // 4)


def step(x, v, dsigma, sigma_next, x0, noise, m):
    """m: [1 or B, S, C] bf16 (already expanded).  Returns the new x."""
    p = euler(x, v, dsigma)
    k = keep(x0, noise, sigma_next)
    return (1 - m) * k + m * p
