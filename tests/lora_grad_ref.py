"""Host reference for the LoRA gradient projection (plain module: tests/test_lora_grad_ref.py checks it on the CPU,
tests/test_hip_lora_grad_kernel.py and tests/test_hip_lora_train_step.py hold the HIP kernel to it).  Everything is torch on
the tensors' own device.

The projection -- the bound
---------------------------
csrc/lora_grad.hip computes, from a bf16 weight gradient dW [N, K], bf16 factors up [N, r] / down [r, K] and an fp32 scale s,

    d_up  [n, j] = s * sum_k dW[n, k] * down[j, k]        L = K, walked in steps of 32 (UP_STEP)
    d_down[j, k] = s * sum_n up[n, j] * dW[n, k]          L = N, walked in steps of 64 (DN_STEP)

on the bf16 MFMA with fp32 accumulation, the reduction zero-padded to L_pad = step * ceil(L / step); where a reduction is
split over workgroups the fp32 partial sums are added in ascending order; s multiplies the finished sum once.  Against
ref = s * (the sum in fp64) (the bf16 values and the fp32 scale are the truth), with u = 2^-24 and
mag = |s| * sum |dW| * |factor|:

  * a product of two bf16 numbers has 16 significant bits: exact in fp32.  Summing L_pad of them in ANY order -- the MFMA's
    inside a step is not documented, steps and partials are added ascending, the padding adds exact zeros -- is a binary tree
    with L_pad leaves: at most L_pad - 1 correctly rounded additions lie on a product's path, every partial sum bounded by
    sum |dW| |factor| to first order: (L_pad - 1) * u * sum |dW| |factor|;
  * the multiplication by s rounds once more: u * |s| * |sum|;
  * the bound counts L_pad + 2 instead of L_pad: the two spare u * mag hold the second-order terms
    ((1 + u)^3073 - 1 - 3073 u ~ (3073 u)^2 / 2 ~ 0.3 u at the largest L_pad here, 3072).

    |out - ref| <= (L_pad + 2) * u * mag

Nothing in it comes from the kernel's output.  The exact cases (integer dW / up / down in [-4, 4], a power-of-two scale) need no
bound: every partial sum is an integer below 16 * 3072 < 2^24, an fp32 number, so the kernel's sum is exact in any order and the
scaling by a power of two is exact too: 0 ulp.
"""
import torch

U32 = 2.0 ** -24
BF16 = torch.bfloat16
UP_STEP, DN_STEP = 32, 64          # csrc/lora_grad.hip: LG_UP_STEP, LG_DN_STEP

# (N, K, r) of tests/test_hip_lora_grad_kernel.py.  The last two are the smallest shapes at which a reduction is split into two
# partials (csrc/lora_grad.hip's header: K = 257 second UP chunk, N = 129 second DOWN chunk), rounded up to K % 8 == 0 / a
# ragged N; N = 65 / K = 33 / K = 129 (second strips and steps) are crossed by (65, 136, 33).
# The launcher picks the kernel's rank tile by rank_pad / 32 = ceil(r / 32) in 1 .. 4 (RT = 2, 4, 6, 8): the last three are the
# first rank, an ordinary rank and the last rank of the third tile (tests/test_lora_grad_ref.py holds the list to all four).
RANK_TILE, MAX_RANK = 32, 128
SHAPES = [(1, 8, 1), (16, 32, 32), (63, 72, 5), (65, 136, 33), (128, 64, 128), (64, 3072, 16), (3072, 64, 16), (3072, 3072, 16),
          (16, 264, 8), (131, 16, 8), (65, 136, 65), (131, 72, 80), (128, 64, 96)]


def f32(x):
    """A Python float rounded to fp32 (what the ABI's ``float scale`` holds)."""
    return float(torch.tensor(x, dtype=torch.float32))


def pad(L, step):
    return step * ((L + step - 1) // step)


def grads64(dw, up, down, s):
    """((d_up, mag_up), (d_down, mag_down)) in fp64."""
    s = f32(s)
    w, u, d = dw.to(torch.float64), up.to(torch.float64), down.to(torch.float64)
    return (s * (w @ d.T), abs(s) * (w.abs() @ d.abs().T)), (s * (u.T @ w), abs(s) * (u.abs().T @ w.abs()))


def bounds(dw, up, down, s):
    """(ref_up, bound_up), (ref_down, bound_down)."""
    N, K = dw.shape
    (ru, mu), (rd, md) = grads64(dw, up, down, s)
    return (ru, (pad(K, UP_STEP) + 2) * U32 * mu), (rd, (pad(N, DN_STEP) + 2) * U32 * md)


def emulate(dw, up, down, s):
    """The kernel's arithmetic in fp32 with ONE of the orders it may use (the reduction index ascending): fp32 results."""
    w, u, d = dw.to(torch.float32), up.to(torch.float32), down.to(torch.float32)
    N, K = w.shape
    du = torch.zeros(N, u.shape[1], dtype=torch.float32, device=w.device)
    for k in range(K):
        du += w[:, k:k + 1] * d[:, k].unsqueeze(0)          # exact products, one rounding per addition
    dd = torch.zeros(u.shape[1], K, dtype=torch.float32, device=w.device)
    for n in range(N):
        dd += u[n].unsqueeze(1) * w[n:n + 1, :]
    sc = torch.tensor(f32(s), dtype=torch.float32, device=w.device)
    return sc * du, sc * dd


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (an element with bound 0 must be exact)."""
    err = (got.to(torch.float64) - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


def ratios(d_up, d_down, dw, up, down, s):
    (ru, bu), (rd, bd) = bounds(dw, up, down, s)
    return worst_ratio(d_up, ru, bu), worst_ratio(d_down, rd, bd)


def check(name, d_up, d_down, dw, up, down, s):
    a, b = ratios(d_up, d_down, dw, up, down, s)
    N, K = dw.shape
    print(f"[parity] lora_grad {name}: N={N} K={K} r={up.shape[1]} observed/bound d_up={a:.4f} d_down={b:.4f}", flush=True)
    assert a <= 1.0 and b <= 1.0, f"{name}: the worst element is {a:.3f} (d_up) / {b:.3f} (d_down) x the derived bound"
    return a, b


def data(N, K, r, seed, device="cpu"):
    """(dw, up, down, s): dw ~ 0.02 N(0, 1) (a gradient), up / down ~ 0.3 N(0, 1), s = 0.75."""
    g = torch.Generator().manual_seed(seed)
    dw = (0.02 * torch.randn(N, K, generator=g)).to(BF16).to(device)
    up = (0.3 * torch.randn(N, r, generator=g)).to(BF16).to(device)
    down = (0.3 * torch.randn(r, K, generator=g)).to(BF16).to(device)
    return dw, up, down, 0.75


def exact_data(N, K, r, seed, device="cpu"):
    """Integer-valued dw / up / down in [-4, 4] and a power-of-two scale: every partial sum is an exact fp32 integer."""
    g = torch.Generator().manual_seed(seed)
    dw = torch.randint(-4, 5, (N, K), generator=g).float().to(BF16).to(device)
    up = torch.randint(-4, 5, (N, r), generator=g).float().to(BF16).to(device)
    down = torch.randint(-4, 5, (r, K), generator=g).float().to(BF16).to(device)
    return dw, up, down, -0.25 if seed % 2 else 2.0


def exact_grads(dw, up, down, s):
    """The fp32 results of an `exact_data` case: the fp64 values are fp32 numbers."""
    (ru, _), (rd, _) = grads64(dw, up, down, s)
    fu, fd = ru.to(torch.float32), rd.to(torch.float32)
    assert torch.equal(fu.to(torch.float64), ru) and torch.equal(fd.to(torch.float64), rd), "not an exact case"
    return fu, fd
