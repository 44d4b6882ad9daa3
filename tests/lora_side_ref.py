"""Host reference for the factored LoRA gradient (plain module: tests/test_lora_side_ref.py checks it on the CPU,
tests/test_hip_lora_side_kernel.py and tests/test_hip_lora_side_train_step.py hold the HIP kernel to it).  Everything is torch
on the tensors' own device.

The gradient -- the bound
-------------------------
csrc/lora_side_grad.hip computes, from the backward operands of a linear y = x W^T (x [M, K], dy [M, N], bf16, M = B * R rows),
bf16 factors up [N, r] / down [r, K] and an fp32 scale s,

    T = x down^T  [M, r]      U = dy up  [M, r]                                   (stage 1, fp32)
    d_up  [n, j] = s * sum_m dy[m, n] * (T_hi + T_lo)[m, j]                       (stage 2)
    d_down[j, k] = s * sum_m (U_hi + U_lo)[m, j] * x[m, k]

on the bf16 MFMA with fp32 accumulation; hi = bf16(t), lo = bf16(t - hi).  Against ref = s * dy^T (x down^T) and
s * (dy up)^T x in fp64 (the bf16 values and the fp32 scale are the truth), with u = 2^-24:

  * stage 1 is the sum lora_grad_ref.py bounds: exact products, L_pad of them (L = K in steps of 32 for T, L = N in steps of 64
    for U) added in some order, the two spare u for second-order terms:
        |t - T| <= e1 = (L_pad + 2) * u * sum |.| |.|            (magT = |x| |down|^T, magU = |dy| |up|)
  * the split: t - hi is exact in fp32 (hi keeps t's leading 8 bits, the rest fits 16), so
        |t - hi - lo| <= 2^-9 |t - hi| <= 2^-18 |t| <= 2^-18 (|T| + e1);     eT = e1 + 2^-18 (|T| + e1)
    and |hi| + |lo| <= (1 + 2^-9) (1 + 2^-9) |t| <= (1 + 2^-7) (|T| + e1) =: A;
  * stage 2 sums the 2 M_pad exact products dy * hi, dy * lo (M_pad = 64 ceil(M / 64); steps, hi before lo and the partials
    of a split reduction ascending -- ANY order is a binary tree with 2 M_pad leaves), then s rounds once; as above
        (2 M_pad + 2) * u * |s| * sum_m |dy| A
  * all of it carried to an output element:

    |d_up - ref|   <= |s| * ( |dy|^T eT + (2 M_pad + 2) u |dy|^T A_T )
    |d_down - ref| <= |s| * ( eU^T |x| + (2 M_pad + 2) u A_U^T |x| )

Nothing in it comes from the kernel's output.  accumulate = 1 adds one more rounding of the sum old + new:
bound + 2^-24 (|old| + |ref| + bound).  Exact cases (integers in [-4, 4], a power-of-two scale): exact when every partial sum
is an integer below 2^24 AND |T|, |U| stay below 2^16, so that hi (8 leading bits) + lo (the remaining <= 8) is t itself;
`exact_grads` asserts both from the magnitudes.
"""
import torch

U32 = 2.0 ** -24
SPLIT = 2.0 ** -18
BF16 = torch.bfloat16
T_STEP, U_STEP, M_STEP = 32, 64, 64          # csrc/lora_side_grad.hip: LS_T_STEP, LS_U_STEP, LS_M_STEP

# (B, R, N, K, r) of tests/test_hip_lora_side_kernel.py.  csrc/lora_side_grad.hip's header: M = 65 second stage-1 strip and
# second stage-2 step, K = 33 / N = 65 second stage-1 step, N = 129 / K = 129 second stage-2 strip, r = 33 second pair of rank
# tiles -- all crossed by the ragged (1, 65, 131, 136, 33); M = 129 splits the m reduction of both roles into two chunks.
# The launcher picks the kernels' rank tile by rank_pad / 32 = ceil(r / 32) in 1 .. 4 (RT = 2, 4, 6, 8): r = 65, 80 and 96 are the
# first rank, an ordinary rank and the last rank of the third tile -- ragged everywhere; batched with both stage-2 reductions
# split (M = 140); with a second chunk (M = 129).  tests/test_lora_side_ref.py holds the list to all four tiles.
RANK_TILE, MAX_RANK = 32, 128
SHAPES = [(1, 1, 1, 8, 1), (1, 64, 16, 32, 32), (1, 65, 131, 136, 33), (1, 129, 16, 8, 8), (3, 43, 9, 20, 4), (2, 96, 128, 64, 128),
          (1, 65, 131, 136, 65), (2, 70, 72, 40, 80), (1, 129, 136, 72, 96)]
PRODUCTION = (1, 2560, 3072, 3072, 16)


def f32(x):
    """A Python float rounded to fp32 (what the ABI's ``float scale`` holds)."""
    return float(torch.tensor(x, dtype=torch.float32))


def pad(L, step):
    return step * ((L + step - 1) // step)


def rows64(t):
    """A [B, R, C] or [R, C] view as fp64 [M, C]."""
    return t.reshape(-1, t.shape[-1]).to(torch.float64)


def grads64(x, dy, up, down, s):
    """(d_up [N, r], d_down [r, K]) in fp64."""
    s = f32(s)
    X, Y, u, d = rows64(x), rows64(dy), up.to(torch.float64), down.to(torch.float64)
    return s * (Y.T @ (X @ d.T)), s * ((Y @ u).T @ X)


def bounds(x, dy, up, down, s):
    """(ref_up, bound_up), (ref_down, bound_down)."""
    s = f32(s)
    X, Y, u, d = rows64(x), rows64(dy), up.to(torch.float64), down.to(torch.float64)
    M, K = X.shape
    N = Y.shape[1]
    aX, aY = X.abs(), Y.abs()
    T, U = X @ d.T, Y @ u
    e1T = (pad(K, T_STEP) + 2) * U32 * (aX @ d.abs().T)
    e1U = (pad(N, U_STEP) + 2) * U32 * (aY @ u.abs())
    eT, eU = e1T + SPLIT * (T.abs() + e1T), e1U + SPLIT * (U.abs() + e1U)
    AT, AU = (1 + 2.0 ** -7) * (T.abs() + e1T), (1 + 2.0 ** -7) * (U.abs() + e1U)
    c2 = (2 * pad(M, M_STEP) + 2) * U32
    b_up = abs(s) * (aY.T @ eT + c2 * (aY.T @ AT))
    b_down = abs(s) * (eU.T @ aX + c2 * (AU.T @ aX))
    return (s * (Y.T @ T), b_up), (s * (U.T @ X), b_down)


def split(t):
    """fp32 t -> (hi, lo) as fp32 values of bf16 numbers."""
    hi = t.to(BF16).to(torch.float32)
    return hi, (t - hi).to(BF16).to(torch.float32)


def emulate(x, dy, up, down, s, mistake=None):
    """The kernel's arithmetic in fp32 with ONE of the orders it may use (every reduction index ascending, hi before lo): fp32
    results.  ``mistake``: one of the wrong kernels tests/test_lora_side_ref.py must see outside the bound."""
    X, Y = x.reshape(-1, x.shape[-1]).to(torch.float32), dy.reshape(-1, dy.shape[-1]).to(torch.float32)
    u, d = up.to(torch.float32), down.to(torch.float32)
    if mistake == "up untransposed":
        u = u.T.contiguous()
    M, K = X.shape
    N, r = Y.shape[1], d.shape[0]
    T = torch.zeros(M, r, dtype=torch.float32, device=X.device)
    for k in range(K):
        T += X[:, k:k + 1] * d[:, k].unsqueeze(0)             # exact products, one rounding per addition
    U = torch.zeros(M, r, dtype=torch.float32, device=X.device)
    for n in range(N):
        U += Y[:, n:n + 1] * u[n].unsqueeze(0)
    (Th, Tl), (Uh, Ul) = split(T), split(U)
    if mistake == "lo dropped":
        Tl, Ul = torch.zeros_like(Tl), torch.zeros_like(Ul)
    du = torch.zeros(N, r, dtype=torch.float32, device=X.device)
    dd = torch.zeros(r, K, dtype=torch.float32, device=X.device)
    rows = range(M_STEP, M) if mistake == "a chunk dropped" else range(M)
    for m in rows:
        du += Y[m].unsqueeze(1) * Th[m].unsqueeze(0)
        du += Y[m].unsqueeze(1) * Tl[m].unsqueeze(0)
        dd += Uh[m].unsqueeze(1) * X[m].unsqueeze(0)
        dd += Ul[m].unsqueeze(1) * X[m].unsqueeze(0)
    sc = torch.tensor(f32(s), dtype=torch.float32, device=X.device)
    if mistake == "scale twice":
        return sc * (sc * du), sc * (sc * dd)
    if mistake == "scale missing":
        return du, dd
    return sc * du, sc * dd


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (an element with bound 0 must be exact)."""
    err = (got.to(torch.float64) - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


def ratios(d_up, d_down, x, dy, up, down, s, old=None):
    """Worst |out - ref| / bound of both outputs.  ``old`` = (old_up, old_down): the outputs were ADDED to these
    (accumulate = 1) -- ref = old + s * sum, bound + 2^-24 (|old| + |ref| + bound)."""
    (ru, bu), (rd, bd) = bounds(x, dy, up, down, s)
    if old is not None:
        ou, od = old[0].to(torch.float64), old[1].to(torch.float64)
        bu, bd = bu + U32 * (ou.abs() + ru.abs() + bu), bd + U32 * (od.abs() + rd.abs() + bd)
        ru, rd = ou + ru, od + rd
    return worst_ratio(d_up, ru, bu), worst_ratio(d_down, rd, bd)


def check(name, d_up, d_down, x, dy, up, down, s, old=None):
    a, b = ratios(d_up, d_down, x, dy, up, down, s, old)
    print(f"[parity] lora_side_grad {name}: x={tuple(x.shape)} dy={tuple(dy.shape)} r={up.shape[1]} observed/bound d_up={a:.3g} "
          f"d_down={b:.3g}", flush=True)
    assert a <= 1.0 and b <= 1.0, f"{name}: the worst element is {a:.3f} (d_up) / {b:.3f} (d_down) x the derived bound"
    return a, b


def data(B, R, N, K, r, seed, device="cpu"):
    """(x, dy, up, down, s): x ~ N(0, 1) (a normalised activation), dy ~ 0.02 N(0, 1) (a gradient), up / down ~ 0.3 N(0, 1),
    s = 0.75; x and dy contiguous [B, R, *]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, R, K, generator=g).to(BF16).to(device)
    dy = (0.02 * torch.randn(B, R, N, generator=g)).to(BF16).to(device)
    up = (0.3 * torch.randn(N, r, generator=g)).to(BF16).to(device)
    down = (0.3 * torch.randn(r, K, generator=g)).to(BF16).to(device)
    return x, dy, up, down, 0.75


def exact_data(B, R, N, K, r, seed, device="cpu"):
    """Integer-valued operands in [-4, 4] and a power-of-two scale (see the module docstring for when the result is exact)."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape: torch.randint(-4, 5, shape, generator=g).float().to(BF16).to(device)  # noqa: E731
    return mk(B, R, K), mk(B, R, N), mk(N, r), mk(r, K), (-0.25 if seed % 2 else 2.0)


def exact_grads(x, dy, up, down, s):
    """The fp32 results of an `exact_data` case; asserts the condition under which any summation order gives them."""
    X, Y, u, d = rows64(x), rows64(dy), up.to(torch.float64), down.to(torch.float64)
    magT, magU = X.abs() @ d.abs().T, Y.abs() @ u.abs()
    assert float(magT.max()) < 2 ** 16 and float(magU.max()) < 2 ** 16, "not an exact case: hi + lo would round T / U"
    assert float((Y.abs().T @ magT).max()) < 2 ** 24 and float((magU.T @ X.abs()).max()) < 2 ** 24, "not an exact case: a partial sum >= 2^24"
    ru, rd = grads64(x, dy, up, down, s)
    fu, fd = ru.to(torch.float32), rd.to(torch.float32)
    assert torch.equal(fu.to(torch.float64), ru) and torch.equal(fd.to(torch.float64), rd), "not an exact case"
    return fu, fd
