"""Host reference for the LoRA merge kernel (plain module: tests/test_lora_ref.py checks it on the CPU,
tests/test_hip_lora_kernel.py holds the HIP kernel to it).  Everything is torch on the tensors' own device.

The merge -- the bound
----------------------
csrc/lora_merge.hip computes, per element of a bf16 weight [N, K] and terms t = 0 .. T - 1 (up_t [N, r_t], down_t [r_t, K],
fp32 scale s_t),

    acc_t = sum_j up_t[n, j] * down_t[j, k]      r_pad_t = 32 * ceil(r_t / 32) products on the bf16 MFMA, fp32 accumulation
    v_0   = float(base);   v_{t+1} = fma(s_t, acc_t, v_t)                                      one fp32 rounding per term
    out   = bf16_rne(v_T)

against ref = base + sum_t s_t * sum_j up * down in fp64 (the bf16 values and the fp32 scales are the truth).  With
u = 2^-24 and mag = |base| + sum_t |s_t| sum_j |up| |down|:

  * a product of two bf16 numbers has 16 significant bits: exact in fp32.  Summing r_pad of them in ANY order (the MFMA's is
    not documented; the padding adds exact zeros) puts at most r_pad - 1 correctly rounded additions on a product's path:
    first order (r_pad - 1) * u * sum_j |up| |down| per term, r_pad the largest of the call;
  * the T fmas round once each, every partial sum bounded by mag (first order): T * u * mag.  Together E <= (r_pad - 1 + T) u mag;
  * the bf16 rounding of v_T moves it by at most half an ulp, 2^-8 * 2^e with 2^e <= |v_T| (8 significant bits), and
    |v_T| <= |ref| + E: at most 2^-8 |ref| + 2^-8 E;
  * the bound counts r_pad + T + 1 instead of r_pad - 1 + T: the two spare u * mag hold the second-order terms of E
    ((1 + u)^132 - 1 - 132 u ~ 1e-12 u) and the cross term 2^-8 E <= 2^-8 * 132 u mag ~ 0.52 u mag.

    |out - ref| <= 2^-8 |ref| + (r_pad + T + 1) * u * mag

Nothing in it comes from the kernel's output.  The exact cases (integer up / down in [-4, 4], power-of-two scales, base a
multiple of 2^-4 with |base| <= 8) need no bound: every partial sum is a multiple of 2^-4 below 2^14, an fp32 number, so the
kernel's v_T is the exact sum whatever the order and its bf16 rounding is the only one.
"""
import torch

U32 = 2.0 ** -24
BF16 = torch.bfloat16

# (N, K, r) of tests/test_hip_lora_kernel.py.  The kernel walks r_pad = 32 * ceil(r / 32) in trips of 32, 1 .. 4 of them; the last
# two shapes are the first and the last rank that take three (tests/test_lora_ref.py holds the list to all four trip counts).
RANK_TILE, MAX_RANK = 32, 128
SHAPES = [(1, 8, 1), (16, 32, 32), (63, 72, 5), (65, 136, 33), (128, 64, 128), (64, 3072, 16), (3072, 64, 16),
          (3072, 12288, 64), (65, 136, 65), (128, 64, 96)]
MIXED_RANKS = (5, 32, 33, 128)
MIXED_RANKS_96 = (96, 5, 80, 33)        # three trips first, then one, three again, two


def r_pad(rank):
    return 32 * ((rank + 31) // 32)


def f32(x):
    """A Python float rounded to fp32 (what the ABI's ``float scale`` holds)."""
    return float(torch.tensor(x, dtype=torch.float32))


def effective_scale(weight, call_scale, alpha, rank):
    """The scale of a term as the model forms it: weight x call scale x alpha / r (host doubles, then one fp32 rounding)."""
    return f32(weight * call_scale * alpha / rank)


def merge64(base, terms):
    """(ref, mag) in fp64: ref = base + sum_t s_t up_t down_t, mag = |base| + sum_t |s_t| |up_t| |down_t|."""
    ref = base.to(torch.float64)
    mag = ref.abs()
    for up, down, s in terms:
        s = f32(s)
        u64, d64 = up.to(torch.float64), down.to(torch.float64)
        ref = ref + s * (u64 @ d64)
        mag = mag + abs(s) * (u64.abs() @ d64.abs())
    return ref, mag


def bound(ref, mag, terms):
    rp = max(r_pad(up.shape[1]) for up, _, _ in terms)
    return 2.0 ** -8 * ref.abs() + (rp + len(terms) + 1) * U32 * mag


def emulate(base, terms):
    """The kernel's arithmetic in fp32 with ONE of the orders the MFMA may use (j ascending): bf16 result."""
    v = base.to(torch.float32)
    for up, down, s in terms:
        uf, df = up.to(torch.float32), down.to(torch.float32)
        acc = torch.zeros_like(v)
        for j in range(uf.shape[1]):
            acc += uf[:, j:j + 1] * df[j:j + 1, :]          # the product is exact in fp32, the addition rounds
        # fma(s, acc, v): the fp64 product of two fp32 numbers is exact; one rounding to fp32 (the double rounding through fp64
        # moves a result by far less than u)
        v = (f32(s) * acc.to(torch.float64) + v.to(torch.float64)).to(torch.float32)
    return v.to(BF16)


def worst_ratio(got, base, terms):
    """max over the elements of |got - ref| / bound (bound > 0 wherever mag > 0; an element with bound 0 must be exact)."""
    ref, mag = merge64(base, terms)
    b = bound(ref, mag, terms)
    err = (got.to(torch.float64) - ref).abs()
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max())


def check(name, got, base, terms):
    r = worst_ratio(got, base, terms)
    N, K = base.shape
    print(f"[parity] lora_merge {name}: N={N} K={K} ranks={[t[0].shape[1] for t in terms]} observed/bound={r:.4f}", flush=True)
    assert r <= 1.0, f"{name}: the worst element is {r:.3f} x the derived bound"
    return r


def data(N, K, ranks, seed, device="cpu", scales=None):
    """(base, terms): base ~ 0.05 N(0, 1) (a weight), up / down ~ 0.3 N(0, 1), scales alternating in sign around 0.5 -- each
    term moves an element by a few hundredths, a few bf16 ulps of the weight."""
    g = torch.Generator().manual_seed(seed)
    base = (0.05 * torch.randn(N, K, generator=g)).to(BF16).to(device)
    terms = []
    for i, r in enumerate(ranks):
        up = (0.3 * torch.randn(N, r, generator=g)).to(BF16).to(device)
        down = (0.3 * torch.randn(r, K, generator=g)).to(BF16).to(device)
        s = scales[i] if scales is not None else (0.5 + 0.125 * i) * (-1.0 if i % 2 else 1.0)
        terms.append((up, down, s))
    return base, terms


def exact_data(N, K, ranks, seed, device="cpu"):
    """Integer-valued up / down in [-4, 4], scales +-2^e (e in -2 .. 1), base a multiple of 2^-4 with |base| <= 8."""
    g = torch.Generator().manual_seed(seed)
    base = (torch.randint(-128, 129, (N, K), generator=g).float() / 16).to(BF16).to(device)
    terms = []
    for i, r in enumerate(ranks):
        up = torch.randint(-4, 5, (N, r), generator=g).float().to(BF16).to(device)
        down = torch.randint(-4, 5, (r, K), generator=g).float().to(BF16).to(device)
        terms.append((up, down, (2.0 ** ((i % 4) - 2)) * (-1.0 if i % 2 else 1.0)))
    return base, terms


def exact_merge(base, terms):
    """The bf16 result of an `exact_data` case: the fp64 sum is an fp32 number, its bf16 rounding the only rounding."""
    ref, _ = merge64(base, terms)
    f = ref.to(torch.float32)
    assert torch.equal(f.to(torch.float64), ref), "not an exact case: the sum does not fit fp32"
    return f.to(BF16)
