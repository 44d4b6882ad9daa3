"""CPU reference for the exact GEMM tests (tests/test_hip_gemm_small.py; checked by tests/test_gemm_small_ref.py).

The data are small integers in bf16 (or integers times a power of two), so the fp64 product `y = a @ w^T + bias` is the
value every fp32 accumulator of a kernel holds, in any summation order.  Each helper below restates the ROUNDING POINTS of
one epilogue of `gemm_bf16_kernel` (csrc/gemm_bf16.hip; the large-tile kernels' shared epilogue, csrc/gemm_epilogue.h, has
the same ones) with plain torch ops on that exact y, so the comparison with a kernel is equality -- except for the two
activations, whose hardware exp2 / rcp leave room for one bf16 step at a rounding boundary.

Nothing here needs a GPU.  The comparison functions (`check_guarded`, `check_ulp`) are the ones the GPU tests call.
"""
import math

import torch

from conftest import bf16_ulp_diff

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
SENTINEL = -24832.0               # a bf16 (and fp32) value no expected output takes; `expected` asserts that
GUARD_ROWS, GUARD_COLS = 3, 8     # columns: a multiple of 8 keeps C's row starts 16-byte aligned (so ldc != N)


def ints(shape, lo, hi, seed):
    """Uniform integers of [lo, hi] as bf16 (|v| <= 256 is exact in bf16)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(BF)


def _fp32_exact(y):
    return torch.equal(y.to(F32).to(F64), y)


def expected(a, w, bias=None, product=None):
    """fp64 `a @ w^T (+ bias)` over the flattened rows of `a`, as fp64.  Asserts what makes it THE value of an fp32
    accumulation in any order: |y| < 2^24 and y representable in fp32 (integers, or integers times a power of two); and
    that no value could be mistaken for untouched memory.  product: an earlier `expected(a, w)` of the same operands, so a
    large product is formed once."""
    y = a.to(F64).reshape(-1, a.shape[-1]) @ w.to(F64).T if product is None else product
    if bias is not None:
        y = y + bias.to(F64)
    assert y.abs().max().item() < 2 ** 24, "sums leave the range in which fp32 holds every integer"
    assert _fp32_exact(y), "y is not representable in fp32: partial sums may round"
    assert (y != SENTINEL).all(), "an expected value equals the sentinel"
    return y


def bf16_of(y):
    """bf16(y) for an fp32-representable fp64 y: ONE rounding (the step to fp32 is exact), to nearest even like the kernel."""
    assert _fp32_exact(y)
    return y.to(F32).to(BF)


def round_once_bf16(x):
    """fp64 -> bf16 with a single rounding.  torch converts through fp32 (two roundings); the nearest of that result and its
    two bf16 neighbours, measured in fp64, is the once-rounded value (a tie of the fp64 value itself keeps torch's choice)."""
    b = x.to(F32).to(BF)
    bits = b.contiguous().view(torch.int16).to(torch.int32)
    mono = torch.where(bits < 0, -(bits & 0x7FFF), bits)          # sign-magnitude -> a monotonic integer line

    def from_mono(m):
        raw = torch.where(m < 0, (-m) | 0x8000, m)
        raw = torch.where(raw >= 0x8000, raw - 0x10000, raw)
        return raw.to(torch.int16).view(BF)

    best, err = b, (b.to(F64) - x).abs()
    for step in (-1, 1):
        cand = from_mono(mono + step)
        e = (cand.to(F64) - x).abs()
        take = e < err
        best, err = torch.where(take, cand, best), torch.where(take, e, err)
    return best


# ---- bf16 output: one function per epilogue ---------------------------------------------------------------------------------

def epi_none(y):
    return bf16_of(y)


def alpha_f32(alpha):
    """The alpha the kernel multiplies by: fk_gemm_args.alpha is a C float."""
    return torch.tensor(float(alpha), dtype=F32)


def epi_scale(y, alpha):
    """bf16(fp32(y) * fp32(alpha)): one fp32 multiply of exact operands, then the store's rounding.  (The bias is not added.)"""
    assert _fp32_exact(y)
    p32 = y.to(F32) * alpha_f32(alpha)
    assert torch.equal(p32, (y * alpha_f32(alpha).to(F64)).to(F32)), "the fp32 multiply is not the once-rounded product"
    return p32.to(BF)


def epi_res(y, res):
    """bf16(float(bf16(y)) + res): y is parked as bf16 in the staging tile, the sum is formed in fp32 and rounded once."""
    return (bf16_of(y).to(F32) + res.reshape(y.shape).to(F32)).to(BF)


def gate_rows(gate, rows_per_batch, M):
    """[M, N]: row m takes the gate of batch m // rows_per_batch."""
    b = torch.arange(M) // rows_per_batch
    return gate[b]


def epi_gate_res(y, res, gate, rows_per_batch):
    """bf16(res + float(bf16(gate * float(bf16(y))))).  gate * bf16(y) has 16 significant bits: exact in fp32, so the inner
    rounding is of the exact product and the whole chain is determined."""
    g = gate_rows(gate, rows_per_batch, y.shape[0]).to(F32)
    prod = g * bf16_of(y).to(F32)
    assert torch.equal(prod.to(F64), g.to(F64) * bf16_of(y).to(F64)), "gate * bf16(y) is not exact in fp32"
    return (res.reshape(y.shape).to(F32) + prod.to(BF).to(F32)).to(BF)


def gelu_tanh64(x):
    """The tanh-form GELU, 0.5 x (1 + tanh u) with u = sqrt(2 / pi) (x + 0.044715 x^3), evaluated as x / (1 + exp(-2 u)) --
    the same function (0.5 (1 + tanh u) = sigmoid(2 u)) without the cancellation of 1 + tanh u: written with tanh, fp64
    itself returns -0 below x = -7 or so, where the value is about -1e-16 and a bf16 result has 8 good bits to compare."""
    u = math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)
    return x / (1.0 + torch.exp(-2.0 * u))


def epi_gelu(y):
    """fp64 gelu (tanh form) of float(bf16(y)), rounded once to bf16."""
    return round_once_bf16(gelu_tanh64(bf16_of(y).to(F64)))


def epi_silu(y):
    x = bf16_of(y).to(F64)
    return round_once_bf16(x / (1.0 + torch.exp(-x)))


# ---- fp32 output ------------------------------------------------------------------------------------------------------------

def f32_none(y, bias=None, res32=None):
    """fp32(y + bias) (+ res32): each fp32 add must be exact -- integers, or integers times a power of two -- which is
    asserted, so the kernel's two adds and this fp64 sum are the same number."""
    assert _fp32_exact(y)
    if bias is not None:
        y = y + bias.to(F64)
        assert _fp32_exact(y), "acc + bias rounds in fp32"
    if res32 is not None:
        y = y + res32.reshape(y.shape).to(F64)
        assert _fp32_exact(y), "+ res rounds in fp32"
    assert (y != SENTINEL).all()
    return y.to(F32)


def f32_scale(y, alpha):
    """fp32(y * alpha): the fp64 product of two fp32 values is exact, so its rounding is the fp32 multiply's."""
    assert _fp32_exact(y)
    out = (y * alpha_f32(alpha).to(F64)).to(F32)
    assert torch.equal(out, y.to(F32) * alpha_f32(alpha))
    return out


# ---- C inside a sentinel-filled buffer, and the comparison functions ----------------------------------------------------------

def guarded_shape(rows, N, dtype=BF):
    """Shape of the whole buffer around a [rows..., N] view and the index of the view: GUARD_ROWS rows before and after the
    last row axis, GUARD_COLS columns left and at least GUARD_COLS right (fp32: the row stride padded to 16 bytes, so the
    view starts 16-byte aligned for any N)."""
    rows = (rows,) if isinstance(rows, int) else tuple(rows)
    ld = N + 2 * GUARD_COLS
    if dtype == F32:
        ld = (ld + 3) // 4 * 4
    shape = (*rows[:-1], rows[-1] + 2 * GUARD_ROWS, ld)
    idx = (*[slice(None)] * (len(rows) - 1), slice(GUARD_ROWS, GUARD_ROWS + rows[-1]), slice(GUARD_COLS, GUARD_COLS + N))
    return shape, idx


def guarded(rows, N, dtype=BF, device="cpu"):
    """(whole buffer, index of C in it, the view C)."""
    shape, idx = guarded_shape(rows, N, dtype)
    buf = torch.full(shape, SENTINEL, dtype=dtype, device=device)
    return buf, idx, buf[idx]


def check_guarded(buf, idx, want, what):
    """Equality of buf[idx] with `want` and an untouched sentinel everywhere else.  (A `want` that lies on the device is
    compared there: the outputs of tens of millions of elements.)"""
    got = buf if want.is_cuda else buf.cpu()
    inner = got[idx]
    want = want.reshape(inner.shape)
    assert inner.dtype == want.dtype, f"{what}: dtype {inner.dtype} vs {want.dtype}"
    bad = inner != want
    if bad.any():
        where = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {inner.numel()} elements differ from the reference, first at "
                             f"{where}: got {inner[tuple(where)].item()} want {want[tuple(where)].item()}")
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[idx] = False
    assert (got[mask] == SENTINEL).all(), f"{what}: the guard band around C was written"


def check_ulp(buf, idx, want, what, max_ulp=1):
    """Every element of buf[idx] within `max_ulp` bf16 steps of `want` (none excluded), the guard band untouched.
    Returns (share of exact matches, largest distance)."""
    got = buf.cpu()
    inner = got[idx]
    want = want.reshape(inner.shape)
    assert not torch.isnan(inner.float()).any(), f"{what}: NaN"
    d = bf16_ulp_diff(inner, want)
    worst = int(d.max())
    exact = float((d == 0).float().mean())
    assert worst <= max_ulp, (f"{what}: {int((d > max_ulp).sum())} of {d.numel()} elements are more than {max_ulp} bf16 ulp "
                              f"from the reference (max {worst})")
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[idx] = False
    assert (got[mask] == SENTINEL).all(), f"{what}: the guard band around C was written"
    return exact, worst


# ---- deliberate mistakes of the kind a tiled kernel makes (the CPU tests plant them and expect the checks above to object) -----
# d: dict(a [B, rows, K], w, bias, res, gate, y = expected(a, w, bias)); finish: y -> the output a kernel would store.

def _drop_last_k_tile(d, finish):
    K = d["a"].shape[-1]
    return finish(expected(d["a"][..., :K - 64], d["w"][:, :K - 64], d["bias"]))


def _swap_rows(d, finish):
    out = finish(d["y"]).clone()
    out[[3, 77]] = out[[77, 3]]
    return out


def _shift_column_group(d, finish):
    out = finish(d["y"]).clone()
    out[:, 8:16] = finish(d["y"])[:, 16:24]
    return out


def _gate_of_the_tile(d, finish):
    """The rows of batch 1 that lie in the 128-row tile which began in batch 0 take batch 0's gate."""
    rows = d["a"].shape[1]
    right = finish(d["y"])
    wrong = epi_gate_res(d["y"], d["res"], d["gate"][[0] * d["gate"].shape[0]], rows)
    out = right.clone()
    out[rows:128] = wrong[rows:128]
    return out


MISTAKES = [_drop_last_k_tile, _swap_rows, _shift_column_group, _gate_of_the_tile]
