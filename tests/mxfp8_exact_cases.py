"""Exact MXFP8 operands with scales spread over the E8M0 range, for tests/test_hip_mxfp8_exact.py; built on the CPU so that the
reference side is checked without a GPU (tests/test_mxfp8_exact_host.py).  Codes and scale bytes are written directly: nothing
here goes through a quantizer.

exact_case
  Elements are the e4m3 codes of the integers -15 .. 15 (-8 .. 8 for K > 4096), taken from `mxfp8_ref._encode_mag`: all exact in
  e4m3, all three mantissa bits in use.  Every k-block b has one exponent e_b of [-96, 96], shared by all rows of both operands;
  every (row, block) adds u (A side) or v (W side) of {0, 1, 2}:  A's scale byte is 127 + e_b + u, W's is 127 - e_b + v.  A
  product term is then (integer) * 2^(u + v), of magnitude <= 225 * 16 = 3600, whatever e_b is -- and a block whose scale byte
  comes from another block, row or operand is off by 2^(e_b - e_b'), up to 2^+-192, instead of a factor a tolerance hides.
  e_b is uniform, except that one block of every case is pinned to -96 or +96: a case of four blocks spans the range too
  (scale bytes from <= 33 to >= 223).
  Exactness: the builder asserts (|a| @ |w|^T).max() + |bias|.max() < 2^24 in units of the smallest term (1, or 2^-shift with
  `act_shift`), on the dequantized fp64 arrays.  That bounds every partial sum in any order of summation, so each one is an
  integer multiple of the unit below 2^24: exact in fp32.  It holds by construction: 3600 K <= 3600 * 4096 < 2^24 with +-15 and
  (64 * 16) K <= 1024 * 6400 < 2^24 with +-8.  `want` is the fp64 product of `mxfp8_ref.dequantize` of both operands.
  narrow = True sets every e_b = 0 (scale bytes 127 .. 129): a kernel that is right there and wrong at the wide range has a
  scale problem, not a summation problem.
  act_shift = True lowers every W scale byte by one constant so that |want + bias| <= 8 (for GELU): a power of two, still exact.

all_codes_case
  K = 256.  W[n, k] is code k (the two NaN codes 0x7f / 0xff replaced by 0), A[m, k] is the code of 1.0 where k == m % 256 and 0
  elsewhere, A's scale bytes are 127, W's vary per (n, block) over 127 +- 40.  y[m, n] = decode(code m % 256) * 2^(s - 127): every
  finite e4m3 code -- subnormals, -0, +-448 -- reaches an accumulator alone, so the sum is exact without a range argument.
"""
import numpy as np

import mxfp8_ref as ref

BLOCK = 32
E_MAX = 96            # |e_b| <= E_MAX
SUB = 3               # u, v in [0, SUB)
ONE = 0x38            # e4m3 code of 1.0


def int_codes(lim):
    """(codes uint8 [2 lim + 1], values int64 [2 lim + 1]) of the integers -lim .. lim, from the reference's encoder."""
    vals = np.arange(-lim, lim + 1, dtype=np.int64)
    codes = ref._encode_mag(np.abs(vals).astype(np.float64)) | ((vals < 0).astype(np.uint8) << 7)
    assert np.array_equal(ref.e4m3_decode(codes), vals.astype(np.float64)), "an integer of the table is not exact in e4m3"
    return codes.astype(np.uint8), vals


def elem_limit(K):
    return 15 if K <= 4096 else 8


def _operand(rows, K, lim, rng):
    """(codes uint8 [rows, K], integer values int64 [rows, K], sub-exponents int64 [rows, K / 32] of {0, 1, 2})."""
    codes, vals = int_codes(lim)
    idx = rng.integers(0, 2 * lim + 1, size=(rows, K))
    return codes[idx], vals[idx], rng.integers(0, SUB, size=(rows, K // BLOCK))


def exact_case(M, N, K, seed=0, narrow=False, act_shift=False):
    """dict(a=(codes, scales), w=(codes, scales), bias float64 [N] (integers of [-4, 4]), want float64 [M, N] (no bias),
    unit (the power of two every term is a multiple of), and the integer parts ai, wi, u, v, e, shift for an independent check)."""
    assert K % 128 == 0 and K <= 6400
    rng = np.random.default_rng([seed, M, N, K, int(narrow), int(act_shift)])
    nb = K // BLOCK
    lim = elem_limit(K)
    aq, ai, u = _operand(M, K, lim, rng)
    wq, wi, v = _operand(N, K, lim, rng)
    e = rng.integers(-E_MAX, E_MAX + 1, size=nb)
    e[rng.integers(0, nb)] = E_MAX * (1 - 2 * rng.integers(0, 2))          # one block at an end of the range
    if narrow:
        e[:] = 0
    bias = rng.integers(-4, 5, size=N).astype(np.float64)
    asc = 127 + e[None, :] + u
    wsc = 127 - e[None, :] + v
    shift = 0
    if act_shift:
        y0 = ref.dequantize(aq, asc) @ ref.dequantize(wq, wsc).T
        shift = max(0, int(np.ceil(np.log2(max(np.abs(y0).max(), 1.0) / 4.0))))   # |y0| 2^-shift <= 4, so |y + bias| <= 8
        wsc = wsc - shift
    assert asc.min() >= 1 and asc.max() <= 254 and wsc.min() >= 1 and wsc.max() <= 254
    a, w = (aq, asc.astype(np.uint8)), (wq, wsc.astype(np.uint8))
    da, dw = ref.dequantize(*a), ref.dequantize(*w)
    unit = 2.0 ** -shift
    assert (np.abs(da) @ np.abs(dw).T).max() + np.abs(bias).max() < 2 ** 24 * unit, "partial sums may round in fp32"
    want = da @ dw.T
    if act_shift:
        assert np.abs(want + bias).max() <= 8
    return dict(a=a, w=w, bias=bias, want=want, unit=unit, ai=ai, wi=wi, u=u, v=v, e=e, shift=shift)


def all_codes_case(M, N, seed=0):
    """dict(a, w, want) with K = 256 and want[m, n] = decode(code m % 256) * 2^(W scale byte of (n, (m % 256) / 32) - 127)."""
    K = 256
    rng = np.random.default_rng([seed, M, N])
    k = np.arange(K)
    wrow = np.where((k & 0x7f) == 0x7f, 0, k).astype(np.uint8)
    wq = np.broadcast_to(wrow, (N, K)).copy()
    aq = np.zeros((M, K), dtype=np.uint8)
    aq[np.arange(M), np.arange(M) % K] = ONE
    asc = np.full((M, K // BLOCK), 127, dtype=np.uint8)
    wsc = (127 + rng.integers(-40, 41, size=(N, K // BLOCK))).astype(np.uint8)
    assert ((aq != 0).sum(1) == 1).all()                       # one term per output: nothing to sum
    want = ref.dequantize(aq, asc) @ ref.dequantize(wq, wsc).T
    return dict(a=(aq, asc), w=(wq, wsc), want=want)
