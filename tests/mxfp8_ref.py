"""Pure numpy reference of the OCP MXFP8 (E4M3 elements, E8M0 block scales) quantizer of include/fk.h.

Independent of the kernel's bit tricks: every element is rounded to the nearest of the 127 positive e4m3fn magnitudes by a
table search, ties to the even code.  Used by tests/test_mxfp8_host.py and tests/test_hip_mxfp8.py.
"""
import numpy as np

BLOCK = 32


def e4m3_values():
    """Magnitudes of the e4m3fn codes 0 .. 126 (0x7f is NaN): exp field 0 = subnormal m * 2^-9, else (1 + m / 8) 2^(exp - 7)."""
    c = np.arange(127)
    e, m = c >> 3, c & 7
    return np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e - 7.0))


_VALS = e4m3_values()


def e4m3_decode(q):
    """uint8 codes -> float64 (NaN for 0x7f / 0xff)."""
    q = np.asarray(q, dtype=np.uint8)
    mag = np.concatenate([_VALS, [np.nan]])[q & 0x7f]
    return np.where(q & 0x80, -mag, mag)


def e8m0_decode(s):
    s = np.asarray(s, dtype=np.int64)
    return np.where(s == 0xff, np.nan, np.ldexp(1.0, (s - 127).clip(-127, 127)))


def _encode_mag(a):
    """float64 magnitudes in [0, 448] -> nearest e4m3 code, ties to even."""
    hi = np.searchsorted(_VALS, a, side="left").clip(0, 126)
    lo = (hi - 1).clip(0, 126)
    dlo, dhi = a - _VALS[lo], _VALS[hi] - a
    pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0))
    return np.where(pick_hi, hi, lo).astype(np.uint8)


def quantize(x):
    """x: float array [M, K] of bf16 values, K % 32 == 0 -> (q uint8 [M, K], scales uint8 [M, K / 32])."""
    x = np.asarray(x, dtype=np.float64)
    M, K = x.shape
    assert K % BLOCK == 0
    b = x.reshape(M, K // BLOCK, BLOCK)
    bad = ~np.isfinite(b).all(-1)
    bs = np.where(np.isfinite(b), b, 0.0)
    amax = np.abs(bs).max(-1)
    _, ex = np.frexp(amax)                       # amax = f 2^ex, f in [0.5, 1): floor(log2 amax) = ex - 1
    e = np.maximum(ex - 1 - 8, -127)
    sbyte = np.where(amax == 0, 127, e + 127)
    e = sbyte - 127
    v = np.ldexp(bs, -e[..., None])
    code = _encode_mag(np.minimum(np.abs(v), 448.0)) | (np.signbit(bs).astype(np.uint8) << 7)
    code = np.where(bad[..., None], np.uint8(0x7f), code)
    sbyte = np.where(bad, 0xff, sbyte)
    return code.reshape(M, K).astype(np.uint8), sbyte.astype(np.uint8)


def dequantize(q, s):
    """(q [M, K], scales [M, K / 32]) -> float64 [M, K]."""
    q, s = np.asarray(q), np.asarray(s)
    return e4m3_decode(q) * np.repeat(e8m0_decode(s), BLOCK, axis=1)
