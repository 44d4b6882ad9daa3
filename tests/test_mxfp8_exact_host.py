"""CPU checks of the reference side of tests/test_hip_mxfp8_exact.py: the builder's exactness asserts hold at every shape the
GPU file uses, the scale bytes span the E8M0 range they claim, `want` equals integer arithmetic that never forms a scale, and
`all_codes_case` delivers every finite e4m3 code."""
import numpy as np
import pytest
import torch

import mxfp8_exact_cases as cases
import mxfp8_ref as ref
import test_hip_mxfp8_exact as gpu

CASES = gpu.host_cases()


def test_integer_codes_come_from_the_reference_encoder():
    for lim in (8, 15):
        codes, vals = cases.int_codes(lim)
        assert np.array_equal(ref.e4m3_decode(codes), vals) and len(set(codes.tolist())) == 2 * lim + 1
    assert {int(c) & 7 for c in cases.int_codes(15)[0]} == set(range(8)), "not every mantissa pattern is in use"
    assert cases.elem_limit(4096) == 15 and cases.elem_limit(6144) == 8 and cases.ONE == int(ref._encode_mag(np.array([1.0]))[0])


def test_the_gpu_file_stays_within_the_stated_shapes():
    for M, N, K, _, _ in CASES:
        assert M <= 2100 and N <= 768 and (K <= 1152 or (K in (6144, 6400) and M <= 300 and N <= 512))
    assert {K // 128 for K in gpu.SWEEP_KS} == {1, 2, 3, 4, 9}
    assert max(gpu.RANDOM_SHAPE) <= 1152 and gpu.C_RANDOM <= gpu.RANDOM_SHAPE[2]


@pytest.mark.parametrize("M,N,K,narrow,act_shift", CASES)
def test_exact_case_is_exact_wide_and_equal_to_integer_arithmetic(M, N, K, narrow, act_shift):
    c = cases.exact_case(M, N, K, narrow=narrow, act_shift=act_shift)          # the builder's own asserts run here
    (aq, asc), (wq, wsc) = c["a"], c["w"]
    assert aq.shape == (M, K) and wq.shape == (N, K) and asc.shape == (M, K // 32) and wsc.shape == (N, K // 32)
    assert aq.dtype == asc.dtype == wq.dtype == wsc.dtype == np.uint8
    assert not ((aq & 0x7f) == 0x7f).any() and not ((wq & 0x7f) == 0x7f).any() and asc.max() < 0xff and wsc.max() < 0xff
    lo, hi = min(asc.min(), wsc.min()), max(asc.max(), int(wsc.max()) + c["shift"])       # act_shift moves all of W's down
    if narrow:
        assert 127 <= asc.min() and asc.max() <= 129 and 127 <= wsc.min() and wsc.max() <= 129
    else:
        assert lo <= 40 and hi >= 214, f"scale bytes span only [{lo}, {hi}]"
    # integer arithmetic: e_b cancels between the operands, what is left is (ai 2^u) (wi 2^v) in units of 2^-shift
    assert np.array_equal(asc.astype(np.int64), 127 + c["e"][None] + c["u"])
    assert np.array_equal(wsc.astype(np.int64), 127 - c["e"][None] + c["v"] - c["shift"])
    assert np.array_equal(ref.e4m3_decode(aq), c["ai"]) and np.array_equal(ref.e4m3_decode(wq), c["wi"])
    ia = torch.from_numpy(c["ai"] << np.repeat(c["u"], 32, axis=1))
    iw = torch.from_numpy(c["wi"] << np.repeat(c["v"], 32, axis=1))
    total = (ia @ iw.T).numpy()
    assert np.abs(total).max() < 2 ** 24
    assert np.array_equal(c["want"] * 2.0 ** c["shift"], total.astype(np.float64))
    assert c["want"].dtype == np.float64 and np.array_equal(c["want"].astype(np.float32).astype(np.float64), c["want"])
    assert set(np.unique(c["bias"])) <= set(range(-4, 5))
    if act_shift:
        assert np.abs(c["want"] + c["bias"]).max() <= 8 and c["shift"] > 0


@pytest.mark.parametrize("M", gpu.CODES_MS)
def test_all_codes_case_reproduces_the_decoder(M):
    N = gpu.CODES_N
    c = cases.all_codes_case(M, N)
    (aq, asc), (wq, wsc) = c["a"], c["w"]
    finite = [k for k in range(256) if (k & 0x7f) != 0x7f]
    assert len(finite) == 254 and all((wq[:, k] == k).all() for k in finite) and (wq[:, [0x7f, 0xff]] == 0).all()
    assert (asc == 127).all() and wsc.min() >= 87 and wsc.max() <= 167 and len(np.unique(wsc)) > 40
    dec = ref.e4m3_decode(np.arange(256))
    dec[[0x7f, 0xff]] = 0.0
    m = np.arange(M) % 256
    want = dec[m][:, None] * np.ldexp(1.0, wsc.astype(np.int64) - 127)[:, m // 32].T
    assert np.array_equal(c["want"], want)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    assert set(m.tolist()) >= set(finite)                       # every finite code, subnormals, -0 and +-448 among them
    assert 448.0 in dec and -448.0 in dec and 2.0 ** -9 in dec and np.signbit(dec[0x80]) and dec[0x80] == 0
