"""CPU: the host reference of the step-cache sums (tests/step_cache_ref.py).  An fp32 emulation of the kernels' summation
order stays inside the bound derived from that order; an emulation that drops the last block's partial, or one row, does not."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_cache_ref as R  # noqa: E402

# (rows, D): one element, a cut chunk, a row of the model width, one past the first grid-stride trip and past 256 partials
SHAPES = [(1, 1), (63, 67), (65, 3080), (130, 3072), (R.ONE_TRIP_ITEMS // 8 + 700, 64)]


def test_layout_counts_the_stages():
    lay = R.layout(1, 1)
    assert (lay["N"], lay["nblk"], lay["iters"], lay["n_final"]) == (1, 1, 1, 9)
    lay = R.layout(R.ONE_TRIP_ITEMS // 8 + 700, 64)
    assert lay["nblk"] == R.MAX_BLOCKS and lay["iters"] == 2 and lay["nf"] == 4 and lay["n_serial"] == 5


@pytest.mark.parametrize("M,D", SHAPES)
def test_emulation_stays_inside_the_bound(M, D):
    a, b = R.data((M, D), seed=M + D)
    r0, r1 = R.check(f"emulate {M}x{D}", R.emulate(a, b), a, b)
    assert r0 <= 1.0 and r1 <= 1.0


@pytest.mark.parametrize("M,D", SHAPES[2:])
def test_a_dropped_partial_or_row_leaves_the_bound(M, D):
    a, b = R.data((M, D), seed=M + D)
    with pytest.raises(AssertionError, match="derived bound"):
        R.check("dropped partial", R.emulate(a, b, drop_last_partial=True), a, b)
    with pytest.raises(AssertionError, match="derived bound"):
        R.check("dropped row", R.emulate(a, b, drop_row=M // 2), a, b)


def test_exact_zeros():
    a, b = R.data((65, 64), seed=3)
    assert R.emulate(b, b)[0] == 0.0
    assert R.emulate(a, torch.zeros_like(b))[1] == 0.0
