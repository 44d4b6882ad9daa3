"""CPU: the host reference of the first-block measure (tests/first_block_ref.py).  The reference is step_cache_ref's, applied to
the exactly defined r = bf16(h1 - h0): an fp32 emulation of the kernel's order stays inside the derived bound, and each mistake
a kernel of this kind can make -- the difference the wrong way round, sum |r| as the denominator, ref compared with h1 instead of
r, a dropped row, a dropped last partial -- lies outside it for the data the GPU test uses."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import first_block_ref as F  # noqa: E402
import step_cache_ref as R  # noqa: E402

# (rows, D): one element, cut chunks, the model width, a padded width, one past the first grid-stride trip and 256 partials
SHAPES = [(1, 1), (3, 7), (2, 13), (10, 3075), (5, 3072), (R.ONE_TRIP_ITEMS // 8 + 700, 64)]


def test_the_reference_is_step_cache_refs_on_the_residual():
    h1, h0, ref = F.data((5, 67), seed=1)
    r = F.residual(h1, h0)
    assert r.dtype == torch.bfloat16 and torch.equal(r, (h1.float() - h0.float()).to(torch.bfloat16))
    assert F.sums64(h1, h0, ref) == R.sums64(r, ref) and F.bound(h1, h0, ref) == R.bound(r, ref)
    assert F.emulate(h1, h0, ref) == R.emulate(r, ref)
    assert F.sums64 is not R.sums64 and F.R is R          # imported, not copied


@pytest.mark.parametrize("M,D", SHAPES)
def test_emulation_stays_inside_the_bound(M, D):
    h1, h0, ref = F.data((M, D), seed=M + D)
    got = F.emulate(h1, h0, ref)
    r0, r1 = F.check(f"emulate {M}x{D}", got, h1, h0, ref)
    assert r0 <= 1.0 and r1 <= 1.0 and F.inside(got, h1, h0, ref)


@pytest.mark.parametrize("M,D", SHAPES[3:])
def test_each_mistake_leaves_the_bound(M, D):
    h1, h0, ref = F.data((M, D), seed=M + D)
    r = F.residual(h1, h0)
    assert F.inside(R.emulate(r, ref), h1, h0, ref)
    wrong = {
        "h0 - h1": R.emulate(F.residual(h0, h1), ref),
        "sum |r| as the denominator": (R.emulate(r, ref)[0], R.emulate(ref, r)[1]),
        "ref against h1": R.emulate(h1, ref),
        "a dropped row": R.emulate(r, ref, drop_row=M // 2),
        "a dropped last partial": R.emulate(r, ref, drop_last_partial=True),
    }
    for name, got in wrong.items():
        assert not F.inside(got, h1, h0, ref), name
        with pytest.raises(AssertionError, match="derived bound"):
            F.check(name, got, h1, h0, ref)


def test_exact_zeros():
    h1, h0, ref = F.data((5, 64), seed=3)
    assert F.emulate(h1, h1, torch.zeros_like(ref)) == (0.0, 0.0)
    assert F.emulate(h1, h0, torch.zeros_like(ref))[1] == 0.0
