"""CPU checks of tests/lora_grad_acc_ref.py: an fp32 emulation of the accumulating projection stays inside the derived bound at
every shape of the GPU file, integer cases are exact, and five mistakes of an accumulate flag fall outside it."""
import pytest
import torch

import lora_grad_acc_ref as A
import lora_grad_ref as R


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_fp32_emulation_is_inside_the_bound(N, K, r):
    dw, up, down, s = R.data(N, K, r, seed=N + K + r)
    ou, od = A.old_like(N, K, r, seed=N + K + r)
    du, dd = A.emulate(ou, od, dw, up, down, s)
    A.check("emulation", du, dd, ou, od, dw, up, down, s)
    # ... and with the multiply and the add contracted into one fma (the product unrounded: here in fp64, rounded once)
    pu, pd = R.emulate(dw, up, down, 1.0)
    sc = R.f32(s)
    fu, fd = (ou.double() + sc * pu.double()).float(), (od.double() + sc * pd.double()).float()
    A.check("emulation, fma", fu, fd, ou, od, dw, up, down, s)


@pytest.mark.parametrize("N,K,r", R.SHAPES[:5])
def test_exact_cases_are_exact(N, K, r):
    dw, up, down, s = R.exact_data(N, K, r, seed=N + K)
    ou, od = A.exact_old(N, K, r, seed=N + K)
    want_u, want_d = A.exact(ou, od, dw, up, down, s)
    du, dd = A.emulate(ou, od, dw, up, down, s)
    assert torch.equal(du, want_u) and torch.equal(dd, want_d)
    (ru, bu), (rd, bd) = A.bounds(ou, od, dw, up, down, s)
    assert torch.equal(ru, want_u.double()) and torch.equal(rd, want_d.double())


def test_five_mistakes_fall_outside_the_bound():
    N = K = r = 128                          # square, so that "the other output" has the right shape
    dw, up, down, s = R.data(N, K, r, seed=9)
    ou, od = A.old_like(N, K, r, seed=9)
    pu, pd = R.emulate(dw, up, down, s)
    good = (ou + pu, od + pd)
    assert max(A.ratios(*good, ou, od, dw, up, down, s)) <= 1.0
    sc = R.f32(s)
    both = {
        "the flag ignored": (pu, pd),
        "old added once per split": (2 * ou + pu, 2 * od + pd),
        "old scaled too": (sc * ou + pu, sc * od + pd),
        "old read from the other output": (od + pu, ou + pd),
    }
    for name, (du, dd) in both.items():
        a, b = A.ratios(du, dd, ou, od, dw, up, down, s)
        assert a > 1.0 and b > 1.0, (name, a, b)
    # only one of the two outputs accumulated: that output is inside, the other outside
    a, b = A.ratios(ou + pu, pd, ou, od, dw, up, down, s)
    assert a <= 1.0 < b, (a, b)
    a, b = A.ratios(pu, od + pd, ou, od, dw, up, down, s)
    assert b <= 1.0 < a, (a, b)
