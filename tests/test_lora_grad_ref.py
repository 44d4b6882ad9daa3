"""CPU checks of tests/lora_grad_ref.py: the fp64 formulas are autograd's through the merge, an fp32 emulation of the
kernel's arithmetic stays inside the derived bound at every shape of the GPU file, and five mistakes fall outside it."""
import pytest
import torch

import lora_grad_ref as R


@pytest.mark.parametrize("N,K,r", [(5, 8, 3), (33, 40, 7)])
def test_fp64_formulas_are_autograd_through_the_merge(N, K, r):
    g = torch.Generator().manual_seed(N)
    w0 = torch.randn(N, K, generator=g, dtype=torch.float64)
    up = torch.randn(N, r, generator=g, dtype=torch.float64, requires_grad=True)
    down = torch.randn(r, K, generator=g, dtype=torch.float64, requires_grad=True)
    dw = torch.randn(N, K, generator=g, dtype=torch.float64)
    s = 0.375
    w = w0 + s * up @ down
    (w * dw).sum().backward()              # d loss / d W = dw
    (ru, _), (rd, _) = R.grads64(dw, up.detach(), down.detach(), s)
    torch.testing.assert_close(ru, up.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(rd, down.grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_fp32_emulation_is_inside_the_bound(N, K, r):
    dw, up, down, s = R.data(N, K, r, seed=N + K + r)
    du, dd = R.emulate(dw, up, down, s)
    R.check("emulation", du, dd, dw, up, down, s)


def test_shapes_reach_every_rank_tile():
    """The launcher instantiates one kernel per ceil(r / 32) in 1 .. 4: the GPU files' shape list must reach each of them, the
    first and the last rank of the tile that went unvisited longest (65, 96) by name."""
    ranks = [s[-1] for s in R.SHAPES]
    assert all(1 <= r <= R.MAX_RANK for r in ranks)
    assert {-(-r // R.RANK_TILE) for r in ranks} == set(range(1, R.MAX_RANK // R.RANK_TILE + 1)) == {1, 2, 3, 4}
    assert {65, 96} <= set(ranks)


@pytest.mark.parametrize("N,K,r", R.SHAPES[:5] + R.SHAPES[-3:])
def test_exact_cases_are_exact(N, K, r):
    dw, up, down, s = R.exact_data(N, K, r, seed=N + K)
    fu, fd = R.exact_grads(dw, up, down, s)
    du, dd = R.emulate(dw, up, down, s)
    assert torch.equal(du, fu) and torch.equal(dd, fd)


def test_five_mistakes_fall_outside_the_bound():
    N = K = r = 128                          # square, so that every mistake below has the right shape
    dw, up, down, s = R.data(N, K, r, seed=9)
    w, u, d = dw.float(), up.float(), down.float()
    good = (s * (w @ d.T), s * (u.T @ w))
    assert max(R.ratios(*good, dw, up, down, s)) <= 1.0
    wrong = {
        "scale missing": (w @ d.T, u.T @ w),
        "up where down belongs": (s * (w @ u.T), s * (d @ w)),
        "a dropped 64-wide strip": (s * (w[:, 64:] @ d[:, 64:].T), s * (u[64:].T @ w[64:])),
        "transposed output": (good[0].T.contiguous(), good[1].T.contiguous()),
        "s applied twice": (s * good[0], s * good[1]),
    }
    for name, (du, dd) in wrong.items():
        a, b = R.ratios(du, dd, dw, up, down, s)
        assert a > 1.0 and b > 1.0, (name, a, b)
