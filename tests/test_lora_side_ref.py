"""CPU checks of tests/lora_side_ref.py: the fp64 formulas are autograd's through the merged linear and lora_grad_ref's applied
to the fp64 weight gradient, an fp32 emulation of the kernel's arithmetic (hi / lo split included) stays inside the derived
bound at every small shape of the GPU file, integer cases are exact, and nine mistakes fall outside the bound."""
import pytest
import torch

import lora_grad_ref as G
import lora_side_ref as R


@pytest.mark.parametrize("B,R_,N,K,r", [(1, 6, 5, 8, 3), (2, 9, 33, 40, 7)])
def test_fp64_formulas_are_autograd_through_the_merged_linear(B, R_, N, K, r):
    g = torch.Generator().manual_seed(N)
    f64 = dict(generator=g, dtype=torch.float64)
    w0, x, dy = torch.randn(N, K, **f64), torch.randn(B, R_, K, **f64), torch.randn(B, R_, N, **f64)
    up = torch.randn(N, r, requires_grad=True, **f64)
    down = torch.randn(r, K, requires_grad=True, **f64)
    s = 0.375
    y = x @ (w0 + s * up @ down).T
    (y * dy).sum().backward()              # d loss / d y = dy
    ru, rd = R.grads64(x, dy, up.detach(), down.detach(), s)
    torch.testing.assert_close(ru, up.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rd, down.grad, rtol=1e-12, atol=1e-12)
    # the projection of the fp64 weight gradient dW = dy^T x (tests/lora_grad_ref.py) is the same pair
    dw = dy.reshape(-1, N).T @ x.reshape(-1, K)
    (pu, _), (pd, _) = G.grads64(dw, up.detach(), down.detach(), s)
    torch.testing.assert_close(ru, pu, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rd, pd, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("B,R_,N,K,r", R.SHAPES)
def test_fp32_emulation_is_inside_the_bound(B, R_, N, K, r):
    x, dy, up, down, s = R.data(B, R_, N, K, r, seed=B + R_ + N + K + r)
    du, dd = R.emulate(x, dy, up, down, s)
    R.check("emulation", du, dd, x, dy, up, down, s)


@pytest.mark.parametrize("B,R_,N,K,r", R.SHAPES)
def test_exact_cases_are_exact(B, R_, N, K, r):
    x, dy, up, down, s = R.exact_data(B, R_, N, K, r, seed=N + K)
    fu, fd = R.exact_grads(x, dy, up, down, s)
    du, dd = R.emulate(x, dy, up, down, s)
    assert torch.equal(du, fu) and torch.equal(dd, fd)


def test_shapes_reach_every_rank_tile():
    """The launcher instantiates one kernel per ceil(r / 32) in 1 .. 4: the GPU files' shape list must reach each of them, the
    first and the last rank of the tile that went unvisited longest (65, 96) by name."""
    ranks = [s[-1] for s in R.SHAPES]
    assert all(1 <= r <= R.MAX_RANK for r in ranks)
    assert {-(-r // R.RANK_TILE) for r in ranks} == set(range(1, R.MAX_RANK // R.RANK_TILE + 1)) == {1, 2, 3, 4}
    assert {65, 96} <= set(ranks)


def test_the_exact_condition_is_checked():
    x, dy, up, down, s = R.exact_data(1, 64, 8, 4096 + 64, 2, seed=0)
    x, down = x.abs().clamp_min(4), down.abs().clamp_min(4)          # |T| = 16 K >= 2^16
    with pytest.raises(AssertionError, match="not an exact case"):
        R.exact_grads(x, dy, up, down, s)


def mistake_data():
    """B = 2, R = 64 (two stage-2 steps), N = r = 16 (so that up^T has up's shape), K = 32; x a view whose batch stride is larger
    than R * ld.  All values positive in [0.5, 1.5): no cancellation, so that T and U are as large as their magnitude sums and
    a relative error of the intermediates is not hidden behind the stage-1 term of the bound."""
    B, R_, N, K, r = 2, 64, 16, 32, 16
    g = torch.Generator().manual_seed(5)
    u = lambda *shape: (0.5 + torch.rand(shape, generator=g)).to(R.BF16)  # noqa: E731
    xbuf = u(B, R_ + 32, K)                                               # batch stride (R + 32) * K
    return xbuf, xbuf[:, :R_], u(B, R_, N), u(N, r), u(r, K), 0.75


def test_nine_mistakes_fall_outside_the_bound():
    xbuf, x, dy, up, down, s = mistake_data()
    B, R_, K = x.shape
    good = R.emulate(x, dy, up, down, s)
    assert max(R.ratios(*good, x, dy, up, down, s)) <= 1.0
    both = lambda a, b: a > 1.0 and b > 1.0  # noqa: E731
    for name in ("lo dropped", "scale twice", "scale missing", "a chunk dropped", "up untransposed"):
        a, b = R.ratios(*R.emulate(x, dy, up, down, s, mistake=name), x, dy, up, down, s)
        # up enters d_up only through T's partner dy^T (.): the untransposed up spoils U, hence d_down
        assert (b > 1.0) if name == "up untransposed" else both(a, b), (name, a, b)
    # the second batch read at R * ld instead of its batch stride: rows [R, 2R) of the flat buffer
    x_wrong = torch.as_strided(xbuf, (B, R_, K), (R_ * K, K, 1))
    assert not torch.equal(x_wrong, x)
    a, b = R.ratios(*R.emulate(x_wrong, dy, up, down, s), x, dy, up, down, s)
    assert both(a, b), ("batch stride", a, b)
    # the flag: a correct accumulate is inside its bound, each confusion outside
    g = torch.Generator().manual_seed(6)
    old = (torch.rand(good[0].shape, generator=g), torch.rand(good[1].shape, generator=g))
    added = (old[0] + good[0], old[1] + good[1])
    assert max(R.ratios(*added, x, dy, up, down, s, old=old)) <= 1.0
    a, b = R.ratios(*good, x, dy, up, down, s, old=old)
    assert both(a, b), ("accumulate = 1 overwrote", a, b)
    a, b = R.ratios(*added, x, dy, up, down, s)
    assert both(a, b), ("accumulate = 0 added", a, b)


def test_the_bound_is_far_below_the_bf16_rounding_of_dw():
    """What the factored gradient gains: its bound relative to the gradient's magnitude sum is below the 2^-9 of a bf16 dW."""
    x, dy, up, down, s = R.data(1, 64, 16, 32, 32, seed=3)
    (_, bu), (_, bd) = R.bounds(x, dy, up, down, s)
    X, Y = R.rows64(x).abs(), R.rows64(dy).abs()
    mag_up = abs(s) * (Y.T @ (X @ down.double().abs().T))
    mag_dn = abs(s) * ((Y @ up.double().abs()).T @ X)
    assert float((bu / mag_up).max()) < 2.0 ** -12 and float((bd / mag_dn).max()) < 2.0 ** -12
