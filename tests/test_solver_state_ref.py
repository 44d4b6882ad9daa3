"""CPU: the float32-state step's rounding bound (derived in ``solver_state_ref``, not fitted), the mistakes that bound -- or an
exact case whose value is known in closed form -- has to catch, and what the float32 state buys on ``solver_ref``'s test equation
when the model input and the velocity stay bf16."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as R  # noqa: E402
import solver_state_ref as S  # noqa: E402

BF = torch.bfloat16
SIG = R.schedule(28, 1024)
FIRST, N = 10, 6                        # steps 10 .. 15 of a 28-step schedule: a run that starts inside it, without history


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 50, 64, generator=g).to(BF)
    vs = [torch.randn(2, 50, 64, generator=g).mul(3).to(BF) for _ in range(N)]
    x0, noise = torch.randn(2, 50, 64, generator=g).mul(2).to(BF), torch.randn(2, 50, 64, generator=g).to(BF)
    m = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (1, 50, 4), generator=g)].to(BF).repeat(1, 1, 16)
    ab2 = [R.coefficients(SIG, FIRST + k, k > 0, lower_order_final=False) for k in range(N)]
    euler = [(float(np.float32(SIG[FIRST + k + 1]) - np.float32(SIG[FIRST + k])), 0.0, 0) for k in range(N)]
    sn = [float(SIG[FIRST + k + 1]) for k in range(N)]
    assert [c[2] for c in ab2] == [0] + [1] * (N - 1)
    assert all(c[0] != float(torch.tensor(c[0]).to(BF)) for c in ab2 + euler), "the coefficients are not bf16 numbers"
    assert all(s != float(torch.tensor(s).to(BF)) for s in sn), "the noise levels are not bf16 numbers"
    return dict(x=x, vs=vs, x0=x0, noise=noise, m=m, ab2=ab2, euler=euler, sn=sn)


def _outside(got, d, coef, masked):
    kw = dict(sigma_next=d["sn"], x0=d["x0"], noise=d["noise"], m=d["m"]) if masked else {}
    ref, bound = S.run64(d["x"], d["vs"], coef, **kw)
    return int((~((got.double() - ref).abs() <= bound)).sum()), float((bound / ref.abs().clamp_min(1e-3)).median())


def _run(d, coef, masked, one_step=S.step, **kw):
    mk = dict(sigma_next=d["sn"], x0=d["x0"], noise=d["noise"], m=d["m"]) if masked else {}
    return S.run32(d["x"], d["vs"], coef, one_step=one_step, **mk, **kw)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("solver", ["euler", "ab2"])
def test_float32_emulation_is_inside_the_summed_bound(data, solver, masked):
    n, rel = _outside(_run(data, data[solver], masked), data, data[solver], masked)
    print(f"[bound] {solver} masked={masked}: {n} outside, median bound / |ref| = {rel:.2e} after {N} steps")
    assert n == 0
    assert rel < 2.0 ** -18          # the bound is a float32 one: far below one bf16 rounding (2^-9) of the state


def test_blend_identities():
    g = torch.Generator().manual_seed(5)
    xs = torch.randn(1, 20, 64, generator=g)                        # a float32 state that is no bf16 number
    v, h, x0, noise = (torch.randn(1, 20, 64, generator=g).to(BF) for _ in range(4))
    c = R.coefficients(SIG, 13, True)
    s = S.step(xs, v, h, *c)
    ones, zeros = torch.ones(1, 20, 64, dtype=BF), torch.zeros(1, 20, 64, dtype=BF)
    assert torch.equal(S.step(xs, v, h, *c, 0.7311, x0, noise, ones).view(torch.int32), s.view(torch.int32))
    k = S.step(xs, v, h, *c, 0.7311, x0, noise, zeros)
    assert torch.equal(k, torch.add(torch.mul(S.f32(0.7311), noise.float()), torch.mul(S.f32(S.one_minus(0.7311)), x0.float())))
    assert torch.equal(S.step(xs, v, h, *c, 0.0, x0, noise, zeros), x0.float())          # the last step: x0 exactly
    assert not torch.equal(s.to(BF).float(), s)


def _step_fma(xs, v, h, c_v, c_h, use_hist, *rest):
    """A contracted multiply-add: the product is not rounded (float64 holds it exactly), the sum is rounded once."""
    s = (xs.double() + float(np.float32(c_v)) * v.double()).float()
    if use_hist:
        s = (s.double() + float(np.float32(c_h)) * h.double()).float()
    assert rest[-1] is None
    return s


def test_a_contracted_fma_changes_bits_in_an_exact_case():
    """c_v = 1 + 2^-23, v = 1 + 2^-7, x = -(1 + 2^-7).  The product is 1 + 2^-7 + 2^-23 + 2^-30 (an integer times 2^-30), which
    float32 rounds to 1 + 2^-7 + 2^-23; the sum with x is then 2^-23 exactly.  An fma keeps the 2^-30: 2^-23 + 2^-30.  The fma is
    the MORE accurate of the two, so no bound against float64 can catch it -- this case does, and the GPU tests hold the kernel
    to the op-by-op bits."""
    c_v = 1 + 2.0 ** -23
    x, v = torch.tensor([-(1 + 2.0 ** -7)]).to(BF), torch.tensor([1 + 2.0 ** -7]).to(BF)
    assert float(x) == -(1 + 2.0 ** -7) and float(np.float32(c_v)) == c_v
    right, fused = S.step(x.float(), v, None, c_v, 0.0, 0), _step_fma(x.float(), v, None, c_v, 0.0, 0, None)
    assert float(right) == 2.0 ** -23 and float(fused) == 2.0 ** -23 + 2.0 ** -30
    # with history too: c_h * h = -(1 + 2^-23) * 2^-23 = -(2^-23 + 2^-46), a float32 number either way, added to the s above
    h = torch.tensor([2.0 ** -23]).to(BF)
    right = S.step(x.float(), v, h, c_v, -c_v, 1)
    fused = _step_fma(x.float(), v, h, c_v, -c_v, 1, None)
    assert float(right) == -2.0 ** -46 and float(fused) == 2.0 ** -30 - 2.0 ** -46


def test_the_bound_catches_the_usual_mistakes(data):
    d = data
    bf = lambda f: float(torch.tensor(f, dtype=torch.float32).to(BF))  # noqa: E731
    wrong = {}
    for solver in ("euler", "ab2"):
        coef = d[solver]
        wrong[f"{solver}: c_v rounded to bf16"] = (_run(d, [(bf(c[0]), c[1], c[2]) for c in coef], False), coef, False)
        wrong[f"{solver}: state rounded to bf16 between steps"] = (
            _run(d, coef, False, one_step=lambda *a: S.step(*a).to(BF).float()), coef, False)
        poisoned = S.run32(torch.full_like(d["x"], float("nan")), d["vs"], coef)      # load_state = 1 at the first step
        wrong[f"{solver}: first step reads a poisoned state"] = (poisoned, coef, False)
        wrong[f"{solver}: sigma_next rounded to bf16 in k"] = (
            _run(d, coef, True, one_step=lambda xs, v, h, c_v, c_h, use, sn, x0, noise, m: torch.add(
                torch.mul(torch.sub(S.f32(1.0), m.float()),
                          torch.add(torch.mul(S.f32(bf(sn)), noise.float()), torch.mul(S.f32(S.one_minus(sn)), x0.float()))),
                torch.mul(m.float(), S.step(xs, v, h, c_v, c_h, use)))), coef, True)
    wrong["ab2: hist read after its store"] = (
        _run(d, d["ab2"], False, one_step=lambda xs, v, h, *a: S.step(xs, v, v, *a)), d["ab2"], False)
    for name, (got, coef, masked) in wrong.items():
        n, _ = _outside(got, d, coef, masked)
        print(f"[mistakes] {name}: {n} of {got.numel()} elements outside the bound")
        assert n > got.numel() // 4, name
    # the variant with everything right, written the same way as the wrong ones, is inside
    right = _run(d, d["ab2"], True, one_step=lambda *a: S.step(*a))
    assert _outside(right, d, d["ab2"], True)[0] == 0


# ---- what the state's type does to the solver ---------------------------------------------------------------------------------------
NS = (14, 28, 56, 112)


@pytest.fixture(scope="module")
def ode():
    x1 = (0.5 + torch.arange(4096, dtype=torch.float64) / 4096 * 1.5).to(BF)         # bf16 start values in [0.5, 2)
    return {(solver, state, n): S.ode_error(n, 1024, solver, state, x1)
            for solver in ("euler", "ab2") for state in ("bf16", "fp32") for n in NS}


@pytest.mark.parametrize("solver", ["euler", "ab2"])
def test_float32_state_is_closer_than_bf16_state(ode, solver):
    """RMS relative error at sigma = 0, S_tgt = 1024, 4096 start values, bf16 model input and bf16 velocity in both arms.
    Observed (bf16 state / fp32 state / fp32 state's final bf16 rounding):
      euler  N=14  8.129e-02 / 8.060e-02 / 8.031e-02     ab2  N=14  2.442e-02 / 2.187e-02 / 2.199e-02
             N=28  3.967e-02 / 3.768e-02 / 3.767e-02          N=28  1.391e-02 / 9.032e-03 / 9.202e-03
             N=56  2.183e-02 / 1.821e-02 / 1.833e-02          N=56  1.719e-02 / 2.705e-03 / 3.182e-03
             N=112 4.327e-02 / 8.997e-03 / 9.194e-03          N=112 4.470e-02 / 7.585e-04 / 1.820e-03
    At N = 14 Euler's truncation error dominates both arms and the margin is 1 %; it is asserted because it holds, not because
    it matters."""
    for n in NS:
        b, (f_state, f_tokens) = ode[solver, "bf16", n][0], ode[solver, "fp32", n]
        print(f"[state] {solver} N={n}: bf16 {b:.3e}, fp32 state {f_state:.3e}, its bf16 rounding {f_tokens:.3e}; "
              f"ratio {b / f_state:.2f}")
        assert f_state < b and f_tokens < b, (solver, n)


def test_bf16_state_stops_ab2_from_converging_and_float32_state_does_not(ode):
    """AB2, same setting.  bf16 state: the error falls from N = 14 to 28 (ratio 1.76) and then RISES -- 28 -> 56: 0.81,
    56 -> 112: 0.38 -- because every step rounds the state by 2^-9 and increments below half an ulp are lost.  float32 state:
    it keeps falling, 14 -> 28: 2.42, 28 -> 56: 3.34, 56 -> 112: 3.57, towards the rule's factor of 4; the floor set by the bf16
    velocity (2^-9 relative per step, averaging out over N steps) is not reached by N = 112.  The returned latents are the
    state's bf16 rounding, whose own 2^-9 is what remains at N = 112 (1.8e-3)."""
    bf = [ode["ab2", "bf16", n][0] for n in NS]
    fp = [ode["ab2", "fp32", n][0] for n in NS]
    print("[order] ab2, bf16 state: " + ", ".join(f"{a / b:.2f}" for a, b in zip(bf, bf[1:])))
    print("[order] ab2, fp32 state: " + ", ".join(f"{a / b:.2f}" for a, b in zip(fp, fp[1:])))
    assert bf[2] > bf[1] and bf[3] > bf[2]                      # more steps, more error
    assert all(a > b for a, b in zip(fp, fp[1:]))               # more steps, less error, all the way
    # Euler on the float32 state falls all the way too (observed 2.14, 2.07, 2.02: first order); on the bf16 state it turns
    # round between N = 56 and 112
    eu = [ode["euler", "fp32", n][0] for n in NS]
    print("[order] euler, fp32 state: " + ", ".join(f"{a / b:.2f}" for a, b in zip(eu, eu[1:])))
    assert all(a > b for a, b in zip(eu, eu[1:]))
    assert ode["euler", "bf16", 112][0] > ode["euler", "bf16", 56][0]
