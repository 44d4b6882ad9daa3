"""CPU: the element rule and the sum bounds of the backward norm kernels (backward_ref) on their own -- the float32 emulations
of the kernels' order pass them at every shape the GPU test uses and stay within a quarter of the margins, those inputs leave
the rule little freedom (the ambiguous share is capped), every planted mistake fails, and the check the rule replaces lets the
largest of them through."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_ref as R  # noqa: E402
from backward_ref import judge  # noqa: E402

BF = torch.bfloat16
U = R.U


def _check(name, v):
    print(v.line(name), flush=True)
    assert v.ok, v.line(name)
    assert v.ambiguous <= R.AMBIGUOUS_CAP, f"{name}: ambiguous share {v.ambiguous:.3e} above the cap {R.AMBIGUOUS_CAP}"


def _worst_u(raw, ref):
    """largest |float32 stage - z| in units of u x scale; where the scale is 0 the stage must be z."""
    d = (raw.double() - ref["z"]).abs()
    pos = ref["err"] > 0
    assert bool((d[~pos] == 0).all())
    return float((d[pos] / (U * ref["err"][pos])).max())


def _within(name, got, ref64, bound):
    share = R.worst_share(got, ref64, bound)
    print(f"[parity] {name}: worst share of the bound {share:.4f}", flush=True)
    assert share <= 1.0, f"{name}: {share:.3f} x the bound"
    return share


def test_chunking_follows_the_launchers():
    assert [R.pick_chunks(r, 16, 512) for r in (1, 16, 17, 37, 300, 8704)] == [1, 1, 2, 3, 19, 512]
    # rows per wave + 3 (LDS) + running sums + 3 + 3
    assert [R.ln_chain(r) for r in (1, 16, 17, 300, 8704)] == [1 + 10, 4 + 10, 3 + 10, 4 + 10, 5 + 3 + 16 + 6]
    assert R.gate_chain(75) == 15 + 1 + 6 and R.dw_chain(1, 24, 80) == 4 + 16 + 2 + 6


@pytest.mark.parametrize("B", R.LN_BS)
@pytest.mark.parametrize("D", R.LN_DS)
def test_ln_bwd_emulation_passes_and_the_inputs_leave_little_freedom(D, B):
    worst = 0.0
    for Rr in R.LN_RS:
        xb, dn, mod, dxb = R.ln_bwd_inputs(D, B, Rr)
        x, scale = xb[:, R.S_TXT:], mod[:, D:2 * D]
        for dx_in in (None, dxb[:, R.S_TXT:]):
            name = f"ln_bwd emulation D={D} B={B} R={Rr}{' + dx_in' if dx_in is not None else ''}"
            ref = R.ln_bwd_ref(x, dn, scale, dx_in)
            raw, dshift, dscale = R.emulate_ln_bwd(x, dn, scale, dx_in, rounded=False)
            worst = max(worst, _worst_u(raw, ref))
            _check(name, judge(raw.to(BF), *R.accept(ref, R.LN_C)))
            _within(name + " dshift", dshift, ref["dshift"], ref["dshift_bound"])
            _within(name + " dscale", dscale, ref["dscale"], ref["dscale_bound"])
            if Rr >= 5:       # the row whose dn is zero: dx_in's bits, or +0
                want = dx_in[B - 1, 3] if dx_in is not None else torch.zeros(D, dtype=BF)
                assert torch.equal(raw.to(BF)[B - 1, 3].view(torch.int16), want.view(torch.int16))
    print(f"[parity] ln_bwd emulation D={D} B={B}: float32 stage within {worst:.2f} u of the scale (margin {R.LN_C})", flush=True)
    assert worst <= R.LN_C / 4


@pytest.mark.parametrize("case", R.QKV_CASES)
def test_qkv_post_bwd_emulation_passes_and_the_inputs_leave_little_freedom(case):
    dq, dk, qkv, w, cos, sin = R.qkv_bwd_inputs(*case)
    s_txt = case[2]
    ref = R.qkv_post_bwd_ref(dq, dk, qkv, w, cos, sin, s_txt)
    raw, dw = R.emulate_qkv_post_bwd(dq, dk, qkv, w, cos, sin, s_txt, rounded=False)
    worst = _worst_u(raw, ref)
    print(f"[parity] qkv_post_bwd emulation {case}: float32 stage within {worst:.2f} u of the scale (margin {R.QKV_C})", flush=True)
    assert worst <= R.QKV_C / 4
    _check(f"qkv_post_bwd emulation {case}", judge(raw.to(BF), *R.accept(ref, R.QKV_C)))
    _within(f"qkv_post_bwd emulation {case} dw", dw, ref["dw"], ref["dw_bound"])
    if s_txt == 0:
        assert bool((dw[:, 1] == 0).all()) and bool((ref["dw"][:, 1] == 0).all())


def test_gate_res_reference():
    B, Rr, N = R.GATE_CASE
    dob, yb, mod = R.gate_inputs(B, Rr, N)
    dout, y, gate = dob[:, R.S_TXT:], yb[:, R.S_TXT:], mod[:, N:2 * N]
    dy, dgate, bound = R.gate_res_ref(dout, y, gate)
    # one product of two bf16 values rounded once: the float32 product is exact, so its conversion is the only rounding
    assert dy.dtype == BF and torch.equal(dy, (dout.float() * gate.float()[:, None]).to(BF))
    assert torch.equal(dy.double(), R.rn_bf16(dout.double() * gate.double()[:, None]))
    t = dout.float() * y.float()
    assert torch.equal(t.double(), dout.double() * y.double())
    _within("gate_res_bwd emulation dgate", R.emulate_gate_sum(t), dgate, bound)
    t[:, 40] = 0                                                     # one row left out
    assert R.worst_share(R.emulate_gate_sum(t), dgate, bound) > 1.0


@pytest.mark.parametrize("D", R.LN_DS)
def test_rule_rejects_ln_bwd_mistakes(D):
    B, Rr = 3, 37
    xb, dn, mod, dxb = R.ln_bwd_inputs(D, B, Rr)
    x, scale, dx_in = xb[:, R.S_TXT:], mod[:, D:2 * D], dxb[:, R.S_TXT:]
    ref = R.ln_bwd_ref(x, dn, scale, dx_in)
    alts, wide = R.accept(ref, R.LN_C)
    for mutant in R.LN_MUTANTS:
        dx, dshift, dscale = R.emulate_ln_bwd(x, dn, scale, dx_in, mutant=mutant)
        v = judge(dx, alts, wide)
        s_sh = R.worst_share(dshift, ref["dshift"], ref["dshift_bound"])
        s_sc = R.worst_share(dscale, ref["dscale"], ref["dscale_bound"])
        print(v.line(f"planted D={D}: {mutant}") + f"; dshift {s_sh:.3g} dscale {s_sc:.3g} x the bound", flush=True)
        assert s_sh <= 1.0                                           # no mutant touches dshift
        if "dscale" in mutant:
            assert v.ok and s_sc > 1.0, mutant
        else:
            assert not v.ok and v.misses >= 8, mutant


@pytest.mark.parametrize("case", [(2, 3, 21, 75), (1, 3, 37, 130)])
def test_rule_rejects_qkv_post_bwd_mistakes(case):
    dq, dk, qkv, w, cos, sin = R.qkv_bwd_inputs(*case)
    s_txt = case[2]
    ref = R.qkv_post_bwd_ref(dq, dk, qkv, w, cos, sin, s_txt)
    alts, wide = R.accept(ref, R.QKV_C)
    for mutant in R.QKV_MUTANTS:
        dx, dw = R.emulate_qkv_post_bwd(dq, dk, qkv, w, cos, sin, s_txt, mutant=mutant)
        v = judge(dx, alts, wide)
        s_dw = R.worst_share(dw, ref["dw"], ref["dw_bound"])
        print(v.line(f"planted {case}: {mutant}") + f"; dw {s_dw:.3g} x the bound", flush=True)
        if mutant.endswith("dw"):
            assert v.ok and s_dw > 1.0, mutant
        else:
            assert not v.ok and v.misses >= 8, mutant
    # the text weight on the first image row touches that row alone
    dx, _ = R.emulate_qkv_post_bwd(dq, dk, qkv, w, cos, sin, s_txt, mutant="text weight for the first image row")
    bad = (dx.view(torch.int16) != R.emulate_qkv_post_bwd(dq, dk, qkv, w, cos, sin, s_txt)[0].view(torch.int16)).any(-1).any(0)
    assert bad.nonzero().flatten().tolist() == [s_txt]


def test_the_check_this_replaces_lets_a_dropped_m1_through():
    """tests/test_hip_backward.py::close_bf16 (max error <= 1.5 % of max|ref|, mean error <= 0.3 % of it) on the inputs of its
    test_ln_modulate_bwd at D = 3072: the emulation WITHOUT the m1 = mean(gl) term passes it, with and without dx_in, and
    misses the element rule on tens of thousands of elements.  This is why the rule exists."""
    def randn(*shape, seed, scale=1.0):
        return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF)

    def close_bf16(got, ref, tol=1.5e-2):
        d = (got.double() - ref.double()).abs()
        scale = ref.abs().max().item()
        return (bool(torch.isfinite(got.float()).all()) and d.max().item() <= tol * scale + 1e-6
                and d.mean().item() <= 0.2 * tol * scale + 1e-7), d.max().item() / scale, d.mean().item() / scale

    B, S_txt, D, Rr = 2, 11, 3072, 37
    x = (randn(B, S_txt + Rr, D, seed=1, scale=2.0) + 0.5)[:, S_txt:]
    scale = randn(B, 6 * D, seed=2, scale=0.3)[:, D:2 * D]
    dn = randn(B, Rr, D, seed=3)
    dx_all = randn(B, S_txt + Rr, D, seed=4, scale=0.5)[:, S_txt:]
    for dx_in in (dx_all, None):
        ref = R.ln_bwd_ref(x, dn, scale, dx_in)
        alts, wide = R.accept(ref, R.LN_C)
        good = R.emulate_ln_bwd(x, dn, scale, dx_in)[0]
        bad = R.emulate_ln_bwd(x, dn, scale, dx_in, mutant="m1 dropped")[0]
        ok, mx, mn = close_bf16(bad, ref["z"].float())
        v_good, v_bad = judge(good, alts, wide), judge(bad, alts, wide)
        print(f"[parity] m1 dropped, D = 3072{' + dx_in' if dx_in is not None else ''}: close_bf16 passes ({mx:.2%} of absmax at "
              f"most, {mn:.2%} on average; allowed 1.5 % / 0.3 %); the rule: {v_bad.misses} of {v_bad.n} elements miss", flush=True)
        assert ok, "the old check was expected to let the dropped m1 through"
        assert v_good.ok and v_good.ambiguous <= R.AMBIGUOUS_CAP
        assert v_bad.misses >= 10000
