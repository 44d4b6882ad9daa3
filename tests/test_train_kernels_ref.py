"""CPU: the references and bounds of tests/train_kernels_ref.py themselves, before any GPU sees them.

``adamw_ref`` against torch.optim.AdamW + clip_grad_norm_ in float64; ``adamw_emu`` (a correct fp32 implementation) inside
``adamw_bounds`` WITHOUT the margin over every input family of test_hip_train_kernels.py; ``adamw_emu`` with each deliberate mistake
outside the bound times MARGIN; ``flow_ref`` against oracle.train.flow_matching_loss + oracle.helpers.pack_latents /
unpack_latents under autograd; the share of gradient elements the neighbour rule excuses, from ``flow_ref`` and the bound alone.
"""
import numpy as np
import pytest
import torch

import train_kernels_ref as R

HP = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8)


def _np(t):
    return t.float().double().numpy()


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adamw_ref_matches_torch_adamw_in_float64(weight_decay):
    """Steps 1, 2, 999, 1000 (the optimiser's step count is set to 998 after the second), clipping active on the first two.
    torch computes step_size, the bias corrections and the decay in double, so the derived scalars stay unrounded here
    (``round32=False``); the hyper-parameters are the fp32-rounded ones on both sides."""
    gen = torch.Generator().manual_seed(3)
    shapes = [(37, 5), (129,)]
    hp = dict(lr=R.f32(HP["lr"]), betas=(R.f32(0.9), R.f32(0.99)), eps=R.f32(HP["eps"]), weight_decay=R.f32(weight_decay))
    ref = [torch.nn.Parameter((0.02 * torch.randn(s, generator=gen)).double()) for s in shapes]
    opt = torch.optim.AdamW(ref, foreach=False, **hp)
    p = [t.detach().numpy().copy() for t in ref]
    m = [np.zeros_like(t) for t in p]
    v = [np.zeros_like(t) for t in p]
    for step in (1, 2, 999, 1000):
        if step == 999:
            for t in ref:
                opt.state[t]["step"] = torch.tensor(998.0)
        grads = [((3.0 if step <= 2 else 0.01) * torch.randn(s, generator=gen)).double() for s in shapes]
        for t, g in zip(ref, grads):
            t.grad = g.clone()
        norm = float(torch.nn.utils.clip_grad_norm_(ref, 1.0))
        opt.step()
        coef = min(1.0, 1.0 / (norm + 1e-6))
        assert (coef < 1.0) == (step <= 2)
        sc = R.adamw_scalars(step, weight_decay=weight_decay, round32=False, **HP)
        for i, g in enumerate(grads):
            p[i], m[i], v[i] = R.adamw_ref(p[i], g.numpy(), m[i], v[i], sc, coef)
            np.testing.assert_allclose(p[i], ref[i].detach().numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(m[i], opt.state[ref[i]]["exp_avg"].numpy(), rtol=1e-12, atol=0)
            np.testing.assert_allclose(v[i], opt.state[ref[i]]["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)


def _family(si, ci):
    n = R.ADAMW_SIZES[si]
    g_bf16, clip, _off, gs = R.ADAMW_COMBOS[ci]
    step, wd, _ = R.adamw_case(si, ci)
    p, g, m, v = R.adamw_inputs(n, g_bf16, seed=n % 1000 + ci)
    _, _, coef = R.adamw_coef(g, clip, gs)
    return (_np(p), _np(g), _np(m), _np(v)), R.adamw_scalars(step, weight_decay=wd, **HP), coef, clip, g_bf16


def _ratios(got, want, bounds):
    return [float(np.max(np.abs(a.astype(np.float64) - b) / e)) for a, b, e in zip(got, want, bounds)]


@pytest.mark.parametrize("si", range(len(R.ADAMW_SIZES)))
def test_adamw_emu_is_within_the_bound_without_the_margin(si):
    """Every (size, combination) the GPU test runs; view offsets change no value, so offset-1 combinations are skipped."""
    worst = [0.0, 0.0, 0.0]
    for ci, combo in enumerate(R.ADAMW_COMBOS):
        if combo[2]:
            continue
        ins, sc, coef, clip, g_bf16 = _family(si, ci)
        r = _ratios(R.adamw_emu(*ins, sc, coef, g_bf16), R.adamw_ref(*ins, sc, coef), R.adamw_bounds(*ins, sc, coef, clip))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert max(r) <= 1.0, (R.ADAMW_SIZES[si], combo, r)
    print(f"[adamw emu] n={R.ADAMW_SIZES[si]}: worst error / bound: master {worst[0]:.3f} m {worst[1]:.3f} v {worst[2]:.3f}")


def test_the_cycled_cases_cover_every_step_decay_and_bf16_choice():
    seen = {R.adamw_case(si, ci) for si in range(len(R.ADAMW_SIZES)) for ci in range(len(R.ADAMW_COMBOS))}
    assert seen == {(s, w, b) for s in (1, 2, 1000) for w in (0.0, 0.01) for b in (False, True)}


@pytest.mark.parametrize("mistake", R.ADAMW_MISTAKES)
def test_adamw_mistakes_leave_the_bound(mistake):
    """At 1027 elements, step 2 (bc2_sqrt = 0.14, far from 1), weight decay 0.01, bf16 gradients, clipping on, grad_scale 0.5: each
    mistake moves some element of master (and, for the coefficient, of m and v) beyond MARGIN times its bound."""
    p, g, m, v = R.adamw_inputs(1027, True, seed=11)
    _, _, coef = R.adamw_coef(g, True, 0.5)
    assert coef < 0.5
    ins = (_np(p), _np(g), _np(m), _np(v))
    sc = R.adamw_scalars(2, weight_decay=0.01, **HP)
    want, bounds = R.adamw_ref(*ins, sc, coef), R.adamw_bounds(*ins, sc, coef, True)
    assert max(_ratios(R.adamw_emu(*ins, sc, coef, True), want, bounds)) <= 1.0
    r = _ratios(R.adamw_emu(*ins, sc, coef, True, mistake=mistake), want, bounds)
    print(f"[adamw mistake] {mistake}: error / bound: master {r[0]:.3g} m {r[1]:.3g} v {r[2]:.3g}")
    assert r[0] > R.MARGIN
    if mistake == "coef_not_applied_to_bf16":
        assert r[1] > R.MARGIN and r[2] > R.MARGIN


def test_bit_equality_premise_no_subnormal_intermediate():
    """The GPU test's bit-equality families (clipping off, grad_scale 1) have no subnormal intermediate in the emulation."""
    for si in range(len(R.ADAMW_SIZES)):
        for ci, (g_bf16, clip, off, gs) in enumerate(R.ADAMW_COMBOS):
            if clip or gs != 1.0 or off:
                continue
            ins, sc, coef, _, _ = _family(si, ci)
            assert coef == 1.0
            trace = []
            R.adamw_emu(*ins, sc, coef, g_bf16, trace=trace)
            assert R.no_subnormals(trace), (si, ci)
    tiny = [np.float32(1e-39)]
    assert not R.no_subnormals([np.array(tiny)])


@pytest.mark.parametrize("variant", R.FLOW_VARIANTS)
def test_flow_ref_matches_the_oracle_under_autograd(variant):
    """Integer data at B=3, C=16, h=12, w=20: every term w d^2 <= 16 * 144 is an integer and the sum of the 11 520 of them stays
    below 2^24 (asserted), so the oracle's fp32 sum is exact and its loss carries only the roundings of its one or two divisions
    (3u with their second-order terms); its gradient 2 w d / denominator at most four fp32 roundings (5u likewise).  ``flow_ref`` in
    float64 must agree to that."""
    from oracle import helpers, train as otrain
    B, C, h, w = shape = R.FLOW_SHAPES[2]
    ins = R.flow_inputs(shape, variant, exact=True, seed=21)
    ref = R.flow_ref(ins["pred"], ins["x"], ins["noise"], ins["sigma"], ins["weight"], ins["area"], ins["mask"])
    assert ref["sum"] == round(ref["sum"]) and ref["sum"] < 2 ** 24          # positive whole terms: every partial sum is below the total
    p = ins["pred"].double().requires_grad_(True)
    weighting = torch.ones(B, 1, 1, 1)
    for k, shp in (("weight", (B, 1, 1, 1)), ("area", (B, 1, h, w)), ("mask", (B, 1, h, w))):
        if ins[k] is not None:
            weighting = weighting * ins[k].view(shp)
    loss = otrain.flow_matching_loss(helpers.unpack_latents(p, h * 8, w * 8), ins["x"], ins["noise"], weighting, weight_mask=ins["mask"])
    loss.backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= 3 * R.U * ref["loss"] and ref["loss"] > 0
    assert bool(((p.grad - ref["grad"]).abs() <= 5 * R.U * ref["grad"].abs()).all()) and float(ref["grad"].abs().max()) > 0
    if ins["mask"] is not None:
        assert ref["denom"] == float(ins["mask"].sum()) * C < ins["x"].numel()
        outside = helpers.pack_latents((1.0 - ins["mask"]).expand(B, C, h, w).contiguous()) > 0
        assert bool(outside.any()) and float(ref["grad"][outside].abs().max()) == 0
    # the token map: the same float64 values through the oracle's packing, and its unpacking as the inverse
    sg = ins["sigma"].double().view(B, 1, 1, 1)
    assert torch.equal(ref["tokens"], helpers.pack_latents((1.0 - sg) * ins["x"].double() + sg * ins["noise"].double()))
    assert torch.equal(helpers.unpack_latents(ref["grad"], h * 8, w * 8), R.unpack(ref["grad"], h, w))
    assert torch.equal(R.unpack(R.pack(ins["x"]), h, w), ins["x"])


@pytest.mark.parametrize("shape", R.FLOW_SHAPES)
def test_flow_gradient_excused_share_is_below_one_percent(shape):
    """From ``flow_ref`` and ``flow_bounds`` alone: the share of gradient elements whose fp64 value lies within the derived fp32
    error of a bf16 rounding boundary (where the neighbour rule admits two values) for the seeds the GPU test uses."""
    for vi, variant in enumerate(R.FLOW_VARIANTS):
        ins = R.flow_inputs(shape, variant, exact=False, seed=40 + vi)
        ref = R.flow_ref(ins["pred"], ins["x"], ins["noise"], None, ins["weight"], ins["area"], ins["mask"])
        b = R.flow_bounds(ins["pred"], ins["x"], ins["noise"], ins["weight"], ins["area"], ins["mask"])
        lo, hi, _ = R.bf16_interval(ref["grad"], b["grad"])
        share = float((lo != hi).double().mean())
        print(f"[flow grad] {shape} {variant}: excused share {share:.5f}, loss bound / loss {b['loss'] / ref['loss']:.3e}")
        assert share <= 0.01
        assert 0 < b["loss"] < 1e-6 * ref["loss"]


def test_round_to_bf16_and_interval():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.0e-6, 0.0], dtype=torch.float64)
    assert R.round_to_bf16(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, float(torch.tensor(-3.0e-6).to(torch.bfloat16)), 0.0]
    lo, hi, mid = R.bf16_interval(torch.tensor([1.0 + 2.0 ** -8 + 1e-9, 1.25], dtype=torch.float64), torch.tensor([1e-8, 1e-8], dtype=torch.float64))
    assert lo.tolist() == [1.0, 1.25] and hi.tolist() == [1.0 + 2.0 ** -7, 1.25] and mid.tolist() == [1.0 + 2.0 ** -7, 1.25]
