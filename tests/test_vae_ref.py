"""CPU checks of tests/vae_ref.py: the bounds tests/test_hip_vae_exact.py holds the HIP kernels to are neither vacuous nor too
tight -- an fp32 emulation of the GroupNorm summation order, the attention rounding model and the oracle's own bf16 evaluation
of GroupNorm-apply and of the convolutions each stay inside them."""
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
import vae_ref as vr

BF = torch.bfloat16
F64 = torch.float64


@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("C,HW", vr.GN_CASES)
def test_groupnorm_summation_order_stays_inside_the_bound(C, HW, kind):
    """The kernels' fp32 summation order, emulated in numpy, against fp64: inside the derived bound for bf16 and fp32 inputs,
    and not by an empty margin (the bound is at most a few thousand times what the order costs on the worst group)."""
    lay = vr.gn_layout(C, HW)
    expect = {(128, 8323): 66, (512, 4100): 129, (128, 66313): 512, (256, 40000): 512, (128, 5): 1, (1024, 300): 19}
    assert lay["nblk"] == expect[(C, HW)] and lay["n_m"] == 16
    x32 = vr.gn_data(C, HW, kind)
    for name, x in (("bf16", x32.to(BF)), ("fp32", x32)):
        st = vr.gn_emulate(x)
        r_mean, r_rstd = vr.gn_check_stats(f"emulated GroupNorm stats {kind} {name}", st, x, C, HW)
        assert r_mean > 0 or r_rstd > 0 or HW * C < 4096


def test_groupnorm_bound_catches_a_skipped_block():
    """The finalize loop stepping by 128 instead of 64 drops blocks 64..127 of nblk = 66: two of 66 partial sums."""
    C, HW = 128, 8323
    x = vr.gn_data(C, HW, "well").to(BF)
    lay = vr.gn_layout(C, HW)
    cut = x.clone()[:, :64 * lay["per_blk"]]                  # what such a kernel would have summed
    ref = vr.gn_stats64(cut)
    wrong = torch.stack([ref["mean"] * cut.shape[1] / HW, ref["rstd"]], dim=-1).float()
    with pytest.raises(AssertionError):
        vr.gn_check_stats("dropped blocks", wrong, x, C, HW)


@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_apply_bound_holds_for_the_bf16_evaluation(silu):
    C, HW = 512, 999
    g = torch.Generator().manual_seed(3)
    x = vr.gn_data(C, HW, "well").to(BF)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(BF), (0.1 * torch.randn(C, generator=g)).to(BF)
    ref = vr.gn_stats64(x)
    stats = torch.stack([ref["mean"], ref["rstd"]], dim=-1).float()
    t64 = vr.gn_apply64(x, stats, gamma, beta)
    mean = stats[..., 0].repeat_interleave(C // 32, dim=1)[:, None, :]
    rstd = stats[..., 1].repeat_interleave(C // 32, dim=1)[:, None, :]
    t32 = (x.float() - mean) * rstd * gamma.float() + beta.float()
    y = F.silu(t32.to(BF).float()).to(BF) if silu else t32.to(BF)
    r = vr.gn_check_apply(f"bf16 evaluation silu={silu}", y, t64, silu)
    assert r > 0.05 if silu else True                          # the bound is used, not vacuous
    bad = y.clone()
    i = t64.abs().flatten().argmax()
    bad.view(-1)[i] = (bad.view(-1)[i].float() * (1 + 2.0 ** -5)).to(BF)   # one element 4 to 8 ulp off
    with pytest.raises(AssertionError):
        vr.gn_check_apply("one wrong element", bad, t64, silu)


@pytest.mark.parametrize("S,scale", [(1, None), (2, None), (31, None), (33, None), (65, None), (129, None), (257, None), (300, 0.01),
                                     (300, 0.125)])
def test_hd512_rounding_model_against_fp64(S, scale):
    """rho, the model's worst row-relative error, is finite and of bf16 size; the model passes its own check at margin 1; a
    result with one wrong row of 512 does not."""
    scale = 512 ** -0.5 if scale is None else scale
    q, k, v = vr.hd512_inputs(2, S, seed=500 + S)
    ref, mod = vr.hd512_ref_and_model(q, k, v, scale)
    r = ar.assert_rows_close(f"hd512 model S={S} scale={scale:.4g}", mod, ref, mod, margin=1.0)
    # S = 1: p = 1, O = v exactly and rho = 0; the floor alone bounds the rows then
    assert (2.0 ** -11 < r["rho"] if S > 1 else r["rho"] == 0.0) and r["rho"] < 2.0 ** -7 and r["ratio"] <= 1.0 + 1e-9
    bad = mod.clone()
    bad[1, 0, S - 1] = ref[1, 0, S - 1] * (1 + 2.0 ** -5)
    with pytest.raises(AssertionError):
        ar.assert_rows_close("one wrong row", bad, ref, mod)


def test_hd512_model_sees_an_extra_key():
    """A key mask off by one (key S admitted: the clamped copy of key S - 1) moves rows beyond the bound at a ragged S."""
    S = 33
    q, k, v = vr.hd512_inputs(2, S, seed=533)
    ref, mod = vr.hd512_ref_and_model(q, k, v, 512 ** -0.5)
    k2, v2 = torch.cat([k, k[:, -1:]], dim=1), torch.cat([v, v[:, -1:]], dim=1)
    q2 = torch.cat([q, q[:, -1:]], dim=1)
    _, wrong = vr.hd512_ref_and_model(q2, k2, v2, 512 ** -0.5)
    with pytest.raises(AssertionError):
        ar.assert_rows_close("extra key", wrong[:, :, :S], ref, mod)


@pytest.mark.parametrize("cin,cout,h,w,mode", [(128, 128, 9, 7, "s1"), (128, 128, 11, 9, "s2"), (512, 256, 5, 5, "1x1"),
                                               (256, 128, 7, 5, "up"), (128, 8, 13, 11, "s1")])
def test_conv_cap_holds_for_the_bf16_evaluation(cin, cout, h, w, mode):
    """The oracle's own evaluation (fp32 convolution of the bf16 operands, rounded to bf16; the residual added in bf16) passes
    the per-element cap; one element two ulps off does not."""
    g = torch.Generator().manual_seed(cin + h)
    ks = 1 if mode == "1x1" else 3
    x = torch.randn(2, cin, h, w, generator=g).to(BF)
    wt = (torch.randn(cout, cin, ks, ks, generator=g) * 0.05).to(BF)
    bias = (torch.randn(cout, generator=g) * 0.1).to(BF)
    xf = x.float()
    if mode == "up":
        y = F.conv2d(F.interpolate(xf, scale_factor=2.0, mode="nearest"), wt.float(), bias.float(), padding=1)
    elif mode == "s2":
        y = F.conv2d(F.pad(xf, (0, 1, 0, 1)), wt.float(), bias.float(), stride=2)
    elif mode == "1x1":
        y = F.conv2d(xf, wt.float(), bias.float())
    else:
        y = F.conv2d(xf, wt.float(), bias.float(), padding=1)
    res = torch.randn(*y.shape, generator=g).to(BF)
    ref64, cap = vr.conv_ref_and_cap(x, wt, bias, mode)
    r = vr.check_cap(f"bf16 evaluation conv {mode}", y.to(BF), ref64, cap)
    assert r > 0.1
    ref64r, capr = vr.conv_ref_and_cap(x, wt, bias, mode, res=res)
    vr.check_cap(f"bf16 evaluation conv {mode} + res", res + y.to(BF), ref64r, capr)
    bad = y.to(BF).clone()
    i = ref64.abs().flatten().argmax()
    bad.view(-1)[i] = (bad.view(-1)[i].float() * (1 + 2.0 ** -6)).to(BF)
    with pytest.raises(AssertionError):
        vr.check_cap("one wrong element", bad, ref64, cap)
