"""CPU: the acceptance rule of the forward small kernels (forward_ref) on its own -- the float32 emulations of the kernels'
arithmetic pass it on every input the GPU tests use, those inputs leave the rule little freedom (the ambiguous share is capped),
and the rule rejects each mistake it exists to catch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forward_ref as R  # noqa: E402

BF = torch.bfloat16


def _check(name, v, cap):
    print(v.line(name), flush=True)
    assert v.ok, v.line(name)
    assert v.ambiguous <= cap, f"{name}: ambiguous share {v.ambiguous:.3e} above the cap {cap}"


def test_rn_bf16_is_round_to_nearest_even_without_the_float32_detour():
    one = torch.tensor([1.0], dtype=torch.float64)
    ulp = 2.0 ** -7
    assert R.rn_bf16(one + ulp / 2).item() == 1.0                    # tie -> even
    assert R.rn_bf16(one + 3 * ulp / 2).item() == 1.0 + 2 * ulp      # tie -> even
    assert R.rn_bf16(one + ulp / 2 + 2.0 ** -40).item() == 1.0 + ulp  # float32 would have made this a tie first
    assert R.rn_bf16(one * 2.0 ** -130).item() == 2.0 ** -130        # bf16 subnormal
    assert R.rn_bf16(one * 1.4 * 2.0 ** -133).item() == 2.0 ** -133
    g = torch.Generator().manual_seed(1)
    v = torch.randn(100000, generator=g, dtype=torch.float64).float()
    assert torch.equal(R.rn_bf16(v.double()).to(BF), v.to(BF))        # from float32 both conversions are one rounding
    b = torch.tensor([1.0, -1.0, 0.0, 1.9921875, -0.5], dtype=torch.float64)
    assert R.bf16_next(b).tolist() == [1.0 + ulp, -1.0 + ulp / 2, 2.0 ** -133, 2.0, -0.5 + ulp / 4]


@pytest.mark.parametrize("B,Rr", R.LN_BR)
@pytest.mark.parametrize("D", R.LN_DS)
def test_ln_emulation_passes_and_the_inputs_leave_little_freedom(D, B, Rr):
    buf, mod = R.ln_inputs(D, B, Rr)
    x = buf[:, R.LN_S_TXT:]
    z, delta = R.ln_stage(x)
    emu = R.emulate_ln(x)
    # the margin's own claim: the emulated float32 stage uses at most half of it (8 of 16 u of the scale |z| + |mean| rstd) --
    # what the device may add, an rsqrtf one ulp (2 u |z|) off the correctly rounded one and fused squares, fits in the rest
    worst = ((R.emulate_ln(x, rounded=False).double() - z).abs() / (delta / 16)).max().item()
    print(f"[parity] ln emulation D={D}: float32 stage within {worst:.2f} u of z (margin 16)", flush=True)
    assert worst <= 8.0
    lo, hi, wide = R.candidates(z, delta)
    for split in R.ln_forms(Rr):
        shift, scale = R.ln_modulation(mod, D, split, Rr)
        alts = [R.ln_tail(lo, shift, scale), R.ln_tail(hi, shift, scale)]
        _check(f"ln emulation D={D} B={B} R={Rr} split={split}", R.judge(R.ln_tail(emu, shift, scale), alts, wide), R.AMBIGUOUS_CAP["ln"])


def test_rule_rejects_ln_mistakes():
    D, B, Rr = 512, 2, 37
    buf, mod = R.ln_inputs(D, B, Rr)
    x = buf[:, R.LN_S_TXT:]
    emu = R.emulate_ln(x)
    shift, scale = R.ln_modulation(mod, D, 21, Rr)
    alts, wide = R.ln_accept(x, shift, scale)
    assert R.judge(R.ln_tail(emu, shift, scale), alts, wide).ok
    f = lambda t: t.float()  # noqa: E731
    planted = {
        "product not rounded": (f(emu) * f(1 + scale) + f(shift)).to(BF),
        "1 + scale not rounded": (f(emu) * (1 + f(scale))).to(BF) + shift,
        "LN not rounded": (R.emulate_ln(x, rounded=False) * f(1 + scale)).to(BF) + shift,
        "shift and scale swapped": R.ln_tail(emu, scale, shift),
        "split off by one row": R.ln_tail(emu, *R.ln_modulation(mod, D, 22, Rr)),
    }
    for name, got in planted.items():
        v = R.judge(got, alts, wide)
        print(v.line("planted: " + name), flush=True)
        assert not v.ok, name
    # off by one touches exactly one row of every batch
    v = R.judge(planted["split off by one row"], alts, wide)
    assert v.first_miss[1] == 21


@pytest.mark.parametrize("case", R.QKV_CASES[:3])
def test_rms_emulation_passes_on_the_small_qkv_inputs(case):
    B, H, s_txt, hh, ww = case
    qkv, w, cos, sin = R.qkv_inputs(*case)
    for which in (0, 1):
        wi, wt = w[which], (w[2 + which] if s_txt else None)
        alts = R.qkv_accept(qkv, which, wi, wt, cos, sin, s_txt)
        _check(f"rms emulation {case} {'qk'[which]}", R.judge(R.qkv_emulated(qkv, which, wi, wt, cos, sin, s_txt), alts, group=2),
               R.AMBIGUOUS_CAP["rms"])
    if s_txt and hh * ww:    # planted: text and image norm weights swapped
        alts = R.qkv_accept(qkv, 0, w[0], w[2], cos, sin, s_txt)
        assert not R.judge(R.qkv_emulated(qkv, 0, w[2], w[0], cos, sin, s_txt), alts, group=2).ok
        assert not R.judge(R.qkv_emulated(qkv, 0, w[0], w[2], cos, sin, s_txt + 1), alts, group=2).ok


def test_large_qkv_input_tells_a_contracted_rope_from_the_specified_one():
    """On the H = 24 input the rule passes the emulation, and an fma in the rotation -- either product kept exact -- moves at
    least 8 elements for which the rule accepts one bit pattern only: 0 misses on the GPU then prove that the kernel does not
    contract, and are not luck."""
    case = R.QKV_LARGE
    s_txt = case[2]
    qkv, w, cos, sin = R.qkv_inputs(*case)
    for which in (0, 1):
        wi, wt = w[which], w[2 + which]
        alts = R.qkv_accept(qkv, which, wi, wt, cos, sin, s_txt)
        good = R.qkv_emulated(qkv, which, wi, wt, cos, sin, s_txt)
        _check(f"rms emulation {case} {'qk'[which]}", R.judge(good, alts, group=2), R.AMBIGUOUS_CAP["rms"])
        una = R.unambiguous_mask(alts, group=2)
        for exact in (0, 1):
            bad = R.qkv_emulated(qkv, which, wi, wt, cos, sin, s_txt, R.rope_contracted(exact))
            moved = int(((bad.view(torch.int16) != good.view(torch.int16)) & una).sum())
            v = R.judge(bad, alts, group=2)
            print(f"[parity] contracted RoPE (product {exact} exact) {'qk'[which]}: {moved} unambiguous elements moved "
                  f"({moved / good.numel():.2e}), rule misses {v.misses}", flush=True)
            assert moved >= 8 and not v.ok and v.misses >= 8


@pytest.mark.parametrize("n", R.SOFTMAX_NS)
def test_softmax_emulation_passes_and_a_forgotten_wave_does_not(n):
    x = R.softmax_inputs(n)
    alts, wide, tiny = R.softmax_accept(x)
    nv = R.softmax_nv(n)
    cap = R.AMBIGUOUS_CAP["softmax_nv32" if nv == 32 else "softmax"]
    print(f"[parity] softmax n={n}: NV={nv} c={R.softmax_c(nv)} below-normal share {tiny.float().mean().item():.3f}", flush=True)
    _check(f"softmax emulation n={n}", R.judge(R.emulate_softmax(x), alts, wide, bounded=tiny), cap)
    if n >= 1024:            # (below 772 columns wave 3 holds nothing)
        assert not R.judge(R.emulate_softmax(x, missing_wave=True), alts, wide, bounded=tiny).ok
    # rows sum to 1 in the reference, the equal row is 1 / n, the spiked row is the spike
    z, _ = R.softmax_stage(x)
    assert (z.sum(-1) - 1).abs().max().item() < 1e-12 and abs(z[2, 0].item() * n - 1) < 1e-12 and z[1].max().item() >= 1 - 1e-12


def test_softmax_margin_counts_the_kernels_operations():
    assert [R.softmax_c(nv) for nv in (1, 4, 16, 32)] == [19, 31, 79, 143]
    assert [R.softmax_nv(n) for n in (4, 1024, 1028, 4096, 4100, 16384, 16388, 32768)] == [1, 1, 4, 4, 16, 16, 32, 32]


def test_timestep_inputs_and_swapped_halves():
    vb, vf = R.timestep_inputs()
    assert vb.numel() == 1282 and vb[1].item() == 2.0 ** -10 and vb[-1].item() == 1.0 and vf.numel() == 1286
    freqs = R.timestep_freqs()
    for name, v in (("bf16", vb), ("fp32", vf)):
        alts, wide = R.timestep_accept(v, freqs)
        ang = (v.to(BF) * 1000).float()[:, None] * freqs[None]
        f32 = torch.cat([torch.cos(ang), torch.sin(ang)], dim=-1).to(BF)          # the float32 library functions of the host
        _check(f"timestep {name} float32 cos | sin", R.judge(f32, alts, wide), R.AMBIGUOUS_CAP["timestep"])
        assert not R.judge(torch.cat([f32[:, 128:], f32[:, :128]], dim=-1), alts, wide).ok
        assert not R.judge(f32, *R.timestep_accept(v, freqs, swap=True)).ok


def test_exact_restatements():
    g = torch.Generator().manual_seed(5)
    a, b, c = (torch.randn(4096, generator=g).to(BF) for _ in range(3))
    assert torch.equal(R.add3(a, b, c), ((a.float() + b.float()).to(BF).float() + c.float()).to(BF))
    s = 3.7
    s32 = torch.tensor(s, dtype=torch.float32)
    want = (b.float() + (s32 * (a.float() - b.float()).to(BF).float()).to(BF).float()).to(BF)
    assert torch.equal(R.true_cfg(a, b, s), want)
