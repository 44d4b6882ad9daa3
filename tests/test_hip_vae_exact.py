"""The VAE kernels (csrc/vae_kernels.hip, csrc/vae_attention.hip, csrc/conv_halo.hip, the implicit-GEMM convolution) against fp64
at the extents the decoder runs them at: GroupNorm finalize with more than 64 blocks and at the 512-block cap, every elementwise
kernel past its first grid-stride trip (more than 8192 x 256 work items), attention_hd512 at S edges / scales / S = 16384, and the
convolutions bounded on every element at ragged extents.  tests/vae_ref.py holds the references and derives the bounds;
tests/test_vae_ref.py checks them on the CPU.

Observed on an MI355X (the [parity] / [rows] lines print them on every run): GroupNorm statistics use 0.010 - 0.119 of the mean
bound and 0.0002 - 0.056 of the rstd bound (ill-conditioned groups, |mean| / std = 32 - 47: at most 0.036 of a bound of ~1e-2
relative) and equal the numpy emulation of the summation order bit for bit in all twelve bf16 cases; GroupNorm-apply reaches
1 ulp / 0.91 of the SiLU bound; attention_hd512 needs 0.37 - 0.97 of the model's own rho (MARGIN 2 never approached; worst at
scale 0.125, 0.85 at S = 16384); the bf16 convolutions reach 0.92 - 0.99 of the per-element cap, as the oracle's own bf16
evaluation does (the cap is one half-ulp at the bottom of a binade)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar
import vae_ref as vr
from conftest import bf16_ulp_diff, report

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64


def _skip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- 1. GroupNorm statistics ------------------------------------------------------------------------------------------------
def _f32_twin_stats(ops, x32):
    """fk_groupnorm_f32_nhwc keeps its statistics in the per-shape buffer group_norm_stats shares: read them from there."""
    from gpt_image_edit_amd import libfk
    B, HW, C = x32.shape
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    ops.group_norm_f32_parts(x32, one, zero, False, 2)
    torch.cuda.synchronize()
    return ops._gn_workspace(libfk.load(), B, HW, C, x32.device)[1].clone()


@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("C,HW", vr.GN_CASES)
def test_group_norm_stats_against_fp64(C, HW, kind):
    """(mean, rstd) of the bf16 kernel and of its fp32 twin within the bound vae_ref derives from the summation order, per
    (batch, group); nblk = 66 / 129 (second finalize iteration for some lanes only), the 512 cap with a ragged per_blk, fewer
    pixels than one iteration, C = 1024.  Ill-conditioned groups (|mean| / std up to 32): the printed ratios are the share of
    the cancellation bound the kernels use."""
    _skip()
    from gpt_image_edit_amd import ops
    x32 = vr.gn_data(C, HW, kind)
    xb = x32.to(BF)
    st = ops.group_norm_stats(xb.cuda()).clone()
    vr.gn_check_stats(f"group_norm_stats {kind}", st, xb, C, HW)
    emu = vr.gn_emulate(xb)
    print(f"[parity] group_norm_stats {kind} C={C} HW={HW}: bit-equal to the emulated summation order: {torch.equal(st.cpu(), emu)}")
    st32 = _f32_twin_stats(ops, x32.cuda())
    vr.gn_check_stats(f"group_norm_f32 stats {kind}", st32, x32, C, HW)


@pytest.mark.parametrize("C,HW", vr.GN_CAPPED)
def test_group_norm_stats_repeat_bit_identical(C, HW):
    _skip()
    from gpt_image_edit_amd import ops
    x = vr.gn_data(C, HW, "ill").to(BF).cuda()
    runs = [ops.group_norm_stats(x).clone() for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    x32 = vr.gn_data(C, HW, "ill").cuda()
    runs = [_f32_twin_stats(ops, x32) for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


# ---- 2. GroupNorm apply -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("B,C,HW", [(1, 128, 131072 + 517), (2, 512, 999)])
def test_group_norm_apply_every_element(B, C, HW, silu):
    """gn_apply_kernel against fp64 from the kernel's OWN statistics (the apply on its own), every element bounded; HW = 131589
    at C = 128 is 16 x 131589 > 8192 x 256 vectors: the last 517 x 16 are written in the second grid-stride trip."""
    _skip()
    from gpt_image_edit_amd import ops
    assert B == 2 or HW * (C // 8) > vr.EW_ONE_TRIP
    g = torch.Generator().manual_seed(C + HW)
    x = (torch.randn(B, HW, C, generator=g) * 1.5 + torch.linspace(-2, 2, C)[None, None, :]).to(BF)
    if B == 2:
        x[1] = (x[1].float() * 0.5 + 1.0).to(BF)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(BF), (0.1 * torch.randn(C, generator=g)).to(BF)
    xd = x.cuda()
    out = torch.full_like(xd, float("nan"))
    ops.group_norm_nhwc(xd, gamma.cuda(), beta.cuda(), silu, out=out)
    stats = ops.group_norm_stats(xd).clone().cpu()         # same input, same shape: the statistics the apply just read
    t64 = vr.gn_apply64(x, stats, gamma, beta)
    vr.gn_check_apply(f"group_norm apply B={B} C={C} HW={HW} silu={silu}", out, t64, silu)


@pytest.mark.parametrize("parts", [2, 3])
def test_group_norm_f32_parts_second_trip(parts):
    """gn_apply_f32_kernel: C = 128, HW = 66053: 32 x 66053 > 8192 x 256 vectors.  hi + lo against fp64 GroupNorm + SiLU at the
    fp32-class tolerance on every element; the third part repeats the first."""
    _skip()
    from gpt_image_edit_amd import ops
    C, HW = 128, 65536 + 517
    assert HW * (C // 4) > vr.EW_ONE_TRIP
    g = torch.Generator().manual_seed(70 + parts)
    a = torch.randn(1, HW, C, generator=g) * 2 + 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.1
    yp = ops.group_norm_f32_parts(a.cuda(), gamma.cuda(), beta.cuda(), True, parts).cpu()
    got = yp[..., :C].float() + yp[..., C:2 * C].float()
    ref = F.silu(F.group_norm(a.double().permute(0, 2, 1), 32, gamma.double(), beta.double(), eps=1e-6)).permute(0, 2, 1).float()
    report(f"fp32 GroupNorm+SiLU parts={parts} second trip", got, ref)
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
    if parts == 3:
        assert torch.equal(yp[..., 2 * C:], yp[..., :C])


# ---- 3. layout and pixel kernels: second trip, exact -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_nchw_to_nhwc_second_trip(dtype):
    _skip()
    from gpt_image_edit_amd import ops
    from oracle import vae as ovae
    C, Cpad, H, W = 16, 32, 257, 259
    assert H * W * Cpad > vr.EW_ONE_TRIP
    z = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(81)).to(dtype)
    got = ops.nchw_to_nhwc(z.cuda(), Cpad, 0.3611, 0.1159).cpu()
    ref = ovae.unscale_latents(z.to(BF))
    assert torch.equal(got[..., :C], ref.permute(0, 2, 3, 1))
    assert not got[..., C:].any(), "padding channels must be zero"


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_nhwc_to_nchw_second_trip(dtype):
    _skip()
    from gpt_image_edit_amd import ops
    from oracle import vae as ovae
    C, Cpad, H, W = 16, 32, 363, 365
    assert H * W * C > vr.EW_ONE_TRIP
    y = torch.randn(1, H, W, Cpad, generator=torch.Generator().manual_seed(82)).to(BF)
    got = ops.nhwc_to_nchw(y.cuda(), C, -0.1159, 0.3611, dtype=dtype).cpu()
    ref = ovae._scalar_op(ovae._scalar_op(y[..., :C].permute(0, 3, 1, 2), "add", -0.1159), "mul", 0.3611)
    assert got.dtype == dtype and torch.equal(got, ref.to(dtype))


def test_pixels_u8_to_nhwc_second_trip():
    _skip()
    from gpt_image_edit_amd import ops
    from oracle import vae as ovae
    hout, wout = 257, 259
    assert hout * wout * 32 > vr.EW_ONE_TRIP
    u8 = torch.randint(0, 256, (2, 200, 131, 3), generator=torch.Generator().manual_seed(83), dtype=torch.uint8)
    got = ops.pixels_to_nhwc(u8.cuda(), hout, wout, 32, renorm=False).cpu()
    ref = ovae.preprocess_uint8(u8, hout, wout)
    assert torch.equal(got[..., :3].permute(0, 3, 1, 2), ref)
    assert not got[..., 3:].any(), "padding channels must be zero"


@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_image_to_u8_second_trip(dtype):
    _skip()
    from gpt_image_edit_amd import ops
    from oracle import vae as ovae
    H, W = 837, 839
    assert H * W * 3 > vr.EW_ONE_TRIP
    img = (torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(84)) * 0.8).to(dtype)
    got = ops.image_to_u8(img.cuda()).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, ovae.postprocess_uint8(img))


def _parts(x):
    hi = x.to(BF)
    return hi, (x - hi.float()).to(BF)


@pytest.mark.parametrize("parts,weight_order", [(3, False), (3, True), (2, False)])
def test_split_f32_rows_second_trip(parts, weight_order):
    _skip()
    from gpt_image_edit_amd import ops
    rows, n, ldx, ps = 131072 + 37, 64, 72, 72
    assert rows * (n // 4) > vr.EW_ONE_TRIP
    xw = torch.randn(rows, ldx, generator=torch.Generator().manual_seed(85)) * 3
    out = torch.zeros(rows, parts * ps, dtype=BF, device="cuda")
    ops.split_f32_rows(xw.cuda()[:, :n], out, parts=parts, weight_order=weight_order)
    o = out.cpu()
    hi, lo = _parts(xw[:, :n])
    want = [hi, lo] if parts == 2 else ([hi, hi, lo] if weight_order else [hi, lo, hi])
    for p, w in enumerate(want):
        assert torch.equal(o[:, p * ps:p * ps + n], w), f"part {p}"
        assert not o[:, p * ps + n:(p + 1) * ps].any(), "columns between the parts must stay untouched"


@pytest.mark.parametrize("parts", [2, 3])
def test_nchw_f32_to_nhwc_parts_second_trip(parts):
    _skip()
    from gpt_image_edit_amd import ops
    C, Cpad, H, W = 3, 32, 257, 259
    assert H * W * Cpad > vr.EW_ONE_TRIP
    x = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(86))
    got = ops.nchw_f32_to_nhwc_parts(x.cuda(), Cpad, parts).cpu()
    hi, lo = _parts(x.permute(0, 2, 3, 1))
    for p, w in enumerate([hi, lo, hi][:parts]):
        assert torch.equal(got[..., p * Cpad:p * Cpad + C], w), f"part {p}"
        assert not got[..., p * Cpad + C:(p + 1) * Cpad].any(), "padding channels must be zero"


def test_nhwc_f32_to_nchw_second_trip():
    _skip()
    from gpt_image_edit_amd import ops
    C, Cpad, H, W = 16, 32, 363, 365
    assert H * W * C > vr.EW_ONE_TRIP
    y = torch.randn(1, H, W, Cpad, generator=torch.Generator().manual_seed(87))
    got = ops.nhwc_f32_to_nchw(y.cuda(), C, -0.1159, 0.3611).cpu()
    add, mul = torch.tensor(-0.1159, dtype=torch.float32), torch.tensor(0.3611, dtype=torch.float32)
    assert torch.equal(got, ((y[..., :C] + add) * mul).permute(0, 3, 1, 2))


# ---- 4. attention_hd512 --------------------------------------------------------------------------------------------------------
def _run_hd512(ops, q, k, v, scale=None, framed=False):
    """The kernel on q, k, v [B, S, 512].  framed: q | k | v as column blocks of one [B, S + 3, 1544] buffer (batch stride above
    S ld, NaN in every row and column the kernel must not read) and the output inside a [B, S + 4, 516] buffer, 4 guard columns
    left of every row and 2 guard rows above and below, all of which must come back untouched."""
    B, S, _ = q.shape
    if not framed:
        out = ops.attention_hd512(q.cuda(), k.cuda(), v.cuda(), scale=scale)
        torch.cuda.synchronize()
        return out.cpu()
    buf = torch.full((B, S + 3, 1536 + 8), float("nan"), dtype=BF)
    buf[:, :S, :512], buf[:, :S, 512:1024], buf[:, :S, 1024:1536] = q, k, v
    d = buf.cuda()
    frame = torch.full((B, S + 4, 516), 7.0, dtype=BF, device="cuda")
    view = frame[:, 2:S + 2, 4:]
    assert view.stride(1) == 516 and d.stride(1) == 1544 and d.stride(0) > S * 1544
    ops.attention_hd512(d[:, :S, :512], d[:, :S, 512:1024], d[:, :S, 1024:1536], out=view, scale=scale)
    torch.cuda.synchronize()
    out = view.cpu().clone()
    view.fill_(7.0)
    assert bool((frame == 7.0).all()), "the kernel wrote outside its output rows"
    return out


@pytest.mark.parametrize("S", [1, 2, 31, 32, 33, 63, 64, 65, 95, 127, 129, 257])
def test_attention_hd512_s_edges(S):
    """Every row against fp64 within MARGIN x the rounding model's own error: one ragged key tile (S < 32), key tile and query
    block boundaries +-1, strided q | k | v and output with guards."""
    _skip()
    from gpt_image_edit_amd import ops
    q, k, v = vr.hd512_inputs(2, S, seed=500 + S)
    got = _run_hd512(ops, q, k, v, framed=True)
    ref, mod = vr.hd512_ref_and_model(q, k, v, 512 ** -0.5)
    r = ar.assert_rows_close(f"attention_hd512 S={S}", got[:, None], ref, mod)
    print(f"[parity] attention_hd512 S={S}: rho={r['rho']:.3e} observed/model={r['ratio']:.3f}")


@pytest.mark.parametrize("scale", [None, 0.01, 0.125])
def test_attention_hd512_scale(scale):
    _skip()
    from gpt_image_edit_amd import ops
    S = 300
    q, k, v = vr.hd512_inputs(2, S, seed=800)
    got = _run_hd512(ops, q, k, v, scale=scale)
    ref, mod = vr.hd512_ref_and_model(q, k, v, 512 ** -0.5 if scale is None else scale)
    r = ar.assert_rows_close(f"attention_hd512 S={S} scale={scale}", got[:, None], ref, mod)
    print(f"[parity] attention_hd512 S={S} scale={scale}: rho={r['rho']:.3e} observed/model={r['ratio']:.3f}")


def test_attention_hd512_matched_keys():
    """S = 1000 (ragged key tile and query block) with a matched key for a third of the queries, anywhere in the sequence."""
    _skip()
    from gpt_image_edit_amd import ops
    S = 1000
    q, k, v = vr.hd512_inputs(2, S, seed=801)
    got = _run_hd512(ops, q, k, v)
    ref, mod = vr.hd512_ref_and_model(q, k, v, 512 ** -0.5)
    r = ar.assert_rows_close(f"attention_hd512 matched S={S}", got[:, None], ref, mod)
    print(f"[parity] attention_hd512 matched S={S}: rho={r['rho']:.3e} observed/model={r['ratio']:.3f}")


def test_attention_hd512_one_hot_selects_exact_value_rows():
    """One-hot attention (a decisive matching logit) copies exactly the selected V row: p = 1 for one key and exactly 0 for the
    others, so any slip of the key <-> k-slot binding of the transpose reads shows as a wrong row or column."""
    _skip()
    from gpt_image_edit_amd import ops
    S = 96
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(3))
    q, k = torch.zeros(1, S, 512), torch.zeros(1, S, 512)
    for i in range(S):
        q[0, i, 5 * i + 3] = 12.0
        k[0, perm[i], 5 * i + 3] = 12.0
    v = ((torch.arange(S * 512, dtype=torch.float32).reshape(1, S, 512) % 251) / 16.0 - 7.0).to(BF)    # exact in bf16
    got = _run_hd512(ops, q.to(BF), k.to(BF), v, scale=8.0)
    assert torch.equal(got[0], v[0, perm])


def test_attention_hd512_1024sq_length():
    """S = 16384, the mid block of a 1024^2 image: 256 rows against fp64 (the first, a middle and the last query block, and a
    spread in between), every row finite, two runs bit-equal."""
    _skip()
    from gpt_image_edit_amd import ops
    S = 16384
    q, k, v = vr.hd512_inputs(1, S, seed=802)
    d = [t.cuda() for t in (q, k, v)]
    a = ops.attention_hd512(*d)
    b = ops.attention_hd512(*d)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    rows = torch.cat([torch.arange(0, 64), torch.arange(8192, 8256), torch.arange(S - 64, S), torch.arange(97, S, 251)[:64]])
    assert len(rows) == 256
    ref, mod = vr.hd512_ref_and_model(q, k, v, 512 ** -0.5, rows=rows)
    r = ar.assert_rows_close(f"attention_hd512 S={S} (256 rows)", a.cpu()[:, rows][:, None], ref, mod)
    print(f"[parity] attention_hd512 S={S}: rho={r['rho']:.3e} observed/model={r['ratio']:.3f}")


# ---- 5. convolutions -------------------------------------------------------------------------------------------------------------
def _conv_operands(cin, cout, h, w, ks, seed):
    """Two batch entries with different data and different GroupNorm statistics."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, cin, h, w, generator=g) * 1.3 + torch.linspace(-1, 1, cin)[None, :, None, None]
    x[1] = x[1] * 0.6 + 1.5
    wt = (torch.randn(cout, cin, ks, ks, generator=g) * 0.03).to(BF)
    bias = (torch.randn(cout, generator=g) * 0.1).to(BF)
    gamma, beta = (1 + 0.1 * torch.randn(cin, generator=g)).to(BF), (0.1 * torch.randn(cin, generator=g)).to(BF)
    return x.to(BF), wt, bias, gamma, beta


@pytest.mark.parametrize("cin,cout,h,w,mode", [(128, 64, 17, 33, "gn"), (512, 256, 17, 33, "gn"), (512, 128, 15, 16, "plain"),
                                               (128, 256, 15, 16, "plain"), (128, 128, 9, 7, "up"), (512, 64, 9, 7, "up")])
def test_conv3x3_halo_f32_ragged_batch(cin, cout, h, w, mode):
    """fk_conv3x3_halo_f32_debug at B = 2 and extents off the 16 x 16 tile both ways, against fp64 F.conv2d on the HIP-normalised
    operand: rtol 1e-3 / atol 1e-4 on every element."""
    _skip()
    from gpt_image_edit_amd import ops
    from gpt_image_edit_amd.vae import _pack_conv
    x, wt, bias, gamma, beta = _conv_operands(cin, cout, h, w, 3, seed=cin + cout + h)
    gn, up = mode == "gn", mode == "up"
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()
    wp = _pack_conv(wt.cuda())
    gn_arg = (ops.group_norm_stats(x_nhwc), gamma.cuda(), beta.cuda(), True) if gn else None
    got = ops.conv3x3_halo(x_nhwc, wp, bias.cuda(), cout, upsample2x=up, gn=gn_arg, out_fp32=True)
    xn = ops.group_norm_nhwc(x_nhwc, gamma.cuda(), beta.cuda(), True) if gn else x_nhwc
    torch.cuda.synchronize()
    xin = xn.permute(0, 3, 1, 2).cpu().double()
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, wt.double(), bias.double(), padding=1).float()
    g = got.permute(0, 3, 1, 2).cpu()
    report(f"conv3x3_halo f32 B=2 {mode} {cin}->{cout} {h}x{w}", g, ref)
    torch.testing.assert_close(g, ref, rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("cin,cout,h,w,mode", [(128, 128, 9, 7, "s1"), (128, 128, 11, 9, "s2"), (512, 256, 5, 5, "1x1"),
                                               (256, 128, 7, 5, "up"), (128, 8, 13, 11, "s1")])
def test_conv_nhwc_every_element(cin, cout, h, w, mode):
    """conv2d_nhwc: the fraction bounds of test_conv_nhwc plus the per-element cap of vae_ref.conv_ref_and_cap, with and without
    a residual."""
    _skip()
    from gpt_image_edit_amd import ops
    from gpt_image_edit_amd.vae import _pack_conv
    ks = 1 if mode == "1x1" else 3
    x, wt, bias, _, _ = _conv_operands(cin, cout, h, w, ks, seed=cin + h)
    ref64, cap = vr.conv_ref_and_cap(x, wt, bias, mode)
    res = torch.randn(*ref64.shape, generator=torch.Generator().manual_seed(4)).to(BF)
    ref64r, capr = vr.conv_ref_and_cap(x, wt, bias, mode, res=res)
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()
    wp = _pack_conv(wt.cuda())
    kw = dict(ksize=ks, stride=2 if mode == "s2" else 1, pad=0 if mode in ("s2", "1x1") else 1, upsample2x=(mode == "up"))
    got = ops.conv2d_nhwc(x_nhwc, wp, bias.cuda(), cout, **kw)
    got_r = ops.conv2d_nhwc(x_nhwc, wp, bias.cuda(), cout, res=res.permute(0, 2, 3, 1).contiguous().cuda(), **kw)
    torch.cuda.synchronize()
    got, got_r = got.permute(0, 3, 1, 2).cpu(), got_r.permute(0, 3, 1, 2).cpu()
    y_bf = (ref64r - res.double()).to(BF)
    assert (bf16_ulp_diff(got, y_bf) > 1).float().mean().item() < 1e-3
    assert (bf16_ulp_diff(got_r, res + y_bf) > 1).float().mean().item() < 2e-3
    vr.check_cap(f"conv2d_nhwc {mode} {cin}->{cout} {h}x{w}", got, ref64, cap)
    vr.check_cap(f"conv2d_nhwc {mode} {cin}->{cout} {h}x{w} + res", got_r, ref64r, capr)


@pytest.mark.parametrize("cin,cout,h,w,mode", [(128, 128, 17, 33, "gn+res"), (512, 256, 9, 7, "up"), (256, 64, 15, 16, "plain+res")])
def test_conv3x3_halo_every_element(cin, cout, h, w, mode):
    """conv3x3_halo (bf16 output) on the HIP-normalised operand: the fraction bounds of test_conv3x3_halo plus the per-element
    cap."""
    _skip()
    from gpt_image_edit_amd import ops
    from gpt_image_edit_amd.vae import _pack_conv
    x, wt, bias, gamma, beta = _conv_operands(cin, cout, h, w, 3, seed=cin + cout + w)
    gn, up, with_res = "gn" in mode, "up" in mode, "res" in mode
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().cuda()
    wp = _pack_conv(wt.cuda())
    xn = ops.group_norm_nhwc(x_nhwc, gamma.cuda(), beta.cuda(), True) if gn else x_nhwc
    xin = xn.permute(0, 3, 1, 2).cpu()
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    res = torch.randn(2, cout, ho, wo, generator=torch.Generator().manual_seed(16)).to(BF) if with_res else None
    ref64, cap = vr.conv_ref_and_cap(xin, wt, bias, "up" if up else "s1", res=res)
    gn_arg = (ops.group_norm_stats(x_nhwc), gamma.cuda(), beta.cuda(), True) if gn else None
    got = ops.conv3x3_halo(x_nhwc, wp, bias.cuda(), cout, upsample2x=up, gn=gn_arg,
                           res=res.permute(0, 2, 3, 1).contiguous().cuda() if with_res else None)
    torch.cuda.synchronize()
    g = got.permute(0, 3, 1, 2).cpu()
    want = (res + (ref64 - res.double()).to(BF)) if with_res else ref64.to(BF)
    assert (bf16_ulp_diff(g, want) > 1).float().mean().item() < 4e-3
    assert (g.float() - want.float()).abs().max().item() <= 2e-2 * want.float().abs().max().item()
    vr.check_cap(f"conv3x3_halo {mode} {cin}->{cout} {h}x{w}", g, ref64, cap)
