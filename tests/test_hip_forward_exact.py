"""GPU: the forward small kernels (csrc/norm_kernels.hip, csrc/elementwise.hip) held to forward_ref's rule -- EVERY element must
be one of the bit patterns that a float64 evaluation of the kernel's one float32 stage, a stated margin and the exactly restated
rest allow -- on every instantiation, on strided views, into poisoned buffers.  The inputs are forward_ref's, the ones
tests/test_forward_ref.py holds to the ambiguity caps on the CPU.  Each case prints a [parity] line: the share of elements for
which the rule had a choice, the share of the others that is bit-equal, and the worst miss."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forward_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
POISON = -12352.0            # a bf16 value no kernel here produces


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


def _check(name, v, cap):
    print(v.line(name), flush=True)
    assert v.ok, v.line(name)
    assert v.ambiguous <= cap


def _poisoned(*shape, dtype=BF):
    return torch.full(shape, POISON, dtype=dtype, device="cuda")


def _untouched(t):
    return bool((t == POISON).all())


# ---- ln_modulate / ln_modulate2 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Rr", R.LN_BR)
@pytest.mark.parametrize("D", R.LN_DS)
def test_ln_modulate_every_element(ops, D, B, Rr):
    """x = the rows [S_TXT:] of a longer [B, S_TXT + R, D] buffer (the batched fk_rows form), the modulation vectors = chunks of
    one [B, 6 D] tensor, out = a view with ld = D + 64; one- and two-stream forms, every split."""
    buf, mod = R.ln_inputs(D, B, Rr)
    x = buf[:, R.LN_S_TXT:]
    lo, hi, wide = R.candidates(*R.ln_stage(x))
    bufd, modd = buf.cuda(), mod.cuda()
    xd = bufd[:, R.LN_S_TXT:]
    ch = [modd[:, i * D:(i + 1) * D] for i in range(6)]
    for split in R.ln_forms(Rr):
        obuf = _poisoned(B, Rr, D + 64)
        if split is None:
            ops.ln_modulate(xd, ch[0], ch[1], out=obuf[:, :, :D])
        else:
            ops.ln_modulate2(xd, ch[0], ch[1], ch[3], ch[4], split, out=obuf[:, :, :D])
        torch.cuda.synchronize()
        assert _untouched(obuf[:, :, D:]) and torch.equal(bufd.cpu(), buf) and torch.equal(modd.cpu(), mod)
        got = obuf[:, :, :D].cpu()
        shift, scale = R.ln_modulation(mod, D, split, Rr)
        v = R.judge(got, [R.ln_tail(lo, shift, scale), R.ln_tail(hi, shift, scale)], wide)
        _check(f"ln_modulate D={D} B={B} R={Rr} split={split}", v, R.AMBIGUOUS_CAP["ln"])
        if D in (512, 1024):
            # 1 / D is a power of two and D x is exact in float32 in any order: the constant row's mean is exact, its output shift
            assert torch.equal(got[0, 1], shift.expand(B, Rr, D)[0, 1])


# ---- qkv_post and the fused QKV epilogue -----------------------------------------------------------------------------------------
def _judge_qk(name, qkv, w, cos, sin, s_txt, q, k):
    for which, got in ((0, q), (1, k)):
        alts = R.qkv_accept(qkv, which, w[which], w[2 + which] if s_txt else None, cos, sin, s_txt)
        _check(f"{name} {'qk'[which]}", R.judge(got, alts, group=2), R.AMBIGUOUS_CAP["rms"])


@pytest.mark.parametrize("case", R.QKV_CASES)
def test_qkv_post_every_pair(ops, case):
    """RMSNorm + RoPE + re-layout: S not a multiple of 64; no text tokens and null text weights with S = 64; text only; and the
    H = 24 case on which a contracted rotation moves dozens of unambiguous elements (tests/test_forward_ref.py), so that no
    miss here means no fma in the rotation.  (Recorded once against the library built with the rotation as a product and an
    fma: 84 misses in q of the H = 24 case, worst 2 bf16 ulp; 4 in q of the first case; and the fused epilogue below no
    longer bit-identical to this kernel.)"""
    B, H, s_txt, hh, ww = case
    S = s_txt + hh * ww
    qkv, w, cos, sin = R.qkv_inputs(*case)
    qkvd, wd = qkv.cuda(), [t.cuda() for t in w]
    guard = 64 * 128
    qb, kb = _poisoned(B * H * S * 128 + guard), _poisoned(B * H * S * 128 + guard)
    q, k = qb[:B * H * S * 128].view(B, H, S, 128), kb[:B * H * S * 128].view(B, H, S, 128)
    ops.qkv_post(qkvd, q, k, wd[0], wd[1], wd[2] if s_txt else None, wd[3] if s_txt else None, cos.cuda(), sin.cuda(), s_txt)
    torch.cuda.synchronize()
    assert _untouched(qb[-guard:]) and _untouched(kb[-guard:])
    assert torch.equal(qkvd.cpu(), qkv)                      # V and the inputs are left alone
    _judge_qk(f"qkv_post {case}", qkv, w, cos, sin, s_txt, q.cpu(), k.cpu())


def test_fused_qkv_epilogue_at_24_heads(ops):
    """FK_EPI_QKV at N = 9216 (H = 24), K = 256, S = 70 + 32 x 33: the launch plan's own tile choice for the production width,
    as a grouped text + image launch -- bit-identical to the unfused projection followed by fk_qkv_post_bf16, and held to the
    rule itself on the projection it stored."""
    B, H, s_txt, hh, ww = R.QKV_LARGE
    S, D, K = s_txt + hh * ww, H * 128, 256
    _, w, cos, sin = R.qkv_inputs(*R.QKV_LARGE)
    g = torch.Generator().manual_seed(61)
    x = torch.randn(B, S, K, generator=g).to(BF).cuda()
    w_i, w_t = ((torch.randn(3 * D, K, generator=g) * 0.06).to(BF).cuda() for _ in range(2))
    b_i, b_t = ((torch.randn(3 * D, generator=g) * 0.1).to(BF).cuda() for _ in range(2))
    nw = [t.cuda() for t in w]                               # q_img k_img q_txt k_txt
    cosd, sind = cos.cuda(), sin.cuda()
    qkv_ref = torch.empty(B, S, 3 * D, dtype=BF, device="cuda")
    ops.gemm_grouped([dict(a=x[:, s_txt:], w=w_i, bias=b_i, out=qkv_ref[:, s_txt:]),
                      dict(a=x[:, :s_txt], w=w_t, bias=b_t, out=qkv_ref[:, :s_txt])])
    q_ref, k_ref = _poisoned(B, H, S, 128), _poisoned(B, H, S, 128)
    ops.qkv_post(qkv_ref, q_ref, k_ref, nw[0], nw[1], nw[2], nw[3], cosd, sind, s_txt)
    qkv, q, k = _poisoned(B, S, 3 * D), _poisoned(B, H, S, 128), _poisoned(B, H, S, 128)
    ops.gemm_grouped([dict(a=x[:, s_txt:], w=w_i, bias=b_i, out=qkv[:, s_txt:],
                           qkv=dict(q_out=q, k_out=k, wq=nw[0], wk=nw[1], cos=cosd, sin=sind, s_offset=s_txt)),
                      dict(a=x[:, :s_txt], w=w_t, bias=b_t, out=qkv[:, :s_txt],
                           qkv=dict(q_out=q, k_out=k, wq=nw[2], wk=nw[3], cos=cosd, sin=sind, s_offset=0))],
                     epilogue=ops.FK_EPI_QKV)
    torch.cuda.synchronize()
    print(f"[parity] fused QKV epilogue H={H}: launch form {ops.gemm_last_variant()}", flush=True)
    assert torch.equal(q, q_ref) and torch.equal(k, k_ref)
    assert torch.equal(qkv[:, :, 2 * D:], qkv_ref[:, :, 2 * D:])          # V third stored in place
    _judge_qk("fused QKV epilogue H=24", qkv_ref.cpu(), w, cos, sin, s_txt, q.cpu(), k.cpu())


# ---- softmax_rows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SOFTMAX_NS)
def test_softmax_rows_every_element(ops, n):
    """every instantiation on both sides of its threshold (NV = 1, 4, 16, 32), row strides larger than n on both sides."""
    x = R.softmax_inputs(n)
    xb = torch.zeros(3, n + 12, device="cuda")
    xb[:, :n] = x.cuda()
    yb = _poisoned(3, n + 20)
    ops.softmax_rows(xb[:, :n], out=yb[:, :n])
    torch.cuda.synchronize()
    assert _untouched(yb[:, n:]) and torch.equal(xb[:, :n].cpu(), x)
    alts, wide, tiny = R.softmax_accept(x)
    nv = R.softmax_nv(n)
    print(f"[parity] softmax_rows n={n}: NV={nv} c={R.softmax_c(nv)} below-normal share {tiny.float().mean().item():.3f}", flush=True)
    _check(f"softmax_rows n={n}", R.judge(yb[:, :n].cpu(), alts, wide, bounded=tiny),
           R.AMBIGUOUS_CAP["softmax_nv32" if nv == 32 else "softmax"])


# ---- timestep_proj ---------------------------------------------------------------------------------------------------------------
def test_timestep_proj_every_bf16_timestep(ops):
    vb, vf = R.timestep_inputs()
    freqs = R.timestep_freqs()
    for name, v in (("bf16", vb), ("fp32", vf)):
        ob = _poisoned(v.numel() + 1, 256)
        ops.timestep_proj(v.cuda(), freqs.cuda(), out=ob[:-1])
        torch.cuda.synchronize()
        assert _untouched(ob[-1])
        alts, wide = R.timestep_accept(v, freqs)
        _check(f"timestep_proj {name}", R.judge(ob[:-1].cpu(), alts, wide), R.AMBIGUOUS_CAP["timestep"])


# ---- transpose -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,Rr,C", [(2, 64, 64), (1, 63, 65), (3, 70, 130), (1, 1, 200), (1, 200, 1)])
def test_transpose_strided_views(ops, batch, Rr, C):
    g = torch.Generator().manual_seed(400 + Rr + C)
    sbuf = torch.randn(batch, Rr + 2, C + 5, generator=g).to(BF)
    dbuf = _poisoned(batch, C + 1, Rr + 7)
    sd = sbuf.cuda()
    ops.transpose(sd[:, 1:Rr + 1, 3:3 + C], dbuf[:, :C, 2:2 + Rr])
    torch.cuda.synchronize()
    want = torch.full((batch, C + 1, Rr + 7), POISON, dtype=BF)
    want[:, :C, 2:2 + Rr] = sbuf[:, 1:Rr + 1, 3:3 + C].transpose(1, 2)
    assert torch.equal(dbuf.cpu(), want) and torch.equal(sd.cpu(), sbuf)


# ---- silu, add3, true_cfg past the grid cap --------------------------------------------------------------------------------------
N_EW = 4096 * 2048 + 8 * 259     # the grid is capped at 4096 blocks of 2048 elements: the second trip is partly filled
H_EW = 4096 * 1024 + 8 * 131     # a 16-byte aligned cut; both halves fit one trip


def _ew_inputs(k):
    g = torch.Generator().manual_seed(500)
    return [(torch.randn(N_EW, generator=g) * s).to(BF) for s in (3.0, 1.0, 0.7)[:k]]


def _whole_and_halves(fn, ts):
    """fn(*tensors, out=) on the whole length into a poisoned buffer, and the same kernel on the two halves."""
    ob = _poisoned(N_EW + 64)
    fn(*ts, out=ob[:N_EW])
    ha, hb = _poisoned(H_EW + 64), _poisoned(N_EW - H_EW + 64)
    fn(*[t[:H_EW] for t in ts], out=ha[:H_EW])
    fn(*[t[H_EW:] for t in ts], out=hb[:N_EW - H_EW])
    torch.cuda.synchronize()
    assert _untouched(ob[N_EW:]) and _untouched(ha[H_EW:]) and _untouched(hb[N_EW - H_EW:])
    assert torch.equal(ob[:H_EW], ha[:H_EW]) and torch.equal(ob[H_EW:N_EW], hb[:N_EW - H_EW])
    return ob[:N_EW].cpu()


def test_silu_second_grid_stride_trip(ops):
    (x,) = _ew_inputs(1)
    got = _whole_and_halves(ops.silu, [x.cuda()])
    assert torch.isfinite(got.float()).all() and not (got == POISON).any()


def test_add3_second_grid_stride_trip(ops):
    a, b, c = _ew_inputs(3)
    got = _whole_and_halves(ops.add3, [a.cuda(), b.cuda(), c.cuda()])
    assert torch.equal(got, R.add3(a, b, c))


def test_true_cfg_second_grid_stride_trip(ops):
    pos, neg = _ew_inputs(2)
    got = _whole_and_halves(lambda p, n, out: ops.true_cfg(p, n, 3.7, out=out), [pos.cuda(), neg.cuda()])
    assert torch.equal(got, R.true_cfg(pos, neg, 3.7))
