"""MXFP8 path on the GPU: the quantizer bit for bit against the numpy reference, the block-scaled GEMM's fp32 parity build
against the fp32 product of the dequantized operands (rtol 1e-3 / atol 1e-4) on every cfg 2 block GEMM shape, and its bf16
epilogues against the same epilogue applied in fp32 to that product."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mxfp8_ref as ref
from conftest import bf16_ulp_diff, report

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def quant_ref(x):
    return ref.quantize(x.float().cpu().double().numpy().reshape(-1, x.shape[-1]))


def dequant_dev(q, s):
    """fp32 dequantization on the device (exact: e4m3 value times a power of two)."""
    lut = torch.from_numpy(np.nan_to_num(ref.e4m3_decode(np.arange(256)), nan=np.nan)).float().to(q.device)
    sc = torch.ldexp(torch.ones((), device=q.device), s.int() - 127)
    return lut[q.long()] * sc.repeat_interleave(32, dim=1)


def edge_rows():
    """Rows of 32-element blocks that hit every quantizer edge (see tests/test_mxfp8_host.py)."""
    rows = [
        [256.0, 1.0625, 1.1875, 1.03125, -1.0625],
        [480.0, 464.0, 508.0, 448.0, 416.0, -480.0],
        [2.0 ** -20], [1.9921875 * 2.0 ** 5], [2.0 ** -130], [-0.0], [],
        [256.0, 2.0 ** -7, 2.0 ** -9, 0.75 * 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 7.5 * 2.0 ** -9, 2.0 ** -11],
        [1.0, float("inf")], [float("nan")], [-float("inf"), 3.0], [3.0e38, -1.0],
    ]
    x = torch.zeros(len(rows), 32, dtype=BF)
    for i, r in enumerate(rows):
        if r:
            x[i, :len(r)] = torch.tensor(r).to(BF)
    return x.reshape(2, -1) if len(rows) % 2 == 0 else x.reshape(1, -1)


def test_quantizer_matches_reference_random_and_edges(ops):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(300, 1024, generator=g) * torch.logspace(-30, 30, 300).unsqueeze(1)).to(BF)
    e = edge_rows()
    x[:e.shape[0], :e.shape[1]] = e
    q, s = ops.quantize_mxfp8(x.cuda())
    torch.cuda.synchronize()
    rq, rs = quant_ref(x)
    assert np.array_equal(s.cpu().numpy(), rs)
    assert np.array_equal(q.cpu().numpy(), rq)


def test_quantizer_on_strided_joint_slices(ops):
    """Text / image slices of a joint [B, S, ld] buffer with B = 2 (fk_rows batch strides)."""
    B, S_txt, S_img, D, ld = 2, 37, 300, 3072, 3072 + 64
    buf = randn(B, S_txt + S_img, ld, seed=5).cuda()
    for sl in (slice(0, S_txt), slice(S_txt, S_txt + S_img)):
        view = buf[:, sl, :D]
        q, s = ops.quantize_mxfp8(view)
        rq, rs = quant_ref(view.contiguous())
        assert np.array_equal(q.cpu().numpy(), rq) and np.array_equal(s.cpu().numpy(), rs)


@pytest.mark.parametrize("N,K", [(9216, 3072), (3072, 3072), (12288, 3072), (3072, 12288), (21504, 3072), (3072, 15360)])
def test_quantizer_on_block_weight_shapes(ops, N, K):
    w = randn(N, K, seed=N + K, scale=0.02).cuda()
    q, s = ops.quantize_mxfp8(w)
    rq, rs = quant_ref(w)
    assert np.array_equal(s.cpu().numpy(), rs)
    assert np.array_equal(q.cpu().numpy(), rq)


def test_quantizer_rejects_bad_shapes(ops):
    with pytest.raises(RuntimeError, match="K % 32"):
        ops.quantize_mxfp8(torch.zeros(4, 48, dtype=BF, device="cuda"))


def _operands(ops, M, N, K, seed):
    a = randn(M, K, seed=seed, scale=0.5).cuda()
    w = randn(N, K, seed=seed + 1, scale=0.02).cuda()
    bias = randn(N, seed=seed + 2, scale=0.1).cuda()
    return ops.quantize_mxfp8(a), ops.quantize_mxfp8(w), bias


def _ref_product(aq, wq, bias):
    return dequant_dev(*aq) @ dequant_dev(*wq).T + bias.float()


def assert_f32_close(name, got, want):
    report(name, got, want)
    bad = ((got - want).abs() > 1e-4 + 1e-3 * want.abs()).float().mean().item()
    print(f"[parity] {name}: frac outside rtol 1e-3 / atol 1e-4 = {bad:.2e}", flush=True)
    assert bad == 0.0


# cfg 2 block GEMMs: M = 2560 image, 512 text, 3072 single-block rows
@pytest.mark.parametrize("M,N,K", [(2560, 9216, 3072), (2560, 3072, 3072), (2560, 12288, 3072), (2560, 3072, 12288),
                                   (512, 9216, 3072), (512, 3072, 12288), (3072, 21504, 3072), (3072, 3072, 15360)])
def test_gemm_mxfp8_fp32_parity(ops, M, N, K):
    aq, wq, bias = _operands(ops, M, N, K, seed=M + N + K)
    want = _ref_product(aq, wq, bias)
    outs = []
    for variant in (0, 128, 256):
        got = ops.gemm_mxfp8(aq, wq, bias, out_fp32=True, variant=variant)
        torch.cuda.synchronize()
        assert_f32_close(f"mxfp8 f32 M{M} N{N} K{K} v{variant} ({ops.gemm_last_variant()})", got, want)
        outs.append(got)
    assert torch.equal(outs[1], outs[2])          # both tile widths accumulate in the same order: identical bits


def test_gemm_mxfp8_ragged_m_and_grouped(ops):
    N, K = 3072, 3072
    aq, wq, bias = _operands(ops, 777, N, K, seed=7)
    got = ops.gemm_mxfp8(aq, wq, bias, out_fp32=True)
    assert_f32_close("mxfp8 f32 ragged M 777", got, _ref_product(aq, wq, bias))
    # grouped img + txt pair: different weights, different rows
    ai, wi, bi = _operands(ops, 2560, N, K, seed=8)
    at, wt, bt = _operands(ops, 512, N, K, seed=9)
    outs = ops.gemm_mxfp8_grouped([dict(a=ai, w=wi, bias=bi), dict(a=at, w=wt, bias=bt)], out_fp32=True)
    assert_f32_close("mxfp8 f32 grouped img", outs[0], _ref_product(ai, wi, bi))
    assert_f32_close("mxfp8 f32 grouped txt", outs[1], _ref_product(at, wt, bt))


def test_gemm_mxfp8_operand_and_scale_lane_maps(ops):
    """Exact small-integer data, distinct scales per (row, block) and an asymmetric W: any transposed or permuted operand,
    scale or accumulator lane map changes the exact result."""
    M, N, K = 256, 256, 256
    g = torch.Generator().manual_seed(11)
    a = torch.randint(-8, 9, (M, K), generator=g).float() * torch.ldexp(torch.ones(M, K // 32), torch.randint(-2, 3, (M, K // 32), generator=g)).repeat_interleave(32, 1)
    w = torch.randint(-8, 9, (N, K), generator=g).float() * torch.ldexp(torch.ones(N, K // 32), torch.randint(-2, 3, (N, K // 32), generator=g)).repeat_interleave(32, 1)
    w[:, 0] += torch.arange(N).float() % 7      # asymmetric
    aq, wq = ops.quantize_mxfp8(a.to(BF).cuda()), ops.quantize_mxfp8(w.to(BF).cuda())
    want = (dequant_dev(*aq).double() @ dequant_dev(*wq).double().T).float()
    got = ops.gemm_mxfp8(aq, wq, None, out_fp32=True)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def _ulp_check(name, got, want, frac=1e-4):
    got = got.cpu()
    want = want.cpu()
    report(name, got, want)
    ulp = bf16_ulp_diff(got, want)
    bad = (ulp > 1).float().mean().item()
    print(f"[parity] {name}: frac(>1ulp)={bad:.2e} max_ulp={int(ulp.max())}", flush=True)
    assert not torch.isnan(got.float()).any() and bad <= frac


def test_gemm_mxfp8_bf16_epilogues(ops):
    """The bf16 epilogues applied to the main loop's own fp32 result (out_fp32 = 2 runs the same accumulation): NONE is
    bf16(acc + bias) exactly; GELU_TANH / GATE_RES within 1 ulp on >= 99.99 % of the fp32-evaluated epilogue.  (Against the
    fp64-exact dequantized product the scaled MFMA's own sum is off by ~1e-5 relative -- test_gemm_mxfp8_fp32_parity -- which
    moves near-zero outputs by more than one bf16 ulp.)"""
    B, R, N, K = 2, 640, 3072, 3072
    M = B * R
    aq, wq, bias = _operands(ops, M, N, K, seed=21)
    y32 = ops.gemm_mxfp8(aq, wq, bias, out_fp32=True)
    report("mxfp8 main loop vs dequantized product", y32, _ref_product(aq, wq, bias))
    yb = y32.to(BF)
    assert torch.equal(ops.gemm_mxfp8(aq, wq, bias), yb)
    # against the exact product of the dequantized operands the rounding of near-zero outputs moves: >= 99 % within 1 ulp
    _ulp_check("mxfp8 NONE vs dequantized product", ops.gemm_mxfp8(aq, wq, bias), _ref_product(aq, wq, bias).to(BF), frac=1e-2)
    _ulp_check("mxfp8 GELU_TANH", ops.gemm_mxfp8(aq, wq, bias, epilogue=ops.FK_EPI_GELU_TANH),
               F.gelu(yb.float(), approximate="tanh").to(BF))
    res = randn(B, R, N, seed=22).cuda()
    gate = randn(B, N, seed=23).cuda()
    out = res.clone()
    ops.gemm_mxfp8(aq, wq, bias, out=out.view(B, R, N), epilogue=ops.FK_EPI_GATE_RES, res=out, gate=gate)
    want = (res.float() + (gate.float().unsqueeze(1) * yb.float().view(B, R, N)).to(BF).float()).to(BF)
    _ulp_check("mxfp8 GATE_RES", out, want)


def test_gemm_mxfp8_qkv_epilogue(ops):
    """FK_EPI_QKV on the MXFP8 main loop equals the MXFP8 projection (FK_EPI_NONE) followed by fk_qkv_post_bf16 bit for bit,
    for a grouped text + image launch (the epilogue is shared with the bf16 kernels)."""
    from oracle import mmdit
    from oracle.helpers import prepare_latent_image_ids
    B, H, S_txt, hh, ww, K = 2, 2, 70, 14, 20, 256
    S_img = hh * ww
    S, D = S_txt + S_img, H * 128
    N = 3 * D
    x = randn(B, S, K, seed=60).cuda()
    xi, xt = ops.quantize_mxfp8(x[:, S_txt:]), ops.quantize_mxfp8(x[:, :S_txt])
    wi, wt = ops.quantize_mxfp8(randn(N, K, seed=61, scale=0.06).cuda()), ops.quantize_mxfp8(randn(N, K, seed=62, scale=0.06).cuda())
    bi, bt = randn(N, seed=63, scale=0.1).cuda(), randn(N, seed=64, scale=0.1).cuda()
    nw = [(1 + randn(128, seed=65 + i, scale=0.1).float()).to(BF).cuda() for i in range(4)]
    ids = torch.cat([torch.zeros(S_txt, 3), prepare_latent_image_ids(hh, ww)])
    cos, sin = (t.cuda() for t in mmdit.rope_tables(ids))
    qkv_ref = torch.empty(B, S, N, dtype=BF, device="cuda")
    ops.gemm_mxfp8_grouped([dict(a=xi, w=wi, bias=bi, out=qkv_ref[:, S_txt:]), dict(a=xt, w=wt, bias=bt, out=qkv_ref[:, :S_txt])])
    q_ref = torch.empty(B, H, S, 128, dtype=BF, device="cuda")
    k_ref = torch.empty_like(q_ref)
    ops.qkv_post(qkv_ref, q_ref, k_ref, nw[0], nw[1], nw[2], nw[3], cos, sin, S_txt)
    qkv = torch.zeros(B, S, N, dtype=BF, device="cuda")
    q, k = torch.zeros_like(q_ref), torch.zeros_like(q_ref)
    ops.gemm_mxfp8_grouped([dict(a=xi, w=wi, bias=bi, out=qkv[:, S_txt:],
                                 qkv=dict(q_out=q, k_out=k, wq=nw[0], wk=nw[1], cos=cos, sin=sin, s_offset=S_txt)),
                            dict(a=xt, w=wt, bias=bt, out=qkv[:, :S_txt],
                                 qkv=dict(q_out=q, k_out=k, wq=nw[2], wk=nw[3], cos=cos, sin=sin, s_offset=0))],
                           epilogue=ops.FK_EPI_QKV)
    torch.cuda.synchronize()
    assert torch.equal(q, q_ref) and torch.equal(k, k_ref)
    assert torch.equal(qkv[:, :, 2 * D:], qkv_ref[:, :, 2 * D:])


def test_gemm_mxfp8_rejects_unsupported(ops):
    aq, wq, _ = _operands(ops, 64, 384, 256, seed=30)
    with pytest.raises(RuntimeError, match="N % 256"):
        ops.gemm_mxfp8(aq, wq)
    aq, wq, _ = _operands(ops, 64, 256, 96, seed=31)
    with pytest.raises(RuntimeError, match="K % 128"):
        ops.gemm_mxfp8(aq, wq)
