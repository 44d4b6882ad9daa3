"""MXFP8 producers that emit quantized activations directly (fk_ln_modulate(2)_mxfp8, fk_gemm_mxfp8_q) and the fused block
schedule built on them.  The fused forms are SPECIFIED as the bits of the two-launch forms (producer to bf16, then
fk_quantize_mxfp8): every comparison here is torch.equal on bytes, no tolerance anywhere.  Output buffers are pre-filled with a
sentinel and carry guard rows / columns: nothing outside the specified window may change."""
import os
import subprocess
import sys

import pytest
import torch

import mxfp8_ref as ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = 3072
SENT = 0xA5
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def guarded(rows, cols, guard=2):
    """Sentinel-filled uint8 [rows + 2 guard, cols] buffer and the view of its inner rows."""
    buf = torch.full((rows + 2 * guard, cols), SENT, dtype=torch.uint8, device="cuda")
    return buf, buf[guard:guard + rows]


def guards_intact(buf, rows, guard=2):
    return bool((buf[:guard] == SENT).all()) and bool((buf[guard + rows:] == SENT).all())


def ln_inputs(B, R, seed):
    """[B, R, D] rows with the quantizer's edge cases among them, and batch-strided modulation views (one [B, 6 D] buffer)."""
    x = randn(B, R, D, seed=seed)
    mod = randn(B, 6 * D, seed=seed + 1, scale=0.5)
    if R >= 6:
        x[0, 1] = 0                                   # an all-zero row (meets a zero shift below: all-zero blocks)
        x[0, 2] *= 2.0 ** -20
        x[0, 3] *= 2.0 ** 12
        x[-1, R - 1] *= 2.0 ** 12
    return x.cuda(), mod.cuda()


def mod_views(mod, j_shift, j_scale):
    return mod[:, j_shift * D:(j_shift + 1) * D], mod[:, j_scale * D:(j_scale + 1) * D]


def assert_pair_equal(got, want, what):
    assert torch.equal(got[0], want[0]), f"{what}: e4m3 bytes differ in {int((got[0] != want[0]).sum())} places"
    assert torch.equal(got[1], want[1]), f"{what}: scale bytes differ in {int((got[1] != want[1]).sum())} places"


def assert_matches_host_reference(pair, n_bf16, what):
    q, s = ref.quantize(n_bf16.float().cpu().double().numpy().reshape(-1, n_bf16.shape[-1]))
    assert (pair[0].cpu().numpy() == q).all() and (pair[1].cpu().numpy() == s).all(), f"{what}: differs from tests/mxfp8_ref.py"


@pytest.mark.parametrize("B,R", [(1, 1), (1, 63), (1, 64), (2, 63), (1, 8704), (2, 2560)])
def test_ln_modulate_mxfp8_equals_ln_then_quantize(ops, B, R):
    x, mod = ln_inputs(B, R, seed=R)
    shift, scale = mod_views(mod, 0, 1)
    if R >= 6:
        shift[0].zero_()                              # zero shift of batch 0: its all-zero row stays all-zero (scale byte 127)
        # one 32-block of one row is zero after modulation: scale = -1 there gives (1 + scale) = 0, shift = 0
        scale[0, 64:96] = -1.0
    n = ops.ln_modulate(x, shift, scale)
    want = ops.quantize_mxfp8(n)
    M = B * R
    qbuf, q = guarded(M, D)
    sbuf, s = guarded(M, D // 32)
    got = ops.ln_modulate_mxfp8(x, shift, scale, out=(q, s))
    torch.cuda.synchronize()
    assert_pair_equal(got, want, f"ln_modulate_mxfp8 B={B} R={R}")
    assert guards_intact(qbuf, M) and guards_intact(sbuf, M)
    assert_matches_host_reference(got, n, f"ln_modulate_mxfp8 B={B} R={R}")
    if R >= 6:
        assert bool((got[1][1] == 127).all()) and bool((got[0][1] == 0).all())         # the all-zero row
        assert bool((got[1][:R, 2] == 127).all())                                        # the zeroed block of every row of batch 0
    fresh = ops.ln_modulate_mxfp8(x, shift, scale)                                       # allocating form
    assert_pair_equal(fresh, want, "ln_modulate_mxfp8 (fresh outputs)")


@pytest.mark.parametrize("B,S_txt,S_img", [(1, 512, 2560), (2, 77, 240), (1, 1, 63), (2, 512, 2560)])
def test_ln_modulate2_mxfp8_equals_ln_then_quantize(ops, B, S_txt, S_img):
    R = S_txt + S_img
    x, mod = ln_inputs(B, R, seed=R + 7)
    sh_t, sc_t = mod_views(mod, 0, 1)
    sh_i, sc_i = mod_views(mod, 3, 4)
    if R >= 6:
        sh_t[0].zero_()
        sh_i[0].zero_()
        sc_i[0, 3040:3072] = -1.0
        x[0, R - 2] = 0                               # an all-zero image row
    n = ops.ln_modulate2(x, sh_t, sc_t, sh_i, sc_i, S_txt)
    want_t, want_i = ops.quantize_mxfp8(n[:, :S_txt]), ops.quantize_mxfp8(n[:, S_txt:])
    # both streams in ONE guarded workspace, image rows first (the block schedule's layout)
    Mi, Mt = B * S_img, B * S_txt
    qbuf, q = guarded(Mi + Mt, D)
    sbuf, s = guarded(Mi + Mt, D // 32)
    got_t, got_i = ops.ln_modulate2_mxfp8(x, sh_t, sc_t, sh_i, sc_i, S_txt, out=(q[Mi:], s[Mi:]), out_b=(q[:Mi], s[:Mi]))
    torch.cuda.synchronize()
    assert_pair_equal(got_t, want_t, "ln_modulate2_mxfp8 text stream")
    assert_pair_equal(got_i, want_i, "ln_modulate2_mxfp8 image stream")
    assert guards_intact(qbuf, Mi + Mt) and guards_intact(sbuf, Mi + Mt)
    assert_matches_host_reference(got_i, n[:, S_txt:].reshape(-1, D), "ln_modulate2_mxfp8 image stream")
    assert_matches_host_reference(got_t, n[:, :S_txt].reshape(-1, D), "ln_modulate2_mxfp8 text stream")
    if R >= 6:
        assert bool((got_i[1][:S_img, 95] == 127).all())


def _operands(ops, M, N, K, seed):
    a = ops.quantize_mxfp8(randn(M, K, seed=seed).cuda())
    w = ops.quantize_mxfp8(randn(N, K, seed=seed + 1, scale=0.05).cuda())
    bias = randn(N, seed=seed + 2, scale=0.5).cuda()
    return a, w, bias


@pytest.mark.parametrize("epi", ["NONE", "GELU_TANH"])
@pytest.mark.parametrize("M,N,want_bn", [(2597, 3072, 128), (2597, 12288, 256), (128, 3072, 128), (8704, 12288, 256)])
def test_gemm_mxfp8_quantized_output_equals_gemm_then_quantize(ops, epi, M, N, want_bn):
    """Both tile widths (the launch plan's choice is asserted: 256 x 128 while 256 x 256 tiles would not fill the chip once),
    ragged M (2597 = 10 tiles + 37 rows), N in {D, 4 D}."""
    K = D
    epilogue = getattr(ops, "FK_EPI_" + epi)
    a, w, bias = _operands(ops, M, N, K, seed=M + N)
    c = ops.gemm_mxfp8(a, w, bias=bias, epilogue=epilogue)
    assert ops.gemm_last_variant() == want_bn
    want = ops.quantize_mxfp8(c)
    qbuf, q = guarded(M, N)
    sbuf, s = guarded(M, N // 32)
    got = ops.gemm_mxfp8(a, w, bias=bias, epilogue=epilogue, out_mx=(q, s))
    assert ops.gemm_last_variant() == want_bn
    torch.cuda.synchronize()
    assert_pair_equal(got, want, f"gemm_mxfp8 out_mx {epi} M={M} N={N}")
    assert guards_intact(qbuf, M) and guards_intact(sbuf, M)
    for bn in (128, 256):                             # and each tile width forced
        forced = ops.gemm_mxfp8(a, w, bias=bias, epilogue=epilogue, out_mx=True, variant=bn)
        assert ops.gemm_last_variant() == bn
        assert_pair_equal(forced, want, f"gemm_mxfp8 out_mx {epi} forced {bn}")


def test_gemm_mxfp8_quantized_output_grouped_and_column_window(ops):
    K = D
    # grouped: two problems of different (ragged) M, own weights, own outputs
    a0, w0, b0 = _operands(ops, 2597, 12288, K, seed=1)
    a1, w1, b1 = _operands(ops, 333, 12288, K, seed=5)
    cs = ops.gemm_mxfp8_grouped([dict(a=a0, w=w0, bias=b0), dict(a=a1, w=w1, bias=b1)], epilogue=ops.FK_EPI_GELU_TANH)
    want = [ops.quantize_mxfp8(c) for c in cs]
    qbuf, q = guarded(2597 + 333, 12288)
    sbuf, s = guarded(2597 + 333, 12288 // 32)
    got = ops.gemm_mxfp8_grouped([dict(a=a0, w=w0, bias=b0, out_mx=(q[:2597], s[:2597])),
                                  dict(a=a1, w=w1, bias=b1, out_mx=(q[2597:], s[2597:]))], epilogue=ops.FK_EPI_GELU_TANH)
    torch.cuda.synchronize()
    for g, wnt in zip(got, want):
        assert_pair_equal(g, wnt, "grouped gemm_mxfp8 out_mx")
    assert guards_intact(qbuf, 2597 + 333) and guards_intact(sbuf, 2597 + 333)
    # column window: N = 4 D into columns [D, 5 D) of a [M, 5 D] buffer (the single block's MLP-up into proj_out's operand)
    M = 2597
    qbuf, q = guarded(M, 5 * D)
    sbuf, s = guarded(M, 5 * D // 32)
    pair = ops.gemm_mxfp8(a0, w0, bias=b0, epilogue=ops.FK_EPI_GELU_TANH, out_mx=(q, s, D))
    torch.cuda.synchronize()
    assert_pair_equal((pair[0][:, D:], pair[1][:, D // 32:]), want[0], "gemm_mxfp8 out_mx column window")
    assert bool((q[:, :D] == SENT).all()) and bool((s[:, :D // 32] == SENT).all()), "neighbouring columns were written"
    assert guards_intact(qbuf, M) and guards_intact(sbuf, M)


def test_fused_producers_reject_bad_arguments_before_launching(ops):
    """FK_EINVAL with a message, outputs untouched: misaligned byte rows, a column offset off the 32-grid, a window wider than
    the buffer, and (block entry points) a workspace one byte too small."""
    M, N, K = 64, 3072, D
    a, w, bias = _operands(ops, M, N, K, seed=3)
    q = torch.full((M, 5 * D + 64), SENT, dtype=torch.uint8, device="cuda")
    s = torch.full((M, 5 * D // 32 + 8), SENT, dtype=torch.uint8, device="cuda")
    einval = r"code -1\)"                           # FK_EINVAL
    q2 = torch.full((M, N + 8), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=einval + r".*multiple of 32"):
        ops.gemm_mxfp8(a, w, bias=bias, out_mx=(q, s, 48))
    with pytest.raises(RuntimeError, match=einval + r".*16-byte aligned"):
        ops.gemm_mxfp8(a, w, bias=bias, out_mx=(q[:, 8:8 + N], s[:, :N // 32]))               # Q off the 16-byte grid
    with pytest.raises(RuntimeError, match=einval + r".*16-byte aligned"):
        ops.gemm_mxfp8(a, w, bias=bias, out_mx=(q2[:, :N], s[:, :N // 32]))                   # row stride N + 8: ldq % 16 != 0
    with pytest.raises(RuntimeError, match=einval + r".*do not hold columns"):
        ops.gemm_mxfp8(a, w, bias=bias, out_mx=(q, s, 5 * D + 64 - N + 32))                   # ld < offset + N
    x, mod = ln_inputs(1, M, seed=9)
    shift, scale = mod_views(mod, 0, 1)
    with pytest.raises(RuntimeError, match=einval + r".*16-byte aligned"):
        ops.ln_modulate_mxfp8(x, shift, scale, out=(q[:, 8:8 + D], s[:, :D // 32]))
    with pytest.raises(RuntimeError, match=einval + r".*4-byte aligned"):
        ops.ln_modulate_mxfp8(x, shift, scale, out=(q[:, :D], s[:, 2:2 + D // 32]))
    torch.cuda.synchronize()
    assert bool((q == SENT).all()) and bool((s == SENT).all()) and bool((q2 == SENT).all())


def _model_and_inputs(layers=(2, 4)):
    from gpt_image_edit_amd import flux_spec, transformer
    from test_hip_mxfp8_model import _kw
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=layers[0], num_single_layers=layers[1])
    model = transformer.HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=31, weight_format="mxfp8")
    return transformer, model, _kw(2, 77, 10, 12, cfg, seed=4)


def test_block_entry_points_fused_and_unfused_give_the_same_stream(ops):
    """fk_double_block_fwd_mx / fk_single_block_fwd_mx (FK_BLOCK_API=1) and fk_mmdit_blocks_fwd_mx (2) with fk_mx_ws.fused set
    and clear, and the per-launch route (0) both ways: the residual stream s after the blocks and the model output are the same
    bits; the standalone quantizer runs 2 x per double and 1 x per single block when fused (8 and 3 when not)."""
    transformer, model, kw = _model_and_inputs()
    saved = transformer.BLOCK_API, transformer.MX_FUSED_QUANT
    try:
        model(**kw)
        results = {}
        for fused in (False, True):
            for api in (0, 1, 2):
                transformer.BLOCK_API, transformer.MX_FUSED_QUANT = api, fused
                n0 = ops.quantize_launch_count()
                out = model(**kw)[0].clone()
                torch.cuda.synchronize()
                (ws,) = model._ws.values()
                results[(fused, api)] = (out, ws.s.clone(), ops.quantize_launch_count() - n0)
        base = results[(False, 2)]
        assert torch.isfinite(base[0].float()).all()
        for key, (out, s, launches) in results.items():
            assert torch.equal(s, base[1]), f"residual stream differs for fused={key[0]} FK_BLOCK_API={key[1]}"
            assert torch.equal(out, base[0]), f"output differs for fused={key[0]} FK_BLOCK_API={key[1]}"
            assert launches == (2 * 2 + 4 * 1 if key[0] else 2 * 8 + 4 * 3), f"{key}: {launches} quantizer launches"
    finally:
        transformer.BLOCK_API, transformer.MX_FUSED_QUANT = saved


def test_block_entry_points_reject_a_workspace_one_byte_too_small(ops):
    import ctypes
    from gpt_image_edit_amd import libfk
    transformer, model, kw = _model_and_inputs()
    saved = transformer.BLOCK_API, transformer.MX_FUSED_QUANT
    try:
        transformer.BLOCK_API, transformer.MX_FUSED_QUANT = 1, True
        want = model(**kw)[0].clone()
        torch.cuda.synchronize()
        (ws,) = model._ws.values()
        pk = model.packed()
        st, sx = model._block_weight_structs(pk), model._block_mx_structs(pk)
        c, mxw = model.__dict__["_block_ws"][1], model.__dict__["_block_ws"][3]
        B, S = ws.s.shape[0], ws.S
        mod = ws.mod
        mp, mbs, stream = ctypes.c_void_p(mod.data_ptr()), mod.stride(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib = libfk.load()
        s_before = ws.s.clone()
        ws.mxq.fill_(SENT)
        ws.mxs.fill_(SENT)
        need_double, need_single = B * S * 5 * D, B * S * 6 * D

        def small(q_bytes, s_bytes):
            return libfk.MxWs(mxw.q, mxw.s, q_bytes, s_bytes, 1, None)

        calls = [
            ("double q", lambda m: lib.fk_double_block_fwd_mx(ctypes.byref(c), ctypes.byref(m), ctypes.byref(st.dbl[0]),
                                                               ctypes.byref(sx.dbl[0]), mp, mbs, stream), (need_double - 1, need_double // 32)),
            ("double s", lambda m: lib.fk_double_block_fwd_mx(ctypes.byref(c), ctypes.byref(m), ctypes.byref(st.dbl[0]),
                                                               ctypes.byref(sx.dbl[0]), mp, mbs, stream), (need_double, need_double // 32 - 1)),
            ("single q", lambda m: lib.fk_single_block_fwd_mx(ctypes.byref(c), ctypes.byref(m), ctypes.byref(st.sgl[0]),
                                                               ctypes.byref(sx.sgl[0]), mp, mbs, stream), (need_single - 1, need_single // 32)),
            # the whole stack checks every block's need before its first launch: a double-block-sized workspace is refused
            ("stack", lambda m: lib.fk_mmdit_blocks_fwd_mx(ctypes.byref(c), ctypes.byref(m), st.dbl, sx.dbl, st.nd, st.sgl, sx.sgl,
                                                           st.ns, mp, mbs, stream), (need_single - 1, need_single // 32)),
        ]
        for name, call, (qb, sb) in calls:
            rc = call(small(qb, sb))
            msg = lib.fk_last_error().decode()
            assert rc == -1, f"{name}: return code {rc}"                 # FK_EINVAL
            assert "workspace" in msg and str(qb) in msg, f"{name}: message {msg!r}"
        torch.cuda.synchronize()
        assert torch.equal(ws.s, s_before) and bool((ws.mxq == SENT).all()) and bool((ws.mxs == SENT).all())
        # exactly enough is accepted
        assert lib.fk_single_block_fwd_mx(ctypes.byref(c), ctypes.byref(small(need_single, need_single // 32)), ctypes.byref(st.sgl[0]),
                                          ctypes.byref(sx.sgl[0]), mp, mbs, stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(model(**kw)[0], want)
    finally:
        transformer.BLOCK_API, transformer.MX_FUSED_QUANT = saved


@pytest.mark.timeout(1500, method="thread")
def test_model_forward_and_edit_identical_under_the_switch(tmp_path):
    """FK_MX_FUSED_QUANT=1 and =0, each with FK_BLOCK_API 0 / 1 / 2, every setting in a fresh child process (the switches are
    read at import): a 2 + 4-block forward and a short edit -- eager and through the captured graph, capture and replay -- give
    identical latents; one fused forward launches the standalone quantizer 2 x 2 + 4 x 1 times."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    results = {}
    for fused in (1, 0):
        for api in (0, 1, 2):
            out = tmp_path / f"f{fused}_a{api}.pt"
            env = dict(os.environ, FK_MX_FUSED_QUANT=str(fused), FK_BLOCK_API=str(api))
            r = subprocess.run([sys.executable, os.path.join(HERE, "mxfp8_fused_child.py"), str(out)], env=env, capture_output=True,
                               text=True, timeout=600)
            print(r.stdout[-400:], flush=True)
            assert r.returncode == 0, f"child fused={fused} api={api} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
            results[(fused, api)] = torch.load(out)
    base = results[(0, 2)]
    for (fused, api), res in results.items():
        assert (res["fused"], res["api"]) == (fused, api)
        for k in ("fwd", "eager2", "graph2", "eager3", "graph3"):
            assert torch.isfinite(res[k].float()).all()
            assert torch.equal(res[k], base[k]), f"{k} differs for FK_MX_FUSED_QUANT={fused} FK_BLOCK_API={api}"
        assert torch.equal(res["eager2"], res["graph2"]) and torch.equal(res["eager3"], res["graph3"])
        assert res["launches"] == (2 * 2 + 4 * 1 if fused else 2 * 8 + 4 * 3), f"fused={fused} api={api}: {res['launches']}"
