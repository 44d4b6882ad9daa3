"""The attention forward as a producer of MXFP8 activations (fk_attention_fwd_ws_mxfp8, ops.attention_mxfp8) and the block
schedule that uses it (fk_mx_ws.fused bit 1, transformer.MX_FUSED_ATTN).  The form is SPECIFIED as the bits of the two-step route
-- attention to bf16 on the same grid, then fk_quantize_mxfp8 of the row-gathered streams -- so every comparison is torch.equal
on bytes.  Destinations are pre-filled with a sentinel and carry guard rows and columns: nothing outside the written windows
(columns beyond H * 128, rows beyond each stream, the scale tail) may change."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = 0xA5
GUARD = 2
EINVAL = r"code -1\)"


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


@pytest.fixture
def grid(ops):
    """Sets the attention grid for one test (0 = plain grid, i.e. `grid` -1; n >= 2 = the stream-K test hook) and restores it."""
    saved = ops.LAUNCH.attn_grid
    yield ops.attention_set_split
    ops.LAUNCH.attn_grid = saved


def qkv(B, H, S, seed, v_scale=True):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, S, 128, generator=g).to(BF)
    k = torch.randn(B, H, S, 128, generator=g).to(BF)
    v = torch.randn(B, S, H * 128, generator=g)
    if v_scale:      # block amaxes spread over many binades: every 32-column block of a head gets its own magnitude
        v = v * torch.exp2(torch.arange(H * 4).repeat_interleave(32).float() % 23 - 11)
    return q.cuda(), k.cuda(), v.to(BF).cuda()


class Dest:
    """Both streams in ONE sentinel-filled pair of buffers, stream B's rows first (the block schedule's layout), guard rows around
    them; with ``wide`` the written window is columns [H*128, 2*H*128) of rows 5*H*128 wide (scales likewise)."""

    def __init__(self, B, H, S, split, wide):
        self.B, self.H, self.S = B, H, S
        self.split = S if split == 0 else split
        self.ra, self.rb = B * self.split, B * (S - self.split)
        W, Ws = H * 128, H * 4
        self.W, self.Ws = W, Ws
        self.c0, self.s0 = (W, Ws) if wide else (0, 0)
        ld, lds = (5 * W, 5 * Ws) if wide else (W, Ws)
        rows = self.ra + self.rb
        self.qbuf = torch.full((rows + 2 * GUARD, ld), SENT, dtype=torch.uint8, device="cuda")
        self.sbuf = torch.full((rows + 2 * GUARD, lds), SENT, dtype=torch.uint8, device="cuda")

        def win(r0, n):
            return (self.qbuf[GUARD + r0:GUARD + r0 + n, self.c0:self.c0 + W], self.sbuf[GUARD + r0:GUARD + r0 + n, self.s0:self.s0 + Ws])
        self.b, self.a = win(0, self.rb), win(self.rb, self.ra)

    def untouched_outside(self):
        q, s = self.qbuf.clone(), self.sbuf.clone()
        rows = self.ra + self.rb
        q[GUARD:GUARD + rows, self.c0:self.c0 + self.W] = SENT
        s[GUARD:GUARD + rows, self.s0:self.s0 + self.Ws] = SENT
        return bool((q == SENT).all()) and bool((s == SENT).all())

    def untouched(self):
        return bool((self.qbuf == SENT).all()) and bool((self.sbuf == SENT).all())


def run_mx(ops, q, k, v, d, split, lse=None):
    return ops.attention_mxfp8(q, k, v, d.a, out_b=d.b if d.rb else None, split=split, lse=lse)


def two_step(ops, q, k, v, split, lse=None):
    """The reference route: bf16 attention (current grid), then the standalone quantizer on each row-gathered stream."""
    B, H, S, _ = q.shape
    o = torch.zeros(B, S, H * 128, dtype=BF, device="cuda")
    ops.attention(q, k, v, o, lse=lse)
    sp = S if split == 0 else split
    want_a = ops.quantize_mxfp8(o[:, :sp])
    want_b = ops.quantize_mxfp8(o[:, sp:]) if sp < S else None
    return o, want_a, want_b


def assert_streams_equal(d, want_a, want_b, what):
    for name, got, want in (("A", d.a, want_a), ("B", d.b, want_b)):
        if want is None:
            continue
        assert torch.equal(got[0], want[0]), f"{what} stream {name}: e4m3 bytes differ in {int((got[0] != want[0]).sum())} places"
        assert torch.equal(got[1], want[1]), f"{what} stream {name}: scale bytes differ in {int((got[1] != want[1]).sum())} places"
    assert d.untouched_outside(), f"{what}: bytes outside the written windows changed"


# one stream with a ragged last tile; a split inside a 64-row query group with B > 1; S just under / at / just over a 256-row
# item; H != 24; (1, 4, 1100, 200): 20 items x 18 KV tiles, which a 7-workgroup stream-K grid cuts
SHAPES = [(1, 2, 77, 0), (2, 3, 333, 77), (1, 24, 256, 0), (2, 2, 257, 1), (1, 2, 255, 255), (1, 4, 1100, 200)]


@pytest.mark.parametrize("wide", [False, True], ids=["ldq=H*128", "ldq=5*H*128"])
@pytest.mark.parametrize("mode", [0, 7], ids=["plain", "streamk7"])
@pytest.mark.parametrize("B,H,S,split", SHAPES)
def test_attention_mxfp8_equals_attention_then_quantize(ops, grid, B, H, S, split, mode, wide):
    grid(mode)
    q, k, v = qkv(B, H, S, seed=S + H)
    _, want_a, want_b = two_step(ops, q, k, v, split)
    d = Dest(B, H, S, split, wide)
    run_mx(ops, q, k, v, d, split)
    torch.cuda.synchronize()
    assert_streams_equal(d, want_a, want_b, f"B={B} H={H} S={S} split={split} grid={mode} wide={wide}")
    assert len(torch.unique(want_a[1])) > 4      # the scale bytes really vary from block to block


@pytest.mark.parametrize("mode", [0, 7], ids=["plain", "streamk7"])
def test_zero_and_inf_blocks_follow_the_quantizers_rule(ops, grid, mode):
    grid(mode)
    B, H, S, split = 2, 2, 300, 77
    q, k, v = qkv(B, H, S, seed=5, v_scale=False)
    v.zero_()
    o, want_a, want_b = two_step(ops, q, k, v, split)
    assert not o.any()
    d = Dest(B, H, S, split, False)
    run_mx(ops, q, k, v, d, split)
    torch.cuda.synchronize()
    assert_streams_equal(d, want_a, want_b, "V = 0")
    for qq, ss in (d.a, d.b):
        assert bool((ss == 127).all()) and bool((qq == 0).all())      # all-zero blocks: scale byte 127, codes 0
    # one Inf in V (batch 1, key 5, head 1, column 40 -> block 1 of that head): every query row of that (batch, head) gets a
    # non-finite value there, so the block has scale byte 0xff and codes 0x7f; the other blocks of the row stay zero blocks
    v[1, 5, 128 + 40] = float("inf")
    o, want_a, want_b = two_step(ops, q, k, v, split)
    assert not torch.isfinite(o[1, :, 128 + 40].float()).any() and torch.isfinite(o[0].float()).all()
    d = Dest(B, H, S, split, True)
    run_mx(ops, q, k, v, d, split)
    torch.cuda.synchronize()
    assert_streams_equal(d, want_a, want_b, "one Inf in V")
    assert bool((d.b[1][d.rb // 2:, 4 + 1] == 0xFF).all()) and bool((d.b[0][d.rb // 2:, 128 + 32:128 + 64] == 0x7F).all())
    assert bool((d.b[1][d.rb // 2:, 4 + 2] == 127).all()) and bool((d.b[1][:d.rb // 2] == 127).all())


@pytest.mark.parametrize("mode", [0, 7], ids=["plain", "streamk7"])
def test_lse_is_the_bf16_entrys(ops, grid, mode):
    grid(mode)
    B, H, S, split = 1, 4, 1100, 200
    q, k, v = qkv(B, H, S, seed=11)
    lse_ref = torch.full((B, H, S), -7.0, dtype=torch.float32, device="cuda")
    lse = lse_ref.clone()
    _, want_a, want_b = two_step(ops, q, k, v, split, lse=lse_ref)
    d = Dest(B, H, S, split, False)
    run_mx(ops, q, k, v, d, split, lse=lse)
    torch.cuda.synchronize()
    assert torch.equal(lse, lse_ref) and bool((lse != -7.0).all())
    assert_streams_equal(d, want_a, want_b, "with lse")


def test_bad_arguments_are_refused_before_launching(ops):
    B, H, S, split = 1, 2, 100, 40
    W, Ws = H * 128, H * 4
    q, k, v = qkv(B, H, S, seed=2)
    qb = torch.full((S + 4, W + 64), SENT, dtype=torch.uint8, device="cuda")
    sb = torch.full((S + 4, Ws + 16), SENT, dtype=torch.uint8, device="cuda")
    qn = torch.full((S, W - 16), SENT, dtype=torch.uint8, device="cuda")       # rows narrower than H * 128
    sn = torch.full((S, Ws - 4), SENT, dtype=torch.uint8, device="cuda")
    ok_a, ok_b = (qb[:split, :W], sb[:split, :Ws]), (qb[split:S, :W], sb[split:S, :Ws])
    cases = {
        "q misaligned": (dict(out=(qb[:split, 8:8 + W], sb[:split, :Ws]), out_b=ok_b, split=split), "16-byte aligned"),
        "q_b misaligned": (dict(out=ok_a, out_b=(qb[split:S, 8:8 + W], sb[split:S, :Ws]), split=split), "16-byte aligned"),
        "scales misaligned": (dict(out=(qb[:split, :W], sb[:split, 2:2 + Ws]), out_b=ok_b, split=split), "4-byte aligned"),
        "scales_b misaligned": (dict(out=ok_a, out_b=(qb[split:S, :W], sb[split:S, 2:2 + Ws]), split=split), "4-byte aligned"),
        "ldq < H * 128": (dict(out=(qn, sb[:S, :Ws]), split=0), "ldq >= H \\* 128"),
        "ldq_scale < H * 4": (dict(out=(qb[:S, :W], sn), split=0), "ldq_scale >= H \\* 4"),
        "split > S": (dict(out=ok_a, out_b=ok_b, split=S + 1), "split"),
        "split < 0": (dict(out=ok_a, out_b=ok_b, split=-1), "split"),
        "null stream B": (dict(out=ok_a, out_b=None, split=split), "second stream"),
    }
    for name, (kw, text) in cases.items():
        with pytest.raises(RuntimeError, match=EINVAL + ".*" + text):
            ops.attention_mxfp8(q, k, v, **kw)
    torch.cuda.synchronize()
    for t in (qb, sb, qn, sn):
        assert bool((t == SENT).all()), "a refused call wrote to its destination"
    # the same buffers, addressed properly, are accepted
    ops.attention_mxfp8(q, k, v, ok_a, out_b=ok_b, split=split)
    torch.cuda.synchronize()
    assert bool((qb[:S, :W] != SENT).any()) and bool((qb[:, W:] == SENT).all()) and bool((qb[S:] == SENT).all())


def _model_and_inputs():
    from test_hip_mxfp8_fused import _model_and_inputs as make
    return make()


@pytest.fixture
def switches():
    from gpt_image_edit_amd import transformer
    saved = transformer.BLOCK_API, transformer.MX_FUSED_QUANT, transformer.MX_FUSED_ATTN
    yield transformer
    transformer.BLOCK_API, transformer.MX_FUSED_QUANT, transformer.MX_FUSED_ATTN = saved


def test_blocks_with_the_attention_producer_give_the_fused_schedules_bits(ops, switches):
    """2 double + 4 single blocks, B = 2, S_txt = 77, 10 x 12 latents, on all three FK_BLOCK_API routes: with MX_FUSED_ATTN the model
    output and the residual stream are those of MX_FUSED_QUANT alone and no standalone quantizer launch is left; without it there
    are still 2 per double and 1 per single block.  The switch alone (MX_FUSED_QUANT off) changes nothing."""
    transformer, model, kw = _model_and_inputs()
    model(**kw)
    results = {}
    for fused, attn in ((True, False), (True, True), (False, True)):
        for api in (0, 1, 2):
            transformer.BLOCK_API, transformer.MX_FUSED_QUANT, transformer.MX_FUSED_ATTN = api, fused, attn
            n0 = ops.quantize_launch_count()
            out = model(**kw)[0].clone()
            torch.cuda.synchronize()
            (ws,) = model._ws.values()
            results[(fused, attn, api)] = (out, ws.s.clone(), ops.quantize_launch_count() - n0)
    base = results[(True, False, 2)]
    assert torch.isfinite(base[0].float()).all()
    for (fused, attn, api), (out, s, launches) in results.items():
        what = f"MX_FUSED_QUANT={fused} MX_FUSED_ATTN={attn} FK_BLOCK_API={api}"
        assert torch.equal(s, base[1]), f"residual stream differs for {what}"
        assert torch.equal(out, base[0]), f"output differs for {what}"
        want = (0 if attn else 2 * 2 + 4 * 1) if fused else 2 * 8 + 4 * 3
        assert launches == want, f"{what}: {launches} quantizer launches, expected {want}"


def test_fused_bit_1_alone_is_refused(ops, switches):
    from gpt_image_edit_amd import libfk
    transformer, model, kw = _model_and_inputs()
    transformer.BLOCK_API, transformer.MX_FUSED_QUANT, transformer.MX_FUSED_ATTN = 1, True, True
    model(**kw)
    torch.cuda.synchronize()
    (ws,) = model._ws.values()
    pk = model.packed()
    st, sx = model._block_weight_structs(pk), model._block_mx_structs(pk)
    c, mxw = model.__dict__["_block_ws"][1], model.__dict__["_block_ws"][3]
    assert mxw.fused == 3
    mod = ws.mod
    mp, mbs, stream = ctypes.c_void_p(mod.data_ptr()), mod.stride(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = libfk.load()
    s_before = ws.s.clone()
    ws.mxq.fill_(SENT)
    ws.mxs.fill_(SENT)
    bad = libfk.MxWs(mxw.q, mxw.s, mxw.q_bytes, mxw.s_bytes, 2, None)
    calls = {
        "single": lambda: lib.fk_single_block_fwd_mx(ctypes.byref(c), ctypes.byref(bad), ctypes.byref(st.sgl[0]), ctypes.byref(sx.sgl[0]),
                                                     mp, mbs, stream),
        "double": lambda: lib.fk_double_block_fwd_mx(ctypes.byref(c), ctypes.byref(bad), ctypes.byref(st.dbl[0]), ctypes.byref(sx.dbl[0]),
                                                     mp, mbs, stream),
        "stack": lambda: lib.fk_mmdit_blocks_fwd_mx(ctypes.byref(c), ctypes.byref(bad), st.dbl, sx.dbl, st.nd, st.sgl, sx.sgl, st.ns, mp,
                                                    mbs, stream),
    }
    for name, call in calls.items():
        rc = call()
        msg = lib.fk_last_error().decode()
        assert rc == -1 and "fused" in msg and "bit 0" in msg, f"{name}: return code {rc}, message {msg!r}"
    torch.cuda.synchronize()
    assert torch.equal(ws.s, s_before) and bool((ws.mxq == SENT).all()) and bool((ws.mxs == SENT).all())


def test_set_mx_fused_attn_bumps_the_launch_epoch_and_toggles_back(ops, switches):
    transformer, model, kw = _model_and_inputs()
    transformer.BLOCK_API, transformer.MX_FUSED_QUANT = 2, True
    transformer.set_mx_fused_attn(False)
    first = model(**kw)[0].clone()
    e0 = ops.launch_config_epoch()
    transformer.set_mx_fused_attn(True)
    assert transformer.MX_FUSED_ATTN is True and ops.launch_config_epoch() == e0 + 1
    n0 = ops.quantize_launch_count()
    on = model(**kw)[0].clone()
    assert ops.quantize_launch_count() == n0
    transformer.set_mx_fused_attn(False)
    assert transformer.MX_FUSED_ATTN is False and ops.launch_config_epoch() == e0 + 2
    again = model(**kw)[0].clone()
    torch.cuda.synchronize()
    assert ops.quantize_launch_count() == n0 + 2 * 2 + 4 * 1
    assert torch.equal(on, first) and torch.equal(again, first)
