"""ln_modulate_bwd, qkv_post_bwd and gate_res_bwd (csrc/backward_kernels.hip) on the GPU, EVERY element they write against
tests/backward_ref.py: dx and d(raw q | k) by the candidate-set rule (the float64 value of the float32 stage, every bf16 a margin
of C x 2^-24 x the stated scale around it can round to, the output one of them bit for bit; the share of elements with a choice
capped), the float32 sums dshift / dscale / dw / dgate within bounds derived from the kernels' summation order, dy bit-equal
to the bf16 product.  Small shapes: the arithmetic of a row does not depend on the row count, and the row-to-chunk mapping is
exact-tested at production sizes in test_hip_backward_exact.py.  Inputs and outputs are views of joint buffers whose
surroundings hold sentinels; every launch is repeated into a differently filled buffer and must give the same bits.  The last
test holds the three launchers' refusals to writing nothing, the backward workspace included."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_ref as R  # noqa: E402
from backward_ref import judge  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
S_TXT = R.S_TXT


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def held(name, got, ref, c):
    """The rule on one bf16 output, the cap on the ambiguous share, and what the run shows of the margin."""
    v = judge(got, *R.accept(ref, c))
    print(v.line(name) + f"; worst observed share of delta {R.observed_share(got, ref, c):.3f}", flush=True)
    assert v.ok, v.line(name)
    assert v.ambiguous <= R.AMBIGUOUS_CAP, f"{name}: ambiguous share {v.ambiguous:.3e} above the cap {R.AMBIGUOUS_CAP}"


def within(name, got, ref64, bound):
    share = R.worst_share(got, ref64, bound)
    print(f"[parity] {name}: worst share of the bound {share:.4f}", flush=True)
    assert share <= 1.0, f"{name}: {share:.3f} x the bound"


@pytest.mark.parametrize("R_", R.LN_RS)
@pytest.mark.parametrize("B", R.LN_BS)
@pytest.mark.parametrize("D", R.LN_DS)
def test_ln_modulate_bwd_every_element(ops, D, B, R_):
    """R = 1, 3: fewer rows than the four waves; 16 -> 17: one workgroup becomes two; 5, 37, 300: a ragged last trip.  x, dx_in,
    dx_out: rows [S_TXT:] of [B, S_TXT + R, D] buffers; dshift | dscale: columns [3 D, 5 D) of a [B, 6 D + 64] float32 buffer."""
    xb, dn, mod, dxb = R.ln_bwd_inputs(D, B, R_)
    xd, dnd, md, dxd = xb.cuda(), dn.cuda(), mod.cuda(), dxb.cuda()
    x, scale = xb[:, S_TXT:], mod[:, D:2 * D]
    for dx_in in (None, dxb[:, S_TXT:]):
        name = f"ln_modulate_bwd D={D} B={B} R={R_}{' + dx_in' if dx_in is not None else ''}"
        ref = R.ln_bwd_ref(x, dn, scale, dx_in)
        res = []
        for fill in (7.0, -3.0):
            out = torch.full_like(xd, fill)
            dmod = torch.full((B, 6 * D + 64), fill, device="cuda", dtype=torch.float32)
            ops.ln_modulate_bwd(xd[:, S_TXT:], dnd, md[:, D:2 * D], out[:, S_TXT:], dmod[:, 3 * D:5 * D],
                                dx_in=None if dx_in is None else dxd[:, S_TXT:])
            torch.cuda.synchronize()
            assert bool((out[:, :S_TXT] == fill).all()), "rows in front of the dx_out view were written"
            assert bool((dmod[:, :3 * D] == fill).all()) and bool((dmod[:, 5 * D:] == fill).all()), "columns outside the dmod window"
            res.append((out[:, S_TXT:].cpu(), dmod[:, 3 * D:5 * D].cpu()))
        assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), "a second launch gave other bits"
        dx, dsum = res[0]
        held(name + " dx", dx, ref, R.LN_C)
        within(name + " dshift", dsum[:, :D], ref["dshift"], ref["dshift_bound"])
        within(name + " dscale", dsum[:, D:], ref["dscale"], ref["dscale_bound"])
        if R_ >= 5:           # the row whose dn is zero
            want = dx_in[B - 1, 3] if dx_in is not None else torch.zeros(D, dtype=BF)
            assert same_bits(dx[B - 1, 3], want), "dn = 0: dx must be dx_in's bits (+0 without it)"
        if dx_in is not None:
            # the form the block backward runs: dx_out IS dx_in (the residual-stream gradient, updated in place)
            g = dxd.clone()
            dmod = torch.zeros(B, 2 * D, device="cuda", dtype=torch.float32)
            ops.ln_modulate_bwd(xd[:, S_TXT:], dnd, md[:, D:2 * D], g[:, S_TXT:], dmod, dx_in=g[:, S_TXT:])
            torch.cuda.synchronize()
            assert same_bits(g[:, S_TXT:].cpu(), dx), "in place differs from out of place"
            assert same_bits(g[:, :S_TXT], dxd[:, :S_TXT]) and same_bits(dmod.cpu(), dsum)
    assert same_bits(xd.cpu(), xb) and same_bits(dnd.cpu(), dn) and same_bits(dxd.cpu(), dxb), "an input was written"


@pytest.mark.parametrize("case", R.QKV_CASES, ids=lambda c: "B{}-H{}-txt{}-S{}".format(*c))
def test_qkv_post_bwd_every_element(ops, case):
    """One token; 75 = 64 + 11 with a text part; 63 and 64 either side of a block, without and with only text; 65 text tokens
    and nothing else; 130 = three blocks with the text / image seam inside the first; 24 heads."""
    B, H, s_txt, S = case
    D = H * 128
    dq, dk, qkv, w, cos, sin = R.qkv_bwd_inputs(*case)
    ref = R.qkv_post_bwd_ref(dq, dk, qkv, w, cos, sin, s_txt)
    wd = [t.cuda() for t in w]
    wt = (wd[2], wd[3]) if s_txt else (None, None)
    dqd, dkd, qkvd, cd, sd = dq.cuda(), dk.cuda(), qkv.cuda(), cos.cuda(), sin.cuda()
    res = []
    for fill in (9.0, -5.0):
        dqkv = torch.full((B, S, 3 * D), fill, device="cuda", dtype=BF)
        dw = ops.qkv_post_bwd(dqd, dkd, qkvd, dqkv, wd[0], wd[1], wt[0], wt[1], cd, sd, s_txt)
        torch.cuda.synchronize()
        assert bool((dqkv[..., 2 * D:] == fill).all()), "the v third was written"
        res.append((dqkv[..., :2 * D].cpu(), dw.cpu()))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1]), "a second launch gave other bits"
    dx, dw = res[0]
    held(f"qkv_post_bwd {case} d(raw q | k)", dx, ref, R.QKV_C)
    within(f"qkv_post_bwd {case} dw", dw, ref["dw"], ref["dw_bound"])
    if s_txt == 0:
        assert bool((bits(dw[:, 1]) == 0).all()), "no text tokens: the text half of dw must be +0"
    assert same_bits(qkvd.cpu(), qkv) and same_bits(dqd.cpu(), dq) and same_bits(dkd.cpu(), dk), "an input was written"


def test_gate_res_bwd_random_data(ops):
    """dy = bf16(dout gate) bit for bit, dgate within the bound of its order, on views of joint buffers."""
    B, R_, N = R.GATE_CASE
    dob, yb, mod = R.gate_inputs(B, R_, N)
    want_dy, dgate, bound = R.gate_res_ref(dob[:, S_TXT:], yb[:, S_TXT:], mod[:, N:2 * N])
    dod, yd, md = dob.cuda(), yb.cuda(), mod.cuda()
    res = []
    for fill in (7.0, -3.0):
        dy = torch.full((B, S_TXT + R_, N), fill, device="cuda", dtype=BF)
        dg = torch.full((B, 2 * N), fill, device="cuda", dtype=torch.float32)
        ops.gate_res_bwd(dod[:, S_TXT:], yd[:, S_TXT:], md[:, N:2 * N], dy[:, S_TXT:], dg[:, N:])
        torch.cuda.synchronize()
        assert bool((dy[:, :S_TXT] == fill).all()) and bool((dg[:, :N] == fill).all()), "rows / columns outside the views"
        res.append((dy[:, S_TXT:].cpu(), dg[:, N:].cpu()))
    assert same_bits(res[0][0], res[1][0]) and same_bits(res[0][1], res[1][1])
    assert same_bits(res[0][0], want_dy), "dy is not the bf16 product"
    within(f"gate_res_bwd B{B} R{R_} N{N} dgate", res[0][1], dgate, bound)


def test_refusals_write_nothing(ops):
    """Every refusal of the three launchers: the code, fk_last_error() naming the function, and sentinel-filled outputs AND the
    backward workspace untouched -- dscale != dshift + D included, which used to be found only after the kernel had run."""
    from gpt_image_edit_amd import libfk
    from gpt_image_edit_amd.libfk import Rows
    lib = libfk.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    V = ctypes.c_void_p
    EINVAL, EUNSUP = -1, -2
    SENT = 777.0
    ws = torch.full((int(lib.fk_bwd_ws_floats()),), SENT, device="cuda", dtype=torch.float32)

    def refused(fn, call, cases, outputs):
        for name, kw, want in cases:
            code = call(**kw)
            assert code == want, (fn, name, code)
            assert lib.fk_last_error().decode().startswith(fn), (fn, name, lib.fk_last_error().decode())
        torch.cuda.synchronize()
        for t in outputs:
            assert bool((t == SENT).all()), f"{fn}: a refused call wrote an output"
        assert bool((ws == SENT).all()), f"{fn}: a refused call wrote the workspace"
        assert call() == 0, lib.fk_last_error().decode()
        torch.cuda.synchronize()
        for t in outputs:
            assert not bool((t == SENT).any()), f"{fn}: the valid call left sentinels"
        ws.fill_(SENT)

    # ---- fk_ln_modulate_bwd_bf16
    B, R_, D = 2, 5, 512
    x, dn, dxi = (torch.randn(B, R_, D, device="cuda").to(BF) for _ in range(3))
    scale = torch.randn(B, D, device="cuda").to(BF)
    dx = torch.full((B, R_, D), SENT, device="cuda", dtype=BF)
    dmod = torch.full((B, 2 * D), SENT, device="cuda", dtype=torch.float32)
    rows = Rows(D, R_, R_ * D)

    def ln(x_p=x.data_ptr(), xr=rows, dn_p=dn.data_ptr(), dnr=rows, sc_p=scale.data_ptr(), mod_bs=D, rpb=R_, in_p=dxi.data_ptr(),
           inr=rows, out_p=dx.data_ptr(), outr=rows, sh_p=dmod.data_ptr(), dsc_off=4 * D, ws_p=ws.data_ptr(), b=B, d=D):
        return lib.fk_ln_modulate_bwd_bf16(V(x_p), xr, V(dn_p), dnr, V(sc_p), mod_bs, rpb, V(in_p), inr, V(out_p), outr, V(sh_p),
                                           V(sh_p + dsc_off if sh_p else 0), 2 * D, V(ws_p), b, d, 1e-6, st)
    odd = Rows(D + 4, R_, R_ * D)
    refused("fk_ln_modulate_bwd_bf16", ln, [
        ("null x", dict(x_p=0), EINVAL), ("null dn", dict(dn_p=0), EINVAL), ("null scale", dict(sc_p=0), EINVAL),
        ("null dx_out", dict(out_p=0), EINVAL), ("null dshift / dscale", dict(sh_p=0), EINVAL), ("null ws", dict(ws_p=0), EINVAL),
        ("x misaligned", dict(x_p=x.data_ptr() + 2), EINVAL), ("dx_in misaligned", dict(in_p=dxi.data_ptr() + 8), EINVAL),
        ("dx_out misaligned", dict(out_p=dx.data_ptr() + 4), EINVAL), ("x stride", dict(xr=odd), EINVAL),
        ("dn stride", dict(dnr=odd), EINVAL), ("dx_in stride", dict(inr=odd), EINVAL), ("dx_out stride", dict(outr=odd), EINVAL),
        ("modulation stride", dict(mod_bs=D + 4), EINVAL), ("B = 0", dict(b=0), EINVAL), ("rows = 0", dict(rpb=0), EINVAL),
        ("D = 1024", dict(d=1024, dsc_off=4 * 1024), EUNSUP),
        ("dscale = dshift + D - 1", dict(dsc_off=4 * (D - 1)), EINVAL), ("dscale = dshift", dict(dsc_off=0), EINVAL),
    ], [dx, dmod])

    # ---- fk_gate_res_bwd_bf16
    N = 512
    dout, y = (torch.randn(B, R_, N, device="cuda").to(BF) for _ in range(2))
    gate = torch.randn(B, N, device="cuda").to(BF)
    dy = torch.full((B, R_, N), SENT, device="cuda", dtype=BF)
    dg = torch.full((B, N), SENT, device="cuda", dtype=torch.float32)
    rows = Rows(N, R_, R_ * N)

    def gate_res(do_p=dout.data_ptr(), dor=rows, y_p=y.data_ptr(), yr=rows, g_p=gate.data_ptr(), g_bs=N, rpb=R_, dy_p=dy.data_ptr(),
                 dyr=rows, dg_p=dg.data_ptr(), ws_p=ws.data_ptr(), b=B, n=N):
        return lib.fk_gate_res_bwd_bf16(V(do_p), dor, V(y_p), yr, V(g_p), g_bs, rpb, V(dy_p), dyr, V(dg_p), N, V(ws_p), b, n, st)
    odd = Rows(N + 4, R_, R_ * N)
    refused("fk_gate_res_bwd_bf16", gate_res, [
        ("null dout", dict(do_p=0), EINVAL), ("null y", dict(y_p=0), EINVAL), ("null gate", dict(g_p=0), EINVAL),
        ("null dy", dict(dy_p=0), EINVAL), ("null dgate", dict(dg_p=0), EINVAL), ("null ws", dict(ws_p=0), EINVAL),
        ("dout misaligned", dict(do_p=dout.data_ptr() + 2), EINVAL), ("gate misaligned", dict(g_p=gate.data_ptr() + 8), EINVAL),
        ("dy misaligned", dict(dy_p=dy.data_ptr() + 4), EINVAL), ("dout stride", dict(dor=odd), EINVAL), ("y stride", dict(yr=odd), EINVAL),
        ("dy stride", dict(dyr=odd), EINVAL), ("gate stride", dict(g_bs=N + 4), EINVAL), ("B = 0", dict(b=0), EINVAL),
        ("rows = 0", dict(rpb=0), EINVAL), ("N = 0", dict(n=0), EINVAL), ("N = 12", dict(n=12), EINVAL),
    ], [dy, dg])

    # ---- fk_qkv_post_bwd_bf16
    H, S, s_txt = 2, 5, 2
    dq, dk = (torch.randn(B, H, S, 128, device="cuda").to(BF) for _ in range(2))
    qkv = torch.randn(B, S, 3 * H * 128, device="cuda").to(BF)
    w = [torch.randn(128, device="cuda").to(BF) for _ in range(4)]
    cos, sin = torch.rand(S, 128, device="cuda"), torch.rand(S, 128, device="cuda")
    dqkv = torch.full((B, S, 3 * H * 128), SENT, device="cuda", dtype=BF)
    dw = torch.full((2, 2, 128), SENT, device="cuda", dtype=torch.float32)

    def qkv_post(dq_p=dq.data_ptr(), dk_p=dk.data_ptr(), x_p=qkv.data_ptr(), o_p=dqkv.data_ptr(), wqi=w[0].data_ptr(),
                 wki=w[1].data_ptr(), wqt=w[2].data_ptr(), wkt=w[3].data_ptr(), c_p=cos.data_ptr(), s_p=sin.data_ptr(),
                 dw_p=dw.data_ptr(), ws_p=ws.data_ptr(), b=B, s=S, t=s_txt, h=H):
        return lib.fk_qkv_post_bwd_bf16(V(dq_p), V(dk_p), V(x_p), V(o_p), V(wqi), V(wki), V(wqt), V(wkt), V(c_p), V(s_p), V(dw_p),
                                        V(ws_p), b, s, t, h, 1e-6, st)
    fn = "fk_qkv_post_bwd_bf16"
    cases = [
        ("null dq", dict(dq_p=0), EINVAL), ("null dk", dict(dk_p=0), EINVAL), ("null qkv", dict(x_p=0), EINVAL),
        ("null dqkv", dict(o_p=0), EINVAL), ("null wq_img", dict(wqi=0), EINVAL), ("null wk_img", dict(wki=0), EINVAL),
        ("null cos", dict(c_p=0), EINVAL), ("null sin", dict(s_p=0), EINVAL), ("null dw", dict(dw_p=0), EINVAL),
        ("null ws", dict(ws_p=0), EINVAL), ("wq_txt missing", dict(wqt=0), EINVAL), ("wk_txt missing", dict(wkt=0), EINVAL),
        ("S_txt > S", dict(t=S + 1), EINVAL), ("S_txt < 0", dict(t=-1), EINVAL), ("B = 0", dict(b=0), EINVAL),
        ("S = 0", dict(s=0, t=0), EINVAL), ("H = 0", dict(h=0), EINVAL),
    ]
    for name, kw, want in cases:
        code = qkv_post(**kw)
        assert code == want, (fn, name, code)
        assert lib.fk_last_error().decode().startswith(fn), (fn, name)
    torch.cuda.synchronize()
    assert bool((dqkv == SENT).all()) and bool((dw == SENT).all()) and bool((ws == SENT).all()), f"{fn}: a refused call wrote"
    assert qkv_post() == 0, lib.fk_last_error().decode()
    torch.cuda.synchronize()
    D2 = 2 * H * 128
    assert not bool((dqkv[..., :D2] == SENT).any()) and bool((dqkv[..., D2:] == SENT).all()) and not bool((dw == SENT).any())
