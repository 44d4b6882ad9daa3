"""Backward kernels (csrc/backward_kernels.hip) at production sizes, against references that leave no slack.

A. Reductions over tokens on inputs whose sums are EXACT: small integers as bf16, every product and every partial sum an
   integer below 2^24, so fp32 adds are exact in any association and the kernel must equal the fp64 host sum bit for bit,
   whatever its chunking.  A dropped, doubled or misplaced row / partial row / batch entry is a whole-number error.  The
   shapes reach what the toy sizes of test_hip_backward.py do not: more than 32 partial rows (the second trip of the
   finalising kernel's loop) and the workspace-halving branch of each launcher; both premises are asserted from the shapes and
   fk_bwd_ws_floats().
B. The outputs that are not exact (dscale, dx of ln_modulate_bwd; everything of qkv_post_bwd) at the same sizes against fp64
   autograd on the host, at the tolerances test_hip_backward.py states, the atol of the fp32 reductions scaled by
   max|ref| / max|ref at that file's small shape| (the sums grow with the row count).
C. The elementwise kernels over every finite bf16 input in [-100, 100] plus zeros, subnormals and the largest finite values
   against the function in fp64 rounded to bf16 once; the un-fused forward helpers against the GEMM epilogues they restate,
   bit for bit; the second trip of the grid-stride loops at a real size (2 x 8704 x 12288).
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import bf16_ulp_diff, report

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TWO24 = float(2 ** 24)
TINY = 2.0 ** -126          # smallest normal bf16 (= smallest normal fp32)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


def randn(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def ints(*shape, seed=0):
    """Integers in [-4, 4] as bf16 (exact; a product of two is exact in bf16 as well)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g, dtype=torch.int8).to(BF)


def close_bf16(name, got, ref, tol=1.5e-2):
    """test_hip_backward.close_bf16: max error <= tol * max|ref|, mean error <= 0.2 * tol * max|ref|."""
    d = report(name, got, ref)
    scale = ref.abs().max().item()
    assert torch.isfinite(got.float()).all()
    assert d.max().item() <= tol * scale + 1e-6, f"{name}: {d.max().item():.3e} vs scale {scale:.3e}"
    assert d.mean().item() <= 0.2 * tol * scale + 1e-7


def sum_f64(x, dims, step=1024):
    """fp64 sum of a [B, R, N] tensor over ``dims`` ((1,) or (0, 1)), R in slices so the fp64 copy stays small."""
    acc = None
    for r0 in range(0, x.shape[1], step):
        s = x[:, r0:r0 + step].double().sum(1)
        acc = s if acc is None else acc + s
    return acc.sum(0) if 0 in dims else acc


def exact(ref64, bound_terms, name):
    """The premise of section A, asserted: the fp64 reference is integral and every partial sum (at most ``bound_terms`` =
    rows x max|term|) stays below 2^24.  Returns the reference as fp32 (exact)."""
    assert bound_terms < TWO24, f"{name}: partial sums may reach {bound_terms} >= 2^24"
    assert torch.equal(ref64, ref64.round()) and ref64.abs().max().item() < TWO24, f"{name}: reference not an exact fp32 integer"
    return ref64.float()


def chunks_of(rows, per_iter, max_chunks, floats_per_chunk, ws_floats):
    """(chunks before halving, chunks after) of a reduction launcher: pick_chunks, then halved while the partial rows
    (floats_per_chunk each) exceed the workspace."""
    c0 = max(1, min((rows + per_iter - 1) // per_iter, max_chunks))
    c = c0
    while c > 1 and c * floats_per_chunk > ws_floats:
        c //= 2
    return c0, c


def ws_floats():
    from gpt_image_edit_amd import libfk
    return int(libfk.load().fk_bwd_ws_floats())


def same_whole(name, got, ref):
    """Bit equality with a whole-number reference; on failure, what went wrong where."""
    got = got.cpu()
    if not torch.equal(got, ref):
        d = (got.double() - ref.double())
        bad = d.nonzero()
        raise AssertionError(f"{name}: {bad.shape[0]} of {ref.numel()} sums differ, max |d| {d.abs().max().item():.1f}, "
                             f"first at {bad[0].tolist()} (got {got[tuple(bad[0])].item()}, want {ref[tuple(bad[0])].item()})")
    print(f"[parity] {name}: bit-identical to the fp64 sum ({ref.numel()} sums, max |sum| {ref.abs().max().item():.0f})", flush=True)


# ---- A. exact sums ---------------------------------------------------------------------------------------------------------
COLSUM_M = [(1, 150), (1, 2560), (1, 8704), (2, 8704)]
COLSUM_N = [3072, 9216, 12288, 2056]
COLSUM_CASES = [(b, r, n, (i + j) % 2 == 1) for i, (b, r) in enumerate(COLSUM_M) for j, n in enumerate(COLSUM_N)] + [(1, 8192, 18432, False)]


@pytest.mark.parametrize("B,R,N,sliced", COLSUM_CASES)
def test_colsum_exact(ops, B, R, N, sliced):
    """out[n] = sum over B * R rows, 5 / 80 / 256 partial rows; ``sliced``: rows 3.. and columns 64.. of a wider buffer.
    (8192, 18432): 256 partial rows of 18432 floats exceed the workspace, the launcher halves its chunks."""
    c0, c = chunks_of(B * R, 32, 256, N, ws_floats())
    if R >= 2560:
        assert c > 32, "more than 32 partial rows: the finalising kernel's loop takes a second trip"
    if N == 18432:
        assert c0 * N > ws_floats() and c < c0, "the workspace-halving branch is taken"
    else:
        assert c == c0
    wide = ints(B, R + 3, N + 64, seed=100 + R + N) if sliced else ints(B, R, N, seed=100 + R + N)
    x = wide[:, 3:, 64:] if sliced else wide
    ref = exact(sum_f64(x, (0, 1)), 4 * B * R, "colsum")
    xd = wide.cuda()
    xd = xd[:, 3:, 64:] if sliced else xd
    xd = xd[0] if B == 1 else xd                   # [M, N] matrix or [2, R, N] view
    got, again = ops.colsum(xd), ops.colsum(xd)
    torch.cuda.synchronize()
    same_whole(f"colsum B{B} R{R} N{N}{' sliced' if sliced else ''} ({c} partial rows)", got, ref)
    assert torch.equal(got, again)


@pytest.mark.parametrize("B,R,N", [(2, 75, 3072), (1, 8704, 3072), (2, 4352, 3072), (6, 4096, 3072)])
def test_gate_res_bwd_exact(ops, B, R, N):
    """dgate[b] = sum_s dout * y and dy = dout * gate[b] on views of joint [B, S_txt + R, N] buffers; dgate into a column
    slice of a wider fp32 buffer.  (6, 4096, 3072): B * 256 * N floats exceed the workspace (halving branch)."""
    S_txt = 11
    c0, c = chunks_of(R, 16, 256, B * N, ws_floats())
    if (B, R) == (6, 4096):
        assert B * c0 * N > ws_floats() and c < c0 and c > 32, "halving branch taken, still more than 32 partial rows"
    else:
        assert c == c0 and (R < 4352 or c > 32)
    dout, y = ints(B, S_txt + R, N, seed=200 + R), ints(B, S_txt + R, N, seed=201 + R)
    mod = ints(B, 3 * N, seed=202 + R)
    ref_dg = torch.stack([exact(sum_f64((dout[b:b + 1, S_txt:].float() * y[b:b + 1, S_txt:].float()), (0, 1)), 16 * R, "dgate")
                          for b in range(B)])
    ref_dy = dout[:, S_txt:].float() * mod[:, None, N:2 * N].float()
    assert ref_dy.abs().max().item() <= 16                 # exact in bf16
    dod, yd, md = dout.cuda(), y.cuda(), mod.cuda()
    res = []
    for fill in (7.0, -3.0):
        dy = torch.full((B, S_txt + R, N), fill, device="cuda", dtype=BF)
        dg = torch.full((B, 2 * N), fill, device="cuda", dtype=torch.float32)
        ops.gate_res_bwd(dod[:, S_txt:], yd[:, S_txt:], md[:, N:2 * N], dy[:, S_txt:], dg[:, N:])
        torch.cuda.synchronize()
        assert (dy[:, :S_txt] == fill).all() and (dg[:, :N] == fill).all(), "rows / columns outside the views were written"
        res.append((dy[:, S_txt:].cpu(), dg[:, N:].cpu()))
    same_whole(f"gate_res_bwd dgate B{B} R{R} ({c} partial rows)", res[0][1], ref_dg)
    assert torch.equal(res[0][0].float(), ref_dy), "dy"
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


LN_CASES = [(2, 37, 3072), (1, 8704, 3072), (2, 8704, 3072), (3, 2560, 512)]


def _ln_chunks(B, R, D):
    c0, c = chunks_of(R, 16, 512, B * 2 * D, ws_floats())
    if (B, R, D) == (2, 8704, 3072):
        assert B * c0 * 2 * D > ws_floats() and c < c0 and c > 32, "halving branch taken, still more than 32 partial rows"
    else:
        assert c == c0 and (R < 2560 or c > 32)
    if (B, R, D) == (1, 8704, 3072):
        assert c == 512
    return c


@pytest.mark.parametrize("B,R,D", LN_CASES)
def test_ln_modulate_bwd_dshift_exact(ops, B, R, D):
    """dshift[b] = sum_s dn, up to 512 partial rows; at (2, 8704, 3072) 2 * 512 * 2 * 3072 floats exceed the workspace."""
    c = _ln_chunks(B, R, D)
    S_txt = 5
    joint = randn(B, S_txt + R, D, seed=300, scale=2.0)
    mod = randn(B, 6 * D, seed=301, scale=0.3)
    dn = ints(B, R, D, seed=302 + R)
    ref = torch.stack([exact(sum_f64(dn[b:b + 1], (0, 1)), 4 * R, "dshift") for b in range(B)])
    jd, md, dnd = joint.cuda(), mod.cuda(), dn.cuda()
    res = []
    for fill in (7.0, -3.0):
        dmod = torch.full((B, 6 * D), fill, device="cuda", dtype=torch.float32)
        out = torch.full_like(jd, fill)
        ops.ln_modulate_bwd(jd[:, S_txt:], dnd, md[:, D:2 * D], out[:, S_txt:], dmod[:, :2 * D])
        torch.cuda.synchronize()
        assert (dmod[:, 2 * D:] == fill).all() and (out[:, :S_txt] == fill).all()
        res.append((dmod[:, :2 * D].cpu(), out[:, S_txt:].cpu()))
    same_whole(f"ln_modulate_bwd dshift B{B} R{R} D{D} ({c} partial rows)", res[0][0][:, :D], ref)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("B,S,H", [(1, 64, 2), (2, 75, 3), (1, 8704, 24)])
def test_rowdot_exact(ops, B, S, H):
    """out[b, h, s] = 128 exact products; ``a`` a column slice of a wider row; (2, 75, 3): B * S * H = 450 is not a
    multiple of the 16 (row, head) units of a workgroup."""
    D = H * 128
    a_w, c = ints(B, S, D + 64, seed=400 + S), ints(B, S, D, seed=401 + S)
    a = a_w[:, :, 64:]
    assert (B * S * H) % 16 != 0 or (B, S, H) != (2, 75, 3)
    ref64 = (a.double().reshape(B, S, H, 128) * c.double().reshape(B, S, H, 128)).sum(-1).transpose(1, 2).contiguous()
    ref = exact(ref64, 16 * 128, "rowdot")
    ad, cd = a_w.cuda()[:, :, 64:], c.cuda()
    got = ops.rowdot(ad, cd, H, out=torch.full((B, H, S), 9.0, device="cuda", dtype=torch.float32))
    again = ops.rowdot(ad, cd, H)
    torch.cuda.synchronize()
    same_whole(f"rowdot B{B} S{S} H{H}", got, ref)
    assert torch.equal(got, again)


@pytest.mark.parametrize("R,C,ld", [(1, 9216, 64), (2, 18432, 64), (3, 1000, 64), (64, 512, 64)])
def test_f32_to_bf16_transposed(ops, R, C, ld):
    """dst[c, r] = bf16(src[r, c]) (one rounding, exact by nature); src a column slice; columns r >= R zeroed."""
    g = torch.Generator().manual_seed(500 + C)
    wide = torch.randn(R, C + 24, generator=g) * 3.0
    src = wide[:, 24:]
    ref = torch.zeros(C, ld, dtype=BF)
    ref[:, :R] = src.t().to(BF)
    srcd = wide.cuda()[:, 24:]
    res = []
    for fill in (7.0, -3.0):
        dst = torch.full((C, ld), fill, device="cuda", dtype=BF)
        ops.f32_to_bf16_transposed(srcd, dst)
        res.append(dst.cpu())
    assert torch.equal(res[0], ref) and torch.equal(res[1], ref)
    print(f"[parity] f32_to_bf16_transposed R{R} C{C}: bit-identical, {ld - R} pad columns zero", flush=True)


# ---- B. the same launches against fp64 autograd ------------------------------------------------------------------------------
def _ln_reference(B, R, D, S_txt):
    """Inputs as test_hip_backward.test_ln_modulate_bwd makes them, and fp64 autograd of n = LN(x) (1 + scale) + shift."""
    joint = randn(B, S_txt + R, D, seed=1, scale=2.0) + 0.5
    mod = randn(B, 6 * D, seed=2, scale=0.3)
    dn = randn(B, R, D, seed=3)
    dx_in = randn(B, S_txt + R, D, seed=4, scale=0.5)
    xr = joint[:, S_txt:].double().requires_grad_(True)
    sh = mod[:, :D].double().requires_grad_(True)
    sc = mod[:, D:2 * D].double().requires_grad_(True)
    n = F.layer_norm(xr, (D,), eps=1e-6) * (1 + sc[:, None]) + sh[:, None]
    n.backward(dn.double())
    return joint, mod, dn, dx_in, xr.grad, sh.grad, sc.grad


@pytest.mark.parametrize("B,R,D", LN_CASES[1:])
def test_ln_modulate_bwd_large_vs_fp64(ops, B, R, D):
    """dx (+ dx_in), dshift, dscale at the training sizes and in the halving branch.  Tolerances of test_hip_backward.py:
    close_bf16 default for dx; rtol 1e-3 and atol 1e-3 (dshift) / 2e-3 (dscale) x max|ref| / max|ref at R = 37 (D = 3072) or
    R = 300 (D = 512)| for the fp32 sums."""
    _ln_chunks(B, R, D)
    S_txt = 11
    small = _ln_reference(2, 37 if D == 3072 else 300, D, S_txt)
    joint, mod, dn, dx_in, dx, dsh, dsc = _ln_reference(B, R, D, S_txt)
    k_sh = dsh.abs().max().item() / small[5].abs().max().item()
    k_sc = dsc.abs().max().item() / small[6].abs().max().item()
    jd, md, dxd = joint.cuda(), mod.cuda(), dx_in.cuda()
    dmod = torch.zeros(B, 6 * D, device="cuda", dtype=torch.float32)
    out = torch.zeros_like(jd)
    ops.ln_modulate_bwd(jd[:, S_txt:], dn.cuda(), md[:, D:2 * D], out[:, S_txt:], dmod[:, :2 * D], dx_in=dxd[:, S_txt:])
    torch.cuda.synchronize()
    close_bf16(f"ln_bwd dx (+dx_in) B{B} R{R} D{D} vs fp64", out[:, S_txt:], (dx + dx_in[:, S_txt:].double()).float())
    assert out[:, :S_txt].abs().max().item() == 0
    report(f"ln_bwd dshift B{B} R{R} D{D} vs fp64 (atol x{k_sh:.1f})", dmod[:, :D], dsh)
    report(f"ln_bwd dscale B{B} R{R} D{D} vs fp64 (atol x{k_sc:.1f})", dmod[:, D:2 * D], dsc)
    torch.testing.assert_close(dmod[:, :D].cpu().double(), dsh, rtol=1e-3, atol=1e-3 * k_sh)
    torch.testing.assert_close(dmod[:, D:2 * D].cpu().double(), dsc, rtol=1e-3, atol=2e-3 * k_sc)
    assert dmod[:, 2 * D:].abs().max().item() == 0


def _qkv_post_reference(B, H, S_txt, S, cos, sin):
    """Inputs as test_hip_backward.test_qkv_post_bwd makes them; fp64 autograd of RMSNorm (with weight) + RoPE per head."""
    D = H * 128
    qkv = randn(B, S, 3 * D, seed=14)
    w = [(1 + randn(128, seed=15 + i, scale=0.1).float()).to(BF) for i in range(4)]   # q_img k_img q_txt k_txt
    dq, dk = randn(B, H, S, 128, seed=20), randn(B, H, S, 128, seed=21)
    c64, s64 = cos.double()[None, None], sin.double()[None, None]
    dx, dw = [], []
    for which, (g, w_i, w_t) in enumerate(((dq, w[0], w[2]), (dk, w[1], w[3]))):
        x = qkv[..., which * D:(which + 1) * D].double().requires_grad_(True)
        wi, wt = w_i.double().requires_grad_(True), w_t.double().requires_grad_(True)
        xh = x.view(B, S, H, 128).transpose(1, 2)
        xh = xh * torch.rsqrt(xh.pow(2).mean(-1, keepdim=True) + 1e-6)
        wsel = torch.cat([wt.expand(S_txt, 128), wi.expand(S - S_txt, 128)])          # [S, 128]
        y = xh * wsel
        yr = y.reshape(B, H, S, 64, 2)
        rot = torch.stack([-yr[..., 1], yr[..., 0]], dim=-1).flatten(3)
        (y * c64 + rot * s64).mul(g.double()).sum().backward()
        dx.append(x.grad)
        dw.append(torch.stack([wi.grad, wt.grad if S_txt else torch.zeros(128, dtype=torch.float64)]))
    return qkv, w, dq, dk, torch.cat(dx, dim=-1), torch.stack(dw)


@pytest.mark.parametrize("B,H,S_txt,S", [(1, 24, 512, 8704), (2, 24, 0, 2560)])
def test_qkv_post_bwd_large_vs_fp64(ops, B, H, S_txt, S):
    """3264 / 1920 partial rows of d(norm weight); (2, 24, 0, 2560): no text stream, wq_txt = None.  Tolerances of
    test_hip_backward.test_qkv_post_bwd: close_bf16 default for d(raw q | k), rtol 2e-3 and atol 2e-3 x max|ref| / max|ref at
    (2, 3, 21, 75)| for dw."""
    from oracle import mmdit
    from oracle.helpers import prepare_latent_image_ids
    nparts = B * H * ((S + 63) // 64)
    assert nparts > 32 and nparts * 512 <= ws_floats()
    D = H * 128

    def tables(s_txt, hh, ww):
        return mmdit.rope_tables(torch.cat([torch.zeros(s_txt, 3), prepare_latent_image_ids(hh, ww)]))
    small = _qkv_post_reference(2, 3, 21, 75, *tables(21, 6, 9))
    side = {8704 - 512: (64, 128), 2560: (40, 64)}[S - S_txt]
    cos, sin = tables(S_txt, *side)
    qkv, w, dq, dk, ref_dx, ref_dw = _qkv_post_reference(B, H, S_txt, S, cos, sin)
    k = ref_dw.abs().max().item() / small[5].abs().max().item()
    dqkv = torch.full((B, S, 3 * D), 9.0, device="cuda", dtype=BF)
    wt = (w[2].cuda(), w[3].cuda()) if S_txt else (None, None)
    args = (dq.cuda(), dk.cuda(), qkv.cuda(), dqkv, w[0].cuda(), w[1].cuda(), wt[0], wt[1], cos.cuda(), sin.cuda(), S_txt)
    dw, dw2 = ops.qkv_post_bwd(*args), ops.qkv_post_bwd(*args)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2)
    close_bf16(f"qkv_post_bwd d(q|k raw) B{B} S{S} vs fp64", dqkv[..., :2 * D], ref_dx.float())
    assert (dqkv[..., 2 * D:] == 9.0).all()
    report(f"qkv_post_bwd dw B{B} H{H} S_txt{S_txt} S{S} vs fp64 ({nparts} partial rows, atol x{k:.1f})", dw, ref_dw)
    torch.testing.assert_close(dw.cpu().double(), ref_dw, rtol=2e-3, atol=2e-3 * k)


# ---- C. elementwise kernels over the whole input range ---------------------------------------------------------------------
def round_to_bf16(x64):
    """fp64 -> the nearest bf16 (ties to even) in ONE rounding, returned as fp64 (torch's own conversion goes through
    fp32: two roundings).  Values that round beyond the largest finite bf16 become inf; below 2^-126 the grid of the
    normal numbers is used (such results are only compared with 2^-126, see bf16_close)."""
    m, e = torch.frexp(x64)
    r = torch.ldexp(torch.round(m * 256.0) / 256.0, e)
    big = torch.tensor(float.fromhex("0x1.fep127"), dtype=torch.float64)
    return torch.where(r.abs() > big, torch.sign(r) * math.inf, r)


def all_bf16_in(lo=100.0):
    """Every finite bf16 with |v| <= lo (zeros of both signs and subnormals included), then the largest finite bf16 of
    both signs and values around the points where fp32 x^2 and x^3 overflow."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    v = bits[torch.isfinite(bits.float()) & (bits.float().abs() <= lo)]
    extra = torch.tensor([float.fromhex("0x1.fep127"), -float.fromhex("0x1.fep127"), 1e13, -1e13, 1.8e19, -1.8e19, 1.9e19, -1.9e19,
                          1e30, -1e30, 500.0, -500.0, 2.0 ** -126, -2.0 ** -126]).to(BF)
    return torch.cat([v, extra])


def bf16_close(name, got, ref64, inputs, sg64=None, amp64=None):
    """got (bf16, host) against the fp64 function value: finite wherever the reference is, within 1 bf16 ulp of the reference
    rounded once; where |reference| is below the smallest normal bf16 a flush to zero is accepted (|got| <= 2^-126).

    sg64, amp64: for the activation kernels, which form sigmoid(.) in fp32 and multiply it by ``amp``.  Where the exact
    sigmoid is below 2^-126 it is not a normal fp32 number (the hardware exp2 / rcp flush it to zero) although
    amp * sigmoid may still be a normal bf16; no fp32 evaluation of that form can do better (torch's own fp32 silu returns
    -0 for x in [-91.5, -89], where x sigmoid(x) is up to 2e-37), so there the rule above is applied to the sigmoid
    instead of the result: |got| <= 2^-126 * |amp|, the bound the exact result obeys (include/fk.h states it)."""
    ok_ref = torch.isfinite(ref64)
    if sg64 is not None:
        flush = ok_ref & (sg64 < TINY) & (ref64.abs() >= TINY)
        lim = TINY * amp64.abs() * (1 + 2.0 ** -7)
        gf = got.double()
        assert torch.isfinite(gf[flush]).all() and (gf[flush].abs() <= lim[flush]).all(), \
            f"{name}: where sigmoid < 2^-126, |got| up to {gf[flush].abs().max().item():.3e} exceeds 2^-126 |amp|"
        if flush.any():
            print(f"[parity] {name}: {flush.sum().item()} results with sigmoid < 2^-126 (inputs "
                  f"{[(t[flush].float().min().item(), t[flush].float().max().item()) for t in inputs]}, |ref| up to "
                  f"{ref64[flush].abs().max().item():.3e}): {(gf[flush] == 0).sum().item()} flushed to zero", flush=True)
        ok_ref = ok_ref & ~flush
    g = got.float()
    assert torch.isfinite(g[ok_ref]).all(), f"{name}: {(~torch.isfinite(g) & ok_ref).sum().item()} non-finite outputs, e.g. at " \
        f"{[t[(~torch.isfinite(g) & ok_ref)][:4].tolist() for t in inputs]}"
    refb = round_to_bf16(ref64)
    small = ok_ref & (ref64.abs() < TINY)
    normal = ok_ref & ~small & torch.isfinite(refb)
    ulp = bf16_ulp_diff(got, refb.to(BF))
    worst = ulp[normal].max().item() if normal.any() else 0
    print(f"[parity] {name}: {normal.sum().item()} normal results, bit-equal {(ulp[normal] == 0).float().mean().item():.4f}, "
          f"max {worst} ulp; {small.sum().item()} below 2^-126, max |got| there {g[small].abs().max().item() if small.any() else 0:.3e}",
          flush=True)
    if worst > 1:
        bad = normal & (ulp > 1)
        rows = [f"in={[t[bad][i].item() for t in inputs]} got={g[bad][i].item():.6e} ref={ref64[bad][i].item():.6e} ulp={ulp[bad][i].item()}"
                for i in range(min(8, int(bad.sum())))]
        lo_hi = [(t[bad].float().min().item(), t[bad].float().max().item()) for t in inputs]
        raise AssertionError(f"{name}: {bad.sum().item()} results beyond 1 ulp; input ranges {lo_hi}; |ref| in "
                             f"[{ref64[bad].abs().min().item():.3e}, {ref64[bad].abs().max().item():.3e}]\n" + "\n".join(rows))
    assert (g[small].abs() <= TINY).all(), f"{name}: a result that should vanish is {g[small].abs().max().item():.3e}"


K0, K1 = math.sqrt(2.0 / math.pi), 0.044715


def _gelu64(x):
    return x * torch.sigmoid(2.0 * K0 * (x + K1 * x ** 3))


def _gelu_grad64(x):
    u2 = 2.0 * K0 * (x + K1 * x ** 3)
    sg, cs = torch.sigmoid(u2), torch.sigmoid(-u2)          # cs = 1 - sg without cancellation
    return sg + x * sg * cs * 2.0 * K0 * (1.0 + 3.0 * K1 * x * x)


def _gelu_sg_amp(x, df):
    """(sigmoid(2u), the factor of it in df * gelu_tanh'(x))."""
    u2 = 2.0 * K0 * (x + K1 * x ** 3)
    sg = torch.sigmoid(u2)
    return sg, None if df is None else df * (1.0 + x * torch.sigmoid(-u2) * 2.0 * K0 * (1.0 + 3.0 * K1 * x * x))


def _silu_grad64(x):
    return torch.sigmoid(x) * (1.0 + x * torch.sigmoid(-x))


def _cross(h, seconds, n_min):
    """h crossed with a handful of second operands, repeated to at least n_min elements; the length a multiple of 8 that
    is not a multiple of 2048."""
    a = h.repeat(len(seconds))
    b = torch.tensor(seconds).to(BF).repeat_interleave(h.numel())
    reps = max(1, -(-n_min // a.numel()))
    a, b = a.repeat(reps), b.repeat(reps)
    n = a.numel() // 8 * 8
    if n % 2048 == 0:
        n -= 8
    return a[:n].contiguous(), b[:n].contiguous()


DF = [1.0, -1.0, 3.140625, -0.0078125, 37.5]
ELEMENTWISE = ["gelu_bwd", "silu_bwd", "gelu_tanh", "silu", "gate_res_fwd", "true_cfg"]


@pytest.mark.parametrize("n_min", [0, 256 * 8 * 2048], ids=["every-input", "several-blocks-per-CU"])
@pytest.mark.parametrize("kernel", ELEMENTWISE)
def test_elementwise_vs_fp64(ops, kernel, n_min):
    """The function in fp64 on the bf16 inputs, rounded to bf16 once; gate_res_fwd and true_cfg are DEFINED with bf16
    rounding points (out = bf16(res + bf16(gate y)); out = bf16(neg + bf16(scale bf16(pos - neg))), include/fk.h), so their
    function is that composition evaluated in fp64 -- and true_cfg is held to the unrounded neg + scale (pos - neg) as well,
    within the three roundings' worth of error (bf16 keeps 8 significant bits: each rounding is within 2^-8 relative):
    2^-8 (2 |scale (pos - neg)| + |result|) (1 + 2^-6)."""
    h, s = _cross(all_bf16_in(), DF, n_min)
    assert h.numel() % 8 == 0 and h.numel() % 2048 != 0 and h.numel() >= n_min
    hd, sd = h.cuda(), s.cuda()
    h64, s64 = h.double(), s.double()
    name = f"{kernel} n={h.numel()}"
    if kernel == "gelu_bwd":
        bf16_close(name, ops.gelu_bwd(hd, sd).cpu(), s64 * _gelu_grad64(h64), (h, s), *_gelu_sg_amp(h64, s64))
    elif kernel == "silu_bwd":
        bf16_close(name, ops.silu_bwd(hd, sd).cpu(), s64 * _silu_grad64(h64), (h, s), torch.sigmoid(h64),
                   s64 * (1.0 + h64 * torch.sigmoid(-h64)))
    elif kernel == "gelu_tanh":
        x = hd.view(-1, 8)
        bf16_close(name, ops.gelu_tanh(x, torch.empty_like(x)).cpu().view(-1), _gelu64(h64), (h,), _gelu_sg_amp(h64, None)[0], h64)
    elif kernel == "silu":
        bf16_close(name, ops.silu(hd).cpu(), h64 * torch.sigmoid(h64), (h,), torch.sigmoid(h64), h64)
    elif kernel == "gate_res_fwd":
        # rows of 8 columns; batch b of the [B, R, 8] view multiplies by gate row b
        B = 5
        R = h.numel() // 8 // B
        y = hd[:B * R * 8].view(B, R, 8)
        res = sd[:B * R * 8].view(B, R, 8)
        gate = torch.tensor(DF).to(BF)[:, None].expand(B, 8).contiguous()
        got = ops.gate_res_fwd(res, y, gate.cuda(), torch.empty_like(y)).cpu().view(-1)
        gy = round_to_bf16(y.cpu().double() * gate.double()[:, None])
        bf16_close(name, got, (res.cpu().double() + gy).view(-1), (h[:B * R * 8], s[:B * R * 8]))
    else:
        for scale in (2.5, 1.0, -0.75, 7.0):
            got = ops.true_cfg(hd, sd, scale).cpu()
            d = round_to_bf16(h64 - s64)
            p = round_to_bf16(scale * d)
            bf16_close(f"{name} scale={scale}", got, s64 + p, (h, s))
            plain = s64 + scale * (h64 - s64)
            fin = torch.isfinite(plain) & torch.isfinite(got.double())
            bound = 2.0 ** -8 * (2.0 * (scale * (h64 - s64)).abs() + plain.abs()) * (1 + 2.0 ** -6) + TINY
            err = (got.double() - plain).abs()
            print(f"[parity] {name} scale={scale} vs unrounded fp64: max err / bound {(err[fin] / bound[fin]).max().item():.3f}", flush=True)
            assert (err[fin] <= bound[fin]).all()


def test_unfused_forward_helpers_equal_the_gemm_epilogues(ops):
    """include/fk.h: fk_gate_res_fwd_bf16 / fk_gelu_tanh_bf16 are the FK_EPI_GATE_RES / FK_EPI_GELU_TANH epilogues on a stored
    GEMM output, "same rounding points": bit for bit, on strided [B, R, N] views."""
    B, R, N, K, S_txt = 2, 300, 3072, 256, 20
    a = randn(B, S_txt + R, K, seed=600).cuda()[:, S_txt:]
    w = randn(N, K, seed=601, scale=K ** -0.5).cuda()
    bias = randn(N, seed=602).cuda()
    res = randn(B, S_txt + R, N, seed=603, scale=2.0).cuda()[:, S_txt:]
    gate = randn(B, 3 * N, seed=604, scale=0.7).cuda()[:, N:2 * N]
    plain = torch.zeros(B, S_txt + R, N + 64, device="cuda", dtype=BF)[:, S_txt:, :N]
    ops.gemm(a, w, bias=bias, out=plain)
    fused = ops.gemm(a, w, bias=bias, epilogue=ops.FK_EPI_GATE_RES, res=res, gate=gate)
    out = torch.full((B, S_txt + R, N), 5.0, device="cuda", dtype=BF)
    ops.gate_res_fwd(res, plain, gate, out[:, S_txt:])
    assert torch.equal(out[:, S_txt:], fused) and (out[:, :S_txt] == 5.0).all()
    fused = ops.gemm(a, w, bias=bias, epilogue=ops.FK_EPI_GELU_TANH)
    out = torch.full((B, S_txt + R, N), 5.0, device="cuda", dtype=BF)
    ops.gelu_tanh(plain, out[:, S_txt:])
    assert torch.equal(out[:, S_txt:], fused) and (out[:, :S_txt] == 5.0).all()
    assert fused.float().abs().max().item() > 0
    print(f"[parity] gate_res_fwd / gelu_tanh == GEMM epilogues on {B} x {R} x {N} strided views: bit-identical", flush=True)


@pytest.mark.parametrize("kernel", ["gelu_bwd", "gelu_tanh", "gate_res_fwd"])
def test_grid_stride_second_trip(ops, kernel):
    """2 x 8704 x 12288 elements: more than fk_bwd_ew_max_blocks() x 2048, so every launcher's grid is capped and its
    threads take a second trip of the grid-stride loop.  Elementwise: the result must equal, bit for bit, the same kernel on
    the two halves separately (neither reaches the cap) -- and fp64 on a sample of 2^20 elements."""
    from gpt_image_edit_amd import libfk
    M, N = 2 * 8704, 12288
    cap = int(libfk.load().fk_bwd_ew_max_blocks()) * 2048
    assert M * N > cap >= M * N // 2, "the whole launch loops, the halves do not"
    g = torch.Generator(device="cuda").manual_seed(700)
    x = (torch.randn(M, N, generator=g, device="cuda") * 2.5).to(BF)
    idx = torch.randint(0, M * N, (1 << 20,), generator=torch.Generator().manual_seed(701))
    idx[:4] = torch.tensor([0, cap - 1, cap, M * N - 1])                # both sides of the seam, both ends
    h = M // 2
    if kernel == "gelu_bwd":
        df = torch.randn(M, N, generator=g, device="cuda").to(BF)
        halves = torch.cat([ops.gelu_bwd(x[:h], df[:h]), ops.gelu_bwd(x[h:], df[h:])])
        dfs = df.view(-1)[idx.cuda()].cpu()
        got = ops.gelu_bwd(x, df, out=df)                                # in place, as the block backward runs it
        xs = x.view(-1)[idx.cuda()].cpu()
        ref, ins = dfs.double() * _gelu_grad64(xs.double()), (xs, dfs)
        extra = _gelu_sg_amp(xs.double(), dfs.double())
    elif kernel == "gelu_tanh":
        got = ops.gelu_tanh(x, torch.empty_like(x))
        halves = torch.cat([ops.gelu_tanh(x[:h], torch.empty_like(x[:h])), ops.gelu_tanh(x[h:], torch.empty_like(x[h:]))])
        xs = x.view(-1)[idx.cuda()].cpu()
        ref, ins, extra = _gelu64(xs.double()), (xs,), (_gelu_sg_amp(xs.double(), None)[0], xs.double())
    else:
        res = torch.randn(M, N, generator=g, device="cuda").to(BF)
        gate = torch.randn(2, N, generator=g, device="cuda").to(BF)
        x3, r3 = x.view(2, M // 2, N), res.view(2, M // 2, N)
        got = ops.gate_res_fwd(r3, x3, gate, torch.empty_like(x3)).view(M, N)
        halves = torch.cat([ops.gate_res_fwd(r3[b:b + 1], x3[b:b + 1], gate[b:b + 1], torch.empty_like(x3[b:b + 1])) for b in (0, 1)]).view(M, N)
        xs, rs = x.view(-1)[idx.cuda()].cpu(), res.view(-1)[idx.cuda()].cpu()
        gs = gate[(idx // (h * N)).cuda(), (idx % N).cuda()].cpu()
        ref, ins, extra = rs.double() + round_to_bf16(xs.double() * gs.double()), (xs, rs, gs), ()
    torch.cuda.synchronize()
    assert torch.equal(got, halves), f"{kernel}: first difference at element {(got != halves).view(-1).nonzero()[0].item()}"
    bf16_close(f"{kernel} {M} x {N} (second grid-stride trip), 2^20 samples", got.view(-1)[idx.cuda()].cpu(), ref, ins, *extra)


@pytest.mark.parametrize("split", [0, 7, 149, 150])
def test_ln_modulate2_equals_two_ln_modulate(ops, split):
    """Rows [0, split) of every batch with modulation (a), the rest with (b): bit for bit what fk_ln_modulate_bf16 gives on
    the two row ranges; split at 0, at a row count that is not a multiple of 4, at the last row, and past it."""
    B, R, D = 2, 150, 3072
    x = randn(B, R + 5, D, seed=800, scale=2.0).cuda()[:, 5:]
    mod = randn(B, 4 * D, seed=801, scale=0.4).cuda()
    sa, ca, sb, cb = (mod[:, i * D:(i + 1) * D] for i in range(4))
    got = ops.ln_modulate2(x, sa, ca, sb, cb, split, out=torch.full((B, R, D), 5.0, device="cuda", dtype=BF))
    want = torch.empty(B, R, D, device="cuda", dtype=BF)
    if split > 0:
        ops.ln_modulate(x[:, :split], sa, ca, out=want[:, :split])
    if split < R:
        ops.ln_modulate(x[:, split:], sb, cb, out=want[:, split:])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.isfinite(got.float()).all() and got.float().abs().max().item() > 0
    print(f"[parity] ln_modulate2 split={split} of {R} rows: bit-identical to ln_modulate on the two row ranges", flush=True)


@pytest.mark.parametrize("B,C,Cpad,H,W", [(2, 3, 32, 17, 23), (1, 16, 32, 64, 64), (1, 3, 3, 5, 7)])
def test_nhwc_f32_to_nchw(ops, B, C, Cpad, H, W):
    """dst[b, c, y, x] = (src[b, y, x, c] + add) * mul in fp32 (two roundings: torch's fp32 ops are the exact reference);
    channels c >= C of the padded source are dropped."""
    g = torch.Generator().manual_seed(900 + C)
    src = torch.randn(B, H, W, Cpad, generator=g) * 3.0
    for add, mul in ((0.0, 1.0), (1.0, 127.5), (-0.1159, 1.0 / 0.3611)):
        got = ops.nhwc_f32_to_nchw(src.cuda(), C, add=add, mul=mul).cpu()
        a32, m32 = torch.tensor(add, dtype=torch.float32), torch.tensor(mul, dtype=torch.float32)
        want = ((src[..., :C].permute(0, 3, 1, 2) + a32) * m32).contiguous()
        assert got.shape == (B, C, H, W) and torch.equal(got, want), f"add={add} mul={mul}"
    print(f"[parity] nhwc_f32_to_nchw B{B} C{C}/{Cpad} {H}x{W}: bit-identical to permute + fp32 (x + add) * mul", flush=True)


def test_adamw_step_scaled_equals_adamw_step_on_prescaled_gradient(ops):
    """fk_adamw_step_scaled(grad, grad_scale, sumsq(grad)) against fk_adamw_step(grad_scale * grad, sumsq(grad_scale * grad)):
    with grad_scale a power of two the pre-scaled gradient is exact and the two differ only in where the clipping
    coefficient is rounded.  Tolerance of test_adamw_with_clipping_matches_torch (rtol 3e-6, atol 3e-8); also beside
    torch.optim.AdamW on the pre-scaled gradient (printed)."""
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    torch.manual_seed(5)
    n, scale = 257 * 33 + 5, 0.125
    ref = torch.nn.Parameter(torch.randn(n) * 0.02)
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
    st = {k: [ref.detach().clone().cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"),
              torch.empty(n, device="cuda", dtype=BF)] for k in ("scaled", "plain")}
    for step in range(1, 5):
        for clip in (step < 4,):                                        # the last step without clipping
            g = torch.randn(n) * (24.0 if step == 1 else 0.08)          # stored sums: 8 x the gradient applied
            ref.grad = g * scale
            if clip:
                torch.nn.utils.clip_grad_norm_([ref], 1.0)
            opt.step()
            gd, gs = g.cuda(), (g * scale).cuda()
            ss, ss_s = (ops.sumsq([gd]), ops.sumsq([gs])) if clip else (None, None)
            m, ea, es, b16 = st["scaled"]
            ops.adamw_step(m, gd, ea, es, step, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, grad_sumsq=ss,
                           max_grad_norm=1.0, param_bf16=b16, grad_scale=scale)
            m, ea, es, b16 = st["plain"]
            libfk.check(lib.fk_adamw_step(p(m), p(b16), p(gs), 0, p(ea), p(es), p(ss_s), 1.0, 1e-3, 0.9, 0.99, 1e-8, 1e-2, step, n,
                                          stream), "fk_adamw_step")
            torch.cuda.synchronize()
            for i, what in enumerate(("master", "exp_avg", "exp_avg_sq")):
                report(f"adamw_step_scaled vs adamw_step step {step} clip={clip} {what}", st["scaled"][i], st["plain"][i])
                torch.testing.assert_close(st["scaled"][i], st["plain"][i], rtol=3e-6, atol=3e-8)
            report(f"adamw_step_scaled step {step} master vs torch.optim.AdamW", st["scaled"][0], ref.detach())
            assert torch.equal(st["scaled"][3].cpu(), st["scaled"][0].cpu().to(BF))
