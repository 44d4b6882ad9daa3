"""Host reference of the two backward kernels with real arithmetic (csrc/backward_kernels.hip: ln_modulate_bwd_kernel,
qkv_post_bwd_kernel) and of gate_res_bwd, and the bounds that hold EVERY element they write.  The rule itself -- the float64
value of the one float32 stage, every bf16 a stated margin around it can round to, the output one of them bit for bit -- is
forward_ref's (rn_bf16, candidates, judge, unambiguous_mask, Verdict); here are the float64 values, the scales of their float32
error, float32 emulations of the kernels' own order, and the bounds of the float32 sums.

dx of ln_modulate_bwd (ln_bwd_ref).  With ln = (x - mean) rstd, gl = dn (1 + scale), m1 = mean(gl), m2 = mean(gl ln):
    z = rstd (gl - m1 - ln m2) (+ dx_in)
The three terms cancel (m1 and ln m2 are O(1 / sqrt(D)) of gl on random data, all of it where 1 + scale = 0), so the float32 error
is measured against the sum of absolute values at every cancellation, never against |z| alone: one float32 ulp of a term is many
ulps of z there, which is why an ulp count is the wrong tool.  With A1 = mean(|gl|), A2 = mean(|gl ln|), mu = |mean| rstd (the
error of the mean moves every ln of the row by the same mu u: forward_ref's factor):
    scale = rstd (|gl| + A1 + |ln| A2 + mu (A2 + |ln| A1)) + |dx_in| + |z|
(mu A2 >= mu |m2|: ln's own error times m2; mu |ln| A1 >= |ln| |mean(gl) mu|: the same error inside m2; |dx_in| + |z| bounds both
operands of the final add).  delta = LN_C u scale, u = 2^-24.

d(raw q | k) of qkv_post_bwd (qkv_post_bwd_ref).  Per pair (g0, g1) of the incoming gradient, gy0 = g0 c0 + g1 s1,
gy1 = g1 c1 - g0 s0 (the RoPE adjoint), rs = rsqrt(mean(x^2) + eps), xh = x rs, gg = gy w, dot = mean(gg xh):
    z = rs (gg - xh dot)
    scale = rs (ga + |xh| mean(ga |xh|)) + |z|,  ga = (|g0 c| + |g1 s|) |w|
ga, not |gg|: where the adjoint's two products cancel, |gg| is far below their rounding errors (a plain float32 restatement is
hundreds of u |gg| off).  |z| for what acts on the whole value: the error of rs and the rounding of the last product.
delta = QKV_C u scale.

The constants.  emulate_ln_bwd / emulate_qkv_post_bwd are the kernels' float32 arithmetic on the CPU in the kernels' order: 8
elements per lane, NV = D / 512 vectors per lane and the xor-shuffle tree over 64 lanes for the LayerNorm kernel, 16 lanes for
the per-head kernel, no fma, rsqrt correctly rounded.  Worst |emulation - float64| / (u scale) over the inputs of the GPU test,
with and without dx_in (tests/test_backward_ref.py asserts that the emulations stay within a quarter of the margins):
    ln_modulate_bwd   D = 512: 1.46    D = 3072: 1.69      4 x 1.69 = 6.8  -> LN_C  = 8
    qkv_post_bwd      head dim 128: 2.29                   4 x 2.29 = 9.2  -> QKV_C = 16
(four times the measurement, rounded up to a power of two).  The factor of four is for what the device does differently: its
rsqrtf (within an ulp of the correctly rounded one) and the multiply-adds the compiler fuses.
With these constants the rule leaves a choice for at most 0.39 % of the elements of any case (AMBIGUOUS_CAP = 0.5 %; at D = 512
and one row that is 2 elements, and the seeds of ln_bwd_inputs are such that no case has 3).

The float32 sums.  Each is a fixed-order recursive sum; a term that passes through n float32 additions picks up at most
n u sum|terms| (first order; gamma_n = n u / (1 - n u) is used), and a term that is itself a rounded float32 expression adds its
own relative error k u:
    bound = gamma(k + n) sum|terms|,  the |terms| from the float64 values
  dshift = sum_r dn          k = 0 (bf16 terms are exact)                     |term| = |dn|
  dscale = sum_r dn ln       k = LN_TERM_K = 16 + 1                            |term| = |dn| (|ln| + mu)
           (ln is forward_ref's float32 stage: within its margin 16 u (|ln| + mu); one rounding of the product)
  n (ln_chain): the launcher takes c = pick_chunks(R, 16, 512) = min(ceil(R / 16), 512) workgroups per batch entry; wave w of
           workgroup k adds rows 4 k + w, 4 k + w + 4 c, ...: ceil(R / (4 c)) additions; the four waves add in LDS one after the
           other: 3; finalize_partials_kernel: 8 running sums per part-group take every 32nd partial row: ceil(c / 32), their
           tree: 3, the four groups: 3.
  dw     = sum_(b,h,s) gy xh  k = QKV_TERM_K = 16 + 3 + 1                      |term| = (|g0 c| + |g1 s|) |xh|
           (xh is forward_ref's RMSNorm stage, margin 16 u |xh|; gy is two products and a sum; one rounding of the product)
  n (dw_chain): 4 rows per thread, 16 row groups added one after the other, then the finalizer over
           P = B H ceil(S / 64) partial rows: ceil(P / 32) + 3 + 3.
  dgate  = sum_r dout y      k = 0 (a product of two bf16 is exact in float32) |term| = |dout y|
  n (gate_chain): c = pick_chunks(R, 16, 256) workgroups, each adds rows k, k + c, ...: ceil(R / c); finalizer as above.
emulate_token_sum / emulate_finalize restate that order in float32 and tests/test_backward_ref.py holds them to the bounds.

gate_res_bwd's dy is one product of two bf16 values rounded once: torch's bf16 multiply on the CPU, bit for bit (gate_res_ref).
"""
import torch

from forward_ref import BF, U, Verdict, _butterfly, bf16_next, candidates, judge, qkv_heads, rn_bf16, unambiguous_mask  # noqa: F401

AMBIGUOUS_CAP = 5e-3          # forward_ref.AMBIGUOUS_CAP's value for the norms: a condition on the inputs, not a measurement
LN_C = 8
QKV_C = 16
LN_TERM_K = 17
QKV_TERM_K = 20
F32 = torch.float32


def _eps32(eps):
    return float(torch.tensor(eps, dtype=F32))


def gamma(n):
    return n * U / (1 - n * U)


def cdiv(a, b):
    return -(-a // b)


# ---- the launchers' chunking -----------------------------------------------------------------------------------------------------
def pick_chunks(rows, per_iter, max_chunks):
    return max(1, min(cdiv(rows, per_iter), max_chunks))


def finalize_chain(nparts):
    return cdiv(nparts, 32) + 3 + 3


def ln_chain(R):
    c = pick_chunks(R, 16, 512)
    return cdiv(R, 4 * c) + 3 + finalize_chain(c)


def gate_chain(R):
    c = pick_chunks(R, 16, 256)
    return cdiv(R, c) + finalize_chain(c)


def dw_chain(B, H, S):
    return 4 + 16 + finalize_chain(B * H * cdiv(S, 64))


# ---- float64 references ----------------------------------------------------------------------------------------------------------
def ln_bwd_ref(x, dn, scale, dx_in=None, eps=1e-6):
    """x, dn [B, R, D] bf16, scale [B, D] bf16, dx_in [B, R, D] bf16 or None.  dict of float64: z (dx before its rounding),
    err (the scale of z's float32 error, see the module docstring), dshift, dscale [B, D], and the two sums' bounds."""
    x, dn = x.double(), dn.double()
    R = x.shape[1]
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + _eps32(eps))
    ln = (x - mean) * rstd
    gl = dn * (1.0 + scale.double())[:, None]
    m1 = gl.mean(-1, keepdim=True)
    m2 = (gl * ln).mean(-1, keepdim=True)
    a1 = gl.abs().mean(-1, keepdim=True)
    a2 = (gl * ln).abs().mean(-1, keepdim=True)
    mu = mean.abs() * rstd
    z = rstd * (gl - m1 - ln * m2)
    err = rstd * (gl.abs() + a1 + ln.abs() * a2 + mu * (a2 + ln.abs() * a1))
    if dx_in is not None:
        z = z + dx_in.double()
        err = err + dx_in.double().abs()
    err = err + z.abs()
    n = ln_chain(R)
    return dict(z=z, err=err, dshift=dn.sum(1), dscale=(dn * ln).sum(1),
                dshift_bound=gamma(n) * dn.abs().sum(1), dscale_bound=gamma(LN_TERM_K + n) * (dn.abs() * (ln.abs() + mu)).sum(1))


def qkv_rows_weight(w_img, w_txt, S, s_txt):
    """[S, 128]: the text weight for tokens s < s_txt, the image weight for the others."""
    if s_txt == 0:
        return w_img.expand(S, 128)
    return torch.where((torch.arange(S) < s_txt)[:, None], w_txt[None], w_img[None])


def qkv_post_bwd_ref(dq, dk, qkv, w, cos, sin, s_txt, eps=1e-6):
    """dq, dk [B, H, S, 128] bf16, qkv [B, S, 3 H 128] bf16, w = (q_img, k_img, q_txt, k_txt) bf16 [128] (the text ones unused
    when s_txt = 0), cos / sin float32 [S, 128].  dict of float64: z, err [B, S, 2 H 128] (the q and k thirds of dqkv), dw
    [which 2][stream 2 (0 = image, 1 = text)][128] and its bound."""
    B, S, D3 = qkv.shape
    H = D3 // 384
    c, s = cos.double(), sin.double()
    txt = (torch.arange(S) < s_txt)[:, None]
    zs, errs, dws, bounds = [], [], [], []
    for which, g in enumerate((dq, dk)):
        x = qkv_heads(qkv, which).double()
        g0, g1 = g.double()[..., 0::2], g.double()[..., 1::2]
        gy = torch.stack([g0 * c[:, 0::2] + g1 * s[:, 1::2], g1 * c[:, 1::2] - g0 * s[:, 0::2]], dim=-1).flatten(-2)
        ga = torch.stack([(g0 * c[:, 0::2]).abs() + (g1 * s[:, 1::2]).abs(), (g1 * c[:, 1::2]).abs() + (g0 * s[:, 0::2]).abs()],
                         dim=-1).flatten(-2)
        rs = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + _eps32(eps))
        xh = x * rs
        wr = qkv_rows_weight(w[which], w[2 + which], S, s_txt).double()
        gg = gy * wr
        z = rs * (gg - xh * (gg * xh).mean(-1, keepdim=True))
        err = rs * (ga * wr.abs() + xh.abs() * (ga * wr.abs() * xh.abs()).mean(-1, keepdim=True)) + z.abs()
        zs.append(z.transpose(1, 2).reshape(B, S, H * 128))
        errs.append(err.transpose(1, 2).reshape(B, S, H * 128))
        t, ta = gy * xh, ga * xh.abs()
        dws.append(torch.stack([(t * ~txt).sum((0, 1, 2)), (t * txt).sum((0, 1, 2))]))
        bounds.append(torch.stack([(ta * ~txt).sum((0, 1, 2)), (ta * txt).sum((0, 1, 2))]))
    return dict(z=torch.cat(zs, -1), err=torch.cat(errs, -1), dw=torch.stack(dws),
                dw_bound=gamma(QKV_TERM_K + dw_chain(B, H, S)) * torch.stack(bounds))


def gate_res_ref(dout, y, gate):
    """dout, y [B, R, N] bf16, gate [B, N] bf16 -> (dy: the torch bf16 product, one rounding of an exact float32 product;
    dgate float64 [B, N]; its bound)."""
    t = dout.double() * y.double()
    return dout * gate[:, None], t.sum(1), gamma(gate_chain(dout.shape[1])) * t.abs().sum(1)


def accept(ref, c):
    """(alternatives, wide) for forward_ref.judge from a reference dict: the candidates of z under delta = c u err."""
    lo, hi, wide = candidates(ref["z"], c * U * ref["err"])
    return [lo, hi], wide


def observed_share(got, ref, c):
    """What an output tells of its float32 stage: where got is not rn(z), the stage lay on got's side of the rounding boundary
    between rn(z) and its neighbour, at least |boundary - z| from z.  Returns the largest such distance as a share of
    delta = c u err (0 where every element is rn(z)); at most 1 for an output that passes the rule."""
    z, delta = ref["z"], c * U * ref["err"]
    g = got.cpu().double()
    b0 = rn_bf16(z)
    moved = (g != b0) & (delta > 0)
    if not moved.any():
        return 0.0
    towards = torch.where(g > b0, bf16_next(b0), -bf16_next(-b0))
    return float((((b0 + towards) / 2 - z).abs() / delta)[moved].max())


def worst_share(got, ref64, bound):
    """largest |got - ref| / bound over the elements with a bound > 0; where the bound is 0 the sum must be the reference."""
    d = (got.double().cpu() - ref64).abs()
    pos = bound > 0
    assert bool((d[~pos] == 0).all()), "a sum whose terms are all zero is not zero"
    return float((d[pos] / bound[pos]).max()) if pos.any() else 0.0


# ---- float32 emulations of the kernels' order ------------------------------------------------------------------------------------
def emulate_finalize(part):
    """finalize_partials_kernel on part [nparts, n] float32: group g of 4 keeps 8 running sums, sum u taking the partial rows
    g + 4 u + 32 j; ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)); then ((s0 + s1) + s2) + s3."""
    nparts, n = part.shape
    s = []
    for grp in range(4):
        a = [torch.zeros(n) for _ in range(8)]
        for i in range(grp, nparts, 32):
            for u in range(8):
                if i + 4 * u < nparts:
                    a[u] = a[u] + part[i + 4 * u]
        s.append(((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])))
    return ((s[0] + s[1]) + s[2]) + s[3]


def emulate_token_sum(t, skip_row=None):
    """The two-stage sum over the rows of t [B, R, D] float32 as ln_modulate_bwd_kernel + the finalizer order it -> [B, D].
    skip_row: the planted error of one row left out."""
    B, R, D = t.shape
    c = pick_chunks(R, 16, 512)
    part = torch.zeros(B, c, D)
    for k in range(c):
        for w in range(4):
            a = torch.zeros(B, D)
            for r in range(4 * k + w, R, 4 * c):
                if r != skip_row:
                    a = a + t[:, r]
            part[:, k] = a if w == 0 else part[:, k] + a
    return torch.stack([emulate_finalize(part[b]) for b in range(B)])


LN_MUTANTS = ("m1 dropped", "m1 halved", "m2 dropped", "1 + scale taken as scale", "dx_in of the neighbouring row",
              "dscale from gl", "one row left out of dscale")


def emulate_ln_bwd(x, dn, scale, dx_in=None, eps=1e-6, mutant=None, rounded=True):
    """ln_modulate_bwd_kernel<D / 512> in float32 on the CPU: lane l of 64 holds columns 512 i + 8 l .. + 7, i < NV; the row sum
    adds pairs, the other three row sums add element by element, each through the xor butterfly (32 .. 1) and times fl(1 / D);
    rstd the correctly rounded 1 / sqrt; d = rstd ((gl - m1) - ln m2) + dx_in.  Returns (dx bf16 -- float32 when not rounded --,
    dshift, dscale float32 [B, D]).  mutant: one of LN_MUTANTS, the planted mistakes."""
    assert mutant is None or mutant in LN_MUTANTS
    B, R, D = x.shape
    NV = D // 512
    inv_d = torch.tensor(1.0 / D, dtype=F32)
    v = x.float().reshape(B * R, NV, 64, 8)
    g = dn.float().reshape(B * R, NV, 64, 8)
    gsc = scale.float() if mutant == "1 + scale taken as scale" else 1.0 + scale.float()
    gsc = gsc[:, None].expand(B, R, D).reshape(B * R, NV, 64, 8)
    s = torch.zeros(B * R, 64)
    for i in range(NV):
        for e in range(4):
            s = s + (v[:, i, :, 2 * e] + v[:, i, :, 2 * e + 1])
    mean = _butterfly(s)[:, :1] * inv_d
    v = v - mean[:, None, None]
    q = torch.zeros_like(s)
    for i in range(NV):
        for e in range(8):
            q = q + v[:, i, :, e] * v[:, i, :, e]
    rstd = (1.0 / torch.sqrt((_butterfly(q)[:, :1] * inv_d + torch.tensor(eps, dtype=F32)).double())).float()[:, None, None]
    ln = v * rstd
    gl = g * gsc
    m1, m2 = torch.zeros_like(s), torch.zeros_like(s)
    for i in range(NV):
        for e in range(8):
            m1 = m1 + gl[:, i, :, e]
            m2 = m2 + gl[:, i, :, e] * ln[:, i, :, e]
    m1 = (_butterfly(m1)[:, :1] * inv_d)[:, None, None]
    m2 = (_butterfly(m2)[:, :1] * inv_d)[:, None, None]
    if mutant == "m1 dropped":
        m1 = torch.zeros_like(m1)
    if mutant == "m1 halved":
        m1 = m1 * 0.5
    if mutant == "m2 dropped":
        m2 = torch.zeros_like(m2)
    d = (rstd * ((gl - m1) - ln * m2)).reshape(B, R, D)
    if dx_in is not None:
        d = d + (torch.roll(dx_in, 1, dims=1) if mutant == "dx_in of the neighbouring row" else dx_in).float()
    else:
        d = d + 0.0               # the kernel adds the +0 it holds in place of dx_in: a -0 (gl = 0 (1 + scale) with scale < -1) becomes +0
    dshift = emulate_token_sum(g.reshape(B, R, D))
    dscale = emulate_token_sum(((gl if mutant == "dscale from gl" else g) * ln).reshape(B, R, D),
                               skip_row=R // 2 if mutant == "one row left out of dscale" else None)
    return (d.to(BF) if rounded else d), dshift, dscale


QKV_MUTANTS = ("mean of squares over 127", "eps 1e-5", "text weight for the first image row", "sin[2e] and sin[2e + 1] swapped",
               "dot scaled by 0.9", "clamped row beyond S counted into dw", "one 64-row block left out of dw")


def emulate_qkv_post_bwd(dq, dk, qkv, w, cos, sin, s_txt, eps=1e-6, mutant=None, rounded=True):
    """qkv_post_bwd_kernel in float32 on the CPU: 16 lanes x 8 elements per head row; per lane four steps
    ss += x0 x0 + x1 x1 and dot += gg0 xh0 + gg1 xh1, each through the xor butterfly (8 .. 1) and times fl(1 / 128); the adjoint
    gy0 = g0 c0 + g1 s1, gy1 = g1 c1 - g0 s0 as two rounded products and one sum; out = rs (gg - xh dot).  dw: thread (row group
    r0 of 16) adds its rows r0, r0 + 16, r0 + 32, r0 + 48 of the 64-row block, the 16 groups add one after the other, the
    finalizer adds the blocks in (b, h, block) order.  Returns (the q and k thirds [B, S, 2 H 128] bf16 -- float32 when not
    rounded --, dw float32 [2][2][128]).  mutant: one of QKV_MUTANTS."""
    assert mutant is None or mutant in QKV_MUTANTS
    B, S, D3 = qkv.shape
    H = D3 // 384
    nb = cdiv(S, 64)
    inv = torch.tensor(1.0 / (127 if mutant == "mean of squares over 127" else 128), dtype=F32)
    inv_dot = torch.tensor(1.0 / 128, dtype=F32)
    eps32 = torch.tensor(1e-5 if mutant == "eps 1e-5" else eps, dtype=F32)
    cut = s_txt + 1 if mutant == "text weight for the first image row" and s_txt else s_txt
    txt = torch.arange(nb * 64).clamp(max=S - 1) < s_txt
    se, so = (sin[:, 1::2], sin[:, 0::2]) if mutant == "sin[2e] and sin[2e + 1] swapped" else (sin[:, 0::2], sin[:, 1::2])
    outs, parts = [], []
    for which, g in enumerate((dq, dk)):
        x = qkv_heads(qkv, which).float()
        g0, g1 = g.float()[..., 0::2], g.float()[..., 1::2]
        gy = torch.stack([g0 * cos[:, 0::2] + g1 * so, g1 * cos[:, 1::2] - g0 * se], dim=-1).flatten(-2)
        xl = x.reshape(-1, 16, 8)
        ss = torch.zeros(xl.shape[0], 16)
        for e in range(4):
            ss = ss + (xl[:, :, 2 * e] * xl[:, :, 2 * e] + xl[:, :, 2 * e + 1] * xl[:, :, 2 * e + 1])
        rs = (1.0 / torch.sqrt((_butterfly(ss)[:, :1] * inv + eps32).double())).float().reshape(B, H, S, 1)
        xh = x * rs
        gg = gy * qkv_rows_weight(w[which], w[2 + which], S, cut).float()
        ggl, xhl = gg.reshape(-1, 16, 8), xh.reshape(-1, 16, 8)
        dot = torch.zeros_like(ss)
        for e in range(4):
            dot = dot + (ggl[:, :, 2 * e] * xhl[:, :, 2 * e] + ggl[:, :, 2 * e + 1] * xhl[:, :, 2 * e + 1])
        dot = (_butterfly(dot)[:, :1] * inv_dot).reshape(B, H, S, 1)
        if mutant == "dot scaled by 0.9":
            dot = dot * 0.9
        out = rs * (gg - xh * dot)
        outs.append(out.transpose(1, 2).reshape(B, S, H * 128))
        # d(norm weight): rows beyond S hold nothing (the planted error: the clamped row S - 1 once more)
        t = torch.zeros(B, H, nb * 64, 128)
        t[:, :, :S] = gy * xh
        if mutant == "clamped row beyond S counted into dw":
            t[:, :, S:] = t[:, :, S - 1:S]
        per_stream = []
        for m in (~txt, txt):
            tm = (t * m[:, None]).reshape(B, H, nb, 4, 16, 128)
            a = torch.zeros(B, H, nb, 16, 128)
            for i in range(4):
                a = a + tm[:, :, :, i]
            tot = torch.zeros(B, H, nb, 128)
            for r in range(16):
                tot = tot + a[:, :, :, r]
            per_stream.append(tot.reshape(B * H * nb, 128))
        parts.append(torch.stack(per_stream, dim=1))                  # [blocks, stream, 128]
    part = torch.stack(parts, dim=1).reshape(B * H * nb, 512)         # [blocks][which][stream][128]
    if mutant == "one 64-row block left out of dw":
        part = part[:-1]
    out = torch.cat(outs, -1)
    return (out.to(BF) if rounded else out), emulate_finalize(part).reshape(2, 2, 128)


def emulate_gate_sum(t):
    """gate_res_bwd_kernel's dgate order on the float32 products t [B, R, N]: workgroup k of c adds rows k, k + c, ...; the
    finalizer adds the c partial rows."""
    B, R, N = t.shape
    c = pick_chunks(R, 16, 256)
    part = torch.zeros(B, c, N)
    for k in range(c):
        for r in range(k, R, c):
            part[:, k] = part[:, k] + t[:, r]
    return torch.stack([emulate_finalize(part[b]) for b in range(B)])


# ---- the inputs of tests/test_hip_backward_elements.py (and of the CPU test that holds them to the cap) -----------------------
LN_DS = (512, 3072)
LN_BS = (1, 3)
LN_RS = (1, 3, 4, 5, 16, 17, 37, 300)
S_TXT = 3                          # x, dx_in, dx_out are rows [S_TXT:] of [B, S_TXT + R, D] buffers
QKV_CASES = ((1, 1, 0, 1), (2, 3, 21, 75), (1, 2, 0, 63), (1, 2, 64, 64), (2, 2, 65, 65), (1, 3, 37, 130), (1, 24, 16, 80))
GATE_CASE = (2, 75, 3072)


def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ln_bwd_inputs(D, B, R):
    """(x buffer [B, S_TXT + R, D], dn [B, R, D], mod [B, 6 D], dx_in buffer like x), all bf16; scale = mod[:, D:2 D].
    scale = -1 on columns [64, 72) of batch 0 (1 + scale = 0: gl = 0 there and z is the two projection terms alone).  Special
    rows of the x view in the last batch: R >= 5: row 1 constant (variance 0, rstd = eps^-1/2), row 3 with dn = 0 (dx must be
    dx_in's bits, or +0 without it); R >= 37: row 2 with |mean| / std = 32.  That row's margin is some 20 times an ordinary
    row's (mu = 32) and about 4 % of its elements are ambiguous: among fewer rows it alone would exceed the cap."""
    xb = (_randn(B, S_TXT + R, D, seed=1004 + D + R, scale=2.0) + 0.5).to(BF)
    dn = _randn(B, R, D, seed=1005 + D + R).to(BF)
    mod = _randn(B, 6 * D, seed=1006 + D, scale=0.3).to(BF)
    dxb = _randn(B, S_TXT + R, D, seed=1007 + D + R, scale=0.5).to(BF)
    mod[0, D + 64:D + 72] = -1.0
    x = xb[:, S_TXT:]
    if R >= 5:
        x[B - 1, 1] = 2.0 ** -9
        dn[B - 1, 3] = 0.0
    if R >= 37:
        x[B - 1, 2] = (64 + _randn(D, seed=1008, scale=2.0)).to(BF)
    return xb, dn, mod, dxb


def qkv_bwd_inputs(B, H, s_txt, S):
    """(dq, dk [B, H, S, 128], qkv [B, S, 3 H 128], w = (q_img, k_img, q_txt, k_txt)) bf16 and cos, sin float32 [S, 128] of
    independent random angles: every (even, odd) pair of a table row holds two different values, so a pair-index mistake shows
    (position tables repeat each value; the kernel's contract is any float32 [S, 128]).  q's head 0 of the last token of the last
    batch entry is all zero (rs = eps^-1/2)."""
    D = H * 128
    dq, dk = _randn(B, H, S, 128, seed=2000 + S).to(BF), _randn(B, H, S, 128, seed=2001 + S).to(BF)
    qkv = _randn(B, S, 3 * D, seed=2002 + S).to(BF)
    qkv[B - 1, S - 1, :128] = 0.0
    w = tuple((1 + _randn(128, seed=2003 + i, scale=0.1)).to(BF) for i in range(4))
    ang = torch.rand(S, 128, generator=torch.Generator().manual_seed(2007 + S), dtype=torch.float64) * 6.283185307179586
    cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    assert bool((cos[:, 0::2] != cos[:, 1::2]).all()) and bool((sin[:, 0::2] != sin[:, 1::2]).all())
    return dq, dk, qkv, w, cos, sin


def gate_inputs(B, R, N):
    """(dout buffer, y buffer [B, S_TXT + R, N], mod [B, 3 N]) bf16; gate = mod[:, N:2 N]."""
    return (_randn(B, S_TXT + R, N, seed=3000).to(BF), _randn(B, S_TXT + R, N, seed=3001, scale=2.0).to(BF),
            _randn(B, 3 * N, seed=3002, scale=0.5).to(BF))
