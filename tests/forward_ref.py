"""Host reference of the forward small kernels (csrc/norm_kernels.hip, csrc/elementwise.hip) and the rule that accepts or
rejects a kernel's output ELEMENT BY ELEMENT -- no share of elements is allowed to be wrong.

Each kernel has one float32 stage whose result is rounded to bf16.  Everything after that rounding (the "tail") is exact or
specified rounding by rounding in include/fk.h, and torch on the CPU restates it bit for bit: a product of two bf16 values is
exact in float32, so `a * b` on bf16 tensors is the kernel's `round_bf(a * b)`, and a float32 `*` or `+` of torch is one IEEE
operation (never an fma).

The rule, for the float32 stage:
  * z = the stage's value in float64 (error ~1e-16, nothing beside the margins below);
  * candidates = every bf16 that is the round-to-nearest-even of some value in [z - delta, z + delta]: round-to-nearest is
    monotone, so these are the bf16 values from rn(z - delta) to rn(z + delta) -- one almost always, two next to a rounding
    boundary, more only where delta exceeds a bf16 ulp of z (z next to 0 under an absolute delta);
  * every candidate goes through the tail; the kernel's output must equal one of the results BIT FOR BIT.  Where there are more
    than two candidates the tail's results for the two end candidates bound the accepted values (every tail here is monotone in
    the candidate), which is the same set wherever the candidates are dense (they are: next to 0).
An element is AMBIGUOUS when the rule accepts more than one bit pattern for it.  That depends only on the input and delta, never
on a kernel; the share is capped (AMBIGUOUS_CAP) so that a kernel cannot hide in it.

An ulp count cannot do this: after `+ shift` cancels, one ulp of the float32 stage is many ulps of the output.

The margins (u = 2^-24, one float32 rounding):
  ln_modulate   delta = 16 u (|z| + |mean| rstd): the error of mean enters z as |mean error| * rstd, that of rstd as |z|; a CPU
                emulation of the kernel's summation order (emulate_ln below) stays within 3.8 u of that scale at D = 512, 1024
                and 3072, and 16 leaves a factor of four for the device's rsqrtf.
  qkv_post      delta = 16 u |z|, z = x rsqrt(mean(x^2) + eps): same argument without a mean.
  timestep_proj delta = 4 u absolute (|z| <= 1; relative ulps mean nothing next to the zeros of sin and cos), 4 u |z| for
                sin of an angle that needs no reduction (timestep_accept).
  softmax_rows  relative, see softmax_c.
"""
import math

import torch

BF = torch.bfloat16
U = 2.0 ** -24
# condition on the test inputs, not a measurement: share of elements for which the rule accepts more than one bit pattern
AMBIGUOUS_CAP = {"ln": 5e-3, "rms": 5e-3, "timestep": 5e-3, "softmax": 5e-3, "softmax_nv32": 2e-2}


# ---- rounding and the rule -------------------------------------------------------------------------------------------------------
def rn_bf16(v):
    """float64 -> the nearest bf16 (ties to even, bf16 subnormals included), returned as float64.  torch's own conversion goes
    through float32 and rounds twice."""
    v = v.double()
    _, e = torch.frexp(v)                       # |v| = m 2^e, m in [0.5, 1)
    q = torch.ldexp(torch.ones_like(v), (e - 1).clamp(min=-126) - 7)   # bf16 spacing at v
    return torch.round(v / q) * q               # both scalings exact; torch.round is half-to-even


def bf16_next(b):
    """the next bf16 above b (b: bf16-valued float64, normal range or 0)."""
    _, e = torch.frexp(b)
    q = torch.ldexp(torch.ones_like(b), (e - 1).clamp(min=-126) - 7)
    # at a negative power of two the spacing above (towards 0) is half that below
    m, _ = torch.frexp(b)
    q = torch.where(m == -0.5, q / 2, q)
    q = torch.where(b == 0, torch.full_like(q, 2.0 ** -133), q)
    return b + q


def candidates(z, delta):
    """(lo, hi, wide): the bf16 range [rn(z - delta), rn(z + delta)] as bf16 tensors, and where it holds more than two values."""
    lo, hi = rn_bf16(z - delta), rn_bf16(z + delta)
    wide = (hi != lo) & (hi != bf16_next(lo))
    return lo.to(BF), hi.to(BF), wide


def _bits(t):
    assert t.dtype == BF
    return t.contiguous().view(torch.int16)


def _line(t):
    """bf16 bits on a monotone integer line (for distances and interval tests)."""
    i = _bits(t).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


class Verdict:
    """What the rule says of one output tensor: n elements, of which `ambiguous` (share) had a choice, `equal_unambiguous`
    (share of the others that are bit-equal to their one accepted value), `misses` elements outside their accepted set, the
    worst of them `worst_ulp` bf16 ulps from the nearest accepted value."""

    def __init__(self, n, ambiguous, equal_unambiguous, misses, worst_ulp, first_miss):
        self.n, self.ambiguous, self.equal_unambiguous = n, ambiguous, equal_unambiguous
        self.misses, self.worst_ulp, self.first_miss = misses, worst_ulp, first_miss

    @property
    def ok(self):
        return self.misses == 0

    def line(self, name):
        return (f"[parity] {name}: n={self.n} ambiguous={self.ambiguous:.3e} bit-equal(unambiguous)={self.equal_unambiguous:.6f} "
                f"misses={self.misses} worst_miss={self.worst_ulp} bf16 ulp"
                + (f" first at {self.first_miss}" if self.misses else ""))


def judge(got, alts, wide=None, group=1, bounded=None):
    """Apply the rule.  got: bf16 tensor; alts: the tail's result for each candidate (combination), same shape -- for a range of
    more than two candidates (`wide`) alts[0] and alts[-1] are the ends.  group = 2: the last dimension is pairs that must match
    ONE alternative jointly (RoPE's two outputs come from one (re, im)).  bounded: elements held to a stated bound
    (alts[0] <= got <= alts[-1]) instead of candidates; they are checked like every other element and left out of the
    ambiguity statistics (must lie inside `wide`)."""
    got = got.cpu()
    g = _bits(got)
    n = g.numel()
    shape = g.shape[:-1] + (g.shape[-1] // group, group)
    ok = torch.zeros(shape[:-1], dtype=torch.bool)
    amb = torch.zeros(shape[:-1], dtype=torch.bool)
    a0 = _bits(alts[0])
    for a in alts:
        ab = _bits(a)
        ok |= (g == ab).view(shape).all(-1)
        amb |= (ab != a0).view(shape).any(-1)
    if bounded is not None:
        amb &= ~bounded
        n -= int(bounded.sum())
    if wide is not None and wide.any():
        assert group == 1
        lo, hi, x = _line(alts[0]), _line(alts[-1]), _line(got)
        ok |= wide & (x >= torch.minimum(lo, hi)) & (x <= torch.maximum(lo, hi)) & ~torch.isnan(got.float())
    dist = torch.stack([(_line(got) - _line(a)).abs() for a in alts]).amin(0)
    bad = ~ok
    bad_e = bad.unsqueeze(-1).expand(shape).reshape(g.shape) if group > 1 else bad
    misses = int(bad_e.sum())
    worst = int(dist[bad_e].max()) if misses else 0
    first = tuple(int(i) for i in bad_e.nonzero()[0]) if misses else None
    n_amb = int(amb.sum()) * group
    una = ~amb if bounded is None else ~amb & ~bounded
    eq = float((ok & una).sum()) / max(int(una.sum()), 1)
    return Verdict(n, n_amb / max(n, 1), eq, misses, worst, first)


def unambiguous_mask(alts, group=1):
    """element mask (shape of alts[0]): the rule accepts exactly one bit pattern."""
    a0 = _bits(alts[0])
    shape = a0.shape[:-1] + (a0.shape[-1] // group, group)
    amb = torch.zeros(shape[:-1], dtype=torch.bool)
    for a in alts:
        amb |= (_bits(a) != a0).view(shape).any(-1)
    return (~amb).unsqueeze(-1).expand(shape).reshape(a0.shape)


# ---- ln_modulate -----------------------------------------------------------------------------------------------------------------
def ln_rows_modulation(mod_a, mod_b, split, R):
    """per-row (shift, scale) [B, R, D] of fk_ln_modulate2_bf16: rows r < split of every batch use mod_a = (shift, scale) [B, D],
    the others mod_b."""
    first = (torch.arange(R) < split)[None, :, None]
    return (torch.where(first, mod_a[0][:, None], mod_b[0][:, None]), torch.where(first, mod_a[1][:, None], mod_b[1][:, None]))


def ln_tail(b, shift, scale):
    """bf16(bf16(b * bf16(1 + scale)) + shift): every operator on bf16 tensors is one float32 operation and one rounding."""
    return b * (1 + scale) + shift


def ln_stage(x, eps=1e-6):
    """(z, delta) of LayerNorm without affine over the last dimension, float64."""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
    z = (x - mean) * rstd
    return z, 16 * U * (z.abs() + mean.abs() * rstd)


def ln_accept(x, shift, scale, eps=1e-6, tail=ln_tail):
    """alternatives and wide mask for judge(): x [B, R, D] bf16, shift / scale broadcastable to it."""
    lo, hi, wide = candidates(*ln_stage(x, eps))
    return [tail(lo, shift, scale), tail(hi, shift, scale)], wide


def emulate_ln(x, eps=1e-6, rounded=True):
    """The kernel's float32 arithmetic on the CPU, in its order: lane l of 64 holds columns 512 i + 8 l .. + 7; it adds its
    elements pair by pair, the wave adds the lanes in an xor butterfly (32 .. 1), mean = sum * fl(1 / D); the same for the
    squared deviations; rstd is the correctly rounded 1 / sqrt (the device's rsqrtf is within an ulp of it).  Returns the
    float32 stage rounded to bf16 (rounded = False: as float32)."""
    D = x.shape[-1]
    NV = D // 512
    v = x.float().reshape(-1, NV, 64, 8)
    s = torch.zeros(v.shape[0], 64)
    for i in range(NV):
        for e in range(4):
            s = s + (v[:, i, :, 2 * e] + v[:, i, :, 2 * e + 1])
    mean = _butterfly(s)[:, :1] * torch.tensor(1.0 / D, dtype=torch.float32)
    q = torch.zeros_like(s)
    for i in range(NV):
        for e in range(8):
            d = v[:, i, :, e] - mean
            q = q + d * d
    var = _butterfly(q)[:, :1] * torch.tensor(1.0 / D, dtype=torch.float32) + torch.tensor(eps, dtype=torch.float32)
    rstd = (1.0 / torch.sqrt(var.double())).float()
    y = ((v - mean[:, None, None]) * rstd[:, None, None]).reshape(x.shape)
    return y.to(BF) if rounded else y


def _butterfly(s):
    n = s.shape[1]
    off = n // 2
    idx = torch.arange(n)
    while off >= 1:
        s = s + s[:, idx ^ off]
        off //= 2
    return s


# ---- qkv_post --------------------------------------------------------------------------------------------------------------------
def rope(re, im, c0, s0, c1, s1):
    """the uncontracted float32 rotation of one pair: two rounded products and one sum per output, then bf16."""
    re, im = re.float(), im.float()
    return (re * c0 + (-im) * s0).to(BF), (im * c1 + re * s1).to(BF)


def rope_contracted(which):
    """what an fma makes of it: product `which` (0 = first, 1 = second) stays exact (float64 holds a bf16 x float32 product
    exactly), the other is rounded to float32, the sum is rounded once."""
    def f(re, im, c0, s0, c1, s1):
        def one(a, ca, b, cb):
            pa, pb = a.double() * ca.double(), b.double() * cb.double()
            if which == 0:
                return (pa + (b.float() * cb).double()).float().to(BF)
            return ((a.float() * ca).double() + pb).float().to(BF)
        return one(re, c0, -im, s0), one(im, c1, re, s1)
    return f


def rms_stage(x, eps=1e-6):
    x = x.double()
    z = x / torch.sqrt((x * x).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
    return z, 16 * U * z.abs()


def emulate_rms(x, eps=1e-6):
    """qkv_post_kernel's float32 RMSNorm on the CPU: 16 lanes x 8 elements per head row, per lane four steps
    ss += x0 x0 + x1 x1, an xor butterfly (8 .. 1), rs = rsqrt(ss * fl(1 / 128) + eps) correctly rounded; bf16(x * rs)."""
    v = x.float().reshape(-1, 16, 8)
    s = torch.zeros(v.shape[0], 16)
    for e in range(4):
        s = s + (v[:, :, 2 * e] * v[:, :, 2 * e] + v[:, :, 2 * e + 1] * v[:, :, 2 * e + 1])
    arg = _butterfly(s)[:, :1] * torch.tensor(1.0 / 128, dtype=torch.float32) + torch.tensor(eps, dtype=torch.float32)
    rs = (1.0 / torch.sqrt(arg.double())).float()
    return (v * rs[:, None]).reshape(x.shape).to(BF)


def qkv_accept(qkv, which, w_img, w_txt, cos, sin, s_txt, rope_fn=rope, eps=1e-6):
    """The four alternatives (candidate combinations of a pair's (re, im)) of q (which = 0) or k (1), each [B, H, S, 128] bf16:
    qkv [B, S, 3 H 128] bf16, norm weights [128] bf16 (w_txt for tokens s < s_txt; None when s_txt == 0), cos / sin fp32 [S, 128]."""
    lo, hi, wide = candidates(*rms_stage(qkv_heads(qkv, which), eps))
    assert not wide.any()
    return [qkv_tail(re, im, w_img, w_txt, cos, sin, s_txt, rope_fn)
            for re in (lo[..., 0::2], hi[..., 0::2]) for im in (lo[..., 1::2], hi[..., 1::2])]


def qkv_heads(qkv, which):
    """q (which = 0) or k (1) of qkv [B, S, 3 H 128] as [B, H, S, 128]."""
    B, S, D3 = qkv.shape
    H = D3 // 384
    return qkv[..., which * H * 128:(which + 1) * H * 128].reshape(B, S, H, 128).transpose(1, 2)


def qkv_tail(re, im, w_img, w_txt, cos, sin, s_txt, rope_fn=rope):
    """bf16(b * w) on the two halves of every pair ([B, H, S, 64] each), the rotation, and the pairs interleaved again."""
    S = cos.shape[0]
    w = w_img.expand(S, 128) if s_txt == 0 else torch.where((torch.arange(S) < s_txt)[:, None], w_txt[None], w_img[None])
    o0, o1 = rope_fn(re * w[:, 0::2], im * w[:, 1::2], cos[:, 0::2], sin[:, 0::2], cos[:, 1::2], sin[:, 1::2])
    return torch.stack([o0, o1], dim=-1).flatten(-2)


def qkv_emulated(qkv, which, w_img, w_txt, cos, sin, s_txt, rope_fn=rope):
    """emulate_rms through the tail: what a kernel with the emulation's float32 stage and `rope_fn` writes."""
    b = emulate_rms(qkv_heads(qkv, which))
    return qkv_tail(b[..., 0::2], b[..., 1::2], w_img, w_txt, cos, sin, s_txt, rope_fn)


# ---- softmax_rows ----------------------------------------------------------------------------------------------------------------
def softmax_nv(n):
    """the kernel instantiation (float4 loads per thread) fk_softmax_rows picks for n columns."""
    return 1 if n <= 1024 else 4 if n <= 4096 else 16 if n <= 16384 else 32


def softmax_c(nv):
    """Relative margin of softmax_rows_kernel<NV> in units of u = 2^-24 (one float32 rounding is at most u relative), from
    the kernel's own operations on p_j = e_j * (1 / sum_k e_k), e_k = expf(x_k - max):
      * expf: documented to 1 ulp = 2 u, once for the numerator e_j and once as the (weighted mean) error of the terms of
        the sum                                                                                                     -> 2 + 2
      * the sum: all terms are positive, so each addition a term passes through costs u of the total: the lane's chain of
        4 NV additions, 6 butterfly steps in the wave, 2 steps across the four waves                                -> 4 NV + 8
      * the reciprocal (correctly rounded division) and the product                                                 -> 1 + 1
      * second-order terms of (1 + u)^k, k < 150                                                                    -> 1
    c = 4 NV + 15: 19, 31, 79, 143 for NV = 1, 4, 16, 32.
    Not in that count, because it depends on the data: the subtraction d = x - max is rounded (half an ulp of d <= u |d|), and
    exp turns an absolute error of its argument into a relative one of its value.  softmax_stage adds u |d_j| for the numerator
    and u sum_k |d_k| e_k / sum_k e_k (the same error averaged over the sum's terms) for the denominator."""
    return 4 * nv + 15


def softmax_stage(x):
    """(z, delta) of a row softmax of float32 scores, float64."""
    nv = softmax_nv(x.shape[-1])
    d = x.double() - x.double().amax(-1, keepdim=True)
    e = torch.exp(d)
    tot = e.sum(-1, keepdim=True)
    z = e / tot
    rel = softmax_c(nv) + d.abs() + (d.abs() * e).sum(-1, keepdim=True) / tot
    return z, rel * U * z


def softmax_accept(x):
    """alternatives, wide mask and the mask of elements below the float32 normal range (there |got| <= 2^-126 is accepted)."""
    z, delta = softmax_stage(x)
    tiny = z < 2.0 ** -126
    lo, hi, wide = candidates(torch.where(tiny, torch.zeros_like(z), z), torch.where(tiny, torch.zeros_like(z), delta))
    lo = torch.where(tiny, torch.tensor(-2.0 ** -126, dtype=BF), lo)
    hi = torch.where(tiny, torch.tensor(2.0 ** -126, dtype=BF), hi)
    return [lo, hi], wide | tiny, tiny


def emulate_softmax(x, missing_wave=False):
    """softmax_rows_kernel<NV> in float32 on the CPU: thread t of 256 holds columns 4 (256 i + t) .. + 3, i < NV (beyond n:
    exp = 0); it adds its 4 NV exponentials in order, the wave adds its lanes in an xor butterfly, the four wave sums add as
    (w0 + w1) + (w2 + w3); p = e * (1 / sum).  expf as the correctly rounded exponential.  missing_wave: the planted error of a
    sum that forgets wave 3."""
    rows, n = x.shape
    nv = softmax_nv(n)
    xp = torch.full((rows, nv * 1024), -3.0e38)
    xp[:, :n] = x
    d = xp - xp.amax(-1, keepdim=True)
    e = torch.exp(d.double()).float().reshape(rows, nv, 256, 4)
    s = torch.zeros(rows, 256)
    for i in range(nv):
        for k in range(4):
            s = s + e[:, i, :, k]
    w = torch.stack([_butterfly(s[:, 64 * j:64 * j + 64])[:, 0] for j in range(4)], dim=1)
    tot = (w[:, 0] + w[:, 1]) + (w[:, 2] if missing_wave else (w[:, 2] + w[:, 3]))
    inv = (1.0 / tot)[:, None, None, None]
    return (e * inv).reshape(rows, -1)[:, :n].to(BF)


# ---- timestep_proj ---------------------------------------------------------------------------------------------------------------
def timestep_freqs():
    return torch.exp(-math.log(10000.0) * torch.arange(128, dtype=torch.float32) / 128)


def timestep_accept(v, freqs, swap=False):
    """v: bf16 or fp32 [B].  The angle fl(bf16(bf16(v) * 1000) * freqs[k]) is exact float32 arithmetic (the bf16 product is
    exact in float32 before its rounding); z = cos | sin of it in float64.  delta = 4 u absolute (|z| <= 1; relative ulps mean
    nothing next to the zeros that an argument reduction has to find) -- except for sin at |angle| <= pi / 4, where it is 4 u |z|:
    no implementation reduces such an argument (it IS the reduced argument, exactly), so its error is that of a polynomial
    times the angle, relative to the result; sinf is documented to 1 ulp = 2 u |z|, and 4 keeps the factor of two that the
    absolute margin has at |z| ~ 1.  Under the absolute margin these elements (sin ~ angle down to 1e-4, a tenth of the table
    for the small timesteps) would each have two or three candidates, 0.75 % of all, and sin(0) could be anything up to 2.4e-7.
    swap: the planted error (sin first)."""
    t = v.to(BF) * 1000                                   # bf16 tensor times a scalar: one product, one rounding
    ang = (t.float()[:, None] * freqs[None, :]).double()
    d_cos = torch.full_like(ang, 4 * U)
    d_sin = torch.where(ang.abs() <= math.pi / 4, 4 * U * torch.sin(ang).abs(), d_cos)
    z = torch.cat([torch.sin(ang), torch.cos(ang)] if swap else [torch.cos(ang), torch.sin(ang)], dim=-1)
    lo, hi, wide = candidates(z, torch.cat([d_sin, d_cos] if swap else [d_cos, d_sin], dim=-1))
    return [lo, hi], wide


# ---- exact restatements ----------------------------------------------------------------------------------------------------------
def add3(a, b, c):
    return (a + b) + c


def true_cfg(pos, neg, scale):
    """bf16(neg + bf16(scale * bf16(pos - neg))) with the scale a float32 number."""
    d = pos - neg
    return neg + (torch.tensor(scale, dtype=torch.float32) * d.float()).to(BF)


# ---- the inputs of tests/test_hip_forward_exact.py (and of the CPU test that holds them to the caps) -----------------------------
LN_DS = (512, 1024, 3072)
LN_BR = ((2, 37), (3, 5))
LN_S_TXT = 3                      # x is rows [S_TXT:] of a [B, S_TXT + R, D] buffer
QKV_CASES = ((2, 3, 21, 6, 9), (1, 2, 0, 8, 8), (1, 2, 64, 0, 0), (1, 24, 70, 32, 33))   # B, H, S_txt, image grid h x w
QKV_LARGE = QKV_CASES[3]
SOFTMAX_NS = (4, 64, 1000, 1024, 1028, 4096, 4100, 16384, 16388, 32768)


def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale)


def ln_inputs(D, B, R):
    """(buffer [B, S_TXT + R, D] bf16, mod [B, 6 D] bf16).  Rows of the x view, in batch 0: 1 = constant (variance 0,
    rstd = 1 / sqrt(eps): the float32 stage is 0 up to the error of the mean times 1000, and the output is shift wherever
    shift is not tiny), 3 = magnitude 1e4, R - 1 of the last batch = mean 30 and spread 0.5 where R > 5; the rest ordinary.
    The margin of the mean-30 row is 60 times an ordinary row's (|mean| rstd = 60) and 4 % of its elements are ambiguous: among
    the 15 rows of the (3, 5) case it alone would exceed the cap at D = 3072, so that case goes without it."""
    buf = (_randn(B, LN_S_TXT + R, D, seed=100 + D + R, scale=2.0) + 0.5).to(BF)
    x = buf[:, LN_S_TXT:]
    x[0, 1] = 2.0 ** -9
    x[0, 3] = _randn(D, seed=102, scale=1e4).to(BF)
    if R > 5:
        x[B - 1, R - 1] = (30 + _randn(D, seed=101, scale=0.5)).to(BF)
    mod = _randn(B, 6 * D, seed=103 + D, scale=0.3).to(BF)
    return buf, mod


def ln_forms(R):
    """None = fk_ln_modulate_bf16, a number = the split of fk_ln_modulate2_bf16 (21 > R: every row is a first-stream row)."""
    return (None, 0, 1, 21, R)


def ln_modulation(mod, D, split, R):
    """per-row (shift, scale) of a form: chunks 0, 1 of mod [B, 6 D] for the first stream, chunks 3, 4 for the second."""
    a, b = (mod[:, :D], mod[:, D:2 * D]), (mod[:, 3 * D:4 * D], mod[:, 4 * D:5 * D])
    return ln_rows_modulation(a, a if split is None else b, R if split is None else split, R)


def qkv_inputs(B, H, s_txt, hh, ww):
    """qkv [B, S, 3 H 128], the four norm weights (q_img, k_img, q_txt, k_txt), cos, sin [S, 128] fp32."""
    from oracle import mmdit
    from oracle.helpers import prepare_latent_image_ids
    S = s_txt + hh * ww
    qkv = _randn(B, S, 3 * H * 128, seed=200 + S).to(BF)
    w = [(1 + _randn(128, seed=210 + i, scale=0.1)).to(BF) for i in range(4)]
    ids = torch.cat([torch.zeros(s_txt, 3), prepare_latent_image_ids(hh, ww)]) if hh * ww else torch.zeros(s_txt, 3)
    if hh * ww == 0:          # text only: give the rows distinct positions so that the rotation is not the identity
        ids[:, 1] = torch.arange(s_txt)
        ids[:, 2] = torch.arange(s_txt) % 7
    cos, sin = mmdit.rope_tables(ids)
    return qkv, w, cos.contiguous(), sin.contiguous()


def softmax_inputs(n):
    """3 rows of fp32 scores: 4 randn; the same with one logit 80 above the rest; all equal."""
    x = _randn(3, n, seed=300 + n, scale=4.0)
    x[1, (7 * n) // 11] = x[1].max() + 80.0
    x[2] = 1.25
    return x


def timestep_inputs():
    """(bf16 values: 0 and every bf16 in [2^-10, 1]; fp32 values: the same plus 1.0, 3.5, 7.0, 10.0)."""
    bits = torch.arange(0x3A80, 0x3F80 + 1, dtype=torch.int32).to(torch.int16)
    v = torch.cat([torch.zeros(1, dtype=BF), bits.view(BF)])
    return v, torch.cat([v.float(), torch.tensor([1.0, 3.5, 7.0, 10.0])])
