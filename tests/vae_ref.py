"""Host references for the VAE kernel tests (plain module: tests/test_vae_ref.py checks them on the CPU,
tests/test_hip_vae_exact.py holds the HIP kernels to them).

GroupNorm statistics -- the bound
---------------------------------
csrc/vae_kernels.hip sums one (batch, group) in three stages:

  thread   fp32, sequential over its pixels (stride ppi = 256 / (C/8)) of the block's `per_blk = ceil(HW / nblk)` pixels,
           four channels per step: s += (v0 + v1) + (v2 + v3), and the same with squares.  n_t = ceil(per_blk / ppi) * 4
           values enter one accumulator; a value passes at most 2 + ceil(per_blk / ppi) <= n_t fp32 additions (and, for fp32
           inputs, one rounding of its square: bf16 squares are exact in fp32).
  block    fp32, thread g adds the n_m = ppi * (C/32/4) = 16 half-chunk sums of group g one after the other.
  finalize fp64 over the nblk block sums, mean and E[x^2] - mean^2 in fp64.

With u = 2^-24, the standard first-order bound of recursive summation over the two fp32 stages is

    |S - sum x|    <= gamma * sum |x|,     |Q - sum x^2| <= gamma * sum x^2,     gamma = (n_t + n_m) * u

(the fp64 stage adds ~nblk * 2^-53, nothing that matters).  Dividing by the count N:

    d(mean) <= gamma * sum|x| / N
    d(var)  <= gamma * E[x^2] + 2 |mean| d(mean)                 (var = E[x^2] - mean^2, first order)
    d(rstd) / rstd <= 1/2 * d(var) / (var + eps)                 (rstd = (var + eps)^-1/2, first order)

and the rstd bound is taken twice for the first-order steps.  Nothing in it comes from a kernel.  The bound grows with
(mean / std)^2: that is the cancellation in E[x^2] - mean^2, and the ill-conditioned data (|mean| / std up to 32) shows how
much of it the kernel actually uses.

Attention with head dimension 512 -- the rounding model
-------------------------------------------------------
`hd512_ref_and_model`: O = softmax(Q K^T c) V in fp64, and the same sums with the two rounding points the header of
csrc/vae_attention.hip names: the un-normalised p = exp2(s - max) rounded to bf16 before P V (the row sum uses the unrounded p)
and one bf16 rounding of O / l.  attention_ref.assert_rows_close derives the row bound from the model's own error.
"""
import functools
import math

import numpy as np
import torch

BF = torch.bfloat16
F64 = torch.float64
U32 = 2.0 ** -24
GN_THREADS, GN_MAX_BLOCKS, GROUPS, GN_EPS = 256, 512, 32, 1e-6
EW_ONE_TRIP = 8192 * 256          # work items the elementwise grid covers in its first trip

GN_CASES = [(128, 128 * 65 + 3), (512, 4100), (128, 65536 + 777), (256, 40000), (128, 5), (1024, 300)]
GN_CAPPED = [(128, 65536 + 777), (256, 40000)]


# ---- GroupNorm statistics ------------------------------------------------------------------------------------------------
def gn_layout(C, HW):
    """The launch geometry of the statistics kernels: nblk, per_blk, ppi, iterations per thread, n_t, n_m."""
    cpr = C // 8
    ppi = GN_THREADS // cpr
    nblk = min(max((HW + ppi * 8 - 1) // (ppi * 8), 1), GN_MAX_BLOCKS)
    per_blk = (HW + nblk - 1) // nblk
    iters = (per_blk + ppi - 1) // ppi
    return dict(nblk=nblk, per_blk=per_blk, ppi=ppi, iters=iters, n_t=iters * 4, n_m=ppi * (C // GROUPS // 4))


@functools.lru_cache(maxsize=None)
def gn_data(C, HW, kind):
    """fp32 [2, HW, C], the two batch entries drawn from different streams.
    'well': N(0, 1.5^2) plus a per-channel offset in [-2, 2].  'ill': per group a mean from +-{4, 8, 16}, std 0.5."""
    out = []
    for b in range(2):
        g = torch.Generator().manual_seed(1000 * b + C + HW % 997 + (7 if kind == "ill" else 0))
        if kind == "well":
            x = torch.randn(HW, C, generator=g) * 1.5 + torch.linspace(-2, 2, C)[None, :] * (1.0 if b == 0 else -0.7)
        else:
            mag = torch.tensor([4.0, 8.0, 16.0])[torch.randint(0, 3, (GROUPS,), generator=g)]
            sign = torch.randint(0, 2, (GROUPS,), generator=g).float() * 2 - 1
            x = torch.randn(HW, C, generator=g) * 0.5 + (mag * sign).repeat_interleave(C // GROUPS)[None, :]
        out.append(x)
    return torch.stack(out)


def gn_stats64(x):
    """x [B, HW, C] (any float dtype; its values are the truth) -> dict of fp64 [B, 32]: mean, var, rstd, and the bound's
    ingredients mean|x| and E[x^2]."""
    B, HW, C = x.shape
    xg = x.to(F64).reshape(B, HW, GROUPS, C // GROUPS)
    mean = xg.mean(dim=(1, 3))
    ex2 = (xg * xg).mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + GN_EPS), mabs=xg.abs().mean(dim=(1, 3)), ex2=ex2)


def gn_bound(ref, C, HW):
    """(bound on |mean - mean64|, bound on |rstd - rstd64|), fp64 [B, 32]: the module docstring's derivation."""
    lay = gn_layout(C, HW)
    gamma = (lay["n_t"] + lay["n_m"]) * U32
    d_mean = gamma * ref["mabs"]
    d_var = gamma * ref["ex2"] + 2.0 * ref["mean"].abs() * d_mean
    d_rstd = 2.0 * ref["rstd"] * 0.5 * d_var / (ref["var"] + GN_EPS)
    return d_mean, d_rstd


def gn_emulate(x):
    """The kernels' summation order in numpy: fp32 per-thread strided sums, fp32 fixed-order in-block merge, fp64 finalize
    (lane i adds blocks i, i + 64, ...; then the halving tree).  x [B, HW, C] -> fp32 [B, 32, 2] (mean, rstd)."""
    B, HW, C = x.shape
    lay = gn_layout(C, HW)
    nblk, per_blk, ppi, iters = lay["nblk"], lay["per_blk"], lay["ppi"], lay["iters"]
    hpg = C // GROUPS // 4
    out = np.zeros((B, GROUPS, 2), np.float32)
    for b in range(B):
        # a pixel beyond its block's range adds (0 + 0) + (0 + 0) = +0 to the accumulator: exact, so padding changes nothing
        xp = np.zeros((nblk, iters * ppi, C), np.float32)
        xb = x[b].to(torch.float32).numpy()
        for blk in range(nblk):
            p0 = blk * per_blk
            p1 = min(p0 + per_blk, HW)
            if p1 > p0:
                xp[blk, :p1 - p0] = xb[p0:p1]
        v = xp.reshape(nblk, iters, ppi, C // 4, 4)          # pixel p0 + prow + k ppi: k outer, prow inner
        s = np.zeros((nblk, ppi, C // 4), np.float32)
        q = np.zeros_like(s)
        for k in range(iters):
            w = v[:, k]
            s = s + ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3]))
            w2 = w * w
            q = q + ((w2[..., 0] + w2[..., 1]) + (w2[..., 2] + w2[..., 3]))
        # thread g: pixel rows outer, the group's half-chunks inner
        sg = s.reshape(nblk, ppi, GROUPS, hpg).transpose(0, 2, 1, 3).reshape(nblk, GROUPS, ppi * hpg)
        qg = q.reshape(nblk, ppi, GROUPS, hpg).transpose(0, 2, 1, 3).reshape(nblk, GROUPS, ppi * hpg)
        bs = np.zeros((nblk, GROUPS), np.float32)
        bq = np.zeros_like(bs)
        for j in range(ppi * hpg):
            bs = bs + sg[:, :, j]
            bq = bq + qg[:, :, j]
        n64 = (nblk + 63) // 64
        ls = np.zeros((64, GROUPS), np.float64)
        lq = np.zeros_like(ls)
        pad_s = np.zeros((n64 * 64, GROUPS), np.float64)
        pad_q = np.zeros_like(pad_s)
        pad_s[:nblk], pad_q[:nblk] = bs, bq
        for j in range(n64):
            ls = ls + pad_s[j * 64:(j + 1) * 64]
            lq = lq + pad_q[j * 64:(j + 1) * 64]
        off = 32
        while off >= 1:
            ls[:off] = ls[:off] + ls[off:2 * off]
            lq[:off] = lq[:off] + lq[off:2 * off]
            off //= 2
        count = float(HW * (C // GROUPS))
        mean = ls[0] / count
        var = np.maximum(lq[0] / count - mean * mean, 0.0)
        out[b, :, 0] = mean.astype(np.float32)
        out[b, :, 1] = (1.0 / np.sqrt(var + np.float64(np.float32(GN_EPS)))).astype(np.float32)
    return torch.from_numpy(out)


def gn_check_stats(name, stats, x, C, HW):
    """stats fp32 [B, 32, 2] against fp64 on x within `gn_bound`; prints and returns the largest observed / bound ratios."""
    ref = gn_stats64(x)
    b_mean, b_rstd = gn_bound(ref, C, HW)
    st = stats.to(F64).cpu()
    assert torch.isfinite(st).all(), f"{name}: non-finite statistics"
    r_mean = ((st[..., 0] - ref["mean"]).abs() / b_mean).max().item()
    r_rstd = ((st[..., 1] - ref["rstd"]).abs() / b_rstd).max().item()
    cond = (ref["mean"].abs() / ref["var"].sqrt()).max().item()
    lay = gn_layout(C, HW)
    print(f"[parity] {name}: C={C} HW={HW} nblk={lay['nblk']} n_t={lay['n_t']} n_m={lay['n_m']} max|mean|/std={cond:.1f} "
          f"observed/bound mean={r_mean:.4f} rstd={r_rstd:.4f} (rstd bound rel max {(b_rstd / ref['rstd']).max().item():.2e})",
          flush=True)
    assert r_mean <= 1.0, f"{name}: mean is {r_mean:.3f} x the derived bound"
    assert r_rstd <= 1.0, f"{name}: rstd is {r_rstd:.3f} x the derived bound"
    return r_mean, r_rstd


# ---- GroupNorm apply -----------------------------------------------------------------------------------------------------
def gn_apply64(x, stats, gamma, beta):
    """t = (x - mean) rstd gamma + beta in fp64 from the given statistics ([B, 32, 2]); x [B, HW, C]."""
    B, HW, C = x.shape
    mean = stats[..., 0].to(F64).repeat_interleave(C // GROUPS, dim=1)[:, None, :]
    rstd = stats[..., 1].to(F64).repeat_interleave(C // GROUPS, dim=1)[:, None, :]
    return (x.to(F64) - mean) * rstd * gamma.to(F64) + beta.to(F64)


def bf16_ulps(a, b):
    """Distance in bf16 ulps between two bf16 tensors (monotonic integer line)."""
    ai = a.contiguous().view(torch.int16).to(torch.int32)
    bi = b.contiguous().view(torch.int16).to(torch.int32)
    ai = torch.where(ai < 0, -(ai & 0x7FFF), ai)
    bi = torch.where(bi < 0, -(bi & 0x7FFF), bi)
    return (ai - bi).abs()


def gn_check_apply(name, got, t64, silu):
    """Every element of the bf16 result.  Without SiLU: within one bf16 ulp of bf16(t64) (fp32 evaluation errs far below half an
    ulp, so only the two neighbours of the correctly rounded value are reachable).  With SiLU, y = silu(bf16(t)):
    |got - y64| <= 2^-8 (|y64| + 1.1 |t64|): one flip of the inner rounding (2^-8 |t|) through |silu'| <= 1.1, plus the outer
    rounding (2^-9 |y|), doubled for the fp32 evaluation and exp."""
    got = got.cpu()
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite values"
    if not silu:
        ulp = bf16_ulps(got, t64.to(BF))
        worst = int(ulp.max())
        print(f"[parity] {name}: max ulp {worst}, share off by one {(ulp == 1).float().mean().item():.2e}", flush=True)
        assert worst <= 1, f"{name}: {int((ulp > 1).sum())} elements beyond 1 ulp (max {worst})"
        return float(worst)
    tb = t64.to(BF).to(F64)
    y64 = tb / (1.0 + torch.exp(-tb))
    ratio = ((got.to(F64) - y64).abs() / (2.0 ** -8 * (y64.abs() + 1.1 * t64.abs())).clamp(min=1e-300)).max().item()
    print(f"[parity] {name}: silu observed/bound max {ratio:.4f}", flush=True)
    assert ratio <= 1.0, f"{name}: an element is {ratio:.3f} x its bound"
    return ratio


# ---- attention, head dimension 512 -----------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634


def hd512_inputs(B, S, seed, matched=True):
    """q, k, v bf16 [B, S, 512] ~ N(0, 1); for a third of the queries k[pi(i)] += 0.9 q[i], pi a permutation of the whole
    sequence (attention_ref.make_inputs at one head of 512): the dominant key lands in any tile and any slot."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, S, 512, generator=g) for _ in range(3))
    if matched:
        for b in range(B):
            pi = torch.randperm(S, generator=g)
            src = torch.arange(0, S, 3)
            k[b, pi[src]] += 0.9 * q[b, src]
    return q.to(BF), k.to(BF), v.to(BF)


def hd512_ref_and_model(q, k, v, scale, rows=None, chunk=512):
    """(ref, model) fp64 [B, 1, R, 512] for query rows `rows` (index tensor; default all): see the module docstring."""
    B, S, _ = q.shape
    rows = torch.arange(S) if rows is None else rows
    ref = torch.zeros(B, 1, len(rows), 512, dtype=F64)
    mod = torch.zeros_like(ref)
    for b in range(B):
        K, V = k[b].to(F64), v[b].to(F64)
        for r0 in range(0, len(rows), chunk):
            idx = rows[r0:r0 + chunk]
            s2 = (q[b, idx].to(F64) @ K.t()) * (scale * LOG2E)
            P = torch.exp2(s2 - s2.max(dim=1, keepdim=True).values)
            l = P.sum(dim=1, keepdim=True)
            ref[b, 0, r0:r0 + len(idx)] = (P @ V) / l
            mod[b, 0, r0:r0 + len(idx)] = ((P.to(BF).to(F64) @ V) / l).to(BF).to(F64)
    return ref, mod


# ---- convolutions ----------------------------------------------------------------------------------------------------------
def conv_ref_and_cap(x, w, bias, mode, res=None):
    """x [B, Cin, H, W], w [Cout, Cin, k, k], bias: bf16-valued tensors.  Returns (ref64, cap) for the bf16 result of a
    convolution kernel that accumulates in fp32 and rounds once:

        |got - ref64| <= 2^-8 |ref64| + 2^-8 A K_eps,   A = conv(|x|, |w|) + |bias|,   K_eps = 9 Cin 2^-24

    and with a residual (got = bf16(res + bf16(y))) the second rounding's 2^-8 |res + y| on top; ref64 then includes res."""
    import torch.nn.functional as F
    xd, wd, bd = x.to(F64), w.to(F64), bias.to(F64)

    def conv(a, ww, bb):
        if mode == "up":
            return F.conv2d(F.interpolate(a, scale_factor=2.0, mode="nearest"), ww, bb, padding=1)
        if mode == "s2":
            return F.conv2d(F.pad(a, (0, 1, 0, 1)), ww, bb, stride=2)
        if mode == "1x1":
            return F.conv2d(a, ww, bb)
        return F.conv2d(a, ww, bb, padding=1)
    y = conv(xd, wd, bd)
    k_eps = 9 * x.shape[1] * U32
    cap = 2.0 ** -8 * y.abs() + 2.0 ** -8 * conv(xd.abs(), wd.abs(), bd.abs()) * k_eps
    if res is not None:
        y = y + res.to(F64)
        cap = cap + 2.0 ** -8 * y.abs()
    return y, cap


def check_cap(name, got, ref64, cap):
    ratio = ((got.to(F64).cpu() - ref64).abs() / cap.clamp(min=1e-300)).max().item()
    print(f"[parity] {name}: per-element observed/cap max {ratio:.4f}", flush=True)
    assert math.isfinite(ratio) and ratio <= 1.0, f"{name}: an element is {ratio:.3f} x its cap"
    return ratio
