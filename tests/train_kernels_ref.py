"""Reference, fp32 emulation and error bounds of the training-step kernels (csrc/train_kernels.hip): the AdamW update, the
noisy-token mix and the flow-matching loss with its gradient.  Host only (numpy / torch float64), modelled on prodigy_ref.py.

``adamw_ref``: one AdamW step in float64 with the scalars the kernel receives (``adamw_scalars``: lr, betas, eps and weight decay
rounded to fp32 first; step_size, bc2_sqrt and decay formed in double and rounded to fp32, as ``fk_adamw_step_scaled`` does on the
host).  ``adamw_emu``: the same step in float32, every operation rounded on its own, in ``adamw_kernel``'s order -- and, on
request, with one of four deliberate mistakes.  ``adamw_bounds``: what separates the two, derived from that operation order alone
(u = 2^-24 per fp32 rounding, every operation of the kernel correctly rounded; an fma contraction only removes roundings) and
never from a kernel's output.

``flow_ref``: noisy tokens, loss and gradient in float64, the packed <-> latent map written with reshape / permute as
``_pack_latents`` does (not the kernel's div / mod chain).  ``flow_bounds``: the same kind of bound for ``flow_loss_kernel``.
``bf16_interval``: the bf16 values a correctly rounded result may take when its fp32 predecessor is within a bound of the fp64 value.
"""
import math

import numpy as np
import torch

from prodigy_ref import MARGIN, TINY, U, U64, clip_coef, f32  # noqa: F401  (re-exported: the tests take them from here)

ADAMW_MISTAKES = ("decay_after_update", "bc2_sqrt_multiplied", "eps_inside_sqrt", "coef_not_applied_to_bf16")
SLACK = 1.0 + 8 * U        # second-order terms of a first-order bound with at most 8 roundings in a chain
MIN_NORMAL = 2.0 ** -126

# launch geometry of train_kernels.hip: grid_for caps every launch at GRID_CAP blocks of THREADS threads, one element per thread and trip
THREADS = 256
GRID_CAP = 2048
WAVE = 64


def blocks_for(n):
    return max(1, min((n + THREADS - 1) // THREADS, GRID_CAP))


def sum_depth(n):
    """Longest chain of double additions between one term and the result of the two-stage reduction over ``n`` terms:
    a thread's trips of the grid-stride loop, log2(64) = 6 shuffle levels, the 4 wave sums; then ``finish_sum_kernel``:
    ceil(blocks / 256) partials per thread, 6 shuffle levels, 4 wave sums."""
    blocks = blocks_for(n)
    trips = (n + blocks * THREADS - 1) // (blocks * THREADS)
    return trips + 6 + THREADS // WAVE + (blocks + THREADS - 1) // THREADS + 6 + THREADS // WAVE


# ---- AdamW -------------------------------------------------------------------------------------------------------------------
def adamw_scalars(step, lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2, round32=True):
    """The scalars of one launch.  Hyper-parameters cross the C ABI as ``float``; ``fk_adamw_step_scaled`` forms the bias corrections
    with double pow, then step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t) and decay = 1 - lr * wd in double, each rounded
    to fp32 once; the kernel forms 1 - beta in fp32 (exact for beta in [0.5, 1]).  ``round32=False`` keeps the derived scalars in
    double: torch.optim.AdamW's own arithmetic on the same hyper-parameters, for the check of the algebra against it."""
    lr, b1, b2, eps, wd = (f32(x) for x in (lr, betas[0], betas[1], eps, weight_decay))
    r = f32 if round32 else float
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    return dict(b1=b1, b2=b2, omb1=r(1.0 - b1), omb2=r(1.0 - b2), eps=eps, step_size=r(lr / bc1), bc2_sqrt=r(math.sqrt(bc2)),
                decay=r(1.0 - lr * wd))


def adamw_ref(p, g, m, v, sc, coef=1.0):
    """float64.  ``g``: the stored gradient; ``coef``: the clipping / grad_scale coefficient (``clip_coef``).  Returns (p, m, v)."""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    g = g * coef
    m1 = m + sc["omb1"] * (g - m)
    v1 = v * sc["b2"] + sc["omb2"] * g * g
    denom = np.sqrt(v1) / sc["bc2_sqrt"] + sc["eps"]
    return p * sc["decay"] - sc["step_size"] * (m1 / denom), m1, v1


def adamw_emu(p, g, m, v, sc, coef=1.0, g_is_bf16=False, mistake=None, trace=None):
    """``adamw_kernel`` in float32, one rounding per operation: g = graw * coef; p1 = p * decay; m = m + (1 - b1) * (g - m) (lerp);
    v = v * b2 + ((1 - b2) * g) * g; denom = sqrt(v) / bc2_sqrt + eps; p = p1 + (-step_size) * (m / denom).
    ``trace``: a list that receives every intermediate (for the no-subnormal premise of the bit-equality check)."""
    F = np.float32
    p, g, m, v = (np.asarray(t, dtype=F) for t in (p, g, m, v))
    b2, omb1, omb2, eps, ss, bc, decay = (F(sc[k]) for k in ("b2", "omb1", "omb2", "eps", "step_size", "bc2_sqrt", "decay"))
    if not (mistake == "coef_not_applied_to_bf16" and g_is_bf16):
        g = g * F(coef)
    p1 = p if mistake == "decay_after_update" else p * decay
    s = g - m
    w = omb1 * s
    m1 = m + w
    a, q = v * b2, omb2 * g
    r = q * g
    v1 = a + r
    if mistake == "eps_inside_sqrt":
        sq = np.sqrt(v1 + eps)
        dv = sq / bc
        denom = dv
    else:
        sq = np.sqrt(v1)
        dv = sq * bc if mistake == "bc2_sqrt_multiplied" else sq / bc
        denom = dv + eps
    qn = m1 / denom
    t = (-ss) * qn
    pn = p1 + t
    if mistake == "decay_after_update":
        pn = pn * decay
    if trace is not None:
        trace.extend([g, p1, s, w, m1, a, q, r, v1, sq, dv, denom, qn, t, pn])
    assert all(x.dtype == F for x in (pn, m1, v1))
    return pn, m1, v1


def no_subnormals(trace):
    """True when every intermediate of ``adamw_emu`` is zero or a normal fp32 number (and finite)."""
    return all(bool(np.all(np.isfinite(x)) and np.all((x == 0) | (np.abs(x) >= MIN_NORMAL))) for x in trace)


def adamw_bounds(p, g, m, v, sc, coef=1.0, clip=False):
    """Per-element bounds on |fp32 kernel - ``adamw_ref``| for (master, m, v), on the same inputs and scalars.

    g^ = fl(g c): e_g = u |g c|; with clipping on the kernel's coefficient may differ from ``clip_coef`` by 3 ulps (its fp32 division and
    the double -> float square root are the compiler's): + 3u |g c|.
    m' = fl(m + fl(omb1 fl(g^ - m))): omb1 e_g + u omb1 |g c - m| (difference) + u omb1 |g c - m| (product) + u |m'| (sum).
    v' = fl(fl(v b2) + fl(fl(omb2 g^) g^)): u v b2 + [2 omb2 |g c| e_g + 2u omb2 (g c)^2] + u v'   with v' = v b2 + omb2 (g c)^2:
         u (2 v b2 + 3 omb2 (g c)^2) + 2 omb2 |g c| e_g.
    sq = fl(sqrt v'^): e_v / (2 sqrt v') + u sqrt v';  dv = fl(sq / bc): e_sq / bc + u sqrt v' / bc;  den = fl(dv + eps): + u den.
    q = fl(m'^ / den^): e_m / den + |m'| e_den / den^2 + u |m' / den|;  t = fl(ss q): ss e_q + u |t|;  p1 = fl(p decay): u |p decay|;
    p' = fl(p1 - t): e_p1 + e_t + u |p'|.
    Each bound times SLACK (the second-order terms) plus TINY (a result in the denormal range loses absolute accuracy)."""
    p, g, m, v = (np.asarray(t, dtype=np.float64).ravel() for t in (p, g, m, v))
    omb1, omb2, b2, ss, bc, eps, decay = (sc[k] for k in ("omb1", "omb2", "b2", "step_size", "bc2_sqrt", "eps", "decay"))
    gc = np.abs(g * coef)
    p_ref, m_ref, v_ref = adamw_ref(p, g, m, v, sc, coef)
    e_g = (4.0 if clip else 1.0) * U * gc + TINY
    s = np.abs(g * coef - m)
    e_m = omb1 * e_g + U * (2 * omb1 * s + np.abs(m_ref))
    e_v = U * (2 * v * b2 + 3 * omb2 * gc * gc) + 2 * omb2 * gc * e_g
    rt = np.sqrt(v_ref)
    e_sq = np.where(rt > 0, e_v / (2 * np.maximum(rt, MIN_NORMAL)), np.sqrt(e_v)) + U * rt
    den = rt / bc + eps
    e_den = e_sq / bc + U * rt / bc + U * den
    t = ss * np.abs(m_ref) / den
    e_q = e_m / den + np.abs(m_ref) * e_den / (den * den) + U * np.abs(m_ref) / den
    e_p = U * np.abs(p * decay) + ss * e_q + U * t + U * np.abs(p_ref)
    return e_p * SLACK + TINY, e_m * SLACK + TINY, e_v * SLACK + TINY


# ---- flow-matching loss --------------------------------------------------------------------------------------------------------
def pack(t):
    """[B, C, h, w] -> [B, (h/2)(w/2), 4C] as FluxKontextPipeline._pack_latents: view(B, C, h/2, 2, w/2, 2).permute(0, 2, 4, 1, 3, 5)."""
    B, C, h, w = t.shape
    return t.reshape(B, C, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(B, (h // 2) * (w // 2), 4 * C)


def unpack(t, h, w):
    """The inverse: view(B, h/2, w/2, C, 2, 2).permute(0, 3, 1, 4, 2, 5)."""
    B, _, ch = t.shape
    return t.reshape(B, h // 2, w // 2, ch // 4, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(B, ch // 4, h, w)


def _weighting(B, C, h, w, weight, area, mask):
    wt = torch.ones(B, 1, h, w, dtype=torch.float64)
    if weight is not None:
        wt = wt * weight.double().view(B, 1, 1, 1)
    if area is not None:
        wt = wt * area.double().view(B, 1, h, w)
    if mask is not None:
        wt = wt * mask.double().view(B, 1, h, w)
    return wt.expand(B, C, h, w)


def flow_ref(pred, x, noise, sigma=None, weight=None, area=None, mask=None):
    """float64.  pred: packed [B, S, 4C]; x, noise: [B, C, h, w]; sigma, weight: [B]; area, mask: [B, 1, h, w].
    tokens = pack((1 - sigma) x + sigma noise) (when sigma is given); d = unpack(pred) - (noise - x); sum = sum of wt d^2;
    denominator = mask.sum() * C with a mask, the element count otherwise; loss = sum / denominator;
    grad = pack(2 wt d / denominator)."""
    B, C, h, w = x.shape
    x64, n64 = x.double(), noise.double()
    out = {}
    if sigma is not None:
        sg = sigma.double().view(B, 1, 1, 1)
        out["tokens"] = pack((1.0 - sg) * x64 + sg * n64)
    t = n64 - x64
    d = unpack(pred.double(), h, w) - t
    wt = _weighting(B, C, h, w, weight, area, mask)
    denom = float(mask.double().sum()) * C if mask is not None else float(x.numel())
    terms = wt * d * d
    out.update(sum=math.fsum(terms.reshape(-1).tolist()), denom=denom, grad=pack(2.0 * wt * d / denom))
    out["loss"] = out["sum"] / denom
    return out


def flow_bounds(pred, x, noise, weight=None, area=None, mask=None):
    """Bounds for ``flow_loss_kernel`` against ``flow_ref``: dict(loss=scalar, grad=per packed element, BEFORE the bf16 rounding).

    d^ = fl(pred - fl(noise - x)): |dd| <= u (|noise - x| + |d|) (1 + u).   wt^ = fl(fl(weight area) mask): 2u wt.
    term^ = fl(wt^ fl(d^ d^)): wt (2 |d| dd + dd^2) from d, 2u (weight) + u (square) + u (product) = 4u relative on wt (|d| + dd)^2,
    a fifth u for their cross terms.  The double sum of the fp32 terms (the conversion is exact) adds U64 per addition along
    the longest chain (``sum_depth``: trips + 6 + 4 in the block, ceil(blocks / 256) + 6 + 4 in the finishing block) plus two
    for the scale (1 / denominator in double, then the product), relative to the sum of the (positive) terms.
    grad32 = fl(fl(2 wt^ d^) inv^), inv^ = fl(1 / denominator) with the denominator exact in fp32 (asserted): 2u (weight) + u (inv)
    + 2u (products) = 5u |grad| plus (2 wt / denominator) dd, times SLACK, plus TINY."""
    B, C, h, w = x.shape
    t = noise.double() - x.double()
    d = unpack(pred.double(), h, w) - t
    wt = _weighting(B, C, h, w, weight, area, mask)
    denom = float(mask.double().sum()) * C if mask is not None else float(x.numel())
    assert denom < 2 ** 24 and (mask is None or float(mask.double().sum()) < 2 ** 24), "the denominator is not exact in fp32"
    dd = U * (t.abs() + d.abs()) * (1.0 + U)
    e_term = wt * (2 * d.abs() * dd + dd * dd) + 5 * U * wt * (d.abs() + dd) ** 2 + TINY
    total = float((wt * d * d).sum())
    loss = (float(e_term.sum()) + (sum_depth(x.numel()) + 2) * U64 * total) / denom
    g = 2.0 * wt * d / denom
    grad = torch.where(wt == 0, torch.zeros_like(g), (5 * U * g.abs() + (2.0 * wt / denom) * dd) * SLACK + TINY)   # wt = 0: exactly (+-)0
    return dict(loss=loss, grad=pack(grad))


def round_to_bf16(x64):
    """fp64 -> the nearest bf16 (ties to even) in ONE rounding, as fp64 (test_hip_backward_exact.round_to_bf16; values in the normal range)."""
    mant, e = torch.frexp(x64)
    return torch.ldexp(torch.round(mant * 256.0) / 256.0, e)


def bf16_interval(ref64, err):
    """(lo, hi, rounded): rounding to bf16 is monotonic, so the bf16 of ANY fp32 value within ``err`` of ``ref64`` lies in
    [round(ref - err), round(ref + err)].  Where lo == hi the result must be the fp64 value rounded once; where they differ, the fp64
    value lies within ``err`` of a rounding boundary and the neighbour on that side is allowed as well."""
    return round_to_bf16(ref64 - err), round_to_bf16(ref64 + err), round_to_bf16(ref64)


# ---- the input families of test_hip_train_kernels.py (shared with the CPU checks of the bounds) ---------------------------------
CAP = GRID_CAP * THREADS
ADAMW_SIZES = (1, 3, 255, 256, 257, 1027, CAP + 1027)
# gradient type (bf16?), clipping, view offset, grad_scale
ADAMW_COMBOS = [(bf, clip, off, gs) for bf in (False, True) for clip in (False, True) for off in (0, 1) for gs in (1.0, 0.5)]
FLOW_SHAPES = ((4, 16, 128, 128), (2, 16, 128, 136), (3, 16, 12, 20))
FLOW_VARIANTS = ("plain", "weighted", "weighted+area", "weighted+area+mask")


def adamw_case(si, ci):
    """(step, weight_decay, with_bf16) cycled over the size index and the combination index: every triple occurs."""
    k = si * (len(ADAMW_COMBOS) + 1) + ci
    return (1, 2, 1000)[k % 3], (0.0, 0.01)[(k // 3) % 2], (k // 6) % 2 == 0


def adamw_inputs(n, g_is_bf16, seed):
    """p ~ 0.02 randn, gradient ~ 0.05 randn (rounded to bf16 on request), m ~ 1e-3 randn, v ~ (1e-3 randn)^2; fp32 torch tensors."""
    gen = torch.Generator().manual_seed(seed)
    p = 0.02 * torch.randn(n, generator=gen)
    g = 0.05 * torch.randn(n, generator=gen)
    if g_is_bf16:
        g = g.to(torch.bfloat16)
    m = 1e-3 * torch.randn(n, generator=gen)
    v = (1e-3 * torch.randn(n, generator=gen)) ** 2
    return p, g, m, v


def adamw_coef(g, clip, grad_scale):
    """(sumsq in float64 or None, max_norm, coefficient): max_norm = 0.37 of the scaled norm, so the coefficient is active."""
    if not clip:
        return None, 1.0, clip_coef(None, 1.0, grad_scale)
    sumsq = math.fsum((g.double() ** 2).tolist())
    max_norm = 0.37 * grad_scale * math.sqrt(sumsq)
    return sumsq, max_norm, clip_coef(sumsq, max_norm, grad_scale)


def flow_inputs(shape, variant, exact, seed):
    """dict(pred bf16 packed, x, noise, sigma, weight, area, mask).  ``exact``: x, noise, pred integers in [-4, 4], weight in {1, 2, 4},
    area integers in [1, 4]; otherwise randn data, weight = sigma^-2 and 'log' area weights.  mask: 0 / 1 on per-sample sub-rectangles
    (h >> b') x (w >> b'') with b', b'' such that at the first shape the count is a power of two."""
    B, C, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    S = (h // 2) * (w // 2)
    sigma = torch.sigmoid(torch.randn(B, generator=gen))
    if exact:
        ri = lambda *s: torch.randint(-4, 5, s, generator=gen).float()          # noqa: E731
        x, noise, pred = ri(B, C, h, w), ri(B, C, h, w), ri(B, S, 4 * C).to(torch.bfloat16)
        weight = torch.tensor([1.0, 2.0, 4.0])[torch.randint(0, 3, (B,), generator=gen)]
        area = torch.randint(1, 5, (B, 1, h, w), generator=gen).float()
    else:
        x, noise = torch.randn(B, C, h, w, generator=gen), torch.randn(B, C, h, w, generator=gen)
        pred = torch.randn(B, S, 4 * C, generator=gen).to(torch.bfloat16)
        weight = sigma ** -2.0
        area = torch.log1p(torch.rand(B, 1, h, w, generator=gen) * 20.0) + 0.25
    mask = torch.zeros(B, 1, h, w)
    rects = [(h, w), (h // 2, w), (h // 2, w // 2), (h // 2, w // 2)]
    for b in range(B):
        mask[b, :, :rects[b][0], :rects[b][1]] = 1.0
    out = dict(pred=pred, x=x, noise=noise, sigma=sigma, weight=None, area=None, mask=None)
    if variant != "plain":
        out["weight"] = weight
    if "area" in variant:
        out["area"] = area
    if "mask" in variant:
        out["mask"] = mask
    return out
