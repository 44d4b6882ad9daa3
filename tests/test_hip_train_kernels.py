"""GPU: the four launch families of csrc/train_kernels.hip (AdamW, sumsq, noisy tokens, flow loss + gradient) against float64 with
the SAME scalars, within the bounds tests/train_kernels_ref.py derives from the operation order times MARGIN = 2, or bit for bit
where the arithmetic is exact.

grid_for: ``want > 2048 ? 2048 : want`` blocks of 256 threads, one element per thread and trip, so CAP = 2048 * 256 = 524 288
elements fill one trip of the grid-stride loops (asserted below against the reference module's constants and the library's
workspace size); every family runs past it.  Every output lives in a sentinel-filled buffer (test_hip_prodigy_kernels._row); the flow
loss is called through the C ABI for that, with the argument order of ops.flow_loss.

AdamW: sizes 1, 3, 255, 256, 257, 1027, CAP + 1027 x gradient fp32 / bf16 x clipping off / on x view offset 0 / 1 x grad_scale 1 / 0.5,
cycling step in {1, 2, 1000}, weight_decay in {0, 0.01}, param_bf16 given / None.  With clipping off and grad_scale = 1 the
coefficient is exactly 1 and every operation of the kernel is one correctly rounded fp32 operation, so there master, m and v
must equal ``adamw_emu`` BIT FOR BIT (premise, asserted on the host: no intermediate of the emulation is subnormal).
Finding: that equality did not hold for the kernel as first written.  ``__fmul_rn`` / ``__fadd_rn`` / ``__fsub_rn`` are plain operators
to hipcc and ``__fsqrt_rn`` its native (1 ulp) square root, so under the default -ffp-contract=fast-honor-pragmas the update was
three fused multiply-adds around a v_sqrt_f32; likewise the noisy-token mix was one fma, which changes the bf16 token of a few
elements in a million against the reference's separately rounded fp32 expression (test_noisy_tokens, 557 056 elements).  Both
kernels now compile with contraction off and AdamW takes sqrtf (correctly rounded in this build); the claim stands as stated.

sumsq / flow loss on exact data (k / 8 with |k| <= 32; integers in [-4, 4] with integer weights): every term and every double
partial sum is exact, so the results equal the float64 host sums bit for bit and a dropped or doubled element at a trip seam is
a whole-number error.  On random data: within depth x 2^-53 x sum (sumsq; depth from ``sum_depth``) and ``flow_bounds``; the bf16
gradient must be the float64 value rounded once, or its neighbour where that value lies within the derived fp32 error of a rounding
boundary (``bf16_interval``), which may excuse at most 1 % of the elements.

Observed on an MI355X (one run, all 157 cases), worst error as a fraction of the derived bound BEFORE the margin: AdamW master 0.942,
m 0.933, v 0.970 (all at CAP + 1027, the maximum over half a million elements; the emulation on the host reaches 0.942 / 0.906 / 0.970), and
bit-equal to the emulation in all 28 cases with coefficient 1; sumsq on random data equal to the exactly rounded float64 sum (ratio 0); flow loss
at most 0.003 (the bound adds the absolute error of every term, the errors themselves have either sign and cancel); gradient: at
most 0.035 % of the elements near a rounding boundary (4 of 11 520; 217 of 2^20 at the largest shape), of which about one in eight took
the neighbour; every exact case bit for bit.  The whole file ran in 4.8 s.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import train_kernels_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PAD = 8
SENT = 12345.0
CAP = 2048 * 256
HP = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8)


def test_cap_is_grid_fors():
    from gpt_image_edit_amd import libfk
    assert CAP == 524_288 == R.CAP == R.GRID_CAP * R.THREADS and R.blocks_for(CAP) == 2048 == R.blocks_for(CAP + 1027)
    assert R.blocks_for(CAP - 256) == 2047
    assert libfk.load().fk_reduce_ws_doubles() >= R.GRID_CAP      # one double per block of a capped launch


def _row(vals, off=0, dtype=None):
    """A device buffer of sentinels with ``vals`` at [PAD + off, PAD + off + n); returns (buffer, view shaped like vals)."""
    dtype = dtype or vals.dtype
    n = vals.numel()
    buf = torch.full((n + 2 * PAD + 1,), SENT, dtype=dtype, device="cuda")
    view = buf[PAD + off: PAD + off + n].view(vals.shape)
    view.copy_(vals)
    return buf, view


def _sentinels_ok(buf, off, n):
    return bool((buf[:PAD + off] == SENT).all()) and bool((buf[PAD + off + n:] == SENT).all())


def _check(name, got, want, bound, named):
    """max |got - want| / bound; a failure names the worst element and the elements of ``named`` (trip seam, last)."""
    got = got.double().cpu().numpy().ravel()
    ratio = np.abs(got - want) / bound
    worst = int(np.argmax(ratio))
    if not ratio[worst] <= R.MARGIN:
        rows = [f"  element {i}: got {got[i]:.9e} want {want[i]:.9e} error / bound {ratio[i]:.3f}" for i in sorted(set(named + [worst]))]
        raise AssertionError(f"{name}: worst error / bound {ratio[worst]:.3f} at element {worst} of {got.size}\n" + "\n".join(rows))
    return float(ratio[worst])


# ---- AdamW -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(R.ADAMW_SIZES)))
@pytest.mark.parametrize("ci", range(len(R.ADAMW_COMBOS)))
def test_adamw(si, ci):
    from gpt_image_edit_amd import ops
    n = R.ADAMW_SIZES[si]
    g_bf16, clip, off, gs = R.ADAMW_COMBOS[ci]
    step, wd, with_bf16 = R.adamw_case(si, ci)
    p, g, m, v = R.adamw_inputs(n, g_bf16, seed=n % 1000 + ci)
    sumsq, max_norm, coef = R.adamw_coef(g, clip, gs)
    assert (coef < gs) == clip and (clip or coef == gs)                        # the clipping coefficient is active exactly when asked
    (bp, vp), (bg, vg), (bm, vm), (bv, vv) = rows = [_row(t, off) for t in (p, g, m, v)]
    bb, vb = _row(torch.zeros(n, dtype=BF), off)
    ops.adamw_step(vp, vg, vm, vv, step, weight_decay=wd, grad_sumsq=None if sumsq is None else torch.tensor([sumsq], dtype=torch.float64).cuda(),
                   max_grad_norm=max_norm, param_bf16=vb if with_bf16 else None, grad_scale=gs, **HP)
    torch.cuda.synchronize()
    ins = tuple(t.float().double().numpy() for t in (p, g, m, v))
    sc = R.adamw_scalars(step, weight_decay=wd, **HP)
    want = R.adamw_ref(*ins, sc, coef)
    bounds = R.adamw_bounds(*ins, sc, coef, clip)
    named = [i for i in (CAP - 1, CAP, n - 1) if 0 <= i < n]
    tag = f"adamw n={n} bf16_grad={g_bf16} clip={clip} off={off} grad_scale={gs} step={step} wd={wd} bf16_copy={with_bf16}"
    r = [_check(f"{tag}: {what}", t, w_, b_, named) for what, t, w_, b_ in zip(("master", "m", "v"), (vp, vm, vv), want, bounds)]
    print(f"[{tag}] master {r[0]:.3f} m {r[1]:.3f} v {r[2]:.3f} of the bound", flush=True)
    assert not torch.equal(vp.cpu(), p)
    if with_bf16:
        assert torch.equal(vb, vp.to(BF)), "the bf16 copy is not the rounded master"
    else:
        assert bool((vb == 0).all())
    assert torch.equal(vg.cpu(), g), "the gradient was written"
    assert all(_sentinels_ok(b, off, n) for b in (bp, bg, bm, bv, bb))
    if not clip and gs == 1.0:
        trace = []
        emu = R.adamw_emu(*ins, sc, coef, g_bf16, trace=trace)
        assert coef == 1.0 and R.no_subnormals(trace), "premise of the bit equality"
        for what, t, e in zip(("master", "m", "v"), (vp, vm, vv), emu):
            t = t.cpu().numpy()
            bad = np.flatnonzero(t.view(np.int32) != e.view(np.int32))
            assert bad.size == 0, (f"{tag}: {what} differs from the fp32 emulation in {bad.size} of {n} elements, first at {bad[0]}: "
                                   f"got {t[bad[0]]!r} emulation {e[bad[0]]!r}")


def check_bf16_gradient_step(ops, master, g16, m, v, step, **hp):
    """What test_hip_training.test_adamw_with_clipping_matches_torch ends with: one unclipped step with a bf16 gradient on the
    state that test has reached, held to ``adamw_ref`` within the bound (it replaces an assertion that the master merely moved)."""
    ins = tuple(t.float().double().cpu().numpy().ravel() for t in (master, g16, m, v))
    sc = R.adamw_scalars(step, lr=hp["lr"], betas=hp["betas"], eps=hp.get("eps", 1e-8), weight_decay=hp["weight_decay"])
    ops.adamw_step(master, g16, m, v, step, **hp)
    torch.cuda.synchronize()
    want, bounds = R.adamw_ref(*ins, sc, 1.0), R.adamw_bounds(*ins, sc, 1.0, False)
    n = ins[0].size
    return [_check(f"adamw bf16 gradient, {tuple(master.shape)}: {what}", t, w_, b_, [n - 1])
            for what, t, w_, b_ in zip(("master", "m", "v"), (master, m, v), want, bounds)]


# ---- sumsq -------------------------------------------------------------------------------------------------------------------
def _eighths(n, seed, dtype):
    """k / 8 with integer |k| <= 32: exact in bf16 and fp32, squares k^2 / 64 exact, sums of up to 2^29 of them exact in double."""
    k = torch.randint(-32, 33, (n,), generator=torch.Generator().manual_seed(seed))
    return (k.float() / 8.0).to(dtype), int((k * k).sum())


def _out64(fill=SENT):
    buf = torch.full((2 * PAD + 1,), SENT, dtype=torch.float64, device="cuda")
    buf[PAD] = fill
    return buf, buf[PAD:PAD + 1]


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [1, 255, 257, CAP - 1, CAP, CAP + 1, CAP + 1027])
def test_sumsq_exact(n, dtype):
    from gpt_image_edit_amd import ops
    vals, k2 = _eighths(n, seed=n % 1000 + 3, dtype=dtype)
    assert n * 1024 < 2 ** 53 and torch.equal(vals.double() * 8, (vals.double() * 8).round())      # premise: exact partial sums
    bg, vg = _row(vals)
    bo, out = _out64()
    ops.sumsq([vg], out=out)
    torch.cuda.synchronize()
    assert float(out) == k2 / 64.0, f"sumsq n={n} {dtype}: got {float(out)!r} want {k2 / 64.0!r} (difference {float(out) * 64 - k2} / 64)"
    assert torch.equal(vg.cpu(), vals) and _sentinels_ok(bg, 0, n) and _sentinels_ok(bo, 0, 1)


@pytest.mark.parametrize("prefill", [0.0, 777.0])
def test_sumsq_list_accumulates_in_order_and_overwrites_out(prefill):
    from gpt_image_edit_amd import ops
    parts = [_eighths(CAP + 1027, 5, torch.float32), _eighths(257, 6, BF), _eighths(1, 7, torch.float32)]
    rows = [_row(vals) for vals, _ in parts]
    bo, out = _out64(prefill)
    got = ops.sumsq([view for _, view in rows], out=out)
    torch.cuda.synchronize()
    assert got is out and float(out) == sum(k2 for _, k2 in parts) / 64.0        # the first tensor overwrites, the others add
    assert _sentinels_ok(bo, 0, 1) and all(_sentinels_ok(b, 0, vals.numel()) for (b, _), (vals, _) in zip(rows, parts))


def test_sumsq_random_within_the_depth_of_the_double_sum():
    """Every term (double) v * (double) v is exact; the two-stage double sum adds 2^-53 per addition along its longest chain."""
    from gpt_image_edit_amd import ops
    n = CAP + 1027
    assert R.sum_depth(n) == 2 + 6 + 4 + 8 + 6 + 4
    vals = 0.05 * torch.randn(n, generator=torch.Generator().manual_seed(8))
    want = math.fsum((vals.double() ** 2).tolist())
    outs = []
    for _ in range(2):
        bo, out = _out64()
        ops.sumsq([vals.cuda()], out=out)
        outs.append(float(out))
        assert _sentinels_ok(bo, 0, 1)
    bound = R.sum_depth(n) * R.U64 * want
    print(f"[sumsq random] n={n}: error / bound {abs(outs[0] - want) / bound:.3f}", flush=True)
    assert abs(outs[0] - want) <= R.MARGIN * bound
    assert outs[0] == outs[1], "two runs differ"


# ---- noisy tokens --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,into_buffer", [((2, 16, 128, 136), False), ((1, 4, 6, 10), False), ((2, 16, 128, 136), True)])
def test_noisy_tokens(shape, into_buffer):
    """torch.equal with pack_latents(((1 - sigma) x + sigma noise).to(bf16)) in fp32 torch.  2 x 16 x 128 x 136 = 557 056 elements: a second
    trip, its seam inside batch 1, w / 2 = 68 no power of two; ``into_buffer``: written into buf[:, :S] of a [B, 2S, 4C] buffer."""
    from gpt_image_edit_amd import ops
    from oracle import helpers
    B, C, h, w = shape
    S = (h // 2) * (w // 2)
    gen = torch.Generator().manual_seed(9)
    x, noise = torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)
    sigma = torch.sigmoid(torch.randn(B, generator=gen))
    sg = sigma.view(B, 1, 1, 1)
    ref = helpers.pack_latents(((1.0 - sg) * x + sg * noise).to(BF))
    assert (B * C * h * w > CAP) == (shape[2] == 128)
    rows = [_row(t) for t in (x, noise, sigma)]
    if into_buffer:
        bo, whole = _row(torch.full((B, 2 * S, 4 * C), SENT, dtype=BF))
        out = whole[:, :S]
    else:
        bo, out = _row(torch.full((B, S, 4 * C), SENT, dtype=BF), off=1)
    got = ops.flow_noisy_tokens(rows[0][1], rows[1][1], rows[2][1], out=out)
    torch.cuda.synchronize()
    bad = (got.cpu().view(torch.int16) != ref.view(torch.int16)).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} of {ref.numel()} tokens differ, first at {bad[0].tolist()}: got "
                               f"{got.cpu()[tuple(bad[0])].item()!r} want {ref[tuple(bad[0])].item()!r}")
    if into_buffer:
        assert bool((whole[:, S:] == SENT).all()) and _sentinels_ok(bo, 0, whole.numel())
    else:
        assert _sentinels_ok(bo, 1, out.numel())
    assert all(torch.equal(view.cpu(), t) and _sentinels_ok(b, 0, t.numel()) for (b, view), t in zip(rows, (x, noise, sigma)))


# ---- flow loss -----------------------------------------------------------------------------------------------------------------
def _flow_loss(ins, want_grad=True, strided=False):
    """fk_flow_loss_weighted_bf16 as ops.flow_loss calls it, with the loss, the gradient and the workspace in sentinel rows.
    ``strided``: pred as the [:, :S] view of a [B, 2S, 4C] buffer whose other half is NaN.  Returns (loss float, grad on the host)."""
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    B, C, h, w = ins["x"].shape
    S = (h // 2) * (w // 2)
    dev = {k: (t.cuda().contiguous() if t is not None else None) for k, t in ins.items()}
    pred = dev["pred"]
    if strided:
        wide = torch.full((B, 2 * S, 4 * C), float("nan"), dtype=BF, device="cuda")
        wide[:, :S] = pred
        pred = wide[:, :S]
        assert pred.stride(0) == 2 * S * 4 * C and pred.stride(1) == 4 * C
    mask_sum = dev["mask"].sum().reshape(1) if dev["mask"] is not None else None
    bg, grad = _row(torch.full((B, S, 4 * C), SENT, dtype=BF), off=1)
    bo, loss = _out64()
    nws = lib.fk_reduce_ws_doubles()
    bw, ws = _row(torch.zeros(nws, dtype=torch.float64))
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)      # noqa: E731
    libfk.check(lib.fk_flow_loss_weighted_bf16(P(pred), pred.stride(0), P(dev["x"]), P(dev["noise"]), P(dev["weight"]), P(dev["area"]),
                                               P(dev["mask"]), P(mask_sum), P(grad if want_grad else None), grad.stride(0) if want_grad else 0,
                                               P(loss), P(ws), B, C, h, w, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "fk_flow_loss_weighted_bf16")
    torch.cuda.synchronize()
    assert _sentinels_ok(bo, 0, 1) and _sentinels_ok(bw, 0, nws) and _sentinels_ok(bg, 1, grad.numel())
    assert bool((ws[R.blocks_for(B * C * h * w):] == 0).all()), "a partial beyond the grid was written"
    if not want_grad:
        assert bool((grad == SENT).all())
    return float(loss), grad.cpu()


_REF = {}


def _flow_case(shape, variant, exact):
    """Inputs, float64 reference and bounds, computed once per case and left unchanged."""
    key = (shape, variant, exact)
    if key not in _REF:
        ins = R.flow_inputs(shape, variant, exact, seed=(20 if exact else 40) + R.FLOW_VARIANTS.index(variant))
        ref = R.flow_ref(ins["pred"], ins["x"], ins["noise"], None, ins["weight"], ins["area"], ins["mask"])
        bounds = R.flow_bounds(ins["pred"], ins["x"], ins["noise"], ins["weight"], ins["area"], ins["mask"])
        _REF[key] = (ins, ref, bounds)
    return _REF[key]


def _outside(ins):
    B, C, h, w = ins["x"].shape
    return R.pack((1.0 - ins["mask"]).expand(B, C, h, w)) > 0


@pytest.mark.parametrize("variant", R.FLOW_VARIANTS)
@pytest.mark.parametrize("shape", R.FLOW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flow_loss_exact(shape, variant):
    """Integer data: every term wt d^2 is an integer <= 16 * 144 = 2304 and every double partial sum is exact, so the loss equals
    sum * (1 / denominator) formed in double as ``finish_sum_kernel`` forms it.  Where 1 / denominator is a power of two (4 x 16 x 128 x 128:
    2^20 elements, 2^15 pixels under the mask) the gradient 2 wt d / denominator is exact in fp32 and must equal the float64 value
    rounded to bf16 once, bit for bit; elsewhere it obeys the neighbour rule with ``flow_bounds``."""
    ins, ref, bounds = _flow_case(shape, variant, True)
    n = ins["x"].numel()
    assert ref["sum"] == round(ref["sum"]) and 2304 * n < 2 ** 53
    loss, grad = _flow_loss(ins)
    want = ref["sum"] * (1.0 / ref["denom"])
    assert loss == want, f"loss * denominator is off by {loss * ref['denom'] - ref['sum']!r} (sum {ref['sum']!r}, denominator {ref['denom']!r})"
    lo, hi, once = R.bf16_interval(ref["grad"], bounds["grad"])
    g = grad.double()
    if shape == R.FLOW_SHAPES[0]:
        assert math.frexp(ref["denom"])[0] == 0.5, "premise: the denominator is a power of two"
        bad = (g != once).nonzero()
        assert bad.shape[0] == 0, f"{bad.shape[0]} gradient elements differ from the float64 value rounded once, first at {bad[0].tolist()}"
    else:
        assert bool(((g >= lo) & (g <= hi)).all())
    if ins["mask"] is not None:
        out = _outside(ins)
        assert bool(out.any()) and float(g[out].abs().max()) == 0 and float(g[~out].abs().max()) > 0
    # the same bits without the gradient, from the strided prediction, and from a second run
    assert _flow_loss(ins, want_grad=False)[0] == loss
    l2, g2 = _flow_loss(ins, strided=True)
    assert l2 == loss and torch.equal(g2.view(torch.int16), grad.view(torch.int16))


@pytest.mark.parametrize("variant", R.FLOW_VARIANTS)
@pytest.mark.parametrize("shape", R.FLOW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_flow_loss_random(shape, variant):
    ins, ref, bounds = _flow_case(shape, variant, False)
    loss, grad = _flow_loss(ins)
    lo, hi, once = R.bf16_interval(ref["grad"], bounds["grad"])
    g = grad.double()
    excused = (lo != hi)
    neighbour = int((g != once).sum())
    print(f"[flow loss random] {shape} {variant}: loss error / bound {abs(loss - ref['loss']) / bounds['loss']:.3f}; gradient: "
          f"{int(excused.sum())} of {g.numel()} elements near a rounding boundary (share {float(excused.double().mean()):.5f}), "
          f"{neighbour} took the neighbour", flush=True)
    assert abs(loss - ref["loss"]) <= R.MARGIN * bounds["loss"]
    bad = ((g < lo) | (g > hi)).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} gradient elements are neither the float64 value rounded once nor an excused neighbour, first at "
                               f"{bad[0].tolist()}: got {g[tuple(bad[0])].item()!r} want {once[tuple(bad[0])].item()!r}")
    assert float(excused.double().mean()) <= 0.01
    if ins["mask"] is not None:
        assert float(g[_outside(ins)].abs().max()) == 0
    # strided prediction (the training step's call), no gradient, and a second run: the same bits
    l2, g2 = _flow_loss(ins, strided=True)
    assert l2 == loss and torch.equal(g2.view(torch.int16), grad.view(torch.int16))
    assert _flow_loss(ins, want_grad=False)[0] == loss
    l3, g3 = _flow_loss(ins)
    assert l3 == loss and torch.equal(g3.view(torch.int16), grad.view(torch.int16))
