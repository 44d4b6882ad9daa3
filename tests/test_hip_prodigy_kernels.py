"""GPU: the four Prodigy kernels (csrc/prodigy.hip) against float64 with the SAME scalars, within the bounds tests/prodigy_ref.py
derives from the operation order, times MARGIN = 2.

Sizes: 1, 3, 4, 5 (below / at / past one 4-element group), 255, 256, 257, 1027 (a ragged tail, more than one block) and
2 097 152 + 1027 = one element group past the first grid-stride trip of the 2048-block cap at 4 elements per lane, plus a tail.
Every size runs aligned (16-byte vectors + scalar tail) and as views offset by one element (the scalar form), with fp32 and bf16
gradients, clipping on and off, grad_scale = 0.5.  With clipping on the bound allows the coefficient 3 more ulps: its fp32
division and the double -> float square root are the compiler's, not pinned by the emulation.

Observed on an MI355X (one run, all 121 cases), worst error as a fraction of the derived bound BEFORE the margin: m 0.967, v 0.991,
s 0.962 (all at the largest size, the maximum over 2 M elements), master 0.962, sum g (p0 - p) 0.152; sum |s| equal to the float64 sum of the kernel's
own s in every case (ratio 0).  The whole file ran in 4.5 s.
"""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

import prodigy_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
PAD = 8
SENT = 12345.0
BIG = 2_097_152 + 1027
SIZES = (1, 3, 4, 5, 255, 256, 257, 1027, BIG)
COMBOS = list(itertools.product((torch.float32, BF), (False, True), (0, 1)))      # gradient type, clipping, view offset
HP = dict(lr=1.0, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01, d0=1e-6, d_coef=1.0)
SLOT = {n: i for i, n in enumerate(R.Ref({}, None).scalars())}
SCAL = dict(d=3.0e-4, d_max=5.0e-4, d_numerator=1.0e-3, d_denom=0.0, d_hat=0.0, dlr=2.5e-4, k=3, skipped=0, sum_dot=0.125, sum_abs=2.0)


def _row(vals, off, dtype=torch.float32):
    """A device buffer of sentinels with ``vals`` at [PAD + off, PAD + off + n); returns (buffer, view)."""
    n = vals.numel()
    buf = torch.full((n + 2 * PAD + 1,), SENT, dtype=dtype, device="cuda")
    view = buf[PAD + off: PAD + off + n]
    view.copy_(vals)
    return buf, view


def _sentinels_ok(buf, off, n):
    return bool((buf[:PAD + off] == SENT).all()) and bool((buf[PAD + off + n:] == SENT).all())


def _state(**kw):
    s = dict(SCAL, **kw)
    return torch.tensor([float(s[k]) for k in SLOT], dtype=torch.float64).cuda()


def _inputs(n, gdtype, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    p0 = (p + 0.01 * torch.randn(n, generator=g)).float()
    grad = (0.05 * torch.randn(n, generator=g)).to(gdtype)
    m = 1e-5 * torch.randn(n, generator=g)
    v = (1e-5 * torch.randn(n, generator=g)) ** 2
    s = 1e-3 * torch.randn(n, generator=g)
    return p, p0, grad, m, v, s


def _hp(i):
    return R.kernel_hp(dict(HP, decouple=i not in (1, 6), safeguard_warmup=i not in (2, 5)))


def _ref(hp, p, p0, m, v, s, **scal):
    ref = R.Ref({"w": p.double().numpy()}, hp)
    ref.p0["w"], ref.m["w"], ref.v["w"], ref.s["w"] = (t.double().numpy() for t in (p0, m, v, s))
    ref.set_scalars(**dict(SCAL, **scal))
    return ref


def _ratio(got, want, bound):
    return float(np.max(np.abs(got.double().cpu().numpy() - want) / bound))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("ci", range(len(COMBOS)))
def test_moments(n, ci):
    from gpt_image_edit_amd import ops
    gdtype, clip, off = COMBOS[ci]
    hp = _hp(ci)
    p, p0, grad, m, v, s = _inputs(n, gdtype, seed=n % 1000 + ci)
    rows = [_row(t, off, t.dtype) for t in (p, p0, grad, m, v, s)]
    (bp, vp), (bp0, vp0), (bg, vg), (bm, vm), (bv, vv), (bs, vs) = rows
    state = _state()
    sumsq = max_norm = None
    if clip:
        sumsq = (grad.double() ** 2).sum().reshape(1).cuda()
        max_norm = 0.37 * 0.5 * math.sqrt(sumsq.item())                     # below the scaled norm: the coefficient is active
    coef = R.clip_coef(None if sumsq is None else sumsq.item(), max_norm, 0.5)
    assert (coef < 0.5) == clip
    ops.prodigy_moments(vp, vp0, vg, vm, vv, vs, state, betas=hp["betas"], beta3=hp["beta3"], weight_decay=hp["weight_decay"],
                        d0=hp["d0"], decouple=hp["decouple"], safeguard_warmup=hp["safeguard_warmup"], grad_sumsq=sumsq,
                        max_grad_norm=max_norm if clip else 1.0, grad_scale=0.5)
    torch.cuda.synchronize()
    ref = _ref(hp, p, p0, m, v, s)
    ref.moments_one("w", grad.double().numpy(), coef)
    B = R.bounds_moments(p, p0, grad.float(), m, v, s, SCAL["d"], SCAL["dlr"], hp, coef)
    extra = 3 * R.U * np.abs(grad.double().numpy() * coef) if clip else 0.0          # the coefficient's own 3 ulps (docstring)
    cm, cv, cs = ref._moment_factors()
    geff = np.abs(grad.double().numpy() * coef) + (0 if hp["decouple"] else abs(hp["weight_decay"]) * np.abs(p.double().numpy()))
    bm_, bv_, bs_ = B["m"] + abs(cm) * extra, B["v"] + 2 * np.abs(cv) * geff * extra, B["s"] + abs(cs) * extra
    rm, rv, rs = _ratio(vm, ref.m["w"], bm_), _ratio(vv, ref.v["w"], bv_), _ratio(vs, ref.s["w"], bs_)
    st = state.cpu().numpy()
    d_abs = abs((st[SLOT["sum_abs"]] - SCAL["sum_abs"]) - float(vs.double().abs().sum()))
    b_abs = B["sum_abs_order"] + 4 * R.U64 * st[SLOT["sum_abs"]]
    d_dot = abs((st[SLOT["sum_dot"]] - SCAL["sum_dot"]) - ref.sum_dot + SCAL["sum_dot"])
    b_dot = B["dot"] + float(np.sum(np.abs(p0.double().numpy() - p.double().numpy()) * extra)) + 4 * R.U64 * abs(st[SLOT["sum_dot"]])
    print(f"[prodigy moments] n={n} {gdtype} clip={clip} off={off}: m {rm:.3f} v {rv:.3f} s {rs:.3f} "
          f"dot {d_dot / b_dot:.3f} abs {d_abs / b_abs:.3f} of the bound", flush=True)
    assert max(rm, rv, rs) <= R.MARGIN
    assert d_abs <= R.MARGIN * b_abs and d_dot <= R.MARGIN * b_dot
    for k in ("d", "d_max", "d_numerator", "dlr", "k", "skipped"):
        assert st[SLOT[k]] == float(SCAL[k]), k
    for (buf, view), orig in zip(rows[:3], (p, p0, grad)):
        assert torch.equal(view.cpu(), orig), "an input was written"
    assert all(_sentinels_ok(buf, off, n) for buf, _ in rows)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("off,decouple,with_bf16", [(0, True, True), (1, True, True), (0, False, True), (1, False, False)])
def test_apply(n, off, decouple, with_bf16):
    from gpt_image_edit_amd import ops
    hp = R.kernel_hp(dict(HP, decouple=decouple))
    p, _, _, m, v, _ = _inputs(n, torch.float32, seed=n % 1000 + 7)
    m = m * 30
    if n > 4:
        v[3] = 0.0                                     # sqrt(0) + d * eps: the scaled eps alone carries the quotient
    (bp, vp), (bm, vm), (bv, vv) = (_row(t, off) for t in (p, m, v))
    bb, vb = _row(torch.zeros(n, dtype=BF), off, BF)
    state = _state(d=4.0e-4)
    ops.prodigy_apply(vp, vm, vv, state, eps=hp["eps"], weight_decay=hp["weight_decay"], decouple=decouple,
                      param_bf16=vb if with_bf16 else None)
    torch.cuda.synchronize()
    ref = _ref(hp, p, p, m, v, m, d=4.0e-4)
    ref.apply_one("w")
    r = _ratio(vp, ref.p["w"], R.bounds_apply(p, m, v, 4.0e-4, SCAL["dlr"], hp))
    print(f"[prodigy apply] n={n} off={off} decouple={decouple}: p {r:.3f} of the bound", flush=True)
    assert r <= R.MARGIN
    assert not torch.equal(vp.cpu(), p)
    if with_bf16:
        assert torch.equal(vb, vp.to(BF)), "the bf16 copy is not the rounded master"
    else:
        assert bool((vb == 0).all())
    assert torch.equal(vm.cpu(), m) and torch.equal(vv.cpu(), v)
    assert all(_sentinels_ok(b, off, n) for b in (bp, bm, bv, bb))
    assert torch.equal(state.cpu(), _state(d=4.0e-4).cpu())


def test_skipped_flag_makes_apply_a_no_op():
    from gpt_image_edit_amd import ops
    n = 1027
    p, _, _, m, v, _ = _inputs(n, torch.float32, seed=1)
    for off in (0, 1):
        (bp, vp), (bm, vm), (bv, vv) = (_row(t, off) for t in (p, m, v))
        bb, vb = _row(torch.full((n,), 3.0, dtype=BF), off, BF)
        ops.prodigy_apply(vp, vm, vv, _state(skipped=1), eps=1e-8, weight_decay=0.01, param_bf16=vb)
        torch.cuda.synchronize()
        assert torch.equal(vp.cpu(), p) and bool((vb == 3.0).all())


@pytest.mark.parametrize("n,off", [(BIG, 0), (BIG, 1), (1027, 0)])
def test_two_launches_give_equal_bits_and_calls_accumulate_in_order(n, off):
    from gpt_image_edit_amd import ops
    hp = _hp(0)
    p, p0, grad, m, v, s = _inputs(n, torch.float32, seed=5)
    outs = []
    for _ in range(2):
        rows = [_row(t, off) for t in (p, p0, grad, m, v, s)]
        state = _state()
        views = [r[1] for r in rows]
        for _call in range(2):                                   # the second call adds onto the first one's running sums
            ops.prodigy_moments(*views, state, betas=hp["betas"], beta3=hp["beta3"], weight_decay=0.01, grad_scale=0.5)
        ops.prodigy_apply(views[0], views[3], views[4], state, eps=1e-8, weight_decay=0.01)
        torch.cuda.synchronize()
        outs.append([t.cpu().clone() for t in views] + [state.cpu().clone()])
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    assert outs[0][-1][SLOT["sum_abs"]] > SCAL["sum_abs"]


def test_begin_and_state():
    """bc = sqrt(1 - beta2^k) / (1 - beta1^k) with the device's pow: 2 ulps of pow amplified by beta^k / (1 - beta^k) <= 99 at k = 1,
    beta2 = 0.99, plus a handful of roundings: 1e-13 relative."""
    from gpt_image_edit_amd import ops
    for k, bias in ((0, True), (3, True), (1000, True), (3, False)):
        hp = R.kernel_hp(dict(HP, use_bias_correction=bias, lr=0.75))
        state = _state(k=k, skipped=1)
        ops.prodigy_begin(state, 0.75, HP["betas"], None, bias)
        got = ops.prodigy_state(state)
        ref = R.Ref({}, hp)
        ref.set_scalars(**dict(SCAL, k=k))
        ref.begin()
        want = ref.scalars()
        assert got["k"] == k and got["skipped"] is False and got["sum_dot"] == 0.0 and got["sum_abs"] == 0.0
        assert got["d"] == SCAL["d"] and got["d_max"] == SCAL["d_max"]
        for key in ("dlr", "d_numerator"):
            assert abs(got[key] - want[key]) <= 1e-13 * abs(want[key]), (key, k, got[key], want[key])
    fresh = ops.prodigy_state(ops.prodigy_init_state(2e-6))
    assert fresh == dict(d=2e-6, d_max=2e-6, d_numerator=0.0, d_denom=0.0, d_hat=0.0, dlr=0.0, k=0, skipped=False, sum_dot=0.0, sum_abs=0.0)


UPDATE_CASES = {
    "d == d0, d_hat above": dict(d=1e-6, d_max=1e-6, d_numerator=3e-10, dlr=1e-6, sum_dot=0.4, sum_abs=7e-5),
    "d == d0, d_hat below": dict(d=1e-6, d_max=1e-6, d_numerator=1e-12, dlr=1e-6, sum_dot=-0.2, sum_abs=7e-3),
    "d > d0, d_hat above": dict(d=3e-4, d_max=3e-4, d_numerator=2e-3, dlr=2.5e-4, sum_dot=0.5, sum_abs=1.5),
    "d > d0, d_hat < d": dict(d=3e-4, d_max=3e-4, d_numerator=1e-5, dlr=2.5e-4, sum_dot=-0.001, sum_abs=1.5),
    "finite growth rate": dict(d=3e-4, d_max=3e-4, d_numerator=2e-3, dlr=2.5e-4, sum_dot=0.5, sum_abs=1.5, growth_rate=1.02),
    "growth rate, d below d_max": dict(d=3e-4, d_max=9e-4, d_numerator=1e-5, dlr=2.5e-4, sum_dot=0.0, sum_abs=1.5, growth_rate=1.5),
    "zero denominator": dict(d=3e-4, d_max=3e-4, d_numerator=2e-3, dlr=2.5e-4, sum_dot=0.0, sum_abs=0.0),
}


@pytest.mark.parametrize("case", sorted(UPDATE_CASES))
def test_update_d(case):
    from gpt_image_edit_amd import ops
    c = dict(UPDATE_CASES[case])
    gr = c.pop("growth_rate", float("inf"))
    hp = R.kernel_hp(dict(HP, growth_rate=gr, d_coef=1.25))
    state = _state(**c)
    ops.prodigy_update_d(state, hp["d0"], 1.25, gr)
    got = ops.prodigy_state(state)
    ref = R.Ref({}, hp)
    ref.set_scalars(**dict(SCAL, **c))
    ref.update_d()
    want = ref.scalars()
    for key in ("d", "d_max", "d_numerator", "d_denom", "d_hat"):
        assert abs(got[key] - want[key]) <= 1e-15 * abs(want[key]), (case, key, got[key], want[key])
    assert got["k"] == want["k"] and got["skipped"] == want["skipped"] and got["dlr"] == c["dlr"]
    if case == "zero denominator":
        assert got["skipped"] and got["k"] == SCAL["k"] and got["d"] == c["d"]
    elif case.startswith("d == d0, d_hat above"):
        assert got["d"] > 1e-6 and got["k"] == SCAL["k"] + 1
    elif case == "d > d0, d_hat < d":
        assert got["d"] == c["d"]
    elif case == "finite growth rate":
        assert got["d"] == pytest.approx(3e-4 * 1.02, rel=1e-15) and got["d_max"] > got["d"]


def test_refused_arguments_write_nothing():
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    n = 64
    bufs = [torch.full((n,), 2.0, device="cuda") for _ in range(6)]
    bf = torch.full((n,), 2.0, device="cuda", dtype=BF)
    state, ws = _state(), torch.zeros(lib.fk_prodigy_ws_doubles(), dtype=torch.float64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def moments(ptrs=None, n_=n, scale=0.5, b=(0.9, 0.99, 0.995), d0=1e-6, state_=state, ws_=ws):
        ptrs = bufs if ptrs is None else ptrs
        return lib.fk_prodigy_moments(P(ptrs[0]), P(ptrs[1]), P(ptrs[2]), 0, P(ptrs[3]), P(ptrs[4]), P(ptrs[5]), P(state_), P(None), 1.0,
                                      scale, b[0], b[1], b[2], 0.01, d0, 1, 1, n_, P(ws_), st)
    bad = [moments(n_=0), moments(n_=-4), moments(scale=0.0), moments(scale=-1.0), moments(d0=0.0), moments(d0=-1e-6),
           moments(b=(1.0, 0.99, 0.995)), moments(b=(0.9, -0.1, 0.995)), moments(b=(0.9, 0.99, 1.5)), moments(state_=None),
           moments(ws_=None)]
    bad += [moments(ptrs=[None if j == i else t for j, t in enumerate(bufs)]) for i in range(6)]
    bad += [lib.fk_prodigy_apply(P(bufs[0]), P(bf), P(bufs[3]), P(bufs[4]), P(state), 1e-8, 0.01, 1, 0, st),
            lib.fk_prodigy_apply(P(None), P(bf), P(bufs[3]), P(bufs[4]), P(state), 1e-8, 0.01, 1, n, st),
            lib.fk_prodigy_apply(P(bufs[0]), P(bf), P(None), P(bufs[4]), P(state), 1e-8, 0.01, 1, n, st),
            lib.fk_prodigy_apply(P(bufs[0]), P(bf), P(bufs[3]), P(bufs[4]), P(None), 1e-8, 0.01, 1, n, st),
            lib.fk_prodigy_begin(P(None), 1.0, 0.9, 0.99, 0.995, 1, st), lib.fk_prodigy_begin(P(state), 1.0, 1.0, 0.99, 0.995, 1, st),
            lib.fk_prodigy_begin(P(state), 1.0, 0.9, 0.99, -0.5, 1, st), lib.fk_prodigy_update_d(P(None), 1e-6, 1.0, 2.0, st),
            lib.fk_prodigy_update_d(P(state), 0.0, 1.0, 2.0, st)]
    torch.cuda.synchronize()
    assert all(code != 0 for code in bad), bad
    assert b"prodigy" in lib.fk_last_error()
    assert all(bool((t == 2.0).all()) for t in bufs + [bf]) and torch.equal(state.cpu(), _state().cpu()) and not bool(ws.any())
    assert moments() == 0                                       # the same call with good arguments runs
