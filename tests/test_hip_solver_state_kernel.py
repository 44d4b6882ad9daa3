"""GPU: ``fk_solver_step_f32`` against the op-by-op float32 torch expression of the step on the CPU (``solver_state_ref.step``:
``torch.mul`` then ``torch.add``, pinned by ``test_solver_state_ref.py``) at 0 ulp on BOTH outputs -- the float32 state's bits
and the bf16 token rows' bits.  Every product and every sum of the rule is one float32 operation, so the expression is exactly
restatable.  The sentinel layout is that of ``test_hip_solver_kernel.py``, with guard elements around the state as well."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref  # noqa: E402
import solver_ref as R  # noqa: E402
import solver_state_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C = 64
PAD_X, PAD_V, GUARD = 16, 8, 4      # rows behind S_tgt in x (a sentinel) and in v: batch strides larger than S_tgt * C; guard rows
SENTINEL, GUARD_VALUE = -7.75, 3.25
STATE_GUARD = 4                     # floats in front of and behind the state: the smallest offset that keeps it 16-byte aligned
# S_tgt = 1: 8 vectors.  5: 40 vectors, no multiple of anything.  1024: 8192 vectors, 32 blocks.
# 131 096: 1 048 768 vectors, 192 past the first trip of a grid capped at 4096 blocks of 256 threads.
SHAPES = {"b1_s1": (1, 1), "b3_s1": (3, 1), "b1_s5": (1, 5), "b3_s5": (3, 5), "b1_s1024": (1, 1024), "b3_s1024": (3, 1024),
          "second_grid_stride_trip": (1, 131072 + 24)}
assert SHAPES["second_grid_stride_trip"][1] * C // 8 > 4096 * 256
SIG = R.schedule(28, 1024)
STEP = 13
COEF = {1: R.coefficients(SIG, STEP, True), 0: R.coefficients(SIG, STEP, False)}    # a real schedule's: no bf16 numbers
SN = float(SIG[STEP + 1])


def _data(B, Sz, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Sz + PAD_X, C, generator=g).to(BF)
    x[:, Sz:] = SENTINEL
    v = torch.randn(B, Sz + PAD_V, C, generator=g).mul(3).to(BF)
    h = torch.randn(B, Sz, C, generator=g).mul(3).to(BF)
    x0 = torch.randn(B, Sz, C, generator=g).mul(2).to(BF)
    noise = torch.randn(B, Sz, C, generator=g).to(BF)
    # a state some steps into a run: near x, and no bf16 number
    state = x[:, :Sz].float() + torch.randn(B, Sz, C, generator=g) * 2.0 ** -10
    return dict(x=x, v=v, h=h, x0=x0, noise=noise, state=state, B=B, S=Sz)


@pytest.fixture(scope="module")
def cases():
    """The inputs per shape, made once and never modified (the kernel works on device copies)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {name: _data(B, Sz, seed) for seed, (name, (B, Sz)) in enumerate(SHAPES.items())}
    d = out["b3_s1024"]
    assert not torch.equal(d["state"].to(BF).float(), d["state"]), "the state must not be bf16-representable"
    return out


def _mask(kind, Bm, Sz, seed=0):
    g = torch.Generator().manual_seed(seed + 100)
    if kind == "zeros":
        return torch.zeros(Bm, Sz, 4, dtype=BF)
    if kind == "ones":
        return torch.ones(Bm, Sz, 4, dtype=BF)
    if kind == "quarter":
        return torch.full((Bm, Sz, 4), 0.25, dtype=BF)
    return torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (Bm, Sz, 4), generator=g)].to(BF)   # mixed within a token


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _run(d, use_hist, load_state, hist="data", mask=None, sigma_next=0.0, coef=None):
    """One launch on fresh device copies; checks what every launch must leave alone and behind, returns (state, x[:, :S]) on
    the CPU.  ``hist``: "data" (the previous velocity), "nan" (a NaN-filled buffer) or None (no buffer).  With ``load_state`` 0
    the state buffer is NaN-filled."""
    from gpt_image_edit_amd import ops
    B, Sz = d["B"], d["S"]
    # x: sentinel rows around the whole buffer, and PAD_X rows behind every sample's target rows
    xbuf = torch.full((B * (Sz + PAD_X) + 2 * GUARD, C), GUARD_VALUE, dtype=BF).cuda()
    xd = xbuf[GUARD:GUARD + B * (Sz + PAD_X)].view(B, Sz + PAD_X, C)
    xd.copy_(d["x"])
    vd = d["v"].cuda()
    sbuf = torch.full((B * Sz * C + 2 * STATE_GUARD,), GUARD_VALUE, dtype=torch.float32).cuda()
    sd = sbuf[STATE_GUARD:STATE_GUARD + B * Sz * C].view(B, Sz, C)
    sd.copy_(d["state"] if load_state else torch.full((B, Sz, C), float("nan")))
    hbuf = hd = None
    if hist is not None:
        hbuf = torch.full((B, Sz + 2 * GUARD, C), GUARD_VALUE, dtype=BF).cuda()
        hd = hbuf[:, GUARD:GUARD + Sz]
        hd.copy_(d["h"] if hist == "data" else torch.full((B, Sz, C), float("nan"), dtype=BF))
    c_v, c_h, _ = coef or COEF[use_hist]
    if mask is None:
        ops.solver_step_f32(sd, xd, vd, Sz, c_v, c_h, use_hist, load_state, hd)
    else:
        ops.solver_step_f32(sd, xd, vd, Sz, c_v, c_h, use_hist, load_state, hd, sigma_next, d["x0"].cuda(), d["noise"].cuda(),
                            mask.cuda())
    xb, got_x, sb = xbuf.cpu(), xd.cpu(), sbuf.cpu()
    assert torch.equal(got_x[:, Sz:], d["x"][:, Sz:]), "rows behind S_tgt (the condition tokens) were written"
    assert bool((xb[:GUARD] == GUARD_VALUE).all()) and bool((xb[GUARD + B * (Sz + PAD_X):] == GUARD_VALUE).all()), "x guards"
    assert bool((sb[:STATE_GUARD] == GUARD_VALUE).all()) and bool((sb[-STATE_GUARD:] == GUARD_VALUE).all()), "state guards written"
    assert torch.equal(vd.cpu(), d["v"]), "v was written"
    if hist is not None:
        hb = hbuf.cpu()
        assert torch.equal(_bits(hb[:, GUARD:GUARD + Sz]), _bits(d["v"][:, :Sz])), "hist does not hold v's bits"
        assert bool((hb[:, :GUARD] == GUARD_VALUE).all()) and bool((hb[:, GUARD + Sz:] == GUARD_VALUE).all()), "hist guards"
    return sb[STATE_GUARD:STATE_GUARD + B * Sz * C].view(B, Sz, C).clone(), got_x[:, :Sz].contiguous()


def _ref(d, use_hist, load_state, m=None, sigma_next=0.0, coef=None):
    Sz = d["S"]
    xs = d["state"] if load_state else d["x"][:, :Sz].float()
    c_v, c_h, _ = coef or COEF[use_hist]
    return S.step(xs, d["v"][:, :Sz], d["h"], c_v, c_h, use_hist, sigma_next, d["x0"], d["noise"], m)


def _same(got, ref, what):
    state, x = got
    ds = int((_bits(state) != _bits(ref)).sum())
    dx = int((_bits(x) != _bits(ref.to(BF))).sum())
    print(f"[state step] {what}: {ds} state elements and {dx} token elements differ in bits", flush=True)
    assert ds == 0 and dx == 0, what
    assert torch.isfinite(state).all()


@pytest.mark.parametrize("load_state", [0, 1])
@pytest.mark.parametrize("use_hist", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_both_outputs_match_the_float32_expression(cases, name, use_hist, load_state):
    d = cases[name]
    assert all(c != float(torch.tensor(c).to(BF)) for c in COEF[1][:2])
    ref = _ref(d, use_hist, load_state)
    # AB2: a history buffer.  Euler (use_hist 0): none at all
    got = _run(d, use_hist, load_state, hist="data" if use_hist else None)
    _same(got, ref, f"{name} use_hist={use_hist} load_state={load_state}")
    assert not torch.equal(got[1], d["x"][:, :d["S"]])
    if use_hist:                                        # the history term is live
        assert not torch.equal(_bits(got[0]), _bits(_ref(d, 0, load_state)))
    if load_state:                                      # the carried state is live: seeding from x gives other bits
        assert not torch.equal(_bits(got[0]), _bits(_ref(d, use_hist, 0)))
    # determinism: a second launch on the same data gives the same bits
    again = _run(d, use_hist, load_state, hist="data" if use_hist else None)
    assert torch.equal(_bits(again[0]), _bits(got[0])) and torch.equal(_bits(again[1]), _bits(got[1]))


@pytest.mark.parametrize("load_state", [0, 1])
@pytest.mark.parametrize("name", ["b3_s5", "b1_s1024", "second_grid_stride_trip"])
def test_first_order_step_never_reads_the_history_and_still_writes_it(cases, name, load_state):
    d = cases[name]
    ref = _ref(d, 0, load_state)
    got = _run(d, 0, load_state, hist="nan")            # _run checks hist == v's bits afterwards
    _same(got, ref, f"{name} NaN history, load_state={load_state}")
    # ... and c_h is not applied there either
    other = _run(d, 0, load_state, hist="nan", coef=(COEF[0][0], COEF[1][1], 0))
    assert torch.equal(_bits(other[0]), _bits(got[0])) and torch.equal(_bits(other[1]), _bits(got[1]))


def test_unrounded_step_size_is_used(cases):
    """Euler on this entry takes ``dsigma`` as the float32 number it is: the result differs from the one a bf16-rounded step size
    gives, and equals the expression with the unrounded one (checked above)."""
    d = cases["b3_s1024"]
    dsig = float(np.float32(SIG[STEP + 1]) - np.float32(SIG[STEP]))
    rounded = float(torch.tensor(dsig).to(BF))
    assert dsig != rounded
    got = _run(d, 0, 1, hist=None, coef=(dsig, 0.0, 0))
    _same(got, _ref(d, 0, 1, coef=(dsig, 0.0, 0)), "euler, unrounded dsigma")
    assert not torch.equal(_bits(got[0]), _bits(_ref(d, 0, 1, coef=(rounded, 0.0, 0))))


@pytest.mark.parametrize("load_state", [0, 1])
@pytest.mark.parametrize("use_hist", [0, 1])
def test_mask_of_ones_is_the_unmasked_step_and_zeros_the_preserved_picture(cases, use_hist, load_state):
    for name in ("b3_s5", "b3_s1024"):
        d = cases[name]
        B, Sz = d["B"], d["S"]
        hist = "data" if use_hist else None
        plain = _run(d, use_hist, load_state, hist=hist)
        for Bm in (1, B):
            ones = _run(d, use_hist, load_state, hist=hist, mask=_mask("ones", Bm, Sz), sigma_next=SN)
            assert torch.equal(_bits(ones[0]), _bits(plain[0])) and torch.equal(_bits(ones[1]), _bits(plain[1]))
            zeros = _run(d, use_hist, load_state, hist=hist, mask=_mask("zeros", Bm, Sz), sigma_next=SN)
            k = torch.add(torch.mul(S.f32(SN), d["noise"].float()), torch.mul(S.f32(S.one_minus(SN)), d["x0"].float()))
            assert torch.equal(_bits(zeros[0]), _bits(k)) and torch.equal(_bits(zeros[1]), _bits(k.to(BF)))
            assert not torch.equal(k.to(BF), inpaint_ref.keep(d["x0"], d["noise"], SN))     # sigma_next is not rounded to bf16
            last = _run(d, use_hist, load_state, hist=hist, mask=_mask("zeros", Bm, Sz), sigma_next=0.0)
            assert torch.equal(_bits(last[1]), _bits(d["x0"])) and torch.equal(_bits(last[0]), _bits(d["x0"].float()))


@pytest.mark.parametrize("kind", ["quarter", "mixed"])
@pytest.mark.parametrize("name", ["b1_s1", "b3_s5", "b3_s1024", "second_grid_stride_trip"])
def test_soft_and_mixed_masks_match_the_same_expression(cases, name, kind):
    d = cases[name]
    B, Sz = d["B"], d["S"]
    for Bm in sorted({1, B}):
        for use_hist, load_state in ((1, 1), (0, 0)):
            mask = _mask(kind, Bm, Sz, 9 + Bm)
            ref = _ref(d, use_hist, load_state, inpaint_ref.expand_mask(mask, C), SN)
            got = _run(d, use_hist, load_state, hist="data" if use_hist else None, mask=mask, sigma_next=SN)
            _same(got, ref, f"{name} {kind} mask batch {Bm} use_hist={use_hist} load_state={load_state}")
            assert not torch.equal(_bits(got[0]), _bits(_ref(d, use_hist, load_state)))      # the mask is live


def test_refusals_are_errors_not_launches():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import libfk, ops
    lib = libfk.load()
    B, Sz = 1, 8
    n = B * Sz * C
    nan = float("nan")
    names = ("x", "v", "hist", "x0", "noise")
    flat = {k: torch.full((n + 16,), nan, device="cuda", dtype=BF) for k in names}          # NaN canaries: outputs and inputs
    sflat = torch.full((n + 16,), nan, device="cuda", dtype=torch.float32)
    mflat = torch.ones(Sz * 4 + 8, device="cuda", dtype=BF)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    c_v, c_h, _ = COEF[1]

    def call(off=None, null=(), alias=None, moff=0, mstride=0, mask=True, strides=None, b=B, s=Sz, c=C, use_hist=1, load_state=1,
             soff=0, sstride=n):
        off, strides = off or {}, strides or {}
        p = {k: (None if k in null else ctypes.c_void_p(flat[k].data_ptr() + 2 * off.get(k, 0))) for k in names}
        p["state"] = None if "state" in null else ctypes.c_void_p(sflat.data_ptr() + 4 * soff)
        if alias:
            p[alias[0]] = p[alias[1]]
        st = {k: strides.get(k, Sz * C) for k in names}
        m = ctypes.c_void_p(mflat.data_ptr() + 2 * moff) if mask else None
        return lib.fk_solver_step_f32(p["state"], sstride, p["x"], st["x"], p["v"], st["v"], p["hist"], st["hist"], p["x0"],
                                      st["x0"], p["noise"], st["noise"], m, mstride, b, s, c, c_v, c_h, use_hist, load_state,
                                      0.5, stream)
    bad = [dict(null=("state",)), dict(null=("x",)), dict(null=("v",)),
           dict(b=0), dict(s=0), dict(c=0), dict(b=-1), dict(s=-3), dict(c=-8), dict(c=12), dict(c=4),           # sizes, C % 8
           dict(off={"x": 4}), dict(off={"v": 4}), dict(off={"hist": 4}), dict(off={"x0": 4}), dict(off={"noise": 4}),  # 8 bytes
           dict(strides={"x": Sz * C + 4}), dict(strides={"v": Sz * C + 4}), dict(strides={"hist": Sz * C + 4}),
           dict(strides={"x0": Sz * C + 4}), dict(strides={"noise": Sz * C + 4}), dict(moff=2), dict(mstride=2),
           dict(soff=2), dict(soff=1), dict(sstride=n + 2), dict(sstride=n + 1),               # the state: 16 bytes, 4 elements
           dict(use_hist=2), dict(use_hist=-1), dict(use_hist=2, mask=False),
           dict(load_state=2), dict(load_state=-1), dict(load_state=2, mask=False),
           dict(null=("hist",)), dict(null=("hist",), mask=False),                             # use_hist = 1 without a buffer
           dict(alias=("hist", "v")), dict(alias=("hist", "v"), use_hist=0), dict(alias=("hist", "x")),
           dict(alias=("hist", "state")), dict(alias=("hist", "state"), use_hist=0),
           dict(alias=("state", "x")), dict(alias=("x", "state")),
           dict(null=("x0",)), dict(null=("noise",)), dict(null=("x0", "noise"))]              # a mask without x0 and noise
    for kw in bad:
        assert call(**kw) == -1, kw                       # FK_EINVAL
        assert "fk_solver_step_f32" in lib.fk_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in flat.values()) and bool(torch.isnan(sflat).all()), "a refused call wrote something"
    # the calls next to the refused ones are taken
    for t in list(flat.values()) + [sflat]:
        t.fill_(1.5)
    assert call(moff=4) == 0                            # the mask needs 8 bytes only
    assert call(mask=False, null=("x0", "noise")) == 0  # no mask: x0 and noise are not needed
    assert call(null=("hist",), use_hist=0) == 0        # Euler: no history buffer
    assert call(soff=4, sstride=n + 4) == 0             # the state's own batch stride
    assert call() == 0 and call(use_hist=0) == 0 and call(load_state=0) == 0
    torch.cuda.synchronize()
    assert bool((flat["hist"][:n] == 1.5).all()) and bool((flat["v"] == 1.5).all()) and not bool((flat["x"][:n] == 1.5).all())
    assert bool((flat["x"][n:] == 1.5).all()) and bool((flat["hist"][n:] == 1.5).all()) and bool((sflat[n + 4:] == 1.5).all())
    assert not bool((sflat[:n] == 1.5).all())
    # through ops the error is an exception that names the entry point, and shapes are checked before the library is called
    z = lambda *s: torch.zeros(*s, device="cuda", dtype=BF)  # noqa: E731
    f = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.float32)  # noqa: E731
    with pytest.raises(RuntimeError, match="fk_solver_step_f32"):
        ops.solver_step_f32(f(1, 8, 12), z(1, 8, 12), z(1, 8, 12), 8, c_v)
    with pytest.raises(RuntimeError, match="fk_solver_step_f32"):
        ops.solver_step_f32(f(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v, c_h, 2, 1, z(1, 8, C))
    with pytest.raises(RuntimeError, match="fk_solver_step_f32"):
        ops.solver_step_f32(f(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v, c_h, 1, 1, None)
    with pytest.raises(RuntimeError, match="fk_solver_step_f32"):
        ops.solver_step_f32(f(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v, load_state=3)
    with pytest.raises(ValueError, match="state"):
        ops.solver_step_f32(z(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v)                   # a bf16 state
    with pytest.raises(ValueError, match="state"):
        ops.solver_step_f32(f(1, 4, C), z(1, 8, C), z(1, 8, C), 8, c_v)
    with pytest.raises(ValueError, match="hist"):
        ops.solver_step_f32(f(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v, c_h, 1, 1, z(1, 4, C))
    with pytest.raises(ValueError, match="mask"):
        ops.solver_step_f32(f(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v, c_h, 1, 1, z(1, 8, C), 0.5, z(1, 8, C), z(1, 8, C),
                            z(1, 8, 8))
    torch.cuda.synchronize()
