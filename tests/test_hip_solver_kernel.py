"""GPU: ``fk_ab2_step_bf16`` against the op-by-op float32 torch expression of the step on the CPU (``solver_ref``, pinned by
``test_solver_ref.py``) at 0 ulp -- every product and every sum of the update is one float32 operation and the result is rounded
to bf16 once, so the expression is exactly restatable.  Shapes and sentinel layout are those of ``test_hip_inpaint_kernels.py``."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref  # noqa: E402
import solver_ref as R  # noqa: E402
from conftest import bf16_ulp_diff  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C = 64
PAD_X, PAD_V, GUARD = 16, 8, 4      # rows behind S_tgt in x (a sentinel), v's own batch stride, guard rows around hist
SENTINEL, GUARD_VALUE = -7.75, 3.25
# S_tgt = 24: 192 vectors, less than one block.  100: 800 vectors, 4 blocks, the last one partial.
# 131 096: 1 048 768 vectors, 192 past the first trip of a grid capped at 4096 blocks of 256 threads.
SHAPES = {"one_partial_block": (2, 24), "four_blocks": (2, 100), "second_grid_stride_trip": (1, 131072 + 24)}
SIG = R.schedule(28, 1024)
STEP = 13
COEF = {1: R.coefficients(SIG, STEP, True), 0: R.coefficients(SIG, STEP, False)}    # a real schedule's: no bf16 numbers


def _data(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S + PAD_X, C, generator=g).to(BF)
    x[:, S:] = SENTINEL
    v = torch.randn(B, S + PAD_V, C, generator=g).mul(3).to(BF)
    h = torch.randn(B, S, C, generator=g).mul(3).to(BF)
    x0 = torch.randn(B, S, C, generator=g).mul(2).to(BF)
    noise = torch.randn(B, S, C, generator=g).to(BF)
    return x, v, h, x0, noise


def _mask(kind, Bm, S, seed):
    g = torch.Generator().manual_seed(seed + 100)
    if kind == "zeros":
        return torch.zeros(Bm, S, 4, dtype=BF)
    if kind == "ones":
        return torch.ones(Bm, S, 4, dtype=BF)
    if kind == "soft":
        return torch.rand(Bm, S, 4, generator=g).to(BF)
    m = (torch.rand(Bm, S, 4, generator=g) < 0.5).to(BF)       # mixed within a token
    m[:, 0], m[:, 1], m[:, 2] = 0, 1, torch.tensor([1.0, 0.0, 0.0, 1.0]).to(BF)
    return m


@pytest.fixture(scope="module")
def cases():
    """(x, v, h, x0, noise) per shape, made once and never modified (the kernel works on device copies)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return {name: _data(B, S, seed) for seed, (name, (B, S)) in enumerate(SHAPES.items())}


def _guarded_hist(h, fill=None):
    """hist as rows [GUARD, GUARD + S) of a larger buffer per sample (its own batch stride), guard rows on both sides."""
    B, S, _ = h.shape
    buf = torch.full((B, S + 2 * GUARD, C), GUARD_VALUE, dtype=BF).cuda()
    view = buf[:, GUARD:GUARD + S]
    if fill is None:
        view.copy_(h)
    else:
        view.copy_(fill)
    return buf, view


def _run(data, S, use_hist, mask=None, sigma_next=0.0, hist_fill=None):
    """One launch; checks what every launch must leave alone and behind, returns the new x[:, :S] on the CPU."""
    from gpt_image_edit_amd import ops
    x, v, h, x0, noise = data
    xd, vd = x.cuda(), v.cuda()
    buf, hist = _guarded_hist(h, hist_fill)
    c_v, c_h, _ = COEF[use_hist]
    if mask is None:
        ops.ab2_step(xd, vd, hist, S, c_v, c_h, use_hist)
    else:
        ops.ab2_step(xd, vd, hist, S, c_v, c_h, use_hist, sigma_next, x0.cuda(), noise.cuda(), mask.cuda())
    got, hb = xd.cpu(), buf.cpu()
    assert torch.equal(got[:, S:], x[:, S:]), "rows behind S_tgt (the condition tokens) were written"
    assert torch.equal(hb[:, GUARD:GUARD + S].view(torch.int16), v[:, :S].view(torch.int16)), "hist does not hold v's bits"
    assert bool((hb[:, :GUARD] == GUARD_VALUE).all()) and bool((hb[:, GUARD + S:] == GUARD_VALUE).all()), "guard rows written"
    assert torch.equal(vd.cpu(), v), "v was written"
    return got[:, :S]


def _ref(data, S, use_hist, m=None, sigma_next=0.0):
    x, v, h, x0, noise = data
    c_v, c_h, _ = COEF[use_hist]
    return R.step(x[:, :S], v[:, :S], h, c_v, c_h, use_hist, sigma_next, x0, noise, m)


@pytest.mark.parametrize("use_hist", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_update_matches_the_float32_expression(cases, name, use_hist):
    B, S = SHAPES[name]
    assert COEF[1][0] != float(torch.tensor(COEF[1][0]).to(BF)) and COEF[1][1] != float(torch.tensor(COEF[1][1]).to(BF))
    got, ref = _run(cases[name], S, use_hist), _ref(cases[name], S, use_hist)
    d = bf16_ulp_diff(got, ref).max().item()
    print(f"[ab2] S_tgt={S} use_hist={use_hist}: max ulp {d}", flush=True)
    assert d == 0
    assert torch.isfinite(got.float()).all() and not torch.equal(got, cases[name][0][:, :S])
    if use_hist:                                        # the history term is live
        assert not torch.equal(got, _ref(cases[name], S, 0))
    # determinism: a second launch on the same data gives the same bits
    assert torch.equal(got, _run(cases[name], S, use_hist))


@pytest.mark.parametrize("name", ["one_partial_block", "second_grid_stride_trip"])
def test_first_step_never_reads_the_history(cases, name):
    B, S = SHAPES[name]
    nan = torch.full((B, S, C), float("nan"), dtype=BF)
    got = _run(cases[name], S, 0, hist_fill=nan)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, _ref(cases[name], S, 0))
    # ... and c_h is not applied there either: the result is the c_h = 0 one whatever c_h is handed over
    from gpt_image_edit_amd import ops
    x, v, h, _, _ = cases[name]
    a, b = x.cuda(), x.cuda()
    ops.ab2_step(a, v.cuda(), nan.cuda(), S, COEF[0][0], 0.0, 0)
    ops.ab2_step(b, v.cuda(), nan.cuda(), S, COEF[0][0], COEF[1][1], 0)
    assert torch.equal(a, b) and torch.equal(a[:, :S].cpu(), got)


@pytest.mark.parametrize("use_hist", [0, 1])
def test_mask_of_ones_is_the_unmasked_step(cases, use_hist):
    for name in ("one_partial_block", "four_blocks"):
        B, S = SHAPES[name]
        plain = _run(cases[name], S, use_hist)
        assert torch.equal(_run(cases[name], S, use_hist, _mask("ones", 1, S, 0), 0.7311), plain)
        assert torch.equal(_run(cases[name], S, use_hist, _mask("ones", B, S, 0), 0.0), plain)


@pytest.mark.parametrize("sigma_next", [0.0, 0.7311, 1.0])
def test_mask_of_zeros_is_the_preserved_picture(cases, sigma_next):
    B, S = SHAPES["one_partial_block"]
    x, v, h, x0, noise = cases["one_partial_block"]
    for use_hist in (0, 1):
        got = _run(cases["one_partial_block"], S, use_hist, _mask("zeros", 1, S, 0), sigma_next)
        assert torch.equal(got, inpaint_ref.keep(x0, noise, sigma_next))
        if sigma_next == 0.0:
            assert torch.equal(got, x0)


@pytest.mark.parametrize("kind", ["mixed", "soft"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_and_soft_masks_match_the_composed_formula(cases, name, kind):
    B, S = SHAPES[name]
    for mask_batch in sorted({1, B}):
        for use_hist in (0, 1):
            mask = _mask(kind, mask_batch, S, 9 + mask_batch)
            got = _run(cases[name], S, use_hist, mask, 0.7311)
            ref = _ref(cases[name], S, use_hist, inpaint_ref.expand_mask(mask, C), 0.7311)
            d = bf16_ulp_diff(got, ref).max().item()
            print(f"[ab2 + mask] S_tgt={S} {kind} mask batch {mask_batch} use_hist={use_hist}: max ulp {d}", flush=True)
            assert d == 0
            if kind == "mixed":      # token 0 is kept, token 1 is the update
                x, v, h, x0, noise = cases[name]
                assert torch.equal(got[:, 0], inpaint_ref.keep(x0, noise, 0.7311)[:, 0])
                assert torch.equal(got[:, 1], _ref(cases[name], S, use_hist)[:, 1])


def test_refusals_are_errors_not_launches():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import libfk, ops
    lib = libfk.load()
    B, S = 1, 8
    n = B * S * C
    names = ("x", "v", "hist", "x0", "noise")
    flat = {k: torch.full((n + 16,), 1.5, device="cuda", dtype=BF) for k in names}
    mflat = torch.ones(S * 4 + 8, device="cuda", dtype=BF)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    c_v, c_h, _ = COEF[1]

    def call(off=None, null=(), alias=None, moff=0, mstride=0, mask=True, strides=None, b=B, s=S, c=C, use_hist=1):
        off, strides = off or {}, strides or {}
        p = {k: (None if k in null else ctypes.c_void_p(flat[k].data_ptr() + 2 * off.get(k, 0))) for k in names}
        if alias:
            p[alias[0]] = p[alias[1]]
        st = {k: strides.get(k, S * C) for k in names}
        m = ctypes.c_void_p(mflat.data_ptr() + 2 * moff) if mask else None
        return lib.fk_ab2_step_bf16(p["x"], st["x"], p["v"], st["v"], p["hist"], st["hist"], p["x0"], st["x0"], p["noise"],
                                    st["noise"], m, mstride, b, s, c, c_v, c_h, use_hist, 0.5, stream)
    bad = [dict(null=("x",)), dict(null=("v",)), dict(null=("hist",)), dict(null=("hist",), mask=False),
           dict(alias=("hist", "v")), dict(alias=("hist", "v"), use_hist=0), dict(alias=("hist", "x")),
           dict(b=0), dict(s=0), dict(c=0), dict(b=-1), dict(s=-3), dict(c=-8), dict(c=12), dict(c=4),
           dict(off={"x": 4}), dict(off={"v": 4}), dict(off={"hist": 4}), dict(off={"x0": 4}), dict(off={"noise": 4}),  # 8 bytes
           dict(strides={"x": S * C + 4}), dict(strides={"v": S * C + 4}), dict(strides={"hist": S * C + 4}),
           dict(strides={"x0": S * C + 4}), dict(strides={"noise": S * C + 4}), dict(moff=2), dict(mstride=2),
           dict(use_hist=2), dict(use_hist=-1), dict(use_hist=2, mask=False),
           dict(null=("x0",)), dict(null=("noise",)), dict(null=("x0", "noise"))]                  # a mask without x0 and noise
    for kw in bad:
        assert call(**kw) == -1, kw                       # FK_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == 1.5).all()) for t in flat.values()), "a refused call wrote something"
    assert call(moff=4) == 0                            # the mask needs 8 bytes only
    assert call(mask=False, null=("x0", "noise")) == 0  # no mask: x0 and noise are not needed
    assert call() == 0 and call(use_hist=0) == 0
    torch.cuda.synchronize()
    assert bool((flat["hist"][:n] == 1.5).all()) and bool((flat["v"] == 1.5).all()) and not bool((flat["x"][:n] == 1.5).all())
    assert bool((flat["x"][n:] == 1.5).all()) and bool((flat["hist"][n:] == 1.5).all())
    # through ops the error is an exception that names the entry point, and shapes are checked before the library is called
    z = lambda *s: torch.zeros(*s, device="cuda", dtype=BF)  # noqa: E731
    with pytest.raises(RuntimeError, match="fk_ab2_step_bf16"):
        ops.ab2_step(z(1, 8, 12), z(1, 8, 12), z(1, 8, 12), 8, c_v, c_h, 1)
    with pytest.raises(RuntimeError, match="fk_ab2_step_bf16"):
        ops.ab2_step(z(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v, c_h, 2)
    with pytest.raises(ValueError, match="hist"):
        ops.ab2_step(z(1, 8, C), z(1, 8, C), z(1, 4, C), 8, c_v, c_h, 1)
    with pytest.raises(ValueError, match="mask"):
        ops.ab2_step(z(1, 8, C), z(1, 8, C), z(1, 8, C), 8, c_v, c_h, 1, 0.5, z(1, 8, C), z(1, 8, C), z(1, 8, 8))
    torch.cuda.synchronize()
