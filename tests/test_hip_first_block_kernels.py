"""GPU: the first-block measure kernel (csrc/step_cache.hip, fk_residual_absdiff_sums_bf16) through
``ops.residual_absdiff_sums``.

``out`` is specified twice over: it holds the bits of ``ops.residual_save`` followed by ``ops.absdiff_sums`` (same decomposition,
same order), and it lies inside the bound tests/step_cache_ref.py derives from that order, around fp64 on the exactly defined
r = bf16(h1 - h0) (tests/first_block_ref.py).  ``r_out`` is held to 0 ulp against the torch expression.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import first_block_ref as F  # noqa: E402
import step_cache_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = 12345.0


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops
    return ops


def _guarded_f32(n, pad=64):
    buf = torch.full((n + 2 * pad,), SENT, device="cuda", dtype=torch.float32)
    return buf, buf[pad:pad + n]


def _guards_ok(buf, n, pad=64):
    return bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all())


def _bits(t):
    return t.view(torch.int32)


def _measure(ops, h1, h0, ref, r_out=None):
    """One launch with sentinels around out and the workspace; a second one must give the same bits."""
    from gpt_image_edit_amd import libfk
    nws = libfk.load().fk_absdiff_ws_floats()
    obuf, out = _guarded_f32(2)
    wbuf, ws = _guarded_f32(nws)
    ops.residual_absdiff_sums(h1, h0, ref, r_out=r_out, out=out, ws=ws)
    first = out.clone()
    ops.residual_absdiff_sums(h1, h0, ref, r_out=r_out, out=out, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(_bits(first), _bits(out)), "two launches differ"
    assert _guards_ok(obuf, 2) and _guards_ok(wbuf, nws), "a sentinel word was written"
    lay = R.layout(h1.numel() // h1.shape[-1], h1.shape[-1])
    assert bool((ws[2 * lay["nblk"]:] == SENT).all()), "the workspace was written past the launch's partials"
    return first.cpu()


def _two_launches(ops, h1, h0, ref):
    """The composition the kernel replaces: residual_save, then absdiff_sums."""
    r = torch.empty(h1.shape, dtype=BF, device="cuda")
    ops.residual_save(h1, h0, r)
    return ops.absdiff_sums(r, ref).cpu(), r


def _padded(t, ld, fill=SENT):
    """t [B, R, D] as the [:, 1:-1, :D] view of a [B, R + 2, ld] buffer of sentinels (a sentinel row either side, row padding)."""
    B, Rr, D = t.shape
    buf = torch.full((B, Rr + 2, ld), fill, dtype=BF, device="cuda")
    v = buf[:, 1:Rr + 1, :D]
    v.copy_(t)
    return buf, v


def _outside_intact(buf, v_shape):
    B, Rr, D = v_shape
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:, 1:Rr + 1, :D] = False
    return bool((buf[keep] == SENT).all())


def _full_check(ops, name, h1, h0, ref, ld):
    """h1, h0, ref: CPU bf16 [B, R, D].  Runs on views with row stride ld; returns out (CPU)."""
    B, Rr, D = h1.shape
    (_, v1), (_, v0), (_, vr) = (_padded(t.cuda(), ld, 3.0) for t in (h1, h0, ref))
    rbuf, r_out = _padded(torch.zeros(B, Rr, D, dtype=BF), ld)
    r_out.fill_(SENT)
    got = _measure(ops, v1, v0, vr, r_out=r_out)
    # r_out: 0 ulp against the torch expression, nothing around it written
    assert torch.equal(r_out.cpu(), F.residual(h1, h0)), f"{name}: r_out"
    assert _outside_intact(rbuf, (B, Rr, D)), f"{name}: written outside r_out's rows / columns"
    # the two-launch composition's bits, with and without r_out
    want, _ = _two_launches(ops, v1, v0, vr)
    assert torch.equal(_bits(got), _bits(want)), f"{name}: {got.tolist()} != two launches {want.tolist()}"
    assert torch.equal(_bits(_measure(ops, v1, v0, vr)), _bits(got)), f"{name}: r_out=None changes out"
    # inside the derived bound of fp64, and the emulated order's bits
    F.check(name, got.tolist(), h1, h0, ref)
    e0, e1 = F.emulate(h1, h0, ref)
    assert got[0].item() == float(e0) and got[1].item() == float(e1)
    return got


# B, R, D, ld
CASES = [(1, 1, 1, 1), (1, 3, 7, 7), (2, 5, 8, 8), (1, 2, 13, 13), (2, 4, 64, 64), (1, 5, 3072, 3072), (2, 5, 3075, 3080)]


@pytest.mark.parametrize("B,Rr,D,ld", CASES)
def test_out_is_the_two_launch_composition_inside_the_bound(ops, B, Rr, D, ld):
    h1, h0, ref = F.data((B, Rr, D), seed=B * 1000 + Rr + D)
    _full_check(ops, f"residual_absdiff_sums {B}x{Rr}x{D} ld={ld}", h1, h0, ref, ld)


@pytest.mark.parametrize("D", [64, 3072])
def test_image_rows_of_a_joint_buffer(ops, D):
    B, S_txt, S_img = 2, 3, 5
    h1, h0, ref = F.data((B, S_img, D), seed=D)
    js = torch.full((B, S_txt + S_img, D), 7.0, dtype=BF, device="cuda")        # the workspace stream: text rows hold 7
    h = js[:, S_txt:]
    h.copy_(h1.cuda())
    assert h.stride(0) != S_img * h.stride(1)
    cur = torch.full((B, S_img + 1, D), SENT, dtype=BF, device="cuda")
    got = _measure(ops, h, h0.cuda(), ref.cuda(), r_out=cur[:, :S_img])
    F.check(f"joint buffer D={D}", got.tolist(), h1, h0, ref)
    want, r = _two_launches(ops, h, h0.cuda(), ref.cuda())
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(cur[:, :S_img], r) and torch.equal(r.cpu(), F.residual(h1, h0)) and bool((cur[:, S_img] == SENT).all())
    assert bool((js[:, :S_txt] == 7.0).all()) and torch.equal(h.cpu(), h1)
    # a view measures as its contiguous copy does
    assert torch.equal(_bits(got), _bits(_measure(ops, h1.cuda(), h0.cuda(), ref.cuda())))


def test_past_one_trip_and_one_block_of_partials(ops):
    B, Rr, D = 2, R.ONE_TRIP_ITEMS // 16 + 350, 64           # 8 items per row: 5600 items past the first trip
    lay = R.layout(B * Rr, D)
    assert lay["iters"] == 2 and lay["nblk"] == R.MAX_BLOCKS > R.THREADS
    h1, h0, ref = F.data((B, Rr, D), seed=77)
    d1, d0, dr = h1.cuda(), h0.cuda(), ref.cuda()
    r_out = torch.full((B, Rr + 1, D), SENT, dtype=BF, device="cuda")
    got = _measure(ops, d1, d0, dr, r_out=r_out[:, :Rr])
    F.check("residual_absdiff_sums second trip", got.tolist(), h1, h0, ref)
    want, r = _two_launches(ops, d1, d0, dr)
    assert torch.equal(_bits(got), _bits(want))
    assert torch.equal(r_out[:, :Rr], r) and torch.equal(r.cpu(), F.residual(h1, h0)) and bool((r_out[:, Rr] == SENT).all())
    e0, e1 = F.emulate(h1, h0, ref)
    assert got[0].item() == float(e0) and got[1].item() == float(e1)


@pytest.mark.parametrize("B,Rr,D", [(2, 5, 64), (1, 5, 3072), (2, 3, 13)])
def test_an_unaligned_view_gives_the_aligned_views_bits(ops, B, Rr, D):
    h1, h0, ref = F.data((B, Rr, D), seed=D + 5)
    aligned = _measure(ops, h1.cuda(), h0.cuda(), ref.cuda())

    def odd(t):      # the same values one element (2 bytes) off a 16-byte boundary
        flat = torch.full((t.numel() + 9,), SENT, dtype=BF, device="cuda")
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 2
        return flat, v

    (_, o1), (_, o0), (_, orf) = odd(h1), odd(h0), odd(ref)
    rflat, r_out = odd(torch.zeros(B, Rr, D, dtype=BF))
    for views in ((o1, h0.cuda(), ref.cuda()), (h1.cuda(), o0, ref.cuda()), (h1.cuda(), h0.cuda(), orf), (o1, o0, orf)):
        assert torch.equal(_bits(_measure(ops, *views)), _bits(aligned))
    got = _measure(ops, h1.cuda(), h0.cuda(), ref.cuda(), r_out=r_out)          # only r_out unaligned
    assert torch.equal(_bits(got), _bits(aligned)) and torch.equal(r_out.cpu(), F.residual(h1, h0))
    assert bool((rflat[:1] == SENT).all()) and bool((rflat[1 + r_out.numel():] == SENT).all())


def test_exact_zeros(ops):
    h1, h0, ref = F.data((2, 5, 3075), seed=5)
    r_out = torch.full((2, 5, 3075), SENT, dtype=BF, device="cuda")
    got = _measure(ops, h1.cuda(), h1.cuda().clone(), torch.zeros_like(ref).cuda(), r_out=r_out)
    assert got.tolist() == [0.0, 0.0] and bool((r_out == 0).all())
    got = _measure(ops, h1.cuda(), h0.cuda(), torch.zeros_like(ref).cuda())
    assert got[1].item() == 0.0 and got[0].item() > 0          # a zero denominator: StepCache.rel_of makes it inf
    r = F.residual(h1, h0)
    got = _measure(ops, h1.cuda(), h0.cuda(), r.cuda())
    assert got[0].item() == 0.0 and got[1].item() > 0


# ---- refused arguments ----------------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(ops):
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    h1c, h0c, refc = F.data((2, 8, 64), seed=1)
    h1, h0, ref = h1c.cuda(), h0c.cuda(), refc.cuda()
    obuf, out = _guarded_f32(2)
    ws = ops.absdiff_ws("cuda")
    ws.fill_(SENT)
    r = torch.full((2, 8, 64), SENT, dtype=BF, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = libfk.Rows(64, 8, 512)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    null = ctypes.c_void_p(0)
    EINVAL, EUNSUP = -1, -2
    fn = lib.fk_residual_absdiff_sums_bf16
    n = ws.numel()

    def call(a=None, ra=rows, b=None, rb=rows, c=None, rc=rows, o=None, ro=rows, M=16, D=64, bf=1, out_=None, ws_=None, nws=n):
        return fn(p(h1) if a is None else a, ra, p(h0) if b is None else b, rb, p(ref) if c is None else c, rc,
                  p(r) if o is None else o, ro, M, D, bf, p(out) if out_ is None else out_, p(ws) if ws_ is None else ws_, nws, st)

    assert call(a=null) == EINVAL and call(b=null) == EINVAL and call(c=null) == EINVAL
    assert call(out_=null) == EINVAL and call(ws_=null) == EINVAL
    assert call(M=0) == EINVAL and call(D=0) == EINVAL
    for which in ("ra", "rb", "rc", "ro"):
        assert call(**{which: libfk.Rows(63, 8, 512)}) == EINVAL                   # ld < D
        assert call(**{which: libfk.Rows(64, 8, -512)}) == EINVAL                  # a negative batch stride
    assert call(nws=1) == EINVAL                                                   # workspace too small
    assert call(bf=0) == EUNSUP                                                    # not bf16
    assert b"bf16" in lib.fk_last_error()
    assert call(o=p(h1)) == EINVAL and call(o=p(h0)) == EINVAL and call(o=p(ref)) == EINVAL      # r_out is an input
    big = torch.full((3, 8, 64), SENT, dtype=BF, device="cuda")                    # ... or overlaps one: batches 0-1 and 1-2 of `big`
    assert call(c=p(big), o=ctypes.c_void_p(big.data_ptr() + 512 * 2)) == EINVAL
    assert call(a=ctypes.c_void_p(big.data_ptr() + 512 * 2), o=p(big)) == EINVAL
    assert bool((big == SENT).all())
    assert call(ro=libfk.Rows(64, 8, 256)) == EINVAL                               # r_out's rows overlap
    torch.cuda.synchronize()
    assert torch.equal(h1.cpu(), h1c) and torch.equal(h0.cpu(), h0c) and torch.equal(ref.cpu(), refc) and bool((r == SENT).all())
    assert bool((obuf == SENT).all()) and bool((ws == SENT).all())
    # a NULL r_out is no refusal, and its fk_rows is not looked at
    assert call(o=null, ro=libfk.Rows(0, 0, 0)) == 0
    torch.cuda.synchronize()
    assert bool((r == SENT).all()) and out[1].item() > 0
    # the wrapper: other dtypes and shapes
    with pytest.raises(RuntimeError, match="bf16"):
        ops.residual_absdiff_sums(h1.float(), h0.float(), ref.float())
    with pytest.raises(ValueError):
        ops.residual_absdiff_sums(h1, h0[:, :4], ref)
    with pytest.raises(ValueError):
        ops.residual_absdiff_sums(h1, h0, ref, r_out=r[:, :4])
    with pytest.raises(ValueError):
        ops.residual_absdiff_sums(h1.transpose(1, 2), h0.transpose(1, 2), ref.transpose(1, 2))
