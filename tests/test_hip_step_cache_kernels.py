"""GPU: the three step-cache kernels (csrc/step_cache.hip) through ``ops``.

The sums are held to fp64 within the bound tests/step_cache_ref.py derives from the summation order (nothing in it comes from
the kernel); save / apply are specified exactly and held to 0 ulp against the torch formula.

Observed / bound ratios of the sums on an MI355X (``-s`` prints them): unmeasured -- see the pull request's summary.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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
    """An fp32 [n] view with `pad` sentinel words either side."""
    buf = torch.full((n + 2 * pad,), SENT, device="cuda", dtype=torch.float32)
    return buf, buf[pad:pad + n]


def _guards_ok(buf, n, pad=64):
    return bool((buf[:pad] == SENT).all()) and bool((buf[pad + n:] == SENT).all())


def _sums(ops, a, b):
    """One launch with sentinels around out and the workspace; a second one must give the same bits."""
    from gpt_image_edit_amd import libfk
    nws = libfk.load().fk_absdiff_ws_floats()
    obuf, out = _guarded_f32(2)
    wbuf, ws = _guarded_f32(nws)
    ops.absdiff_sums(a, b, out=out, ws=ws)
    first = out.clone()
    ops.absdiff_sums(a, b, out=out, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), out.view(torch.int32)), "two launches differ"
    assert _guards_ok(obuf, 2) and _guards_ok(wbuf, nws), "a sentinel word was written"
    lay = R.layout(a.numel() // a.shape[-1], a.shape[-1])
    assert bool((ws[2 * lay["nblk"]:] == SENT).all()), "the workspace was written past the launch's partials"
    return first.cpu()


# B, R, D: one element; D = 64 / 3072 / 3080 with R around 64; a cut last chunk (D % 8 = 3); an unaligned row stride (ld = 67)
CASES = [(1, 1, 1), (2, 63, 64), (1, 64, 64), (2, 65, 64), (1, 63, 3072), (2, 64, 3072), (1, 65, 3080), (2, 64, 3080),
         (2, 65, 3075), (3, 63, 67)]


@pytest.mark.parametrize("B,Rr,D", CASES)
def test_sums_against_fp64(ops, B, Rr, D):
    a, b = R.data((B, Rr, D), seed=B * 1000 + Rr + D)
    got = _sums(ops, a.cuda(), b.cuda())
    R.check(f"absdiff_sums {B}x{Rr}x{D}", got.tolist(), a, b)
    e0, e1 = R.emulate(a, b)          # the emulated order is the kernel's: same bits (a statement about the order, not the bound)
    assert got[0].item() == float(e0) and got[1].item() == float(e1)


def test_sums_past_one_trip_and_one_block_of_partials(ops):
    Rr = R.ONE_TRIP_ITEMS // 8 // 2 + 350            # B = 2, D = 64: 8 items per row, 5600 items past the first trip
    a, b = R.data((2, Rr, 64), seed=77)
    lay = R.layout(2 * Rr, 64)
    assert lay["iters"] == 2 and lay["nblk"] == R.MAX_BLOCKS > R.THREADS
    got = _sums(ops, a.cuda(), b.cuda())
    R.check("absdiff_sums second trip", got.tolist(), a, b)
    e0, e1 = R.emulate(a, b)
    assert got[0].item() == float(e0) and got[1].item() == float(e1)


@pytest.mark.parametrize("D,ld", [(3072, 3072), (64, 64), (3075, 3080)])
def test_sums_on_batch_strided_views_with_a_text_offset(ops, D, ld):
    B, S_txt, S_img = 2, 5, 65
    a, b = R.data((B, S_img, D), seed=D)
    ja = torch.full((B, S_txt + S_img, ld), 7.0, dtype=BF).cuda()      # the joint buffers: text rows and row padding hold 7
    jb = torch.full((B, S_txt + S_img, ld), -3.0, dtype=BF).cuda()
    va, vb = ja[:, S_txt:, :D], jb[:, S_txt:, :D]
    va.copy_(a.cuda()), vb.copy_(b.cuda())
    assert va.stride(0) != S_img * va.stride(1)
    got = _sums(ops, va, vb)
    R.check(f"absdiff_sums strided D={D}", got.tolist(), a, b)
    assert torch.equal(got, _sums(ops, a.cuda(), b.cuda())), "a view sums as its contiguous copy does"
    # one strided, one contiguous
    assert torch.equal(got, _sums(ops, va, b.cuda()))


def test_exact_zeros(ops):
    a, b = R.data((2, 65, 3080), seed=5)
    got = _sums(ops, b.cuda(), b.cuda())
    assert got[0].item() == 0.0 and got[1].item() > 0
    got = _sums(ops, a.cuda(), torch.zeros_like(b).cuda())
    assert got[1].item() == 0.0 and got[0].item() > 0


# ---- save / apply ---------------------------------------------------------------------------------------------------------
def _joint(B, S_txt, S_img, ld, fill):
    return torch.full((B, S_txt + S_img + 1, ld), fill, dtype=BF, device="cuda")     # one sentinel row behind the image rows


EW_CASES = [(1, 1, 1, 1), (2, 65, 3072, 3072), (2, 63, 3075, 3080), (3, 64, 67, 67), (2, 64, 64, 64)]


@pytest.mark.parametrize("B,S_img,D,ld", EW_CASES)
def test_save_and_apply_are_exact_on_strided_views(ops, B, S_img, D, ld):
    S_txt = 3
    g = torch.Generator().manual_seed(B + S_img + D)
    h_out = torch.randn(B, S_img, D, generator=g).to(BF).cuda()
    h0 = (torch.randn(B, S_img, D, generator=g) * 0.7).to(BF).cuda()
    js = _joint(B, S_txt, S_img, ld, SENT)                 # the residual stream: h_out lives in its image rows
    h = js[:, S_txt:S_txt + S_img, :D]
    h.copy_(h_out)
    r = torch.full((B, S_img + 1, D), SENT, dtype=BF, device="cuda")
    ops.residual_save(h, h0, r[:, :S_img])
    want_r = (h_out.float() - h0.float()).to(BF)
    assert torch.equal(r[:, :S_img], want_r) and bool((r[:, S_img] == SENT).all())
    before = js.clone()
    # apply into the stream: out = h0 + r, text rows, the sentinel row and the row padding untouched
    ops.residual_apply(h0, r[:, :S_img], out=h)
    want = (h0.float() + want_r.float()).to(BF)
    assert torch.equal(h, want)
    keep = torch.ones_like(js, dtype=torch.bool)
    keep[:, S_txt:S_txt + S_img, :D] = False
    assert torch.equal(js[keep], before[keep])
    # out aliasing h0
    h0c = h0.clone()
    ops.residual_apply(h0c, r[:, :S_img], out=h0c)
    assert torch.equal(h0c, want)


def test_save_and_apply_second_trip(ops):
    B, S_img, D = 2, R.ONE_TRIP_ITEMS // 8 // 2 + 350, 64
    g = torch.Generator().manual_seed(9)
    h_out = torch.randn(B, S_img, D, generator=g).to(BF).cuda()
    h0 = torch.randn(B, S_img, D, generator=g).to(BF).cuda()
    r = torch.full((B, S_img + 1, D), SENT, dtype=BF, device="cuda")
    ops.residual_save(h_out, h0, r[:, :S_img])
    want_r = (h_out.float() - h0.float()).to(BF)
    assert torch.equal(r[:, :S_img], want_r) and bool((r[:, S_img] == SENT).all())
    out = torch.full((B, S_img + 1, D), SENT, dtype=BF, device="cuda")
    ops.residual_apply(h0, r[:, :S_img], out=out[:, :S_img])
    assert torch.equal(out[:, :S_img], (h0.float() + want_r.float()).to(BF)) and bool((out[:, S_img] == SENT).all())


# ---- refused arguments ----------------------------------------------------------------------------------------------------
def test_refused_arguments_write_nothing(ops):
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    a, b = (t.cuda() for t in R.data((2, 8, 64), seed=1))
    obuf, out = _guarded_f32(2)
    ws = ops.absdiff_ws("cuda")
    ws.fill_(SENT)
    r = torch.full((2, 8, 64), SENT, dtype=BF, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = libfk.Rows(64, 8, 512)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    null = ctypes.c_void_p(0)
    EINVAL, EUNSUP = -1, -2
    sums = lib.fk_absdiff_sums_bf16
    assert sums(null, rows, p(b), rows, 16, 64, 1, p(out), p(ws), ws.numel(), st) == EINVAL
    assert sums(p(a), rows, null, rows, 16, 64, 1, p(out), p(ws), ws.numel(), st) == EINVAL
    assert sums(p(a), rows, p(b), rows, 16, 64, 1, null, p(ws), ws.numel(), st) == EINVAL
    assert sums(p(a), rows, p(b), rows, 16, 64, 1, p(out), null, ws.numel(), st) == EINVAL
    assert sums(p(a), rows, p(b), rows, 16, 0, 1, p(out), p(ws), ws.numel(), st) == EINVAL            # D < 1
    assert sums(p(a), rows, p(b), rows, 0, 64, 1, p(out), p(ws), ws.numel(), st) == EINVAL            # no rows
    assert sums(p(a), libfk.Rows(63, 8, 512), p(b), rows, 16, 64, 1, p(out), p(ws), ws.numel(), st) == EINVAL   # ld < D
    assert sums(p(a), rows, p(b), rows, 16, 64, 1, p(out), p(ws), 1, st) == EINVAL                     # workspace too small
    assert sums(p(a), rows, p(b), rows, 16, 64, 0, p(out), p(ws), ws.numel(), st) == EUNSUP            # not bf16
    assert b"bf16" in lib.fk_last_error()
    for fn in (lib.fk_residual_save_bf16, lib.fk_residual_apply_bf16):
        assert fn(null, rows, p(b), rows, p(r), rows, 16, 64, 1, st) == EINVAL
        assert fn(p(a), rows, p(b), rows, null, rows, 16, 64, 1, st) == EINVAL
        assert fn(p(a), rows, p(b), rows, p(r), rows, 16, 0, 1, st) == EINVAL
        assert fn(p(a), rows, p(b), libfk.Rows(8, 8, 512), p(r), rows, 16, 64, 1, st) == EINVAL
        assert fn(p(a), rows, p(b), rows, p(r), rows, 16, 64, 0, st) == EUNSUP
        assert fn(p(a), rows, p(b), rows, p(b), rows, 16, 64, 1, st) == EINVAL                         # out is the SECOND input
        assert fn(p(a), rows, p(a), rows, p(r), rows, 16, 64, 1, st) == EINVAL                         # the inputs overlap
        assert fn(p(a), rows, p(b), rows, p(r), libfk.Rows(64, 8, 256), 16, 64, 1, st) == EINVAL       # the output's rows overlap
    # out overlapping h0 without being it: save never, apply only as the same view
    assert lib.fk_residual_save_bf16(p(a), rows, p(b), rows, p(a), rows, 16, 64, 1, st) == EINVAL
    shifted = ctypes.c_void_p(a.data_ptr() + 64 * 2)
    assert lib.fk_residual_apply_bf16(p(a), rows, p(b), rows, shifted, libfk.Rows(64, 7, 512), 14, 64, 1, st) == EINVAL
    torch.cuda.synchronize()
    a2, b2 = R.data((2, 8, 64), seed=1)
    assert torch.equal(a.cpu(), a2) and torch.equal(b.cpu(), b2) and bool((r == SENT).all())
    assert bool((obuf == SENT).all()) and bool((ws == SENT).all())
    # the wrappers: other dtypes and shapes
    with pytest.raises(RuntimeError, match="bf16"):
        ops.absdiff_sums(a.float(), b.float(), out=out, ws=ws)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.residual_save(a.half(), b.half(), r.half())
    with pytest.raises(ValueError):
        ops.residual_apply(a, b[:, :4], r)
    with pytest.raises(ValueError):
        ops.absdiff_sums(a.transpose(1, 2), b.transpose(1, 2))
    torch.cuda.synchronize()
    assert bool((obuf == SENT).all()) and bool((ws == SENT).all())
