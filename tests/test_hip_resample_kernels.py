"""GPU: ``fk_resample_pass_u8`` and ``fk_bytes_overlay_u8`` (csrc/resample.hip) against tests/resample_ref.py -- and against Pillow
itself where it imports -- on EVERY byte: the rules are integer arithmetic, so there is no tolerance anywhere in this file.

The kernel's own sizes (csrc/resample.hip): a horizontal tile is 256 outputs of one row and stages its source span in LDS pieces of
8192 bytes; a vertical block owns 256 lanes of 4 bytes (1 byte when the view is not 4-byte aligned); a launch has at most 8192
blocks and strides over the rest."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
FILTERS = ("lanczos", "bicubic", "bilinear")
CASES = [((97, 131), (40, 50)), ((64, 64), (64, 64)), ((300, 401), (128, 96)), ((50, 70), (123, 211)), ((1, 1), (5, 7)),
         ((7, 3), (1, 1)), ((513, 257), (256, 128)), ((1000, 37), (16, 16)), ((33, 65), (32, 64))]
TILE, PIECE_BYTES, MAX_BLOCKS = 256, 8192, 8192


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops
    return ops


def _rand(shape, seed, kind="rand"):
    rng = np.random.default_rng(seed)
    if kind == "rand":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return rng.choice(np.array([0, 255], dtype=np.uint8), shape)


def _gpu(ops, a, oh, ow, f):
    out = ops.resample_u8(torch.from_numpy(a).cuda(), oh, ow, f)
    assert out.is_contiguous() and out.dtype == torch.uint8
    return out.cpu().numpy()


def _pil(a, oh, ow, name):
    from PIL import Image
    flt = {"lanczos": Image.LANCZOS, "bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[name]
    return np.asarray(Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).resize((ow, oh), flt)).reshape(oh, ow, a.shape[2])


@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("case", CASES, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in CASES])
def test_equal_to_the_reference_and_to_pillow(ops, f, case):
    (H, W), (oh, ow) = case
    try:
        import PIL  # noqa: F401
        have_pil = True
    except ImportError:
        have_pil = False
    for B, C, kind in ((1, 1, "rand"), (3, 3, "rand"), (1, 3, "edges"), (3, 1, "edges")):
        a = _rand((B, H, W, C), seed=H + 3 * W + C, kind=kind)
        got = _gpu(ops, a, oh, ow, f)
        assert got.shape == (B, oh, ow, C)
        assert np.array_equal(got, R.resize(a, oh, ow, f)), (B, C, kind)
        if have_pil:
            for b in range(B):
                assert np.array_equal(got[b], _pil(a[b], oh, ow, f)), (B, C, kind, b)


def test_equal_size_returns_the_source_and_launches_nothing(ops):
    a = torch.from_numpy(_rand((2, 9, 11, 3), 1)).cuda()
    assert ops.resample_u8(a, 9, 11, "lanczos") is a
    view = a[:, 2:7, 3:9]
    out = ops.resample_u8(view, 5, 6, "bicubic")
    assert out.is_contiguous() and torch.equal(out, view)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("axis", [0, 1])
def test_each_pass_alone_at_its_tile_edges(ops, axis, C):
    """Horizontal: 255 / 256 / 257 / 513 outputs (one below, at, one above a tile; a third tile).  Vertical: rows of 1020 / 1024 /
    1028 bytes with the dword lanes, 255 / 256 / 257 bytes with the byte lanes (an odd row length).  Down- and upscales."""
    f = "bicubic"
    if axis == 1:
        shapes = [((3, 300), n) for n in (255, 256, 257, 513)] + [((2, 100), 257), ((2, 600), 256)]
    else:
        row_bytes = (1020, 1024, 1028, 255, 256, 257, 771) if C == 1 else (1020, 1032, 1023, 255, 258, 771)
        shapes = [((37, n // C), 20) for n in row_bytes] + [((9, 1024 // C + 3), 23)]
    for (H, W), n in shapes:
        for B in (1, 3):
            a = _rand((B, H, W, C), seed=H + W + n + B)
            got = ops.resample_pass_u8(torch.from_numpy(a).cuda(), axis, n, f).cpu().numpy()
            assert np.array_equal(got, R.pass_u8(a, axis, n, f)), (H, W, n, B)


@pytest.mark.parametrize("f", FILTERS)
def test_windows_wider_than_the_source_and_upscale_edges(ops, f):
    for (H, W), (oh, ow) in (((5, 5), (2, 2)), ((3, 4), (1, 1)), ((2, 2), (1, 1)),          # Win < ksize: the window is the whole row
                             ((4, 5), (37, 41)), ((2, 3), (64, 300))):                       # upscales: windows shrink at both edges
        a = _rand((2, H, W, 3), seed=H * W + oh)
        assert np.array_equal(_gpu(ops, a, oh, ow, f), R.resize(a, oh, ow, f)), (H, W, oh, ow)


def test_a_span_longer_than_one_lds_piece(ops):
    """One tile's windows cover more source than one LDS piece holds: 20x and 40x downscales of long rows."""
    for C, W, n in ((3, 6000, 300), (1, 20000, 500), (3, 8500, 100)):
        assert W * C > PIECE_BYTES
        a = _rand((1, 2, W, C), seed=W)
        got = ops.resample_pass_u8(torch.from_numpy(a).cuda(), 1, n, "lanczos").cpu().numpy()
        assert np.array_equal(got, R.pass_u8(a, 1, n, "lanczos")), (C, W, n)


def test_ksize_at_the_cap_and_one_over(ops):
    from gpt_image_edit_amd import helpers, libfk
    a = _rand((1, 512, 512, 3), seed=9)
    assert helpers.resample_coeffs(512, 2, "bilinear")[2] == helpers.FK_RESAMPLE_MAX_KSIZE == 513
    assert np.array_equal(_gpu(ops, a, 2, 2, "bilinear"), R.resize(a, 2, 2, "bilinear"))
    # one over: refused by the entry, dst untouched
    src = torch.from_numpy(a).cuda()
    for axis in (0, 1):
        dst = torch.full((1, 512, 2, 3) if axis == 1 else (1, 2, 512, 3), 0x5A, dtype=torch.uint8, device="cuda")
        bounds = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
        kk = torch.zeros(514 * 2, dtype=torch.int32, device="cuda")
        vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        rc = libfk.load().fk_resample_pass_u8(vp(src), src.stride(0), src.stride(1), vp(dst), 1, 512, 512, 3, axis, 2, vp(bounds), vp(kk),
                                              514, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == -1 and "ksize=514 is above FK_RESAMPLE_MAX_KSIZE = 513" in libfk.load().fk_last_error().decode()
        assert bool((dst == 0x5A).all())
    with pytest.raises(ValueError, match="FK_RESAMPLE_MAX_KSIZE"):
        ops.resample_u8(torch.zeros(1, 514, 4, 3, dtype=torch.uint8, device="cuda"), 2, 4, "bilinear")


@pytest.mark.parametrize("f", FILTERS)
def test_a_strided_crop_view_keeps_the_poison_out(ops, f):
    """The box is a view with the picture's strides, at byte offsets that are no multiple of 4; whatever lies around it must not
    reach an output byte.  A crop of zeros in a picture of 255s must come out all zero."""
    for C in (1, 3):
        for (x0, y0, x1, y1), (oh, ow) in (((13, 9, 110, 77), (32, 48)), ((1, 0, 130, 97), (50, 40)), ((50, 40, 57, 45), (64, 96)),
                                           ((3, 5, 128, 90), (85, 60)), ((7, 2, 71, 66), (64, 300))):
            pic = np.full((2, 97, 131, C), 255, dtype=np.uint8)
            pic[:, y0:y1, x0:x1] = _rand((2, y1 - y0, x1 - x0, C), seed=x0 + y0)
            t = torch.from_numpy(pic).cuda()
            got = ops.resample_u8(t[:, y0:y1, x0:x1], oh, ow, f).cpu().numpy()
            assert np.array_equal(got, R.resize(pic[:, y0:y1, x0:x1], oh, ow, f)), (C, x0, y0, oh, ow)
            t[:, y0:y1, x0:x1] = 0
            assert int(ops.resample_u8(t[:, y0:y1, x0:x1], oh, ow, f).max()) == 0, (C, x0, y0, oh, ow)
            assert bool((t.cpu().numpy()[:, :y0] == 255).all())                            # and the source is only read


def test_dst_inside_a_sentinel_filled_buffer(ops):
    a = _rand((2, 41, 53, 3), seed=4)
    src = torch.from_numpy(a).cuda()
    for oh, ow, pad in ((17, 29, 64), (41, 29, 61), (17, 53, 3)):                          # both passes, horizontal alone, vertical alone
        n = 2 * oh * ow * 3
        buf = torch.full((pad + n + 64,), 0xC3, dtype=torch.uint8, device="cuda")
        out = buf[pad:pad + n].view(2, oh, ow, 3)
        assert ops.resample_u8(src, oh, ow, "lanczos", out=out) is out
        assert np.array_equal(out.cpu().numpy(), R.resize(a, oh, ow, "lanczos"))
        assert bool((buf[:pad] == 0xC3).all()) and bool((buf[pad + n:] == 0xC3).all())


def test_past_the_first_grid_trip(ops):
    """More work items than the launch has blocks, in either pass."""
    a = _rand((1, MAX_BLOCKS + 9, 8, 1), seed=6)                                           # horizontal: one item per source row
    got = ops.resample_pass_u8(torch.from_numpy(a).cuda(), 1, 4, "bilinear").cpu().numpy()
    assert np.array_equal(got, R.pass_u8(a, 1, 4, "bilinear"))
    b = _rand((3, 1400, 4, 1), seed=7)                                                     # vertical: one item per output row
    assert 3 * 2800 > MAX_BLOCKS
    got = ops.resample_pass_u8(torch.from_numpy(b).cuda(), 0, 2800, "bicubic").cpu().numpy()
    assert np.array_equal(got, R.pass_u8(b, 0, 2800, "bicubic"))


@pytest.mark.parametrize("f", FILTERS)
def test_both_clips_and_repeat_launches(ops, f):
    H, W = 64, 96
    board = np.zeros((1, H, W, 3), dtype=np.uint8)
    board[:, ::2, 1::2] = 255
    board[:, 1::2, ::2] = 255
    blocks = np.kron(_rand((1, 8, 12, 1), seed=2, kind="edges"), np.ones((1, 8, 8, 3), dtype=np.uint8))      # hard edges: overshoot
    for a in (np.full((1, H, W, 3), 255, dtype=np.uint8), np.zeros((1, H, W, 3), dtype=np.uint8), board, blocks):
        for oh, ow in ((24, 40), (100, 150), (61, 96)):
            ref = R.resize(a, oh, ow, f)
            got = _gpu(ops, a, oh, ow, f)
            assert np.array_equal(got, ref)
            assert np.array_equal(_gpu(ops, a, oh, ow, f), got)                            # a second launch: the same bits
    assert (R.resize(np.full((1, H, W, 3), 255, dtype=np.uint8), 24, 40, f) == 255).all()
    if f != "bilinear":                                                                    # the clip is exercised at both ends
        from gpt_image_edit_amd import helpers
        bounds, kk, _ = helpers.resample_coeffs(96, 150, f)
        row = blocks[0, 0, :, 0].astype(np.int64)
        acc = np.array([(kk[i, :bounds[i, 1] - bounds[i, 0]].numpy().astype(np.int64) * row[bounds[i, 0]:bounds[i, 1]]).sum()
                        for i in range(150)]) + (1 << 21)
        assert (acc >> 22).min() < 0 and (acc >> 22).max() > 255


# ---- fk_bytes_overlay_u8 -----------------------------------------------------------------------------------------------------------
def test_overlay_equals_the_integer_rule(ops):
    Hp, Wp, box = 37, 67, (5, 3, 61, 30)
    bh, bw = box[3] - box[1], box[2] - box[0]
    for B, No, Na in ((3, 1, 1), (3, 3, 3), (1, 1, 1), (2, 1, 2), (2, 2, 1)):
        res = _rand((B, bh, bw, 3), seed=B + No)
        orig = _rand((No, Hp, Wp, 3), seed=10 + No)
        alpha = _rand((Na, Hp, Wp), seed=20 + Na)
        alpha[:, 5:12, 7:30] = 0
        alpha[:, 12:20, 7:30] = 255
        got = ops.bytes_overlay(torch.from_numpy(res).cuda(), torch.from_numpy(orig).cuda(), torch.from_numpy(alpha).cuda(), box)
        got = got.cpu().numpy()
        assert np.array_equal(got, R.overlay(res, orig, alpha, box)), (B, No, Na)
        full = np.broadcast_to(orig, (B, Hp, Wp, 3))
        outside = np.ones((Hp, Wp), dtype=bool)
        outside[box[1]:box[3], box[0]:box[2]] = False
        assert np.array_equal(got[:, outside], full[:, outside])                           # the input's bytes outside the box
        assert np.array_equal(got[:, 5:12, 7:30], full[:, 5:12, 7:30])                     # ... and at a == 0
        assert np.array_equal(got[:, 12:20, 7:30], res[:, 12 - box[1]:20 - box[1], 7 - box[0]:30 - box[0]])       # res at a == 255
        none = ops.bytes_overlay(torch.from_numpy(res).cuda(), torch.from_numpy(orig).cuda(), None, box).cpu().numpy()
        assert np.array_equal(none, R.overlay(res, orig, None, box))
        assert np.array_equal(none[:, box[1]:box[3], box[0]:box[2]], res)


def test_overlay_every_alpha_against_every_pair(ops):
    """All 256 alphas against a 16 x 16 grid of (result, original) bytes: the grid tests/test_resample_ref.py holds to the exact
    quotient."""
    vals = np.array(sorted(set(range(0, 256, 17)) | {1, 127, 128, 254})[:16], dtype=np.uint8)
    a, r, o = np.meshgrid(np.arange(256, dtype=np.uint8), vals, vals, indexing="ij")
    H, W = 256, 256
    alpha = a.reshape(1, H, W)
    res = np.repeat(r.reshape(1, H, W, 1), 3, axis=3)
    orig = np.repeat(o.reshape(1, H, W, 1), 3, axis=3)
    got = ops.bytes_overlay(torch.from_numpy(res).cuda(), torch.from_numpy(orig).cuda(), torch.from_numpy(alpha).cuda(), (0, 0, W, H))
    assert np.array_equal(got.cpu().numpy(), R.blend(alpha[..., None], res, orig))


def test_overlay_refusals(ops):
    res = torch.zeros(2, 8, 12, 3, dtype=torch.uint8, device="cuda")
    orig = torch.zeros(1, 20, 30, 3, dtype=torch.uint8, device="cuda")
    alpha = torch.zeros(1, 20, 30, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="the result is 8 x 12, the box 8 x 11"):
        ops.bytes_overlay(res, orig, alpha, (5, 6, 16, 14))
    with pytest.raises(RuntimeError, match="is empty or outside the 30 x 20 picture"):
        ops.bytes_overlay(res, orig, alpha, (20, 6, 32, 14))
    with pytest.raises(RuntimeError, match="2 original pictures for a batch of 3"):
        ops.bytes_overlay(torch.zeros(3, 8, 12, 3, dtype=torch.uint8, device="cuda"), torch.cat([orig, orig]), alpha, (5, 6, 17, 14))
    with pytest.raises(ValueError, match="alpha is"):
        ops.bytes_overlay(res, orig, alpha[:, :10].contiguous(), (5, 6, 17, 14))
    with pytest.raises(TypeError):
        ops.bytes_overlay(res.float(), orig, alpha, (5, 6, 17, 14))
