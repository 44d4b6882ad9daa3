"""GPU: the four mask-box kernels against tests/mask_ops_ref.py.  Every output lives between sentinel guard bytes that must
survive the launch.  K1 equals numpy; K2 is held to 0 ulp of the op-by-op float32 restatement; K3 to 1 bf16 ulp of bf16(float64) on
every element and to the whole-picture kernel's bits; K4 to the bound derived in mask_ops_ref.overlay_delta on every byte, to the
original's bytes where they are taken, and to fk_image_to_u8_nhwc's bits.

K3 runs its rule in float64 (csrc/mask_ops.hip says why: float32 cannot hold 1 bf16 ulp where the normalised value crosses 0 -- the
op-by-op float32 evaluation, mask_ops_ref.crop(dtype=float32), misses it on 1 to 8 elements of ~20 000 per case, by up to 75 ulp)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as o
    return o


def _rand_u8(shape, seed, lo=0):
    return torch.randint(lo, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


class Guarded:
    """A contiguous device tensor of ``shape`` / ``dtype`` in the middle of a byte buffer filled with a sentinel."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(*shape)

    def intact(self):
        return bool((self.raw[:GUARD] == FILL).all() and (self.raw[-GUARD:] == FILL).all())

    def untouched(self):
        return bool((self.raw == FILL).all())


# ---- K1 ---------------------------------------------------------------------------------------------------------------------------
def _bbox(ops, mask, thr):
    out = Guarded((4,), torch.int32)
    ops.mask_bbox(mask.cuda(), thr, out=out.t)
    torch.cuda.synchronize()
    assert out.intact()
    return out.t.tolist()


# (1200, 1200) x 3: 1 080 000 four-byte vectors > 4096 * 256, the vector kernel's second grid-stride trip;
# (1031, 1021) x 1: 1 052 651 bytes > 4096 * 256, the byte kernel's
@pytest.mark.parametrize("Bm, H, W", [(1, 1, 1), (3, 1, 1), (1, 37, 67), (3, 37, 67), (1, 36, 68), (3, 1200, 1200), (1, 1031, 1021)])
def test_bbox_equals_numpy(ops, Bm, H, W):
    empty = torch.zeros(Bm, H, W, dtype=torch.uint8)
    assert _bbox(ops, empty, 1) == [W, H, 0, 0] == R.bbox_numpy(empty, 1)
    assert _bbox(ops, empty, 0) == [0, 0, W, H]
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):       # one pixel in each corner, in the last sample
        m = empty.clone()
        m[Bm - 1, y, x] = 1
        assert _bbox(ops, m, 1) == [x, y, x + 1, y + 1]
    m = empty.clone()
    m[0, H // 3:H // 3 + 5, W // 2:W // 2 + 3] = 200
    m[Bm - 1, H - 1 - H // 4, W // 5] = 130
    m[Bm // 2, H // 2, W - 1 - W // 7] = 99
    for thr in (1, 100, 131, 201, 255):
        assert _bbox(ops, m, thr) == R.bbox_numpy(m, thr), thr
    if H * W < 10000:
        rnd = _rand_u8((Bm, H, W), 11)
        for thr in (250, 255):
            assert _bbox(ops, rnd, thr) == R.bbox_numpy(rnd, thr)


# ---- K2 ---------------------------------------------------------------------------------------------------------------------------
# sigma chosen for R = ceil(3 sigma): 2, 6 (wider than the 3 x 5 plane: the clamp folds taps), 3, 12, 192
@pytest.mark.parametrize("H, W, sigma, R_", [(1, 1, 0.6, 2), (3, 5, 2.0, 6), (37, 67, 1.0, 3), (130, 258, 4.0, 12), (200, 70, 64.0, 192)])
def test_blur_is_the_float32_restatement_bit_for_bit(ops, H, W, sigma, R_):
    from gpt_image_edit_amd import helpers
    assert (helpers.gaussian_taps(sigma).numel() - 1) // 2 == R_
    m = _rand_u8((2, H, W), 12)
    m[1, : H // 2] = 255                                 # a hard edge and flat ends next to the noise
    m[1, H // 2:] = 0
    out = Guarded((2, H, W), torch.uint8)
    ops.mask_blur(m.cuda(), sigma, out=out.t)
    torch.cuda.synchronize()
    assert out.intact()
    R.check_blur(out.t.cpu(), m, sigma)


def test_blur_second_grid_stride_trip(ops):
    m = _rand_u8((1, 1031, 1021), 13)                    # 1 052 651 pixels > 4096 * 256
    got = ops.mask_blur(m.cuda(), 0.5).cpu()
    R.check_blur(got, m, 0.5)


# ---- K3 ---------------------------------------------------------------------------------------------------------------------------
# (picture H x W, box, output h x w): up, down, mixed; odd sizes; the first box touches the right and bottom edges
# then a box at equal size (every sample lies on a source pixel: the float32 value of the byte) and at twice its size (weights 1/4 and
# 3/4: interpolated values that are exactly 127.5, a normalised 0)
CROPS = [((37, 67), (5, 3, 67, 37), (64, 96)), ((128, 192), (0, 0, 101, 91), (37, 53)), ((70, 90), (10, 20, 33, 64), (48, 31)),
         ((40, 50), (3, 4, 35, 28), (24, 32)), ((40, 50), (3, 4, 35, 28), (48, 64))]


def _crop(ops, u8, box, out, renorm, cpad=32):
    g = Guarded((u8.shape[0], *out, cpad), BF)
    ops.pixels_box_to_nhwc(u8.cuda(), box, *out, cpad, renorm, out=g.t)
    torch.cuda.synchronize()
    assert g.intact()
    return g.t.cpu()


@pytest.mark.parametrize("size, box, out", CROPS)
@pytest.mark.parametrize("renorm", [0, 1])
def test_crop_within_one_bf16_ulp_of_float64(ops, size, box, out, renorm):
    u8 = _rand_u8((2, *size, 3), 14, lo=128 if renorm else 0)
    got = _crop(ops, u8, box, out, renorm)
    want = R.crop(u8, box, *out, renorm).to(BF)
    d = (R.bf16_index(got[..., :3]) - R.bf16_index(want)).abs()
    print(f"crop {size} {box} -> {out} renorm={renorm}: {int((d > 1).sum())} of {d.numel()} beyond 1 ulp, worst {int(d.max())}")
    R.check_crop(got, u8, box, *out, renorm)


@pytest.mark.parametrize("renorm", [0, 1])
def test_crop_of_the_whole_picture_at_equal_size_is_the_whole_picture_kernel(ops, renorm):
    u8 = _rand_u8((2, 37, 67, 3), 15, lo=128 if renorm else 0)
    got = _crop(ops, u8, (0, 0, 67, 37), (37, 67), renorm)
    assert torch.equal(got, ops.pixels_to_nhwc(u8.cuda(), 37, 67, 32, renorm).cpu())


def test_crop_second_grid_stride_trip(ops):
    u8 = _rand_u8((1, 40, 50, 3), 16)
    out = (190, 180)                                     # 190 * 180 * 32 = 1 094 400 elements > 4096 * 256
    got = _crop(ops, u8, (3, 4, 44, 39), out, 0)
    R.check_crop(got, u8, (3, 4, 44, 39), *out, 0)


# ---- K4 ---------------------------------------------------------------------------------------------------------------------------
def _overlay(ops, img, orig, alpha, box):
    g = Guarded((img.shape[0], *orig.shape[1:]), torch.uint8)
    ops.image_overlay(img.cuda(), orig.cuda(), None if alpha is None else alpha.cuda(), box, out=g.t)
    torch.cuda.synchronize()
    assert g.intact()
    return g.t.cpu()


def _alpha(shape, seed):
    a = _rand_u8(shape, seed)
    a[:, ::3] = 0
    a[:, 1::3] = 255
    return a


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("size, box, hw", [((37, 67), (5, 3, 67, 37), (16, 24)), ((33, 29), (4, 6, 17, 25), (40, 48)),
                                           ((50, 41), (0, 9, 41, 50), (24, 56))])
@pytest.mark.parametrize("N, Bm", [(1, 1), (1, 3), (3, 1), (3, 3), (1, None)])
def test_overlay_within_the_derived_bound(ops, dtype, size, box, hw, N, Bm):
    g = torch.Generator().manual_seed(17)
    img = (torch.rand(3, 3, *hw, generator=g) * 2.4 - 1.2).to(dtype)
    orig = _rand_u8((N, *size, 3), 18)
    alpha = None if Bm is None else _alpha((Bm, *size), 19)
    got = _overlay(ops, img, orig, alpha, box)
    worst = R.check_overlay(got, img, orig, alpha, box)
    print(f"overlay {size} {box} <- {hw} {dtype}: worst |d| {worst:.6f}, bound {0.5 + R.overlay_delta(max(hw)):.6f}")


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("alpha", ["255", None])
def test_overlay_of_the_whole_picture_at_equal_size_is_image_to_u8(ops, dtype, alpha):
    img = (torch.rand(3, 3, 37, 67, generator=torch.Generator().manual_seed(20)) * 2.4 - 1.2).to(dtype)
    orig = _rand_u8((1, 37, 67, 3), 21)
    a = None if alpha is None else torch.full((1, 37, 67), 255, dtype=torch.uint8)
    got = _overlay(ops, img, orig, a, (0, 0, 67, 37))
    assert torch.equal(got, ops.image_to_u8(img.cuda()).cpu())


def test_overlay_second_grid_stride_trip(ops):
    img = (torch.rand(1, 3, 40, 50, generator=torch.Generator().manual_seed(22)) * 2 - 1).to(BF)
    size, box = (600, 610), (7, 9, 600, 580)             # 600 * 610 * 3 = 1 098 000 bytes > 4096 * 256
    orig, alpha = _rand_u8((1, *size, 3), 23), _alpha((1, *size), 24)
    R.check_overlay(_overlay(ops, img, orig, alpha, box), img, orig, alpha, box)


# ---- refusals write nothing -------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    m = _rand_u8((2, 9, 12), 25).cuda()
    u8 = _rand_u8((2, 9, 12, 3), 26).cuda()
    img = torch.zeros(2, 3, 8, 8, dtype=BF, device="cuda")
    out4, ws = Guarded((4,), torch.int32), Guarded((16384,), torch.int32)
    with pytest.raises(RuntimeError, match="threshold=300"):
        ops.mask_bbox(m, 300, out=out4.t, ws=ws.t)
    with pytest.raises(RuntimeError, match="workspace of 100 ints"):
        ops.mask_bbox(m, 1, out=out4.t, ws=ws.t[:100])
    blur = Guarded((2, 9, 12), torch.uint8)
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    taps = torch.ones(3, device="cuda")
    plane = Guarded((2, 9, 12), F32)
    p = lambda t: ops._ptr(t)  # noqa: E731
    assert lib.fk_mask_blur_u8(p(m), p(blur.t), p(plane.t), p(taps), 193, 2, 9, 12, ops._stream()) == -1
    assert lib.fk_mask_blur_u8(p(m), p(blur.t), p(plane.t), p(plane.t), 1, 2, 9, 12, ops._stream()) == -1
    crop = Guarded((2, 8, 8, 32), BF)
    for box in ((0, 0, 13, 9), (-1, 0, 12, 9), (4, 4, 4, 9), (0, 0, 12, 10)):
        assert lib.fk_pixels_u8_box_to_nhwc_bf16(p(u8), p(crop.t), 2, 9, 12, *box, 8, 8, 32, 0, ops._stream()) == -1
        assert "empty or outside" in lib.fk_last_error().decode()
    over = Guarded((2, 9, 12, 3), torch.uint8)
    with pytest.raises(RuntimeError, match="empty or outside"):
        ops.image_overlay(img, u8, m, (0, 0, 13, 9), out=over.t)
    with pytest.raises(RuntimeError, match="3 original pictures for a batch of 2"):
        ops.image_overlay(img, torch.cat([u8, u8[:1]]), m, (0, 0, 12, 9), out=over.t)
    with pytest.raises(RuntimeError, match="alpha_batch=3"):
        ops.image_overlay(img, u8, torch.cat([m, m[:1]]), (0, 0, 12, 9), out=over.t)
    torch.cuda.synchronize()
    for g in (out4, ws, blur, plane, crop, over):
        assert g.untouched()
