"""CPU: the references and checkers of the mask-box kernels (tests/mask_ops_ref.py) and the host helpers they stand on
(``helpers.gaussian_taps``, ``helpers.mask_crop_box``).  A checker that accepts a wrong kernel tests nothing, so each is shown a
correct float32 evaluation (must pass) and the classic wrong ones (must fail).  No GPU needed."""
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref as R  # noqa: E402

from gpt_image_edit_amd import helpers  # noqa: E402

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def _rand_u8(shape, seed, lo=0):
    return torch.randint(lo, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---- taps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.3, 0.5, 1.0, 4.0, 7.7, 64.0])
def test_taps_are_symmetric_and_sum_to_one(sigma):
    t = helpers.gaussian_taps(sigma)
    R_ = (t.numel() - 1) // 2
    assert t.dtype == F32 and t.numel() == 2 * R_ + 1 and R_ == int(-(-3.0 * sigma // 1))        # R = ceil(3 sigma)
    assert torch.equal(t, t.flip(0)) and t.argmax().item() == R_ and (t > 0).all()
    assert abs(t.to(F64).sum().item() - 1.0) <= (2 * R_ + 1) * 2.0 ** -24
    raw = R.taps_raw64(sigma)
    assert torch.equal(t, (raw / raw.sum()).to(F32))


@pytest.mark.parametrize("sigma", [0, 0.0, -1.0, 64.5, float("nan"), float("inf")])
def test_taps_refuse_a_sigma_outside_the_range(sigma):
    with pytest.raises(ValueError, match="mask_blur"):
        helpers.gaussian_taps(sigma)


@pytest.mark.parametrize("sigma", [0.5, 4.0, 64.0])
@pytest.mark.parametrize("value", [0, 255])
def test_constant_planes_blur_to_themselves(sigma, value):
    plane = torch.full((1, 9, 13), value, dtype=torch.uint8)
    assert torch.equal(R.blur_fp32(plane, helpers.gaussian_taps(sigma)), plane)
    R.check_blur(plane, plane, sigma)


def test_blur_checker_accepts_the_restatement_and_rejects_wrong_blurs():
    m = _rand_u8((2, 11, 17), 1)
    m[:, :, :3] = 255                                   # an edge that a wrap would fold onto the other side
    m[:, :, -3:] = 0
    sigma = 1.5
    taps = helpers.gaussian_taps(sigma)
    good = R.blur_fp32(m, taps)
    R.check_blur(good, m, sigma)
    with pytest.raises(AssertionError):                 # unnormalised taps
        R.check_blur(R.blur_fp32(m, R.taps_raw64(sigma).to(F32)), m, sigma)
    with pytest.raises(AssertionError):                 # wrap instead of clamp at the edge
        R.check_blur(R.blur_fp32(m, taps, wrap=True), m, sigma)
    with pytest.raises(AssertionError):                 # no blur at all
        R.check_blur(m, m, sigma)


# ---- the bilinear rule --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src, dst", [((5, 7), (9, 16)), ((9, 16), (5, 7)), ((6, 11), (13, 4)), ((1, 1), (3, 2)), ((4, 4), (4, 4))])
def test_bilinear_reference_is_torch_interpolate(src, dst):
    p = torch.rand(2, 3, *src, generator=torch.Generator().manual_seed(2), dtype=F64)
    want = torch.nn.functional.interpolate(p, size=dst, mode="bilinear", align_corners=False)
    assert (R.bilinear(p, *dst) - want).abs().max().item() <= 1e-5
    if src == dst:
        assert torch.equal(R.bilinear(p, *dst), p) and torch.equal(R.bilinear(p.to(F32), *dst, dtype=F32), p.to(F32))


CROPS = [((37, 67), (5, 3, 67, 37), (64, 96)), ((40, 50), (0, 0, 33, 29), (15, 21)), ((30, 41), (7, 2, 20, 30), (48, 9))]


@pytest.mark.parametrize("size, box, out", CROPS)
@pytest.mark.parametrize("renorm", [0, 1])
def test_crop_checker_rejects_wrong_crops(size, box, out, renorm):
    u8 = _rand_u8((2, *size, 3), 3, lo=128 if renorm else 0)

    def as_kernel(v):
        return torch.cat([v.to(BF), torch.zeros(*v.shape[:3], 5, dtype=BF)], dim=-1)
    R.check_crop(as_kernel(R.crop(u8, box, *out, renorm)), u8, box, *out, renorm)
    x0, y0, x1, y1 = box
    wrong = {"no half-pixel offset": R.crop(u8, box, *out, renorm, half=0.0),
             "x and y swapped": R.crop(u8, box, *out, renorm, swap=True),
             "origin off by one in x": R.crop(u8, (x0 + 1 if x1 < size[1] else x0 - 1, y0, x1 + 1 if x1 < size[1] else x1 - 1, y1),
                                             *out, renorm),
             "origin off by one in y": R.crop(u8, (x0, y0 + 1 if y1 < size[0] else y0 - 1, x1, y1 + 1 if y1 < size[0] else y1 - 1),
                                             *out, renorm),
             "the other renorm": R.crop(u8, box, *out, 1 - renorm)}
    for name, v in wrong.items():
        with pytest.raises(AssertionError):
            R.check_crop(as_kernel(v), u8, box, *out, renorm)
            pytest.fail(f"the crop checker accepted: {name}")
    with pytest.raises(AssertionError, match="pad channels"):
        R.check_crop(as_kernel(R.crop(u8, box, *out, renorm)) + torch.tensor([0, 0, 0, 0, 0, 1, 0, 0], dtype=BF), u8, box, *out, renorm)


@pytest.mark.parametrize("renorm", [0, 1])
def test_a_sample_on_a_source_pixel_may_take_the_float32_value_of_the_byte(renorm):
    """K3 evaluates its rule in float64 but gives a sample that lies on a source pixel the whole-picture kernel's float32 value:
    for every byte that can occur the two are at most 1 bf16 ulp apart, so the crop's bound holds on either side."""
    u = torch.arange(128 if renorm else 0, 256)
    v32 = ((u.to(F32) / 255.0) - 0.5) / 0.5
    v64 = ((u.to(F64) / 255.0) - 0.5) / 0.5
    if renorm:
        v32, v64 = 2.0 * v32 - 1.0, 2.0 * v64 - 1.0
    d = (R.bf16_index(v32.to(BF)) - R.bf16_index(v64.to(BF))).abs()
    assert int(d.max()) <= 1 and int((d > 0).sum()) <= 1
    # and the crop checker takes the whole-picture values at equal size
    u8 = _rand_u8((1, 9, 11, 3), 7, lo=128 if renorm else 0)
    u8[0, 0, 0, 0] = 191
    v = ((u8.to(F32) / 255.0) - 0.5) / 0.5
    got = torch.cat([(2.0 * v - 1.0 if renorm else v).to(BF), torch.zeros(1, 9, 11, 1, dtype=BF)], dim=-1)
    R.check_crop(got, u8, (0, 0, 11, 9), 9, 11, renorm)


def test_float32_cannot_hold_one_bf16_ulp_where_the_normalised_value_crosses_zero():
    """Why K3 is float64: the op-by-op float32 evaluation of the same rule misses the crop's bound near v = 0."""
    u8 = _rand_u8((2, 37, 67, 3), 14)
    v32 = R.crop(u8, (5, 3, 67, 37), 64, 96, 0, dtype=F32)
    with pytest.raises(AssertionError, match="beyond 1 bf16 ulp"):
        R.check_crop(torch.cat([v32.to(BF), torch.zeros(2, 64, 96, 1, dtype=BF)], dim=-1), u8, (5, 3, 67, 37), 64, 96, 0)


# ---- the overlay ------------------------------------------------------------------------------------------------------------------
def test_overlay_delta_is_the_sum_of_its_roundings():
    # the derivation of mask_ops_ref.overlay_delta, term by term, for a 96-sample side
    n, U = 96, 2.0 ** -24
    ds = 3 * n * U                      # quotient, product, difference: each rounded on a magnitude <= n
    dg = 2 * ds + 12 * U                # two axes, slope <= 1; then the three mixes
    dc = 255 * dg + 255 * U             # c = g * 255
    dv = dc + 3 * 65025 * U / 255 + 255 * U
    assert R.overlay_delta(n) == pytest.approx(dv, rel=1e-12)
    assert 65025 == 255 * 255 and R.overlay_delta(96) < 0.01 and R.overlay_delta(4096) < 0.5


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("size, box, hw", [((37, 67), (5, 3, 67, 37), (16, 24)), ((20, 30), (0, 0, 30, 20), (20, 30)),
                                           ((33, 29), (4, 6, 17, 25), (40, 48))])
def test_overlay_checker_accepts_float32_and_rejects_wrong_overlays(dtype, size, box, hw):
    g = torch.Generator().manual_seed(4)
    img = (torch.rand(3, 3, *hw, generator=g) * 2.4 - 1.2).to(dtype)        # beyond [-1, 1]: the clamp is used
    orig = _rand_u8((1, *size, 3), 5)
    alpha = _rand_u8((3, *size), 6)
    alpha[:, ::3] = 0
    alpha[:, 1::3] = 255

    def as_kernel(v):
        return v.clamp(0, 255).round().to(torch.uint8)
    v32, taken = R.overlay(img, orig, alpha, box, dtype=F32)
    assert taken.any() and (~taken).any()
    worst = R.check_overlay(as_kernel(v32), img, orig, alpha, box)          # a correct float32 evaluation passes
    assert worst <= 0.5 + R.overlay_delta(max(hw))
    R.check_overlay(as_kernel(R.overlay(img, orig, None, box, dtype=F32)[0]), img, orig, None, box)
    x0, y0, x1, y1 = box
    whole = box == (0, 0, size[1], size[0])
    moved = box if whole else (x0 + 1, y0, x1 + 1, y1) if x1 < size[1] else (x0 - 1, y0, x1 - 1, y1)
    wrong = {"no half-pixel offset": R.overlay(img, orig, alpha, box, half=0.0)[0],
             "inverted alpha": R.overlay(img, orig, alpha, box, invert=True)[0],
             "x and y swapped": R.overlay(img.transpose(-1, -2), orig, alpha, box)[0],
             "origin off by one": R.overlay(img, orig, alpha, moved)[0],
             "alpha ignored": R.overlay(img, orig, None, box)[0]}
    if whole:
        del wrong["origin off by one"]                  # the whole picture has nowhere to move to
        if hw == tuple(size):
            del wrong["no half-pixel offset"]           # equal sizes: s = X with and without the offset
    for name, v in wrong.items():
        with pytest.raises(AssertionError):
            R.check_overlay(as_kernel(v), img, orig, alpha, box)
            pytest.fail(f"the overlay checker accepted: {name}")


def test_overlay_ends_are_taken_not_computed():
    img = torch.full((1, 3, 4, 4), 0.3)
    orig = torch.full((1, 4, 4, 3), 77, dtype=torch.uint8)
    alpha = torch.tensor([0, 255, 128, 1], dtype=torch.uint8).view(1, 1, 4).expand(1, 4, 4).contiguous()
    v, taken = R.overlay(img, orig, alpha, (0, 0, 4, 4))
    c = R.image_unit(img)[0, 0, 0, 0].item() * 255
    assert taken[0, 0].tolist() == [True, False, False, False]
    assert v[0, 0, 0, 0] == 77 and v[0, 0, 1, 0] == c
    assert v[0, 0, 2, 0].item() == pytest.approx((128 * c + 127 * 77) / 255, abs=1e-9)


# ---- K1's reference and the box rule ------------------------------------------------------------------------------------------------
def test_bbox_reference():
    m = torch.zeros(2, 5, 7, dtype=torch.uint8)
    assert R.bbox_numpy(m, 1) == [7, 5, 0, 0]
    m[1, 2, 3] = 9
    assert R.bbox_numpy(m, 1) == [3, 2, 4, 3] and R.bbox_numpy(m, 10) == [7, 5, 0, 0]
    m[0, 4, 0] = 255
    assert R.bbox_numpy(m, 1) == [0, 2, 4, 5] and R.bbox_numpy(m, 0) == [0, 0, 7, 5]


def test_crop_box_rule():
    pics = [(100, 100), (192, 128), (67, 37), (640, 480)]
    targets = [(96, 64), (64, 96), (64, 64), (1024, 1024), (16, 48)]
    seen_fit = seen_clamped = 0
    for (W, H), (tw, th), pad in itertools.product(pics, targets, (0, 3, 32)):
        for bbox in ((0, 0, 1, 1), (W - 1, H - 1, W, H), (W // 3, H // 4, W // 3 + 9, H // 4 + 20), (5, H // 2, W - 7, H // 2 + 4),
                     (0, 0, W, H), (W // 2, 0, W // 2 + 1, H)):
            x0, y0, x1, y1 = box = helpers.mask_crop_box(bbox, W, H, pad, tw, th)
            assert all(isinstance(v, int) for v in box)
            px0, py0, px1, py1 = max(bbox[0] - pad, 0), max(bbox[1] - pad, 0), min(bbox[2] + pad, W), min(bbox[3] + pad, H)
            assert x0 <= px0 and y0 <= py0 and x1 >= px1 and y1 >= py1, (box, bbox)           # contains the padded bbox
            assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H                                    # lies inside the picture
            bw, bh = x1 - x0, y1 - y0
            assert bw == px1 - px0 or bh == py1 - py0                                         # only one side grows
            if bw < W and bh < H:       # it fits: the grown side is the nearest integer to the target's aspect
                assert abs(bw * th - bh * tw) <= max(tw, th), (box, bbox, tw, th)
                assert min(abs(bw - bh * tw / th), abs(bh - bw * th / tw)) <= 1
                seen_fit += 1
            else:
                seen_clamped += 1
            if bbox == (0, 0, W, H):
                assert box == (0, 0, W, H)                                                    # the whole picture stays whole
    assert seen_fit > 50 and seen_clamped > 50
    # the odd pixel goes to the far side; a box at the edge is shifted back inside, not cut
    assert helpers.mask_crop_box((10, 10, 14, 11), 100, 100, 0, 64, 64) == (10, 9, 14, 13)
    assert helpers.mask_crop_box((10, 10, 11, 14), 100, 100, 0, 64, 64) == (9, 10, 13, 14)
    assert helpers.mask_crop_box((10, 10, 11, 15), 100, 100, 0, 64, 64) == (8, 10, 13, 15)
    assert helpers.mask_crop_box((0, 0, 4, 40), 100, 100, 0, 64, 64) == (0, 0, 40, 40)
    assert helpers.mask_crop_box((96, 0, 100, 40), 100, 100, 0, 64, 64) == (60, 0, 100, 40)
    assert helpers.mask_crop_box((10, 10, 20, 40), 100, 100, 2, 96, 64) == (0, 8, 51, 42)
    # larger than the picture: clamped, and the aspect differs
    assert helpers.mask_crop_box((0, 0, 30, 100), 50, 100, 0, 64, 64) == (0, 0, 50, 100)
    for bad in ((5, 5, 5, 9), (5, 5, 9, 5), (100, 100, 0, 0)):
        with pytest.raises(ValueError, match="empty"):
            helpers.mask_crop_box(bad, 100, 100, 0, 64, 64)
    with pytest.raises(ValueError):
        helpers.mask_crop_box((0, 0, 4, 4), 100, 100, -1, 64, 64)
    with pytest.raises(ValueError):
        helpers.mask_crop_box((0, 0, 101, 4), 100, 100, 0, 64, 64)
