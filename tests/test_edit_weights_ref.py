"""CPU: tests/edit_weights_ref.py (the numpy restatement the HIP stages are held to) against independent implementations --
Pillow for the grey and the threshold, scipy.ndimage for the closing and the labelling, torch for the pool and the weight -- and
the proof that this comparison rejects each plausible mistake on an input the correct restatement passes."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image, ImageChops
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_weights_ref as R  # noqa: E402


# ---- the independent stages -----------------------------------------------------------------------------------------------------
def pil_diff_mask(ref, tgt, threshold=18):
    grey = ImageChops.difference(Image.fromarray(ref), Image.fromarray(tgt)).convert("L")
    return np.array(grey.point(lambda v: 255 if v >= threshold else 0), dtype=np.uint8)


def scipy_close5(plane):
    d = ndimage.binary_dilation(plane >= 128, structure=R.ELLIPSE5, border_value=0)
    return np.where(ndimage.binary_erosion(d, structure=R.ELLIPSE5, border_value=1), 255, 0).astype(np.uint8)


def scipy_filter(plane, threshold=0.3):
    labels, n = ndimage.label(plane >= 128, structure=np.ones((3, 3), dtype=bool))
    total = np.count_nonzero(plane >= 128)
    out = np.zeros(plane.shape, dtype=np.uint8)
    for lbl in range(1, n + 1):
        comp = labels == lbl
        if comp.sum() >= threshold * total:                      # float64, as the reference writes it
            out[comp] = 255
    return out


def torch_pool8(plane):
    t = torch.from_numpy(plane).float().div(255.0)[None, None]
    return (F.max_pool2d(t, kernel_size=8, stride=8)[0, 0] > 0).to(torch.uint8).mul(255).numpy()


def torch_weight(mask_ds, weight_type):
    t = torch.from_numpy(mask_ds).float()
    b = t.bool()
    x = b.numel() / b.sum()
    weight = torch.round(torch.log2(x) + 1 if weight_type == "log" else 2 ** (x ** 0.5 - 1), decimals=6)
    t[t == 255] = weight
    t[t == 0] = 1.0
    return t.unsqueeze(0)


def composed(refs, target, weight_type="log"):
    """The chain of one sample out of Pillow, scipy and torch stages: refs [R, H, W, 3], target [H, W, 3]."""
    masks = [scipy_filter(scipy_close5(pil_diff_mask(r, target))) for r in refs]
    inter = np.logical_and.reduce([m >= 128 for m in masks])
    if inter.sum() == 0:
        inter[:] = True
    mask_ds = scipy_close5(torch_pool8(np.where(inter, 255, 0).astype(np.uint8)))
    return mask_ds, torch_weight(mask_ds, weight_type)


def _planes(seed, shape, density):
    return np.where(np.random.default_rng(seed).random(shape) < density, 255, 0).astype(np.uint8)


# ---- E1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(1, 1), (7, 5), (37, 53)])
def test_grey_and_threshold_equal_pillow_on_random_pairs(H, W):
    g = np.random.default_rng(H * 100 + W)
    for k in range(4):
        ref = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        tgt = np.clip(ref.astype(int) + g.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8) if k % 2 else \
            g.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for thr in (1, 18, 200):
            assert np.array_equal(R.diff_mask(ref, tgt, thr), pil_diff_mask(ref, tgt, thr))


def test_grey_around_the_threshold_equals_pillow():
    ref, tgt, grey = R.grid_17_18_19()
    assert all((grey == v).sum() > 100 for v in (17, 18, 19))
    got = R.diff_mask(ref, tgt, 18)
    assert np.array_equal(got, pil_diff_mask(ref, tgt, 18)) and np.array_equal(got[0] == 255, grey >= 18)
    assert np.array_equal(R.diff_mask(tgt, ref, 18), got)                       # the difference is symmetric
    # mistake: `>` for `>=` -- the greys of exactly 18 go black
    assert not np.array_equal(R.diff_mask(ref, tgt, 18, strict=True), pil_diff_mask(ref, tgt, 18))


# ---- E2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (5, 5), (33, 31), (130, 70)])
@pytest.mark.parametrize("density", [0.02, 0.5, 0.98])
def test_closing_equals_scipy(shape, density):
    m = _planes(7, (2,) + shape, density)
    got = R.close5(m)
    for n in range(2):
        assert np.array_equal(got[n], scipy_close5(m[n]))
    assert np.all(got >= m)                                                     # a closing only adds


def test_closing_rejects_a_square_element_and_a_black_outside():
    # a black hole of the ellipse's own shape: the ellipse fits into it, so it stays open; the square does not, and fills it
    hole = np.full((1, 12, 12), 255, dtype=np.uint8)
    hole[0, 3:8, 4:9][R.ELLIPSE5] = 0
    assert R.close5(hole)[0].min() == 0
    assert np.array_equal(R.close5(hole)[0], scipy_close5(hole[0]))
    assert not np.array_equal(R.close5(hole, element=R.SQUARE5)[0], scipy_close5(hole[0]))
    # erosion that counts the outside as black eats the border of a full plane
    full = np.full((1, 9, 9), 255, dtype=np.uint8)
    assert np.array_equal(R.close5(full)[0], scipy_close5(full[0])) and R.close5(full).min() == 255
    assert not np.array_equal(R.close5(full, erode_outside=False)[0], scipy_close5(full[0]))


# ---- E3 -------------------------------------------------------------------------------------------------------------------------
def same_partition(a, b):
    """Two labellings name the same components: the map label -> label is a bijection on every pixel."""
    pairs = np.unique(np.stack([a.ravel(), b.ravel()], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


@pytest.mark.parametrize("density", [0.1, 0.4, 0.5, 0.6, 0.9])
def test_labelling_partition_equals_scipy(density):
    plane = _planes(int(density * 10), (41, 57), density) >= 128
    got, n = R.label_bfs(plane)
    want, m = ndimage.label(plane, structure=np.ones((3, 3), dtype=bool))
    assert n == m and same_partition(got, want) and np.array_equal(got > 0, plane)
    for shape in (R.serpentine(16, 16), R.spiral(17, 15)):
        assert R.label_bfs(shape >= 128)[1] == 1 == ndimage.label(shape >= 128, structure=np.ones((3, 3), dtype=bool))[1]
    assert int((R.serpentine(64, 64) >= 128).sum()) >= 64 * 64 // 2


def test_integer_keep_rule_equals_the_float64_one():
    """den * area >= num * total against area >= 0.3 * total: at a tie (area = 3k, total = 10k) the float64 product rounds to the
    integer 3k itself, so the component is kept by both; off a tie the two sides differ by at least 0.1."""
    g = np.random.default_rng(0)
    ks = np.concatenate([np.arange(1, 2000), g.integers(2000, (2 ** 31 - 1) // 10, 20000)])
    for k in ks:
        k = int(k)
        assert 0.3 * (10 * k) == 3 * k
        assert R.keep_int(3 * k, 10 * k) and R.keep_float(3 * k, 10 * k)
        assert not R.keep_int(3 * k - 1, 10 * k) and not R.keep_float(3 * k - 1, 10 * k)
        assert not R.keep_int(3 * k - 1, 10 * k + 1) and not R.keep_float(3 * k - 1, 10 * k + 1)
    total = g.integers(1, 2 ** 31 - 1, 20000)
    area = (total * g.random(20000) * 0.6).astype(np.int64)
    for a, t in zip(area, total):
        assert R.keep_int(a, t) == R.keep_float(a, t)
    for t in range(1, 300):
        for a in range(0, t + 1):
            assert R.keep_int(a, t) == R.keep_float(a, t)


def test_filter_equals_scipy_and_rejects_its_mistakes():
    for seed, density in ((1, 0.3), (2, 0.5), (3, 0.7)):
        m = _planes(seed, (2, 29, 43), density)
        got = R.filter_components(m)
        for n in range(2):
            assert np.array_equal(got[n], scipy_filter(m[n]))
    for k in (1, 7, 30):
        tie, below = R.blobs(3 * k, 7 * k), R.blobs(3 * k - 1, 7 * k + 1)
        assert np.array_equal(R.filter_components(tie[None])[0], scipy_filter(tie)) and np.array_equal(scipy_filter(tie), tie)
        got = R.filter_components(below[None])[0]
        assert np.array_equal(got, scipy_filter(below)) and int((got >= 128).sum()) == 7 * k + 1
    # mistake: 4-connectivity -- a diagonal chain is one component of 8-connectivity and 20 single pixels of 4-connectivity
    chain = np.zeros((24, 24), dtype=np.uint8)
    chain[np.arange(20), np.arange(20)] = 255
    chain[20:23, 0:3] = 255                                                      # 9 pixels: 9 / 29 is kept, 20 / 29 is kept
    assert np.array_equal(R.filter_components(chain[None])[0], scipy_filter(chain)) and np.array_equal(scipy_filter(chain), chain)
    assert not np.array_equal(R.filter_components(chain[None], connectivity=4)[0], scipy_filter(chain))
    # mistake: H * W as the denominator -- 40 and 60 white pixels of 960: both pass 0.3 of the white count, none 0.3 of the plane
    two = R.blobs(40, 60)
    assert np.array_equal(R.filter_components(two[None])[0], scipy_filter(two)) and np.array_equal(scipy_filter(two), two)
    assert not np.array_equal(R.filter_components(two[None], denominator="plane")[0], scipy_filter(two))


# ---- E4, E5 and the weight -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(8, 8), (15, 15), (100, 76), (96, 128)])
def test_and_pool_equals_torch_and_rejects_its_mistakes(H, W):
    a, b = _planes(1, (2, H, W), 0.02), _planes(2, (2, H, W), 0.9)
    a[1] = 0                                                                     # sample 1: an empty intersection
    masks = np.stack([a, b], 1)
    mask_ds, counts = R.and_pool8(masks)
    for s in range(2):
        inter = (a[s] >= 128) & (b[s] >= 128)
        assert counts[s, 0] == inter.sum()
        plane = np.where(inter if inter.any() else np.ones_like(inter), 255, 0).astype(np.uint8)
        assert np.array_equal(mask_ds[s], scipy_close5(torch_pool8(plane)))
        assert counts[s, 1] == (mask_ds[s] >= 128).sum()
    assert counts[1, 0] == 0 and mask_ds[1].min() == 255
    if H % 8:                                                                    # mistake: ceil sizes, against F.max_pool2d's own
        single = np.where((a[0] >= 128) & (b[0] >= 128), 255, 0).astype(np.uint8)
        assert R.and_pool8(single[None, None], close_pooled=False)[0][0].shape == torch_pool8(single).shape
        assert np.array_equal(R.and_pool8(single[None, None], close_pooled=False)[0][0], torch_pool8(single))
        assert R.and_pool8(single[None, None], ceil=True, close_pooled=False)[0][0].shape != torch_pool8(single).shape
    if H >= 96:
        ring = np.zeros((1, 1, H, W), dtype=np.uint8)
        ring[0, 0, 16:72, 16:72] = 255
        ring[0, 0, 40:48, 40:48] = 0                                             # one pooled pixel of hole
        want = scipy_close5(torch_pool8(ring[0, 0]))
        assert np.array_equal(R.and_pool8(ring)[0][0], want)
        assert not np.array_equal(R.and_pool8(ring, close_pooled=False)[0][0], want)   # mistake: the pooled closing left out


def test_weight_scalar_is_the_float32_torch_expression():
    differ = 0
    for count in range(1, 193):
        m = np.zeros(192, dtype=np.uint8)
        m[:count] = 255
        for kind in ("log", "exp"):
            want = torch_weight(m.reshape(12, 16), kind).max() if count < 192 else torch.tensor(1.0)
            got = R.weight_scalar(192, count, kind)
            assert got.dtype == torch.float32 and torch.equal(got, want.reshape(())), (count, kind)
            differ += int(not torch.equal(R.weight_scalar(192, count, kind, dtype=torch.float64), got))
    assert differ > 0                                                            # mistake: a float64 scalar lands on other float32 values
    with pytest.raises(NotImplementedError, match=r"Support log \| exp, but found lin"):
        R.weight_scalar(192, 3, "lin")
    assert torch.equal(R.weight_fill(np.array([[[255, 0]]], dtype=np.uint8), [2.5]), torch.tensor([[[[2.5, 1.0]]]]))


# ---- the chain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", [(96, 128), (100, 76)])
@pytest.mark.parametrize("kind", ["log", "exp"])
def test_chain_equals_the_composition(H, W, kind):
    ref, tgt = R.edit_pair(H, W, seed=H)
    ref2, _ = R.edit_pair(H, W, seed=H + 1)
    ref2 = np.where(np.arange(W)[None, :, None] < W // 2, ref2, ref)             # a second reference: differs on the left half too
    for refs in (ref[None], np.stack([ref, ref2])):
        mask_ds, weights = R.chain(refs[None], tgt[None], kind)
        want_mask, want_w = composed(refs, tgt, kind)
        assert np.array_equal(mask_ds[0], want_mask) and torch.equal(weights[0], want_w)
        assert 0 < (mask_ds >= 128).sum() < mask_ds.size and float(weights.max()) > 1.0
    # one reference: the repainted rectangle, pooled
    mask_ds, _ = R.chain(ref[None, None], tgt[None])
    box = np.zeros((H, W), dtype=np.uint8)
    box[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 255
    assert np.array_equal(mask_ds[0], scipy_close5(torch_pool8(box)))
    # identical pictures: reconstruction data, all white, weight 1
    mask_ds, weights = R.chain(ref[None, None], ref[None], kind)
    assert mask_ds.min() == 255 and torch.equal(weights, torch.ones_like(weights))
    assert np.array_equal(mask_ds[0], composed(ref[None], ref, kind)[0])


def test_chain_raises_and_shortcuts():
    ref, _ = R.edit_pair(96, 128, seed=5)
    tgt = ref.copy()
    tgt[40, 50:53] = ref[40, 50:53] ^ 0x80                                       # 3 pixels of 12288: ratio 0.00024
    with pytest.raises(ValueError, match="TOO SMALL mask_intersect_area_ratio"):
        R.chain(ref[None, None], tgt[None])
    with pytest.raises(ValueError, match="empty intersection"):
        R.chain(np.stack([ref, ref])[None], ref[None])
    with pytest.raises(NotImplementedError, match="found lin"):
        R.chain(ref[None, None], tgt[None], "lin")
    for kw in (dict(need_weight=False), dict()):
        refs = ref[None, None] if kw else np.empty((1, 0, 96, 128, 3), dtype=np.uint8)
        mask_ds, weights = R.chain(refs, tgt[None], **kw)
        assert mask_ds.shape == (1, 12, 16) and mask_ds.min() == 255 and torch.equal(weights, torch.ones(1, 1, 12, 16))
