"""GPU: the five edit-weight stages against tests/edit_weights_ref.py, equal at every byte.  Every output lives between sentinel
guard bytes that must survive, and a refused call leaves its whole buffer untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_weights_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
TILE = 32                        # FK_MASK_CLOSE_TILE


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as o
    return o


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


def _noise(seed, shape, density):
    return np.where(np.random.default_rng(seed).random(shape) < density, 255, 0).astype(np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- E1 -------------------------------------------------------------------------------------------------------------------------
def _diff(ops, ref, tgt, thr=18):
    out = Guarded(ref.shape[:3], torch.uint8)
    ops.edit_diff_mask(_dev(ref), _dev(tgt), thr, out=out.t)
    torch.cuda.synchronize()
    assert out.intact()
    return out.t.cpu().numpy()


@pytest.mark.parametrize("N, H, W", [(1, 1, 1), (3, 7, 5), (3, 37, 53), (1, 64, 64)])
def test_diff_mask_equals_the_rule(ops, N, H, W):
    g = np.random.default_rng(H)
    ref = g.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    near = np.clip(ref.astype(int) + g.integers(-30, 31, ref.shape), 0, 255).astype(np.uint8)
    for tgt, thr in ((near, 18), (near, 1), (g.integers(0, 256, ref.shape, dtype=np.uint8), 18), (ref, 18), (ref, 0)):
        assert np.array_equal(_diff(ops, ref, tgt, thr), R.diff_mask(ref, tgt, thr))


def test_diff_mask_reads_a_reference_slice_in_place(ops):
    g = np.random.default_rng(3)
    refs = g.integers(0, 256, (3, 2, 37, 53, 3), dtype=np.uint8)                 # [B, R, H, W, 3]
    tgt = np.clip(refs[:, 0].astype(int) + g.integers(-30, 31, refs[:, 0].shape), 0, 255).astype(np.uint8)
    d_refs, d_tgt = _dev(refs), _dev(tgt)
    for r in range(2):
        out = Guarded((3, 37, 53), torch.uint8)
        ops.edit_diff_mask(d_refs[:, r], d_tgt, 18, out=out.t)                   # a view at the batch stride R * H * W * 3
        torch.cuda.synchronize()
        assert out.intact() and np.array_equal(out.t.cpu().numpy(), R.diff_mask(refs[:, r], tgt, 18))


def test_diff_mask_at_greys_17_18_19(ops):
    ref, tgt, grey = R.grid_17_18_19()
    got = _diff(ops, ref[None], tgt[None])
    assert np.array_equal(got[0, 0] == 255, grey >= 18) and np.array_equal(got, R.diff_mask(ref[None], tgt[None]))
    only = (grey == 17) | (grey == 18)                                           # a pair whose greys are all 17 or 18
    got = _diff(ops, ref[None][:, :, only], tgt[None][:, :, only])
    assert np.array_equal(got[0, 0] == 255, grey[only] == 18) and 0 < (got == 255).sum() < got.size


# ---- E2 -------------------------------------------------------------------------------------------------------------------------
def _close(ops, m):
    out = Guarded(m.shape, torch.uint8)
    ops.mask_close5(_dev(m), out=out.t)
    torch.cuda.synchronize()
    assert out.intact()
    return out.t.cpu().numpy()


@pytest.mark.parametrize("H, W", [(1, 1), (1, 9), (5, 5), (130, 70), (TILE - 1, TILE + 1), (TILE + 1, TILE - 1), (TILE, TILE),
                                  (2 * TILE + 1, 2 * TILE - 1)])
def test_close5_equals_the_rule(ops, H, W):
    for density in (0.02, 0.5, 0.98):
        m = _noise(H + W, (2, H, W), density)
        assert np.array_equal(_close(ops, m), R.close5(m)), density
    empty = np.zeros((1, H, W), dtype=np.uint8)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):                # one white pixel in a corner stays one pixel
        m = empty.copy()
        m[0, y, x] = 255
        assert np.array_equal(_close(ops, m), R.close5(m)) and np.array_equal(R.close5(m), m)
    hole = np.full((1, H, W), 255, dtype=np.uint8)
    hole[0, H // 2, W // 2] = 0                                                   # a single black hole is filled
    assert np.array_equal(_close(ops, hole), R.close5(hole)) and (R.close5(hole).min() == 255 or H * W == 1)
    full = np.full((1, H, W), 255, dtype=np.uint8)
    assert _close(ops, full).min() == 255 and _close(ops, empty).max() == 0       # a border neither erodes nor dilates


def test_close5_keeps_a_hole_the_ellipse_fits(ops):
    m = np.full((1, 40, 40), 255, dtype=np.uint8)
    m[0, 29:34, 30:35][R.ELLIPSE5] = 0                                            # across the tile edge at 32
    got = _close(ops, m)
    assert np.array_equal(got, R.close5(m)) and np.array_equal(got, m)


# ---- E3 -------------------------------------------------------------------------------------------------------------------------
def _filter(ops, m, num=3, den=10):
    """(bytes, status word): the workspace is guarded too."""
    N, H, W = m.shape
    out = Guarded(m.shape, torch.uint8)
    ws = Guarded((1 + N + 2 * N * H * W,), torch.int32)
    ops.mask_filter_components(_dev(m), num, den, out=out.t, ws=ws.t, check=True)
    torch.cuda.synchronize()
    assert out.intact() and ws.intact()
    return out.t.cpu().numpy(), int(ws.t[0])


def _u_shape(H, W):
    m = np.zeros((H, W), dtype=np.uint8)
    m[:, 2] = m[:, W - 3] = m[H - 1, 2:W - 2] = 255
    return m


def _diagonals(H):
    d = np.zeros((2, H, H), dtype=np.uint8)
    d[0, np.arange(H), np.arange(H)] = 255
    d[1, np.arange(H), H - 1 - np.arange(H)] = 255
    return d


def _checkerboard(H, W):
    return np.where((np.add.outer(np.arange(H), np.arange(W)) % 2) == 0, 255, 0).astype(np.uint8)


SHAPES = {
    "empty": lambda: np.zeros((1, 9, 13), dtype=np.uint8),
    "full": lambda: np.full((2, 33, 70), 255, dtype=np.uint8),
    "diagonals": lambda: _diagonals(67),
    "checkerboard": lambda: _checkerboard(37, 53)[None],
    "spiral": lambda: R.spiral(64, 64)[None],
    "serpentine": lambda: R.serpentine(64, 64)[None],
    "u": lambda: _u_shape(100, 70)[None],
    "noise": lambda: np.stack([_noise(s, (96, 160), d) for s, d in ((1, 0.4), (2, 0.5), (3, 0.6))]),
    "one_pixel_planes": lambda: np.array([255, 0, 255], dtype=np.uint8).reshape(3, 1, 1),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_filter_components_equals_the_rule(ops, name):
    m = SHAPES[name]()
    want = R.filter_components(m)
    got, status = _filter(ops, m)
    assert status == 0                                                            # the longest chains stay inside the bounds
    assert np.array_equal(got, want)
    again, status = _filter(ops, m)                                               # the same bytes from two launches
    assert status == 0 and np.array_equal(again, got)
    if name in ("diagonals", "checkerboard", "spiral", "serpentine", "u", "full"):
        assert np.array_equal(want, m)                                            # one component per plane: all of it is kept
    # a fraction that drops something on noise; 1 / 1 keeps a component only when it is the whole plane's white
    for num, den in ((1, 2), (1, 1), (0, 1)):
        assert np.array_equal(_filter(ops, m, num, den)[0], R.filter_components(m, num, den)), (num, den)


@pytest.mark.parametrize("k", [1, 7, 30])
def test_filter_components_at_the_tie(ops, k):
    tie, below = R.blobs(3 * k, 7 * k), R.blobs(3 * k - 1, 7 * k + 1)
    got, status = _filter(ops, np.stack([tie, below]))
    assert status == 0 and np.array_equal(got[0], tie)                            # 3 : 7 exactly: both kept
    assert np.array_equal(got, R.filter_components(np.stack([tie, below])))
    assert int((got[1] >= 128).sum()) == 7 * k + 1                                # 3k - 1 of 10k: dropped


def test_planes_never_connect(ops):
    m = np.zeros((3, 12, 20), dtype=np.uint8)
    m[0, -1, :] = 255                                                             # plane 0 ends in a white row
    m[1, 0, :] = 255                                                              # plane 1 begins with one
    m[1, 5:11, 3:18] = 255                                                        # and holds a larger blob: its first row is dropped
    m[2, 4, 4] = 255
    got, status = _filter(ops, m)
    want = R.filter_components(m)
    assert status == 0 and np.array_equal(got, want)
    assert got[0, -1].min() == 255 and got[1, 0].max() == 0 and got[2, 4, 4] == 255


def test_filter_components_in_place(ops):
    m = _noise(5, (2, 40, 56), 0.5)
    d = _dev(m)
    ops.mask_filter_components(d, out=d)
    assert np.array_equal(d.cpu().numpy(), R.filter_components(m))


def test_refusals_write_nothing(ops):
    m = _dev(_noise(1, (1, 16, 16), 0.5))
    out = Guarded((1, 16, 16), torch.uint8)
    ws = Guarded((1 + 1 + 2 * 256,), torch.int32)
    short = Guarded((1 + 1 + 2 * 256 - 1,), torch.int32)
    for call, text in ((lambda: ops.mask_filter_components(m, 3, 0, out=out.t, ws=ws.t), "keep 3 / 0"),
                       (lambda: ops.mask_filter_components(m, -1, 10, out=out.t, ws=ws.t), "keep -1 / 10"),
                       (lambda: ops.mask_filter_components(m, out=out.t, ws=short.t), "workspace of 2052 bytes"),
                       (lambda: ops.edit_diff_mask(torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device="cuda"),
                                                   torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device="cuda"), 300, out=out.t),
                        "threshold=300"),
                       (lambda: ops.mask_filter_components(m, out=out.t, ws=out.raw[GUARD:GUARD + 256].view(torch.int32)),
                        "workspace of 256 bytes"),
                       (lambda: ops.mask_close5(out.t, out=out.t), "dst must be a buffer of its own")):
        with pytest.raises(RuntimeError, match=text):
            call()
        torch.cuda.synchronize()
        assert out.untouched() and ws.untouched() and short.untouched()
    with pytest.raises(RuntimeError, match="fk_mask_and_pool8_u8: .*sides are 8..4096"):
        ops.mask_and_pool8(torch.zeros(1, 1, 8, 4104, dtype=torch.uint8, device="cuda"))


# ---- E4 -------------------------------------------------------------------------------------------------------------------------
def _pool(ops, masks, status=None):
    """(mask_ds, counts) as numpy: the three buffers the stage writes are framed by guard bytes."""
    B, _, H, W = masks.shape
    bufs = (Guarded((B, H // 8, W // 8), torch.uint8), Guarded((B, H // 8, W // 8), torch.uint8), Guarded((B, 2), torch.int32))
    mask_ds, counts = ops.mask_and_pool8(_dev(masks), status=status, out=tuple(b.t for b in bufs))
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs)
    assert mask_ds.data_ptr() == bufs[1].t.data_ptr() and counts.data_ptr() == bufs[2].t.data_ptr()
    return mask_ds.cpu().numpy(), counts.cpu().numpy()


@pytest.mark.parametrize("H, W", [(8, 8), (15, 15), (100, 76), (96, 128)])
@pytest.mark.parametrize("Rn", [1, 2])
def test_and_pool8_equals_the_rule(ops, H, W, Rn):
    a, b = _noise(H, (3, H, W), 0.03), _noise(W, (3, H, W), 0.9)
    a[1] = 0                                                                      # sample 1: empty, between two that are not
    a[2, H // 2, W // 2] = b[2, H // 2, W // 2] = 255
    masks = np.stack([a, b][:Rn], 1)
    mask_ds, counts = _pool(ops, masks)
    want_ds, want_counts = R.and_pool8(masks)
    assert mask_ds.shape == (3, H // 8, W // 8) and counts.dtype == np.int32
    assert np.array_equal(counts, want_counts) and np.array_equal(mask_ds, want_ds)
    plain_ds, plain_counts = ops.mask_and_pool8(_dev(masks))                      # the wrapper's own buffers: the same result
    assert np.array_equal(plain_ds.cpu().numpy(), want_ds) and np.array_equal(plain_counts.cpu().numpy(), want_counts)
    assert want_counts[1, 0] == 0 and want_ds[1].min() == 255 and want_counts[1, 1] == (H // 8) * (W // 8)
    assert want_counts[2, 0] > 0


def test_and_pool8_closes_the_pooled_mask_and_carries_the_status(ops):
    ring = np.zeros((1, 1, 96, 128), dtype=np.uint8)
    ring[0, 0, 16:72, 16:72] = 255
    ring[0, 0, 40:48, 40:48] = 0                                                  # one pooled pixel of hole: closed
    mask_ds, counts = _pool(ops, ring)
    want_ds, want_counts = R.and_pool8(ring)
    assert np.array_equal(mask_ds, want_ds) and want_ds[0, 5, 5] == 255
    assert np.array_equal(counts, want_counts) and want_counts[0, 1] == (want_ds == 255).sum() >= 49
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert np.array_equal(_pool(ops, ring, status)[1], want_counts)
    status[0] = 1                                                                 # a labelling that had reached a bound
    assert _pool(ops, ring, status)[1].tolist() == [[-1, -1]]


# ---- E5 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, h, w", [(1, 1, 1), (3, 12, 9), (2, 56, 56)])
def test_weight_fill_equals_torch_where(ops, B, h, w):
    m = _noise(h, (B, h, w), 0.5)
    wv = torch.tensor([1.0, 2.584963, 7.25][:B])
    out = Guarded((B, 1, h, w), torch.float32)
    ops.mask_weight_fill(_dev(m), wv.cuda(), out=out.t)
    torch.cuda.synchronize()
    want = torch.where(torch.from_numpy(m)[:, None] == 255, wv.view(B, 1, 1, 1), torch.tensor(1.0))
    assert out.intact() and torch.equal(out.t.cpu(), want)
