"""numpy restatement of the two byte rules of csrc/resample.hip (include/fk.h states them), for the CPU and the GPU tests:

* ``resize`` / ``pass_u8``: Pillow's 8-bit antialiased resize, built on the tables of ``helpers.resample_coeffs`` -- horizontal pass
  into a uint8 intermediate, then the vertical pass, a pass whose axis keeps its size skipped; int64 accumulators, with the
  assertion that every one of them fits the kernels' int32;
* ``overlay``: ``fk_bytes_overlay_u8``'s integer blend.

Arrays are uint8 ``[..., H, W, C]``; a crop is crop-then-resize, i.e. ``resize(a[y0:y1, x0:x1], ...)``."""
import numpy as np

from gpt_image_edit_amd import helpers

BITS = helpers.RESAMPLE_PRECISION_BITS


def pass_u8(a, axis, n_out, filter):
    """One pass along ``axis`` (0: vertical, 1: horizontal) of uint8 [..., H, W, C]."""
    a = np.asarray(a)
    assert a.dtype == np.uint8 and a.ndim >= 3 and axis in (0, 1)
    ax = a.ndim - 3 + axis
    bounds, kk, _ = helpers.resample_coeffs(a.shape[ax], n_out, filter)
    bounds, kk = bounds.numpy(), kk.numpy().astype(np.int64)
    src = np.moveaxis(a, ax, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], dtype=np.uint8)
    for i in range(n_out):
        xmin, xmax = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << (BITS - 1)) + np.tensordot(kk[i, :xmax - xmin], src[xmin:xmax], axes=(0, 0))
        assert np.abs(acc).max(initial=0) < 1 << 31
        out[i] = np.clip(acc >> BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, ax))


def resize(a, out_h, out_w, filter):
    a = np.asarray(a)
    H, W = a.shape[-3], a.shape[-2]
    if W != out_w:
        a = pass_u8(a, 1, out_w, filter)
    if H != out_h:
        a = pass_u8(a, 0, out_h, filter)
    return a


def nearest(a, out_h, out_w):
    """The gather the feature stands beside: F.interpolate's nearest source index per axis."""
    a = np.asarray(a)
    H, W = a.shape[-3], a.shape[-2]
    rows = np.minimum(np.floor(np.arange(out_h, dtype=np.float32) * np.float32(H / out_h)).astype(np.int64), H - 1)
    cols = np.minimum(np.floor(np.arange(out_w, dtype=np.float32) * np.float32(W / out_w)).astype(np.int64), W - 1)
    return np.take(np.take(a, rows, axis=a.ndim - 3), cols, axis=a.ndim - 2)


def blend(a, r, o):
    """The overlay's value inside the box, elementwise on integer arrays: o at a == 0, r at a == 255, else
    (2 (a r + (255 - a) o) + 255) // 510."""
    a, r, o = (np.asarray(v).astype(np.int64) for v in (a, r, o))
    mixed = (2 * (a * r + (255 - a) * o) + 255) // 510
    return np.where(a == 0, o, np.where(a == 255, r, mixed)).astype(np.uint8)


def overlay(res, orig, alpha, box):
    """res uint8 [B, y1-y0, x1-x0, 3], orig uint8 [1 or B, H, W, 3], alpha uint8 [1 or B, H, W] or None -> uint8 [B, H, W, 3]."""
    res, orig = np.asarray(res), np.asarray(orig)
    x0, y0, x1, y1 = box
    B = res.shape[0]
    out = np.broadcast_to(orig, (B,) + orig.shape[1:]).copy()
    a = np.full((B,) + orig.shape[1:3], 255, dtype=np.uint8) if alpha is None else np.broadcast_to(np.asarray(alpha), (B,) + orig.shape[1:3])
    out[:, y0:y1, x0:x1] = blend(a[:, y0:y1, x0:x1, None], res, out[:, y0:y1, x0:x1])
    return out
