"""numpy restatement of the edit-region weight stages (include/fk.h, E1 .. E5) and of the chain edit_region_weights runs.

Each function states the rule the HIP kernel is held to at every byte.  The keyword arguments that default to the rule's own
value (``connectivity=8``, ``element=ELLIPSE5``, ...) exist so that tests/test_edit_weights_ref.py can build each plausible
mistake and show that the comparison rejects it; nothing else passes them.
"""
from collections import deque

import numpy as np
import torch

ELLIPSE5 = np.array([[0, 0, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 1, 0, 0]], dtype=bool)
SQUARE5 = np.ones((5, 5), dtype=bool)
AREA_THRESHOLD = 0.001


def white(mask):
    return np.asarray(mask) >= 128


def diff_mask(ref, tgt, threshold=18, strict=False):
    """E1 on uint8 [..., 3] arrays."""
    d = np.abs(ref.astype(np.int64) - tgt.astype(np.int64))
    grey = (19595 * d[..., 0] + 38470 * d[..., 1] + 7471 * d[..., 2] + 32768) >> 16
    return np.where(grey > threshold if strict else grey >= threshold, 255, 0).astype(np.uint8)


def _morph(plane, element, dilate, outside):
    """One pass over a bool plane; ``outside`` is the value a position beyond the plane counts as."""
    H, W = plane.shape
    r = element.shape[0] // 2
    padded = np.full((H + 2 * r, W + 2 * r), outside, dtype=bool)
    padded[r:r + H, r:r + W] = plane
    out = np.zeros((H, W), dtype=bool) if dilate else np.ones((H, W), dtype=bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if element[dy + r, dx + r]:
                win = padded[r + dy:r + dy + H, r + dx:r + dx + W]
                out = (out | win) if dilate else (out & win)
    return out


def close5(mask, element=ELLIPSE5, erode_outside=True):
    """E2 on uint8 [N, H, W]: dilation (the outside adds nothing), then erosion (the outside takes nothing)."""
    out = np.empty(mask.shape, dtype=np.uint8)
    for n, plane in enumerate(white(mask)):
        out[n] = np.where(_morph(_morph(plane, element, True, False), element, False, erode_outside), 255, 0)
    return out


def label_bfs(plane, connectivity=8):
    """int32 labels of a bool plane, 0 on black, components numbered from 1 in raster order of their first pixel: a plain BFS."""
    H, W = plane.shape
    labels = np.zeros((H, W), dtype=np.int32)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connectivity == 8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    n = 0
    for y0 in range(H):
        for x0 in range(W):
            if not plane[y0, x0] or labels[y0, x0]:
                continue
            n += 1
            labels[y0, x0] = n
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and plane[yy, xx] and not labels[yy, xx]:
                        labels[yy, xx] = n
                        todo.append((yy, xx))
    return labels, n


def keep_int(area, total, num=3, den=10):
    return den * int(area) >= num * int(total)


def keep_float(area, total, threshold=0.3):
    """The reference's test, a float64 product."""
    return bool(area >= threshold * total)


def filter_components(mask, num=3, den=10, connectivity=8, denominator="white"):
    """E3 on uint8 [N, H, W]."""
    out = np.zeros(mask.shape, dtype=np.uint8)
    for n, plane in enumerate(white(mask)):
        labels, count = label_bfs(plane, connectivity)
        total = int(plane.sum()) if denominator == "white" else plane.size
        areas = np.bincount(labels.ravel(), minlength=count + 1)
        for lbl in range(1, count + 1):
            if keep_int(areas[lbl], total, num, den):
                out[n][labels == lbl] = 255
    return out


def and_pool8(masks, ceil=False, close_pooled=True):
    """E4 on uint8 [B, R, H, W] -> (mask_ds uint8 [B, h, w], counts int32 [B, 2])."""
    B, R, H, W = masks.shape
    inter = np.logical_and.reduce(white(masks), axis=1)
    counts = np.zeros((B, 2), dtype=np.int32)
    counts[:, 0] = inter.reshape(B, -1).sum(1)
    inter[counts[:, 0] == 0] = True
    h, w = (-(-H // 8), -(-W // 8)) if ceil else (H // 8, W // 8)
    padded = np.zeros((B, h * 8, w * 8), dtype=bool)
    hh, ww = min(H, h * 8), min(W, w * 8)
    padded[:, :hh, :ww] = inter[:, :hh, :ww]
    pooled = np.where(padded.reshape(B, h, 8, w, 8).any(axis=(2, 4)), 255, 0).astype(np.uint8)
    mask_ds = close5(pooled) if close_pooled else pooled
    counts[:, 1] = white(mask_ds).reshape(B, -1).sum(1)
    return mask_ds, counts


def weight_scalar(numel, count, weight_type="log", dtype=torch.float32):
    """get_weight's scalar: the reference's torch CPU expressions (float32; ``dtype`` only for the mistake of a float64 one)."""
    x = (numel / torch.tensor(count, dtype=torch.int64)).to(dtype)
    if weight_type == "log":
        weight = torch.log2(x) + 1
    elif weight_type == "exp":
        weight = 2 ** (x ** 0.5 - 1)
    else:
        raise NotImplementedError(f"Support log | exp, but found {weight_type}")
    return torch.round(weight, decimals=6).to(torch.float32)


def weight_fill(mask_ds, w):
    """E5: fp32 [B, 1, h, w]."""
    m = torch.from_numpy(white(mask_ds))[:, None]
    return torch.where(m, torch.as_tensor(w, dtype=torch.float32).view(-1, 1, 1, 1), torch.tensor(1.0))


def chain(refs, target, weight_type="log", need_weight=True, **mistakes):
    """edit_region_weights on uint8 arrays refs [B, R, H, W, 3], target [B, H, W, 3] -> (mask_ds uint8, weights fp32 tensor).
    ``mistakes``: strict=, element=, erode_outside=, connectivity=, denominator=, ceil=, close_pooled=, dtype= (see the module's
    docstring)."""
    if weight_type not in ("log", "exp"):
        raise NotImplementedError(f"Support log | exp, but found {weight_type}")
    B, R, H, W, _ = refs.shape
    pick = lambda *names: {k: mistakes[k] for k in names if k in mistakes}                          # noqa: E731
    if R == 0 or not need_weight:
        h, w = H // 8, W // 8
        return np.full((B, h, w), 255, dtype=np.uint8), torch.ones(B, 1, h, w)
    masks = np.empty((B, R, H, W), dtype=np.uint8)
    for r in range(R):
        m = diff_mask(refs[:, r], target, 18, **pick("strict"))
        m = close5(m, **pick("element", "erode_outside"))
        masks[:, r] = filter_components(m, 3, 10, **pick("connectivity", "denominator"))
    mask_ds, counts = and_pool8(masks, **pick("ceil", "close_pooled"))
    ws = []
    for b in range(B):
        ratio = np.float64(counts[b, 0]) / np.float64(H * W)
        if ratio < AREA_THRESHOLD:
            if ratio != 0.0:
                raise ValueError(f"TOO SMALL mask_intersect_area_ratio: {ratio}, sample {b}")
            if R != 1:
                raise ValueError(f"sample {b}: an empty intersection with {R} references")
        ws.append(weight_scalar(mask_ds[b].size, int(counts[b, 1]), weight_type, **pick("dtype")))
    return mask_ds, weight_fill(mask_ds, torch.stack(ws))


# ---- inputs the tests share ---------------------------------------------------------------------------------------------------
def edit_pair(H, W, seed, box=None, speckles=12, pinholes=12):
    """(reference, target) uint8 [H, W, 3]: the target is the reference with one repainted rectangle ``box`` = (y0, x0, y1, x1),
    isolated changed pixels outside it (speckles) and unchanged pixels inside it (pinholes)."""
    g = np.random.default_rng(seed)
    ref = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    tgt = ref.copy()
    y0, x0, y1, x1 = box if box is not None else (H // 4, W // 4, H // 4 + H // 2, W // 4 + W // 2)
    tgt[y0:y1, x0:x1] = ref[y0:y1, x0:x1] ^ 0x80                    # every channel moves by 128: grey 128
    for _ in range(pinholes):
        y, x = g.integers(y0 + 3, y1 - 3), g.integers(x0 + 3, x1 - 3)
        tgt[y, x] = ref[y, x]
    for _ in range(speckles):
        y, x = g.integers(0, H), g.integers(0, W)
        if not (y0 - 4 <= y < y1 + 4 and x0 - 4 <= x < x1 + 4):
            tgt[y, x] = ref[y, x] ^ 0x80
    return ref, tgt


def grid_17_18_19():
    """Every (d_R, d_G, d_B) of a grid whose grey is 17, 18 or 19, as a one-row pair of fewer than 4096 pixels (reference = d, target = 0)."""
    d = np.array([(r, g, b) for r in range(0, 64) for g in range(0, 36) for b in range(0, 256, 10)], dtype=np.int64)
    grey = (19595 * d[:, 0] + 38470 * d[:, 1] + 7471 * d[:, 2] + 32768) >> 16
    d = d[(grey >= 17) & (grey <= 19)].astype(np.uint8)
    return d[None], np.zeros_like(d)[None], grey[(grey >= 17) & (grey <= 19)]


def blobs(a, b, H=24, W=40):
    """Two separate blobs of exactly a and b pixels."""
    m = np.zeros((H, W), dtype=np.uint8)
    for area, x0 in ((a, 0), (b, W // 2)):
        rows, rest = divmod(area, W // 2 - 2)
        m[:rows, x0:x0 + W // 2 - 2] = 255
        m[rows, x0:x0 + rest] = 255
    return m


def serpentine(H, W):
    """A one-pixel path that fills every other row and turns at alternating ends: one component about H * W / 2 long."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0::2] = 255
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 255
    return m


def spiral(H, W):
    """A one-pixel path spiralling inward with a one-pixel gap between its turns."""
    m = np.zeros((H, W), dtype=np.uint8)
    inside = lambda y, x: 0 <= y < H and 0 <= x < W                                                 # noqa: E731

    def free(y, x, dy, dx):                                        # the next cell is black and so is the one behind it
        ny, nx = y + dy, x + dx
        return inside(ny, nx) and not m[ny, nx] and not (inside(ny + dy, nx + dx) and m[ny + dy, nx + dx])

    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 255
    for _ in range(H * W):
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy                                       # turn right
            if not free(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = 255
    return m
