"""The per-pixel loss weights of an edit sample, made on the device from the (reference pictures, target picture) bytes.

The reference's stage-1 and stage-2 configs set ``mask_weight_type: 'log'``: the loss of a sample is multiplied by a map that
weighs the edited region by ``log2(picture area / edited area) + 1`` (univa/utils/get_mask.py: get_weight_mask).  This module is
the producer of ``DenoiserTrainStep.forward_backward(area_mask_weights=)``.  The pixel work is five HIP stages (include/fk.h,
E1 .. E5); what stays here is the reference's scalar bookkeeping on the one pair of counts per sample that is read back.
"""
import numpy as np
import torch

from . import ops

AREA_THRESHOLD = 0.001      # get_weight_mask: a smaller, non-empty intersection is refused
DIFF_THRESHOLD = 18         # get_mask(..., threshold=18)
KEEP = (3, 10)              # filter_small_components(area_threshold=0.3), as an integer fraction


def _read_back(counts):
    """The call's one device -> host copy: int32 [B, 2], 8 B bytes."""
    return counts.cpu()


def _as_u8(pic, what):
    a = np.asarray(pic)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{what} must be an RGB picture of bytes [H, W, 3], not {a.dtype} {a.shape}")
    return torch.from_numpy(np.array(a, order="C"))             # a copy: a PIL image's array is read-only


def _from_lists(refs, target, device):
    if not isinstance(refs, (list, tuple)) or len(refs) != len(target) or len(target) == 0:
        raise ValueError("refs and target must be lists with one entry per sample")
    tgt = [_as_u8(t, "a target") for t in target]
    per = [[_as_u8(r, "a reference") for r in sample] for sample in refs]
    R, shape = len(per[0]), tgt[0].shape
    if any(len(s) != R for s in per):
        raise ValueError("every sample must have the same number of references")
    if any(p.shape != shape for p in tgt) or any(p.shape != shape for s in per for p in s):
        raise ValueError("all pictures of a call must have one size")
    target = torch.stack(tgt).to(device)
    if R == 0:
        return torch.empty((len(tgt), 0) + tuple(shape), dtype=torch.uint8, device=device), target
    return torch.stack([torch.stack(s) for s in per]).to(device), target


def weight_scalar(numel, white, weight_type):
    """get_weight's scalar, in the reference's own torch CPU expressions (float32)."""
    x = numel / torch.tensor(white, dtype=torch.int64)
    if weight_type == "log":
        weight = torch.log2(x) + 1
    elif weight_type == "exp":
        weight = 2 ** (x ** 0.5 - 1)
    else:
        raise NotImplementedError(f"Support log | exp, but found {weight_type}")
    return torch.round(weight, decimals=6)


def edit_region_weights(refs, target, weight_type="log", need_weight=True, device="cuda"):
    """(mask_ds uint8 [B, H // 8, W // 8], weights fp32 [B, 1, H // 8, W // 8]) on the device.

    ``refs`` uint8 [B, R, H, W, 3] and ``target`` uint8 [B, H, W, 3] on the device -- or, per sample, a list of R PIL images /
    numpy arrays and one target picture, all of one size, which are uploaded to ``device``.  Per reference: the difference mask
    at grey 18, its closing with the 5 x 5 ellipse, its components of at least 3 / 10 of the white pixels; then the AND over the
    references, the all-white plane for an empty intersection of a single reference (reconstruction data), the 8 x 8 max pool and
    its closing.  One stream, one read-back (the two counts per sample), from which the reference's scalars follow: an
    intersection of less than 0.001 of the picture raises ValueError, the weight is ``log2(x) + 1`` ("log") or
    ``2 ** (sqrt(x) - 1)`` ("exp") of x = pooled pixels / white pooled pixels, rounded to 6 decimals.  R == 0 (text-to-image) and
    ``need_weight=False`` give the all-white mask and weights of exactly 1."""
    if weight_type not in ("log", "exp"):
        raise NotImplementedError(f"Support log | exp, but found {weight_type}")
    if isinstance(target, (list, tuple)):
        refs, target = _from_lists(refs, target, device)
    if not (torch.is_tensor(refs) and torch.is_tensor(target)) or refs.dtype != torch.uint8 or target.dtype != torch.uint8:
        raise ValueError("refs / target must be uint8 tensors [B, R, H, W, 3] / [B, H, W, 3] or per-sample lists of pictures")
    if target.dim() != 4 or target.shape[3] != 3 or refs.dim() != 5 or refs.shape[0] != target.shape[0] \
            or tuple(refs.shape[2:]) != tuple(target.shape[1:]):
        raise ValueError(f"refs {tuple(refs.shape)} / target {tuple(target.shape)} are not [B, R, H, W, 3] / [B, H, W, 3]")
    B, H, W, _ = target.shape
    R = refs.shape[1]
    if B < 1 or H < 8 or W < 8 or H > 4096 or W > 4096:
        raise ValueError(f"edit_region_weights: {B} pictures of {H} x {W}: sides are 8..4096")
    h, w = H // 8, W // 8
    dev = target.device
    if R == 0 or not need_weight:
        return (torch.full((B, h, w), 255, dtype=torch.uint8, device=dev), torch.ones((B, 1, h, w), dtype=torch.float32, device=dev))
    refs, target = refs.contiguous(), target.contiguous()
    diff = torch.empty((R, B, H, W), dtype=torch.uint8, device=dev)           # reference-major: each reference's slab is contiguous
    for r in range(R):
        ops.edit_diff_mask(refs[:, r], target, DIFF_THRESHOLD, out=diff[r])    # read in place, at the batch stride of refs
    planes = diff.view(R * B, H, W)
    closed = ops.mask_close5(planes)
    ws = ops.mask_components_ws(R * B, H, W, dev)
    kept = ops.mask_filter_components(closed, KEEP[0], KEEP[1], out=closed, ws=ws, check=False)
    masks = kept.view(R, B, H, W).permute(1, 0, 2, 3).contiguous()
    mask_ds, counts = ops.mask_and_pool8(masks, status=ws)
    counts = _read_back(counts)
    scalars = []
    for b in range(B):
        inter, white = int(counts[b, 0]), int(counts[b, 1])
        if inter < 0:
            raise RuntimeError("edit_region_weights: fk_mask_filter_components_u8 reached a loop bound (FK_EBOUND)")
        ratio = np.float64(inter) / np.float64(H * W)
        if ratio < AREA_THRESHOLD:
            if ratio != 0.0:
                raise ValueError(f"TOO SMALL mask_intersect_area_ratio: {ratio}, sample {b}")
            if R != 1:
                raise ValueError(f"sample {b}: an empty intersection is reconstruction data, which has one reference, not {R}")
        if white <= 0:
            raise ValueError(f"sample {b}: the pooled mask is empty")
        scalars.append(weight_scalar(h * w, white, weight_type))
    wvec = torch.stack(scalars).to(dtype=torch.float32).to(dev)
    return mask_ds, ops.mask_weight_fill(mask_ds, wvec)
