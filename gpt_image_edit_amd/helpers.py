"""Host-side index helpers of the FLUX-Kontext pipeline driver (product code, runs on any device).

Same behaviour as the static helpers of the reference's ``FluxKontextPipeline``
(``univa/utils/flux_pipeline.py:106-116, 561-598``) -- training code calls them directly
(``train_denoiser.py:925,1009,1021,1098``) so the names and argument orders are kept.
Checked against golden vectors produced by the reference itself (tests/golden/helpers.npz).
"""
import math

import torch

# (width, height) pairs, univa/utils/flux_pipeline.py:85-103
PREFERRED_KONTEXT_RESOLUTIONS = [
    (672, 1568), (688, 1504), (720, 1456), (752, 1392), (800, 1328), (832, 1248), (880, 1184),
    (944, 1104), (1024, 1024), (1104, 944), (1184, 880), (1248, 832), (1328, 800), (1392, 752),
    (1456, 720), (1504, 688), (1568, 672),
]


def calculate_shift(image_seq_len, base_seq_len=256, max_seq_len=4096, base_shift=0.5, max_shift=1.15):
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    return image_seq_len * m + (base_shift - m * base_seq_len)


def _prepare_latent_image_ids(batch_size, height, width, device, dtype):
    ids = torch.zeros(height, width, 3)
    ids[..., 1] += torch.arange(height)[:, None]
    ids[..., 2] += torch.arange(width)[None, :]
    return ids.reshape(height * width, 3).to(device=device, dtype=dtype)


def _pack_latents(latents, batch_size, num_channels_latents, height, width):
    x = latents.view(batch_size, num_channels_latents, height // 2, 2, width // 2, 2)
    x = x.permute(0, 2, 4, 1, 3, 5)
    return x.reshape(batch_size, (height // 2) * (width // 2), num_channels_latents * 4)


def _unpack_latents(latents, height, width, vae_scale_factor):
    batch_size, _, channels = latents.shape
    height = 2 * (int(height) // (vae_scale_factor * 2))
    width = 2 * (int(width) // (vae_scale_factor * 2))
    x = latents.view(batch_size, height // 2, width // 2, channels // 4, 2, 2)
    x = x.permute(0, 3, 1, 4, 2, 5)
    return x.reshape(batch_size, channels // 4, height, width)


def fit_to_max_area(height, width, max_area, multiple_of):
    """Resolution fix-up at the top of the pipeline call (flux_pipeline.py:877-885)."""
    aspect = width / height
    w = round((max_area * aspect) ** 0.5)
    h = round((max_area / aspect) ** 0.5)
    return h // multiple_of * multiple_of, w // multiple_of * multiple_of


def preferred_condition_size(image_height, image_width, multiple_of, auto_resize=True):
    """Condition-image size selection (flux_pipeline.py:960-970)."""
    if auto_resize:
        aspect = image_width / image_height
        _, image_width, image_height = min((abs(aspect - w / h), w, h) for w, h in PREFERRED_KONTEXT_RESOLUTIONS)
    return image_height // multiple_of * multiple_of, image_width // multiple_of * multiple_of


def strength_t_start(num_inference_steps, strength):
    """First step of the ``num_inference_steps``-step schedule an edit of the given ``strength`` runs (diffusers'
    ``get_timesteps``): 1.0 = all of them, from pure noise; smaller values start later, from the re-noised picture."""
    if not 0.0 < float(strength) <= 1.0:
        raise ValueError(f"The value of strength should be in (0, 1] but is {strength}")
    init_timestep = min(num_inference_steps * float(strength), num_inference_steps)
    return int(max(num_inference_steps - init_timestep, 0))


MASK_BLUR_MAX_SIGMA = 64.0      # R = ceil(3 sigma) <= 192 = FK_MASK_BLUR_MAX_RADIUS (include/fk.h)


def gaussian_taps(sigma):
    """The 2R + 1 taps of the mask feather (fk_mask_blur_u8), R = ceil(3 sigma): float64 exp(-k^2 / (2 sigma^2)) divided by their
    float64 sum, rounded to fp32.  Symmetric; they sum to 1 within (2R + 1) * 2^-24."""
    sigma = float(sigma)
    if not 0.0 < sigma <= MASK_BLUR_MAX_SIGMA:
        raise ValueError(f"`mask_blur` is a sigma in (0, {MASK_BLUR_MAX_SIGMA:g}] pixels, not {sigma}")
    R = int(math.ceil(3.0 * sigma))
    w = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-R, R + 1)]
    total = math.fsum(w)
    return torch.tensor([v / total for v in w], dtype=torch.float64).to(torch.float32)


FK_RESAMPLE_MAX_KSIZE = 513     # include/fk.h: lanczos down to 1/85, bicubic to 1/128, bilinear to 1/256
RESAMPLE_PRECISION_BITS = 22    # coefficients are fixed point with 22 fractional bits; 2^21 rounds the shifted sum


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(x * math.pi) / (x * math.pi)


def _bilinear_filter(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic_filter(x):
    a, x = -0.5, abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos_filter(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


RESAMPLE_FILTERS = {"bilinear": (_bilinear_filter, 1.0), "bicubic": (_bicubic_filter, 2.0), "lanczos": (_lanczos_filter, 3.0)}
_resample_cache = {}


def resample_coeffs(n_in, n_out, filter):
    """The tables of one pass of Pillow's 8-bit antialiased resize along an axis of ``n_in`` samples resized to ``n_out``
    (include/fk.h: fk_resample_pass_u8 states the rule): ``(bounds, kk, ksize)`` with ``bounds`` int32 [n_out, 2] holding
    ``(xmin, xmax)`` of each output's source window and ``kk`` int32 [n_out, ksize] its fixed-point weights (2^22 = 1), zero past
    ``xmax - xmin``.  Float64 on the host, operation by operation in the rule's order (the sum of the weights in ascending tap
    order; ``math.sin``, not a vector library's); cached, so the tensors are shared: do not write to them.  Raises when the window
    is wider than ``FK_RESAMPLE_MAX_KSIZE`` or when a row's weights could overflow the kernels' int32 accumulator."""
    n_in, n_out = int(n_in), int(n_out)
    if filter not in RESAMPLE_FILTERS:
        raise ValueError(f"`filter` is one of {sorted(RESAMPLE_FILTERS)}, not {filter!r}")
    if n_in <= 0 or n_out <= 0:
        raise ValueError(f"cannot resample {n_in} samples to {n_out}")
    key = (n_in, n_out, filter)
    if key in _resample_cache:
        return _resample_cache[key]
    f, filter_support = RESAMPLE_FILTERS[filter]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = filter_support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    if ksize > FK_RESAMPLE_MAX_KSIZE:
        raise ValueError(f"{filter} from {n_in} to {n_out} samples needs windows of {ksize} taps: more than "
                         f"FK_RESAMPLE_MAX_KSIZE = {FK_RESAMPLE_MAX_KSIZE}")
    ss = 1.0 / fs
    one = 1 << RESAMPLE_PRECISION_BITS
    bounds = torch.zeros((n_out, 2), dtype=torch.int32)
    kk = torch.zeros((n_out, ksize), dtype=torch.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [f((t + xmin - center + 0.5) * ss) for t in range(xmax - xmin)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        row = [int(v * one - 0.5) if v < 0 else int(v * one + 0.5) for v in w]
        if 255 * sum(abs(v) for v in row) + (one >> 1) >= 1 << 31:
            raise ValueError(f"{filter} from {n_in} to {n_out} samples: the weights of output {i} overflow an int32 sum")
        bounds[i, 0], bounds[i, 1] = xmin, xmax
        kk[i, :len(row)] = torch.tensor(row, dtype=torch.int32)
    _resample_cache[key] = (bounds, kk, ksize)
    return _resample_cache[key]


def _grow(lo, hi, want, limit):
    """[lo, hi) grown to `want` samples about its centre (the odd one to the far side), shifted back inside [0, limit) and, if it
    is still larger, clamped to it."""
    grow = max(want - (hi - lo), 0)
    lo, hi = lo - grow // 2, hi + (grow - grow // 2)
    if lo < 0:
        lo, hi = 0, hi - lo
    if hi > limit:
        lo, hi = lo - (hi - limit), limit
    return max(lo, 0), hi


def mask_crop_box(bbox, W, H, pad, target_w, target_h):
    """The box a cropped masked edit works on (diffusers' ``get_crop_region``, restated in integer arithmetic): the mask's bounding
    box ``(x0, y0, x1, y1)`` (exclusive ends) padded by ``pad`` and clamped to the W x H picture; then the side that is short for
    the target's aspect grows until ``bw * target_h`` and ``bh * target_w`` are as close as integers allow; then the box is shifted
    back inside the picture.  A box that is still larger than the picture is clamped: its aspect then differs from the target's,
    and the resize stretches."""
    x0, y0, x1, y1 = (int(v) for v in bbox)
    W, H, pad, target_w, target_h = int(W), int(H), int(pad), int(target_w), int(target_h)
    if x1 <= x0 or y1 <= y0:
        raise ValueError("the mask is empty: there is no box to crop to")
    if pad < 0 or min(W, H, target_w, target_h) <= 0 or x0 < 0 or y0 < 0 or x1 > W or y1 > H:
        raise ValueError(f"bad crop arguments: bbox {(x0, y0, x1, y1)} in a {W} x {H} picture, pad {pad}")
    x0, y0, x1, y1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x1 + pad, W), min(y1 + pad, H)
    bw, bh = x1 - x0, y1 - y0
    if bw * target_h < bh * target_w:       # narrow for the target: the width that brings bw * target_h nearest bh * target_w
        x0, x1 = _grow(x0, x1, (2 * bh * target_w + target_h) // (2 * target_h), W)
    elif bw * target_h > bh * target_w:
        y0, y1 = _grow(y0, y1, (2 * bw * target_h + target_w) // (2 * target_w), H)
    return x0, y0, x1, y1
