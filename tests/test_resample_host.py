"""CPU: the host side of ``resample=`` with ``ops`` and the models stubbed (the pattern of tests/test_inpaint_overlay_host.py): the
refusals, that ``None`` / ``"nearest"`` issue the calls the pipeline always issued, the order and the arguments of the new calls for
the condition image, ``init_image``, a crop and the overlay, that the loop's graph key does not see the keyword, and the
command-line flag.  The stubs record each ``ops`` call; ``resample_u8`` answers with the numpy reference, so the bytes that decide the
second normalisation are real.  The kernels' arithmetic is tests/test_hip_resample_kernels.py's business."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref as M  # noqa: E402
import resample_ref as R  # noqa: E402

from gpt_image_edit_amd import helpers, ops, pipeline  # noqa: E402

BF = torch.bfloat16
H, W = 64, 96               # the target
PH, PW = 128, 192           # the picture
U8 = torch.uint8


class _Vae:
    config = SimpleNamespace(block_out_channels=(1, 2, 3, 4), latent_channels=16, shift_factor=0.1, scaling_factor=0.3)

    def encode(self, x, post_add=0.0, post_mul=1.0, nhwc=False):
        b, h, w = (x.shape[0], x.shape[1], x.shape[2]) if nhwc else (x.shape[0], x.shape[2], x.shape[3])
        lat = torch.zeros(b, 16, h // 8, w // 8, dtype=BF)
        return SimpleNamespace(latent_dist=SimpleNamespace(mode=lambda: lat))

    def decode(self, z, return_dict=False, pre_div=1.0, pre_add=0.0):
        return (torch.zeros(z.shape[0], 3, z.shape[2] * 8, z.shape[3] * 8, dtype=BF),)


class _Transformer:
    device = torch.device("cpu")
    config = SimpleNamespace(in_channels=64, guidance_embeds=True)

    def __call__(self, hidden_states=None, **kw):
        return (torch.zeros_like(hidden_states),)


@pytest.fixture
def env(monkeypatch):
    calls = []

    def rec(name, result):
        def f(*a, **kw):
            calls.append((name, tuple(x if not torch.is_tensor(x) else (tuple(x.shape), x.dtype) for x in a)))
            return result(*a, **kw)
        monkeypatch.setattr(ops, name, f)
    rec("pixels_to_nhwc", lambda u8, h, w, cpad=32, renorm=False: torch.zeros(u8.shape[0], h, w, cpad, dtype=BF))
    rec("pixels_box_to_nhwc", lambda u8, box, h, w, cpad=32, renorm=False: torch.zeros(u8.shape[0], h, w, cpad, dtype=BF))
    rec("image_to_u8", lambda img: torch.zeros(img.shape[0], img.shape[2], img.shape[3], 3, dtype=U8))
    rec("image_overlay", lambda img, orig, alpha, box: torch.zeros(img.shape[0], *orig.shape[1:], dtype=U8))
    rec("bytes_overlay", lambda res, orig, alpha, box: torch.zeros(res.shape[0], *orig.shape[1:], dtype=U8))
    rec("resample_u8", lambda v, h, w, f: torch.from_numpy(R.resize(v.numpy(), h, w, f)))
    rec("mask_blur", lambda m, sigma: m.clone())
    rec("mask_bbox", lambda m, thr=1: torch.tensor(M.bbox_numpy(m.numpy(), thr), dtype=torch.int32))
    for name in ("euler_step", "euler_inpaint_step", "scale_noise"):
        rec(name, lambda *a, **kw: None)
    pipe = pipeline.FluxKontextPipeline(_Transformer(), _Vae(), use_graph=False)
    g = torch.Generator().manual_seed(1)
    e = SimpleNamespace(pipe=pipe, calls=calls)
    e.pic = torch.randint(0, 256, (1, PH, PW, 3), generator=g, dtype=U8)
    e.mask = torch.zeros(PH, PW, dtype=U8)
    e.mask[40:70, 100:130] = 255
    e.kw = dict(prompt_embeds=torch.zeros(1, 8, 4096, dtype=BF), pooled_prompt_embeds=torch.zeros(1, 768, dtype=BF), height=H,
                width=W, num_inference_steps=2, max_area=H * W, _auto_resize=False, output_type="np_uint8")
    return e


def _names(calls):
    return [c[0] for c in calls]


def test_refusals(env):
    def bad(match, **kw):
        env.calls.clear()
        with pytest.raises(ValueError, match=match):
            env.pipe(**dict(env.kw, **kw))
        assert env.calls == []                                                      # before any work
    bad("`resample` is None", image=env.pic, resample="area")
    bad("`resample` is None", image=env.pic, resample="LANCZOS")
    bad("`resample` is None", image=env.pic, resample=3)
    flt = torch.zeros(1, 3, PH, PW)
    lat = torch.zeros(1, 16, H // 8, W // 8, dtype=BF)
    for f in ("bilinear", "bicubic", "lanczos"):
        bad("`image` is a float tensor or latents", image=flt, resample=f)
        bad("`image` is a float tensor or latents", image=lat, resample=f)
        bad("`init_image` is a float tensor or latents", image=env.pic, init_image=flt, mask_image=env.mask, resample=f)
        bad("`init_image` is a float tensor or latents", image=env.pic, init_image=lat, mask_image=env.mask, resample=f)
    env.pipe(image=flt, resample="nearest", **env.kw)                               # nearest is the float route's own resize
    env.pipe(image=None, resample="lanczos", **env.kw)                              # no picture: nothing to filter, nothing refused
    assert "resample_u8" not in _names(env.calls)


def test_none_and_nearest_are_todays_calls(env):
    for extra in (dict(image=env.pic), dict(image=env.pic, mask_image=env.mask),
                  dict(image=env.pic, mask_image=env.mask, padding_mask_crop=8, mask_blur=2.0),
                  dict(image=env.pic, init_image=env.pic, mask_image=env.mask, strength=0.5, overlay=True)):
        env.calls.clear()
        env.pipe(**env.kw, **extra)
        plain = list(env.calls)
        assert plain and "resample_u8" not in _names(plain) and "bytes_overlay" not in _names(plain)
        for value in (None, "nearest"):
            env.calls.clear()
            env.pipe(resample=value, **env.kw, **extra)
            assert env.calls == plain, (value, list(extra))


@pytest.mark.parametrize("f", ["bilinear", "bicubic", "lanczos"])
def test_condition_and_init_image(env, f):
    u8 = ((1, PH, PW, 3), U8)
    env.pipe(image=env.pic, resample=f, **env.kw)
    assert _names(env.calls) == ["resample_u8", "pixels_to_nhwc", "euler_step", "euler_step", "image_to_u8"]
    assert env.calls[0][1] == (u8, PH, PW, f)                                       # a multiple of 16: the snap keeps the size
    assert env.calls[1][1][:3] == (u8, PH, PW)
    env.calls.clear()
    odd = torch.zeros(1, 150, 203, 3, dtype=U8)
    env.pipe(image=odd, resample=f, **env.kw)
    assert env.calls[0] == ("resample_u8", (((1, 150, 203, 3), U8), 144, 192, f))
    assert env.calls[1][1][:3] == (((1, 144, 192, 3), U8), 144, 192)                # the gather at equal size: an identity
    # a masked edit: the condition to its snapped size, the preserved picture to the target's
    env.calls.clear()
    env.pipe(image=odd, init_image=env.pic, mask_image=env.mask, strength=0.5, resample=f, **env.kw)
    assert _names(env.calls) == ["resample_u8", "pixels_to_nhwc", "resample_u8", "pixels_to_nhwc", "scale_noise", "euler_inpaint_step",
                                 "image_to_u8"]
    assert env.calls[2][1] == (u8, H, W, f) and env.calls[3][1][:3] == (((1, H, W, 3), U8), H, W)
    # `image` alone stands in as the preserved picture: resized once more, to the target
    env.calls.clear()
    env.pipe(image=env.pic, mask_image=env.mask, resample=f, **env.kw)
    assert _names(env.calls)[:4] == ["resample_u8", "pixels_to_nhwc", "resample_u8", "pixels_to_nhwc"]
    assert env.calls[0][1] == (u8, PH, PW, f) and env.calls[2][1] == (u8, H, W, f)


def test_crop_and_overlay(env):
    f = "lanczos"
    out = env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=8, mask_blur=2.0, resample=f, **env.kw)
    box = helpers.mask_crop_box((100, 40, 130, 70), PW, PH, 8, W, H)
    assert box == (81, 32, 150, 78) and out.crop_box == box
    bh, bw = box[3] - box[1], box[2] - box[0]
    cond = (bh // 16 * 16, bw // 16 * 16)
    assert _names(env.calls) == ["mask_blur", "mask_bbox", "resample_u8", "pixels_to_nhwc", "resample_u8", "pixels_to_nhwc",
                                 "euler_inpaint_step", "euler_inpaint_step", "image_to_u8", "resample_u8", "bytes_overlay"]
    view = ((1, bh, bw, 3), U8)                                                     # the box's view of the picture, no box argument
    assert env.calls[2][1] == (view, *cond, f) and env.calls[3][1][:3] == (((1, *cond, 3), U8), *cond)
    assert env.calls[4][1] == (view, H, W, f) and env.calls[5][1][:3] == (((1, H, W, 3), U8), H, W)
    assert env.calls[9][1] == (((1, H, W, 3), U8), bh, bw, f)                       # the decode's bytes to the box's size
    assert env.calls[10][1] == (((1, bh, bw, 3), U8), ((1, PH, PW, 3), U8), ((1, PH, PW), U8), box)
    assert "pixels_box_to_nhwc" not in _names(env.calls) and "image_overlay" not in _names(env.calls)
    assert out.images.shape == (1, PH, PW, 3) and out.images.dtype == np.uint8
    # an overlay without a crop: the box is the whole picture
    env.calls.clear()
    out = env.pipe(image=env.pic, mask_image=env.mask, overlay=True, resample=f, **env.kw)
    assert env.calls[-2][1] == (((1, H, W, 3), U8), PH, PW, f) and env.calls[-1][1][3] == (0, 0, PW, PH) and out.crop_box is None
    # "latent" returns the crop's latents: nothing behind the decode
    env.calls.clear()
    env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=8, resample=f, **dict(env.kw, output_type="latent"))
    assert _names(env.calls).count("resample_u8") == 2 and "bytes_overlay" not in _names(env.calls)


def test_renorm_is_decided_on_the_resized_bytes(env):
    """Every byte of the box is >= 128, but the box holds an edge between 128 and 255: lanczos undershoots below 128 beside it, so
    the resized crop is not normalised a second time, where the point-sampled crop is."""
    pic = torch.full((1, PH, PW, 3), 128, dtype=U8)
    pic[:, :, 115:] = 255
    env.pipe(image=pic, mask_image=env.mask, padding_mask_crop=8, **env.kw)
    assert [c[1][-1] for c in env.calls if c[0] == "pixels_box_to_nhwc"] == [True, True]
    env.calls.clear()
    env.pipe(image=pic, mask_image=env.mask, padding_mask_crop=8, resample="lanczos", **env.kw)
    assert [c[1][-1] for c in env.calls if c[0] == "pixels_to_nhwc"] == [False, False]
    env.calls.clear()
    env.pipe(image=pic, mask_image=env.mask, padding_mask_crop=8, resample="bilinear", **env.kw)      # no overshoot: still >= 128
    assert [c[1][-1] for c in env.calls if c[0] == "pixels_to_nhwc"] == [True, True]


def test_the_graph_key_does_not_see_the_keyword(env, monkeypatch):
    keys = []
    real = env.pipe._denoise
    monkeypatch.setattr(env.pipe, "_denoise", lambda L, *a, **kw: keys.append(env.pipe._graph_key(L)) or real(L, *a, **kw))
    monkeypatch.setattr(ops, "launch_config_epoch", lambda: 0)
    same = torch.zeros(1, PH, PW, 3, dtype=U8)
    for value in (None, "nearest", "bilinear", "lanczos"):
        env.pipe(image=same, resample=value, **env.kw)
    assert len(keys) == 4 and all(k == keys[0] for k in keys)


def test_cli_flag():
    from gpt_image_edit_amd.eval import gen_samples
    from gpt_image_edit_amd.serve import cli
    base = ["--model_path", "m", "--flux_path", "f"]
    a = cli.build_parser().parse_args(base)
    assert a.resample == "nearest" and cli.resample_kwargs(a) == {}
    for f in ("bilinear", "bicubic", "lanczos"):
        a = cli.build_parser().parse_args(base + ["--resample", f])
        assert cli.resample_kwargs(a) == {"resample": f}
    assert cli.resample_kwargs(cli.build_parser().parse_args(base + ["--resample", "nearest"])) == {}
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--resample", "area"])
    assert cli.resample_kwargs(SimpleNamespace()) == {}                             # a caller's own namespace without the flag
    g = gen_samples.build_parser().parse_args(base + ["--gedit_prompt_path", "p", "--output_dir", "o", "--resample", "lanczos"])
    assert cli.resample_kwargs(g) == {"resample": "lanczos"}
