"""CPU: the host side of ``padding_mask_crop`` / ``mask_blur`` / ``overlay`` with ``ops`` and the models stubbed: every refusal,
that the default call issues the calls it always issued, the order of the new calls, how ``overlay=None`` resolves, ``crop_box`` on
the output, and the command-line flags.  The stubs record each ``ops`` call and return tensors of the right shape; the arithmetic is
tests/test_hip_mask_ops_kernels.py's and tests/test_hip_inpaint_overlay_pipeline.py's business."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref as R  # noqa: E402

from gpt_image_edit_amd import helpers, ops, pipeline  # noqa: E402

BF = torch.bfloat16
H, W = 64, 96               # the target
PH, PW = 128, 192           # the picture


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
    rec("image_to_u8", lambda img: torch.zeros(img.shape[0], img.shape[2], img.shape[3], 3, dtype=torch.uint8))
    rec("image_overlay", lambda img, orig, alpha, box: torch.zeros(img.shape[0], *orig.shape[1:], dtype=torch.uint8))
    rec("mask_blur", lambda m, sigma: m.clone())
    rec("mask_bbox", lambda m, thr=1: torch.tensor(R.bbox_numpy(m.numpy(), thr), dtype=torch.int32))
    for name in ("euler_step", "euler_inpaint_step", "scale_noise"):
        rec(name, lambda *a, **kw: None)
    pipe = pipeline.FluxKontextPipeline(_Transformer(), _Vae(), use_graph=False)
    g = torch.Generator().manual_seed(1)
    e = SimpleNamespace(pipe=pipe, calls=calls)
    e.pic = torch.randint(0, 256, (1, PH, PW, 3), generator=g, dtype=torch.uint8)
    e.mask = torch.zeros(PH, PW, dtype=torch.uint8)
    e.mask[40:70, 100:130] = 255
    e.kw = dict(prompt_embeds=torch.zeros(1, 8, 4096, dtype=BF), pooled_prompt_embeds=torch.zeros(1, 768, dtype=BF), height=H,
                width=W, num_inference_steps=2, max_area=H * W, _auto_resize=False, output_type="np_uint8")
    return e


def _names(calls):
    return [c[0] for c in calls]


def test_default_keywords_issue_the_calls_the_masked_edit_always_issued(env):
    env.pipe(image=env.pic, mask_image=env.mask, **env.kw)
    plain = list(env.calls)
    env.calls.clear()
    out = env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=None, mask_blur=0.0, overlay=None, **env.kw)
    assert env.calls == plain and out.crop_box is None
    assert _names(plain) == ["pixels_to_nhwc", "pixels_to_nhwc", "euler_inpaint_step", "euler_inpaint_step", "image_to_u8"]
    env.calls.clear()
    env.pipe(image=env.pic, mask_image=env.mask, overlay=False, **env.kw)          # an explicit "off" is the default path too
    assert env.calls == plain
    env.calls.clear()
    assert env.pipe(image=env.pic, **env.kw).crop_box is None                       # and the unmasked edit has the field
    assert _names(env.calls) == ["pixels_to_nhwc", "euler_step", "euler_step", "image_to_u8"]


def test_call_order_with_crop_blur_and_overlay(env):
    out = env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=8, mask_blur=2.0, overlay=True, **env.kw)
    box = helpers.mask_crop_box((100, 40, 130, 70), PW, PH, 8, W, H)
    assert box == (81, 32, 150, 78) and out.crop_box == box
    bh, bw = box[3] - box[1], box[2] - box[0]
    cond = (bh // 16 * 16, bw // 16 * 16)
    assert _names(env.calls) == ["mask_blur", "mask_bbox", "pixels_box_to_nhwc", "pixels_box_to_nhwc", "euler_inpaint_step",
                                 "euler_inpaint_step", "image_overlay"]
    u8 = ((1, PH, PW, 3), torch.uint8)
    m8 = ((1, PH, PW), torch.uint8)
    assert env.calls[0][1] == (m8, 2.0)
    assert env.calls[1][1] == (m8, 1)                                               # alpha >= 1
    assert env.calls[2][1] == (u8, box, *cond, 32, False)                           # the condition: the same crop, snapped
    assert env.calls[3][1] == (u8, box, H, W, 32, False)                            # the preserved picture at the target
    assert env.calls[6][1] == (((1, 3, H, W), BF), u8, m8, box)
    assert out.images.shape == (1, PH, PW, 3) and out.images.dtype == np.uint8 and out.latents.shape == (1, 24, 64)
    # `init_image`: the condition stays whole (today's gather), only the preserved picture is cropped
    env.calls.clear()
    other = torch.zeros(1, 80, 80, 3, dtype=torch.uint8)
    env.pipe(image=other, init_image=env.pic, mask_image=env.mask, padding_mask_crop=8, **env.kw)
    assert _names(env.calls) == ["mask_bbox", "pixels_to_nhwc", "pixels_box_to_nhwc", "euler_inpaint_step", "euler_inpaint_step",
                                 "image_overlay"]
    assert env.calls[1][1][:3] == (((1, 80, 80, 3), torch.uint8), 80, 80)
    # a box that snaps to the target's size: one crop serves as condition and as preserved picture
    env.calls.clear()
    big = torch.zeros(PH, PW, dtype=torch.uint8)
    big[10:80, 20:120] = 255
    out = env.pipe(image=env.pic, mask_image=big, padding_mask_crop=0, **env.kw)
    assert out.crop_box == (18, 10, 123, 80) and _names(env.calls).count("pixels_box_to_nhwc") == 1


def test_renorm_is_decided_on_the_box(env):
    pic = torch.full((1, PH, PW, 3), 200, dtype=torch.uint8)
    pic[0, 0, 0, 0] = 3                                                             # a dark byte outside the box
    env.pipe(image=pic, mask_image=env.mask, padding_mask_crop=8, **env.kw)
    assert [c[1][-1] for c in env.calls if c[0] == "pixels_box_to_nhwc"] == [True, True]
    env.calls.clear()
    pic[0, 50, 110, 1] = 127                                                        # ... and one inside it
    env.pipe(image=pic, mask_image=env.mask, padding_mask_crop=8, **env.kw)
    assert [c[1][-1] for c in env.calls if c[0] == "pixels_box_to_nhwc"] == [False, False]


def test_overlay_none_resolves_to_the_crop(env):
    def run(**kw):
        env.calls.clear()
        return env.pipe(**{**env.kw, "image": env.pic, "mask_image": env.mask, **kw})
    out = run(padding_mask_crop=8)                                                  # a crop is pasted back
    assert "image_overlay" in _names(env.calls) and out.images.shape == (1, PH, PW, 3)
    out = run(padding_mask_crop=8, overlay=False)                                   # unless the caller says no: the crop itself
    assert _names(env.calls)[-1] == "image_to_u8" and out.images.shape == (1, H, W, 3) and out.crop_box == (81, 32, 150, 78)
    out = run(padding_mask_crop=8, output_type="latent")                            # the crop's latents, nothing overlaid
    assert "image_overlay" not in _names(env.calls) and "image_to_u8" not in _names(env.calls)
    assert out.images.shape == (1, 24, 64) and out.crop_box == (81, 32, 150, 78)
    out = run(padding_mask_crop=8, overlay=False, output_type="pt_raw")
    assert tuple(out.images.shape) == (1, 3, H, W)
    out = run(overlay=True)                                                         # without a crop: the whole picture is the box
    assert env.calls[-1][0] == "image_overlay" and env.calls[-1][1][3] == (0, 0, PW, PH) and out.crop_box is None
    assert "mask_bbox" not in _names(env.calls) and "pixels_box_to_nhwc" not in _names(env.calls)
    assert out.images.shape == (1, PH, PW, 3)
    out = run(mask_blur=1.5)                                                        # a feather alone: no overlay, no read-back
    assert _names(env.calls)[0] == "mask_blur" and _names(env.calls)[-1] == "image_to_u8" and "mask_bbox" not in _names(env.calls)
    out = run(padding_mask_crop=8, output_type="pil")
    assert out.images[0].size == (PW, PH)
    # a float mask's bytes are rint(255 m)
    run(overlay=True, mask_image=(env.mask.float() / 255)[None, None])
    assert env.calls[-1][1][2] == ((1, PH, PW), torch.uint8)


def test_refusals(env):
    def bad(match, **kw):
        env.calls.clear()
        args = dict(env.kw, image=env.pic, mask_image=env.mask)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            env.pipe(**args)
        assert env.calls == [] or _names(env.calls) in (["mask_bbox"], ["mask_blur"], ["mask_blur", "mask_bbox"])   # nothing encoded
    for sigma in (64.5, 1000, -1.0, float("nan"), float("inf")):
        bad("mask_blur", mask_blur=sigma)
    for pad in (-1, 2.5, "8", True):
        bad("padding_mask_crop", padding_mask_crop=pad)
    bad("need `mask_image`", mask_image=None, padding_mask_crop=8)
    bad("need `mask_image`", mask_image=None, overlay=True)
    bad("need `mask_image`", mask_image=None, mask_blur=2.0)
    bad("is empty", mask_image=torch.zeros(PH, PW, dtype=torch.uint8), padding_mask_crop=8)
    # no bytes to keep: a float tensor or latents as the preserved picture
    flt = torch.zeros(1, 3, PH, PW)
    lat = torch.zeros(1, 16, H // 8, W // 8, dtype=BF)
    for pic in (flt, lat):
        bad("no bytes to keep", image=pic, padding_mask_crop=8)
        bad("no bytes to keep", image=pic, overlay=True)
        bad("no bytes to keep", init_image=pic, overlay=True)
    # sizes differ, in either mode
    small = torch.zeros(PH // 2, PW, dtype=torch.uint8)
    small[5:9, 5:9] = 255
    bad("at one size", mask_image=small, padding_mask_crop=8)
    bad("at one size", mask_image=small, overlay=True)
    # overlay with an output that is no uint8 picture
    for ot in ("pt", "np", "pt_raw", "latent"):
        bad("output_type", overlay=True, output_type=ot)
    for ot in ("pt", "np", "pt_raw"):
        bad("output_type", padding_mask_crop=8, output_type=ot)                     # overlay=None is "on" here
    bad("batch", image=torch.cat([env.pic] * 3), overlay=True)
    bad("picture to preserve", image=None, overlay=True)
    dot = torch.zeros(PH, PW, dtype=torch.uint8)
    dot[5, 5] = 255
    bad("smaller than one", mask_image=dot, padding_mask_crop=2)                    # an 8 x 5 box holds no 16-pixel token


def test_cli_flags(tmp_path):
    from PIL import Image
    from gpt_image_edit_amd.serve import cli
    base = ["--model_path", "m", "--flux_path", "f"]
    a = cli.build_parser().parse_args(base)
    assert (a.mask_crop_padding, a.mask_blur, a.overlay) == (None, 0.0, False) and cli.inpaint_kwargs(a) == {}
    Image.fromarray(np.zeros((8, 8), dtype=np.uint8)).save(tmp_path / "m.png")
    a = cli.build_parser().parse_args(base + ["--mask", str(tmp_path / "m.png")])
    assert set(cli.inpaint_kwargs(a)) == {"mask_image"}                             # nothing is passed at the defaults
    a = cli.build_parser().parse_args(base + ["--mask", str(tmp_path / "m.png"), "--mask_crop_padding", "0", "--mask_blur", "3.5",
                                              "--overlay"])
    kw = cli.inpaint_kwargs(a)
    assert kw["padding_mask_crop"] == 0 and kw["mask_blur"] == 3.5 and kw["overlay"] is True and "strength" not in kw
    a = cli.build_parser().parse_args(base + ["--mask", str(tmp_path / "m.png"), "--mask_crop_padding", "16"])
    assert cli.inpaint_kwargs(a)["padding_mask_crop"] == 16 and "overlay" not in cli.inpaint_kwargs(a)
    for flags in (["--overlay"], ["--mask_blur", "2"], ["--mask_crop_padding", "4"]):
        a = cli.build_parser().parse_args(base + ["--prompt_embeds", "e.pt"] + flags)
        with pytest.raises(SystemExit, match="go with --mask"):
            cli.main(a)
