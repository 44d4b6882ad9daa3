"""GPU: ``padding_mask_crop`` / ``mask_blur`` / ``overlay`` through ``FluxKontextPipeline`` on the tiny model of
``test_hip_inpaint_pipeline.py`` (1 double + 2 single blocks, 64 x 96 target, uint8 pictures up to 128 x 192).  Everything in
front of the first step and behind the decode is specified exactly, so the pipeline is held to bit equality with the same work done
through the public ops and the plain masked call."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, W = 2, 64, 96
HL, WL = H // 8, W // 8
PH, PW = 128, 192
PAD = 8


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    from gpt_image_edit_amd.vae import HipAutoencoderKL
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2)
    tr = HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=21)
    vae = HipAutoencoderKL(device="cuda", init="synthetic", seed=22)
    g = torch.Generator().manual_seed(31)
    e = SimpleNamespace(pipe=FluxKontextPipeline(tr, vae, use_graph=False), graphed=FluxKontextPipeline(tr, vae, use_graph=True))
    e.pic = torch.randint(0, 256, (1, PH, PW, 3), generator=g, dtype=torch.uint8)      # the big picture, one for the batch
    e.small = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)      # a picture of the target's size
    e.mask = torch.zeros(PH, PW, dtype=torch.uint8)
    e.mask[40:70, 100:130] = 255
    e.mask2 = torch.zeros(PH, PW, dtype=torch.uint8)                                   # the same extent elsewhere: the same box size
    e.mask2[30:60, 80:110] = 255
    e.small_mask = torch.zeros(H, W, dtype=torch.uint8)
    e.small_mask[:, :40] = 255                                                         # the edge sits on latent column 5
    emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    noise = e.pipe._pack_latents(torch.randn(B, 16, HL, WL, generator=g).to(BF), B, 16, HL, WL).contiguous().cuda()
    e.kw = dict(prompt_embeds=emb, pooled_prompt_embeds=pooled, height=H, width=W, guidance_scale=4.0, latents=noise,
                num_inference_steps=3, max_area=H * W, _auto_resize=False, output_type="np_uint8")
    return e


def test_t1_default_keywords_are_todays_call(env):
    for ot in ("latent", "np_uint8"):
        kw = dict(env.kw, output_type=ot, image=env.small, mask_image=env.small_mask)
        a = env.pipe(**kw)
        b = env.pipe(padding_mask_crop=None, mask_blur=0.0, overlay=None, **kw)
        assert torch.equal(a.latents, b.latents) and torch.isfinite(a.latents.float()).all()
        assert np.array_equal(a.images, b.images) if ot == "np_uint8" else torch.equal(a.images, b.images)
        assert b.crop_box is None


def test_t2_overlay_without_a_crop_keeps_the_pictures_bytes(env):
    kw = dict(env.kw, image=env.small, mask_image=env.small_mask)
    plain = env.pipe(**kw)
    out = env.pipe(overlay=True, **kw)
    assert torch.equal(out.latents, plain.latents) and out.crop_box is None
    assert out.images.shape == (B, H, W, 3) and out.images.dtype == np.uint8
    keep = (env.small_mask == 0).numpy()
    pic = env.small.expand(B, H, W, 3).numpy()
    assert np.array_equal(out.images[:, keep], pic[:, keep])                          # the input's own bytes, not a VAE round trip
    assert not np.array_equal(plain.images[:, keep], pic[:, keep])
    assert np.array_equal(out.images[:, ~keep], plain.images[:, ~keep])               # alpha 255 at equal size: the plain result


def _crop_reference(env, mask, box):
    """The plain masked call fed the crop built with the public ops."""
    from gpt_image_edit_amd import ops
    x0, y0, x1, y1 = box
    renorm = bool(env.pic[:, y0:y1, x0:x1].min() >= 128)
    cond_hw = ((y1 - y0) // 16 * 16, (x1 - x0) // 16 * 16)
    pic = env.pic.cuda()
    cond = env.pipe._encode_vae_image(ops.pixels_box_to_nhwc(pic, box, *cond_hw, 32, renorm), nhwc=True)
    keep = env.pipe._encode_vae_image(ops.pixels_box_to_nhwc(pic, box, H, W, 32, renorm), nhwc=True)
    return env.pipe(**dict(env.kw, image=cond, init_image=keep, mask_image=mask[y0:y1, x0:x1].contiguous(), output_type="pt_raw"))


def test_t3_crop(env):
    from gpt_image_edit_amd import helpers, ops
    out = env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=PAD, **env.kw)
    box = helpers.mask_crop_box(R.bbox_numpy(env.mask[None].numpy(), 1), PW, PH, PAD, W, H)
    assert out.crop_box == box == (81, 32, 150, 78)
    ref = _crop_reference(env, env.mask, box)
    assert torch.isfinite(out.latents.float()).all() and torch.equal(out.latents, ref.latents)
    lat = env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=PAD, **dict(env.kw, output_type="latent"))
    assert torch.equal(lat.images, ref.latents) and lat.crop_box == box               # "latent": the crop's latents, nothing overlaid
    # the picture's size; outside the box and under alpha 0 its own bytes; inside, the overlay of the crop's decode
    x0, y0, x1, y1 = box
    assert out.images.shape == (B, PH, PW, 3) and out.images.dtype == np.uint8
    outside = np.ones((PH, PW), dtype=bool)
    outside[y0:y1, x0:x1] = False
    pic = env.pic.expand(B, PH, PW, 3).numpy()
    assert np.array_equal(out.images[:, outside], pic[:, outside])
    assert np.array_equal(out.images[:, (env.mask == 0).numpy()], pic[:, (env.mask == 0).numpy()])
    want = ops.image_overlay(ref.images.contiguous(), env.pic.cuda(), env.mask[None].cuda(), box).cpu().numpy()
    assert np.array_equal(out.images, want) and not np.array_equal(out.images, pic)
    R.check_overlay(torch.from_numpy(out.images), ref.images.cpu(), env.pic, env.mask[None], box)


def test_t4_mask_blur(env, monkeypatch):
    from gpt_image_edit_amd import ops
    sigma = 3.0
    seen = []
    real = env.pipe._prepare_mask
    monkeypatch.setattr(env.pipe, "_prepare_mask", lambda *a, **kw: seen.append(real(*a, **kw)) or seen[-1])
    kw = dict(env.kw, image=env.small, mask_image=env.small_mask, mask_blur=sigma)
    out = env.pipe(overlay=True, **kw)
    feathered = ops.mask_blur(env.small_mask[None].cuda(), sigma)
    assert 0 < int(((feathered > 0) & (feathered < 255)).sum())                       # there is a feather
    assert torch.equal(seen[0], ops.pack_inpaint_mask(feathered[:, None].float() / 255.0, HL, WL))
    # the feathered mask is the mask everywhere: the plain call fed its bytes gives the same latents
    plain = env.pipe(**dict(env.kw, image=env.small, mask_image=feathered.cpu()))
    assert torch.equal(out.latents, plain.latents)
    raw = env.pipe(overlay=False, **dict(kw, output_type="pt_raw"))
    assert torch.equal(raw.latents, out.latents)
    want = ops.image_overlay(raw.images.contiguous(), env.small.cuda(), feathered, (0, 0, W, H)).cpu().numpy()
    assert np.array_equal(out.images, want)
    R.check_overlay(torch.from_numpy(out.images), raw.images.cpu(), env.small, feathered.cpu(), (0, 0, W, H))


def test_t5_graph_route(env):
    def run(pipe, mask):
        return pipe(image=env.pic, mask_image=mask, padding_mask_crop=PAD, mask_blur=1.0, **env.kw)
    eager, graph = run(env.pipe, env.mask), run(env.graphed, env.mask)
    torch.cuda.synchronize()
    assert eager.crop_box == graph.crop_box and torch.equal(eager.latents, graph.latents)
    assert np.array_equal(eager.images, graph.images)
    key, graph_obj = env.graphed._loop_graph[0], env.graphed._loop_graph[2]
    eager2, graph2 = run(env.pipe, env.mask2), run(env.graphed, env.mask2)            # another mask, the same shapes: a replay
    assert env.graphed._loop_graph[0] == key and env.graphed._loop_graph[2] is graph_obj
    assert eager2.crop_box == graph2.crop_box != eager.crop_box
    assert torch.equal(eager2.latents, graph2.latents) and np.array_equal(eager2.images, graph2.images)
    assert not torch.equal(graph2.latents, graph.latents)


def test_t6_refusals(env):
    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            env.pipe(**{**env.kw, "image": env.pic, "mask_image": env.mask, **kw})
    bad("mask_blur", mask_blur=64.5)
    bad("mask_blur", mask_blur=-1.0)
    bad("padding_mask_crop", padding_mask_crop=-1)
    bad("need `mask_image`", mask_image=None, padding_mask_crop=PAD)
    bad("need `mask_image`", mask_image=None, overlay=True)
    bad("is empty", mask_image=torch.zeros(PH, PW, dtype=torch.uint8), padding_mask_crop=PAD)
    flt = torch.rand(1, 3, PH, PW).cuda() * 2 - 1
    bad("no bytes to keep", image=flt, padding_mask_crop=PAD)
    bad("no bytes to keep", image=flt, overlay=True)
    bad("no bytes to keep", init_image=torch.zeros(1, 16, HL, WL, dtype=BF).cuda(), overlay=True)
    bad("at one size", mask_image=env.small_mask, padding_mask_crop=PAD)
    bad("at one size", mask_image=env.small_mask, overlay=True)
    bad("output_type", overlay=True, output_type="pt")
    bad("output_type", overlay=True, output_type="latent")
    bad("output_type", padding_mask_crop=PAD, output_type="np")
