"""GPU: ``resample=`` through ``FluxKontextPipeline`` on the tiny model of ``test_hip_inpaint_overlay_pipeline.py`` (1 double + 2
single blocks, 64 x 96 target, uint8 pictures up to 150 x 203).  The resize is specified byte for byte, so a call with a filter is held
to BIT equality with the plain call fed the bytes tests/resample_ref.py computes on the CPU: no tolerance anywhere."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref as M  # noqa: E402
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, W = 2, 64, 96
HL, WL = H // 8, W // 8
PH, PW = 128, 192
BIG = (150, 203)            # snaps to (144, 192): a mild downscale on both axes
PAD = 8
FILTERS = ("bilinear", "bicubic", "lanczos")


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
    g = torch.Generator().manual_seed(33)
    e = SimpleNamespace(pipe=FluxKontextPipeline(tr, vae, use_graph=False), graphed=FluxKontextPipeline(tr, vae, use_graph=True))
    e.big = torch.randint(0, 256, (1, *BIG, 3), generator=g, dtype=torch.uint8)
    e.big2 = torch.randint(0, 256, (1, 131, 170, 3), generator=g, dtype=torch.uint8)
    e.pic = torch.randint(0, 256, (1, PH, PW, 3), generator=g, dtype=torch.uint8)
    e.small = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)
    e.mask = torch.zeros(PH, PW, dtype=torch.uint8)
    e.mask[40:70, 100:130] = 255
    e.small_mask = torch.zeros(H, W, dtype=torch.uint8)
    e.small_mask[:, :40] = 255
    emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    noise = e.pipe._pack_latents(torch.randn(B, 16, HL, WL, generator=g).to(BF), B, 16, HL, WL).contiguous().cuda()
    e.kw = dict(prompt_embeds=emb, pooled_prompt_embeds=pooled, height=H, width=W, guidance_scale=4.0, latents=noise,
                num_inference_steps=3, max_area=H * W, _auto_resize=False, output_type="latent")
    return e


def _resize(u8, hw, f):
    return torch.from_numpy(R.resize(u8.numpy(), hw[0], hw[1], f))


def test_t1_none_and_nearest_are_todays_call(env):
    for ot in ("latent", "np_uint8"):
        kw = dict(env.kw, output_type=ot, image=env.big)
        a = env.pipe(**kw)
        assert torch.isfinite(a.latents.float()).all()
        for value in (None, "nearest"):
            b = env.pipe(resample=value, **kw)
            assert torch.equal(a.latents, b.latents)
            assert np.array_equal(a.images, b.images) if ot == "np_uint8" else torch.equal(a.images, b.images)


@pytest.mark.parametrize("f", FILTERS)
def test_t2_condition_image(env, f):
    from gpt_image_edit_amd import helpers
    ih, iw = env.pipe.image_processor.get_default_height_width(env.big.permute(0, 3, 1, 2))
    assert (ih, iw) == (144, 192) == helpers.preferred_condition_size(ih, iw, 16, False)      # the snap's fixed point, on the CPU
    assert env.pipe.image_processor.get_default_height_width(torch.zeros(1, 3, ih, iw)) == (ih, iw)
    out = env.pipe(image=env.big, resample=f, **env.kw)
    ref = env.pipe(image=_resize(env.big, (ih, iw), f), **env.kw)
    assert torch.isfinite(out.latents.float()).all() and torch.equal(out.latents, ref.latents)


@pytest.mark.parametrize("f", FILTERS)
def test_t3_init_image_mask_and_strength(env, f):
    kw = dict(env.kw, image=env.small, mask_image=env.small_mask, strength=0.5)
    out = env.pipe(init_image=env.big2, resample=f, **kw)
    ref = env.pipe(init_image=_resize(env.big2, (H, W), f), **kw)
    assert torch.isfinite(out.latents.float()).all() and torch.equal(out.latents, ref.latents)
    assert not torch.equal(out.latents, env.pipe(init_image=env.big2, **kw).latents)          # and the nearest gather is another picture


def _crop_inputs(env, f):
    from gpt_image_edit_amd import helpers
    box = helpers.mask_crop_box(M.bbox_numpy(env.mask[None].numpy(), 1), PW, PH, PAD, W, H)
    assert box == (81, 32, 150, 78)
    x0, y0, x1, y1 = box
    cond_hw = ((y1 - y0) // 16 * 16, (x1 - x0) // 16 * 16)
    crop = env.pic[:, y0:y1, x0:x1]
    return box, dict(image=_resize(crop, cond_hw, f), init_image=_resize(crop, (H, W), f), mask_image=env.mask[y0:y1, x0:x1].contiguous())


@pytest.mark.parametrize("f", FILTERS)
def test_t4_crop(env, f):
    box, plain = _crop_inputs(env, f)
    out = env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=PAD, resample=f, **env.kw)
    ref = env.pipe(**plain, **env.kw)
    assert out.crop_box == box and torch.equal(out.latents, ref.latents) and torch.equal(out.images, ref.latents)


@pytest.mark.parametrize("f", FILTERS)
def test_t5_overlay(env, f):
    from gpt_image_edit_amd import ops
    box, plain = _crop_inputs(env, f)
    x0, y0, x1, y1 = box
    out = env.pipe(image=env.pic, mask_image=env.mask, padding_mask_crop=PAD, resample=f, **dict(env.kw, output_type="np_uint8"))
    raw = env.pipe(**plain, **dict(env.kw, output_type="pt_raw"))
    assert torch.equal(out.latents, raw.latents)
    decoded = ops.image_to_u8(raw.images.contiguous()).cpu().numpy()
    want = R.overlay(R.resize(decoded, y1 - y0, x1 - x0, f), env.pic.numpy(), env.mask[None].numpy(), box)
    assert out.images.shape == (B, PH, PW, 3) and out.images.dtype == np.uint8 and np.array_equal(out.images, want)
    outside = np.ones((PH, PW), dtype=bool)
    outside[y0:y1, x0:x1] = False
    pic = env.pic.expand(B, PH, PW, 3).numpy()
    assert np.array_equal(out.images[:, outside], pic[:, outside]) and not np.array_equal(out.images, pic)
    # at equal size with a binary mask: today's overlay bytes
    kw = dict(env.kw, output_type="np_uint8", image=env.small, mask_image=env.small_mask, overlay=True)
    assert np.array_equal(env.pipe(resample=f, **kw).images, env.pipe(**kw).images)


def test_t6_graph_route(env):
    def run(pipe, pic):
        return pipe(image=pic, mask_image=env.mask, padding_mask_crop=PAD, resample="lanczos", **dict(env.kw, output_type="np_uint8"))
    eager, graph = run(env.pipe, env.pic), run(env.graphed, env.pic)
    torch.cuda.synchronize()
    assert eager.crop_box == graph.crop_box and torch.equal(eager.latents, graph.latents)
    assert np.array_equal(eager.images, graph.images)
    key, graph_obj = env.graphed._loop_graph[0], env.graphed._loop_graph[2]
    other = env.pic.flip(2).contiguous()                                               # another picture, the same shapes: a replay
    eager2, graph2 = run(env.pipe, other), run(env.graphed, other)
    assert env.graphed._loop_graph[0] == key and env.graphed._loop_graph[2] is graph_obj
    assert torch.equal(eager2.latents, graph2.latents) and np.array_equal(eager2.images, graph2.images)
    assert not torch.equal(graph2.latents, graph.latents)
    # the keyword is no part of the key: the nearest call of the same shapes replays the same graph
    env.graphed(image=env.pic, mask_image=env.mask, padding_mask_crop=PAD, **dict(env.kw, output_type="np_uint8"))
    assert env.graphed._loop_graph[0] == key and env.graphed._loop_graph[2] is graph_obj


def test_t7_the_keyword_is_not_ignored(env):
    lanczos = env.pipe(image=env.big, resample="lanczos", **env.kw)
    nearest = env.pipe(image=env.big, resample="nearest", **env.kw)
    assert not torch.equal(lanczos.latents, nearest.latents)


def test_t8_refusals(env):
    flt = torch.rand(1, 3, PH, PW).cuda() * 2 - 1
    with pytest.raises(ValueError, match="`resample` is None"):
        env.pipe(image=env.big, resample="box", **env.kw)
    with pytest.raises(ValueError, match="`image` is a float tensor or latents"):
        env.pipe(image=flt, resample="lanczos", **env.kw)
    with pytest.raises(ValueError, match="`init_image` is a float tensor or latents"):
        env.pipe(image=env.small, init_image=torch.zeros(1, 16, HL, WL, dtype=BF).cuda(), mask_image=env.small_mask, resample="bicubic",
                 **env.kw)
