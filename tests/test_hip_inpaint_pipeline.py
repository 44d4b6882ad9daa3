"""GPU: masked (inpaint) edits and ``strength`` through ``FluxKontextPipeline`` on the tiny model of ``test_hip_pipeline.py``
(1 double + 2 single blocks, 64 x 96 target).  The step is specified exactly, so the pipeline is held to bit equality:
against the unmasked call (mask of ones), against the encoded picture (mask of zeros), and against an in-test loop that calls
``pipe.transformer`` per step and does the step in torch bf16 ops on the device."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, W = 2, 64, 96
HL, WL = H // 8, W // 8                 # latent 8 x 12 -> 4 x 6 = 24 target tokens
S_TGT = (HL // 2) * (WL // 2)
GUIDANCE = 4.0


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
    pipe = FluxKontextPipeline(tr, vae, use_graph=False)
    g = torch.Generator().manual_seed(7)
    e = SimpleNamespace(pipe=pipe, graphed=FluxKontextPipeline(tr, vae, use_graph=True))
    e.cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()          # condition image at the target size
    e.cond_other = (torch.rand(B, 3, 96, 64, generator=g) * 2 - 1).cuda()  # ... and one of another shape
    e.init = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()          # a picture to preserve that is not the condition
    e.emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    e.pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    e.neg = dict(negative_prompt_embeds=torch.randn(B, 40, 4096, generator=g).to(BF).cuda(),
                 negative_pooled_prompt_embeds=torch.randn(B, 768, generator=g).to(BF).cuda(), true_cfg_scale=2.5)
    e.noise = pipe._pack_latents(torch.randn(B, 16, HL, WL, generator=g).to(BF), B, 16, HL, WL).contiguous().cuda()
    # half mask at the latent size: columns < 5 repaint, so the edge sits on odd latent column 5 and the tokens of column
    # pair (4, 5) carry both; sample-wise masks differ in test cases that pass batch 2
    half = torch.zeros(1, 1, HL, WL)
    half[..., :5] = 1
    e.half = half
    other = torch.zeros(1, 1, HL, WL)
    other[:, :, 3:, :] = 1                                                 # edge on odd latent row 3
    e.other = other
    e.kw = dict(prompt_embeds=e.emb, pooled_prompt_embeds=e.pooled, height=H, width=W, guidance_scale=GUIDANCE,
                latents=e.noise, output_type="latent", max_area=H * W, _auto_resize=False)
    return e


def _encode_packed(pipe, img):
    return pipe._pack_latents(pipe._encode_vae_image(img), B, 16, HL, WL).contiguous()


def _manual_loop(pipe, cond_img, x0, noise, mask_full, n, t_start, emb, pooled):
    """The edit's loop with the step in torch bf16 ops on the device: same model calls as the pipeline makes (conditioning of the
    loop's steps prepared in one pass, one forward per step on the [target | condition] tokens), then ``inpaint_ref.step``."""
    from gpt_image_edit_amd import helpers
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler
    cond_lat = pipe._encode_vae_image(cond_img)
    ch, cw = cond_lat.shape[2:]
    cond_tok = pipe._pack_latents(cond_lat, B, 16, ch, cw)
    ids_t = helpers._prepare_latent_image_ids(B, HL // 2, WL // 2, "cuda", BF)
    ids_c = helpers._prepare_latent_image_ids(B, ch // 2, cw // 2, "cuda", BF)
    ids_c[..., 0] = 1
    s = FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=helpers.calculate_shift(S_TGT), device="cpu")
    start = noise if t_start == 0 else R.keep(x0, noise, float(s._sigmas_host[t_start]))
    tokens = torch.cat([start, cond_tok], dim=1).contiguous()
    t_model = (s.timesteps[t_start:].to(BF) / 1000)[:, None].expand(-1, B).contiguous().cuda()
    guidance = torch.full([B], GUIDANCE, device="cuda", dtype=torch.float32)
    pipe.transformer.prepare_conditioning(t_model, guidance, pooled)
    txt_ids, img_ids = torch.zeros(emb.shape[1], 3, device="cuda", dtype=BF), torch.cat([ids_t, ids_c], dim=0)
    seen = []
    for k, i in enumerate(range(t_start, n)):
        v = pipe.transformer(hidden_states=tokens, timestep=t_model[k], guidance=guidance, pooled_projections=pooled,
                             encoder_hidden_states=emb, txt_ids=txt_ids, img_ids=img_ids, joint_attention_kwargs={},
                             return_dict=False)[0]
        new = R.step(tokens[:, :S_TGT], v[:, :S_TGT], s.dsigma(i), s.sigma_next(i), x0, noise, mask_full)
        tokens[:, :S_TGT].copy_(new)
        seen.append(new.clone())
    return tokens[:, :S_TGT].contiguous(), seen


def _full_mask(mask_lat):
    from gpt_image_edit_amd import ops
    return R.expand_mask(ops.pack_inpaint_mask(mask_lat, HL, WL), 64).cuda()


def test_all_ones_mask_is_the_unmasked_edit(env):
    plain = env.pipe(image=env.cond, num_inference_steps=3, **env.kw).latents
    ones = env.pipe(image=env.cond, num_inference_steps=3, mask_image=torch.ones(1, 1, H, W), **env.kw).latents
    assert torch.isfinite(plain.float()).all() and torch.equal(ones, plain)
    # a picture to preserve without a mask, at full strength, changes nothing either
    assert torch.equal(env.pipe(image=env.cond, num_inference_steps=3, init_image=env.init, **env.kw).latents, plain)


@pytest.mark.parametrize("true_cfg", [False, True])
def test_all_zeros_mask_returns_the_encoded_picture(env, true_cfg):
    extra = env.neg if true_cfg else {}
    zeros = torch.zeros(B, 1, HL, WL)
    # the condition image is the picture (its latents are reused) ...
    out = env.pipe(image=env.cond, num_inference_steps=3, mask_image=zeros, **env.kw, **extra).latents
    assert torch.equal(out, _encode_packed(env.pipe, env.cond))
    # ... or `init_image` is, next to a condition image of another shape
    out = env.pipe(image=env.cond_other, init_image=env.init, num_inference_steps=3, mask_image=zeros, **env.kw, **extra).latents
    assert torch.equal(out, _encode_packed(env.pipe, env.init))
    assert not torch.equal(out, _encode_packed(env.pipe, env.cond))


def test_half_mask_matches_the_in_test_loop(env):
    x0 = _encode_packed(env.pipe, env.init)
    seen = []
    out = env.pipe(image=env.cond_other, init_image=env.init, num_inference_steps=4, mask_image=env.half, **env.kw,
                   callback_on_step_end=lambda p, i, t, kw: seen.append(kw["latents"].clone()) or {}).latents
    m = _full_mask(env.half)
    want, want_steps = _manual_loop(env.pipe, env.cond_other, x0, env.noise, m, 4, 0, env.emb, env.pooled)
    assert torch.isfinite(out.float()).all() and torch.equal(out, want)
    assert len(seen) == 4 and all(torch.equal(a, b) for a, b in zip(seen, want_steps)), "the callback sees the blended latents"
    keep_only = (m[0].sum(-1) == 0)                       # tokens with no repainted sub-pixel
    mixed = (m[0].sum(-1) > 0) & (m[0].sum(-1) < 64)
    assert keep_only.any() and mixed.any() and (m[0].sum(-1) == 64).any()
    assert torch.equal(out[:, keep_only], x0[:, keep_only])
    sel = m.expand(B, -1, -1) == 0
    assert torch.equal(out[sel], x0[sel]) and not torch.equal(out[~sel], x0[~sel])
    # one mask per sample
    two = torch.cat([env.half, env.other])
    out2 = env.pipe(image=env.cond_other, init_image=env.init, num_inference_steps=4, mask_image=two, **env.kw).latents
    want2, _ = _manual_loop(env.pipe, env.cond_other, x0, env.noise, _full_mask(two), 4, 0, env.emb, env.pooled)
    assert torch.equal(out2, want2) and torch.equal(out2[0], out[0]) and not torch.equal(out2[1], out[1])


@pytest.mark.parametrize("masked", [False, True])
def test_strength_one_half_runs_the_second_half_of_the_schedule(env, masked):
    seen = []
    extra = dict(mask_image=env.half) if masked else {}
    out = env.pipe(image=env.cond, num_inference_steps=6, strength=0.5, **env.kw, **extra,
                   callback_on_step_end=lambda p, i, t, kw: seen.append((i, float(t))) or {}).latents
    assert [i for i, _ in seen] == [0, 1, 2] and env.pipe.num_timesteps == 3 and env.pipe.scheduler.begin_index == 3
    assert [t for _, t in seen] == [float(t) for t in env.pipe.scheduler.timesteps[3:]]
    x0 = _encode_packed(env.pipe, env.cond)
    m = _full_mask(env.half) if masked else torch.ones(1, S_TGT, 64, device="cuda", dtype=BF)
    want, _ = _manual_loop(env.pipe, env.cond, x0, env.noise, m, 6, 3, env.emb, env.pooled)
    assert torch.equal(out, want)
    full = env.pipe(image=env.cond, num_inference_steps=6, **env.kw, **extra).latents
    assert not torch.equal(out, full)


def test_graph_route_replays_masked_edits(env):
    def run(pipe, mask, **kw):
        args = dict(env.kw, **kw)
        if mask is not None:
            args["mask_image"] = mask
        return pipe(image=env.cond_other, init_image=None if mask is None else env.init, num_inference_steps=3,
                    **args).latents.clone()
    eager_half, graph_half = run(env.pipe, env.half), run(env.graphed, env.half)
    torch.cuda.synchronize()
    assert torch.isfinite(graph_half.float()).all() and torch.equal(eager_half, graph_half)
    key = env.graphed._loop_graph[0]
    graph_obj = env.graphed._loop_graph[2]
    eager_other, graph_other = run(env.pipe, env.other), run(env.graphed, env.other)    # another mask, same shape: a replay
    assert env.graphed._loop_graph[0] == key and env.graphed._loop_graph[2] is graph_obj
    assert torch.equal(eager_other, graph_other) and not torch.equal(graph_other, graph_half)
    # another noise through the same graph
    noise2 = torch.roll(env.noise, 1, dims=1).contiguous()
    assert torch.equal(run(env.pipe, env.half, latents=noise2), run(env.graphed, env.half, latents=noise2))
    assert env.graphed._loop_graph[2] is graph_obj
    # a per-sample mask is another graph
    two = torch.cat([env.half, env.other])
    assert torch.equal(run(env.pipe, two), run(env.graphed, two)) and env.graphed._loop_graph[0] != key
    # without a mask after a masked call: the plain edit
    assert torch.equal(run(env.graphed, None), run(env.pipe, None))
    assert env.graphed._loop_graph[0] != key


def test_validation(env):
    for bad in (0, 0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="strength"):
            env.pipe(image=env.cond, num_inference_steps=3, strength=bad, **env.kw)
    with pytest.raises(ValueError, match="picture to preserve"):
        env.pipe(num_inference_steps=3, mask_image=env.half, **env.kw)
    with pytest.raises(ValueError, match="picture to preserve"):
        env.pipe(num_inference_steps=3, strength=0.5, **env.kw)
    with pytest.raises(ValueError, match="batch"):
        env.pipe(image=env.cond, num_inference_steps=3, mask_image=torch.zeros(3, 1, HL, WL), **env.kw)
    with pytest.raises(ValueError, match="mask_image"):
        env.pipe(image=env.cond, num_inference_steps=3, mask_image=torch.zeros(1, 3, HL, WL), **env.kw)
    # a uint8 mask (what the command line passes after PIL's "L"): 255 = repaint, the same edit as the float mask
    u8 = (torch.nn.functional.interpolate(env.half, size=(H, W), mode="nearest")[0, 0] * 255).to(torch.uint8)
    a = env.pipe(image=env.cond, num_inference_steps=3, mask_image=u8, **env.kw).latents
    b = env.pipe(image=env.cond, num_inference_steps=3, mask_image=env.half, **env.kw).latents
    assert torch.equal(a, b)
