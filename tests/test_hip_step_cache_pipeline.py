"""GPU: the step cache through ``FluxKontextPipeline`` on the tiny model of ``test_hip_inpaint_pipeline.py`` (1 double + 2
single blocks, 64 x 64 target, 4 steps).  A cached edit is exactly defined -- which steps run the blocks, and what the others
add -- so every comparison is bit equality on ``output_type="latent"``."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, W, N = 2, 64, 64, 4
HL, WL = H // 8, W // 8
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
    g = torch.Generator().manual_seed(7)
    e = SimpleNamespace(tr=tr, vae=vae, pipe=FluxKontextPipeline(tr, vae, use_graph=False),
                        graphed=FluxKontextPipeline(tr, vae, use_graph=True))
    e.cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    e.emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    e.pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    e.neg_emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    e.neg_pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    e.noise = e.pipe._pack_latents(torch.randn(B, 16, HL, WL, generator=g).to(BF), B, 16, HL, WL).contiguous().cuda()
    e.noise2 = torch.roll(e.noise, 3, dims=1).contiguous()
    half = torch.zeros(1, 1, HL, WL)
    half[..., :5] = 1
    e.half = half
    e.kw = dict(image=e.cond, prompt_embeds=e.emb, pooled_prompt_embeds=e.pooled, height=H, width=W, guidance_scale=GUIDANCE,
                latents=e.noise, output_type="latent", max_area=H * W, _auto_resize=False, num_inference_steps=N)
    e.plain = e.pipe(**e.kw).latents.clone()
    assert torch.isfinite(e.plain.float()).all()
    return e


def _cache(**kw):
    from gpt_image_edit_amd.step_cache import StepCache
    return StepCache(**kw)


def _run(pipe, env, sc, **kw):
    return pipe(**dict(env.kw, **kw), step_cache=sc).latents.clone()


# ---- identity cases ---------------------------------------------------------------------------------------------------------
def test_none_is_the_plain_call(env):
    assert torch.equal(env.pipe(**env.kw, step_cache=None).latents, env.plain)
    assert torch.equal(env.graphed(**env.kw, step_cache=None).latents, env.plain)


@pytest.mark.parametrize("route", ["eager", "graph"])
def test_full_schedule_is_the_plain_call(env, route):
    sc = _cache(schedule=range(N))
    out = _run(env.pipe if route == "eager" else env.graphed, env, sc)
    assert torch.equal(out, env.plain)
    assert sc.block_passes == N and sc.computed_steps == list(range(N))


def test_threshold_zero_is_the_plain_call(env):
    sc = _cache(threshold=0.0)
    assert torch.equal(_run(env.pipe, env, sc), env.plain)
    assert sc.block_passes == N and sc.computed_steps == list(range(N)) and len(sc.rel_l1) == N - 1


# ---- schedule=[0]: the residual of step 0 on every later step ----------------------------------------------------------------
def test_schedule_zero_matches_a_loop_of_public_ops(env):
    from gpt_image_edit_amd import helpers, ops
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler
    pipe, tr = env.pipe, env.tr
    sc = _cache(schedule=[0])
    out = _run(pipe, env, sc)
    assert sc.block_passes == 1 and sc.computed_steps == [0]
    assert not torch.equal(out, env.plain)

    D, P = tr.inner_dim, tr.p
    cond_lat = pipe._encode_vae_image(env.cond)
    cond_tok = pipe._pack_latents(cond_lat, B, 16, HL, WL)
    ids_t = helpers._prepare_latent_image_ids(B, HL // 2, WL // 2, "cuda", BF)
    ids_c = helpers._prepare_latent_image_ids(B, HL // 2, WL // 2, "cuda", BF)
    ids_c[..., 0] = 1
    s = FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / N, N), mu=helpers.calculate_shift(S_TGT), device="cpu")
    tokens = torch.cat([env.noise, cond_tok], dim=1).contiguous()
    S_img, S_txt = tokens.shape[1], env.emb.shape[1]
    t_model = (s.timesteps.to(BF) / 1000)[:, None].expand(-1, B).contiguous().cuda()
    guidance = torch.full([B], GUIDANCE, device="cuda", dtype=torch.float32)
    tr.prepare_conditioning(t_model, guidance, env.pooled)
    txt_ids, img_ids = torch.zeros(S_txt, 3, device="cuda", dtype=BF), torch.cat([ids_t, ids_c], dim=0)
    # step 0: one full forward; what the blocks added to their input is the stream they left minus x_embedder's output
    h0 = ops.gemm(tokens, P("x_embedder.weight"), P("x_embedder.bias"))
    v = tr(hidden_states=tokens, timestep=t_model[0], guidance=guidance, pooled_projections=env.pooled,
           encoder_hidden_states=env.emb, txt_ids=txt_ids, img_ids=img_ids, joint_attention_kwargs={}, return_dict=False)[0]
    h_out = tr._workspace(B, S_txt, S_img).s[:, S_txt:]
    r = (h_out.float() - h0.float()).to(BF)
    ops.euler_step(tokens, v, S_TGT, s.dsigma(0))
    off = tr.packed().mod_out
    for i in range(1, N):
        mod = tr._cond.mod[i]
        h0 = ops.gemm(tokens, P("x_embedder.weight"), P("x_embedder.bias"))
        h = ops.residual_apply(h0, r, out=torch.empty_like(h0))
        n = ops.ln_modulate(h, mod[:, off + D: off + 2 * D], mod[:, off: off + D])
        v = ops.gemm(n, P("proj_out.weight"), P("proj_out.bias"))
        ops.euler_step(tokens, v, S_TGT, s.dsigma(i))
    assert torch.equal(out, tokens[:, :S_TGT])
    # and through the graph
    scg = _cache(schedule=[0])
    assert torch.equal(_run(env.graphed, env, scg), out) and scg.block_passes == 1


# ---- adaptive mode ----------------------------------------------------------------------------------------------------------
def test_threshold_inf_computes_the_first_and_last_step(env):
    sc = _cache(threshold=math.inf)
    out = _run(env.pipe, env, sc)
    assert sc.computed_steps == [0, N - 1] and sc.block_passes == 2
    assert len(sc.rel_l1) == N - 1 and all(math.isfinite(x) and x > 0 for x in sc.rel_l1)
    assert torch.equal(out, _run(env.pipe, env, _cache(schedule=[0, N - 1])))


def _adaptive(env, pipe=None, n=6, **kw):
    """An adaptive run at a mid threshold: the median of the rel_l1 the same call records when every step computes.
    Six steps give five measures: the two below the median cannot both be the last step's, and the first of them that follows a
    computed step is skipped, so with a trajectory near the probe's some steps skip and some compute."""
    pipe = pipe or env.pipe
    probe = _cache(threshold=0.0)
    _run(pipe, env, probe, num_inference_steps=n, **kw)
    thr = float(np.median(probe.rel_l1))
    sc = _cache(threshold=thr)
    out = _run(pipe, env, sc, num_inference_steps=n, **kw)
    return sc, out


def test_adaptive_run_then_replay(env, capsys):
    n = 6
    sc, out = _adaptive(env, n=n)
    assert 1 < sc.block_passes < n, (sc.rel_l1, sc.computed_steps)
    assert sc.block_passes == len(sc.computed_steps) and sc.computed_steps[0] == 0 and sc.computed_steps[-1] == n - 1
    # with use_graph=True an adaptive call runs the eager loop, and says so once
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    fresh = FluxKontextPipeline(env.tr, env.vae, use_graph=True)
    capsys.readouterr()
    scg = _cache(threshold=sc.threshold)
    assert torch.equal(_run(fresh, env, scg, num_inference_steps=n), out) and scg.computed_steps == sc.computed_steps
    _run(fresh, env, _cache(threshold=sc.threshold), num_inference_steps=n)
    assert capsys.readouterr().out.count("eager loop") == 1
    # replay of the decisions: eager, and through the graph twice
    rp = _cache(schedule=sc.computed_steps)
    assert torch.equal(_run(env.pipe, env, rp, num_inference_steps=n), out) and rp.block_passes == sc.block_passes
    g1 = _run(env.graphed, env, _cache(schedule=sc.computed_steps), num_inference_steps=n)
    graph_obj = env.graphed._loop_graph[2]
    rp2 = _cache(schedule=sc.computed_steps)
    g2 = _run(env.graphed, env, rp2, num_inference_steps=n)
    assert torch.equal(g1, out) and torch.equal(g2, out) and env.graphed._loop_graph[2] is graph_obj
    assert rp2.block_passes == sc.block_passes and rp2.computed_steps == sc.computed_steps
    # other noise through the same graph: the eager schedule run with that noise
    g3 = _run(env.graphed, env, _cache(schedule=sc.computed_steps), num_inference_steps=n, latents=env.noise2)
    want = _run(env.pipe, env, _cache(schedule=sc.computed_steps), num_inference_steps=n, latents=env.noise2)
    assert env.graphed._loop_graph[2] is graph_obj and torch.equal(g3, want) and not torch.equal(g3, out)
    # another schedule is another graph
    _run(env.graphed, env, _cache(schedule=range(n)), num_inference_steps=n)
    assert env.graphed._loop_graph[2] is not graph_obj


# ---- composition: each cached run equals its eager counterpart ----------------------------------------------------------------
def _eager_vs_graph(env, n=6, pipes=None, **kw):
    eager, graphed = pipes or (env.pipe, env.graphed)
    sc, out = _adaptive(env, pipe=eager, n=n, **kw)
    assert 1 < len(sc.computed_steps) < eager.num_timesteps, (sc.rel_l1, sc.computed_steps)
    rp = _run(eager, env, _cache(schedule=sc.computed_steps), num_inference_steps=n, **kw)
    gr = _run(graphed, env, _cache(schedule=sc.computed_steps), num_inference_steps=n, **kw)
    assert torch.isfinite(out.float()).all() and torch.equal(rp, out) and torch.equal(gr, out)
    return sc, out


def test_with_true_cfg(env):
    one = dict(image=env.cond[:1], prompt_embeds=env.emb[:1], pooled_prompt_embeds=env.pooled[:1], latents=env.noise[:1],
               negative_prompt_embeds=env.neg_emb[:1], negative_pooled_prompt_embeds=env.neg_pooled[:1], true_cfg_scale=2.5)
    sc, out = _eager_vs_graph(env, **one)
    # one decision for the whole model batch: a full schedule is the plain true-CFG call
    plain = env.pipe(**dict(env.kw, **one, num_inference_steps=6)).latents
    full = _cache(schedule=range(6))
    assert torch.equal(_run(env.pipe, env, full, num_inference_steps=6, **one), plain) and full.block_passes == 6
    assert not torch.equal(out, plain)


def test_with_mask_image(env):
    sc, out = _eager_vs_graph(env, mask_image=env.half)
    from gpt_image_edit_amd import ops
    x0 = env.pipe._pack_latents(env.pipe._encode_vae_image(env.cond), B, 16, HL, WL).contiguous()
    m = ops.pack_inpaint_mask(env.half, HL, WL).cuda()                       # [1, S_tgt, 4]: element j of a token is sub-pixel j % 4
    sel = (m.repeat(1, 1, 16) == 0).expand(B, -1, -1)
    assert sel.any() and (~sel).any()
    assert torch.equal(out[sel], x0[sel]) and not torch.equal(out[~sel], x0[~sel])   # the kept region: the encoded picture
    full = _cache(schedule=range(6))
    assert torch.equal(_run(env.pipe, env, full, num_inference_steps=6, mask_image=env.half),
                       env.pipe(**dict(env.kw, num_inference_steps=6, mask_image=env.half)).latents)


def test_with_strength(env):
    sc, out = _eager_vs_graph(env, n=12, strength=0.5)           # executes steps 6 .. 11 of the schedule: indices 0 .. 5
    assert env.pipe.num_timesteps == 6 and sc.computed_steps[0] == 0 and sc.computed_steps[-1] == 5
    full = _cache(schedule=range(6))
    assert torch.equal(_run(env.pipe, env, full, num_inference_steps=12, strength=0.5),
                       env.pipe(**dict(env.kw, num_inference_steps=12, strength=0.5)).latents)
    with pytest.raises(ValueError, match="schedule"):            # index 6 is outside the six executed steps
        _run(env.pipe, env, _cache(schedule=[0, 6]), num_inference_steps=12, strength=0.5)


def test_with_callback(env):
    seen = []
    sc = _cache(schedule=[0, 2])
    out = _run(env.pipe, env, sc, callback_on_step_end=lambda p, i, t, kw: seen.append(kw["latents"].clone()) or {})
    assert len(seen) == N and torch.equal(seen[-1], out) and sc.block_passes == 2
    assert torch.equal(out, _run(env.pipe, env, _cache(schedule=[0, 2])))
    # a callback keeps a graph pipeline on the eager loop, cached or not
    assert torch.equal(out, _run(env.graphed, env, _cache(schedule=[0, 2]), callback_on_step_end=lambda p, i, t, kw: {}))


def test_with_mxfp8(env):
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    env.tr.set_weight_format("mxfp8")
    try:
        pipes = (FluxKontextPipeline(env.tr, env.vae, use_graph=False), FluxKontextPipeline(env.tr, env.vae, use_graph=True))
        plain = pipes[0](**dict(env.kw, num_inference_steps=6)).latents.clone()
        full = _cache(schedule=range(6))
        assert torch.equal(_run(pipes[0], env, full, num_inference_steps=6), plain) and full.block_passes == 6
        sc, out = _eager_vs_graph(env, pipes=pipes)
        assert not torch.equal(out, plain)
    finally:
        env.tr.set_weight_format("bf16")
    assert torch.equal(env.pipe(**env.kw).latents, env.plain)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_a_skipped_step_before_a_computed_one_is_refused(env):
    tr = env.tr
    st = tr.step_cache_state(measure=False)
    tokens = torch.cat([env.noise, env.noise], dim=1).contiguous()
    ids = torch.zeros(tokens.shape[1], 3, device="cuda", dtype=BF)
    tr.step_cache_begin(st, hidden_states=tokens, encoder_hidden_states=env.emb, pooled_projections=env.pooled,
                        timestep=torch.full([B], 0.5, device="cuda", dtype=BF), img_ids=ids,
                        txt_ids=torch.zeros(env.emb.shape[1], 3, device="cuda", dtype=BF),
                        guidance=torch.full([B], GUIDANCE, device="cuda", dtype=torch.float32))
    with pytest.raises(RuntimeError, match="no residual"):
        tr.step_cache_end(st, compute=False)
    assert st.block_passes == 0
    with pytest.raises(RuntimeError, match="step_cache_begin"):
        tr.step_cache_end(st, compute=True)
    # the pipeline validates the schedule before any GPU work
    with pytest.raises(ValueError, match="schedule"):
        _run(env.pipe, env, _cache(schedule=[0, N]))
