"""GPU: the float32 latent state through ``FluxKontextPipeline`` on the tiny model of ``test_hip_solver_pipeline.py`` (1 double + 2
single blocks, 64 x 96 target, B = 2), for the Euler and the AB2 scheduler.  The step is specified exactly, so everything here is
bit equality: against that file's in-test loop (the pipeline's model calls, made by hand) with the step done by
``solver_state_ref.step`` -- torch float32 ops on the device, the state carried in float32 from step to step -- eager against
graph, and the default state against a call without the keyword."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as R  # noqa: E402
import solver_state_ref as S  # noqa: E402
import test_hip_solver_pipeline as P  # noqa: E402     (its _loop: the model calls of an edit with the step handed in)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, W, HL, WL, S_TGT, N = P.B, P.H, P.W, P.HL, P.WL, P.S_TGT, P.N
SOLVERS = ("euler", "ab2")


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    from gpt_image_edit_amd.scheduler import FlowMatchMultistepScheduler
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    from gpt_image_edit_amd.vae import HipAutoencoderKL
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2)
    tr = HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=21)
    vae = HipAutoencoderKL(device="cuda", init="synthetic", seed=22)
    g = torch.Generator().manual_seed(7)
    e = SimpleNamespace(tr=tr)
    e.eager = {"euler": FluxKontextPipeline(tr, vae, use_graph=False),
               "ab2": FluxKontextPipeline(tr, vae, FlowMatchMultistepScheduler(), use_graph=False)}
    e.graphed = {"euler": FluxKontextPipeline(tr, vae, use_graph=True),
                 "ab2": FluxKontextPipeline(tr, vae, FlowMatchMultistepScheduler(), use_graph=True)}
    e.pipe = e.eager["ab2"]                  # what P._loop packs and encodes with
    e.cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    e.emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    e.pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    e.neg = dict(negative_prompt_embeds=torch.randn(B, 40, 4096, generator=g).to(BF).cuda(),
                 negative_pooled_prompt_embeds=torch.randn(B, 768, generator=g).to(BF).cuda(), true_cfg_scale=2.5)
    e.noise = e.pipe._pack_latents(torch.randn(B, 16, HL, WL, generator=g).to(BF), B, 16, HL, WL).contiguous().cuda()
    e.noise2 = torch.roll(e.noise, 3, dims=1).contiguous()
    half = torch.zeros(1, 1, HL, WL)
    half[..., :5] = 1                       # the edge sits on odd latent column 5: tokens of column pair (4, 5) carry both
    e.half = half
    e.kw = dict(image=e.cond, prompt_embeds=e.emb, pooled_prompt_embeds=e.pooled, height=H, width=W, guidance_scale=P.GUIDANCE,
                latents=e.noise, output_type="latent", max_area=H * W, _auto_resize=False)
    e.x0 = e.pipe._pack_latents(e.pipe._encode_vae_image(e.cond), B, 16, HL, WL).contiguous()
    # the N-step edits on the float32 state, computed once
    e.fp32 = {s: e.eager[s](num_inference_steps=N, latent_state="fp32", **e.kw).latents.clone() for s in SOLVERS}
    assert all(torch.isfinite(t.float()).all() and t.dtype == BF for t in e.fp32.values())
    return e


def _state_loop(env, solver, n, mask_full=None, noise=None, replace=None, **kw):
    """``P._loop`` with the step on a float32 state held here: seeded from the bf16 tokens at the first step and after
    ``replace(k, x)`` (the callback) returned new latents, else carried unrounded; the tokens get its bf16 rounding."""
    sig = R.schedule(n, S_TGT)
    noise = env.noise if noise is None else noise
    st = SimpleNamespace(state=None, h=None)

    def step(i, first, x, v):
        xs = x.float() if first or st.state is None else st.state
        if solver == "euler":
            c = (float(np.float32(sig[i + 1]) - np.float32(sig[i])), 0.0, 0)
        else:
            c = R.coefficients(sig, i, not first)
        st.state = S.step(xs, v, st.h, *c, float(sig[i + 1]), env.x0, noise, mask_full)
        st.h = v
        return st.state.to(BF)

    def on_step(k, x):
        out = replace(k, x)
        if out is not None:
            st.state = None
        return out
    return P._loop(env, n, noise=noise, step=step, on_step=on_step if replace is not None else None, **kw)


@pytest.mark.parametrize("solver", SOLVERS)
def test_five_steps_match_the_in_test_loop_and_the_switch_is_live(env, solver):
    assert torch.equal(env.fp32[solver], _state_loop(env, solver, N))
    plain = env.eager[solver](num_inference_steps=N, **env.kw).latents.clone()
    named = env.eager[solver](num_inference_steps=N, latent_state="bf16", **env.kw).latents
    assert torch.equal(named, plain)                                      # the default, named: the call without the keyword
    assert not torch.equal(env.fp32[solver], plain)                       # and the float32 state is another computation
    if solver == "ab2":
        assert torch.equal(plain, P._loop(env, N))
    else:
        assert torch.equal(plain, P._loop(env, N, step=P._euler_step(env, N)))


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("solver", SOLVERS)
def test_short_schedules(env, solver, n):
    out = env.eager[solver](num_inference_steps=n, latent_state="fp32", **env.kw).latents
    assert torch.equal(out, _state_loop(env, solver, n))
    if n == 1:      # one step from bf16 noise: the unrounded sum, rounded once -- what the bf16-state AB2 step computes too
        assert torch.equal(out, env.eager["ab2"](num_inference_steps=1, **env.kw).latents)


@pytest.mark.parametrize("solver", SOLVERS)
def test_eager_and_graph(env, solver):
    pipe = env.graphed[solver]
    g1 = pipe(num_inference_steps=N, latent_state="fp32", **env.kw).latents.clone()
    torch.cuda.synchronize()
    assert torch.equal(g1, env.fp32[solver])
    key, G, graph = pipe._loop_graph
    assert "fp32" in key and G.state.dtype == torch.float32 and G.state.data_ptr() != G.tokens.data_ptr()
    kw2 = dict(env.kw, latents=env.noise2)
    g2 = pipe(num_inference_steps=N, latent_state="fp32", **kw2).latents.clone()    # other noise: a replay, the state left by the last call
    assert pipe._loop_graph[0] == key and pipe._loop_graph[2] is graph
    e2 = env.eager[solver](num_inference_steps=N, latent_state="fp32", **kw2).latents
    assert torch.equal(g2, e2) and not torch.equal(g2, g1)
    assert torch.equal(g2, _state_loop(env, solver, N, noise=env.noise2))
    assert torch.equal(pipe(num_inference_steps=N, latent_state="fp32", **env.kw).latents, env.fp32[solver])
    # the other state captures anew and is the eager bf16 call
    b = pipe(num_inference_steps=N, **env.kw).latents.clone()
    assert pipe._loop_graph[0] != key and "bf16" in pipe._loop_graph[0]
    assert torch.equal(b, env.eager[solver](num_inference_steps=N, **env.kw).latents)


@pytest.mark.parametrize("solver", SOLVERS)
def test_inpaint_and_strength(env, solver):
    pipe = env.eager[solver]
    kw = dict(num_inference_steps=N, latent_state="fp32", **env.kw)
    ones = pipe(mask_image=torch.ones(1, 1, H, W), **kw).latents
    assert torch.equal(ones, env.fp32[solver])
    zeros = pipe(mask_image=torch.zeros(B, 1, HL, WL), **kw).latents
    assert torch.equal(zeros, env.x0)                                     # the encoded picture, bit for bit
    out = pipe(mask_image=env.half, strength=0.6, **kw).latents
    assert pipe.scheduler.begin_index == 2 and pipe.num_timesteps == 3
    m = P._full_mask(env.half)
    want = _state_loop(env, solver, N, mask_full=m, t_start=2)
    assert torch.equal(out, want)
    sel = m.expand(B, -1, -1) == 0
    assert torch.equal(out[sel], env.x0[sel]) and not torch.equal(out[~sel], env.x0[~sel])
    # strength alone: the update everywhere, the state seeded from the re-noised picture
    assert torch.equal(pipe(strength=0.6, **kw).latents, _state_loop(env, solver, N, t_start=2))
    # and the masked edit through the graph
    assert torch.equal(env.graphed[solver](mask_image=env.half, strength=0.6, **kw).latents, want)


@pytest.mark.parametrize("solver", SOLVERS)
def test_composes_with_true_cfg(env, solver):
    out = env.eager[solver](num_inference_steps=N, latent_state="fp32", **env.kw, **env.neg).latents
    assert torch.equal(out, _state_loop(env, solver, N, true_cfg=True)) and not torch.equal(out, env.fp32[solver])


@pytest.mark.parametrize("solver", SOLVERS)
def test_composes_with_the_step_cache(env, solver):
    from gpt_image_edit_amd.step_cache import StepCache
    sc = StepCache(schedule=[0, 2, 4])
    out = env.eager[solver](num_inference_steps=N, latent_state="fp32", step_cache=sc, **env.kw).latents.clone()
    assert sc.block_passes == 3 and sc.computed_steps == [0, 2, 4]
    assert torch.equal(out, _state_loop(env, solver, N, schedule=(0, 2, 4))) and not torch.equal(out, env.fp32[solver])
    scg = StepCache(schedule=[0, 2, 4])
    assert torch.equal(env.graphed[solver](num_inference_steps=N, latent_state="fp32", step_cache=scg, **env.kw).latents, out)
    assert scg.block_passes == 3


@pytest.mark.parametrize("solver", SOLVERS)
def test_a_callback_that_replaces_the_latents_reseeds_the_state(env, solver):
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(kw["latents"].clone())
        return {"latents": (kw["latents"].float() * 0.5).to(BF)} if i == 1 else {}
    out = env.eager[solver](num_inference_steps=N, latent_state="fp32", callback_on_step_end=cb, **env.kw).latents
    want_seen = []
    want = _state_loop(env, solver, N,
                       replace=lambda k, x: (want_seen.append(x.clone()), (x.float() * 0.5).to(BF) if k == 1 else None)[1])
    assert torch.equal(out, want) and not torch.equal(out, env.fp32[solver])
    assert len(seen) == N and all(torch.equal(a, b) for a, b in zip(seen, want_seen))
    # a callback that returns nothing leaves the state carried: the run without a callback
    out = env.eager[solver](num_inference_steps=N, latent_state="fp32", callback_on_step_end=lambda *a: {}, **env.kw).latents
    assert torch.equal(out, env.fp32[solver])
