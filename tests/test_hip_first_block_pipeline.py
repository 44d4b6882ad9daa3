"""GPU: the first-block step cache (``StepCache(measure="first_block")``) through ``FluxKontextPipeline`` on the tiny model of
``test_hip_step_cache_pipeline.py`` (1 double + 2 single blocks, 64 x 64 target, 4 steps, B = 2).  A cached edit is exactly
defined -- block 0 at every step, blocks 1 .. end on the computed ones, their cached residual on the others -- so every
comparison is bit equality on ``output_type="latent"``."""
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
FB = "first_block"


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
    e = SimpleNamespace(tr=tr, vae=vae, cfg=cfg, pipe=FluxKontextPipeline(tr, vae, use_graph=False),
                        graphed=FluxKontextPipeline(tr, vae, use_graph=True))
    e.cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    e.emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    e.pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    e.neg_emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    e.neg_pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    e.noise = e.pipe._pack_latents(torch.randn(B, 16, HL, WL, generator=g).to(BF), B, 16, HL, WL).contiguous().cuda()
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
    return StepCache(measure=FB, **kw)


def _run(pipe, env, sc, **kw):
    return pipe(**dict(env.kw, **kw), step_cache=sc).latents.clone()


# ---- identities: block 0 followed by blocks 1 .. end is the plain block loop ---------------------------------------------------
@pytest.mark.parametrize("route", ["eager", "graph"])
def test_full_schedule_and_threshold_zero_are_the_plain_call(env, route):
    pipe = env.pipe if route == "eager" else env.graphed
    sc = _cache(schedule=range(N))
    assert torch.equal(_run(pipe, env, sc), env.plain)
    assert sc.block_passes == N and sc.computed_steps == list(range(N))
    sc = _cache(threshold=0.0)                   # adaptive: the eager loop on either pipeline
    assert torch.equal(_run(pipe, env, sc), env.plain)
    assert sc.block_passes == N and sc.computed_steps == list(range(N)) and len(sc.rel_l1) == N - 1
    assert all(math.isfinite(x) and x > 0 for x in sc.rel_l1)


# ---- schedule=[0]: block 0 at every step, the tail of step 0 on every later one ------------------------------------------------
def test_schedule_zero_matches_a_loop_of_public_ops(env):
    """h1 (the stream behind block 0) comes from a SECOND model that holds only block 0, loaded from the same weights: the check
    does not run the block-range code it checks."""
    from gpt_image_edit_amd import helpers, ops
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    pipe, tr = env.pipe, env.tr
    sc = _cache(schedule=[0])
    out = _run(pipe, env, sc)
    assert sc.block_passes == 1 and sc.computed_steps == [0]
    assert not torch.equal(out, env.plain)

    tr0 = HipFluxTransformer2DModel(dict(env.cfg, num_layers=1, num_single_layers=0), device="cuda", init="empty")
    full = tr.state_dict()
    tr0.load_state_dict({k: full[k] for k in tr0.state_dict()}, strict=True)

    D, P = tr.inner_dim, tr.p
    cond_tok = pipe._pack_latents(pipe._encode_vae_image(env.cond), B, 16, HL, WL)
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

    def stream_after(model, i):
        v = model(hidden_states=tokens, timestep=t_model[i], guidance=guidance, pooled_projections=env.pooled,
                  encoder_hidden_states=env.emb, txt_ids=txt_ids, img_ids=img_ids, joint_attention_kwargs={}, return_dict=False)[0]
        return v, model._workspace(B, S_txt, S_img).s[:, S_txt:]

    # step 0: one full forward; what blocks 1 .. end added is the stream they left minus the stream block 0 left
    _, h1 = stream_after(tr0, 0)
    v, h_out = stream_after(tr, 0)
    tail = (h_out.float() - h1.float()).to(BF)
    ops.euler_step(tokens, v, S_TGT, s.dsigma(0))
    off = tr.packed().mod_out
    for i in range(1, N):
        mod = tr._cond.mod[i]
        _, h1 = stream_after(tr0, i)
        h = ops.residual_apply(h1, tail, out=torch.empty_like(tail))
        n = ops.ln_modulate(h, mod[:, off + D: off + 2 * D], mod[:, off: off + D])
        v = ops.gemm(n, P("proj_out.weight"), P("proj_out.bias"))
        ops.euler_step(tokens, v, S_TGT, s.dsigma(i))
    assert torch.equal(out, tokens[:, :S_TGT])
    # and through the graph
    scg = _cache(schedule=[0])
    assert torch.equal(_run(env.graphed, env, scg), out) and scg.block_passes == 1
    # the other measure's schedule=[0] skips block 0 too: other bits
    from gpt_image_edit_amd.step_cache import StepCache
    assert not torch.equal(_run(pipe, env, StepCache(schedule=[0])), out)


# ---- adaptive mode ----------------------------------------------------------------------------------------------------------
def test_adaptive_run_then_replay(env, capsys):
    probe = _cache(threshold=0.0)
    _run(env.pipe, env, probe)
    thr = math.nextafter(probe.rel_l1[0], math.inf)      # just above step 1's measure: step 1 is skipped by construction
    sc = _cache(threshold=thr)
    out = _run(env.pipe, env, sc)
    assert sc.rel_l1[0] == probe.rel_l1[0] and 1 not in sc.computed_steps
    # the decisions, recomputed from the recorded measures with the pure rule
    want = [0] + [i for i in range(1, N) if sc.decide(0.0, sc.rel_l1[i - 1], i, N)[0]]
    assert sc.computed_steps == want and sc.block_passes == len(want) < N and want[-1] == N - 1
    assert len(sc.rel_l1) == N - 1
    assert not torch.equal(out, env.plain)
    # a use_graph pipeline runs the adaptive mode eagerly and says so once
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    fresh = FluxKontextPipeline(env.tr, env.vae, use_graph=True)
    capsys.readouterr()
    scg = _cache(threshold=thr)
    assert torch.equal(_run(fresh, env, scg), out) and scg.computed_steps == sc.computed_steps and scg.rel_l1 == sc.rel_l1
    _run(fresh, env, _cache(threshold=thr))
    assert capsys.readouterr().out.count("eager loop") == 1
    # replay of the decisions: a skipped step still runs block 0, so the schedule gives the adaptive run's bits
    rp = _cache(schedule=sc.computed_steps)
    assert torch.equal(_run(env.pipe, env, rp), out) and rp.block_passes == sc.block_passes and rp.rel_l1 == []
    g1 = _run(env.graphed, env, _cache(schedule=sc.computed_steps))
    graph_obj = env.graphed._loop_graph[2]
    g2 = _run(env.graphed, env, _cache(schedule=sc.computed_steps))
    assert torch.equal(g1, out) and torch.equal(g2, out) and env.graphed._loop_graph[2] is graph_obj
    # the measure mode is part of the graph's key
    from gpt_image_edit_amd.step_cache import StepCache
    gi = _run(env.graphed, env, StepCache(schedule=sc.computed_steps))
    assert env.graphed._loop_graph[2] is not graph_obj and not torch.equal(gi, out)


def test_threshold_inf_computes_the_first_and_last_step(env):
    sc = _cache(threshold=math.inf)
    out = _run(env.pipe, env, sc)
    assert sc.computed_steps == [0, N - 1] and sc.block_passes == 2
    assert torch.equal(out, _run(env.pipe, env, _cache(schedule=[0, N - 1])))


def test_the_two_measures_do_not_leak_into_one_another(env):
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    from gpt_image_edit_amd.step_cache import StepCache
    pipe = FluxKontextPipeline(env.tr, env.vae, use_graph=False)
    makers = [lambda: StepCache(schedule=[0, 2]), lambda: _cache(schedule=[0, 2]),
              lambda: StepCache(threshold=math.inf), lambda: _cache(threshold=math.inf)]
    first = [_run(pipe, env, m()) for m in makers]
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[2], first[3])
    for k in (3, 0, 1, 2, 1, 0, 3, 2):
        assert torch.equal(_run(pipe, env, makers[k]()), first[k]), k
    assert torch.equal(pipe(**env.kw).latents, env.plain)


# ---- composition ------------------------------------------------------------------------------------------------------------
def _eager_graph_and_full(env, sched, n_exec, **kw):
    """schedule `sched`: eager == graph and != the plain call; the full schedule == the plain call."""
    out = _run(env.pipe, env, _cache(schedule=sched), **kw)
    assert torch.isfinite(out.float()).all()
    assert torch.equal(_run(env.graphed, env, _cache(schedule=sched), **kw), out)
    plain = env.pipe(**dict(env.kw, **kw)).latents.clone()
    full = _cache(schedule=range(n_exec))
    assert torch.equal(_run(env.pipe, env, full, **kw), plain) and full.block_passes == n_exec
    assert not torch.equal(out, plain)
    return out


def test_with_true_cfg(env):
    one = dict(image=env.cond[:1], prompt_embeds=env.emb[:1], pooled_prompt_embeds=env.pooled[:1], latents=env.noise[:1],
               negative_prompt_embeds=env.neg_emb[:1], negative_pooled_prompt_embeds=env.neg_pooled[:1], true_cfg_scale=2.5)
    _eager_graph_and_full(env, [0, 2], N, **one)
    sc = _cache(threshold=math.inf)              # one decision for the 2B model batch
    assert torch.equal(_run(env.pipe, env, sc, **one), _run(env.pipe, env, _cache(schedule=[0, N - 1]), **one))
    assert sc.computed_steps == [0, N - 1] and len(sc.rel_l1) == N - 1


def test_with_mask_and_strength(env):
    out = _eager_graph_and_full(env, [0, 2], 4, mask_image=env.half, strength=0.5, num_inference_steps=8)
    assert env.pipe.num_timesteps == 4
    from gpt_image_edit_amd import ops
    x0 = env.pipe._pack_latents(env.pipe._encode_vae_image(env.cond), B, 16, HL, WL).contiguous()
    m = ops.pack_inpaint_mask(env.half, HL, WL).cuda()
    sel = (m.repeat(1, 1, 16) == 0).expand(B, -1, -1)
    assert torch.equal(out[sel], x0[sel]) and not torch.equal(out[~sel], x0[~sel])   # the kept region: the encoded picture


def test_with_a_callback_that_rewrites_latents(env):
    seen = []

    def cb(p, i, t, kw):
        seen.append(i)
        return {"latents": (kw["latents"].float() * 0.75).to(BF)}

    plain = env.pipe(**env.kw, callback_on_step_end=cb).latents.clone()
    assert not torch.equal(plain, env.plain)
    assert torch.equal(_run(env.pipe, env, _cache(schedule=range(N)), callback_on_step_end=cb), plain)
    sc = _cache(schedule=[0, 2])
    out = _run(env.pipe, env, sc, callback_on_step_end=cb)
    assert sc.block_passes == 2 and not torch.equal(out, plain) and seen == list(range(N)) * 3
    assert torch.equal(out, _run(env.graphed, env, _cache(schedule=[0, 2]), callback_on_step_end=cb))   # a callback: the eager loop


def test_with_an_attention_mask(env):
    S_img = 2 * S_TGT
    mask = torch.ones(B, S_img, dtype=torch.bool, device="cuda")
    mask[1, S_TGT - 3:S_TGT] = False
    jak = dict(joint_attention_kwargs={"attention_mask": mask})
    plain = env.pipe(**env.kw, **jak).latents.clone()
    assert not torch.equal(plain, env.plain)
    assert torch.equal(_run(env.pipe, env, _cache(schedule=range(N)), **jak), plain)
    sc = _cache(threshold=math.inf)
    out = _run(env.pipe, env, sc, **jak)
    assert sc.computed_steps == [0, N - 1] and not torch.equal(out, plain)
    assert torch.equal(out, _run(env.pipe, env, _cache(schedule=[0, N - 1]), **jak))
    assert not torch.equal(out, _run(env.pipe, env, _cache(schedule=[0, N - 1])))


def _over_routes(env, pipe, fused_settings):
    """schedule [0, 2] and the full schedule on every route: FK_BLOCK_API 0 (per launch), 1 (per block), 2 (per forward)."""
    from gpt_image_edit_amd import transformer
    saved = transformer.BLOCK_API, transformer.MX_FUSED_QUANT
    res = {}
    try:
        for fused in fused_settings:
            for api in (0, 1, 2):
                transformer.BLOCK_API, transformer.MX_FUSED_QUANT = api, fused
                plain = pipe(**env.kw).latents.clone()
                full = _run(pipe, env, _cache(schedule=range(N)))
                assert torch.equal(full, plain), f"fused={fused} FK_BLOCK_API={api}: the full schedule is not the plain call"
                res[fused, api] = (_run(pipe, env, _cache(schedule=[0, 2])), _run(pipe, env, _cache(threshold=math.inf)), plain)
    finally:
        transformer.BLOCK_API, transformer.MX_FUSED_QUANT = saved
    for fused in fused_settings:
        base = res[fused, 0]
        assert not torch.equal(base[0], base[2]) and not torch.equal(base[1], base[2])
        for api in (1, 2):
            for got, want in zip(res[fused, api], base):
                assert torch.equal(got, want), f"fused={fused}: FK_BLOCK_API={api} differs from the per-launch route"
    return res


def test_c_entry_routes_give_the_per_launch_bits(env):
    res = _over_routes(env, env.pipe, [False])
    assert torch.equal(res[False, 0][2], env.plain)


def test_with_mxfp8_plain_and_fused_schedule(env):
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    env.tr.set_weight_format("mxfp8")
    try:
        pipe = FluxKontextPipeline(env.tr, env.vae, use_graph=False)
        res = _over_routes(env, pipe, [False, True])
        assert not torch.equal(res[False, 0][2], env.plain)
        graphed = FluxKontextPipeline(env.tr, env.vae, use_graph=True)
        assert torch.equal(_run(graphed, env, _cache(schedule=[0, 2])), _run(pipe, env, _cache(schedule=[0, 2])))
    finally:
        env.tr.set_weight_format("bf16")
    assert torch.equal(env.pipe(**env.kw).latents, env.plain)


@pytest.mark.parametrize("nd,ns", [(2, 2), (0, 3)])
def test_a_range_that_starts_inside_a_struct_array(env, nd, ns):
    """Block 1 is double block 1, or single block 1 of a model without double blocks: the C entry points get a pointer INTO their
    struct arrays (the tiny model's range (1, 3) starts at single block 0).  A computed step is the plain forward's bits on every
    route, and the skipped step's bits do not depend on the route."""
    from gpt_image_edit_amd import transformer
    tr = transformer.HipFluxTransformer2DModel(dict(env.cfg, num_layers=nd, num_single_layers=ns), device="cuda", init="synthetic",
                                               seed=5)
    tokens = torch.cat([env.noise, torch.roll(env.noise, 1, dims=1)], dim=1).contiguous()
    ids = torch.zeros(tokens.shape[1], 3, device="cuda", dtype=BF)
    ids[:, 1] = torch.arange(tokens.shape[1], device="cuda") % 8
    fwd = dict(hidden_states=tokens, encoder_hidden_states=env.emb, pooled_projections=env.pooled,
               timestep=torch.full([B], 0.5, device="cuda", dtype=BF), img_ids=ids,
               txt_ids=torch.zeros(env.emb.shape[1], 3, device="cuda", dtype=BF),
               guidance=torch.full([B], GUIDANCE, device="cuda", dtype=torch.float32))
    saved = transformer.BLOCK_API
    try:
        for fmt in ("bf16", "mxfp8"):
            tr.set_weight_format(fmt)
            skipped = None
            for api in (0, 1, 2):
                transformer.BLOCK_API = api
                plain = tr(**fwd, return_dict=False)[0].clone()
                assert torch.isfinite(plain.float()).all()
                st = tr.step_cache_state(measure=True, mode=FB)
                tr.step_cache_begin(st, **fwd)
                assert torch.equal(tr.step_cache_end(st, True), plain), (fmt, api)
                tr.step_cache_begin(st, **fwd)
                v = tr.step_cache_end(st, False)           # the same input: h1 + (h_final - h1) is h_final up to one bf16 rounding
                assert st.sums.tolist()[0] == 0.0 and st.sums.tolist()[1] > 0 and st.block_passes == 1
                assert torch.isfinite(v.float()).all()
                skipped = v if skipped is None else skipped
                assert torch.equal(v, skipped), (fmt, api)
    finally:
        transformer.BLOCK_API = saved


def test_with_a_lora_adapter(env):
    """A merged adapter is an ordinary weight: block 0 and the blocks behind it see it alike, through the eager loop and the graph."""
    mods = ("transformer_blocks.0.attn.to_q", "transformer_blocks.0.ff.net.0.proj", "single_transformer_blocks.0.proj_mlp",
            "single_transformer_blocks.1.proj_out", "x_embedder")
    g = torch.Generator().manual_seed(11)
    sd = {}
    for m in mods:
        n, k = env.tr.p(m + ".weight").shape
        sd[f"transformer.{m}.lora_A.weight"] = (0.05 * torch.randn(4, k, generator=g)).to(BF)
        sd[f"transformer.{m}.lora_B.weight"] = (0.05 * torch.randn(n, 4, generator=g)).to(BF)
    before = _run(env.pipe, env, _cache(schedule=[0, 2]))
    env.pipe.load_lora_weights(sd, adapter_name="fb")
    try:
        plain = env.pipe(**env.kw).latents.clone()
        assert not torch.equal(plain, env.plain)
        assert torch.equal(_run(env.pipe, env, _cache(schedule=range(N))), plain)
        out = _run(env.pipe, env, _cache(schedule=[0, 2]))
        assert not torch.equal(out, before) and not torch.equal(out, plain)
        assert torch.equal(_run(env.graphed, env, _cache(schedule=[0, 2])), out)
        sc = _cache(threshold=math.inf)
        assert torch.equal(_run(env.pipe, env, sc), _run(env.pipe, env, _cache(schedule=[0, N - 1]))) and sc.block_passes == 2
    finally:
        env.pipe.unload_lora_weights()
    assert torch.equal(_run(env.pipe, env, _cache(schedule=[0, 2])), before)
    assert torch.equal(_run(env.graphed, env, _cache(schedule=[0, 2])), before)
    assert torch.equal(env.pipe(**env.kw).latents, env.plain)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_a_model_of_one_block_is_refused(env):
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    tr0 = HipFluxTransformer2DModel(dict(env.cfg, num_layers=1, num_single_layers=0), device="cuda", init="synthetic", seed=3)
    with pytest.raises(ValueError, match="nothing to skip"):
        tr0.step_cache_state(measure=False, mode=FB)
    with pytest.raises(ValueError, match="nothing to skip"):
        _run(FluxKontextPipeline(tr0, env.vae, use_graph=False), env, _cache(schedule=[0]))
    tr0.step_cache_state(measure=False)          # the other measure has no such limit
    with pytest.raises(ValueError, match="mode"):
        env.tr.step_cache_state(measure=False, mode="second_block")
