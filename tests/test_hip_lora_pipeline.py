"""GPU: LoRA adapters through ``FluxKontextPipeline`` on the tiny model of ``test_hip_step_cache_pipeline.py`` (1 double + 2
single blocks, 64 x 64 target, 4 steps).  A merged adapter is an ordinary weight, so every comparison is bit equality on
``output_type="latent"`` -- against the same edit on a second model whose parameters are the tensors ``ops.lora_merge`` gives
standalone (the kernel's own correctness is tests/test_hip_lora_kernel.py's business)."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, W, N = 2, 64, 64, 4
HL, WL = H // 8, W // 8
GUIDANCE = 4.0
D0, S0, S1 = "transformer_blocks.0.", "single_transformer_blocks.0.", "single_transformer_blocks.1."
# adapter A: r = 8, alpha = 4; adapter B: r = 33, no alpha.  Together: to_q / to_k / add_q_proj (fused copies), ff.net.0.proj,
# the single blocks' proj_mlp / proj_out, norm1.linear (the fused modulation), x_embedder; to_q and proj_mlp carry both
MODS_A = (D0 + "attn.to_q", D0 + "attn.to_k", D0 + "attn.add_q_proj", D0 + "ff.net.0.proj", S0 + "proj_mlp", "x_embedder")
MODS_B = (D0 + "attn.to_q", D0 + "norm1.linear", S0 + "proj_mlp", S1 + "proj_out")


def _adapter(tr, mods, rank, alpha, seed):
    g = torch.Generator().manual_seed(seed)
    st = {}
    for m in mods:
        n, k = tr.p(m + ".weight").shape
        st[f"transformer.{m}.lora_A.weight"] = (0.05 * torch.randn(rank, k, generator=g)).to(BF)
        st[f"transformer.{m}.lora_B.weight"] = (0.05 * torch.randn(n, rank, generator=g)).to(BF)
        if alpha is not None:
            st[f"transformer.{m}.alpha"] = torch.tensor(float(alpha))
    return st


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import safetensors.torch as st
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    from gpt_image_edit_amd.vae import HipAutoencoderKL
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2)
    tr = HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=21)
    tr2 = HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=21)       # takes the standalone-merged tensors
    vae = HipAutoencoderKL(device="cuda", init="synthetic", seed=22)
    g = torch.Generator().manual_seed(7)
    e = SimpleNamespace(tr=tr, tr2=tr2, vae=vae, pipe=FluxKontextPipeline(tr, vae, use_graph=False),
                        graphed=FluxKontextPipeline(tr, vae, use_graph=True), pipe2=FluxKontextPipeline(tr2, vae, use_graph=False))
    d = tmp_path_factory.mktemp("lora")
    e.state = {"A": _adapter(tr, MODS_A, 8, 4, seed=1), "B": _adapter(tr, MODS_B, 33, None, seed=2)}
    e.meta = {"A": (MODS_A, 8, 4.0), "B": (MODS_B, 33, 33.0)}
    e.path = {}
    for name, sd in e.state.items():
        e.path[name] = str(d / f"{name}.safetensors")
        st.save_file(sd, e.path[name])
    e.orig = {m + ".weight": tr.p(m + ".weight").data.clone() for m in set(MODS_A) | set(MODS_B)}
    assert all(torch.equal(p.data, tr2.p(n).data) for n, p in tr.named_parameters())
    cond = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    emb = torch.randn(B, 40, 4096, generator=g).to(BF).cuda()
    pooled = torch.randn(B, 768, generator=g).to(BF).cuda()
    noise = e.pipe._pack_latents(torch.randn(B, 16, HL, WL, generator=g).to(BF), B, 16, HL, WL).contiguous().cuda()
    e.half = torch.zeros(1, 1, HL, WL)
    e.half[..., :5] = 1
    e.kw = dict(image=cond, prompt_embeds=emb, pooled_prompt_embeds=pooled, height=H, width=W, guidance_scale=GUIDANCE,
                latents=noise, output_type="latent", max_area=H * W, _auto_resize=False, num_inference_steps=N)
    e.plain = e.pipe(**e.kw).latents.clone()
    assert torch.isfinite(e.plain.float()).all()
    return e


def _merged_reference(env, active, call_scale=1.0):
    """tr2 <- the originals, then every touched weight <- ops.lora_merge(original, terms) standalone; ``active``: [(adapter,
    weight)] in merge order, the scale of a term weight x call scale x alpha / r rounded to fp32."""
    from gpt_image_edit_amd import ops
    for n, w in env.orig.items():
        env.tr2.p(n).data.copy_(w)
    terms = {}
    for name, weight in active:
        mods, r, alpha = env.meta[name]
        for m in mods:
            s = float(torch.tensor(weight * call_scale * alpha / r, dtype=torch.float32))
            terms.setdefault(m + ".weight", []).append((env.state[name][f"transformer.{m}.lora_B.weight"].cuda(),
                                                        env.state[name][f"transformer.{m}.lora_A.weight"].cuda(), s))
    for n, ts in terms.items():
        env.tr2.p(n).data.copy_(ops.lora_merge(env.orig[n], ts, out=torch.empty_like(env.orig[n])))
    return env.pipe2


def _edit(pipe, env, **kw):
    return pipe(**dict(env.kw, **kw)).latents.clone()


@pytest.fixture()
def clean(env):
    yield env
    env.pipe.unload_lora_weights()
    env.tr.set_weight_format("bf16")
    env.tr2.set_weight_format("bf16")


def test_a_adapters_are_the_standalone_merged_model(clean):
    env = clean
    assert env.pipe.load_lora_weights(env.path["A"], adapter_name="A") == []
    env.pipe.load_lora_weights(env.state["B"], adapter_name="B")          # a dict is taken too
    assert env.pipe.get_active_adapters() == ["A", "B"]
    out = _edit(env.pipe, env)
    assert torch.isfinite(out.float()).all() and not torch.equal(out, env.plain)
    assert torch.equal(out, _edit(_merged_reference(env, [("A", 1.0), ("B", 1.0)]), env))
    for n in env.orig:                                                    # the parameters themselves are the merged tensors
        assert torch.equal(env.tr.p(n).data, env.tr2.p(n).data) and not torch.equal(env.tr.p(n).data, env.orig[n]), n
    assert not any("lora" in k for k in env.tr.state_dict())


def test_b_unload_restores_every_parameter(clean):
    env = clean
    env.pipe.load_lora_weights(env.path["A"], adapter_name="A")
    env.pipe.load_lora_weights(env.path["B"], adapter_name="B")
    _edit(env.pipe, env, joint_attention_kwargs={"scale": 0.7})
    env.pipe.unload_lora_weights()
    _merged_reference(env, [])                                            # tr2 = the originals
    assert all(torch.equal(p.data, env.tr2.p(n).data) for n, p in env.tr.named_parameters())
    assert env.pipe.get_active_adapters() == [] and not env.tr._lora_base
    assert torch.equal(_edit(env.pipe, env), env.plain)
    assert torch.equal(_edit(env.pipe, env, joint_attention_kwargs={"scale": 0.3}), env.plain)    # no adapters: ignored


def test_c_call_scale_is_the_adapter_weight(clean):
    env = clean
    env.pipe.load_lora_weights(env.path["A"], adapter_name="A")
    env.pipe.load_lora_weights(env.path["B"], adapter_name="B")
    env.pipe.set_adapters(["A", "B"], [1.0, 0.75])
    half = _edit(env.pipe, env, joint_attention_kwargs={"scale": 0.5})
    env.pipe.set_adapters(["A", "B"], [0.5, 0.375])
    assert torch.equal(_edit(env.pipe, env), half) and not torch.equal(half, env.plain)
    assert torch.equal(half, _edit(_merged_reference(env, [("A", 0.5), ("B", 0.375)]), env))
    assert torch.equal(_edit(env.pipe, env, joint_attention_kwargs={"scale": 0.0}), env.plain)
    assert torch.equal(_edit(env.pipe, env), half)                        # and back: from the base, not from the zeroed weights


def test_d_delete_leaves_the_other_adapter_alone(clean):
    env = clean
    env.pipe.load_lora_weights(env.path["A"], adapter_name="A")
    env.pipe.load_lora_weights(env.path["B"], adapter_name="B")
    env.pipe.delete_adapters("A")
    assert env.pipe.get_active_adapters() == ["B"]
    out = _edit(env.pipe, env)
    weights = {n: env.tr.p(n).data.clone() for n in env.orig}
    env.pipe.unload_lora_weights()
    env.pipe.load_lora_weights(env.path["B"], adapter_name="B")
    assert all(torch.equal(env.tr.p(n).data, w) for n, w in weights.items())
    assert torch.equal(_edit(env.pipe, env), out) and not torch.equal(out, env.plain)


def test_e_graph_route(clean, monkeypatch):
    from gpt_image_edit_amd import ops
    env = clean
    merges, real = [], ops.lora_merge
    monkeypatch.setattr(ops, "lora_merge", lambda *a, **k: (merges.append(1), real(*a, **k))[1])
    env.pipe.load_lora_weights(env.path["A"], adapter_name="A")
    env.pipe.load_lora_weights(env.path["B"], adapter_name="B")
    eager = _edit(env.pipe, env)
    assert torch.equal(_edit(env.graphed, env), eager)
    serial, graph_obj = env.tr._pack_serial, env.graphed._loop_graph[2]
    del merges[:]
    assert torch.equal(_edit(env.graphed, env, joint_attention_kwargs={"scale": 1.0}), eager)     # same scale: replay, no merge
    assert merges == [] and env.tr._pack_serial == serial and env.graphed._loop_graph[2] is graph_obj
    scaled = _edit(env.graphed, env, joint_attention_kwargs={"scale": 0.5})
    assert len(merges) == len(env.orig) and env.tr._pack_serial > serial and env.graphed._loop_graph[2] is not graph_obj
    assert torch.equal(scaled, _edit(env.pipe, env, joint_attention_kwargs={"scale": 0.5})) and not torch.equal(scaled, eager)
    assert len(merges) == len(env.orig)


def test_f_mxfp8(clean):
    env = clean
    env.tr.set_weight_format("mxfp8"), env.tr2.set_weight_format("mxfp8")
    plain8 = _edit(env.pipe, env)
    env.pipe.load_lora_weights(env.path["A"], adapter_name="A")
    env.pipe.load_lora_weights(env.path["B"], adapter_name="B")
    out = _edit(env.pipe, env)
    assert not torch.equal(out, plain8)
    assert torch.equal(out, _edit(_merged_reference(env, [("A", 1.0), ("B", 1.0)]), env))
    env.pipe.unload_lora_weights()
    assert torch.equal(_edit(env.pipe, env), plain8)                      # the MXFP8 copies were re-quantized from the base


def test_g_composes_with_mask_and_step_cache(clean):
    from gpt_image_edit_amd.step_cache import StepCache
    env = clean
    env.pipe.load_lora_weights(env.path["A"], adapter_name="A")
    env.pipe.load_lora_weights(env.path["B"], adapter_name="B")
    ref = _merged_reference(env, [("A", 1.0), ("B", 1.0)])
    for kw in (dict(mask_image=env.half), dict(step_cache=lambda: StepCache(schedule=[0, 2])),
               dict(mask_image=env.half, step_cache=lambda: StepCache(schedule=[0, 2]))):
        mk = lambda: {k: (v() if callable(v) else v) for k, v in kw.items()}     # noqa: E731  (a fresh StepCache per call)
        out = _edit(env.pipe, env, **mk())
        assert torch.equal(out, _edit(ref, env, **mk())), sorted(kw)
        assert torch.equal(out, _edit(env.graphed, env, **mk())), sorted(kw)
