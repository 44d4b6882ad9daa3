"""MXFP8 weight format of HipFluxTransformer2DModel on the GPU: the three block routes give identical bits, format switching
and in-place weight writes re-pack correctly, the graph-captured loop equals the eager one, and the error against the fp32
oracle (full depth) and against the bf16 path over a 28-step edit stays within the recorded bounds."""
import pytest
import torch

from conftest import report
from test_hip_mmdit import _StreamedState, _inputs

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _kw(B, S_txt, h, w, cfg, seed):
    hs, enc, pooled, t, gd, img_ids, txt_ids = _inputs(B, S_txt, h, w, cfg, seed=seed)
    return dict(hidden_states=hs.cuda(), timestep=t.cuda(), guidance=gd.cuda(), pooled_projections=pooled.cuda(),
                encoder_hidden_states=enc.cuda(), txt_ids=txt_ids.cuda(), img_ids=img_ids.cuda(), return_dict=False)


def _cos(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return (a @ b / (a.norm() * b.norm())).item()


def test_mxfp8_block_routes_give_the_same_bits():
    """FK_BLOCK_API 0 (per launch), 1 (per block), 2 (per forward): identical bits for a full-depth mxfp8 forward, call
    after call, at batch 2 with ragged row counts."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import flux_spec, transformer
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG)
    model = transformer.HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=31, weight_format="mxfp8")
    kw = _kw(2, 77, 10, 12, cfg, seed=4)
    saved = transformer.BLOCK_API
    try:
        outs = []
        for api in (0, 1, 2, 2, 1, 0):
            transformer.BLOCK_API = api
            outs.append(model(**kw)[0].clone())
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0].float()).all()
        for o in outs[1:]:
            assert torch.equal(o, outs[0])
        model.set_weight_format("bf16")
        assert not torch.equal(model(**kw)[0], outs[0])      # the format is really applied
    finally:
        transformer.BLOCK_API = saved


def test_mxfp8_format_switching_and_requantization():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import flux_spec, transformer
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=2, num_single_layers=2)
    kw = _kw(1, 64, 8, 8, cfg, seed=5)
    ref = transformer.HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=7)
    out_bf = ref(**kw)[0].clone()
    model = transformer.HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=7)
    serial0 = model.__dict__.get("_pack_serial", 0)
    model.set_weight_format("mxfp8")
    out_mx = model(**kw)[0].clone()
    assert model._pack_serial > serial0 and model.packed().format == "mxfp8"
    model.set_weight_format("bf16")
    assert torch.equal(model(**kw)[0], out_bf)             # exactly the bits of a model that never switched
    model.set_weight_format("mxfp8")
    assert torch.equal(model(**kw)[0], out_mx)
    # an in-place write to a (non-fused) block weight re-quantizes it: same output as a freshly packed model
    for name in ("transformer_blocks.1.ff.net.2.weight", "single_transformer_blocks.0.proj_out.weight",
                 "transformer_blocks.0.attn.to_q.weight"):
        with torch.no_grad():
            model.p(name).mul_(0.75)
    serial1 = model._pack_serial
    out_w = model(**kw)[0].clone()
    assert model._pack_serial > serial1 and not torch.equal(out_w, out_mx)
    fresh = transformer.HipFluxTransformer2DModel(cfg, device="cuda", weight_format="mxfp8")
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(fresh(**kw)[0], out_w)
    # save_pretrained keeps the bf16 parameters and today's config (no format key)
    assert "weight_format" not in vars(model.config)


@pytest.mark.timeout(1200, method="thread")
def test_mxfp8_full_depth_accuracy_against_the_oracle():
    """Full-depth (19 + 38 blocks) mxfp8 forward at S = 640 against the fp32 oracle (exact arithmetic on the bf16 weights)
    and at cfg 2's S = 2560 against the bf16 oracle; the bf16 path's figure beside it.  Asserted: cosine >= 0.99."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    from oracle import mmdit
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG)
    model = HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=17)
    for (S_txt, hw, seed, dtype) in ((128, 16, 6, torch.float32), (512, 32, 9, BF)):
        hs, enc, pooled, t, gd, img_ids, txt_ids = _inputs(1, S_txt, hw, hw, cfg, seed=seed)
        kw = _kw(1, S_txt, hw, hw, cfg, seed=seed)
        model.set_weight_format("bf16")
        out_bf = model(**kw)[0].float().cpu()
        model.set_weight_format("mxfp8")
        out_mx = model(**kw)[0].float().cpu()
        cast = (lambda x: x.float()) if dtype == torch.float32 else (lambda x: x)
        ref = mmdit.flux_forward(_StreamedState(model.state_dict(), dtype), cast(hs), cast(enc), cast(pooled), t, img_ids,
                                 txt_ids, gd, config=cfg).float()
        S = S_txt + 2 * hw * hw
        which = "fp32" if dtype == torch.float32 else "bf16"
        c_mx, c_bf = _cos(out_mx, ref), _cos(out_bf, ref)
        report(f"mxfp8 d19s38 S={S} vs {which}-oracle", out_mx, ref)
        report(f"bf16 d19s38 S={S} vs {which}-oracle", out_bf, ref)
        scale = ref.abs().max().item()
        print(f"[parity] full depth S={S} vs {which} oracle: cosine mxfp8 {c_mx:.6f}  bf16 {c_bf:.6f}; max|d|/scale mxfp8 "
              f"{(out_mx - ref).abs().max().item() / scale:.3e} bf16 {(out_bf - ref).abs().max().item() / scale:.3e}", flush=True)
        assert torch.isfinite(out_mx).all() and c_mx >= 0.99


def _edit_setup(use_graph):
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    from gpt_image_edit_amd.vae import HipAutoencoderKL
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=2, num_single_layers=4)
    tr = HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=3)
    vae = HipAutoencoderKL(device="cuda", init="synthetic", seed=4)
    return tr, [FluxKontextPipeline(tr, vae, use_graph=g) for g in use_graph]


def _edit(pipe, seed, steps, H=256):
    g = torch.Generator().manual_seed(seed)
    cond = torch.rand(1, 3, H, H, generator=g) * 2 - 1
    emb = torch.randn(1, 300, 4096, generator=g).to(BF)
    pooled = torch.randn(1, 768, generator=g).to(BF)
    noise = torch.randn(1, 16, H // 8, H // 8, generator=g).to(BF)
    out = pipe(image=cond.cuda(), prompt_embeds=emb.cuda(), pooled_prompt_embeds=pooled.cuda(), height=H, width=H,
               num_inference_steps=steps, guidance_scale=3.5, latents=pipe._pack_latents(noise, 1, 16, H // 8, H // 8).cuda(),
               output_type="pt_raw", max_area=H * H, _auto_resize=False)
    return out.latents.clone()


# mxfp8 vs bf16 latents after a 28-step edit (2 + 4 blocks, S = 812), as fractions of the bf16 latents' largest magnitude.
# Recorded on the MI355X: max 5.4e-2, mean 9.3e-3 (cosine 0.9989); asserted with 2x margin
EDIT28_MAX, EDIT28_MEAN = 0.11, 0.019


def test_mxfp8_graph_loop_and_28_step_edit():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tr, (eager, graphed) = _edit_setup((False, True))
    lat_bf = _edit(eager, 1, 28)
    tr.set_weight_format("mxfp8")
    lat_mx = _edit(eager, 1, 28)
    for seed in (2, 3):                   # seed 2 captures, 3 replays with new inputs
        le, lg = _edit(eager, seed, 6), _edit(graphed, seed, 6)
        torch.cuda.synchronize()
        assert torch.equal(le, lg), f"graph replay differs from the eager mxfp8 loop (seed {seed})"
    scale = lat_bf.float().abs().max().item()
    d = (lat_mx.float() - lat_bf.float()).abs()
    print(f"[parity] 28-step edit mxfp8 vs bf16 latents: max {d.max().item() / scale:.3e} mean {d.mean().item() / scale:.3e} "
          f"of scale {scale:.2f}; cosine {_cos(lat_mx.float(), lat_bf.float()):.6f}", flush=True)
    assert torch.isfinite(lat_mx.float()).all()
    assert d.max().item() <= EDIT28_MAX * scale and d.mean().item() <= EDIT28_MEAN * scale


def test_gemm_mxfp8_rejects_inconsistent_epilogue_arguments():
    """The QKV / GATE_RES / output fields are checked like fk_gemm_bf16's before anything launches."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops
    M, N, K = 64, 768, 256
    aq = ops.quantize_mxfp8(torch.randn(M, K, device="cuda").to(BF))
    wq = ops.quantize_mxfp8(torch.randn(N, K, device="cuda").to(BF))
    q = torch.empty(1, 2, 64, 128, dtype=BF, device="cuda")
    nw = torch.ones(128, dtype=BF, device="cuda")
    cs = torch.zeros(64, 64, 2, device="cuda")
    good = dict(q_out=q, k_out=torch.empty_like(q), wq=nw, wk=nw, cs=cs, s_offset=0)
    ops.gemm_mxfp8(aq, wq, epilogue=ops.FK_EPI_QKV, qkv=good)        # N = 3 * 2 * 128: accepted
    with pytest.raises(RuntimeError, match="N = 3\\*H\\*128"):
        ops.gemm_mxfp8(aq, wq, epilogue=ops.FK_EPI_QKV, qkv=dict(good, q_out=q[:, :1], k_out=q[:, :1]))    # H = 1: N != 3 * 128
    with pytest.raises(RuntimeError, match="exceed S_total"):
        ops.gemm_mxfp8(aq, wq, epilogue=ops.FK_EPI_QKV, qkv=dict(good, s_offset=10))
    with pytest.raises(RuntimeError, match="gate pointer"):
        out = torch.zeros(1, M, N, dtype=BF, device="cuda")
        ops.gemm_mxfp8(aq, wq, out=out, epilogue=ops.FK_EPI_GATE_RES, res=out, gate=torch.zeros(1, N + 1, dtype=BF, device="cuda")[:, 1:])
    with pytest.raises(RuntimeError, match="epilogue"):
        ops.gemm_mxfp8(aq, wq, epilogue=ops.FK_EPI_GELU_TANH, out_fp32=True)
