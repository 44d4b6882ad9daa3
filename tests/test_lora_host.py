"""CPU tests of the LoRA host layer (gpt_image_edit_amd/lora.py, the model's adapter API, the command-line flags): key
parsing and refusals, the effective-scale arithmetic, merge-only-on-change (counted through a stubbed ``ops.lora_merge``),
the more-than-four error and the refusals around training."""
import pytest
import torch

BF16 = torch.bfloat16
Q = "transformer_blocks.0.attn.to_q"
FF = "transformer_blocks.0.ff.net.0.proj"
PM = "single_transformer_blocks.1.proj_mlp"


def _state(mods, prefix="transformer.", alpha=None, seed=0):
    """{module: (N, K, r)} -> a PEFT-layout state dict."""
    g = torch.Generator().manual_seed(seed)
    st = {}
    for m, (N, K, r) in mods.items():
        st[f"{prefix}{m}.lora_A.weight"] = torch.randn(r, K, generator=g)
        st[f"{prefix}{m}.lora_B.weight"] = torch.randn(N, r, generator=g)
        if alpha is not None:
            st[f"{prefix}{m}.alpha"] = torch.tensor(float(alpha))
    return st


def test_parse_prefix_alpha_and_ignored_keys(tmp_path):
    from gpt_image_edit_amd import lora
    st = _state({Q: (128, 128, 8)}, alpha=4)
    st.update(_state({FF: (512, 128, 33)}))
    st["text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_A.weight"] = torch.zeros(4, 8)
    st["text_encoder_2.encoder.block.0.layer.0.SelfAttention.q.lora_B.weight"] = torch.zeros(8, 4)
    mods, ignored = lora.parse_lora_state(st)
    assert set(mods) == {Q, FF} and len(ignored) == 2 and all(k.startswith("text_encoder") for k in ignored)
    assert (mods[Q].rank, mods[Q].alpha) == (8, 4.0) and (mods[FF].rank, mods[FF].alpha) == (33, 33.0)
    assert mods[Q].down.shape == (8, 128) and mods[Q].up.shape == (128, 8)
    # another prefix; and the same through a safetensors file
    mods2, _ = lora.parse_lora_state(_state({Q: (128, 128, 8)}, prefix="unet."), prefix="unet.")
    assert set(mods2) == {Q}
    st_mod, _ = pytest.importorskip("safetensors.torch"), None
    path = tmp_path / "a.safetensors"
    st_mod.save_file({k: v.contiguous() for k, v in st.items()}, str(path))
    mods3, ignored3 = lora.parse_lora_state(str(path))
    assert set(mods3) == {Q, FF} and len(ignored3) == 2 and torch.equal(mods3[FF].up, mods[FF].up) and mods3[Q].alpha == 4.0


@pytest.mark.parametrize("key,tensor", [
    ("transformer." + Q + ".lora_B.bias", torch.zeros(128)),
    ("transformer.transformer_blocks.0.attn.norm_q.weight", torch.zeros(128)),
    ("transformer." + Q + ".bias", torch.zeros(128)),
    ("double_blocks.0.img_attn.qkv.lora_A.weight", torch.zeros(8, 128)),                       # BFL
    ("lora_unet_double_blocks_0_img_attn_qkv.lora_down.weight", torch.zeros(8, 128)),          # kohya
    ("transformer.transformer_blocks.0.attn.to_qkv.lora_down.weight", torch.zeros(8, 128)),
])
def test_parser_refusals_name_the_key(key, tensor):
    from gpt_image_edit_amd import lora
    st = _state({Q: (128, 128, 8)})
    st[key] = tensor
    with pytest.raises(ValueError) as e:
        lora.parse_lora_state(st)
    assert key in str(e.value)


def test_parser_names_at_most_five_keys_and_incomplete_pairs():
    from gpt_image_edit_amd import lora
    st = {f"bad.{i}.weight": torch.zeros(1) for i in range(8)}
    with pytest.raises(ValueError) as e:
        lora.parse_lora_state(st)
    assert sum(f"bad.{i}.weight" in str(e.value) for i in range(8)) == 5 and "8 keys" in str(e.value)
    half = {"transformer." + Q + ".lora_A.weight": torch.zeros(8, 128)}
    with pytest.raises(ValueError, match="lora_A"):
        lora.parse_lora_state(half)
    mismatch = {"transformer." + Q + ".lora_A.weight": torch.zeros(8, 128), "transformer." + Q + ".lora_B.weight": torch.zeros(128, 4)}
    with pytest.raises(ValueError, match="to_q"):
        lora.parse_lora_state(mismatch)


@pytest.fixture()
def model(monkeypatch):
    """A one-head (D = 128) model on the CPU and a stub of ops.lora_merge that records its calls and writes fp32 torch's
    result (the kernel itself is tests/test_hip_lora_kernel.py's business)."""
    from gpt_image_edit_amd import flux_spec, ops
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2, num_attention_heads=1)
    m = HipFluxTransformer2DModel(cfg, device="cpu", init="empty")
    g = torch.Generator().manual_seed(3)
    for p in m.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g) * 0.05)
    calls = []

    def stub(base, terms, out=None):
        out = base if out is None else out
        calls.append([(tuple(up.shape), float(s)) for up, down, s in terms])
        v = base.float()
        for up, down, s in terms:
            v = v + float(s) * (up.float() @ down.float())
        out.copy_(v.to(BF16))
        return out

    monkeypatch.setattr(ops, "lora_merge", stub)
    m.calls = calls
    return m


def test_model_refuses_what_does_not_fit(model):
    with pytest.raises(ValueError) as e:
        model.load_lora_adapter(_state({"transformer_blocks.7.attn.to_q": (128, 128, 8)}))
    assert "transformer.transformer_blocks.7.attn.to_q.lora_A.weight" in str(e.value)
    with pytest.raises(ValueError) as e:
        model.load_lora_adapter(_state({Q: (128, 64, 8)}))
    assert "transformer." + Q + ".lora_B.weight" in str(e.value)
    with pytest.raises(ValueError, match="to_q"):
        model.load_lora_adapter(_state({Q: (128, 128, 129)}))
    with pytest.raises(ValueError, match="norm_q"):       # a 1-D parameter is no Linear weight
        model.load_lora_adapter(_state({"transformer_blocks.0.attn.norm_q": (128, 1, 1)}))
    assert not model.lora_loaded() and not model.calls and not model._lora_base


def test_effective_scale_and_merge_only_on_change(model):
    model._packed = "stale"
    ignored = model.load_lora_adapter({**_state({Q: (128, 128, 8), FF: (512, 128, 8)}, alpha=4),
                                       "text_encoder.x.lora_A.weight": torch.zeros(1, 1)}, adapter_name="a", weight=0.5)
    assert ignored == ["text_encoder.x.lora_A.weight"]
    assert model.active_adapters() == ["a"] and model._packed is None
    assert sorted(model.calls) == [[((128, 8), 0.25)], [((512, 8), 0.25)]]           # 0.5 x 1.0 x 4 / 8, one launch per weight
    assert set(model._lora_base) == {Q + ".weight", FF + ".weight"} and not any(k.startswith("_lora") for k in model.state_dict())
    del model.calls[:]
    model.load_lora_adapter(_state({Q: (128, 128, 33)}, seed=1), adapter_name="b")
    assert model.calls == [[((128, 8), 0.25), ((128, 33), 1.0)]]                     # only to_q changed; both adapters as its terms
    del model.calls[:]
    model._packed = "kept"
    model.set_lora_scale(1.0), model.set_adapters(["a", "b"], [0.5, 1.0])            # nothing changed: no merge, packs kept
    assert model.calls == [] and model._packed == "kept"
    model.set_lora_scale(0.5)
    assert sorted(model.calls) == sorted([[((128, 8), 0.125), ((128, 33), 0.5)], [((512, 8), 0.125)]]) and model._packed is None
    del model.calls[:]
    model.set_adapters(["b", "a"], [1.0, 0.5])                                       # order is part of the tuple: to_q only
    assert model.calls == [[((128, 33), 0.5), ((128, 8), 0.125)]]
    del model.calls[:]
    model.set_adapters("b", 3.0)                                                     # a leaves: ff goes back to its base
    assert model.calls == [[((128, 33), 1.5)]]
    assert torch.equal(model.p(FF + ".weight").data, model._lora_base[FF + ".weight"])
    s = float(torch.tensor(0.3 * 0.7 * 4 / 8, dtype=torch.float32))
    del model.calls[:]
    model.set_adapters(["a"], [0.3]), model.set_lora_scale(0.7)
    assert model.calls[-1] in ([((128, 8), s)], [((512, 8), s)])


def test_every_merge_is_from_the_base_and_unload_is_exact(model):
    orig = {n: p.data.clone() for n, p in model.named_parameters()}
    model.load_lora_adapter(_state({Q: (128, 128, 8), PM: (512, 128, 8)}), adapter_name="a")
    once = model.p(Q + ".weight").data.clone()
    assert not torch.equal(once, orig[Q + ".weight"])
    model.set_lora_scale(0.25), model.set_lora_scale(1.0)
    assert torch.equal(model.p(Q + ".weight").data, once)                            # not merged on top of a merged weight
    model.load_lora_adapter(_state({Q: (128, 128, 4)}, seed=5), adapter_name="b")
    model.delete_adapters("a")
    both_gone_then_b = model.p(Q + ".weight").data.clone()
    model.unload_lora()
    assert all(torch.equal(p.data, orig[n]) for n, p in model.named_parameters())
    assert not model._lora_base and not model.lora_loaded() and model.active_adapters() == []
    model.load_lora_adapter(_state({Q: (128, 128, 4)}, seed=5), adapter_name="b")
    assert torch.equal(model.p(Q + ".weight").data, both_gone_then_b)                # A, B, delete A == B alone
    model.unload_lora(), model.unload_lora()
    assert all(torch.equal(p.data, orig[n]) for n, p in model.named_parameters())


def test_more_than_four_adapters_on_one_weight(model):
    for i in range(4):
        model.load_lora_adapter(_state({Q: (128, 128, 4)}, seed=i), adapter_name=f"a{i}")
    before = model.p(Q + ".weight").data.clone()
    with pytest.raises(ValueError, match="more than 4 active adapters.*to_q"):
        model.load_lora_adapter(_state({Q: (128, 128, 4)}, seed=9), adapter_name="a4")
    assert model.active_adapters() == ["a0", "a1", "a2", "a3"] and torch.equal(model.p(Q + ".weight").data, before)
    model.load_lora_adapter(_state({FF: (512, 128, 4)}, seed=9), adapter_name="a4")   # another weight: fine
    with pytest.raises(ValueError, match="already loaded"):
        model.load_lora_adapter(_state({FF: (512, 128, 4)}), adapter_name="a4")
    with pytest.raises(ValueError, match="not loaded"):
        model.set_adapters(["nope"])


def test_refusals_around_training(model):
    from gpt_image_edit_amd.backward import FluxBackward
    model.load_lora_adapter(_state({Q: (128, 128, 4)}), adapter_name="a")
    with pytest.raises(RuntimeError, match="LoRA"):
        FluxBackward(model)
    assert not model._train_packs
    model.unload_lora()
    model._train_packs = True
    with pytest.raises(RuntimeError, match="training"):
        model.load_lora_adapter(_state({Q: (128, 128, 4)}), adapter_name="a")
    assert not model.lora_loaded()


def test_cli_flags():
    from gpt_image_edit_amd import lora
    from gpt_image_edit_amd.eval import gen_samples
    from gpt_image_edit_amd.serve import cli
    a = cli.build_parser().parse_args(["--model_path", "m", "--flux_path", "f", "--lora", "x.safetensors:0.5", "--lora", "dir/y.safetensors",
                                       "--lora_scale", "0.75"])
    assert a.lora == ["x.safetensors:0.5", "dir/y.safetensors"] and a.lora_scale == 0.75
    assert [lora.parse_lora_arg(s) for s in a.lora] == [("x.safetensors", 0.5), ("dir/y.safetensors", 1.0)]
    assert lora.parse_lora_arg("a:b.safetensors") == ("a:b.safetensors", 1.0) and lora.parse_lora_arg("p:-2") == ("p", -2.0)
    assert cli.lora_kwargs(a) == {"joint_attention_kwargs": {"scale": 0.75}}
    d = cli.build_parser().parse_args(["--model_path", "m", "--flux_path", "f"])
    assert d.lora == [] and d.lora_scale == 1.0 and cli.lora_kwargs(d) == {}
    g = gen_samples.build_parser().parse_args(["--model_path", "m", "--flux_path", "f", "--gedit_prompt_path", "p", "--output_dir", "o",
                                               "--lora", "z:2"])
    assert g.lora == ["z:2"] and g.lora_scale == 1.0

    class Pipe:
        def __init__(self): self.seen = []
        def load_lora_weights(self, path, adapter_name="default"): self.seen.append((path, adapter_name))
        def set_adapters(self, names, weights=None): self.seen.append((names, weights))
    p = Pipe()
    assert lora.load_cli_adapters(p, a.lora) == ["lora0", "lora1"]
    assert p.seen == [("x.safetensors", "lora0"), ("dir/y.safetensors", "lora1"), (["lora0", "lora1"], [0.5, 1.0])]
    assert lora.load_cli_adapters(Pipe(), []) == []
