"""CPU tests of the LoRA training host layer (``LoraMixin.add_lora_adapter`` / ``lora_mark_stale`` / ``lora_state_dict``,
``FluxBackward(lora=)``, ``DenoiserTrainStep(lora=)``) with the ops stubbed, as tests/test_lora_host.py does: target selection
and its refusals, the initialisation, parameter names, the refusals, one merge per touched weight after an optimiser step, and
the two round trips (saved adapter, ``kind="lora"`` optimiser state)."""
import pytest
import torch

BF16 = torch.bfloat16
D0, S0, S1 = "transformer_blocks.0.", "single_transformer_blocks.0.", "single_transformer_blocks.1."
QKV = ("to_q", "to_k", "to_v")
DEFAULT = sorted([D0 + f"attn.{n}.weight" for n in QKV + ("to_out.0",)] + [s + f"attn.{n}.weight" for s in (S0, S1) for n in QKV])


@pytest.fixture()
def model(monkeypatch):
    """The one-head (D = 128) CPU model of tests/test_lora_host.py; ops.lora_merge / sumsq / adamw_step as torch stubs."""
    from gpt_image_edit_amd import flux_spec, ops
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2, num_attention_heads=1)
    m = HipFluxTransformer2DModel(cfg, device="cpu", init="empty")
    g = torch.Generator().manual_seed(3)
    for p in m.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g) * 0.05)
    merges = []

    def merge(base, terms, out=None):
        out = base if out is None else out
        merges.append(tuple(base.shape))
        v = base.float()
        for up, down, s in terms:
            v = v + float(s) * (up.float() @ down.float())
        out.copy_(v.to(BF16))
        return out

    def sumsq(tensors, out=None):
        return torch.stack([t.double().pow(2).sum() for t in tensors]).sum().reshape(1)

    def adamw_step(master, grad, exp_avg, exp_avg_sq, step, lr, betas=None, eps=None, weight_decay=None, grad_sumsq=None,
                   max_grad_norm=None, param_bf16=None, grad_scale=1.0):
        exp_avg.add_(grad.float())
        exp_avg_sq.add_(grad.float() ** 2)
        master.sub_(lr * grad.float())
        param_bf16.copy_(master)

    monkeypatch.setattr(ops, "lora_merge", merge)
    monkeypatch.setattr(ops, "sumsq", sumsq)
    monkeypatch.setattr(ops, "adamw_step", adamw_step)
    m.merges = merges
    return m


def test_default_and_suffix_target_selection(model):
    assert model.add_lora_adapter("t", rank=4) == DEFAULT
    assert model.active_adapters() == ["t"] and len(model.merges) == len(DEFAULT)
    e = model._lora_adapters["t"][DEFAULT[0]]
    assert (e.rank, e.alpha) == (4, 4.0)                                   # alpha defaults to the rank
    model.unload_lora()
    # a suffix names every module that ends in it; q / k / v of an attention come as a group
    assert model.add_lora_adapter("q", rank=2, alpha=8, target_modules=["to_q"]) == sorted(
        p + f"attn.{n}.weight" for p in (D0, S0, S1) for n in QKV)
    assert model._lora_adapters["q"][D0 + "attn.to_k.weight"].alpha == 8.0
    assert model.add_lora_adapter("a", rank=2, target_modules="add_k_proj") == sorted(
        D0 + f"attn.{n}.weight" for n in ("add_q_proj", "add_k_proj", "add_v_proj"))
    assert model.add_lora_adapter("m", rank=2, target_modules=["ff.net.2", "proj_mlp", S1 + "proj_out.weight"]) == sorted(
        [D0 + "ff.net.2.weight", S0 + "proj_mlp.weight", S1 + "proj_mlp.weight", S1 + "proj_out.weight"])
    assert model.active_adapters() == ["q", "a", "m"]


@pytest.mark.parametrize("targets,named", [(["x_embedder"], "x_embedder.weight"), (["norm_q"], "attn.norm_q.weight"),
                                           (["to_q", "nope"], "nope"), (["proj_out"], "proj_out.weight"),
                                           ([D0 + "norm1.linear.bias"], "norm1.linear.bias")])
def test_target_refusals_name_the_keys(model, targets, named):
    with pytest.raises(ValueError) as e:
        model.add_lora_adapter("t", rank=4, target_modules=targets)
    assert named in str(e.value)
    assert not model.lora_loaded() and not model.merges and not model._lora_base


def test_other_refusals(model):
    for rank in (0, 129):
        with pytest.raises(ValueError, match="rank"):
            model.add_lora_adapter("t", rank=rank)
    model.add_lora_adapter("t", rank=4)
    with pytest.raises(ValueError, match="already loaded"):
        model.add_lora_adapter("t", rank=4)
    model._train_packs = True
    with pytest.raises(RuntimeError, match="training"):
        model.add_lora_adapter("u", rank=4)
    with pytest.raises(ValueError, match="not loaded"):
        model.lora_state_dict("nope")


def test_initialisation(model):
    before = {n: p.data.clone() for n, p in model.named_parameters()}
    model.add_lora_adapter("t", rank=8, seed=5)
    assert all(torch.equal(p.data, before[n]) for n, p in model.named_parameters())      # up = 0: the base weights bit for bit
    ent = model._lora_adapters["t"]
    for pname, e in ent.items():
        N, K = model.p(pname).shape
        assert e.up.shape == (N, 8) and e.down.shape == (8, K) and e.up.dtype == e.down.dtype == BF16
        assert not bool(e.up.any()) and bool(e.down.any())
        assert float(e.down.float().abs().max()) <= K ** -0.5 and float(e.down.float().abs().max()) > 0.5 * K ** -0.5
    model.unload_lora()
    model.add_lora_adapter("again", rank=8, seed=5)
    model.add_lora_adapter("other", rank=8, seed=6)
    again, other = model._lora_adapters["again"], model._lora_adapters["other"]
    assert all(torch.equal(again[p].down, ent[p].down) for p in ent)
    assert not any(torch.equal(other[p].down, ent[p].down) for p in ent)


def test_backward_refuses_by_default_and_accepts_with_the_keyword(model):
    from gpt_image_edit_amd.backward import FluxBackward
    model.add_lora_adapter("t", rank=4, target_modules=[S0 + "attn.to_k", D0 + "ff.net.2"])
    with pytest.raises(RuntimeError, match="LoRA"):
        FluxBackward(model)
    assert not model._train_packs
    bw = FluxBackward(model, lora="t")
    assert bw.trainable == {S0 + f"attn.{n}.weight" for n in QKV} | {D0 + "ff.net.2.weight"} and model._train_packs
    with pytest.raises(RuntimeError, match="training"):
        model.load_lora_adapter({}, adapter_name="late")


def test_train_step_names_and_refusals(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    model.add_lora_adapter("t", rank=4, weight=0.5)
    model.set_lora_scale(0.25)
    with pytest.raises(ValueError, match="not built"):
        DenoiserTrainStep(model, lora="t", sharded=True)
    with pytest.raises(ValueError, match="not loaded"):
        DenoiserTrainStep(model, lora="nope")
    with pytest.raises(ValueError, match="trainable"):
        DenoiserTrainStep(model, lora="t", trainable=DEFAULT)
    assert not model._train_packs
    ts = DenoiserTrainStep(model, lora="t")
    assert model._lora_scale == 1.0                                         # the train step sets the call scale to 1.0
    assert ts.trainable_names() == {p[:-len("weight")] + s for p in DEFAULT for s in ("lora_A.weight", "lora_B.weight")}
    e = model._lora_adapters["t"][DEFAULT[0]]
    stem = DEFAULT[0][:-len("weight")]
    assert ts._param(stem + "lora_A.weight") is e.down and ts._param(stem + "lora_B.weight") is e.up
    assert ts.bw.trainable == set(DEFAULT)


def _fake_grads(ts, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(ts._param(k).shape, generator=g) for k in sorted(ts.trainable_names())}


def test_optimizer_step_remerges_exactly_the_touched_weights(model):
    from gpt_image_edit_amd import lora
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    g = torch.Generator().manual_seed(1)
    frozen = {f"transformer.{D0}ff.net.0.proj.lora_A.weight": torch.randn(4, 128, generator=g),
              f"transformer.{D0}ff.net.0.proj.lora_B.weight": torch.randn(512, 4, generator=g),
              f"transformer.{D0}attn.to_q.lora_A.weight": torch.randn(4, 128, generator=g),
              f"transformer.{D0}attn.to_q.lora_B.weight": torch.randn(128, 4, generator=g)}
    model.load_lora_adapter(frozen, adapter_name="f")
    model.add_lora_adapter("t", rank=4)
    ts = DenoiserTrainStep(model, lora="t", lr=0.5)
    before = {n: p.data.clone() for n, p in model.named_parameters()}
    del model.merges[:]
    from types import SimpleNamespace
    kept = model._packed = SimpleNamespace(mod_w=None, copies=[], sources=[], versions=None)
    ts.optimizer_step(_fake_grads(ts))
    assert len(model.merges) == len(DEFAULT), "one merge per touched weight, none elsewhere"
    assert sorted(model.merges) == sorted(tuple(model.p(p).shape) for p in DEFAULT)
    assert model._packed is kept                                            # refresh() re-copies in place; nothing is re-packed
    changed = sorted(n for n, p in model.named_parameters() if not torch.equal(p.data, before[n]))
    assert changed == DEFAULT
    # every merge is from the saved base with both adapters' terms where both are active
    q = D0 + "attn.to_q.weight"
    e, f = model._lora_adapters["t"][q], model._lora_adapters["f"][q]
    want = (model._lora_base[q].float() + f.up.float() @ f.down.float() + e.up.float() @ e.down.float()).to(BF16)
    assert torch.equal(model.p(q).data, want)
    assert ts.step_count == 1 and set(ts.state) == ts.trainable_names()
    del model.merges[:]
    model._lora_sync()
    assert model.merges == []                                               # nothing is stale any more
    # the saved adapter is what parse_lora_state reads
    sd = model.lora_state_dict("t")
    assert set(sd) == {f"transformer.{p[:-len('weight')]}{s}" for p in DEFAULT for s in ("lora_A.weight", "lora_B.weight", "alpha")}
    mods, ignored = lora.parse_lora_state(sd)
    assert ignored == [] and set(mods) == {p[:-len(".weight")] for p in DEFAULT}
    for mod, m in mods.items():
        e = model._lora_adapters["t"][mod + ".weight"]
        assert torch.equal(m.up, e.up) and torch.equal(m.down, e.down) and m.alpha == e.alpha == 4.0 and m.rank == 4
        assert m.up.dtype == BF16 and bool(m.up.any())
    assert set(model.lora_state_dict("t", prefix="unet.")) == {k.replace("transformer.", "unet.", 1) for k in sd}


def test_lora_optimizer_state_round_trips(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    model.add_lora_adapter("t", rank=4, seed=2)
    base = {n: p.data.clone() for n, p in model.named_parameters()}
    ts = DenoiserTrainStep(model, lora="t", lr=0.5)
    ts.optimizer_step(_fake_grads(ts, 1))
    ts.optimizer_step(_fake_grads(ts, 2))
    sd = ts.state_dict()
    assert sd["kind"] == "lora" and sd["step"] == 2 and set(sd["state"]) == ts.trainable_names()
    trained = {n: p.data.clone() for n, p in model.named_parameters()}
    # a new step object on a new model with a fresh adapter of the same targets
    for n, p in model.named_parameters():
        p.data.copy_(base[n])
    model._lora_init()
    model._train_packs = False
    model.add_lora_adapter("t", rank=4, seed=9)
    ts2 = DenoiserTrainStep(model, lora="t", lr=0.5)
    del model.merges[:]
    ts2.load_state_dict(sd)
    assert ts2.step_count == 2 and len(model.merges) == len(DEFAULT)
    assert all(torch.equal(p.data, trained[n]) for n, p in model.named_parameters())
    for k, st in ts.state.items():
        assert all(torch.equal(a, b) for a, b in zip(st, ts2.state[k]))
        assert torch.equal(ts2._param(k), st[0].to(BF16))
    g3 = _fake_grads(ts, 3)
    ts.optimizer_step(g3), ts2.optimizer_step({k: v.clone() for k, v in g3.items()})
    assert all(torch.equal(a, b) for k in ts.state for a, b in zip(ts.state[k], ts2.state[k]))
    with pytest.raises(ValueError, match="lora"):
        ts2.load_state_dict(dict(kind="per_tensor", step=0, state={}))
