"""CPU tests of the Prodigy host layer (``DenoiserTrainStep(optimizer="prodigy")``, ``zero.ShardedAdamW(optimizer="prodigy")``) with
the ops stubbed as tests/test_lora_train_host.py does (tests/prodigy_stub.py): argument resolution and refusals, the 5-tuple state,
the order of the op calls, one re-merge per touched weight after a LoRA step, both ``state_dict`` round trips with the
cross-optimiser refusal, and that the default and ``optimizer="adamw"`` issue the same op calls."""
import pytest
import torch

import prodigy_stub as S

BF16 = torch.bfloat16
D0, S0, S1 = "transformer_blocks.0.", "single_transformer_blocks.0.", "single_transformer_blocks.1."
QKV = ("to_q", "to_k", "to_v")
DEFAULT = sorted([D0 + f"attn.{n}.weight" for n in QKV + ("to_out.0",)] + [s + f"attn.{n}.weight" for s in (S0, S1) for n in QKV])
FULL = [D0 + "attn.to_q.weight", S0 + "proj_out.bias", S1 + "attn.to_k.weight"]


@pytest.fixture()
def model(monkeypatch):
    """The one-head (D = 128) CPU model of tests/test_lora_train_host.py; the Prodigy ops, sumsq, adamw_step and lora_merge as stubs."""
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

    def adamw_step(master, grad, exp_avg, exp_avg_sq, step, lr, betas=None, eps=None, weight_decay=None, grad_sumsq=None,
                   max_grad_norm=None, param_bf16=None, grad_scale=1.0):
        S.calls.append(("adamw", master.numel(), step, lr, tuple(betas), eps, weight_decay, max_grad_norm))
        master.sub_(lr * grad.float())
        param_bf16.copy_(master)

    S.install(monkeypatch, ops)
    monkeypatch.setattr(ops, "lora_merge", merge)
    monkeypatch.setattr(ops, "adamw_step", adamw_step)
    m.merges = merges
    return m


def _fake_grads(ts, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return {k: scale * torch.randn(ts._param(k).shape, generator=g) for k in sorted(ts.trainable_names())}


def test_argument_resolution_and_refusals(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    from gpt_image_edit_amd.zero import PRODIGY_DEFAULTS, resolve_optimizer
    assert resolve_optimizer("adamw", None, None) == ("adamw", 1e-6, None)
    assert resolve_optimizer("adamw", 3e-4, None) == ("adamw", 3e-4, None)
    assert resolve_optimizer("prodigy", None, None) == ("prodigy", 1.0, PRODIGY_DEFAULTS)
    assert PRODIGY_DEFAULTS == dict(beta3=None, d0=1e-6, d_coef=1.0, growth_rate=float("inf"), use_bias_correction=True,
                                    safeguard_warmup=True, decouple=True)
    _, lr, hp = resolve_optimizer("prodigy", 0.5, dict(d_coef=2.0, safeguard_warmup=False))
    assert lr == 0.5 and hp["d_coef"] == 2.0 and hp["safeguard_warmup"] is False and hp["decouple"] is True
    for lr in (0.1, 1e-6, 0.0, -1.0):
        with pytest.raises(ValueError, match="lr"):
            resolve_optimizer("prodigy", lr, None)
    with pytest.raises(ValueError, match="optimizer"):
        resolve_optimizer("sgd", None, None)
    with pytest.raises(ValueError, match="unknown keys nope"):
        resolve_optimizer("prodigy", None, dict(nope=1))
    with pytest.raises(ValueError, match="adamw"):
        resolve_optimizer("adamw", None, dict(d0=1e-5))
    for bad in (dict(d0=0.0), dict(d_coef=-1.0), dict(growth_rate=1.0), dict(beta3=1.0)):
        with pytest.raises(ValueError):
            resolve_optimizer("prodigy", None, bad)
    # the train step resolves through the same function, before it touches the model
    for kw in (dict(optimizer="lion"), dict(optimizer="prodigy", lr=1e-4), dict(prodigy=dict(d0=1e-5))):
        with pytest.raises(ValueError):
            DenoiserTrainStep(model, trainable=FULL, **kw)
    assert not model._train_packs
    ts = DenoiserTrainStep(model, trainable=FULL)
    assert (ts.optimizer, ts.lr, ts.prodigy) == ("adamw", 1e-6, None)
    with pytest.raises(RuntimeError, match="adamw"):
        ts.prodigy_state()


def test_five_tuple_state_and_call_order(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    ts = DenoiserTrainStep(model, trainable=FULL, optimizer="prodigy", weight_decay=0.01, prodigy=dict(d0=1e-4))
    assert ts.lr == 1.0 and ts.prodigy["d0"] == 1e-4 and ts.trainable_names() == set(FULL)
    assert ts.prodigy_state()["d"] == 1e-4 and ts.prodigy_state()["k"] == 0            # before the first step: no buffer yet
    start = {k: ts._param(k).data.clone() for k in FULL}
    sumsq = ts.optimizer_step(_fake_grads(ts))
    assert sumsq.dtype == torch.float64 and ts.step_count == 1
    sizes = [ts._param(k).numel() for k in sorted(FULL)]
    assert S.calls == [("sumsq", 3), ("begin",)] + [("moments", n) for n in sizes] + [("update_d",)] + [("apply", n) for n in sizes]
    for k in FULL:
        st = ts.state[k]
        assert len(st) == 5 and all(t.dtype == torch.float32 and t.shape == start[k].shape for t in st)
        master, m, v, s, p0 = st
        assert torch.equal(p0, start[k].float()), "p0 is the bf16 parameter at state creation"
        assert bool(m.any()) and bool(v.any()) and bool(s.any())
    assert ts.prodigy_state()["k"] == 1 and not ts.prodigy_state()["skipped"]
    # a zero gradient from the start: the step is skipped on the device, nothing moves
    model2_ts = DenoiserTrainStep(model, trainable=FULL, optimizer="prodigy")
    before = {k: model2_ts._param(k).data.clone() for k in FULL}
    model2_ts.optimizer_step({k: torch.zeros_like(v) for k, v in _fake_grads(model2_ts).items()})
    assert model2_ts.prodigy_state()["skipped"] and model2_ts.prodigy_state()["k"] == 0
    assert all(torch.equal(model2_ts._param(k).data, before[k]) for k in FULL)


def test_default_and_adamw_issue_the_same_op_calls(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    logs = []
    start = {k: model.p(k).data.clone() for k in FULL}
    for kw in (dict(), dict(optimizer="adamw"), dict(optimizer="adamw", lr=None, prodigy=None)):
        for k in FULL:
            model.p(k).data.copy_(start[k])
        model._train_packs = False
        ts = DenoiserTrainStep(model, trainable=FULL, **kw)
        del S.calls[:]
        ts.optimizer_step(_fake_grads(ts))
        ts.optimizer_step(_fake_grads(ts, 1))
        logs.append(list(S.calls))
        assert all(len(st) == 3 for st in ts.state.values()) and ts.pstate is None
        assert set(ts.state_dict()) == {"kind", "step", "state"}, "an AdamW state keeps exactly its keys"
    assert logs[0] == logs[1] == logs[2]
    assert [c[0] for c in logs[0]] == ["sumsq"] + ["adamw"] * 3 + ["sumsq"] + ["adamw"] * 3
    assert logs[0][1][2:] == (1, 1e-6, (0.9, 0.99), 1e-8, 0.0, 1.0)


def test_lora_step_remerges_exactly_the_touched_weights(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    model.add_lora_adapter("t", rank=4)
    ts = DenoiserTrainStep(model, lora="t", optimizer="prodigy")
    before = {n: p.data.clone() for n, p in model.named_parameters()}
    del model.merges[:]
    ts.optimizer_step(_fake_grads(ts, scale=1e-2))
    assert len(model.merges) == len(DEFAULT), "one merge per touched weight, none elsewhere"
    assert sorted(n for n, p in model.named_parameters() if not torch.equal(p.data, before[n])) == DEFAULT
    for k, st in ts.state.items():
        assert len(st) == 5
        if k.endswith(ts.LORA_B):
            assert not bool(st[4].any()), "up starts at 0, so its p0 is 0"
        else:
            assert bool(st[4].any())
    for _ in range(3):
        ts.optimizer_step(_fake_grads(ts, scale=1e-2))
    assert ts.prodigy_state()["k"] == 4


def test_per_tensor_state_round_trips_and_the_other_optimiser_is_refused(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    start = {k: model.p(k).data.clone() for k in FULL}
    kw = dict(trainable=FULL, optimizer="prodigy", weight_decay=0.01, prodigy=dict(d0=1e-3, use_bias_correction=False, safeguard_warmup=False))
    ts = DenoiserTrainStep(model, **kw)
    for i in range(3):
        ts.optimizer_step(_fake_grads(ts, 0, 0.1))               # the same gradient again: p0 - p points along it, d grows
    sd = ts.state_dict()
    assert sd["optimizer"] == "prodigy" and sd["kind"] == "per_tensor" and sd["step"] == 3 and sd["scalars"].dtype == torch.float64
    assert sd["hp"]["d0"] == 1e-3 and sd["hp"]["lr"] == 1.0 and sd["hp"]["weight_decay"] == 0.01
    assert all(len(st) == 5 for st in sd["state"].values())
    assert ts.prodigy_state()["d"] > 1e-3, "d did not move in three steps: the resume check below would not see the scalars"
    for k in FULL:
        model.p(k).data.copy_(start[k])
    model._train_packs = False
    ts2 = DenoiserTrainStep(model, **kw)
    ts2.load_state_dict(sd)
    assert ts2.step_count == 3 and ts2.prodigy_state() == ts.prodigy_state()
    g = _fake_grads(ts, 9, 0.1)
    trained = {k: ts.state[k][0].clone() for k in FULL}
    assert all(torch.equal(ts2._param(k).data, trained[k].to(BF16)) for k in FULL)
    ts2.optimizer_step({k: v.clone() for k, v in g.items()})
    for k in FULL:                                             # the same step on the original object, from the same masters
        model.p(k).data.copy_(trained[k])
    ts.optimizer_step(g)
    assert all(torch.equal(a, b) for k in FULL for a, b in zip(ts.state[k], ts2.state[k])) and torch.equal(ts.pstate, ts2.pstate)
    model._train_packs = False
    adam = DenoiserTrainStep(model, trainable=FULL)
    with pytest.raises(ValueError, match="prodigy"):
        adam.load_state_dict(sd)
    adam.optimizer_step(_fake_grads(adam))
    with pytest.raises(ValueError, match="adamw"):
        ts2.load_state_dict(adam.state_dict())


def test_sharded_state_round_trips_and_the_other_optimiser_is_refused(tmp_path):
    from gpt_image_edit_amd.zero import ShardedAdamW
    shapes = {"a.weight": (33, 17), "a.bias": (33,), "b.weight": (50, 7)}
    params = lambda: {n: (torch.randn(s, generator=torch.Generator().manual_seed(len(n))) * 0.05).to(BF16) for n, s in shapes.items()}  # noqa: E731
    kw = dict(kernels=S, optimizer="prodigy", weight_decay=0.01, bucket_numel=400, prodigy=dict(d0=1e-3, use_bias_correction=False,
                                                                                              safeguard_warmup=False))
    opt = ShardedAdamW(params(), **kw)
    assert opt.hp["lr"] == 1.0 and len(opt.layout.buckets) == 3
    adam = ShardedAdamW(params(), kernels=S, bucket_numel=400)
    assert adam.hp["lr"] == 1e-6 and adam.s is None and adam.pstate is None
    assert opt.state_bytes() == (adam.state_bytes()[0], opt.layout.slice_numel * 4 * 6) and adam.state_bytes()[1] == opt.layout.slice_numel * 16
    assert torch.equal(opt.p0, opt.master) and not bool(opt.s.any())
    grads = lambda i: {n: 0.1 * torch.randn(s, generator=torch.Generator().manual_seed(50 + i)) for n, s in shapes.items()}  # noqa: E731
    del S.calls[:]
    for i in range(3):
        opt.accumulate(grads(0))                                   # the same gradient again: p0 - p points along it, d grows
        opt.step()
    chunks = [b["chunk"] for b in opt.layout.buckets]
    assert S.calls[:9] == [("sumsq", 1), ("begin",)] + [("moments", c) for c in chunks] + [("update_d",)] + [("apply", c) for c in chunks]
    assert opt.prodigy_state()["k"] == 3 and opt.prodigy_state()["d"] > 1e-3
    opt.save(str(tmp_path))
    sd = opt.state_dict()
    assert sd["optimizer"] == "prodigy" and set(sd) >= {"s", "p0", "scalars", "prodigy"} and set(adam.state_dict()) == set(sd) - {
        "optimizer", "s", "p0", "scalars", "prodigy"}
    opt2 = ShardedAdamW(params(), **kw)
    opt2.load(str(tmp_path))
    assert opt2.step_count == 3 and opt2.prodigy_state() == opt.prodigy_state()
    assert all(torch.equal(opt.params[n], opt2.params[n]) for n in shapes)
    for o in (opt, opt2):
        o.accumulate(grads(7))
        o.step()
    for name in ("master", "exp_avg", "exp_avg_sq", "s", "p0", "pstate", "flat_param"):
        assert torch.equal(getattr(opt, name), getattr(opt2, name)), name
    with pytest.raises(ValueError, match="prodigy"):
        adam.load_state_dict(sd)
    with pytest.raises(ValueError, match="adamw"):
        opt2.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="layout"):
        ShardedAdamW(params(), **dict(kw, bucket_numel=None)).load_state_dict(sd)
