"""CPU tests of ``DenoiserTrainStep(model, lora=name, data_parallel=True)`` with the ops stubbed as in
tests/test_lora_train_host.py plus a torch stand-in for ``ops.lora_grad`` that honours ``accumulate``: names and layout order, the
factors as views of the flat buffer, the refusals, two passes through the sink summed and the step on their mean, ``discard()``,
one merge per touched weight, the ``kind="lora_dp"`` round trip, every cross-mode load refused, a tensor written twice."""
import pytest
import torch

BF16 = torch.bfloat16
D0, S0, S1 = "transformer_blocks.0.", "single_transformer_blocks.0.", "single_transformer_blocks.1."
QKV = ("to_q", "to_k", "to_v")
DEFAULT = sorted([D0 + f"attn.{n}.weight" for n in QKV + ("to_out.0",)] + [s + f"attn.{n}.weight" for s in (S0, S1) for n in QKV])
A, B = "lora_A.weight", "lora_B.weight"
LR = 0.5


@pytest.fixture()
def model(monkeypatch):
    """The one-head (D = 128) CPU model of tests/test_lora_train_host.py.  The AdamW stand-in is plain SGD on
    ``grad_scale * grad`` (no clipping), so a step shows which mean it was given."""
    from gpt_image_edit_amd import flux_spec, ops
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2, num_attention_heads=1)
    m = HipFluxTransformer2DModel(cfg, device="cpu", init="empty")
    g = torch.Generator().manual_seed(3)
    for p in m.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g) * 0.05)
    merges, calls = [], []

    def merge(base, terms, out=None):
        out = base if out is None else out
        merges.append(tuple(base.shape))
        v = base.float()
        for up, down, s in terms:
            v = v + float(s) * (up.float() @ down.float())
        out.copy_(v.to(BF16))
        return out

    def sumsq(tensors, out=None):
        tensors = [tensors] if torch.is_tensor(tensors) else tensors
        return torch.stack([t.double().pow(2).sum() for t in tensors]).sum().reshape(1)

    def adamw_step(master, grad, exp_avg, exp_avg_sq, step, lr, betas=None, eps=None, weight_decay=None, grad_sumsq=None,
                   max_grad_norm=None, param_bf16=None, grad_scale=1.0):
        exp_avg.add_(grad.float())
        exp_avg_sq.add_(grad.float() ** 2)
        master.sub_(lr * grad_scale * grad.float())
        param_bf16.copy_(master)

    def lora_grad(dw, up, down, scale, d_up=None, d_down=None, ws=None, accumulate=False):
        calls.append(bool(accumulate))
        pu, pd = float(scale) * (dw.float() @ down.float().T), float(scale) * (up.float().T @ dw.float())
        if accumulate:
            d_up.add_(pu), d_down.add_(pd)
        else:
            d_up.copy_(pu), d_down.copy_(pd)
        return d_up, d_down

    monkeypatch.setattr(ops, "lora_merge", merge)
    monkeypatch.setattr(ops, "sumsq", sumsq)
    monkeypatch.setattr(ops, "adamw_step", adamw_step)
    monkeypatch.setattr(ops, "lora_grad", lora_grad)
    monkeypatch.setattr(ops, "lora_grad_ws", lambda N, K, r, dev: torch.empty(0))
    m.merges, m.grad_calls = merges, calls
    return m


def _step(model, **kw):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    return DenoiserTrainStep(model, lora="t", lr=LR, data_parallel=True, **kw)


def _dws(model, seed):
    g = torch.Generator().manual_seed(seed)
    return {p: (0.1 * torch.randn(model.p(p).shape, generator=g)).to(BF16) for p in DEFAULT}


def _proj(model, dws):
    """name -> the fp32 projection of ``dws`` onto the adapter's current factors, as the stand-in computes it."""
    out = {}
    for p, dw in dws.items():
        e = model._lora_adapters["t"][p]
        stem = p[:-len("weight")]
        out[stem + B], out[stem + A] = dw.float() @ e.down.float().T, e.up.float().T @ dw.float()
    return out


def _one_pass(ts, dws):
    out = {}
    ts.opt.begin_micro_batch()
    ts._lora_sink(out)(dws)
    return out


def _randomise_up(model, seed=4):
    g = torch.Generator().manual_seed(seed)
    for e in model._lora_adapters["t"].values():
        e.up.copy_(0.1 * torch.randn(e.up.shape, generator=g))


def test_names_layout_order_and_views(model):
    from gpt_image_edit_amd.zero import backward_order
    model.add_lora_adapter("t", rank=4)
    _randomise_up(model)
    before = {p: (e.up.clone(), e.down.clone()) for p, e in model._lora_adapters["t"].items()}
    ts = _step(model)
    names = {p[:-len("weight")] + s for p in DEFAULT for s in (A, B)}
    assert ts.trainable_names() == names and ts.opt is not None and ts.opt.world == 1
    assert ts.opt.layout.names == backward_order(sorted(names))
    assert ts.opt.layout.names[0].startswith(S1) and ts.opt.layout.names[-1].startswith(D0)      # the last block's come first
    flat = ts.opt.flat_param
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 2
    for p, e in model._lora_adapters["t"].items():
        stem = p[:-len("weight")]
        assert e.up is ts.opt.params[stem + B] and e.down is ts.opt.params[stem + A]
        assert ts._param(stem + B) is e.up and ts._param(stem + A) is e.down
        assert lo <= e.up.data_ptr() < hi and lo <= e.down.data_ptr() < hi and e.up.dtype == BF16
        assert torch.equal(e.up, before[p][0]) and torch.equal(e.down, before[p][1])
    # lora_state_dict reads the flat buffer: a write there shows with no copy in between
    flat.fill_(0.25)
    sd = model.lora_state_dict("t")
    assert all(bool((v == 0.25).all()) for k, v in sd.items() if not k.endswith("alpha"))


def test_refusals(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    model.add_lora_adapter("t", rank=4)
    with pytest.raises(ValueError, match="sharded=True"):
        DenoiserTrainStep(model, data_parallel=True)
    with pytest.raises(ValueError, match="not built") as e:
        DenoiserTrainStep(model, lora="t", sharded=True)
    assert "data_parallel=True" in str(e.value)
    with pytest.raises(ValueError, match="not built"):
        DenoiserTrainStep(model, lora="t", sharded=True, data_parallel=True)
    assert not model._train_packs


def test_two_passes_sum_and_the_step_uses_the_mean(model):
    model.add_lora_adapter("t", rank=4)
    _randomise_up(model)
    ts = _step(model)
    dw1, dw2 = _dws(model, 1), _dws(model, 2)
    p1, p2 = _proj(model, dw1), _proj(model, dw2)
    g1 = _one_pass(ts, dw1)
    assert set(g1) == ts.trainable_names() and model.grad_calls == [False] * len(DEFAULT)
    assert all(torch.equal(g1[k], p1[k]) for k in g1)
    g2 = _one_pass(ts, dw2)
    assert model.grad_calls[len(DEFAULT):] == [True] * len(DEFAULT)
    for k in g2:
        assert g2[k].data_ptr() == g1[k].data_ptr() == ts.opt.grad_view(k).data_ptr()       # the live running sums, no copy
        assert torch.equal(g2[k], p1[k] + p2[k])
    masters = {k: ts._param(k).float().clone() for k in g2}
    del model.merges[:]
    ts.optimizer_step(g2)
    assert ts.step_count == 1
    for k in masters:
        want = masters[k] - LR * 0.5 * (p1[k] + p2[k])
        torch.testing.assert_close(ts._param(k).float(), want.to(BF16).float(), rtol=0, atol=0)
    # one merge per touched weight, from the saved base with the new factors
    assert sorted(model.merges) == sorted(tuple(model.p(p).shape) for p in DEFAULT)
    q = D0 + "attn.to_q.weight"
    e = model._lora_adapters["t"][q]
    assert torch.equal(model.p(q).data, (model._lora_base[q].float() + e.up.float() @ e.down.float()).to(BF16))
    # the next step starts over: its first pass overwrites
    del model.grad_calls[:]
    g3 = _one_pass(ts, dw1)
    assert model.grad_calls == [False] * len(DEFAULT)
    p3 = _proj(model, dw1)
    assert all(torch.equal(g3[k], p3[k]) for k in g3)


def test_discard_makes_the_next_pass_overwrite(model):
    model.add_lora_adapter("t", rank=4)
    _randomise_up(model)
    ts = _step(model)
    _one_pass(ts, _dws(model, 1))
    ts.discard()
    assert not bool(ts.opt.grad_slice.any())
    del model.grad_calls[:]
    dw2 = _dws(model, 2)
    g = _one_pass(ts, dw2)
    assert model.grad_calls == [False] * len(DEFAULT)
    p2 = _proj(model, dw2)
    assert all(torch.equal(g[k], p2[k]) for k in g)
    before = {k: ts._param(k).float().clone() for k in g}
    ts.optimizer_step(g)
    for k in before:                                                        # one micro-batch: the mean is the pass itself
        assert torch.equal(ts._param(k).float(), (before[k] - LR * p2[k]).to(BF16).float())


def test_a_tensor_written_twice_in_one_pass_raises(model):
    model.add_lora_adapter("t", rank=4)
    ts = _step(model)
    dws = _dws(model, 1)
    ts.opt.begin_micro_batch()
    sink = ts._lora_sink({})
    first = {p: dws[p] for p in DEFAULT[:3]}
    sink(first)
    with pytest.raises(RuntimeError, match="twice"):
        sink({DEFAULT[0]: dws[DEFAULT[0]]})
    sink({p: dws[p] for p in DEFAULT[3:]})
    with pytest.raises(RuntimeError, match="begin_micro_batch"):             # the pass is complete: its bucket has been reduced
        sink(first)
    # the intake itself, on a staged optimiser: zeroed staging, overwrite on every pass
    from gpt_image_edit_amd.zero import ShardedAdamW
    opt = ShardedAdamW({"a": torch.zeros(3, 5, dtype=BF16), "b": torch.zeros(7, dtype=BF16)}, lr=LR, stage_always=True)
    for micro in range(2):
        opt.begin_micro_batch()
        va, acc = opt.grad_target("a")
        assert acc is False and va.shape == (3, 5) and va.dtype == torch.float32 and not bool(va.any())
        va.fill_(micro + 1.0)
        opt.written(["a"])
        with pytest.raises(RuntimeError, match="twice"):
            opt.grad_target("a")
        with pytest.raises(RuntimeError, match="twice"):
            opt.written(["a"])
        vb, _ = opt.grad_target("b")
        vb.fill_(10.0 * (micro + 1))
        opt.written(["b"])
    opt._flush()
    assert torch.equal(opt.grad_slice[:22], torch.cat([torch.full((15,), 3.0), torch.full((7,), 30.0)]))
    direct = ShardedAdamW({"a": torch.zeros(3, 5, dtype=BF16)}, lr=LR)
    assert direct.grad_target("a")[1] is False
    direct.written(["a"])
    direct.begin_micro_batch()
    assert direct.grad_target("a")[1] is True


def test_state_round_trip_and_cross_mode_refusals(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    model.add_lora_adapter("t", rank=4, seed=2)
    base = {n: p.data.clone() for n, p in model.named_parameters()}
    ts = _step(model)
    for seed in (1, 2):
        ts.optimizer_step(_one_pass(ts, _dws(model, seed)))
    sd = ts.state_dict()
    assert sd["kind"] == "lora_dp" and sd["opt"]["step"] == 2 and sd["opt"]["signature"]["names"] == ts.opt.layout.names
    trained = {n: p.data.clone() for n, p in model.named_parameters()}
    factors = {k: ts._param(k).clone() for k in ts.trainable_names()}
    for n, p in model.named_parameters():
        p.data.copy_(base[n])
    model._lora_init()
    model._train_packs = False
    model.add_lora_adapter("t", rank=4, seed=9)
    ts2 = _step(model)
    del model.merges[:]
    ts2.load_state_dict(sd)
    assert ts2.step_count == 2 and len(model.merges) == len(DEFAULT)
    assert all(torch.equal(p.data, trained[n]) for n, p in model.named_parameters())
    assert all(torch.equal(ts2._param(k), factors[k]) for k in factors)
    for name in ("master", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(ts2.opt, name), getattr(ts.opt, name))
    # every cross-mode load is refused, and the message names both settings
    kinds = dict(per_tensor=dict(kind="per_tensor", step=0, state={}), lora=dict(kind="lora", step=0, state={}),
                 sharded=dict(kind="sharded", opt={}), lora_dp=sd)
    for kind, other in kinds.items():
        if kind != "lora_dp":
            with pytest.raises(ValueError) as e:
                ts2.load_state_dict(other)
            assert f"'{kind}'" in str(e.value) and "'lora_dp'" in str(e.value)
    model._lora_init()
    model._train_packs = False
    model.add_lora_adapter("t", rank=4, seed=9)
    plain = DenoiserTrainStep(model, lora="t", lr=LR)
    for kind in ("per_tensor", "sharded", "lora_dp"):
        with pytest.raises(ValueError) as e:
            plain.load_state_dict(kinds[kind])
        assert f"'{kind}'" in str(e.value) and "'lora'" in str(e.value)
    model.unload_lora()
    model._train_packs = False
    full = DenoiserTrainStep(model, lr=LR, trainable=[DEFAULT[0]])
    for kind in ("lora", "sharded", "lora_dp"):
        with pytest.raises(ValueError) as e:
            full.load_state_dict(kinds[kind])
        assert f"'{kind}'" in str(e.value) and "'per_tensor'" in str(e.value)
    shard = DenoiserTrainStep(model, lr=LR, trainable=[DEFAULT[0]], sharded=True)
    for kind in ("per_tensor", "lora", "lora_dp"):
        with pytest.raises(ValueError) as e:
            shard.load_state_dict(kinds[kind])
        assert f"'{kind}'" in str(e.value) and "'sharded'" in str(e.value)
