"""GPU: ``DenoiserTrainStep(model, lora=..., lora_backward="factored")`` on the configuration of tests/test_hip_lora_train_step.py
(full width, one double + one single block, 16 x 16 latents, 64 text tokens), B = 1 (block-level backward entry points) and B = 2
(per-launch route).

The gradient reference is fp64 on the operands the side sink RECEIVED (cloned through a wrapping callback): every factor's
gradient within the bound derived in tests/lora_side_ref.py; against the projected step (the parent's code) within both paths'
bounds plus 2^-9 |s| sum |dW| |factor|, the bf16 rounding of dW that only the projected path has."""
import pytest
import torch

import lora_grad_ref as P
import lora_side_ref as S
from test_hip_lora_train_step import D0, S0, LR, RANK, _batch, _model, _names, _random_adapter, _step

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
QKV = ("to_q", "to_k", "to_v")
# every side leaf of both block kinds and both streams (backward.FluxBackward.SIDE_LEAVES)
TARGETS = sorted([D0 + f"attn.{n}.weight" for n in QKV + ("add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out")]
                 + [D0 + "ff.net.0.proj.weight", D0 + "ff_context.net.0.proj.weight"]
                 + [S0 + f"attn.{n}.weight" for n in QKV] + [S0 + "proj_mlp.weight"])
MODS = [p[:-len(".weight")] for p in TARGETS]
SCALE = S.f32(0.75 * 10 / 5)


def _loaded(mods=MODS, frozen=False):
    model = _model()
    if frozen:
        model.load_lora_adapter(_random_adapter(model, [D0 + "attn.to_q", D0 + "ff.net.0.proj"], 8, 4, seed=5), adapter_name="f", weight=0.5)
    model.load_lora_adapter(_random_adapter(model, mods, 5, 10, seed=6), adapter_name="t", weight=0.75)
    return model


def _factored(model, **kw):
    """(step, operands): the factored step with its side sink wrapped so that ``operands[pname]`` holds clones of the last
    (dy, x) the sink received for that target."""
    ts = _step(model, lora="t", lora_backward="factored", **kw)
    operands = {}
    make = ts._lora_side_sink

    def wrapped(out):
        inner = make(out)

        def side_sink(pname, dy, x):
            assert pname not in operands or operands[pname] is None, f"two side calls for {pname} in one pass"
            operands[pname] = (dy.clone(), x.clone())
            inner(pname, dy, x)
        return side_sink
    ts._lora_side_sink = wrapped
    return ts, operands


def _projected(model, **kw):
    """(step, dws): the projected step with its sink wrapped so that ``dws[pname]`` holds a clone of the dW bits it projected."""
    ts = _step(model, lora="t", **kw)
    dws = {}
    make = ts._lora_sink

    def wrapped(out):
        inner = make(out)

        def sink(block_grads):
            dws.update({k: v.clone() for k, v in block_grads.items()})
            inner(block_grads)
        return sink
    ts._lora_sink = wrapped
    return ts, dws


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_a_fresh_adapters_first_pass_has_the_projected_loss_bits():
    a, b = _model(), _model()
    mods = ["to_q", "to_out.0", "proj_mlp"]
    assert a.add_lora_adapter("t", rank=RANK, target_modules=mods) == b.add_lora_adapter("t", rank=RANK, target_modules=mods)
    batch = _batch()
    loss_p, grads_p, d_p = _step(a, lora="t").forward_backward(**batch)
    ts = _step(b, lora="t", lora_backward="factored")
    assert ts.bw.side == set(b._lora_adapters["t"]) and not ts.bw.trainable
    loss, grads, d_enc = ts.forward_backward(**batch)
    assert torch.equal(loss, loss_p) and torch.equal(d_enc, d_p) and set(grads) == set(grads_p) == ts.trainable_names()
    for p in b._lora_adapters["t"]:
        dn, up = _names(p)
        assert not bool(grads[dn].any()), f"{dn}: up is zero, so d_down must be exactly zero"
        assert bool(grads[up].any()) and bool(torch.isfinite(grads[up]).all()), up


@pytest.mark.parametrize("B,frozen", [(1, True), (2, False)])
def test_gradients_against_fp64_on_the_received_operands_and_against_the_projected_step(B, frozen, monkeypatch):
    from gpt_image_edit_amd.backward import FluxBackward
    routes = []
    for name in ("_double_backward_c", "_double_backward", "_single_backward_c", "_single_backward"):
        real = getattr(FluxBackward, name)
        monkeypatch.setattr(FluxBackward, name, lambda self, *a, _n=name, _r=real, **k: (routes.append(_n), _r(self, *a, **k))[1])
    batch = _batch(B)
    model = _loaded(frozen=frozen)
    ts, ops_ = _factored(model)
    assert ts.bw.side == set(TARGETS) and not ts.bw.trainable
    loss, grads, d_enc = ts.forward_backward(**batch)
    assert routes == (["_single_backward_c", "_double_backward_c"] if B == 1 else ["_single_backward", "_double_backward"])
    first = {k: v.clone() for k, v in grads.items()}
    got = dict(ops_)
    ops_.clear()
    loss2, grads2, d_enc2 = ts.forward_backward(**batch)
    assert torch.equal(loss, loss2) and torch.equal(d_enc, d_enc2) and all(_same_bits(first[k], grads2[k]) for k in first), \
        "the factored backward is not deterministic"
    tp, dws = _projected(_loaded(frozen=frozen))
    loss_p, grads_p, d_enc_p = tp.forward_backward(**batch)
    assert torch.equal(loss, loss_p) and torch.equal(d_enc, d_enc_p) and set(grads) == set(grads_p) and set(got) == set(TARGETS)
    worst = 0.0
    for p in TARGETS:
        dn, up = _names(p)
        e = model._lora_adapters["t"][p]
        dy, x = got[p]
        assert dy.shape[0] == B and dy.shape[-1] == e.up.shape[0] and x.shape[-1] == e.down.shape[1]
        S.check(p, first[up], first[dn], x, dy, e.up, e.down, SCALE)
        # the projected step: within ITS bound of the projection of its own dW bits; those bits are the bf16 rounding of dy^T x
        P.check(p, grads_p[up], grads_p[dn], dws[p], e.up, e.down, SCALE)
        (_, bfu), (_, bfd) = S.bounds(x, dy, e.up, e.down, SCALE)
        (_, bpu), (_, bpd) = P.bounds(dws[p], e.up, e.down, SCALE)
        dw = (S.rows64(dy).T @ S.rows64(x)).abs()
        tol_u = bfu + bpu + 2.0 ** -9 * abs(SCALE) * (dw @ e.down.double().abs().T)
        tol_d = bfd + bpd + 2.0 ** -9 * abs(SCALE) * (e.up.double().abs().T @ dw)
        ru = S.worst_ratio(first[up], grads_p[up].double(), tol_u)
        rd = S.worst_ratio(first[dn], grads_p[dn].double(), tol_d)
        print(f"[parity] factored vs projected {p}: observed/tolerance d_up={ru:.3g} d_down={rd:.3g}", flush=True)
        assert ru <= 1.0 and rd <= 1.0, (p, ru, rd)
        worst = max(worst, ru, rd)
    print(f"[parity] factored vs projected, B={B}: worst observed/tolerance {worst:.3g}", flush=True)


def test_block_entry_route_and_per_launch_route_give_equal_bits(monkeypatch):
    from gpt_image_edit_amd import backward
    batch = _batch()
    out = []
    for api in (1, 0):
        monkeypatch.setattr(backward, "BLOCK_API", api)
        ts, got = _factored(_loaded())
        loss, grads, d_enc = ts.forward_backward(**batch)
        out.append((loss, {k: v.clone() for k, v in grads.items()}, d_enc, dict(got)))
    (l1, g1, d1, o1), (l0, g0, d0, o0) = out
    assert torch.equal(l1, l0) and torch.equal(d1, d0) and set(g1) == set(g0)
    for p in TARGETS:                              # the same operand bits reach the kernel on both routes ...
        assert torch.equal(o1[p][0], o0[p][0]) and torch.equal(o1[p][1], o0[p][1]), p
    for k in g1:                                   # ... hence the same gradient bits
        assert _same_bits(g1[k], g0[k]), k


def test_one_optimizer_step_against_fp32_adamw():
    from gpt_image_edit_amd import ops
    from oracle import train as otrain
    orig = {n: p.data.clone() for n, p in _model().named_parameters()}
    model = _model()
    model.load_lora_adapter(_random_adapter(model, MODS, 5, 10, seed=6), adapter_name="t")
    s = S.f32(10 / 5)
    before = {n: p.data.clone() for n, p in model.named_parameters()}
    ts = _step(model, lora="t", lora_backward="factored")
    batch = _batch()
    loss, grads, _ = ts.forward_backward(**batch)
    params = {k: ts._param(k).float().cpu() for k in grads}
    want_p, _, want_norm = otrain.adamw_step(params, {k: g.cpu() for k, g in grads.items()}, {}, lr=LR)
    norm = ts.optimizer_step(grads).sqrt().item()
    assert abs(norm - want_norm.item()) <= 1e-4 * want_norm.item()
    for k in grads:
        assert (ts.state[k][0].cpu() - want_p[k]).abs().max().item() <= 1e-5, k                 # the fp32 master
        new = ts._param(k).float().cpu()
        assert (new - want_p[k]).abs().max().item() <= 2.0 ** -8 * want_p[k].abs().max().item() + 1e-6, k   # its bf16 copy
        assert not torch.equal(new, params[k]), f"{k} did not move"
    for n, p in model.named_parameters():
        if n not in TARGETS:
            assert torch.equal(p.data, before[n]), f"{n} is not the adapter's and changed"
            continue
        e = model._lora_adapters["t"][n]
        want = ops.lora_merge(orig[n], [(e.up, e.down, s)], out=torch.empty_like(orig[n]))
        assert torch.equal(p.data, want) and not torch.equal(p.data, before[n]), n
    loss3, _, _ = ts.forward_backward(**batch)              # packs and transposes follow the re-merged side targets too
    fresh = _model()
    fresh.load_state_dict(model.state_dict())
    loss4, _, _ = _step(fresh, trainable=TARGETS).forward_backward(**batch)
    assert torch.equal(loss3, loss4) and loss3.item() != loss.item(), "the step after the update does not see the re-merged weights"


def _run(steps, resume_from=None, collect=None, mode="factored"):
    model = _model()
    model.add_lora_adapter("t", rank=RANK, seed=3)
    ts = _step(model, lora="t", lora_backward=mode)
    if resume_from is not None:
        ts.load_state_dict(resume_from)
    batch = _batch(seed=1)
    out = []
    for i in range(steps):
        if collect is not None and i == collect:
            out.append(ts.state_dict())
        r = ts.step(**batch)
        out.append((r["loss"].clone(), {k: g.clone() for k, g in r["grads"].items()}))
    return model, ts, out


def test_ten_steps_lower_the_loss_and_resume_is_bit_identical():
    model, ts, out = _run(10, collect=2)
    sd = out.pop(2)
    losses = [l.item() for l, _ in out]
    print("[lora train, factored] losses:", " ".join(f"{x:.6f}" for x in losses), flush=True)
    assert losses[-1] < losses[0], losses
    assert sd["kind"] == "lora" and sd["step"] == 2 and set(sd["state"]) == ts.trainable_names()
    model_c, ts_c, out_c = _run(1, resume_from=sd)
    assert ts_c.step_count == 3
    assert torch.equal(out_c[0][0], out[2][0]) and all(_same_bits(out_c[0][1][k], out[2][1][k]) for k in out[2][1])
    model_d, _, _ = _run(3)
    assert all(torch.equal(p.data, model_d.p(n).data) for n, p in model_c.named_parameters())
    # the optimiser state does not record the mode: the projected step loads it and continues from the same factors
    model_e, ts_e, out_e = _run(1, resume_from=sd, mode="projected")
    assert ts_e.step_count == 3 and torch.equal(out_e[0][0], out[2][0])


def test_data_parallel_two_micro_batches():
    from test_hip_lora_dp_train_step import _batch2
    b1, b2 = _batch(), _batch2()
    model = _loaded()
    ts, got = _factored(model, data_parallel=True)
    assert ts.opt is not None and ts.opt.direct
    l1, g1, _ = ts.forward_backward(**b1)
    first = {k: v.clone() for k, v in g1.items()}
    ops1 = dict(got)
    got.clear()
    l2, g2, _ = ts.forward_backward(**b2)
    assert l1.item() != l2.item() and all(g2[k].data_ptr() == g1[k].data_ptr() == ts.opt.grad_view(k).data_ptr() for k in g1)
    for p in TARGETS:
        dn, up = _names(p)
        e = model._lora_adapters["t"][p]
        S.check(p + " pass 1", first[up], first[dn], ops1[p][1], ops1[p][0], e.up, e.down, SCALE)
        S.check(p + " pass 2", g2[up], g2[dn], got[p][1], got[p][0], e.up, e.down, SCALE, old=(first[up], first[dn]))
    # the step on the running sums against the non-accumulating factored step on the caller-side mean of its two passes
    m_ref = _loaded()
    ts_ref = _step(m_ref, lora="t", lora_backward="factored")
    _, r1, _ = ts_ref.forward_backward(**b1)
    r1 = {k: v.clone() for k, v in r1.items()}
    _, r2, _ = ts_ref.forward_backward(**b2)
    for k in r1:                                   # one micro-batch: the same bits in either optimiser's buffers
        assert _same_bits(r1[k], first[k]), k
    ts.optimizer_step(g2)
    ts_ref.optimizer_step({k: ((r1[k] + r2[k]) / 2).contiguous() for k in r2})
    for n, p in model.named_parameters():
        a, b = p.data.float(), m_ref.p(n).data.float()
        assert (a - b).abs().max().item() <= 2.0 ** -8 * b.abs().max().item() + 1e-6, n
    # discard() starts over: the pass after it overwrites (were b1 still in the sums, the two results would differ)
    got.clear()
    ts.forward_backward(**b1)
    ts.discard()
    got.clear()
    _, g, _ = ts.forward_backward(**b2)
    after_b1 = {k: v.clone() for k, v in g.items()}
    ts.discard()
    got.clear()
    _, g, _ = ts.forward_backward(**b2)
    assert all(_same_bits(g[k], after_b1[k]) for k in g) and ts.step_count == 1


def test_one_prodigy_step():
    from test_hip_prodigy_train_step import _PerTensor, _checked_step
    from test_hip_prodigy_train_step import _step as _pstep
    model = _model()
    model.add_lora_adapter("t", rank=RANK, seed=3)
    ts = _pstep(model, lora="t", lora_backward="factored")
    assert ts.optimizer == "prodigy" and ts.bw.side == set(model._lora_adapters["t"])
    ratios = {}
    _checked_step(_PerTensor(ts), _batch(seed=1), "lora factored", ratios)
    print("[prodigy step] lora factored, worst ratios:", ratios, flush=True)
    assert ts.prodigy_state()["k"] == 1 and any(bool(e.up.any()) for e in model._lora_adapters["t"].values())


def test_an_adapter_on_ff_net_2_trains_through_the_mixed_path():
    """ff.net.2's operands do not survive the block: it stays in the wgrad set and is projected from dW -- with the bits of the
    projected step -- while the other targets of the same adapter go through the side sink."""
    mods = [D0 + "ff.net.2", D0 + "attn.to_out.0", S0 + "proj_mlp", S0 + "proj_out"]
    batch = _batch()
    model = _loaded(mods)
    ts, got = _factored(model)
    side = {D0 + "attn.to_out.0.weight", S0 + "proj_mlp.weight"}
    assert ts.bw.side == side and ts.bw.trainable == {D0 + "ff.net.2.weight", S0 + "proj_out.weight"}
    loss, grads, _ = ts.forward_backward(**batch)
    tp, dws = _projected(_loaded(mods))
    loss_p, grads_p, _ = tp.forward_backward(**batch)
    assert torch.equal(loss, loss_p) and set(grads) == set(grads_p) == ts.trainable_names() and set(got) == side
    for p in (D0 + "ff.net.2.weight", S0 + "proj_out.weight"):
        for k in _names(p):
            assert _same_bits(grads[k], grads_p[k]) and bool(grads[k].any()), k
    for p in side:
        dn, up = _names(p)
        e = model._lora_adapters["t"][p]
        S.check(p, grads[up], grads[dn], got[p][1], got[p][0], e.up, e.down, SCALE)
    before = {p: model.p(p).data.clone() for p in model._lora_adapters["t"]}
    ts.optimizer_step(grads)
    assert all(not torch.equal(model.p(p).data, before[p]) for p in before), "a target was not re-merged after the step"
