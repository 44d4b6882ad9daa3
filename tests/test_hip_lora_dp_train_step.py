"""GPU: ``DenoiserTrainStep(model, lora=name, data_parallel=True)`` at world 1 on the configuration of
tests/test_hip_lora_train_step.py (full width, one double + one single block, 16 x 16 latents, 64 text tokens).

One micro-batch must be the ``lora=`` step bit for bit up to the optimiser (whose flat pass is held to ``oracle.train.adamw_step``
at the tolerances of ``test_one_optimizer_step``); two micro-batches are held to the accumulate bound of tests/lora_grad_acc_ref.py
against the fp64 projections of the PARENT's ``dW`` (a plain model with ``trainable=`` the targets), and the step to the ``lora=``
step on the caller-side mean; then ``discard()``, save / resume, Prodigy against its restarted float64 reference, a frozen adapter.

Observed on an MI355X (one run): the running sums of two micro-batches at most 0.0036 of the accumulate bound (to_out.0, d_up); the
Prodigy steps at the per-tensor LoRA path's figures (m 0.495, v 0.486, s 0.865, master 0.942 of the bounds before the margin)."""
import pytest
import torch

import lora_grad_acc_ref as A
import lora_grad_ref as R
from test_hip_lora_train_step import DEFAULT_TARGETS, D0, LR, RANK, _batch, _model, _names, _random_adapter, _step

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
MODS = [p[:-len(".weight")] for p in DEFAULT_TARGETS]


def _batch2():
    """The second micro-batch: the first with other ``noise`` and ``sigmas``."""
    return dict(_batch(), noise=torch.randn(1, 16, 16, 16, generator=torch.Generator().manual_seed(9)).cuda(),
                sigmas=torch.tensor([0.5]).cuda())


def _pair(frozen=False, **kw):
    """(model, lora= step), (model, data_parallel step) on identical models with the same random adapter."""
    out = []
    for dp in (False, True):
        model = _model()
        if frozen:
            model.load_lora_adapter(_random_adapter(model, [D0 + "attn.to_q", D0 + "ff.net.0.proj"], 8, 4, seed=5), adapter_name="f",
                                    weight=0.5)
        model.load_lora_adapter(_random_adapter(model, MODS, 5, 10, seed=6), adapter_name="t")
        out.append((model, _step(model, lora="t", **(dict(data_parallel=True) if dp else {}), **kw)))
    return out


def test_one_micro_batch_is_the_lora_step_and_the_flat_optimiser_pass():
    from gpt_image_edit_amd import ops
    from oracle import train as otrain
    orig = {n: p.data.clone() for n, p in _model().named_parameters()}
    (m_ref, ts_ref), (model, ts) = _pair()
    assert ts.opt is not None and ts.opt.direct and len(ts.opt.layout.buckets) == 1
    before = {n: p.data.clone() for n, p in model.named_parameters()}
    batch = _batch()
    loss_ref, g_ref, d_ref = ts_ref.forward_backward(**batch)
    loss, grads, d_enc = ts.forward_backward(**batch)
    assert torch.equal(loss, loss_ref) and torch.equal(d_enc, d_ref) and set(grads) == set(g_ref) == ts.trainable_names()
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), g_ref[k].view(torch.int32)), k
        assert grads[k].data_ptr() == ts.opt.grad_view(k).data_ptr(), f"{k} is a copy, not the optimiser's view"
    params = {k: ts._param(k).float().cpu() for k in grads}
    want_p, _, want_norm = otrain.adamw_step(params, {k: g.cpu() for k, g in grads.items()}, {}, lr=LR)
    norm = ts.optimizer_step(grads).sqrt().item()
    assert abs(norm - want_norm.item()) <= 1e-4 * want_norm.item()
    L = ts.opt.layout
    for k in grads:
        lo, n, shape = L.offsets[k]
        master = ts.opt.master[lo:lo + n].view(shape).cpu()
        assert (master - want_p[k]).abs().max().item() <= 1e-5, k                                # the fp32 master
        new = ts._param(k).float().cpu()
        assert (new - want_p[k]).abs().max().item() <= 2.0 ** -8 * want_p[k].abs().max().item() + 1e-6, k   # its bf16 copy
        assert not torch.equal(new, params[k]), f"{k} did not move"
    s = R.f32(10 / 5)
    for n, p in model.named_parameters():
        if n not in DEFAULT_TARGETS:
            assert torch.equal(p.data, before[n]), f"{n} is not the adapter's and changed"
            continue
        e = model._lora_adapters["t"][n]
        assert torch.equal(model._lora_base[n], orig[n])
        want = ops.lora_merge(orig[n], [(e.up, e.down, s)], out=torch.empty_like(orig[n]))
        assert torch.equal(p.data, want) and not torch.equal(p.data, before[n]), n


def test_two_micro_batches_against_the_parents_dw_and_the_caller_side_mean():
    (m_ref, ts_ref), (model, ts) = _pair()
    s = R.f32(10 / 5)
    b1, b2 = _batch(), _batch2()
    plain = _model()
    plain.load_state_dict(model.state_dict())
    parent = _step(plain, trainable=DEFAULT_TARGETS)
    dws = []
    for b in (b1, b2):
        _, dw, _ = parent.forward_backward(**b)
        dws.append({k: v.clone() for k, v in dw.items()})
    l1, g1, _ = ts.forward_backward(**b1)
    first = {k: v.clone() for k, v in g1.items()}
    l2, g2, _ = ts.forward_backward(**b2)
    assert l1.item() != l2.item() and all(g2[k].data_ptr() == g1[k].data_ptr() for k in g1)
    worst = 0.0
    for p in DEFAULT_TARGETS:
        a, b = _names(p)
        e = model._lora_adapters["t"][p]
        R.check(p + " pass 1", first[b], first[a], dws[0][p], e.up, e.down, s)
        worst = max(worst, *A.check(p + " pass 2", g2[b], g2[a], first[b], first[a], dws[1][p], e.up, e.down, s))
    print(f"[parity] lora_dp running sums: worst observed/bound {worst:.4f}", flush=True)
    # the lora= step stepped on the caller-side mean of its own two passes
    _, r1, _ = ts_ref.forward_backward(**b1)
    r1 = {k: v.clone() for k, v in r1.items()}
    _, r2, _ = ts_ref.forward_backward(**b2)
    ts.optimizer_step(g2)
    ts_ref.optimizer_step({k: ((r1[k] + r2[k]) / 2).contiguous() for k in r2})
    for n, p in model.named_parameters():      # the tolerance of test_sharded_gradient_accumulation_and_modified_gradient_error
        a, b = p.data.float(), m_ref.p(n).data.float()
        assert (a - b).abs().max().item() <= 2.0 ** -8 * b.abs().max().item() + 1e-6, n
    for k in g2:
        a, b = ts._param(k).float(), ts_ref._param(k).float()
        assert (a - b).abs().max().item() <= 2.0 ** -8 * b.abs().max().item() + 1e-6, k


def test_two_passes_over_one_batch_double_the_gradient_and_discard_starts_over():
    (_, _), (model, ts) = _pair()
    batch = _batch()
    _, g, _ = ts.forward_backward(**batch)
    once = {k: v.clone() for k, v in g.items()}
    _, g, _ = ts.forward_backward(**batch)
    for k in g:                                   # x + x = 2 x is exact in fp32 (fused or not)
        assert torch.equal(g[k], 2 * once[k]), k
    ts.discard()
    _, g, _ = ts.forward_backward(**_batch2())
    fresh = _pair()[1][1]
    _, want, _ = fresh.forward_backward(**_batch2())
    for k in g:
        assert torch.equal(g[k].view(torch.int32), want[k].view(torch.int32)), k
    assert ts.opt._micro == 0


def _run(steps, resume_from=None, collect=None):
    model = _model()
    model.add_lora_adapter("t", rank=RANK, seed=3)
    ts = _step(model, lora="t", data_parallel=True)
    if resume_from is not None:
        ts.load_state_dict(resume_from)
    b1, b2 = _batch(seed=1), _batch2()
    out = []
    for i in range(steps):
        if collect is not None and i == collect:
            out.append(ts.state_dict())
        ts.forward_backward(**b2)                  # two micro-batches per step
        r = ts.step(**b1)
        out.append((r["loss"].clone(), {k: g.clone() for k, g in r["grads"].items()}))
    return model, ts, out


def test_three_steps_save_resume_and_the_saved_adapter(tmp_path):
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    from gpt_image_edit_amd.vae import HipAutoencoderKL
    model, ts, out = _run(4, collect=3)
    sd = out.pop(3)
    assert sd["kind"] == "lora_dp" and sd["opt"]["step"] == 3 and ts.step_count == 4
    model_c, ts_c, out_c = _run(1, resume_from=sd)
    assert ts_c.step_count == 4
    assert torch.equal(out_c[0][0], out[3][0]) and all(torch.equal(out_c[0][1][k], out[3][1][k]) for k in out[3][1])
    assert all(torch.equal(p.data, model.p(n).data) for n, p in model_c.named_parameters())
    assert torch.equal(ts_c.opt.flat_param, ts.opt.flat_param) and torch.equal(ts_c.opt.master, ts.opt.master)
    assert any(bool(e.up.any()) for e in model._lora_adapters["t"].values())
    with pytest.raises(ValueError, match="lora_dp"):
        plain = _model()
        plain.add_lora_adapter("t", rank=RANK, seed=3)
        _step(plain, lora="t").load_state_dict(sd)
    # the factors are views of the flat buffer: the saved file holds the trained values
    vae = HipAutoencoderKL(device="cuda", init="synthetic", seed=22)
    path = FluxKontextPipeline(model, vae, use_graph=False).save_lora_weights(str(tmp_path / "adapter.safetensors"), adapter_name="t")
    fresh = _model()
    assert FluxKontextPipeline(fresh, vae, use_graph=False).load_lora_weights(path, adapter_name="t") == []
    assert all(torch.equal(p.data, fresh.p(n).data) for n, p in model.named_parameters())
    assert any(not torch.equal(fresh.p(n).data, fresh._lora_base[n]) for n in DEFAULT_TARGETS)


def test_prodigy_steps_against_the_restarted_reference_and_the_frozen_adapter_stays():
    from test_hip_prodigy_train_step import _Sharded, _checked_step
    from test_hip_prodigy_train_step import _step as _pstep
    model = _model()
    model.load_lora_adapter(_random_adapter(model, [D0 + "attn.to_q", D0 + "ff.net.0.proj"], 8, 4, seed=5), adapter_name="f", weight=0.5)
    frozen = {p: (e.up.clone(), e.down.clone()) for p, e in model._lora_adapters["f"].items()}
    merged_f = model.p(D0 + "ff.net.0.proj.weight").data.clone()
    assert model.add_lora_adapter("t", rank=RANK, seed=3) == DEFAULT_TARGETS
    ts = _pstep(model, lora="t", data_parallel=True)
    assert ts.opt.optimizer == "prodigy" and ts.opt.direct
    acc, batch, ratios = _Sharded(ts), _batch(seed=1), {}
    for i in range(3):
        _checked_step(acc, batch, f"lora dp {i}", ratios)
    print("[prodigy step] lora dp, worst ratios:", ratios, flush=True)
    for p, (up, down) in frozen.items():
        e = model._lora_adapters["f"][p]
        assert torch.equal(e.up, up) and torch.equal(e.down, down), f"the frozen adapter's {p} changed"
    assert torch.equal(model.p(D0 + "ff.net.0.proj.weight").data, merged_f) and not torch.equal(merged_f, model._lora_base[D0 + "ff.net.0.proj.weight"])
    assert any(bool(e.up.any()) for e in model._lora_adapters["t"].values())
    assert ts.prodigy_state()["k"] == 3
