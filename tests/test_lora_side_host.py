"""CPU tests of the factored LoRA backward's host layer (``FluxBackward(side=)``, ``DenoiserTrainStep(lora_backward=)``) with the
ops stubbed, as tests/test_lora_train_host.py does: keyword validation, the wgrad set without exactly the side targets, one side
call per target per pass with the right operand views (per-launch route, every kernel a shape-only stand-in), the
``grad_target`` / ``written`` protocol, and the default mode's unchanged calls."""
import types

import pytest
import torch

BF16 = torch.bfloat16
D0, S0, S1 = "transformer_blocks.0.", "single_transformer_blocks.0.", "single_transformer_blocks.1."
QKV = ("to_q", "to_k", "to_v")
DEFAULT = sorted([D0 + f"attn.{n}.weight" for n in QKV + ("to_out.0",)] + [s + f"attn.{n}.weight" for s in (S0, S1) for n in QKV])
# every kind of target: side-routable ones of both block kinds and both streams, and three that stay projected
MIXED = ["to_q", "add_k_proj", "to_out.0", "to_add_out", "ff.net.0.proj", "ff_context.net.0.proj", "proj_mlp", "ff.net.2",
         S1 + "proj_out.weight", D0 + "norm1.linear.weight"]
PROJECTED = {D0 + "ff.net.2.weight", S1 + "proj_out.weight", D0 + "norm1.linear.weight"}
A, B = "lora_A.weight", "lora_B.weight"
S_TXT, S_IMG, D = 8, 24, 128


@pytest.fixture()
def model(monkeypatch):
    """The one-head (D = 128) CPU model of tests/test_lora_train_host.py.  EVERY function of ``ops`` that would reach the library is
    a stand-in that only produces a tensor of the right shape (``out=`` when given), records its name, and for the two LoRA
    gradient calls what it was handed."""
    from gpt_image_edit_amd import flux_spec, ops
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2, num_attention_heads=1)
    m = HipFluxTransformer2DModel(cfg, device="cpu", init="empty")
    g = torch.Generator().manual_seed(3)
    for p in m.parameters():
        p.data.copy_(torch.randn(p.shape, generator=g) * 0.05)
    log = types.SimpleNamespace(calls=[], side=[], proj=[])

    def merge(base, terms, out=None):
        out = base if out is None else out
        v = base.float()
        for up, down, s in terms:
            v = v + float(s) * (up.float() @ down.float())
        out.copy_(v.to(BF16))
        return out

    def gemm(a, w=None, bias=None, out=None, **kw):
        log.calls.append("gemm")
        return out if out is not None else torch.zeros(*a.shape[:-1], w.shape[0], dtype=BF16)

    def lora_grad(dw, up, down, scale, d_up=None, d_down=None, ws=None, accumulate=False):
        log.calls.append("lora_grad")
        log.proj.append((tuple(dw.shape), up, down, float(scale), d_up, d_down, bool(accumulate)))
        d_up.fill_(1.0), d_down.fill_(1.0)
        return d_up, d_down

    def lora_side_grad(x, dy, up, down, scale, d_up=None, d_down=None, ws=None, accumulate=False):
        log.calls.append("lora_side_grad")
        log.side.append(types.SimpleNamespace(x=x, dy=dy, up=up, down=down, scale=float(scale), d_up=d_up, d_down=d_down,
                                              ws=ws, accumulate=bool(accumulate)))
        d_up.fill_(2.0), d_down.fill_(2.0)
        return d_up, d_down

    def generic(name, result=None):
        def f(*args, **kw):
            log.calls.append(name)
            if kw.get("out") is not None:
                return kw["out"]
            return result(*args, **kw) if result is not None else None
        return f

    special = dict(
        lora_merge=merge, gemm=gemm, lora_grad=lora_grad, lora_side_grad=lora_side_grad,
        gemm_grouped=generic("gemm_grouped"), lora_grad_ws=lambda N, K, r, dev: torch.empty(0),
        lora_side_grad_ws_floats=lambda B_, R, N, K, r: B_ * R + N + K + r,
        colsum=generic("colsum", lambda x, **kw: torch.zeros(x.shape[-1])),
        qkv_post_bwd=generic("qkv_post_bwd", lambda *a, **kw: torch.zeros(2, 2, 128)),
        rowdot=generic("rowdot"),
        sumsq=lambda tensors, out=None: torch.stack([t.double().pow(2).sum() for t in ([tensors] if torch.is_tensor(tensors) else tensors)]).sum().reshape(1),
        flow_loss=generic("flow_loss", lambda pred, *a, **kw: (torch.zeros(1, dtype=torch.float64), torch.zeros_like(pred))),
    )

    def adamw_step(master, grad, exp_avg, exp_avg_sq, step, lr, betas=None, eps=None, weight_decay=None, grad_sumsq=None,
                   max_grad_norm=None, param_bf16=None, grad_scale=1.0):
        master.sub_(lr * grad_scale * grad.float())
        param_bf16.copy_(master)
    special["adamw_step"] = adamw_step
    keep = {"pack_rope", "rows_of", "launch_plan", "launch_config_epoch", "pack_key_mask"}
    for name, fn in list(vars(ops).items()):
        if name in special:
            monkeypatch.setattr(ops, name, special[name])
        elif isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not name.startswith("_") and name not in keep:
            monkeypatch.setattr(ops, name, generic(name))
    m.log = log
    return m


def _batch(B_=1):
    g = torch.Generator().manual_seed(1)
    h = w = 8                                           # 16 target tokens + 8 condition tokens = S_IMG
    return dict(model_input=torch.randn(B_, 16, h, w, generator=g), cond_latents=torch.randn(B_, 16, 4, 8, generator=g),
                noise=torch.randn(B_, 16, h, w, generator=g), sigmas=torch.full((B_,), 0.5),
                prompt_embeds=torch.randn(B_, S_TXT, 4096, generator=g).to(BF16), pooled=torch.randn(B_, 768, generator=g).to(BF16))


def test_keyword_validation(model):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    model.add_lora_adapter("t", rank=4)
    with pytest.raises(ValueError, match="lora_backward"):
        DenoiserTrainStep(model, lora="t", lora_backward="side")
    with pytest.raises(ValueError, match="needs lora="):
        DenoiserTrainStep(model, lora_backward="factored")
    assert not model._train_packs                        # refused before the model was touched
    assert DenoiserTrainStep(model, lora="t").lora_backward == "projected"


def test_the_wgrad_set_excludes_exactly_the_side_targets(model):
    from gpt_image_edit_amd.backward import FluxBackward
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    targets = model.add_lora_adapter("t", rank=4, target_modules=MIXED)
    full = model.lora_backward_weights("t")
    ts = DenoiserTrainStep(model, lora="t", lora_backward="factored")
    side = set(targets) - PROJECTED
    assert ts.bw.side == side and all(FluxBackward.side_routable(k) for k in side)
    assert not any(FluxBackward.side_routable(k) for k in PROJECTED)
    # the wgrad set: the projected targets only -- the side targets are gone, and with them the q / k / v members that only
    # completed a group whose fused weight gradient nobody reads any more
    assert ts.bw.trainable == PROJECTED and ts.bw.trainable | side | (full - set(targets)) == full
    assert ts.bw._rewritten == full                      # refresh() still re-packs everything the optimiser rewrites
    assert ts.trainable_names() == {p[:-len("weight")] + s for p in targets for s in (A, B)}
    # side=None: nothing changes
    model2_bw = FluxBackward(model, lora="t")
    assert model2_bw.trainable == full and model2_bw.side == set()


def test_side_refusals(model):
    from gpt_image_edit_amd.backward import FluxBackward
    model.add_lora_adapter("t", rank=4)
    with pytest.raises(ValueError, match="not in the trainable set"):
        FluxBackward(model, lora="t", side={D0 + "ff.net.2.weight"})
    # a full-weight backward (every trainable weight's gradient is read): a q / k / v group is side as a whole
    model.unload_lora()
    names = [D0 + f"attn.{n}.weight" for n in QKV]
    with pytest.raises(ValueError, match="as a whole"):
        FluxBackward(model, trainable=names, side=names[:1])
    bw = FluxBackward(model, trainable=names + [D0 + "ff.net.2.weight"], side=names + [D0 + "ff.net.2.weight"])
    assert bw.side == set(names) and bw.trainable == {D0 + "ff.net.2.weight"}
    bw._saved = object()
    with pytest.raises(RuntimeError, match="side_sink"):
        bw.backward(torch.zeros(1, S_IMG, 64, dtype=BF16))


@pytest.mark.parametrize("B_", [1, 2])
def test_one_side_call_per_target_with_the_right_views(model, B_):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    targets = model.add_lora_adapter("t", rank=4, weight=0.5, target_modules=MIXED)
    ts = DenoiserTrainStep(model, lora="t", lora_backward="factored", store_activations=True)
    # the optimiser's protocol, recorded
    seen = []
    real_target, real_written = ts.local.grad_target, ts.local.written
    ts.local.grad_target = lambda name: (seen.append(("target", name)), real_target(name))[1]
    ts.local.written = lambda names: (seen.append(("written", tuple(names))), real_written(names))[1]
    loss, grads, _ = ts.forward_backward(**_batch(B_))
    log = model.log
    side = sorted(set(targets) - PROJECTED)
    assert len(log.side) == len(side) and len(log.proj) == len(PROJECTED)
    bufs = ts.bw._buf
    S = S_TXT + S_IMG
    img, txt = slice(S_TXT, None), slice(0, S_TXT)
    want = {}                                           # target -> (dy view, x view) on the backward's own buffers
    blk = bufs["blk0"]
    for k, n in enumerate(QKV):
        want[D0 + f"attn.{n}.weight"] = (bufs["dqkv"][:, img, k * D:(k + 1) * D], blk.n[:, img])
    for k, n in enumerate(("add_q_proj", "add_k_proj", "add_v_proj")):
        want[D0 + f"attn.{n}.weight"] = (bufs["dqkv"][:, txt, k * D:(k + 1) * D], blk.n[:, txt])
    o = bufs["o_ckpt"][0]
    want[D0 + "attn.to_out.0.weight"] = (bufs["dy"][:, img], o[:, img])
    want[D0 + "attn.to_add_out.weight"] = (bufs["dy"][:, txt], o[:, txt])
    want[D0 + "ff.net.0.proj.weight"] = (bufs["dff"][:, img], blk.n2[:, img])
    want[D0 + "ff_context.net.0.proj.weight"] = (bufs["dff"][:, txt], blk.n2[:, txt])
    for j, s in ((1, S0), (2, S1)):
        n1 = bufs[f"blk{j}"].n
        want[s + "proj_mlp.weight"] = (bufs["dff"], n1)
        for k, n in enumerate(QKV):
            want[s + f"attn.{n}.weight"] = (bufs["dqkv"][:, :, k * D:(k + 1) * D], n1)
    assert sorted(want) == side

    def same_view(a, b):
        return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype

    by_factor = {}
    for c in log.side:
        pname = next(p for p, e in model._lora_adapters["t"].items() if e.up is c.up)
        assert pname not in by_factor, f"two side calls for {pname}"
        by_factor[pname] = c
        e = model._lora_adapters["t"][pname]
        dy, x = want[pname]
        assert same_view(c.dy, dy) and same_view(c.x, x), pname
        assert c.dy.shape == (B_, dy.shape[1], e.up.shape[0]) and c.x.shape == (B_, x.shape[1], e.down.shape[1])
        assert c.down is e.down and c.scale == 0.5 and c.accumulate is False        # the merge scale (alpha / rank = 1, weight 0.5)
        stem = pname[:-len("weight")]
        assert c.d_up is grads[stem + B] and c.d_down is grads[stem + A] and bool((c.d_up == 2.0).all())
        assert c.ws is ts._side_ws and c.ws.numel() >= B_ * dy.shape[1] + e.up.shape[0] + e.down.shape[1] + e.rank
    assert sorted(by_factor) == side
    # the order of the backward: single blocks from the last, then the double block
    order = [next(p for p, e in model._lora_adapters["t"].items() if e.up is c.up) for c in log.side]
    assert [p.split(".")[0] + "." + p.split(".")[1] for p in order] == ["single_transformer_blocks.1"] * 4 + \
        ["single_transformer_blocks.0"] * 4 + ["transformer_blocks.0"] * 10
    # grad_target (up, then down), then written([up, down]) -- per target, side and projected alike
    assert len(seen) == 3 * len(targets)
    for i in range(0, len(seen), 3):
        (k0, up), (k1, down), (k2, both) = seen[i:i + 3]
        assert (k0, k1, k2) == ("target", "target", "written") and both == (up, down)
        assert up.endswith(B) and down == up[:-len(B)] + A
    assert set(grads) == ts.trainable_names()
    for p in PROJECTED:                                  # the mixed path: these came through the projection of dW
        assert bool((grads[p[:-len("weight")] + B] == 1.0).all())
    # no wgrad GEMM, no dW, no bias reduction for a side target: the only weight-gradient work left is the projected targets'
    ts.optimizer_step(grads)
    assert ts.step_count == 1


def test_the_default_mode_makes_the_same_calls_as_before(model):
    """``lora_backward="projected"`` (the default) against a step built without the keyword: the same stubbed calls in the same
    order, no side call, the wgrad set untouched."""
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    targets = model.add_lora_adapter("t", rank=4, target_modules=MIXED)
    runs = []
    for kw in ({}, dict(lora_backward="projected")):
        model._train_packs = False
        ts = DenoiserTrainStep(model, lora="t", store_activations=True, **kw)
        assert ts.bw.side == set() and ts.bw.trainable == model.lora_backward_weights("t")
        del model.log.calls[:], model.log.side[:], model.log.proj[:]
        ts.forward_backward(**_batch())
        assert not model.log.side and len(model.log.proj) == len(targets)
        runs.append(list(model.log.calls))
    assert runs[0] == runs[1] and "lora_side_grad" not in runs[0]
    # and the factored step replaces, for its side targets, wgrad work by side calls: fewer GEMMs, the same projections left
    model._train_packs = False
    ts = DenoiserTrainStep(model, lora="t", store_activations=True, lora_backward="factored")
    del model.log.calls[:], model.log.side[:], model.log.proj[:]
    ts.forward_backward(**_batch())
    calls = model.log.calls
    assert calls.count("lora_side_grad") == len(targets) - len(PROJECTED) and calls.count("lora_grad") == len(PROJECTED)
    assert calls.count("gemm") < runs[0].count("gemm") and calls.count("colsum") < runs[0].count("colsum")
