"""GPU: ``DenoiserTrainStep(optimizer="prodigy")`` on the model and batch of tests/test_hip_lora_train_step.py (full width, one double +
one single block, 16 x 16 latents, 64 text tokens): full-weight steps, LoRA steps (r = 16) and the sharded path at world 1.

Every step is held against the float64 reference of tests/prodigy_ref.py RESTARTED from the state read back before the step and fed
the step's own gradients and the step's own squared norm, so the bounds are the single-step ones of the kernels (times MARGIN = 2;
the clipping coefficient gets its 3 ulps as in tests/test_hip_prodigy_kernels.py): m, v, s per element, the two sums, d_hat through
the quotient, then -- with the kernel's new d handed to the reference, the same scalars -- the masters per element and the bf16
parameters as their rounding.

Observed on an MI355X (one run), worst error as a fraction of the derived bound BEFORE the margin -- full steps: m 0.496, v 0.499, s 0.951,
master 0.966, sum |s| 0.030, sum g (p0 - p) 0.002, d_hat 0.009; LoRA steps: m 0.495, v 0.486, s 0.865, master 0.942, sum |s| 0.074, d_hat
0.039; the sharded path at world 1 gave the per-tensor path's figures.  In these three-step runs d stays at d0 (d_hat is still below it);
it moves in the ten-step run: losses 3.410 -> 2.751, d 1.0e-4 -> 1.28e-3 from the fourth step on.  The file ran in 13 s.
"""
import numpy as np
import pytest
import torch

import prodigy_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
RANK = 16
D0, S0 = "transformer_blocks.0.", "single_transformer_blocks.0."
DEFAULT_TARGETS = sorted([D0 + f"attn.{n}.weight" for n in ("to_q", "to_k", "to_v", "to_out.0")]
                         + [S0 + f"attn.{n}.weight" for n in ("to_q", "to_k", "to_v")])
FULL = [D0 + "attn.to_q.weight", D0 + "attn.to_out.0.weight"]      # 2 x 9.4 M elements: the float64 replay of a step stays at seconds
WD = 0.01
PR = dict(d0=1e-4)      # an element moves by ~dlr per step.  The ten-step test needs BOTH a visible loss change and room for d to grow:
#                         at the 1e-3 that tests/test_hip_lora_train_step.py uses as its AdamW lr the merged bf16 weights move by a few
#                         ulps per step, and a tenth of it still moves them within ten steps (d_hat ~ d0 (k + 1) / 2 on consistent
#                         gradients, so d should leave d0 after a few steps); the default 1e-6 would not change a bf16 weight at all
# LoRA runs: without the safeguard the denominator sum |s| grows with dlr = d * bc (~0.5 d) instead of d, so on consistent gradients
# d_hat ~ 0.3 (k - 1) d instead of 0.18 (k - 1) d: d leaves d0 around step 5 instead of 7 and ten steps leave a margin
PR_LORA = dict(PR, safeguard_warmup=False)


def _model():
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=1)
    return HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=41)


def _batch(B=1, S_txt=64, h=16, w=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    b = dict(model_input=torch.randn(B, 16, h, w, generator=g), cond_latents=torch.randn(B, 16, h, w, generator=g),
             noise=torch.randn(B, 16, h, w, generator=g), sigmas=torch.tensor([0.25, 0.75][:B]),
             prompt_embeds=torch.randn(B, S_txt, 4096, generator=g).to(BF), pooled=torch.randn(B, 768, generator=g).to(BF))
    return {k: v.cuda() for k, v in b.items()}


def _random_adapter(model, mods, rank, alpha, seed):
    g = torch.Generator().manual_seed(seed)
    st = {}
    for m in mods:
        n, k = model.p(m + ".weight").shape
        st[f"transformer.{m}.lora_A.weight"] = (0.02 * torch.randn(rank, k, generator=g)).to(BF)
        st[f"transformer.{m}.lora_B.weight"] = (0.02 * torch.randn(n, rank, generator=g)).to(BF)
        st[f"transformer.{m}.alpha"] = torch.tensor(float(alpha))
    return st


def _step(model, **kw):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    return DenoiserTrainStep(model, optimizer="prodigy", weight_decay=WD, prodigy=dict(PR_LORA if "lora" in kw else PR), **kw)


class _PerTensor:
    """State access of the per-tensor path: name -> (master, m, v, s, p0) as float64 numpy, the scalars, the bf16 parameters."""

    def __init__(self, ts):
        self.ts = ts

    def names(self):
        return sorted(self.ts.trainable_names())

    def state(self):
        out = {}
        for k in self.names():
            st = self.ts.state.get(k)
            if st is None:                      # before the first step: what _state() will create
                p = self.ts._param(k).detach().float()
                st = (p, torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p), p)
            out[k] = tuple(t.detach().double().cpu().numpy().ravel() for t in st)
        return out

    def scalars(self):
        return self.ts.prodigy_state()

    def param(self, k):
        return self.ts._param(k).detach().float().cpu().numpy().ravel()


class _Sharded(_PerTensor):
    """The same through the flat chunks of ``zero.ShardedAdamW`` at world 1 (a bucket's chunk is the bucket)."""

    def state(self):
        o, L = self.ts.opt, self.ts.opt.layout
        assert o.world == 1 and all(b["offset"] == b["state_offset"] for b in L.buckets)
        out = {}
        for k in self.names():
            lo, n, _ = L.offsets[k]
            out[k] = tuple(t[lo:lo + n].detach().double().cpu().numpy() for t in (o.master, o.exp_avg, o.exp_avg_sq, o.s, o.p0))
        return out


def _checked_step(acc, batch, label, ratios):
    """One ``forward_backward`` + ``optimizer_step`` of ``acc.ts``, checked against the float64 reference restarted from the state
    before it.  Returns the loss."""
    ts = acc.ts
    before, sc = acc.state(), acc.scalars()
    loss, grads, _ = ts.forward_backward(**batch)
    g64 = {k: grads[k].detach().double().cpu().numpy().ravel() for k in acc.names()}
    sumsq = float(ts.optimizer_step(grads).item())
    after, sc2 = acc.state(), acc.scalars()
    hp = R.kernel_hp(dict(ts.prodigy, lr=ts.lr, betas=ts.betas, eps=ts.eps, weight_decay=ts.weight_decay))
    coef = R.clip_coef(sumsq, ts.max_grad_norm)
    ref = R.Ref({k: st[0] for k, st in before.items()}, hp)
    for k, (p, m, v, s, p0) in before.items():
        ref.m[k], ref.v[k], ref.s[k], ref.p0[k] = m.copy(), v.copy(), s.copy(), p0.copy()
    ref.set_scalars(**{k: sc[k] for k in ("d", "d_max", "d_numerator", "k")})
    ref.begin()
    assert abs(sc2["dlr"] - ref.dlr) <= 1e-13 * ref.dlr                       # the device's pow (tests/test_hip_prodigy_kernels.py)
    ref.set_scalars(dlr=sc2["dlr"])
    ref.moments(g64, coef)
    dot_b = abs_b = 0.0
    r = dict(m=0.0, v=0.0, s=0.0)
    clipped = coef < 1.0
    for k, (p, m, v, s, p0) in before.items():
        B = R.bounds_moments(p, p0, g64[k], m, v, s, sc["d"], sc2["dlr"], hp, coef)
        cm, cv, cs = ref._moment_factors()
        extra = 3 * R.U * np.abs(g64[k] * coef) if clipped else 0.0
        bm, bv, bs = B["m"] + abs(cm) * extra, B["v"] + 2 * np.abs(cv * g64[k] * coef) * extra, B["s"] + abs(cs) * extra
        for a, i, b in (("m", 1, bm), ("v", 2, bv), ("s", 3, bs)):
            r[a] = max(r[a], float(np.max(np.abs(after[k][i] - getattr(ref, a)[k]) / b)))
        assert np.array_equal(after[k][4], p0), f"{k}: p0 moved"
        dot_b += B["dot"] + float(np.sum(np.abs(p0 - p) * extra))
        abs_b += B["sum_abs"] + float(np.sum(abs(cs) * extra))
    assert max(r.values()) <= R.MARGIN, (label, r)
    r["dot"] = abs(sc2["sum_dot"] - ref.sum_dot) / (R.MARGIN * dot_b) if dot_b else 0.0
    r["abs"] = abs(sc2["sum_abs"] - ref.sum_abs) / (R.MARGIN * abs_b)
    assert r["dot"] <= 1.0 and r["abs"] <= 1.0, (label, r)
    d, dlr = ref.d, ref.dlr
    ref.update_d()
    assert not sc2["skipped"] and sc2["k"] == ref.k == sc["k"] + 1
    bd = R.MARGIN * R.bound_d_hat(d, dlr, ref.d_numerator, ref.d_denom, dot_b, abs_b, hp)
    err = abs(sc2["d_hat"] - ref.d_hat)
    r["d_hat"] = err / bd if bd else float(err != 0.0)             # first step: p == p0, both numerators are exactly 0
    assert r["d_hat"] <= 1.0 and abs(sc2["d"] - ref.d) <= bd and sc2["d"] >= sc["d"], (label, sc2, ref.scalars())
    ref.set_scalars(d=sc2["d"])                                                # the same scalars for the second pass
    r["p"] = 0.0
    for k in before:
        ref.m[k], ref.v[k] = after[k][1], after[k][2]                         # ... and the kernel's own moments
        ref.apply_one(k)
        bp = R.bounds_apply(before[k][0], after[k][1], after[k][2], sc2["d"], sc2["dlr"], hp)
        r["p"] = max(r["p"], float(np.max(np.abs(after[k][0] - ref.p[k]) / bp)))
        want_bf = torch.from_numpy(after[k][0]).float().to(BF).float().numpy()
        assert np.array_equal(acc.param(k), want_bf), f"{k}: the bf16 parameter is not the rounded master"
    assert r["p"] <= R.MARGIN, (label, r)
    print(f"[prodigy step] {label}: d {sc['d']:.4e} -> {sc2['d']:.4e}, loss {loss.item():.6f}, of the bounds: "
          + " ".join(f"{k} {v:.3f}" for k, v in r.items()), flush=True)
    for k, v in r.items():
        ratios[k] = max(ratios.get(k, 0.0), v)
    return loss


def test_three_full_steps_against_the_restarted_reference():
    ts = _step(_model(), trainable=FULL)
    acc, batch, ratios = _PerTensor(ts), _batch(), {}
    for i in range(3):
        _checked_step(acc, batch, f"full {i}", ratios)
    assert all(len(st) == 5 for st in ts.state.values()) and ts.step_count == 3
    print("[prodigy step] full, worst ratios:", ratios, flush=True)


def test_three_lora_steps_against_the_restarted_reference_and_the_frozen_adapter_stays():
    model = _model()
    model.load_lora_adapter(_random_adapter(model, [D0 + "attn.to_q", D0 + "ff.net.0.proj"], 8, 4, seed=5), adapter_name="f", weight=0.5)
    frozen = {p: (e.up.clone(), e.down.clone()) for p, e in model._lora_adapters["f"].items()}
    assert model.add_lora_adapter("t", rank=RANK, seed=3) == DEFAULT_TARGETS
    ts = _step(model, lora="t")
    acc, batch, ratios = _PerTensor(ts), _batch(seed=1), {}
    for i in range(3):
        _checked_step(acc, batch, f"lora {i}", ratios)
    for k, st in ts.state.items():
        assert bool(st[4].any()) != k.endswith(ts.LORA_B), "up starts at 0, so its p0 is 0; down's is not"
    for p, (up, down) in frozen.items():
        e = model._lora_adapters["f"][p]
        assert torch.equal(e.up, up) and torch.equal(e.down, down), f"the frozen adapter's {p} changed"
    assert any(bool(e.up.any()) for e in model._lora_adapters["t"].values())
    print("[prodigy step] lora, worst ratios:", ratios, flush=True)


def test_sharded_world1_steps_against_the_same_reference():
    ts = _step(_model(), trainable=FULL, sharded=True, bucket_numel=9_500_000)
    assert len(ts.opt.layout.buckets) == 2 and ts.opt.optimizer == "prodigy"
    acc, batch, ratios = _Sharded(ts), _batch(), {}
    for i in range(2):
        _checked_step(acc, batch, f"sharded {i}", ratios)
    # the first step of both paths sees the same gradients: the same d within the d_hat bound's order (both passed it above)
    pt = _step(_model(), trainable=FULL)
    _checked_step(_PerTensor(pt), batch, "per-tensor 0", {})
    print("[prodigy step] sharded, worst ratios:", ratios, flush=True)


_RUN = {}


def _run(steps, resume_from=None, collect=None):
    model = _model()
    model.add_lora_adapter("t", rank=RANK, seed=3)
    ts = _step(model, lora="t")
    if resume_from is not None:
        ts.load_state_dict(resume_from)
    batch = _batch(seed=1)
    out = []
    for i in range(steps):
        if collect is not None and i == collect:
            out.append(ts.state_dict())
        r = ts.step(**batch)
        out.append((r["loss"].clone(), {k: g.clone() for k, g in r["grads"].items()}, ts.prodigy_state()))
    return model, ts, out


def test_ten_lora_steps_lower_the_loss_d_grows_and_resume_is_bit_identical():
    model, ts, out = _run(10, collect=2)
    sd = out.pop(2)
    losses, ds = [l.item() for l, _, _ in out], [s["d"] for _, _, s in out]
    print("[prodigy lora] losses:", " ".join(f"{x:.6f}" for x in losses), "d:", " ".join(f"{x:.3e}" for x in ds), flush=True)
    assert ts.lr == 1.0
    assert losses[-1] < losses[0], losses
    assert ds[-1] > PR["d0"] and all(b >= a for a, b in zip(ds, ds[1:])), ds
    assert sd["kind"] == "lora" and sd["optimizer"] == "prodigy" and sd["step"] == 2 and all(len(st) == 5 for st in sd["state"].values())
    # resume after two steps: the third step is the uninterrupted run's, bit for bit
    model_c, ts_c, out_c = _run(1, resume_from=sd)
    assert ts_c.step_count == 3 and out_c[0][2] == out[2][2]
    assert torch.equal(out_c[0][0], out[2][0]) and all(torch.equal(out_c[0][1][k], out[2][1][k]) for k in out[2][1])
    model_d, ts_d, _ = _run(3)
    assert all(torch.equal(p.data, model_d.p(n).data) for n, p in model_c.named_parameters())
    assert all(torch.equal(a, b) for k in ts_d.state for a, b in zip(ts_d.state[k], ts_c.state[k])) and torch.equal(ts_d.pstate, ts_c.pstate)
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    plain = _model()
    plain.add_lora_adapter("t", rank=RANK, seed=3)
    with pytest.raises(ValueError, match="prodigy"):
        DenoiserTrainStep(plain, lora="t", lr=1e-3).load_state_dict(sd)


def test_adamw_with_and_without_the_keyword_gives_equal_bits():
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    batch, res = _batch(), []
    for kw in (dict(), dict(optimizer="adamw", prodigy=None)):
        model = _model()
        ts = DenoiserTrainStep(model, lr=1e-3, trainable=FULL, **kw)
        r = ts.step(**batch)
        r2 = ts.step(**batch)
        res.append((r["loss"], r2["loss"], r2["grad_sumsq"], {k: model.p(k).data.clone() for k in FULL}, ts.state_dict()))
    (l0, l1, s0, p0, sd0), (l0b, l1b, s0b, p0b, sd0b) = res
    assert torch.equal(l0, l0b) and torch.equal(l1, l1b) and torch.equal(s0, s0b) and not torch.equal(l0, l1)
    assert all(torch.equal(p0[k], p0b[k]) for k in FULL)
    assert set(sd0) == set(sd0b) == {"kind", "step", "state"}
    assert all(len(sd0["state"][k]) == 3 and all(torch.equal(a, b) for a, b in zip(sd0["state"][k], sd0b["state"][k])) for k in FULL)
