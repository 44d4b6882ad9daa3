"""CPU: the multistep solver's host logic -- the scheduler (the parent's schedule, the refusal), the command-line flag, and the
calls the pipeline's loop makes with ``ops`` replaced by a recorder and the transformer and the VAE by stand-ins (the pattern of
tests/test_first_block_host.py).  With the default scheduler the recorded calls are the ones the loop made before."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as R  # noqa: E402

BF = torch.bfloat16
B, H, W = 2, 64, 96
HL, WL = H // 8, W // 8
S_TGT = (HL // 2) * (WL // 2)


# ---- the scheduler --------------------------------------------------------------------------------------------------------------
def _pair(n=7, s_tgt=1024):
    from gpt_image_edit_amd import helpers
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
    a, b = FlowMatchEulerDiscreteScheduler(), FlowMatchMultistepScheduler()
    for s in (a, b):
        s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=helpers.calculate_shift(s_tgt), device="cpu")
    return a, b


def test_schedule_is_the_parents_bits():
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
    a, b = _pair()
    assert issubclass(FlowMatchMultistepScheduler, FlowMatchEulerDiscreteScheduler)
    assert torch.equal(a.timesteps, b.timesteps) and torch.equal(a.sigmas, b.sigmas)
    assert a._sigmas_host.tobytes() == b._sigmas_host.tobytes() and b._sigmas_host.dtype == np.float32
    assert all(a.dsigma(i) == b.dsigma(i) and a.sigma_next(i) == b.sigma_next(i) for i in range(7))
    assert b.order == 1 and b.solver_order == 2 and b.lower_order_final is True and a.order == 1
    assert not hasattr(a, "solver_order")
    assert FlowMatchMultistepScheduler(lower_order_final=False).lower_order_final is False
    assert b.config == a.config and FlowMatchMultistepScheduler(shift=2.0).config["shift"] == 2.0
    b.set_begin_index(3)
    assert b.begin_index == 3 and b.index_for_timestep(b.timesteps[4]) == 4
    # without dynamic shifting too
    c = FlowMatchMultistepScheduler(use_dynamic_shifting=False)
    c.set_timesteps(num_inference_steps=5)
    d = FlowMatchEulerDiscreteScheduler(use_dynamic_shifting=False)
    d.set_timesteps(num_inference_steps=5)
    assert torch.equal(c.sigmas, d.sigmas)


def test_a_schedule_that_does_not_decrease_is_refused():
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
    for bad in ([1.0, 0.5, 0.5, 0.25], [1.0, 0.25, 0.5], [0.5, 1.0], [1.0, 0.5, 0.0]):   # the last: the appended 0 repeats it
        s = FlowMatchMultistepScheduler(use_dynamic_shifting=False, shift=1.0)
        with pytest.raises(ValueError, match="strictly decreasing"):
            s.set_timesteps(sigmas=bad)
        FlowMatchEulerDiscreteScheduler(use_dynamic_shifting=False, shift=1.0).set_timesteps(sigmas=bad)   # the parent takes it
    s = FlowMatchMultistepScheduler(use_dynamic_shifting=False, shift=1.0)
    s.set_timesteps(sigmas=[1.0, 0.5, 0.25])
    assert s.coefficients(1, True) == (-0.25 * 1.25, 0.25 * 0.25, 1)       # r = 1/2: c_v = d (1 + 1/4), c_h = -d / 4
    assert s.coefficients(1, False) == (-0.25, 0.0, 0) and s.coefficients(2, True) == (-0.25, 0.0, 0)


def test_both_command_lines_parse_the_flag(monkeypatch):
    from gpt_image_edit_amd.eval import gen_samples
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
    from gpt_image_edit_amd.serve import cli
    base = ["--model_path", "m", "--flux_path", "f"]
    gbase = base + ["--gedit_prompt_path", "p", "--output_dir", "o"]
    for parser, args in ((cli.build_parser(), base), (gen_samples.build_parser(), gbase)):
        assert parser.parse_args(args).solver == "euler"
        assert parser.parse_args(args + ["--solver", "ab2"]).solver == "ab2"
        with pytest.raises(SystemExit):
            parser.parse_args(args + ["--solver", "heun"])
    assert cli.SOLVERS == {"euler": FlowMatchEulerDiscreteScheduler, "ab2": FlowMatchMultistepScheduler}
    assert cli.solver_kwargs(cli.build_parser().parse_args(base)) == {}            # the default: load_pipe is called as before
    seen = []

    class Stop(Exception):
        pass

    def fake_load_pipe(model_path, flux_path, device, weight_format="bf16", solver="euler"):
        seen.append(solver)
        raise Stop
    monkeypatch.setattr(cli, "load_pipe", fake_load_pipe)
    monkeypatch.setattr(gen_samples.dp, "init_from_env", lambda: (0, 0, 1))
    monkeypatch.setattr(gen_samples.torch.cuda, "set_device", lambda d: None)
    for extra in ([], ["--solver", "ab2"]):
        with pytest.raises(Stop):
            cli.main(cli.build_parser().parse_args(base + extra))
        with pytest.raises(Stop):
            gen_samples.main(gen_samples.build_parser().parse_args(gbase + extra))
    assert seen == ["euler", "euler", "ab2", "ab2"]


# ---- the loop's calls -----------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, a, k))
            return k.get("out")
        return f


class _Transformer:
    config = SimpleNamespace(in_channels=64, guidance_embeds=True)
    device, dtype = "cpu", BF

    def __init__(self):
        self.calls = 0

    def __call__(self, hidden_states=None, **kw):
        self.calls += 1
        return (torch.full_like(hidden_states, float(self.calls)),)


def _pipe(monkeypatch, scheduler=None, use_graph=False):
    from gpt_image_edit_amd import pipeline
    rec = _Recorder()
    monkeypatch.setattr(pipeline, "ops", rec)
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=[1, 2, 3, 4], latent_channels=16, scaling_factor=1.0,
                                                 shift_factor=0.0))
    pipe = pipeline.FluxKontextPipeline(_Transformer(), vae, scheduler, use_graph=use_graph)
    g = torch.Generator().manual_seed(3)
    kw = dict(image=torch.randn(B, 16, HL, WL, generator=g).to(BF), prompt_embeds=torch.randn(B, 5, 32, generator=g).to(BF),
              pooled_prompt_embeds=torch.randn(B, 8, generator=g).to(BF), height=H, width=W,
              latents=torch.randn(B, S_TGT, 64, generator=g).to(BF), output_type="latent", max_area=H * W, _auto_resize=False)
    seen = []
    inner = pipe._denoise
    monkeypatch.setattr(pipe, "_denoise", lambda L, *a: (seen.append(L), inner(L, *a))[1])
    return SimpleNamespace(pipe=pipe, rec=rec, kw=kw, L=seen)


def _steps(rec):
    return [c for c in rec.calls if c[0] in ("euler_step", "euler_inpaint_step", "ab2_step")]


def _multistep(**kw):
    from gpt_image_edit_amd.scheduler import FlowMatchMultistepScheduler
    return FlowMatchMultistepScheduler(**kw)


@pytest.mark.parametrize("lower_order_final", [True, False])
def test_recorded_calls_of_an_ab2_edit(monkeypatch, lower_order_final):
    e = _pipe(monkeypatch, _multistep(lower_order_final=lower_order_final))
    n = 5
    e.pipe(num_inference_steps=n, **e.kw)
    calls, L = _steps(e.rec), e.L[0]
    assert [c[0] for c in calls] == ["ab2_step"] * n and e.pipe.transformer.calls == n
    assert [c[1][6] for c in calls] == ([0, 1, 1, 1, 0] if lower_order_final else [0, 1, 1, 1, 1])
    sig = R.schedule(n, S_TGT)
    for i, (_, a, k) in enumerate(calls):
        tokens, v, hist, s_tgt, c_v, c_h, use_hist, sigma_next, x0, noise, mask = a
        assert not k and tokens is L.tokens and hist is L.hist and s_tgt == S_TGT
        assert (c_v, c_h, use_hist) == R.coefficients(sig, i, i > 0, lower_order_final)
        assert sigma_next == 0.0 and x0 is None and noise is None and mask is None
        assert float(v.flatten()[0]) == i + 1                            # this step's velocity
    assert tuple(L.hist.shape) == (B, S_TGT, 64) and L.hist.dtype == BF and L.hist.is_contiguous()
    assert L.hist.data_ptr() != L.tokens.data_ptr()
    assert L.ab2 == [R.coefficients(sig, i, i > 0, lower_order_final) for i in range(n)]
    assert len(L.dsigma) == n                                            # the loop's length is still the Euler list's


def test_one_step_is_a_single_first_order_call(monkeypatch):
    for lof in (True, False):
        e = _pipe(monkeypatch, _multistep(lower_order_final=lof))
        e.pipe(num_inference_steps=1, **e.kw)
        (name, a, _), = _steps(e.rec)
        sig = R.schedule(1, S_TGT)
        assert name == "ab2_step" and a[4:7] == (float(sig[1] - sig[0]), 0.0, 0) and a[4] == -1.0
    e = _pipe(monkeypatch, _multistep())
    e.pipe(num_inference_steps=2, **e.kw)
    assert [c[1][6] for c in _steps(e.rec)] == [0, 0]


def test_strength_starts_without_history_at_the_begin_index(monkeypatch):
    e = _pipe(monkeypatch, _multistep())
    e.pipe(num_inference_steps=6, strength=0.5, **e.kw)
    calls = _steps(e.rec)
    sig = R.schedule(6, S_TGT)
    assert e.pipe.scheduler.begin_index == 3 and [c[0] for c in calls] == ["ab2_step"] * 3
    assert [c[1][6] for c in calls] == [0, 1, 0]
    assert [c[1][4:7] for c in calls] == [R.coefficients(sig, 3, False), R.coefficients(sig, 4, True), R.coefficients(sig, 5, True)]
    # an edit that preserves a picture hands the keep region's noise level on, and no mask means no x0 / noise
    assert [c[1][7] for c in calls] == [float(sig[4]), float(sig[5]), 0.0]
    assert all(c[1][8] is None and c[1][9] is None and c[1][10] is None for c in calls)
    assert [c[0] for c in e.rec.calls if c[0] == "scale_noise"] == ["scale_noise"]


def test_default_scheduler_makes_the_calls_it_made(monkeypatch):
    e = _pipe(monkeypatch)
    e.pipe(num_inference_steps=4, **e.kw)
    L = e.L[0]
    sch = e.pipe.scheduler
    assert type(sch).__name__ == "FlowMatchEulerDiscreteScheduler"
    assert [c[0] for c in e.rec.calls] == ["euler_step"] * 4              # nothing else goes through ops in this edit
    for i, (_, a, k) in enumerate(e.rec.calls):
        assert not k and a[0] is L.tokens and a[2:] == (S_TGT, sch.dsigma(i)) and len(a) == 4
    assert L.ab2 is None and L.hist is None                               # no coefficient list, no history buffer
    e = _pipe(monkeypatch)
    e.pipe(num_inference_steps=6, strength=0.5, **e.kw)
    sch = e.pipe.scheduler
    assert [c[0] for c in e.rec.calls] == ["scale_noise"] + ["euler_inpaint_step"] * 3
    for k, (_, a, kw) in enumerate(e.rec.calls[1:]):
        assert not kw and a[2:] == (S_TGT, sch.dsigma(3 + k), sch.sigma_next(3 + k), None, None, None)
    assert e.L[0].ab2 is None and e.L[0].hist is None


def test_graph_key_differs_between_the_two_schedulers(monkeypatch):
    keys = {}
    for name, sch in (("euler", None), ("ab2", _multistep()), ("ab2_full", _multistep(lower_order_final=False))):
        e = _pipe(monkeypatch, sch, use_graph=True)
        got = []
        monkeypatch.setattr(e.pipe, "_denoise_graph", lambda L, got=got: (got.append(L), L.tokens)[1])
        e.pipe(num_inference_steps=4, **e.kw)
        keys[name] = e.pipe._graph_key(got[0])
        assert keys[name] == e.pipe._graph_key(got[0])
    assert len(set(keys.values())) == 3
    assert keys["euler"][-2:] == (1, None) and keys["ab2"][-2] == 2
    assert keys["ab2"][-1] == tuple(R.coefficients(R.schedule(4, S_TGT), i, i > 0) for i in range(4))
    assert keys["euler"][:-2] == keys["ab2"][:-2]                          # the solver is the only difference
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    assert "hist" not in FluxKontextPipeline._GRAPH_INPUTS               # the graph's own buffer, not an input
