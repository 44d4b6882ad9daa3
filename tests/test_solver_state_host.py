"""CPU: the float32 latent state's host logic -- the keyword, the command-line flag, and the calls the pipeline's loop makes with
``ops`` replaced by a recorder and the transformer and the VAE by stand-ins (the pattern of tests/test_solver_host.py).  With the
default state the recorded calls are the ones the loop made before, for both schedulers."""
import inspect
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solver_ref as R  # noqa: E402

BF = torch.bfloat16
B, H, W = 2, 64, 96
HL, WL = H // 8, W // 8
S_TGT = (HL // 2) * (WL // 2)
STEP_OPS = ("euler_step", "euler_inpaint_step", "ab2_step", "solver_step_f32")


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


def _multistep(**kw):
    from gpt_image_edit_amd.scheduler import FlowMatchMultistepScheduler
    return FlowMatchMultistepScheduler(**kw)


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
    return [c for c in rec.calls if c[0] in STEP_OPS]


# ---- the keyword and the flag -----------------------------------------------------------------------------------------------------
def test_keyword_is_validated_before_any_work(monkeypatch):
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    p = inspect.signature(FluxKontextPipeline.__call__).parameters
    assert p["latent_state"].default == "bf16" and list(p)[-1] == "latent_state"       # appended: positional callers are untouched
    for bad in ("fp16", "float32", "FP32", "", None, 32):
        e = _pipe(monkeypatch)
        with pytest.raises(ValueError, match="latent_state"):
            e.pipe(num_inference_steps=2, latent_state=bad, **e.kw)
        assert e.rec.calls == [] and e.pipe.transformer.calls == 0
    from gpt_image_edit_amd import ops
    q = inspect.signature(ops.solver_step_f32).parameters
    assert list(q) == ["state", "x", "v", "s_tgt", "c_v", "c_h", "use_hist", "load_state", "hist", "sigma_next", "x0", "noise",
                       "mask"]
    assert (q["c_h"].default, q["use_hist"].default, q["load_state"].default, q["sigma_next"].default) == (0.0, 0, 1, 0.0)
    assert all(q[n].default is None for n in ("hist", "x0", "noise", "mask"))


def test_both_command_lines_parse_the_flag(monkeypatch):
    from gpt_image_edit_amd.eval import gen_samples
    from gpt_image_edit_amd.serve import cli
    base = ["--model_path", "m", "--flux_path", "f"]
    gbase = base + ["--gedit_prompt_path", "p", "--output_dir", "o"]
    for parser, args in ((cli.build_parser(), base), (gen_samples.build_parser(), gbase)):
        assert parser.parse_args(args).latent_state == "bf16"
        assert parser.parse_args(args + ["--latent_state", "fp32"]).latent_state == "fp32"
        assert parser.parse_args(args + ["--latent_state", "fp32", "--solver", "ab2"]).solver == "ab2"
        with pytest.raises(SystemExit):
            parser.parse_args(args + ["--latent_state", "fp16"])
    assert cli.latent_state_kwargs(cli.build_parser().parse_args(base)) == {}           # the default: the pipeline is called as before
    assert cli.latent_state_kwargs(cli.build_parser().parse_args(base + ["--latent_state", "fp32"])) == {"latent_state": "fp32"}
    assert cli.latent_state_kwargs(SimpleNamespace()) == {}
    # the flag reaches the pipeline call of the prompt-embeds route
    got = []

    def fake_pipe(**kw):
        got.append(kw)
        return SimpleNamespace(images=[None])
    fake_pipe.device = "cpu"
    monkeypatch.setattr(cli, "prepare_condition_pixels", lambda paths: None)
    monkeypatch.setattr(cli.torch, "Generator", lambda device=None: SimpleNamespace(manual_seed=lambda seed: None))
    for extra in ([], ["--latent_state", "fp32"]):
        cli.generate_image(fake_pipe, None, None, [], 64, 64, cli.build_parser().parse_args(base + extra))
    assert "latent_state" not in got[0] and got[1]["latent_state"] == "fp32"
    assert "latent_state_kwargs(args)" in inspect.getsource(gen_samples.main) and \
        "latent_state_kwargs(args)" in inspect.getsource(cli.run_t5_only)


# ---- the loop's calls -----------------------------------------------------------------------------------------------------------
def _check_state_buffer(L):
    assert L.latent_state == "fp32" and L.state.dtype == torch.float32 and tuple(L.state.shape) == (B, S_TGT, 64)
    assert L.state.is_contiguous() and L.state.data_ptr() != L.tokens.data_ptr()


def test_recorded_calls_of_an_euler_edit_on_the_float32_state(monkeypatch):
    e = _pipe(monkeypatch)
    n = 5
    out = e.pipe(num_inference_steps=n, latent_state="fp32", **e.kw)
    calls, L, sch = _steps(e.rec), e.L[0], e.pipe.scheduler
    assert [c[0] for c in e.rec.calls] == ["solver_step_f32"] * n and e.pipe.transformer.calls == n
    _check_state_buffer(L)
    assert L.hist is None and L.ab2 is None
    for i, (_, a, k) in enumerate(calls):
        state, tokens, v, s_tgt, c_v, c_h, use_hist, load_state, hist, sigma_next, x0, noise, mask = a
        assert not k and state is L.state and tokens is L.tokens and s_tgt == S_TGT
        assert (c_v, c_h, use_hist) == (sch.dsigma(i), 0.0, 0) and hist is None
        assert c_v != float(torch.tensor(c_v).to(BF)) or i == 0, "the step size is handed over unrounded"
        assert load_state == (0 if i == 0 else 1)
        assert sigma_next == 0.0 and x0 is None and noise is None and mask is None
        assert float(v.flatten()[0]) == i + 1
    assert any(c[1][4] != float(torch.tensor(c[1][4]).to(BF)) for c in calls)
    assert out.latents.dtype == BF and out.images.dtype == BF             # the returned latents stay the bf16 token rows


@pytest.mark.parametrize("lower_order_final", [True, False])
def test_recorded_calls_of_an_ab2_edit_on_the_float32_state(monkeypatch, lower_order_final):
    e = _pipe(monkeypatch, _multistep(lower_order_final=lower_order_final))
    n = 5
    e.pipe(num_inference_steps=n, latent_state="fp32", **e.kw)
    calls, L = _steps(e.rec), e.L[0]
    assert [c[0] for c in e.rec.calls] == ["solver_step_f32"] * n and e.pipe.transformer.calls == n
    _check_state_buffer(L)
    sig = R.schedule(n, S_TGT)
    assert [c[1][6] for c in calls] == ([0, 1, 1, 1, 0] if lower_order_final else [0, 1, 1, 1, 1])      # use_hist as before
    assert [c[1][7] for c in calls] == [0, 1, 1, 1, 1]                                                  # load_state
    for i, (_, a, k) in enumerate(calls):
        assert not k and a[0] is L.state and a[1] is L.tokens and a[3] == S_TGT and a[8] is L.hist and L.hist is not None
        assert a[4:7] == R.coefficients(sig, i, i > 0, lower_order_final)
        assert a[9:] == (0.0, None, None, None)
    assert L.hist.dtype == BF and L.hist.data_ptr() != L.state.data_ptr()


def test_one_step_schedule(monkeypatch):
    for sch in (None, _multistep(), _multistep(lower_order_final=False)):
        e = _pipe(monkeypatch, sch)
        e.pipe(num_inference_steps=1, latent_state="fp32", **e.kw)
        (name, a, _), = e.rec.calls
        assert name == "solver_step_f32" and a[4:8] == (-1.0, 0.0, 0, 0)


def test_strength_seeds_the_state_from_the_renoised_picture(monkeypatch):
    for sch in (None, _multistep()):
        e = _pipe(monkeypatch, sch)
        e.pipe(num_inference_steps=6, strength=0.5, latent_state="fp32", **e.kw)
        sig = R.schedule(6, S_TGT)
        assert [c[0] for c in e.rec.calls] == ["scale_noise"] + ["solver_step_f32"] * 3      # the start tokens, then the steps
        L = e.L[0]
        assert e.rec.calls[0][2]["out"].data_ptr() == L.tokens.data_ptr()                    # written where step 0 reads them
        calls = _steps(e.rec)
        assert [c[1][7] for c in calls] == [0, 1, 1]
        assert [c[1][9] for c in calls] == [float(sig[4]), float(sig[5]), 0.0]               # the keep region's noise levels
        assert all(c[1][10:] == (None, None, None) for c in calls)                           # no mask: no x0, no noise
        if sch is None:
            assert [c[1][4:7] for c in calls] == [(e.pipe.scheduler.dsigma(3 + k), 0.0, 0) for k in range(3)]
        else:
            assert [c[1][4:7] for c in calls] == [R.coefficients(sig, 3, False), R.coefficients(sig, 4, True),
                                                  R.coefficients(sig, 5, True)]


def test_mask_hands_x0_noise_and_mask_to_the_step(monkeypatch):
    from gpt_image_edit_amd import ops
    e = _pipe(monkeypatch)
    e.rec.pack_inpaint_mask = ops.pack_inpaint_mask                      # host-side torch: the real one
    e.pipe(num_inference_steps=3, mask_image=torch.ones(1, 1, H, W), latent_state="fp32", **e.kw)
    L = e.L[0]
    calls = _steps(e.rec)
    assert len(calls) == 3 and L.mask is not None
    sch = e.pipe.scheduler
    for i, (_, a, _) in enumerate(calls):
        assert a[9] == sch.sigma_next(i) and a[10] is L.x0 and a[11] is L.noise and a[12] is L.mask


@pytest.mark.parametrize("ab2", [False, True])
def test_a_callback_that_returns_latents_reseeds_the_state_at_the_next_step_only(monkeypatch, ab2):
    e = _pipe(monkeypatch, _multistep() if ab2 else None)
    new = torch.full((B, S_TGT, 64), 0.5, dtype=BF)
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(i)
        return {"latents": new} if i in (1, 3) else ({} if i == 2 else None)
    e.pipe(num_inference_steps=6, latent_state="fp32", callback_on_step_end=cb, **e.kw)
    calls = _steps(e.rec)
    assert seen == list(range(6)) and [c[1][7] for c in calls] == [0, 1, 0, 1, 0, 1]
    assert torch.equal(e.L[0].tokens[:, :S_TGT], new)                    # copied into the token rows as before (ops is a stub)
    if ab2:                                                              # the history is not reset by a callback, as before
        assert [c[1][6] for c in calls] == [0, 1, 1, 1, 1, 0]
    # a callback that returns nothing changes nothing
    e = _pipe(monkeypatch, _multistep() if ab2 else None)
    e.pipe(num_inference_steps=4, latent_state="fp32", callback_on_step_end=lambda *a: None, **e.kw)
    assert [c[1][7] for c in _steps(e.rec)] == [0, 1, 1, 1]


def test_graph_key_differs_between_the_two_states(monkeypatch):
    from gpt_image_edit_amd.pipeline import FluxKontextPipeline
    for sch in (None, _multistep):
        keys = {}
        for state in ("bf16", "fp32"):
            e = _pipe(monkeypatch, sch and sch(), use_graph=True)
            got = []
            monkeypatch.setattr(e.pipe, "_denoise_graph", lambda L, got=got: (got.append(L), L.tokens)[1])
            e.pipe(num_inference_steps=4, latent_state=state, **e.kw)
            keys[state] = e.pipe._graph_key(got[0])
            assert state in keys[state]
        assert keys["bf16"] != keys["fp32"]
        assert [a == b for a, b in zip(keys["bf16"], keys["fp32"])].count(False) == 1        # the state is the only difference
        assert keys["bf16"][-2:] == keys["fp32"][-2:]                                        # the solver's entries stay last
    assert "state" not in FluxKontextPipeline._GRAPH_INPUTS and "hist" not in FluxKontextPipeline._GRAPH_INPUTS


def test_default_state_makes_the_calls_the_loop_made(monkeypatch):
    """Without the keyword, and with ``latent_state="bf16"``: the step calls, in order and argument by argument, that the loop
    made before the keyword existed, and no float32 buffer."""
    for kw_state in ({}, {"latent_state": "bf16"}):
        e = _pipe(monkeypatch)
        e.pipe(num_inference_steps=4, **kw_state, **e.kw)
        L, sch = e.L[0], e.pipe.scheduler
        assert [c[0] for c in e.rec.calls] == ["euler_step"] * 4
        for i, (_, a, k) in enumerate(e.rec.calls):
            assert not k and a[0] is L.tokens and a[2:] == (S_TGT, sch.dsigma(i)) and len(a) == 4
        assert L.state is None and L.latent_state == "bf16" and L.hist is None
        e = _pipe(monkeypatch)
        e.pipe(num_inference_steps=6, strength=0.5, **kw_state, **e.kw)
        sch = e.pipe.scheduler
        assert [c[0] for c in e.rec.calls] == ["scale_noise"] + ["euler_inpaint_step"] * 3
        for k, (_, a, kw) in enumerate(e.rec.calls[1:]):
            assert not kw and a[2:] == (S_TGT, sch.dsigma(3 + k), sch.sigma_next(3 + k), None, None, None)
        assert e.L[0].state is None
        e = _pipe(monkeypatch, _multistep())
        e.pipe(num_inference_steps=5, **kw_state, **e.kw)
        L = e.L[0]
        sig = R.schedule(5, S_TGT)
        assert [c[0] for c in e.rec.calls] == ["ab2_step"] * 5
        for i, (_, a, k) in enumerate(e.rec.calls):
            assert not k and a[0] is L.tokens and a[2] is L.hist and a[3] == S_TGT and len(a) == 11
            assert a[4:7] == R.coefficients(sig, i, i > 0) and a[7:] == (0.0, None, None, None)
        assert L.state is None
        # a callback that returns latents: copied, and nothing else changes
        e = _pipe(monkeypatch)
        e.pipe(num_inference_steps=3, callback_on_step_end=lambda p, i, t, kw: {"latents": kw["latents"]}, **kw_state, **e.kw)
        assert [c[0] for c in e.rec.calls] == ["euler_step"] * 3
