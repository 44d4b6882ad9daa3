"""CPU: the first-block step cache's host logic -- the rule (gpt_image_edit_amd/step_cache.py), the command-line forms, and the
call sequence of the transformer's two-phase forward in that mode with ``ops`` and the block routes replaced by recorders."""
import argparse
import math
from types import SimpleNamespace

import pytest
import torch

from gpt_image_edit_amd.step_cache import StepCache, from_args

FB = "first_block"


def _run(sc, rels):
    n = len(rels) + 1
    sc.begin(n)
    return [sc.step(i, None if i == 0 else (rels[i - 1], 1.0)) for i in range(n)]


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def test_first_and_last_step_always_compute():
    sc = StepCache(threshold=1e9, measure=FB)
    assert sc.decide(0.0, 123.0, 0, 5) == (True, 0.0)
    assert sc.decide(0.0, 0.0, 4, 5) == (True, 0.0)
    assert sc.decide(0.0, 0.0, 3, 5) == (False, 0.0)
    assert _run(sc, [0.0] * 4) == [True, False, False, False, True]
    assert _run(StepCache(threshold=1e9, measure=FB), []) == [True]


def test_the_comparison_is_greater_or_equal_and_nothing_accumulates():
    sc = StepCache(threshold=0.5, measure=FB)
    assert sc.decide(0.0, 0.5, 1, 9) == (True, 0.0) and sc.decide(0.0, math.nextafter(0.5, 0.0), 1, 9) == (False, 0.0)
    rels = [0.2, 0.2, 0.2, 0.4, 0.5, 0.3, 0.6, 0.1]
    # the other measure adds these up (.2 .4 .6*): this one compares each on its own
    assert _run(sc, rels) == [True, False, False, False, False, True, False, True, True]
    assert sc.computed_steps == [0, 5, 7, 8] and sc.rel_l1 == rels
    assert _run(StepCache(threshold=0.5), rels) == [True, False, False, True, False, True, False, True, True]
    # decide is pure: an accumulator handed in is ignored and none comes back
    before = (list(sc.computed_steps), list(sc.rel_l1))
    assert sc.decide(123.0, 0.2, 3, 9) == (False, 0.0) and sc.decide(123.0, 0.2, 3, 9) == (False, 0.0)
    assert (sc.computed_steps, sc.rel_l1) == before
    rp = StepCache(schedule=sc.computed_steps, measure=FB)
    assert _run(rp, rels) == [True, False, False, False, False, True, False, True, True] and rp.rel_l1 == []


def test_zero_denominator_and_the_ends_of_the_threshold_range():
    sc = StepCache(threshold=1e30, measure=FB)
    sc.begin(4)
    assert [sc.step(0), sc.step(1, (0.0, 0.0)), sc.step(2, (1.0, 1.0)), sc.step(3, (1.0, 1.0))] == [True, True, False, True]
    assert sc.rel_l1 == [math.inf, 1.0, 1.0]
    assert StepCache(threshold=math.inf, measure=FB).decide(0.0, math.inf, 1, 4) == (True, 0.0)
    assert StepCache(threshold=1.0, measure=FB).decide(0.0, math.nan, 1, 4) == (True, 0.0)     # never skip on a NaN
    assert _run(StepCache(threshold=0, measure=FB), [0.0, 0.3, 0.0, 0.1]) == [True] * 5
    sc = StepCache(threshold=math.inf, measure=FB)
    assert _run(sc, [5.0, 1e30, 7.0, 2.0]) == [True, False, False, False, True] and sc.computed_steps == [0, 4]


def test_constructor_refusals_and_attributes():
    with pytest.raises(ValueError, match="coefficients"):
        StepCache(threshold=0.1, measure=FB, coefficients=(0.0, 2.0))
    with pytest.raises(ValueError, match="coefficients"):
        StepCache(schedule=[0], measure=FB, coefficients=(0.5, 1.0))
    StepCache(threshold=0.1, measure=FB, coefficients=[0, 1])                 # the default, spelt out
    for bad in ("second_block", None, "", 1):
        with pytest.raises(ValueError, match="measure"):
            StepCache(threshold=0.1, measure=bad)
    with pytest.raises(ValueError, match="exactly one"):
        StepCache(measure=FB)
    with pytest.raises(ValueError, match="exactly one"):
        StepCache(threshold=0.1, schedule=[0], measure=FB)
    sc = StepCache(threshold=0.25, measure=FB)
    assert sc.measure == FB and sc.first_block and sc.adaptive and sc.threshold == 0.25 and sc.schedule is None
    d = StepCache(threshold=0.25)
    assert d.measure == "input" and not d.first_block and StepCache(threshold=0.25, measure="input").measure == "input"
    # the default mode's attributes are the first-block mode's but for `measure`
    a, b = vars(d), vars(sc)
    assert set(a) == set(b) and {k for k in a if a[k] != b[k]} == {"measure"}


def test_schedule_with_first_block_validates_as_before():
    for bad in ([], [1, 2], [0, 2, 2], [0, 3, 1], [0, -1], [0, 1.5]):
        with pytest.raises(ValueError, match="schedule"):
            StepCache(schedule=bad, measure=FB)
    sc = StepCache(schedule=range(4), measure=FB)
    assert sc.schedule == (0, 1, 2, 3) and not sc.adaptive and sc.first_block
    sc.validate(4)
    with pytest.raises(ValueError, match="schedule"):
        sc.validate(3)
    with pytest.raises(ValueError):
        sc.validate(0)
    assert _run(StepCache(schedule=[0, 2], measure=FB), [9.0, 9.0, 9.0]) == [True, False, True, False]


def test_command_line_forms():
    assert from_args(measure=FB) is None
    sc = from_args(threshold=0.25, measure=FB)
    assert sc.first_block and sc.adaptive and sc.threshold == 0.25
    assert from_args(schedule="0,2,5", measure=FB).schedule == (0, 2, 5) and from_args(schedule="0,2", measure=FB).first_block
    assert from_args(threshold=0.25).measure == "input" and from_args(threshold=0.25, measure="input").measure == "input"
    with pytest.raises(ValueError, match="coefficients"):
        from_args(threshold=0.1, coefficients="0,2", measure=FB)
    with pytest.raises(ValueError, match="measure"):
        from_args(threshold=0.1, measure="nope")


def test_both_command_lines_parse_the_flag():
    from gpt_image_edit_amd.eval import gen_samples
    from gpt_image_edit_amd.serve import cli
    p = argparse.ArgumentParser()
    cli.add_step_cache_arguments(p)
    a = p.parse_args(["--step_cache_threshold", "0.1", "--step_cache_measure", "first_block"])
    sc = cli.step_cache_kwargs(a)["step_cache"]
    assert sc.first_block and sc.threshold == 0.1
    assert cli.step_cache_kwargs(p.parse_args(["--step_cache_schedule", "0,2"]))["step_cache"].measure == "input"
    assert cli.step_cache_kwargs(p.parse_args(["--step_cache_measure", "first_block"])) == {}
    with pytest.raises(SystemExit):
        p.parse_args(["--step_cache_measure", "second_block"])
    import inspect
    src = inspect.getsource(gen_samples)
    assert "add_step_cache_arguments" in src and "step_cache_kwargs(args)" in src     # gen_samples shares the flag and its reading
    full = cli.build_parser() if hasattr(cli, "build_parser") else None
    if full is not None:
        assert any("--step_cache_measure" in x.option_strings for x in full._actions)


# ---- the transformer's call sequence ------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a, **k):
            self.calls.append((name, a, k))
            if name == "absdiff_ws":
                return torch.zeros(4)
            return k.get("out")
        return f


@pytest.fixture
def fake(monkeypatch):
    """A HipFluxTransformer2DModel without weights or a GPU: frame, modulation, blocks and head are recorders, ``ops`` too."""
    from gpt_image_edit_amd import transformer
    rec = _Recorder()
    monkeypatch.setattr(transformer, "ops", rec)
    Bq, S_txt, S_img, D = 2, 3, 5, 16
    tr = object.__new__(transformer.HipFluxTransformer2DModel)
    torch.nn.Module.__init__(tr)
    tr.inner_dim = D
    s = torch.zeros(Bq, S_txt + S_img, D, dtype=torch.bfloat16)
    pk = SimpleNamespace(double=[SimpleNamespace(mod_img=0, mod_txt=0)], single=[SimpleNamespace(mod=0)] * 2)
    f = SimpleNamespace(pk=pk, ws=SimpleNamespace(s=s), B=Bq, S_img=S_img, S_txt=S_txt, hs="hs", enc="enc", h=s[:, S_txt:],
                        cx=s[:, :S_txt])
    tr._infer_frame = lambda *a: f
    mod = torch.zeros(Bq, 8 * D, dtype=torch.bfloat16)
    tr._infer_modulation = lambda *a: mod
    tr._infer_blocks = lambda f_, mod_, key_mask=None, blocks=None: rec.calls.append(("blocks", (mod_, key_mask), dict(blocks=blocks)))
    tr._infer_head = lambda f_, mod_: rec.calls.append(("head", (mod_,), {})) or "sample"
    tr.p = lambda name: name
    tr.packed = lambda: pk
    return SimpleNamespace(tr=tr, rec=rec, f=f, pk=pk, x=SimpleNamespace(is_cuda=True))


def _names(rec):
    out = [c[0] if c[0] != "blocks" else ("blocks", c[2]["blocks"]) for c in rec.calls]
    rec.calls.clear()
    return out


def test_call_sequence_of_a_schedule_run(fake):
    tr, rec, f = fake.tr, fake.rec, fake.f
    st = tr.step_cache_state(measure=False, mode=FB)
    assert st.mode == FB and not st.measure
    tr.step_cache_begin(st, fake.x)
    calls = list(rec.calls)
    assert _names(rec) == ["gemm", "gemm", ("blocks", (0, 1))]           # both embedders into the stream, then block 0: no measure
    assert calls[0][1][1] == "x_embedder.weight" and calls[0][2]["out"] is f.h
    assert calls[1][1][1] == "context_embedder.weight" and calls[1][2]["out"] is f.cx
    with pytest.raises(RuntimeError, match="no residual"):
        tr.step_cache_end(st, compute=False)
    rec.calls.clear()
    tr.step_cache_begin(st, fake.x)
    rec.calls.clear()
    assert tr.step_cache_end(st, compute=True) == "sample"
    calls = list(rec.calls)
    assert _names(rec) == [("blocks", (1, 3)), "residual_save", "head"]
    assert calls[1][1][0] is f.h and calls[1][1][1] is st.h0 and calls[1][1][2] is st.r     # tail = h_final - h1 (the kept copy)
    assert st.block_passes == 1 and st.have_residual
    # a skipped step: block 0 still runs, then h = h1 + tail in place on the stream and the head
    tr.step_cache_begin(st, fake.x)
    assert _names(rec) == ["gemm", "gemm", ("blocks", (0, 1))]
    assert tr.step_cache_end(st, compute=False) == "sample"
    calls = list(rec.calls)
    assert _names(rec) == ["residual_apply", "head"]
    assert calls[0][1][0] is f.h and calls[0][1][1] is st.r and calls[0][2]["out"] is f.h
    assert st.block_passes == 1
    with pytest.raises(RuntimeError, match="step_cache_begin"):
        tr.step_cache_end(st, compute=True)


def test_call_sequence_of_an_adaptive_run(fake):
    tr, rec, f = fake.tr, fake.rec, fake.f
    st = tr.step_cache_state(measure=True, mode=FB)
    tr.step_cache_begin(st, fake.x)
    calls = list(rec.calls)
    # step 0: nothing to compare with -- r1 alone
    assert _names(rec) == ["absdiff_ws", "gemm", "gemm", ("blocks", (0, 1)), "residual_save"]
    cur0 = st.cur
    assert calls[4][1][0] is f.h and calls[4][1][1] is st.h0 and calls[4][1][2] is cur0
    tr.step_cache_end(st, compute=True)
    assert _names(rec) == [("blocks", (1, 3)), "residual_save", "head"]
    assert st.prev is cur0 and st.cur is not cur0                        # this step's r1 is the reference now
    # step 1: the fused measure on the stream's image rows, r1 into the other buffer
    tr.step_cache_begin(st, fake.x)
    calls = list(rec.calls)
    assert _names(rec) == ["gemm", "gemm", ("blocks", (0, 1)), "residual_absdiff_sums"]
    name, a, k = calls[3]
    assert a[0] is f.h and a[1] is st.h0 and a[2] is cur0 and k["r_out"] is st.cur and k["out"] is st.sums and k["ws"] is st.absdiff_ws
    tr.step_cache_end(st, compute=False)
    assert _names(rec) == ["residual_apply", "head"]
    assert st.prev is cur0                                               # a skipped step leaves the reference where it is
    tr.step_cache_begin(st, fake.x)
    assert rec.calls[3][1][2] is cur0
    rec.calls.clear()
    cur2 = st.cur
    tr.step_cache_end(st, compute=True)
    assert st.prev is cur2 and st.block_passes == 2


def test_default_mode_calls_are_unchanged(fake):
    tr, rec, f = fake.tr, fake.rec, fake.f
    st = tr.step_cache_state(measure=True)
    assert st.mode == "input"
    tr.step_cache_begin(st, fake.x)
    assert _names(rec) == ["absdiff_ws", "gemm", "ln_modulate"]          # x_embedder into h0, the modulated input; no block
    tr.step_cache_end(st, compute=True)
    calls = list(rec.calls)
    assert _names(rec) == ["gemm", ("blocks", None), "residual_save", "head"]     # context_embedder, ALL blocks: no range
    assert calls[2][1][0] is f.h and calls[2][1][1] is st.h0 and calls[2][1][2] is st.r
    tr.step_cache_begin(st, fake.x)
    assert _names(rec) == ["gemm", "ln_modulate", "absdiff_sums"]
    tr.step_cache_end(st, compute=False)
    calls = list(rec.calls)
    assert _names(rec) == ["residual_apply", "head"]
    assert calls[0][1][0] is st.h0 and calls[0][2]["out"] is f.h


def test_a_model_of_one_block_is_refused(fake):
    fake.pk.single = []
    with pytest.raises(ValueError, match="nothing to skip"):
        fake.tr.step_cache_state(measure=False, mode=FB)
    fake.tr.step_cache_state(measure=False)
    with pytest.raises(ValueError, match="mode"):
        fake.tr.step_cache_state(measure=False, mode="second_block")


def test_block_ranges():
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel as T
    pk = SimpleNamespace(double=[0] * 3, single=[0] * 4)
    R = T._block_ranges
    assert R(pk, None) == (range(0, 3), range(0, 4))
    assert R(pk, (0, 1)) == (range(0, 1), range(0, 0)) and R(pk, (1, 7)) == (range(1, 3), range(0, 4))
    assert R(pk, (3, 4)) == (range(3, 3), range(0, 1)) and R(pk, (4, 7)) == (range(3, 3), range(1, 4))
    none = SimpleNamespace(double=[], single=[0] * 2)
    assert R(none, (0, 1)) == (range(0, 0), range(0, 1)) and R(none, (1, 2)) == (range(0, 0), range(1, 2))
    for bad in ((-1, 2), (2, 1), (0, 8)):
        with pytest.raises(ValueError):
            R(pk, bad)
