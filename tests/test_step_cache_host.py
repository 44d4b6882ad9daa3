"""CPU: the step cache's host logic (gpt_image_edit_amd/step_cache.py) -- the adaptive rule, schedule validation, the
polynomial's order, the command-line forms."""
import math

import pytest

from gpt_image_edit_amd.step_cache import StepCache, from_args, parse_float_list, parse_int_list


def _run(sc, rels):
    """Drive a cache through n = len(rels) + 1 steps with hand-made measures (sums = (rel, 1))."""
    n = len(rels) + 1
    sc.begin(n)
    return [sc.step(i, None if i == 0 else (rels[i - 1], 1.0)) for i in range(n)]


def test_first_and_last_step_always_compute():
    sc = StepCache(threshold=1e9)
    assert sc.decide(0.0, 123.0, 0, 5) == (True, 0.0)
    assert sc.decide(0.0, 0.0, 4, 5) == (True, 0.0)
    assert sc.decide(0.0, 0.0, 3, 5) == (False, 0.0)
    assert _run(sc, [0.0] * 4) == [True, False, False, False, True]
    assert _run(StepCache(threshold=1e9), []) == [True]             # one step: it is both


def test_accumulate_and_reset_on_a_hand_made_list():
    sc = StepCache(threshold=0.5)
    rels = [0.2, 0.2, 0.2, 0.1, 0.5, 0.3, 0.1]
    #  acc: .2   .4   .6*  .1   .6*  .3   last
    assert _run(sc, rels) == [True, False, False, True, False, True, False, True]
    assert sc.computed_steps == [0, 3, 5, 7] and sc.rel_l1 == rels
    # decide is pure: same arguments, same answer, no state touched
    before = (list(sc.computed_steps), list(sc.rel_l1))
    assert sc.decide(0.4, 0.2, 3, 8) == (True, 0.0) and sc.decide(0.4, 0.2, 3, 8) == (True, 0.0)
    compute, acc = sc.decide(0.2, 0.2, 2, 8)
    assert compute is False and acc == pytest.approx(0.4)
    assert (sc.computed_steps, sc.rel_l1) == before
    # a replay of the recorded decisions
    rp = StepCache(schedule=sc.computed_steps)
    assert _run(rp, rels) == [True, False, False, True, False, True, False, True] and rp.rel_l1 == []


def test_zero_denominator_computes():
    assert StepCache.rel_of((0.0, 0.0)) == math.inf and StepCache.rel_of((3.0, 0.0)) == math.inf
    assert StepCache.rel_of((1.0, 4.0)) == 0.25
    sc = StepCache(threshold=1e30)
    sc.begin(4)
    assert [sc.step(0), sc.step(1, (0.0, 0.0)), sc.step(2, (1.0, 1.0)), sc.step(3, (1.0, 1.0))] == [True, True, False, True]
    assert StepCache(threshold=math.inf).decide(0.0, math.inf, 1, 4) == (True, 0.0)


def test_threshold_zero_and_inf():
    assert _run(StepCache(threshold=0), [0.0, 0.3, 0.0, 0.1]) == [True] * 5
    sc = StepCache(threshold=math.inf)
    assert _run(sc, [5.0, 1e30, 7.0, 2.0]) == [True, False, False, False, True] and sc.computed_steps == [0, 4]


def test_polynomial_is_lowest_order_first():
    assert StepCache.polyval((1.0, 2.0, 3.0), 2.0) == 1.0 + 2.0 * 2.0 + 3.0 * 4.0
    assert StepCache.polyval((0.0, 1.0), 0.37) == 0.37               # the default is the identity
    assert StepCache(threshold=1.0).coefficients == (0.0, 1.0)
    sc = StepCache(threshold=1.0, coefficients=(0.5, 0.0, 2.0))      # 0.5 + 2 x^2
    compute, acc = sc.decide(0.0, 0.1, 1, 9)
    assert compute is False and acc == pytest.approx(0.52)
    assert sc.decide(acc, 0.1, 2, 9) == (True, 0.0)                  # 1.04 >= 1
    with pytest.raises(ValueError):
        StepCache(threshold=1.0, coefficients=())


def test_exactly_one_mode():
    with pytest.raises(ValueError, match="exactly one"):
        StepCache()
    with pytest.raises(ValueError, match="exactly one"):
        StepCache(threshold=0.1, schedule=[0])
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            StepCache(threshold=bad)


def test_schedule_validation():
    for bad in ([], [1, 2], [0, 2, 2], [0, 3, 1], [0, -1], [0, 1.5]):
        with pytest.raises(ValueError, match="schedule"):
            StepCache(schedule=bad)
    sc = StepCache(schedule=range(4))
    assert sc.schedule == (0, 1, 2, 3) and not sc.adaptive
    sc.validate(4)
    with pytest.raises(ValueError, match="schedule"):
        sc.validate(3)                                               # step 3 of a 3-step call
    with pytest.raises(ValueError):
        sc.validate(0)
    StepCache(threshold=0.3).validate(1)


def test_command_line_forms():
    assert parse_int_list("0,1, 3") == [0, 1, 3] and parse_float_list("0.5,-1e-3") == [0.5, -1e-3]
    assert from_args() is None
    sc = from_args(threshold=0.25, coefficients="0.1,2")
    assert sc.adaptive and sc.threshold == 0.25 and sc.coefficients == (0.1, 2.0)
    assert from_args(schedule="0,2,5").schedule == (0, 2, 5)
    with pytest.raises(ValueError):
        from_args(threshold=0.1, schedule="0")
    with pytest.raises(ValueError):
        from_args(coefficients="0,1")
