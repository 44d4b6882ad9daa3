"""CPU checks of tests/lora_ref.py: an fp32 emulation of the merge kernel's arithmetic stays inside the derived bound at every
shape the GPU file uses, and each plausible mistake of the kernel or of the host around it falls outside it."""
import pytest
import torch

import lora_ref as R


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_emulation_is_inside_the_bound(N, K, r):
    base, terms = R.data(N, K, (r,), seed=N + K + r)
    assert R.check("emulated", R.emulate(base, terms), base, terms) <= 1.0


def test_shapes_reach_every_rank_tile():
    """The merge kernel walks ceil(r / 32) = 1 .. 4 trips of its r_pad loop: the GPU file's shape list must reach each count,
    the first and the last rank of the one that went unvisited longest (65, 96) by name."""
    ranks = [s[-1] for s in R.SHAPES]
    assert all(1 <= r <= R.MAX_RANK for r in ranks)
    assert {-(-r // R.RANK_TILE) for r in ranks} == set(range(1, R.MAX_RANK // R.RANK_TILE + 1)) == {1, 2, 3, 4}
    assert {65, 96} <= set(ranks)


@pytest.mark.parametrize("n_terms", [1, 2, 3, 4])
def test_emulation_with_mixed_ranks_is_inside_the_bound(n_terms):
    base, terms = R.data(65, 136, R.MIXED_RANKS[:n_terms], seed=n_terms)
    assert R.check("emulated mixed", R.emulate(base, terms), base, terms) <= 1.0


@pytest.mark.parametrize("N,K", [(65, 136), (128, 64)])
def test_emulation_with_a_rank_96_term_among_others_is_inside_the_bound(N, K):
    base, terms = R.data(N, K, R.MIXED_RANKS_96, seed=7 * 96)       # the data of the GPU file's case
    assert terms[1][2] < 0
    assert R.check("emulated mixed, 96", R.emulate(base, terms), base, terms) <= 1.0


def test_exact_cases_are_exact_in_any_order(ranks=R.MIXED_RANKS, N=65, K=136, seed=3):
    base, terms = R.exact_data(N, K, ranks, seed=seed)
    want = R.exact_merge(base, terms)
    assert torch.equal(R.emulate(base, terms), want)
    flipped = [(up.flip(1), down.flip(0), s) for up, down, s in terms]        # the rank summed in the opposite order
    assert torch.equal(R.emulate(base, flipped), want)
    assert not torch.equal(want, base)


@pytest.mark.parametrize("N,K,ranks", [(63, 72, (80,)), (130, 200, (96, 5, 65))])
def test_exact_cases_with_three_trips_are_exact_in_any_order(N, K, ranks):
    test_exact_cases_are_exact_in_any_order(ranks, N, K, seed=N + K)     # the data of the GPU file's cases


def _case():
    return R.data(64, 64, (8, 33), seed=11)


def test_a_dropped_rank_column_is_outside():
    base, terms = _case()
    up, down, s = terms[1]
    wrong = [terms[0], (up[:, :-1], down[:-1], s)]
    assert R.worst_ratio(R.emulate(base, wrong), base, terms) > 1.0


def test_a_dropped_term_is_outside():
    base, terms = _case()
    assert R.worst_ratio(R.emulate(base, terms[:1]), base, terms) > 1.0


def test_alpha_over_r_omitted_is_outside():
    base, terms = R.data(64, 64, (8,), seed=12)
    up, down, _ = terms[0]
    right = [(up, down, R.effective_scale(1.0, 1.0, 4.0, 8))]
    assert R.effective_scale(1.0, 1.0, 4.0, 8) == 0.5 and R.effective_scale(0.5, 0.5, 33.0, 33) == 0.25
    assert R.worst_ratio(R.emulate(base, right), base, right) <= 1.0
    assert R.worst_ratio(R.emulate(base, [(up, down, 1.0)]), base, right) > 1.0


def test_up_and_down_swapped_is_outside_for_a_square_case():
    base, terms = R.data(64, 64, (64,), seed=13)
    up, down, s = terms[0]
    assert R.worst_ratio(R.emulate(base, [(down, up, s)]), base, terms) > 1.0
    assert R.worst_ratio(R.emulate(base, [(down.t().contiguous(), up.t().contiguous(), s)]), base, terms) > 1.0


def test_one_wrong_row_is_outside():
    base, terms = _case()
    got = R.emulate(base, terms)
    assert R.worst_ratio(got, base, terms) <= 1.0
    got[17] = got[18]
    assert R.worst_ratio(got, base, terms) > 1.0


def test_the_bound_is_tight_enough_to_see_one_bf16_ulp():
    """Two bf16 neighbours cannot both lie inside the bound of an element that is not tiny: 2^-8 |ref| is one ulp at most."""
    base, terms = _case()
    got = R.emulate(base, terms)
    bits = got.view(torch.int16).clone()
    big = got.float().abs() > 0.01
    bits[big] += 2
    assert R.worst_ratio(bits.view(torch.bfloat16), base, terms) > 1.0
