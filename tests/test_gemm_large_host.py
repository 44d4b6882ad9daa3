"""CPU checks of the reference side of tests/test_hip_gemm_large_exact.py: the data rules of tests/gemm_large_cases.py hold for
every case the GPU file builds (one shared `host_cases()` list), every forced launch form applies to its shapes, the
comparison functions see each planted mistake, the stream-K cases contain every move of `cut()`, and every (B, R) of the
batch-boundary section puts a boundary inside a tile."""
import pytest
import torch

import gemm_large_cases as L
import gemm_small_ref as R
from gemm_small_ref import BF, F32, F64

CASES = L.host_cases()


def test_the_case_list_covers_the_sections():
    assert {c[0] for c in CASES} == set("ABCDEFG")
    assert {c[3] for c in CASES if c[0] == "A"} == {64, 128, 192, 256, 320}
    assert {c[6] for c in CASES if c[0] == "B"} == set(L.EPILOGUES)
    assert {(c[4], c[5]) for c in CASES if c[0] == "C" and c[6] in L.GATED} == set(L.C_BR)
    assert {c[3] // 128 for c in CASES if c[0] == "E" and c[6] == "f32"} == {2, 4, 6, 48, 50}       # K-tiles of a half
    assert L.persistent_grid(256) == (8092, 8448, 28, 289)
    assert max(c[1] * c[2] for c in CASES if c[0] != "G") <= 2100 * 768, "only section G has a large output"


def _mixed_applies(M, N):
    nbm = -(-M // 256)
    return N % 256 == 0 and N >= 512 and any(nbm * 2 * (N // 256 - cb) >= 8 for cb in range(1, N // 256))


def test_every_forced_form_applies_to_its_shapes():
    """fk_gemm2_launch's conditions restated: a forced form that does not apply falls back to another one, and the GPU file
    would then fail its `gemm_last_variant()` assertion -- a mistake in the tables, found here first."""
    for table in (L.A_SHAPES, L.B_SHAPES):
        for form, shapes in table.items():
            for M, N in shapes:
                assert M >= 192 and N % 8 == 0                       # below 192 rows ops.gemm takes the 128 x 128 kernel
                assert form == 128 or N % 256 == 0
                assert form != 384 or _mixed_applies(M, N)
    assert all(f == 128 or n % 256 == 0 for f in L.C_FORMS + L.D_FORMS for n in (L.C_N, L.D_N))
    assert all(B * Rr >= 192 for B, Rr in L.C_BR)
    for K in L.E_KS:
        assert (K // 64) % 4 == 0
    assert all(N % 256 == 0 for _, N in L.E_SHAPES) and {L.tiles256(M, N) for M, N in L.E_SHAPES} == {1, 4, 3}
    assert {L.tiles256(M, N) for M, N, _ in L.E_SEQUENCE} == {1, 2, 6} and len(L.E_SEQUENCE) == 20
    assert all((K // 64) % 4 == 0 and N % 256 == 0 and M >= 192 for M, N, K in L.E_SEQUENCE)
    for slots, M, N, K in L.streamk_cases():
        nk, t = K // 64, L.tiles256(M, N)
        assert N % 256 == 0 and M >= 192 and t * nk >= slots * (nk + 2 * L.SK_MIN_PART)
        assert (t - 1) * nk < slots * (nk + 2 * L.SK_MIN_PART), "not the smallest grid the forced form takes"
    for cus in (256, 304, 64):
        M, N, B, Rr = L.persistent_grid(cus)
        assert L.tiles256(M, N) >= 4 * cus and M % 256 != 0 and B * Rr == M and N % 256 == 0


@pytest.mark.parametrize("section,M,N,K,B,Rr,epi", CASES)
def test_data_rules(section, M, N, K, B, Rr, epi):
    P = L.case_problem(M, N, K, B, epi, big=section == "G")              # `expected`'s range and fp32 asserts run here
    # integer operands behind NaN padding, row strides K + 16
    for full, view, rows in ((P.a_full, P.a, M), (P.w_full, P.w, N)):
        assert full.shape == (rows, K + L.PAD) and view.shape == (rows, K) and view.stride(0) == K + L.PAD
        assert view.data_ptr() == full.data_ptr() and torch.isnan(full[:, K:].float()).all()
        assert torch.equal(view.float(), view.float().round()) and view.float().abs().max() <= 2
    if K > 320:
        assert P.a.float().abs().max() <= 1 and P.w.float().abs().max() <= 1 and (P.a == 0).float().mean() >= 0.6
    assert P.bias.float().abs().max() <= 4 and P.res.float().abs().max() <= 32
    if epi in L.GATED:
        assert P.tight and P.gate.shape == (B, N) and P.gate.stride(0) == 3 * N and L.gates_differ(P)
    if section == "G":
        # the one large problem: the rules of the sums on its first and its ragged last row tile and on the rows at every batch
        # boundary (about 470 of 8092 rows, each with its own gate row); the GPU test, which forms the whole product anyway,
        # asserts the bound that implies them for every element (gemm_large_cases.big_bound_holds)
        P, Rr = P.sample(L.sample_rows(M, B, Rr), Rr), 1
    assert P.y0.dtype == F64 and torch.equal(P.y0, P.y0.round())
    if epi == "f32":
        assert L.want(epi, P)[0].dtype == F32
        return
    if epi in L.ACTIVATIONS:
        w_act, y_act = P.act
        assert torch.isnan(w_act[:, K:].float()).all() and y_act.abs().max() <= 8
        assert L.want(epi, P)[1] == "ulp"
        return
    # bf16 equality cases: unit sensitivity at every rounding point, no case excused
    for v in L.rounding_points(epi, P, Rr):
        assert v.abs().max().item() <= 255 and L.unit_sensitive(v), f"max |v| = {v.abs().max().item()}"
    w, kind = L.want(epi, P, Rr)
    assert kind == "eq" and w.dtype == BF
    if epi in L.ALPHAS:
        assert L.scale_is_sensitive(P, epi)
    if epi in L.GATED:
        assert L.gate_is_exact(P, Rr)
    if section == "G":
        assert L.big_bound_holds(P, epi)


def test_the_problems_of_a_grouped_launch_share_nothing():
    """Section D: each problem has its own W, bias and gate, so a tile that reads them through the wrong problem index stores
    other bits: no two problems share a bias, a W row or -- at any batch index they both have -- a gate row."""
    for epi in L.D_EPILOGUES:
        ps = [L.case_problem(B * Rr, L.D_N, L.D_K, B, epi) for B, Rr in L.D_BR]
        for i, p in enumerate(ps):
            for q in ps[i + 1:]:
                assert not torch.equal(p.bias, q.bias) and (p.bias != q.bias).float().mean() > 0.5
                assert not (p.w == q.w).all(dim=1).any() and (p.w != q.w).float().mean() > 0.5
                nb = min(p.B, q.B)
                assert (p.gate[:nb] != q.gate[:nb]).all(), "two problems of the group share a gate value at (batch, column)"
    assert len({L.gate_seed(B * Rr, L.D_K) % len(L.GATE_VALUES) for B, Rr in L.D_BR}) == len(L.D_BR)


def test_unit_sensitivity_is_the_255_rule():
    """Every integer of |v| <= 255 is sensitive; from 256 on a bf16 step is 2 and a unit can round away (256 + 1 -> 256)."""
    one = lambda x: L.unit_sensitive(torch.tensor([x], dtype=F64))      # noqa: E731
    assert all(one(float(x)) for x in range(-255, 256))
    assert not one(256.0) and not one(-256.0) and not one(260.0) and not L.unit_sensitive(torch.tensor([3.0, 256.0], dtype=F64))
    assert L.unit_sensitive(torch.arange(-255.0, 256.0, dtype=F64))


# ---- the comparison functions see the planted mistakes ---------------------------------------------------------------------------

MB, MR, MN, MK = 4, 70, 512, 128                                         # a case of section C: batches end inside the first tile


def _gate_of_the_neighbouring_batch(d, finish):
    return R.epi_gate_res(d["y"], d["res"], d["gate"].roll(1, 0), MR)


def _k_tile(d):
    return d["a"].reshape(-1, MK)[:, :64].double() @ d["w"][:, :64].double().T


def _k_tile_summed_twice(d, finish):
    return finish(d["y"] + _k_tile(d))


def _k_tile_left_out(d, finish):
    return finish(d["y"] - _k_tile(d))


def _one_product_off_by_one(d, finish):
    y = d["y"].clone()
    y[MR + 5, 300] += d["unit"]
    return finish(y)


SUMS = [_k_tile_summed_twice, _k_tile_left_out, _one_product_off_by_one]


@pytest.fixture(scope="module")
def data():
    assert (MB, MR) in L.C_BR and (MN, MK) == (L.C_N, L.C_K)
    P = L.case_problem(MB * MR, MN, MK, MB, "gate_res")
    return dict(a=P.a.reshape(MB, MR, MK), w=P.w, bias=P.bias, res=P.res.view(MB, MR, MN), gate=P.gate, y=P.y, unit=1.0, P=P)


def _in_buffer(out):
    buf, idx, c = R.guarded(out.shape[0], out.shape[1], out.dtype)
    c.copy_(out)
    return buf, idx


def _ids(f):
    return f.__name__.strip("_")


@pytest.mark.parametrize("mistake", R.MISTAKES + [_gate_of_the_neighbouring_batch] + SUMS, ids=_ids)
def test_gated_equality_check_sees_each_mistake(data, mistake):
    finish = lambda y: R.epi_gate_res(y, data["res"], data["gate"], MR)      # noqa: E731
    want = finish(data["y"])
    R.check_guarded(*_in_buffer(want), want, "correct")
    with pytest.raises(AssertionError, match="differ"):
        R.check_guarded(*_in_buffer(mistake(data, finish)), want, mistake.__name__)


@pytest.mark.parametrize("finish", [R.epi_none, R.f32_none, lambda y: R.epi_res(y, L.problem(MB * MR, MN, MK, MB, True).res)],
                         ids=["none_bias", "f32", "res"])
@pytest.mark.parametrize("mistake", R.MISTAKES[:3] + SUMS, ids=_ids)
def test_plain_equality_checks_see_each_mistake(data, mistake, finish):
    want = finish(data["y"])
    R.check_guarded(*_in_buffer(want), want, "correct")
    with pytest.raises(AssertionError, match="differ"):
        R.check_guarded(*_in_buffer(mistake(data, finish)), want, mistake.__name__)


@pytest.mark.parametrize("name", L.ACTIVATIONS)
@pytest.mark.parametrize("mistake", R.MISTAKES[:3] + SUMS[:2], ids=_ids)
def test_ulp_check_sees_each_mistake(data, mistake, name):
    """On the activations' data (w scaled so that |y| <= 8).  One product off by one is left to the equality checks: behind a
    saturated activation a single unit can stay inside one bf16 step."""
    P = data["P"]
    w_act = P.act[0][:, :MK]
    d = dict(data, w=w_act, y=P.act[1])
    finish = R.epi_gelu if name == "gelu" else R.epi_silu
    want = finish(d["y"])
    assert R.check_ulp(*_in_buffer(want), want, "correct") == (1.0, 0)
    with pytest.raises(AssertionError, match="ulp"):
        R.check_ulp(*_in_buffer(mistake(d, finish)), want, mistake.__name__)


def test_nan_padding_reaches_the_output():
    """A kernel that reads 8 columns past K multiplies NaN into the sum: no comparison passes."""
    P = L.problem(300, 392, 64)
    y = P.a_full[:, :72].double() @ P.w_full[:, :72].double().T
    assert torch.isnan(y).all()


# ---- stream-K: the moves of cut() ----------------------------------------------------------------------------------------------

def test_streamk_cases_contain_every_move_of_cut():
    seen = set()
    for slots, M, N, K in L.streamk_cases():
        nk, t = K // 64, L.tiles256(M, N)
        pos, kinds = L.cut_kinds(t, nk, slots)
        assert len(pos) == slots - 1 and pos == sorted(pos) and 0 < pos[0] and pos[-1] < t * nk
        for j, (c, kind) in enumerate(zip(pos, kinds), start=1):
            raw = t * nk * j // slots
            assert {"boundary": c == raw and c % nk == 0, "in_place": c == raw and L.SK_MIN_PART <= c % nk <= nk - L.SK_MIN_PART,
                    "back": c == raw - raw % nk and 0 < raw % nk < L.SK_MIN_PART,
                    "forward": c == raw + nk - raw % nk and 0 < nk - raw % nk < L.SK_MIN_PART}[kind]
        inside = [c for c in pos if c % nk]
        assert len({c // nk for c in inside}) == len(inside), "a tile is cut twice"
        assert all(L.SK_MIN_PART <= c % nk <= nk - L.SK_MIN_PART for c in inside), "a part shorter than sk_min_part"
        assert all(b - a >= nk for a, b in zip([0] + pos, pos + [t * nk])), "a range shorter than one tile"
        seen |= set(kinds)
    assert seen == {"boundary", "back", "forward", "in_place"}, seen
    assert {s for s, *_ in L.streamk_cases()} == {2, 3, 4, 5} and {k for *_, k in L.streamk_cases()} == {2048, 3072, 6400}
    assert L.cut_kinds(4, 32, 2) == ([64], ["boundary"]) and L.cut_kinds(7, 48, 4) == ([96, 168, 240], ["forward", "in_place", "back"])


# ---- batch boundaries ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Rr", L.C_BR)
def test_a_batch_boundary_lies_inside_a_tile(B, Rr):
    inside = [b * Rr for b in range(1, B) if (b * Rr) % 256 != 0]
    assert inside, f"(B, R) = ({B}, {Rr}): every batch ends on a 256-row tile boundary"
    if Rr < 256:
        assert B * Rr > Rr, "the short-batch path needs a second batch"
    # joint buffers: the batch stride exceeds R x ld, so no operand of the slice run is flat
    S = L.C_S_TXT + Rr
    assert S * (L.C_K + L.PAD) > Rr * (L.C_K + L.PAD)
