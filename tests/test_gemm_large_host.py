"""CPU checks of the reference side of tests/test_hip_gemm_large_exact.py: the data rules of tests/gemm_large_cases.py hold for
every case the GPU file builds (one shared `host_cases()` list), every forced launch form applies to its shapes, the
comparison functions see each planted mistake, the stream-K cases contain every move of `cut()`, and every (B, R) of the
batch-boundary section puts a boundary inside a tile.  Section W (tests/test_hip_gemm_walk_exact.py, the tile walk under
workgroup caps) goes through the same `host_cases()`; for it, too: every (launch, cap) has more tiles than workgroups, and the
mixed grid's place order, restated in gemm_large_cases.py, is that of csrc/gemm_tile_map.h."""
import pytest
import torch

import gemm_large_cases as L
import gemm_small_ref as R
from gemm_small_ref import BF, F32, F64

CASES = L.host_cases()


def test_the_case_list_covers_the_sections():
    assert {c[0] for c in CASES} == set("ABCDEFGW")
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


# ---- section W: the tile walk under caps ------------------------------------------------------------------------------------------

WALK = L.walk_launches()


def test_walk_caps():
    assert L.walk_caps(1) == [] and L.walk_caps(2) == [1] and L.walk_caps(3) == [1, 2] and L.walk_caps(4) == [1, 2, 3]
    assert L.walk_caps(9) == [1, 2, 3, 8] and L.walk_caps(28) == [1, 2, 3, 27]
    for tiles in range(2, 40):
        caps = L.walk_caps(tiles)
        assert 1 in caps and tiles - 1 in caps and len(set(caps)) == len(caps) and all(1 <= c < tiles for c in caps)
        assert {2, 3} & set(range(1, tiles)) <= set(caps)


def test_the_walk_tables_cover_their_parts():
    assert {c[0] for c in WALK} == set("ABCDH") and {c[1] for c in WALK} == set(L.W_FORMS)
    for form in L.W_FORMS:
        assert {c[4] for c in WALK if c[:2] == ("A", form)} == set(L.A_KS) | set(L.W_LONG_KS)
        assert {c[2][0] for c in WALK if c[:2] == ("A", form) and c[4] == 64} >= {257, 300, 513}      # ragged row tiles
        assert {(c[2][0], c[3]) for c in WALK if c[:2] == ("B", form)} == set(L.B_SHAPES[form])
    assert {c[6] for c in CASES if c[0] == "W" and c[3] in L.B_KS} >= set(L.EPILOGUES)
    assert {(c[4], c[5]) for c in CASES if c[0] == "W" and c[2] == L.C_N and c[3] == L.C_K and c[6] in L.GATED} == set(L.C_BR)
    assert all(c[6] == L.W_EPI_A for c in CASES if c[0] == "W" and c[3] in L.W_LONG_KS)
    # shapes: at most 2100 x 1024, the long-K ones 513 x 1024 x 6400 at most
    assert all(max(Ms) <= 2100 and N <= 1024 for _, _, Ms, N, _ in WALK)
    assert all(Ms[0] <= 513 for _, _, Ms, N, K in WALK if K > 320)


def test_every_walk_launch_has_more_tiles_than_its_cap():
    """The launcher walks only where tiles > cap; at tiles <= cap it silently keeps one workgroup per tile, and a GPU case there
    would pass without having run gemm_walk_kernel.  Every (launch, cap) of section W really walks, on any number of CUs."""
    pairs = 0
    for part, form, Ms, N, K in WALK:
        assert N % 256 == 0 and K % 64 == 0 and (len(Ms) > 1 or Ms[0] >= 192)
        assert form == 256 or L.mixed_big_cols(sum(-(-M // 256) for M in Ms), N) > 0, "the forced mixed form does not apply"
        for cus in (256, 304, 64):
            tiles = sum(L.walk_grid(form, Ms, N, cus))
            caps = L.walk_caps(tiles)
            assert tiles >= 2 and caps[0] == 1 and caps[-1] == tiles - 1
            assert all(tiles > cap >= 1 for cap in caps)
            pairs += cus == 256 and len(caps)
    assert pairs > 300
    # the hand-over patterns of the issue: one workgroup for the whole launch, tiles == cap + 1, and (the GPU file's extra
    # tests) a cap of at least the tile count, where the rule declines
    assert L.walk_grid(256, (513,), 768) == (9, 0) and L.walk_grid(384, (513,), 1024) == (3, 18)
    assert L.walk_grid(256, tuple(B * Rr for B, Rr in L.D_BR), L.D_N) == (28, 0)
    assert L.walk_grid(384, tuple(B * Rr for B, Rr in L.W_GM_BR), L.W_GM_N) == (7, 28)


def test_makespan_and_the_forced_mixed_split():
    """The launcher's plan restated: on 256 CUs every small grid of these tables ends with its one round of big tiles, so the
    first split with at least 8 small tiles is taken -- one column of 256 x 256 tiles (what tests/test_hip_gemm_walk.py's
    docstring states for 768 x 1024: 3 big + 18 small)."""
    assert L.makespan(3, 18, 0.61, 256) == 1.0 and L.makespan(0, 600, 0.61, 256) == pytest.approx(1.83)
    assert L.makespan(300, 0, 0.61, 256) == 2.0 and L.makespan(300, 300, 0.61, 256) == pytest.approx(2.22)
    for nbm in (2, 3, 4, 7):
        assert L.mixed_big_cols(nbm, 768) == 1 and L.mixed_big_cols(nbm, 1024) == 1
    assert L.mixed_big_cols(4, 512) == 1 and L.mixed_big_cols(3, 512) == 0 and L.mixed_big_cols(3, 1000) == 0
    cb = L.mixed_big_cols(10, 9216)      # the flagship fused-QKV grid: the plan's own mixed grid, more than one round of big tiles
    assert 1 < cb < 36 and L.walk_grid(384, (2560,), 9216) == (10 * cb, 20 * (36 - cb))


def test_mixed_place_order_is_the_tile_maps(tmp_path):
    """`mix_table` / `mix_place` against tm_fill_mix / tm_mix_place of csrc/gemm_tile_map.h, through tests/gemm_walk_main.cpp
    (--places), for every mixed launch of section W and the flagship fused-QKV grid."""
    import subprocess
    from test_gemm_tile_map import _compiler
    from test_gemm_walk_map import _build
    cxx = _compiler()
    assert cxx, "no host C++ compiler found (g++ / clang++ / $CXX)"
    exe = str(tmp_path / "gemm_walk_places")
    r = _build(cxx, exe, sanitize=False)
    assert r.returncode == 0, r.stderr[-4000:]
    grids = {(Ms, N) for _, form, Ms, N, _ in WALK if form == 384} | {((2560,), 9216), ((2048, 512), 1024)}
    for Ms, N in sorted(grids):
        cb = L.mixed_big_cols(sum(-(-M // 256) for M in Ms), N)
        for group_m in (1, 8):
            run = subprocess.run([exe, "--places", str(N), str(cb), str(group_m), *map(str, Ms)], capture_output=True, text=True, timeout=60)
            assert run.returncode == 0, run.stdout + run.stderr
            lines = [tuple(map(int, ln.split())) for ln in run.stdout.split("\n") if ln]
            tb, ts = L.walk_grid(384, Ms, N)
            assert lines[0] == (tb, ts) and len(lines) == 1 + tb + ts
            table = L.mix_table(tb, ts)
            assert [(int(s), t) for s, t in (L.mix_place(table, b) for b in range(tb + ts))] == lines[1:], f"Ms {Ms} N {N}"


def test_shape_changes_of_the_mixed_walk():
    """How many hand-overs of section W change the tile shape (the workgroup barrier in `hand_over`).

    The mixed grid's place order is big tiles first: place b = xcd + 8 idx is big iff idx < big_cnt[xcd], and big_cnt falls with
    the XCD (tb / 8 + (xcd < tb % 8)), so no place behind a small tile names a big one (tests/gemm_walk_main.cpp checks exactly
    this for every grid of its sweep).  A workgroup takes its places g, g + G, ... in rising order, whatever G is.  So NO grid
    permits a small -> big hand-over, and a workgroup's list changes shape at most ONCE: "alternating" lists do not exist, the
    barrier is reached by big -> small hand-overs alone.  Asserted: that bound for every (launch, cap); that EVERY mixed
    (launch, cap) of section W has at least one such hand-over (workgroup 0 starts big and, tiles > cap, ends small), so every
    mixed launch of the GPU file passes the barrier; and that the tables reach several of them in one launch, in several
    workgroups, behind one, two and three big tiles of the same workgroup."""
    mixed = [(part, Ms, N, K) for part, form, Ms, N, K in WALK if form == 384]
    assert len(mixed) >= 30
    behind = set()
    for part, Ms, N, K in mixed:
        tb, ts = L.walk_grid(384, Ms, N)
        for cap in L.walk_caps(tb + ts):
            most, to_small, to_big = L.shape_changes(tb, ts, cap)
            assert most == 1 and to_big == 0 and 1 <= to_small <= min(cap, tb)
            assert to_small == min(cap, tb) or cap == tb + ts - 1       # every workgroup that starts big ends small
            lists = L.walk_shapes(tb, ts, cap)
            assert sum(map(len, lists)) == tb + ts and lists[0][0] is False and lists[0][-1] is True
            behind |= {ls.index(True) for ls in lists if not ls[0] and ls[-1]}
    assert behind >= {1, 2, 3}, behind
    for tb, ts, cap in ((260, 200, 256), (260, 200, 7), (9, 24, 5), (17, 8, 3), (3, 18, 20)):      # any grid, any G
        most, to_small, to_big = L.shape_changes(tb, ts, cap)
        assert most <= 1 and to_big == 0
    for part, form, Ms, N, K in WALK:
        if form == 256:
            assert all(L.shape_changes(*L.walk_grid(256, Ms, N), cap) == (0, 0, 0) for cap in L.walk_caps(sum(L.walk_grid(256, Ms, N))))


def test_the_problems_of_the_mixed_grouped_launch_share_nothing():
    for epi in L.D_EPILOGUES:
        ps = [L.case_problem(B * Rr, L.W_GM_N, L.W_GM_K, B, epi) for B, Rr in L.W_GM_BR]
        for i, p in enumerate(ps):
            for q in ps[i + 1:]:
                assert (p.bias != q.bias).float().mean() > 0.5 and not (p.w == q.w).all(dim=1).any()
                nb = min(p.B, q.B)
                assert (p.gate[:nb] != q.gate[:nb]).all(), "two problems of the group share a gate value at (batch, column)"
    assert len({L.gate_seed(B * Rr, L.W_GM_K) % len(L.GATE_VALUES) for B, Rr in L.W_GM_BR}) == len(L.W_GM_BR)
    assert len({-(-B * Rr // 256) for B, Rr in L.W_GM_BR}) > 1 and all((B * Rr) % 256 for B, Rr in L.W_GM_BR)      # ragged M
