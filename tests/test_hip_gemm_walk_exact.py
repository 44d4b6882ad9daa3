"""Exact tests of the tile walk of the large-tile bf16 GEMMs -- gemm_walk_kernel, store_tile<..., WALK> and launch_walk of
csrc/gemm_pingpong_bf16.hip -- under workgroup caps: all 28 instantiations <EPI, MIX, M16> against the fp64 integer product.

tests/test_hip_gemm_walk.py holds the walk to the one-workgroup-per-tile launch on random data.  Here the reference is
`gemm_large_cases.want()`, the data that of tests/test_hip_gemm_large_exact.py (integer operands, |v| <= 255 at every bf16
rounding point, NaN behind column K of A and W, per-problem W / bias / gate offset, power-of-two gates; section "W" of
tests/gemm_large_cases.py, held to those rules on the CPU by tests/test_gemm_large_host.py), and the assertion EQUALITY over
the whole sentinel-filled buffer around C; GELU / SiLU within 1 bf16 ulp, the bound tests/test_hip_gemm_small.py derives.
NaN behind K matters to the walk in particular: past a tile's last K-tile it issues clamped requests that are never read, and
a workgroup's last tile requests its own K-tile 0 once more.

Every launch runs under `ops.gemm_set_walk("walk", cap)` for each cap of `gemm_large_cases.walk_caps(tiles)`: 1 (one workgroup
walks the whole launch), 2, 3 and tiles - 1 (workgroup 0 alone is handed a second tile), each only where tiles > cap -- the
launcher declines silently otherwise, and tests/test_gemm_large_host.py asserts that no (launch, cap) here is such a case.
`ops.gemm_last_variant()` is asserted after every launch (the walk reports the form it walks, 256 / 384).  Mixed grids: the
place order is big tiles first, so a workgroup changes shape at most once, big -> small (the workgroup barrier of `hand_over`);
every mixed (launch, cap) here has such a hand-over (test_gemm_large_host.py::test_shape_changes_of_the_mixed_walk).

Parts (the letters of test_hip_gemm_large_exact.py's sections, whose tables they reuse), and which instantiation each test runs
(EPI, MIX = form 384, M16 = mfma 16; a mixed launch runs both K loops, walk_run8 and walk_run9, of its instantiation):
  A  K pipeline, 1 .. 5 K-tiles x row / column edges, and K = 3072, 6144, 6400            <none, form, mfma>
  B  all ten epilogues, the in-place ones included                none_bias, none -> <none>, scale_* -> <scale>, res* -> <res>,
                                                                  gelu -> <GELU>, silu -> <SiLU>, gate_res* -> <gate_res>, each x form x mfma
  C  batch boundaries inside a tile, row slices of joint buffers and dense 3-D operands   <none | res | gate_res, 256, mfma>
  D  grouped launches of M = 1, 300, 2100, 257 (256) and of M = 300, 520, 257 (384)       <none | gate_res, form, mfma>
  H  the fused QKV epilogue, text + image grouped, token offset                           <QKV, form, mfma>
  B (6 EPI) and H (QKV) x 2 forms x 2 MFMA shapes are the 28.
  declines: a cap of at least the tile count, and the plan's tile_per_wg: same form reported, same values.

The one recorded run (MI355X, 256 CUs, `pytest -m gpu tests/test_hip_gemm_walk_exact.py -s`): 76 tests, all passed, 5.3 s for the
whole file, process start included; the slowest test is A [256-16] at 0.47 s (the first to upload its problems), every other
one below 0.4 s.
  Launch forms seen (`[form]` lines; the forced form after every launch of every test):
    A  256 and 384 on both MFMA shapes: 110 / 120 launches at K = 64 .. 320, 12 each at K = 3072, 6144, 6400
    B  256 (12 launches) and 384 (8) for each of the ten epilogues on both MFMA shapes
    C  256, both layouts, both MFMA shapes: 100 launches each            D  256 (12 launches) and 384 (8), both epilogues, both shapes
    H  256 with caps 1, 2, 3, 11 (N = 3 H 128) / 1, 2, 3, 7 (N = 2 H 128), 384 with caps 1, 2, 3, 19 / 1, 2, 3, 11
    declines  256 at cap >= 6 tiles, 384 at cap >= 10 tiles, and under tile_per_wg
  GELU / SiLU, exact share and largest distance (`[ulp]` lines; the assertion is max <= 1 ulp, not these shares):
    B  GELU  form 256 / 384, either MFMA shape: 1.000000, max 0 ulp  (2368512 / 1843200 elements)
       SiLU  form 256 / 384, either MFMA shape: 0.999939 / 0.999922, max 1 ulp
  Control run, on a copy of the library in which `hand_over` loads the bias quads of the NEXT tile's columns (nx.n0 for w.n0:
  other values, the same addresses' range): 56 of the 76 tests fail -- every test of A, C, D and H and the seven bias-carrying
  epilogues of B -- and 20 pass: `none` and the two scaled epilogues of B (no bias) and the eight tests in which the launcher
  declines.  Both tests of tests/test_hip_mmdit_walk.py and 29 of the 34 of tests/test_hip_gemm_walk.py fail on that copy too.
  So the compared bytes come from gemm_walk_kernel, which `gemm_last_variant()` cannot show.
"""
import contextlib
import functools

import pytest
import torch

import gemm_large_cases as L
import gemm_small_ref as R
from gemm_small_ref import BF, GUARD_COLS, SENTINEL
from test_hip_gemm_large_exact import _a3, _dev, _h_fused_qkv, _launch, _run, _seen, forced
from test_hip_gemm_small import _all_shapes, _UlpStats

pytestmark = pytest.mark.gpu

FORM_MFMA = [(f, m) for f in L.W_FORMS for m in L.MFMA_OF[f]]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def walking(ops, cap, form="walk"):
    """The tile walk's launch control around one launch, restored afterwards."""
    ops.gemm_set_walk(form, cap)
    try:
        yield
    finally:
        ops.gemm_set_walk("default")


@functools.lru_cache(maxsize=None)
def _caps(form, Ms, N):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = sum(L.walk_grid(form, Ms, N, cus))
    caps = L.walk_caps(tiles)
    assert all(tiles > cap for cap in caps)
    return caps


# ---- A: the K pipeline ---------------------------------------------------------------------------------------------------------

def _a_run(ops, form, mfma, shapes, what):
    def run(M, N, K, cap):
        P = L.case_problem(M, N, K, 1, L.W_EPI_A)
        buf, idx, _ = R.guarded(M, N, device="cuda")
        with walking(ops, cap):
            _run(ops, L.W_EPI_A, P, _dev(P).a, buf, idx, form, f"W-A form {form} mfma {mfma} M {M} N {N} K {K} cap {cap}")

    launches = [(M, N, K, cap) for M, N, K in shapes for cap in _caps(form, (M,), N)]
    with forced(ops, form, mfma):
        _all_shapes(run, launches)
    _seen("W-A", f"{what} forced {form} mfma {mfma}, {len(launches)} launches", form)


@pytest.mark.parametrize("form,mfma", FORM_MFMA)
def test_w_a_k_tile_counts(ops, form, mfma):
    """K = 64 .. 320, one to five K-tiles: the prefetched K-tile 0 is the tile's only one, one trip, the odd exit, two trips, the
    odd exit after two; M around the row tile's edge, bias, bf16 out.  Form 256: 22 launches per K (the nine shapes of more than
    one tile under their caps), 110 in all; form 384: 24 per K, 120 in all."""
    _a_run(ops, form, mfma, [(M, N, K) for K in L.A_KS for M, N in L.A_SHAPES[form]], "K tiles")


@pytest.mark.parametrize("form,mfma", FORM_MFMA)
def test_w_a_long_k(ops, form, mfma):
    """K = 3072, 6144, 6400 (48, 96, 100 K-tiles) at 513 x 768 (form 256: 9 tiles) / 513 x 1024 (form 384: 3 + 18 tiles), sparse
    operands: 12 launches (caps 1, 2, 3, tiles - 1)."""
    M, N = L.W_LONG_SHAPES[form]
    _a_run(ops, form, mfma, [(M, N, K) for K in L.W_LONG_KS], "long K")


# ---- B: every epilogue -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,mfma", FORM_MFMA)
@pytest.mark.parametrize("epi", L.EPILOGUES)
def test_w_b_every_epilogue(ops, epi, form, mfma):
    """K = 64, 192.  Form 256: 300 x 768 (6 tiles, caps 1, 2, 3, 5) and 513 x 256 (3 tiles, caps 1, 2): 12 launches; form 384:
    300 x 768 (2 + 8 tiles, caps 1, 2, 3, 9): 8 launches.  The in-place forms start from the residual in C."""
    stats = _UlpStats()

    def run(M, N, K, cap):
        P = L.case_problem(M, N, K, 1, epi)
        D = _dev(P)
        gated = epi in L.GATED
        buf, idx, _ = R.guarded((1, M) if gated else M, N, device="cuda")
        with walking(ops, cap):
            _run(ops, epi, P, _a3(D, 1, M) if gated else D.a, buf, idx, form,
                 f"W-B {epi} form {form} mfma {mfma} M {M} N {N} K {K} cap {cap}", rows_per_batch=M, stats=stats)

    launches = [(M, N, K, cap) for M, N in L.B_SHAPES[form] for K in L.B_KS for cap in _caps(form, (M,), N)]
    try:
        with forced(ops, form, mfma):
            _all_shapes(run, launches)
    finally:
        if stats.n:
            print(stats.line(f"W-B {epi} form {form} mfma {mfma}, {len(launches)} launches"), flush=True)
    _seen("W-B", f"{epi} forced {form} mfma {mfma}, {len(launches)} launches", form)


# ---- C: batch boundaries inside a tile ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["row_slices_of_joint_buffers", "dense_3d"])
@pytest.mark.parametrize("mfma", L.MFMA_OF[L.W_C_FORM])
def test_w_c_batch_boundaries_inside_a_tile(ops, mfma, layout):
    """Section C's (B, R) -- rows per batch 1 .. 257 -- and epilogues at N = 512, form 256: 2, 4 or 6 tiles, so consecutive tiles
    of a workgroup lie in other batches' rows.  25 (launch shape, cap) pairs x 4 epilogues = 100 launches.  row_slices: nothing
    outside the written window of C changes, and the residual's buffer is not written."""
    form, N, K, S_txt = L.W_C_FORM, L.C_N, L.C_K, L.C_S_TXT

    def run(B, Rr, epi, cap):
        P = L.case_problem(B * Rr, N, K, B, epi)
        D = _dev(P)
        what = f"W-C {layout} {epi} form {form} mfma {mfma} B {B} R {Rr} cap {cap}"
        with walking(ops, cap):
            if layout == "dense_3d":
                buf, idx, c = R.guarded(B * Rr, N, device="cuda")
                _launch(ops, epi, D, _a3(D, B, Rr), c.view(B, Rr, N))
            else:
                S = S_txt + Rr
                xd = torch.full((B, S, K + L.PAD), float("nan"), dtype=BF, device="cuda")
                xd[:, S_txt:, :K] = _a3(D, B, Rr)
                rd = torch.full((B, S, N + 16), 99.0, dtype=BF, device="cuda")
                rd[:, S_txt:, :N] = D.res.view(B, Rr, N)
                buf = torch.full((B, S + R.GUARD_ROWS, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
                idx = (slice(None), slice(S_txt, S), slice(GUARD_COLS, GUARD_COLS + N))
                _launch(ops, epi, D, xd[:, S_txt:, :K], buf[idx], res=rd[:, S_txt:, :N])
        got = ops.gemm_last_variant()
        assert got == form, f"{what}: launch form {got}, expected {form}"
        R.check_guarded(buf, idx, L.want(epi, P, Rr)[0], what)
        if layout != "dense_3d":
            assert (rd[:, :S_txt] == 99).all() and (rd[:, :, N:] == 99).all(), f"{what}: the residual's buffer was written"

    launches = [(B, Rr, epi, cap) for B, Rr in L.C_BR for epi in L.C_EPILOGUES for cap in _caps(form, (B * Rr,), N)]
    with forced(ops, form, mfma):
        _all_shapes(run, launches)
    _seen("W-C", f"{layout} forced {form} mfma {mfma}, {len(launches)} launches", form)


# ---- D: grouped launches -----------------------------------------------------------------------------------------------------------------

def _d_run(ops, form, mfma, epi, brs, N, K, group_ms):
    Ms = tuple(B * Rr for B, Rr in brs)
    launches = 0
    for group_m in group_ms:
        for cap in _caps(form, Ms, N):
            probs, checks = [], []
            for B, Rr in brs:
                P = L.case_problem(B * Rr, N, K, B, epi)
                D = _dev(P)
                buf, idx, c = R.guarded((B, Rr), N, device="cuda")
                pr = dict(a=_a3(D, B, Rr), w=D.w, bias=D.bias, out=c)
                if epi == "gate_res":
                    pr.update(res=D.res.view(B, Rr, N), gate=D.gate_wide[:, N:2 * N])
                probs.append(pr)
                checks.append((buf, idx, L.want(epi, P, Rr)[0],
                               f"W-D {epi} form {form} mfma {mfma} group_m {group_m} cap {cap} M {B * Rr} of {Ms}"))
            with forced(ops, form, mfma, group_m=group_m), walking(ops, cap):
                ops.gemm_grouped(probs, epilogue=ops.FK_EPI_GATE_RES if epi == "gate_res" else ops.FK_EPI_NONE)
                assert ops.gemm_last_variant() == form
            launches += 1
            _all_shapes(lambda *ch: R.check_guarded(*ch), checks)
    _seen("W-D", f"{epi} M {Ms} forced {form} mfma {mfma}, {launches} launches", form)


@pytest.mark.parametrize("epi", L.D_EPILOGUES)
@pytest.mark.parametrize("mfma", L.MFMA_OF[L.W_D_FORM])
def test_w_d_grouped_launches(ops, mfma, epi):
    """M = 1, 300, 2100 and 257 in one call (28 tiles of 256 x 256 at N = 512), each problem with its own W, bias and gate, grouping
    depths 0, 1, 3 x caps 1, 2, 3, 27: 12 launches.  Consecutive tiles of a workgroup belong to different problems."""
    _d_run(ops, L.W_D_FORM, mfma, epi, L.D_BR, L.D_N, L.D_K, L.D_GROUP_M)


@pytest.mark.parametrize("epi", L.D_EPILOGUES)
@pytest.mark.parametrize("mfma", L.MFMA_OF[384])
def test_w_d_grouped_launch_on_the_mixed_grid(ops, mfma, epi):
    """M = 300, 520 and 257 (2 + 3 + 2 ragged row tiles) at N = 768 on the mixed form: 7 big + 28 small tiles over three problems,
    grouping depths 0, 2 x caps 1, 2, 3, 34: 8 launches."""
    _d_run(ops, 384, mfma, epi, L.W_GM_BR, L.W_GM_N, L.W_GM_K, L.W_GM_GROUP_M)


# ---- H: the fused QKV epilogue ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("thirds", L.W_H_THIRDS, ids=["q_k_v", "q_k"])
@pytest.mark.parametrize("form,mfma", FORM_MFMA)
def test_w_h_fused_qkv_epilogue(ops, form, mfma, thirds):
    """Section H's case -- H = 2, B = 2, image rows of a batch (280) ending inside a tile, text + image grouped, token offset 70 --
    with the fused launch under each cap (form 256: 12 / 8 tiles, form 384: 20 / 12; 4 launches) against the unfused projection,
    launched one workgroup per tile, followed by fk_qkv_post_bf16: q, k and the v third of C bit for bit."""
    Ms, Ns = L.w_h_problems()
    caps = _caps(form, Ms, Ns[L.W_H_THIRDS.index(thirds)])

    def launch_under(cap):
        ctx = functools.partial(walking, ops, cap)
        ctx.what = f"W-H N = {thirds} H 128 form {form} mfma {mfma} cap {cap}: "
        return ctx

    _h_fused_qkv(ops, form, mfma, thirds, plain_launch=functools.partial(walking, ops, 0, "tile_per_wg"),
                 fused_launches=[launch_under(cap) for cap in caps])
    _seen("W-H", f"N = {thirds} H 128 forced {form} mfma {mfma}, caps {caps}", form)


# ---- where the launcher declines ---------------------------------------------------------------------------------------------------------

DECLINE_EPILOGUES = ("none_bias", "res_inplace", "gate_res", "gelu")


@pytest.mark.parametrize("form,mfma", FORM_MFMA)
def test_a_cap_of_at_least_the_tile_count_keeps_one_workgroup_per_tile(ops, form, mfma):
    """"walk" with cap == tiles, tiles + 1 and 1000: the launcher's `tiles > Gw` rule declines silently -- the form reported is the
    forced one and the values are the expected ones.  300 x 768 x 192, four epilogues: 12 launches."""
    M, N, K = 300, 768, 192
    tiles = sum(L.walk_grid(form, (M,), N, torch.cuda.get_device_properties(0).multi_processor_count))

    def run(epi, cap):
        P = L.case_problem(M, N, K, 1, epi)
        D = _dev(P)
        gated = epi in L.GATED
        buf, idx, _ = R.guarded((1, M) if gated else M, N, device="cuda")
        with walking(ops, cap):
            _run(ops, epi, P, _a3(D, 1, M) if gated else D.a, buf, idx, form, f"declined {epi} form {form} mfma {mfma} cap {cap}",
                 rows_per_batch=M)

    with forced(ops, form, mfma):
        _all_shapes(run, [(epi, cap) for epi in DECLINE_EPILOGUES for cap in (tiles, tiles + 1, 1000)])
    _seen("declines", f"cap >= {tiles} tiles forced {form} mfma {mfma}", form)


@pytest.mark.parametrize("form,mfma", FORM_MFMA)
def test_tile_per_wg_keeps_one_workgroup_per_tile(ops, form, mfma):
    """The plan's tile_per_wg: the same form reported, the expected values.  300 x 768 x 192, four epilogues: 4 launches."""
    M, N, K = 300, 768, 192

    def run(epi):
        P = L.case_problem(M, N, K, 1, epi)
        D = _dev(P)
        gated = epi in L.GATED
        buf, idx, _ = R.guarded((1, M) if gated else M, N, device="cuda")
        with walking(ops, 0, "tile_per_wg"):
            _run(ops, epi, P, _a3(D, 1, M) if gated else D.a, buf, idx, form, f"tile_per_wg {epi} form {form} mfma {mfma}",
                 rows_per_batch=M)

    with forced(ops, form, mfma):
        _all_shapes(run, [(epi,) for epi in DECLINE_EPILOGUES])
    _seen("declines", f"tile_per_wg forced {form} mfma {mfma}", form)
