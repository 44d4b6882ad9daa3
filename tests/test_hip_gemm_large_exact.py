"""Exact tests of the large-tile bf16 GEMMs -- gemm8 / gemm9 / gemm_mix / gemm10, the split-K pairs and the stream-K ranges of
csrc/gemm_pingpong_bf16.hip with store_tile of csrc/gemm_epilogue.h -- under every forced launch form, at their edges.

Data, and why the assertion is EQUALITY: tests/gemm_large_cases.py states the rules (integer operands whose every partial sum
fp32 holds exactly; |v| <= 255 at every bf16 rounding point, so a sum that is off by ONE changes the stored value; power-of-two
gates that differ between neighbouring batches and columns; NaN behind column K of A and W; C inside a sentinel-filled buffer),
tests/test_gemm_large_host.py asserts them on the CPU for every case built here.  GELU / SiLU: every element within 1 bf16 ulp
of the once-rounded fp64 value, none excluded -- the bound tests/test_hip_gemm_small.py derives for the same gelu_tanh_f / silu_f.
`ops.gemm_last_variant()` is asserted after every launch.

Sections
  A  K pipeline on the fp32 accumulators (out_fp32 = 2, with bias): 1 .. 5 K-tiles x row / column edges, forms 128 / 256 / 384 / 1024
  B  every epilogue x forms 128 / 256 / 384 / 1024
  C  batch boundaries inside a tile (rows per batch 1 .. 257): row slices of joint buffers, and dense 3-D operands
  D  grouped launches of M = 1, 300, 2100, 257 under three grouping depths
  E  split-K pairs (512) on a workspace of the test's own: halves of 2 .. 50 K-tiles, three exchanges, one slot short (256),
     twenty unsynchronized launches of 1, 2 and 6 tiles on one workspace
  F  stream-K ranges (640) on 2 .. 5 slots: cuts left in place, moved back, moved forward and on a tile boundary
  G  gemm10 walking the tile list (tiles >= 4 x CUs), ragged last row tile
  H  the fused QKV epilogue under forms 128 / 256 / 384 / 1024, H = 2, N = 3 H 128 and 2 H 128, against projection + fk_qkv_post_bf16

The one recorded run (MI355X, 256 CUs, `pytest -m gpu tests/test_hip_gemm_large_exact.py -s`, sections E and F as processes of
their own): 108 tests, all passed, 21.8 s for the whole file (A-D, G, H and the keyword test 14.8 s, E 3.4 s, F 3.6 s, process
start included); the slowest test is G [192-gate_res] at 2.3 s (the G tests 1.1 .. 2.3 s, every other one below 0.7 s).
  Launch forms seen (`[form]` lines; the forced form in every launch of every section):
    A  128, 256, 384 on both MFMA shapes, 1024 on 16: 120 / 60 / 30 / 60 shapes each
    B  128, 256, 384, 1024 for each of the ten epilogues        C  128, 256, 1024, both layouts        D  128, 256, 1024
    E  512 with slots == tiles (59 launches per exchange -- symmetric, whole, unannounced -- and MFMA shape, and the twenty-launch
       sequences, whose control words came back 4 x uses further on), 256 one slot short
    F  640 on all 12 grids per epilogue and MFMA shape           G  1024 (8092 x 8448, 1056 tiles on 256 CUs)
    H  128, 256, 384, 1024 for N = 3 H 128 and N = 2 H 128
  GELU / SiLU, exact share and largest distance (`[ulp]` lines; the assertion is max <= 1 ulp, not these shares):
    B  GELU  form 128 / 256 / 384 / 1024: 1.000000 each, max 0 ulp  (470400 / 1446912 / 921600 / 723456 elements)
       SiLU  form 128 / 256 / 384 / 1024: 0.999932 / 0.999950 / 0.999922 / 0.999950, max 1 ulp
    E  GELU  under split-K pairs, every exchange, both MFMA shapes: 1.000000, max 0 ulp  (1051392 elements each)
  Control run: with ONE element of the device copy of A raised by one (last row, last column of K) all 93 tests of A .. G fail.
"""
import contextlib
import functools
from types import SimpleNamespace

import pytest
import torch

import gemm_large_cases as L
import gemm_small_ref as R
from gemm_small_ref import BF, F32, GUARD_COLS, SENTINEL
from test_hip_gemm_small import _all_shapes, _UlpStats

pytestmark = pytest.mark.gpu

FORM_MFMA = [(f, m) for f in (128, 256, 384, 1024) for m in L.MFMA_OF[f]]
FORM3_MFMA = [(f, m) for f in L.C_FORMS for m in L.MFMA_OF[f]]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def forced(ops, variant, mfma, group_m=0, exchange="default"):
    """Forced launch controls, restored afterwards."""
    ops.gemm_set_variant(variant)
    ops.gemm_set_mfma(mfma)
    ops.gemm_set_group_m(group_m)
    ops.gemm_set_splitk_exchange(exchange)
    try:
        yield
    finally:
        ops.gemm_set_variant(0)
        ops.gemm_set_mfma(0)
        ops.gemm_set_group_m(0)
        ops.gemm_set_splitk_exchange("default")


def _upload(P):
    a_full, w_full = P.a_full.cuda(), P.w_full.cuda()          # the whole padded buffers: the views are taken on the device
    return SimpleNamespace(a_full=a_full, w_full=w_full, a=a_full[:, :P.K], w=w_full[:, :P.K], bias=P.bias.cuda(), P=P)


@functools.lru_cache(maxsize=None)
def _dev(P):
    """Device copies of a (small) problem's inputs, made once."""
    D = _upload(P)
    D.res, D.gate_wide = P.res.cuda(), P.gate_wide.cuda()
    return D


def _a3(D, B, Rr):
    """A as [B, R, K]: dense batches of the padded rows."""
    return D.a_full.view(B, Rr, D.P.K + L.PAD)[:, :, :D.P.K]


@functools.lru_cache(maxsize=None)
def _ws(slots):
    """A split-K workspace of the tests' own, zeroed once; one per slot count (the control words lie behind `slots` tiles)."""
    from gpt_image_edit_amd import libfk
    return torch.zeros(slots * libfk.FK_SPLITK_SLOT_BYTES, dtype=torch.uint8, device="cuda"), slots


def _launch(ops, epi, D, a, c, res=None, ws=None):
    """One call of epilogue `epi` on device views a -> c (res: the device residual of the out-of-place forms)."""
    P, w, bias = D.P, D.w, D.bias
    kw = {} if ws is None else dict(splitk_ws=ws)
    if res is None and epi in ("res", "gate_res"):
        res = D.res.view(c.shape)
    if epi.endswith("_inplace"):
        c.copy_(D.res.view(c.shape))
        res = c
    if epi == "f32":
        ops.gemm(a, w, bias, out=c, out_fp32=2, **kw)
    elif epi == "none_bias":
        ops.gemm(a, w, bias, out=c, **kw)
    elif epi == "none":
        ops.gemm(a, w, out=c, **kw)
    elif epi in L.ALPHAS:
        ops.gemm(a, w, out=c, epilogue=ops.FK_EPI_SCALE, alpha=L.ALPHAS[epi], **kw)
    elif epi in ("res", "res_inplace"):
        ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_RES, res=res, **kw)
    elif epi in L.GATED:
        ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_GATE_RES, res=res, gate=D.gate_wide[:, P.N:2 * P.N], **kw)
    elif epi in L.ACTIVATIONS:
        if not hasattr(D, "w_act"):
            D.w_act = P.act[0].cuda()[:, :P.K]
        ops.gemm(a, D.w_act, bias, out=c, epilogue=ops.FK_EPI_GELU_TANH if epi == "gelu" else ops.FK_EPI_SILU, **kw)
    else:
        raise ValueError(epi)


def _check(buf, idx, want, kind, what, stats=None):
    if kind == "ulp":
        if stats is not None:
            stats.add(buf, idx, want)
        R.check_ulp(buf, idx, want, what, max_ulp=1)
    else:
        R.check_guarded(buf, idx, want, what)


def _run(ops, epi, P, a, buf, idx, variant, what, rows_per_batch=None, res=None, ws=None, stats=None):
    _launch(ops, epi, _dev(P), a, buf[idx], res=res, ws=ws)
    got = ops.gemm_last_variant()
    assert got == variant, f"{what}: launch form {got}, expected {variant}"
    want, kind = L.want(epi, P, rows_per_batch)
    _check(buf, idx, want, kind, what, stats)


def _seen(section, what, variant):
    print(f"[form] {section} {what}: launch form {variant}", flush=True)


# ---- A: the K pipeline on the accumulators --------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,mfma", FORM_MFMA)
def test_a_k_tile_counts_on_the_fp32_accumulators(ops, form, mfma):
    """K = 64 .. 320: one to five K-tiles -- the prologue's clamped requests alone, one trip, the odd exit, two trips, the odd
    exit after two -- at M around the 256-row tile edge and N around the column tile, fp32(acc + bias) from the main loop."""
    def run(M, N, K):
        P = L.case_problem(M, N, K, 1, "f32")
        buf, idx, _ = R.guarded(M, N, F32, device="cuda")
        _run(ops, "f32", P, _dev(P).a, buf, idx, form, f"A form {form} mfma {mfma} M {M} N {N} K {K}")

    with forced(ops, form, mfma):
        _all_shapes(run, [(M, N, K) for K in L.A_KS for M, N in L.A_SHAPES[form]])
    _seen("A", f"forced {form} mfma {mfma}, {len(L.A_KS) * len(L.A_SHAPES[form])} shapes", form)


# ---- B: epilogues x forms -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", (128, 256, 384, 1024))
@pytest.mark.parametrize("epi", L.EPILOGUES)
def test_b_every_epilogue_under_every_form(ops, epi, form):
    stats = _UlpStats()

    def run(mfma, M, N, K):
        P = L.case_problem(M, N, K, 1, epi)
        D = _dev(P)
        gated = epi in L.GATED
        buf, idx, _ = R.guarded((1, M) if gated else M, N, device="cuda")
        with forced(ops, form, mfma):
            _run(ops, epi, P, _a3(D, 1, M) if gated else D.a, buf, idx, form, f"B {epi} form {form} mfma {mfma} M {M} N {N} K {K}",
                 rows_per_batch=M, stats=stats)

    shapes = [(mfma, M, N, K) for mfma in L.MFMA_OF[form] for M, N in L.B_SHAPES[form] for K in L.B_KS]
    try:
        _all_shapes(run, shapes)
    finally:
        if stats.n:
            print(stats.line(f"B {epi} form {form}, {len(shapes)} launches"), flush=True)
    _seen("B", f"{epi} forced {form}", form)


# ---- C: batch boundaries inside a tile ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["row_slices_of_joint_buffers", "dense_3d"])
@pytest.mark.parametrize("form,mfma", FORM3_MFMA)
def test_c_batch_boundaries_inside_a_tile(ops, form, mfma, layout):
    """Rows per batch from 1 to 257: batches that end inside a 256-row tile, several per tile (the float-reciprocal quotient
    of TileRows::crossed), one row each.  row_slices: A, the residual and C are [:, S_txt:] of joint [B, S, ld] buffers -- batch
    strides above R x ld, nothing flat, NaN / 99 / the sentinel in the text rows.  dense_3d: flat A and C, the gate alone batched."""
    N, K, S_txt = L.C_N, L.C_K, L.C_S_TXT

    def run(B, Rr, epi):
        P = L.case_problem(B * Rr, N, K, B, epi)
        D = _dev(P)
        what = f"C {layout} {epi} form {form} mfma {mfma} B {B} R {Rr}"
        if layout == "dense_3d":
            buf, idx, c = R.guarded(B * Rr, N, device="cuda")
            _launch(ops, epi, D, _a3(D, B, Rr), c.view(B, Rr, N))
        else:
            S = S_txt + Rr
            xd = torch.full((B, S, K + L.PAD), float("nan"), dtype=BF, device="cuda")
            xd[:, S_txt:, :K] = _a3(D, B, Rr)
            rd = torch.full((B, S, N + 16), 99.0, dtype=BF, device="cuda")
            rd[:, S_txt:, :N] = D.res.view(B, Rr, N)
            buf = torch.full((B, S + R.GUARD_ROWS, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")   # 3 guard rows behind a batch
            idx = (slice(None), slice(S_txt, S), slice(GUARD_COLS, GUARD_COLS + N))
            _launch(ops, epi, D, xd[:, S_txt:, :K], buf[idx], res=rd[:, S_txt:, :N])
        got = ops.gemm_last_variant()
        assert got == form, f"{what}: launch form {got}, expected {form}"
        R.check_guarded(buf, idx, L.want(epi, P, Rr)[0], what)
        if layout != "dense_3d":
            assert (rd[:, :S_txt] == 99).all() and (rd[:, :, N:] == 99).all(), f"{what}: the residual's buffer was written"

    with forced(ops, form, mfma):
        _all_shapes(run, [(B, Rr, epi) for B, Rr in L.C_BR for epi in L.C_EPILOGUES])
    _seen("C", f"{layout} forced {form} mfma {mfma}", form)


# ---- D: grouped launches ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epi", L.D_EPILOGUES)
@pytest.mark.parametrize("form,mfma", FORM3_MFMA)
def test_d_grouped_launches(ops, form, mfma, epi):
    """M = 1, 300, 2100 and 257 in one call, each problem with its own W, bias (and gate), under grouping depths 0 (default), 1, 3."""
    N, K = L.D_N, L.D_K
    for group_m in L.D_GROUP_M:
        probs, checks = [], []
        for B, Rr in L.D_BR:
            P = L.case_problem(B * Rr, N, K, B, epi)
            D = _dev(P)
            buf, idx, c = R.guarded((B, Rr), N, device="cuda")
            pr = dict(a=_a3(D, B, Rr), w=D.w, bias=D.bias, out=c)
            if epi == "gate_res":
                pr.update(res=D.res.view(B, Rr, N), gate=D.gate_wide[:, N:2 * N])
            probs.append(pr)
            checks.append((buf, idx, L.want(epi, P, Rr)[0], f"D {epi} form {form} mfma {mfma} group_m {group_m} M {B * Rr}"))
        with forced(ops, form, mfma, group_m=group_m):
            ops.gemm_grouped(probs, epilogue=ops.FK_EPI_GATE_RES if epi == "gate_res" else ops.FK_EPI_NONE)
            assert ops.gemm_last_variant() == form
        _all_shapes(lambda *ch: R.check_guarded(*ch), checks)
    _seen("D", f"{epi} forced {form} mfma {mfma}", form)


# ---- E: split-K pairs on a workspace of the test's own ------------------------------------------------------------------------------

def _e_operands(P, epi):
    D = _dev(P)
    if epi == "gate_res":
        B, Rr = L.E_GATE_BR
        buf, idx, _ = R.guarded((B, Rr), P.N, device="cuda")
        return _a3(D, B, Rr), buf, idx, Rr
    buf, idx, _ = R.guarded(P.M, P.N, F32 if epi == "f32" else BF, device="cuda")
    return D.a, buf, idx, None


@pytest.mark.parametrize("mfma", (16, 32))
@pytest.mark.parametrize("exchange", L.E_EXCHANGES)
def test_e_splitk_pairs(ops, exchange, mfma):
    """Two half-K workgroups per tile with halves of 2, 4, 6, 48 and 50 K-tiles, slots == tiles: the form must be 512."""
    stats = _UlpStats()

    def run(M, N, K, epi):
        P = L.case_problem(M, N, K, L.E_GATE_BR[0], epi)
        a, buf, idx, rpb = _e_operands(P, epi)
        _run(ops, epi, P, a, buf, idx, 512, f"E {exchange} mfma {mfma} {epi} M {M} N {N} K {K}", rows_per_batch=rpb,
             ws=_ws(L.tiles256(M, N)), stats=stats)

    shapes = [(M, N, K, epi) for K in L.E_KS for M, N in L.E_SHAPES for epi in L.E_EPILOGUES if L.e_applies(M, N, K, epi)]
    try:
        with forced(ops, 512, mfma, exchange=exchange):
            _all_shapes(run, shapes)
    finally:
        print(stats.line(f"E gelu, {exchange} exchange, mfma {mfma}"), flush=True)
    _seen("E", f"{exchange} exchange mfma {mfma}, {len(shapes)} launches", 512)


@pytest.mark.parametrize("mfma", (16, 32))
def test_e_one_slot_short_runs_the_unsplit_kernel(ops, mfma):
    """slots == tiles - 1: the pairs do not fit the workspace, the launcher must report 256 and the result is just as exact."""
    def run(M, N, K, epi):
        P = L.case_problem(M, N, K, L.E_GATE_BR[0], epi)
        a, buf, idx, rpb = _e_operands(P, epi)
        _run(ops, epi, P, a, buf, idx, 256, f"E one slot short mfma {mfma} {epi} M {M} N {N} K {K}", rows_per_batch=rpb,
             ws=_ws(L.tiles256(M, N) - 1))

    with forced(ops, 512, mfma):
        _all_shapes(run, [(M, N, K, epi) for K in (256, 6400) for M, N in L.E_SHAPES[1:] for epi in ("f32", "none_bias", "gate_res")
                          if L.e_applies(M, N, K, epi)])
    _seen("E", f"one slot short mfma {mfma}", 256)


@pytest.mark.parametrize("mfma", (16, 32))
@pytest.mark.parametrize("exchange", L.E_EXCHANGES)
def test_e_twenty_launches_share_one_workspace(ops, exchange, mfma):
    """Launches of 1, 2 and 6 tiles (halves of 2 and 6 K-tiles) alternate on one stream and one 6-slot workspace without a
    synchronize in between.  The control words are never reset: every use of a slot must leave its counter and its flag
    exactly 4 further on, which is read back from the workspace's tail (slot s is used by the launches of more than s tiles)."""
    from gpt_image_edit_amd import libfk
    ws = _ws(6)

    def control_words():
        torch.cuda.synchronize()
        return ws[0][6 * (libfk.FK_SPLITK_SLOT_BYTES - 8):].view(torch.int32).view(6, 2).cpu().to(torch.int64)

    before = control_words()
    jobs = []
    for M, N, K in L.E_SEQUENCE:
        P = L.case_problem(M, N, K, 1, "none_bias")
        jobs.append((P, _dev(P), R.guarded(M, N, device="cuda")))
    torch.cuda.synchronize()
    with forced(ops, 512, mfma, exchange=exchange):
        for P, D, (buf, idx, c) in jobs:
            ops.gemm(D.a, D.w, D.bias, out=c, splitk_ws=ws)
            assert ops.gemm_last_variant() == 512
    uses = torch.tensor([sum(L.tiles256(M, N) > slot for M, N, _ in L.E_SEQUENCE) for slot in range(6)])
    moved = (control_words() - before) % 2 ** 32
    assert torch.equal(moved, (4 * uses)[:, None].expand(6, 2)), f"control words moved by {moved.tolist()}, uses {uses.tolist()}"
    _all_shapes(lambda i, P, buf, idx: R.check_guarded(buf, idx, L.want("none_bias", P)[0],
                                                       f"E launch {i} of 20, {exchange} mfma {mfma} M {P.M} N {P.N} K {P.K}"),
                [(i, P, buf, idx) for i, (P, D, (buf, idx, c)) in enumerate(jobs)])
    _seen("E", f"twenty launches, {exchange} exchange mfma {mfma}", 512)


# ---- F: stream-K ranges forced ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mfma", (16, 32))
@pytest.mark.parametrize("epi", L.F_EPILOGUES)
def test_f_streamk_ranges(ops, epi, mfma):
    """Workspaces of 2 .. 5 slots = that many workgroups, grids just large enough: between them the cases hold a cut left in
    place, one moved back, one moved forward and one on a tile boundary (tests/test_gemm_large_host.py classifies them)."""
    def run(slots, M, N, K):
        B = 2 if epi in L.GATED else 1
        P = L.case_problem(M, N, K, B, epi)
        D = _dev(P)
        kinds = ",".join(L.cut_kinds(L.tiles256(M, N), K // 64, slots)[1])
        if epi in L.GATED:
            buf, idx, _ = R.guarded((B, M // B), N, device="cuda")
            a = _a3(D, B, M // B)
        else:
            buf, idx, _ = R.guarded(M, N, F32 if epi == "f32" else BF, device="cuda")
            a = D.a
        _run(ops, epi, P, a, buf, idx, 640, f"F {epi} mfma {mfma} slots {slots} M {M} N {N} K {K} cuts {kinds}",
             rows_per_batch=M // B, ws=_ws(slots))

    with forced(ops, 640, mfma):
        _all_shapes(run, L.streamk_cases())
    _seen("F", f"{epi} mfma {mfma}, {len(L.streamk_cases())} grids", 640)


# ---- G: gemm10 walking the tile list ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,epi", [(K, epi) for K in L.G_KS for epi in L.G_EPILOGUES])
def test_g_persistent_gemm10_walks_the_tile_list(ops, K, epi):
    """tiles >= 4 x CUs: one workgroup per CU walks the tile list (rows x (rows + 1) tiles, so the workgroups take unequal
    counts), the last row tile ragged.  The one large output of the file: compared on the device, its reference formed once per K."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M, N, B, Rr = L.persistent_grid(cus)
    P = L.case_problem(M, N, K, B, epi, big=True)
    assert L.big_bound_holds(P, epi), "unit sensitivity: a sum of the large problem leaves the range of 1-wide bf16 steps"
    D = _upload(P)
    what = f"G {epi} M {M} N {N} K {K} ({cus} CUs, {L.tiles256(M, N)} tiles)"
    with forced(ops, 1024, 16):
        if epi == "f32":
            buf, idx, c = R.guarded(M, N, F32, device="cuda")
            ops.gemm(D.a, D.w, D.bias, out=c, out_fp32=2)
        elif epi == "none_bias":
            buf, idx, c = R.guarded(M, N, device="cuda")
            ops.gemm(D.a, D.w, D.bias, out=c)
        else:
            buf, idx, c = R.guarded((B, Rr), N, device="cuda")
            ops.gemm(_a3(D, B, Rr), D.w, D.bias, out=c, epilogue=ops.FK_EPI_GATE_RES, res=P.res.cuda().view(B, Rr, N),
                     gate=P.gate_wide.cuda()[:, N:2 * N])
        assert ops.gemm_last_variant() == 1024
    R.check_guarded(buf, idx, L.want(epi, P, Rr)[0].cuda(), what)
    _seen("G", what, 1024)


# ---- H: the fused QKV epilogue under each forced form ---------------------------------------------------------------------------

@pytest.mark.parametrize("thirds", (3, 2), ids=["q_k_v", "q_k"])
@pytest.mark.parametrize("form,mfma", FORM_MFMA)
def test_h_fused_qkv_epilogue(ops, form, mfma, thirds):
    """FK_EPI_QKV at H = 2 (a 256-wide tile spans two heads), N = 3 H 128 and N = 2 H 128, B = 2 with the image rows of a batch
    (280) ending inside a tile, text + image in one grouped launch: bit for bit the projection followed by fk_qkv_post_bf16;
    q / k start sentinel-filled, and of C only the v third is stored."""
    _h_fused_qkv(ops, form, mfma, thirds)
    _seen("H", f"N = {thirds} H 128 forced {form} mfma {mfma}", form)


def _h_fused_qkv(ops, form, mfma, thirds, plain_launch=contextlib.nullcontext, fused_launches=(contextlib.nullcontext,)):
    """Section H's case.  plain_launch / fused_launches: context managers around the unfused reference launch and around each
    fused launch under test (tests/test_hip_gemm_walk_exact.py sets the tile walk's controls there)."""
    from oracle import mmdit
    from oracle.helpers import prepare_latent_image_ids
    B, H, S_txt, hh, ww, K = 2, 2, 70, 14, 20, 192
    S, D = S_txt + hh * ww, H * 128
    g = torch.Generator().manual_seed(71)
    x = torch.randn(B, S, K, generator=g).to(BF).cuda()
    w_i, w_t = ((torch.randn(3 * D, K, generator=g) * 0.06).to(BF).cuda() for _ in range(2))
    b_i, b_t = ((torch.randn(3 * D, generator=g) * 0.1).to(BF).cuda() for _ in range(2))
    nw = [(1 + torch.randn(128, generator=g) * 0.1).to(BF).cuda() for _ in range(4)]           # q_i k_i q_t k_t
    ids = torch.cat([torch.zeros(S_txt, 3), prepare_latent_image_ids(hh, ww)])
    cos, sin = (t.cuda() for t in mmdit.rope_tables(ids))
    Nf = thirds * D
    assert (B, S_txt, hh * ww, H) == (L.W_H_BATCH, L.W_H_S_TXT, L.W_H_S_IMG, L.W_H_HEADS)
    with forced(ops, form, mfma):
        plain = torch.empty(B, S, 3 * D, dtype=BF, device="cuda")
        with plain_launch():
            ops.gemm_grouped([dict(a=x[:, S_txt:], w=w_i, bias=b_i, out=plain[:, S_txt:]),
                              dict(a=x[:, :S_txt], w=w_t, bias=b_t, out=plain[:, :S_txt])])
        assert ops.gemm_last_variant() == form
        q_ref = torch.empty(B, H, S, 128, dtype=BF, device="cuda")
        k_ref = torch.empty_like(q_ref)
        ops.qkv_post(plain, q_ref, k_ref, nw[0], nw[1], nw[2], nw[3], cos, sin, S_txt)
        for fused_launch in fused_launches:
            q, k = torch.full_like(q_ref, SENTINEL), torch.full_like(q_ref, SENTINEL)
            fused = torch.full((B, S + 1, Nf + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
            fv = fused[:, :S, GUARD_COLS:GUARD_COLS + Nf]
            with fused_launch():
                ops.gemm_grouped([dict(a=x[:, S_txt:], w=w_i[:Nf], bias=b_i[:Nf], out=fv[:, S_txt:],
                                       qkv=dict(q_out=q, k_out=k, wq=nw[0], wk=nw[1], cos=cos, sin=sin, s_offset=S_txt)),
                                  dict(a=x[:, :S_txt], w=w_t[:Nf], bias=b_t[:Nf], out=fv[:, :S_txt],
                                       qkv=dict(q_out=q, k_out=k, wq=nw[2], wk=nw[3], cos=cos, sin=sin, s_offset=0))],
                                 epilogue=ops.FK_EPI_QKV)
            assert ops.gemm_last_variant() == form
            torch.cuda.synchronize()
            what = getattr(fused_launch, "what", "")
            assert torch.equal(q, q_ref), f"{what}{(q != q_ref).sum().item()} elements of q differ"
            assert torch.equal(k, k_ref), f"{what}{(k != k_ref).sum().item()} elements of k differ"
            want = torch.full_like(fused, SENTINEL)
            if thirds == 3:
                want[:, :S, GUARD_COLS + 2 * D:GUARD_COLS + 3 * D] = plain[:, :, 2 * D:]
            assert torch.equal(fused, want), f"{what}C: only the v third is stored by the fused epilogue, the guard band stays"


# ---- the wrapper's keyword --------------------------------------------------------------------------------------------------------

def test_splitk_ws_keyword_only_overrides_the_workspace(ops):
    """Without `splitk_ws` the wrapper builds the fk_gemm_args it built before: the stream's workspace from K = 6144 on, none below."""
    import ctypes
    a, w = torch.zeros(256, 6144, dtype=BF, device="cuda"), torch.zeros(256, 6144, dtype=BF, device="cuda")
    stream_ws, stream_slots = ops.splitk_workspace(a.device)
    mine = _ws(3)

    def fields(K, **kw):
        args, _ = ops._gemm_args(a[:, :K], w[:, :K], None, None, ops.FK_EPI_NONE, None, None, False, 1.0, **kw)
        return args, bytes(ctypes.string_at(ctypes.addressof(args), ctypes.sizeof(args)))

    long_default, _ = fields(6144)
    assert (long_default.splitk_ws, long_default.splitk_slots) == (stream_ws.data_ptr(), stream_slots)
    short_default, _ = fields(128)
    assert not short_default.splitk_ws and short_default.splitk_slots == 0
    for K in (128, 6144):
        own, _ = fields(K, splitk_ws=mine)
        assert (own.splitk_ws, own.splitk_slots) == (mine[0].data_ptr(), 3)
    none_given, _ = fields(6144, splitk_ws=None)
    # the two structs differ in nothing but the address of the output each call allocated
    none_given.C = long_default.C
    assert bytes(ctypes.string_at(ctypes.addressof(none_given), ctypes.sizeof(none_given))) == \
        bytes(ctypes.string_at(ctypes.addressof(long_default), ctypes.sizeof(long_default)))
    for bad in ((mine[0][:100], 3), (mine[0].view(torch.int8), 3), (mine[0], 0), (mine[0], 4)):
        with pytest.raises(ValueError, match="splitk_ws"):
            fields(128, splitk_ws=bad)
