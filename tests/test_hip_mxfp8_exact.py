"""Exact tests of the MXFP8 GEMM family (csrc/gemm_mxfp8.hip; `store_tile` / `store_tile_mxq` of csrc/gemm_epilogue.h) against the
CPU fp64 product of the dequantized operands, at the K-tile, scale-range and tile edges, and the containment of NaN blocks.

Data (tests/mxfp8_exact_cases.py, checked on the CPU by tests/test_mxfp8_exact_host.py)
  Elements are the e4m3 codes of the integers -15 .. 15 (-8 .. 8 for the split-K pairs' K >= 6144); the scale bytes are
  127 + e_b + u on A and 127 - e_b + v on W with one e_b of [-96, 96] per k-block and u, v of {0, 1, 2} per (row, block).  Every
  product term is an integer times 2^(u + v), every partial sum an integer below 2^24: the fp32 accumulators hold the fp64
  product in ANY order of summation and the assertion is EQUALITY -- while a scale byte taken from the wrong block, row or
  operand is wrong by up to 2^+-192.  `narrow` cases (e_b = 0) tell a scale problem from a summation problem.
  `all_codes_case` sends every finite e4m3 code through the MFMA alone.

Buffers
  C is always a view inside a sentinel-filled buffer (tests/gemm_small_ref.py: 3 guard rows, 8 guard columns, so ldc != N): the
  band must come back untouched.  (Integer sums can equal the sentinel; such an element is still compared, it just does not show
  that it was written.)  The operands are row-strided views, lda8 = K + 16 and lda_scale = K / 32 + 4, whose padding columns hold
  NaN codes (0x7f) and NaN scales (0xff): a read past K turns the output into NaN.  `ops.gemm_last_variant()` is asserted after
  every launch.

Bounds that are not equality
  GELU_TANH: every element within 1 bf16 ulp of `gemm_small_ref.epi_gelu`, none excluded -- the bound tests/test_hip_gemm_small.py
  states and justifies for the same `gelu_tanh_f`.  The one recorded run (MI355X, `pytest -m gpu tests/test_hip_mxfp8_exact.py -s`):
    GELU_TANH K 384, 6 shapes = 571392 elements: exact share 1.000000, max 0 bf16 ulp, with variant 128 and with variant 256.
  The assertion is max <= 1 ulp, not that share.
  Random real-valued operands (M 300, N 512, K 1152) against the fp64 product: |got - ref| <= C_RANDOM * 2^-24 * (|a| @ |w|^T) for
  every element.  The MFMA's internal order of summation is not specified, so C_RANDOM is not derived: it is 4 x the measured
  maximum of that ratio, rounded up to a power of two (the margin is for other seeds).  Measured in that run: 63.4763, the same
  for both variants (they accumulate in the same order), so C_RANDOM = 256.  K * 2^-24 * sum|terms| is the worst case of ANY fp32
  summation, so C_RANDOM <= K (= 1152) is asserted too: a larger measured value would be a bug to chase, not a bound to set.

Scale range: the wide cases (e_b of [-96, 96], scale bytes 31 .. 225, W's lower still in the GELU cases) are exact in every launch form; nothing had to be narrowed.

Time: the whole file (63 tests) ran in 5.8 s in that run; the slowest test, the first one to touch the device, took 0.37 s.
"""
import functools

import numpy as np
import pytest
import torch

import gemm_small_ref as R
import mxfp8_exact_cases as cases
import mxfp8_ref as ref
from conftest import bf16_ulp_diff
from gemm_small_ref import BF, F32, F64, GUARD_COLS, SENTINEL
from test_hip_gemm_small import _all_shapes

pytestmark = pytest.mark.gpu

VARIANTS = (128, 256)
SWEEP_KS = (128, 256, 384, 512, 1152)                 # 1, 2, 3, 4 and 9 K-tiles
SWEEP_MS, SWEEP_NS = (1, 255, 256, 257, 300), (256, 768)
NARROW_SHAPES = {128: (300, 256), 256: (257, 768), 384: (300, 768), 512: (255, 256), 1152: (300, 768)}
CODES_MS, CODES_N = (256, 300), 256
GROUP_MS, GROUP_N, GROUP_K = (1, 300, 2100, 257), 512, 384      # 2100 rows: 9 row tiles, a full group of 8 and a ragged one of 1
SPLITK_KS, SPLITK_SHAPES = (6144, 6400), ((256, 256), (300, 512))   # 6400: 25 K-tiles per half, part 1 starts on an odd K-tile
SPLITK_BR = {256: (2, 128), 300: (2, 150)}            # GATE_RES batches: 150 ends inside the tile and inside a 128-row half
EXCHANGES = ("whole", "symmetric", "unannounced")
EPI_K, EPI_N = 384, 512
GATE_BR = ((2, 150), (4, 70), (5, 60), (300, 1))      # the last three: several batch boundaries per tile (rpb < 256)
MXQ_MS, MXQ_NS, MXQ_KS = (1, 257, 300), (256, 768), (128, 384)
NAN_M, NAN_N, NAN_K = 300, 512, 384
RANDOM_SHAPE = (300, 512, 1152)
C_RANDOM = 256.0                                      # 4 x the measured 63.48, rounded up to a power of two (docstring)
Q_FILL = 0xA5                                         # fill byte of the quantized-output buffers around the window


def host_cases():
    """Every (M, N, K, narrow, act_shift) this file builds with `cases.exact_case` (tests/test_mxfp8_exact_host.py walks it)."""
    out = [(M, N, K, False, False) for K in SWEEP_KS for M in SWEEP_MS for N in SWEEP_NS]
    out += [(M, N, K, True, False) for K, (M, N) in NARROW_SHAPES.items()]
    out += [(M, GROUP_N, GROUP_K, False, False) for M in GROUP_MS]
    out += [(M, N, K, False, False) for K in SPLITK_KS for M, N in SPLITK_SHAPES]
    out += [(B * Rr, EPI_N, EPI_K, False, False) for B, Rr in GATE_BR]
    out += [(M, N, K, False, s) for M in MXQ_MS for N in MXQ_NS for K in MXQ_KS for s in (False, True)]
    out += [(NAN_M, NAN_N, NAN_K, False, False), (NAN_M, NAN_N, 6144, False, False)]
    return sorted(set(out))


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _case(M, N, K, narrow=False, act_shift=False):
    """One exact case, built once and shared (never modified): the builder's dict plus the fp64 tensors the checks use."""
    c = cases.exact_case(M, N, K, narrow=narrow, act_shift=act_shift)
    c["y0"] = torch.from_numpy(c["want"])
    c["bias_t"] = torch.from_numpy(c["bias"]).to(BF)
    c["y"] = c["y0"] + c["bias_t"].to(F64)
    return c


def _strided(pair):
    """An operand pair on the device as row-strided views: ld = K + 16 (codes) and K / 32 + 4 (scales), the padding columns
    holding NaN codes and NaN scales."""
    q, s = (np.ascontiguousarray(t) for t in pair)
    rows, K = q.shape
    qb = torch.full((rows, K + 16), 0x7f, dtype=torch.uint8, device="cuda")
    sb = torch.full((rows, K // 32 + 4), 0xff, dtype=torch.uint8, device="cuda")
    qb[:, :K] = torch.from_numpy(q).cuda()
    sb[:, :K // 32] = torch.from_numpy(s).cuda()
    return qb[:, :K], sb[:, :K // 32]


def _done(ops, variant, what):
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == variant, f"{what}: launch form {ops.gemm_last_variant()}, expected {variant}"


def _f32(y):
    out = y.to(F32)
    assert torch.equal(out.to(F64), y), "the expected value is not an fp32 number"
    return out


def _three_outputs(ops, c, a, w, variant, what, **kw):
    """fp32, bf16 without bias and bf16 with the integer bias of one case, each into its own guarded buffer, each exact."""
    M, N = c["want"].shape
    buf, idx, out = R.guarded(M, N, F32, device="cuda")
    ops.gemm_mxfp8(a, w, out=out, out_fp32=True, variant=variant, **kw)
    _done(ops, variant, what)
    R.check_guarded(buf, idx, _f32(c["y0"]), f"{what} fp32")
    buf, idx, out = R.guarded(M, N, device="cuda")
    ops.gemm_mxfp8(a, w, out=out, variant=variant, **kw)
    _done(ops, variant, what)
    R.check_guarded(buf, idx, R.epi_none(c["y0"]), f"{what} bf16")
    buf, idx, out = R.guarded(M, N, device="cuda")
    ops.gemm_mxfp8(a, w, c["bias_t"].cuda(), out=out, variant=variant, **kw)
    _done(ops, variant, what)
    R.check_guarded(buf, idx, R.epi_none(c["y"]), f"{what} bf16 + bias")


# ---- 1: the main loop at 1, 2, 3, 4 and 9 K-tiles ---------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", SWEEP_KS)
def test_main_loop_sweep(ops, K, variant):
    def run(M, N):
        c = _case(M, N, K)
        _three_outputs(ops, c, _strided(c["a"]), _strided(c["w"]), variant, f"v{variant} M {M} N {N} K {K}")

    _all_shapes(run, [(M, N) for M in SWEEP_MS for N in SWEEP_NS])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("K", SWEEP_KS)
def test_main_loop_narrow_scales(ops, K, variant):
    """e_b = 0: the same sums with scale bytes 127 .. 129.  Passing here and failing in the sweep is a scale problem."""
    M, N = NARROW_SHAPES[K]
    c = _case(M, N, K, narrow=True)
    _three_outputs(ops, c, _strided(c["a"]), _strided(c["w"]), variant, f"narrow v{variant} M {M} N {N} K {K}")


# ---- 2: every finite e4m3 code ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M", CODES_MS)
def test_every_e4m3_code(ops, M, variant):
    c = cases.all_codes_case(M, CODES_N)
    buf, idx, out = R.guarded(M, CODES_N, F32, device="cuda")
    ops.gemm_mxfp8(_strided(c["a"]), _strided(c["w"]), out=out, out_fp32=True, variant=variant)
    _done(ops, variant, "all codes")
    R.check_guarded(buf, idx, _f32(torch.from_numpy(c["want"])), f"every e4m3 code, v{variant} M {M}")


# ---- 3: grouped launch, ragged last group -------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_grouped_ragged_last_group(ops, variant):
    cs = [_case(M, GROUP_N, GROUP_K) for M in GROUP_MS]
    for dtype in (F32, BF):
        bufs = [R.guarded(M, GROUP_N, dtype, device="cuda") for M in GROUP_MS]
        ops.gemm_mxfp8_grouped([dict(a=_strided(c["a"]), w=_strided(c["w"]), out=b[2]) for c, b in zip(cs, bufs)],
                               out_fp32=dtype == F32, variant=variant)
        _done(ops, variant, "grouped")
        for c, (buf, idx, _), M in zip(cs, bufs, GROUP_MS):
            R.check_guarded(buf, idx, _f32(c["y0"]) if dtype == F32 else R.epi_none(c["y0"]), f"grouped v{variant} {dtype} M {M}")


# ---- 4: split-K pairs at the smallest K and at an odd number of K-tiles per half ----------------------------------------------

def _gate_res_problem(c, B, Rr, seed):
    """(residual bf16 [B, Rr, N] of integers, gate_wide bf16 [B, 3 N]) for FK_EPI_GATE_RES on case c."""
    N = c["want"].shape[1]
    g = torch.Generator().manual_seed(seed)
    return R.ints((B, Rr, N), -64, 64, seed), (torch.randn(B, 3 * N, generator=g) * 0.7).to(BF)


@pytest.mark.parametrize("M,N", SPLITK_SHAPES)
@pytest.mark.parametrize("K", SPLITK_KS)
def test_splitk_pairs_short_and_odd_halves(ops, K, M, N):
    from test_hip_mxfp8_splitk import _split_launch
    c = _case(M, N, K)
    a, w = _strided(c["a"]), _strided(c["w"])
    B, Rr = SPLITK_BR[M]
    res, gate_wide = _gate_res_problem(c, B, Rr, 40 + K + M)
    bias = c["bias_t"].cuda()
    gate = gate_wide.cuda()[:, N:2 * N]
    tiles = (M + 255) // 256 * (N // 256)

    def f32(**kw):
        buf, idx, out = R.guarded(M, N, F32, device="cuda")
        ops.gemm_mxfp8(a, w, out=out, out_fp32=True, **kw)
        torch.cuda.synchronize()
        return buf, idx

    def bf(**kw):
        buf, idx, out = R.guarded(M, N, device="cuda")
        ops.gemm_mxfp8(a, w, out=out, **kw)
        torch.cuda.synchronize()
        return buf, idx

    def gate_res(**kw):
        buf, idx, out = R.guarded((B, Rr), N, device="cuda")
        out.copy_(res.cuda())
        ops.gemm_mxfp8(a, w, bias, out=out, res=out, gate=gate, epilogue=ops.FK_EPI_GATE_RES, **kw)
        torch.cuda.synchronize()
        return buf, idx

    want_gr = R.epi_gate_res(c["y"], res, gate_wide[:, N:2 * N], Rr)
    buf, idx = gate_res(variant=256)
    assert ops.gemm_last_variant() == 256
    R.check_guarded(buf, idx, want_gr.view(B, Rr, N), f"unsplit GATE_RES M {M} N {N} K {K}")
    gr_unsplit = buf.cpu()
    try:
        for ex in EXCHANGES:
            ops.gemm_set_splitk_exchange(ex)
            for rep in range(2):                               # twice on the same workspace: nothing is reset in between
                what = f"split-K {ex} #{rep} M {M} N {N} K {K}"
                buf, idx = _split_launch(ops, tiles, lambda: f32(splitk=True, variant=512))
                R.check_guarded(buf, idx, _f32(c["y0"]), f"{what} fp32")
                buf, idx = _split_launch(ops, tiles, lambda: bf(splitk=True, variant=512))
                R.check_guarded(buf, idx, R.epi_none(c["y0"]), f"{what} bf16")
                buf, idx = _split_launch(ops, tiles, lambda: gate_res(splitk=True, variant=512))
                R.check_guarded(buf, idx, want_gr.view(B, Rr, N), f"{what} GATE_RES")
                assert torch.equal(buf.cpu(), gr_unsplit), f"{what}: GATE_RES differs from the unsplit 256 x 256 launch"
    finally:
        ops.gemm_set_splitk_exchange("default")


# ---- 5: epilogues on exact accumulators ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_gelu_every_element_within_one_ulp(ops, variant):
    n = exact = worst = 0
    shapes = [(M, N) for M in MXQ_MS for N in MXQ_NS]

    def run(M, N):
        nonlocal n, exact, worst
        c = _case(M, N, EPI_K, act_shift=True)
        buf, idx, out = R.guarded(M, N, device="cuda")
        ops.gemm_mxfp8(_strided(c["a"]), _strided(c["w"]), c["bias_t"].cuda(), out=out, epilogue=ops.FK_EPI_GELU_TANH, variant=variant)
        _done(ops, variant, "GELU")
        want = R.epi_gelu(c["y"])
        d = bf16_ulp_diff(buf.cpu()[idx], want)
        n, exact, worst = n + d.numel(), exact + int((d == 0).sum()), max(worst, int(d.max()))
        R.check_ulp(buf, idx, want, f"GELU v{variant} M {M} N {N} K {EPI_K}", max_ulp=1)

    try:
        _all_shapes(run, shapes)
    finally:
        print(f"[ulp] mxfp8 GELU_TANH v{variant} K {EPI_K}, {len(shapes)} shapes: {n} elements, exact share "
              f"{exact / max(n, 1):.6f}, max {worst} bf16 ulp", flush=True)


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("B,Rr", GATE_BR)
@pytest.mark.parametrize("variant", VARIANTS)
def test_gate_res_on_joint_buffers(ops, variant, B, Rr, inplace):
    """Residual and C as the row slices [:, S_txt:] of joint [B, S_txt + Rr, ld] buffers, the gate a column slice of [B, 3 N]."""
    S_txt, N = 2, EPI_N
    M, S = B * Rr, 2 + Rr
    c = _case(M, N, EPI_K)
    res, gate_wide = _gate_res_problem(c, B, Rr, 50 + B)
    gate = gate_wide.cuda()[:, N:2 * N]
    buf = torch.full((B, S + 1, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
    idx = (slice(None), slice(S_txt, S), slice(GUARD_COLS, GUARD_COLS + N))
    if inplace:
        buf[idx] = res.cuda()
        rd, rv = None, buf[idx]
    else:
        rd = torch.full((B, S, N + 16), 99.0, dtype=BF, device="cuda")
        rd[:, S_txt:, :N] = res.cuda()
        rv = rd[:, S_txt:, :N]
    ops.gemm_mxfp8(_strided(c["a"]), _strided(c["w"]), c["bias_t"].cuda(), out=buf[idx], res=rv, gate=gate,
                   epilogue=ops.FK_EPI_GATE_RES, variant=variant)
    _done(ops, variant, "GATE_RES")
    want = R.epi_gate_res(c["y"], res, gate_wide[:, N:2 * N], Rr)
    R.check_guarded(buf, idx, want.view(B, Rr, N), f"GATE_RES v{variant} B {B} R {Rr} {'in place' if inplace else ''}")
    if rd is not None:
        assert (rd[:, :S_txt] == 99).all() and (rd[:, :, N:] == 99).all() and torch.equal(rd[:, S_txt:, :N].cpu(), res)


@pytest.mark.parametrize("variant", VARIANTS)
def test_qkv_epilogue_two_heads_per_tile(ops, variant):
    """FK_EPI_QKV bit for bit against FK_EPI_NONE + fk_qkv_post_bf16, N = 768 (H = 2): with variant 256 a tile spans two heads and
    the q | k | v boundaries lie on tile edges; K = 128 is a single K-tile.  q / k start sentinel-filled: unwritten rows show."""
    from oracle import mmdit
    from oracle.helpers import prepare_latent_image_ids
    B, H, S_txt, hh, ww, K = 2, 2, 20, 12, 15, 128
    S_img = hh * ww
    S, D = S_txt + S_img, H * 128
    N = 3 * D
    g = torch.Generator().manual_seed(60)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(BF)

    def quant(x):
        return _strided(ref.quantize(x.reshape(-1, x.shape[-1]).double().numpy()))

    x = rnd(B, S, K)
    xi, xt = quant(x[:, S_txt:]), quant(x[:, :S_txt])
    wi, wt = quant(rnd(N, K, scale=0.06)), quant(rnd(N, K, scale=0.06))
    bi, bt = rnd(N, scale=0.1).cuda(), rnd(N, scale=0.1).cuda()
    nw = [(1 + rnd(128, scale=0.1).float()).to(BF).cuda() for _ in range(4)]
    ids = torch.cat([torch.zeros(S_txt, 3), prepare_latent_image_ids(hh, ww)])
    cos, sin = (t.cuda() for t in mmdit.rope_tables(ids))
    qkv_ref = torch.full((B, S, N), SENTINEL, dtype=BF, device="cuda")
    ops.gemm_mxfp8_grouped([dict(a=xi, w=wi, bias=bi, out=qkv_ref[:, S_txt:]), dict(a=xt, w=wt, bias=bt, out=qkv_ref[:, :S_txt])],
                           variant=variant)
    _done(ops, variant, "QKV projection")
    q_ref = torch.full((B, H, S, 128), SENTINEL, dtype=BF, device="cuda")
    k_ref = torch.full_like(q_ref, SENTINEL)
    ops.qkv_post(qkv_ref, q_ref, k_ref, nw[0], nw[1], nw[2], nw[3], cos, sin, S_txt)
    qkv = torch.full((B, S, N), SENTINEL, dtype=BF, device="cuda")
    q, k = torch.full_like(q_ref, SENTINEL), torch.full_like(q_ref, SENTINEL)
    ops.gemm_mxfp8_grouped([dict(a=xi, w=wi, bias=bi, out=qkv[:, S_txt:],
                                 qkv=dict(q_out=q, k_out=k, wq=nw[0], wk=nw[1], cos=cos, sin=sin, s_offset=S_txt)),
                            dict(a=xt, w=wt, bias=bt, out=qkv[:, :S_txt],
                                 qkv=dict(q_out=q, k_out=k, wq=nw[2], wk=nw[3], cos=cos, sin=sin, s_offset=0))],
                           epilogue=ops.FK_EPI_QKV, variant=variant)
    _done(ops, variant, "QKV epilogue")
    assert not (q_ref == SENTINEL).any() and not (k_ref == SENTINEL).any()
    assert torch.equal(q, q_ref) and torch.equal(k, k_ref)
    assert torch.equal(qkv[:, :, 2 * D:], qkv_ref[:, :, 2 * D:]) and not (qkv_ref == SENTINEL).any()


def _mxq_buffers(M, N, window):
    """(out_mx argument, q buffer, scale buffer, index of the written q window, index of the written scale window): the whole-
    buffer form as row-strided [M, N] views, or the column-window form (col_offset 256 of [M, 256 + N + 256]); both between
    guard rows, everything filled with Q_FILL."""
    G = R.GUARD_ROWS
    ld = 256 + N + 256 if window else N + 16
    qb = torch.full((M + 2 * G, ld), Q_FILL, dtype=torch.uint8, device="cuda")
    sb = torch.full((M + 2 * G, ld // 32 if window else N // 32 + 4), Q_FILL, dtype=torch.uint8, device="cuda")
    c0 = 256 if window else 0
    qi, si = (slice(G, G + M), slice(c0, c0 + N)), (slice(G, G + M), slice(c0 // 32, (c0 + N) // 32))
    arg = (qb[G:G + M], sb[G:G + M], 256) if window else (qb[qi], sb[si])
    return arg, qb, sb, qi, si


def _check_mxq(qb, sb, qi, si, want_pair, what):
    for name, buf, idx, want in (("codes", qb, qi, want_pair[0]), ("scales", sb, si, want_pair[1])):
        got = buf.cpu().numpy()
        bad = got[idx] != want
        assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} {name} differ from the reference quantizer, first at "
                               f"{np.argwhere(bad)[0].tolist()}")
        mask = np.ones_like(got, dtype=bool)
        mask[idx] = False
        assert (got[mask] == Q_FILL).all(), f"{what}: {name} outside the window were written"


def _bf16_as_f64(t):
    return t.cpu().to(F64).numpy()


@pytest.mark.parametrize("window", [False, True], ids=["whole", "column_window"])
@pytest.mark.parametrize("epi", ["none", "gelu"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_quantized_output(ops, variant, epi, window):
    """out_mx: the pair `mxfp8_ref.quantize` gives for the exact bf16 result (NONE) or for the kernel's own bf16 GELU output of
    the same launch form -- which test_gelu_every_element_within_one_ulp holds to the fp64 GELU."""
    def run(M, N, K):
        c = _case(M, N, K, act_shift=epi == "gelu")
        a, w, bias = _strided(c["a"]), _strided(c["w"]), c["bias_t"].cuda()
        what = f"out_mx {epi} v{variant} M {M} N {N} K {K}"
        if epi == "gelu":
            e = ops.FK_EPI_GELU_TANH
            y16 = ops.gemm_mxfp8(a, w, bias, epilogue=e, variant=variant)
            _done(ops, variant, what)
        else:
            e, y16 = ops.FK_EPI_NONE, R.epi_none(c["y"])
        arg, qb, sb, qi, si = _mxq_buffers(M, N, window)
        ops.gemm_mxfp8(a, w, bias, epilogue=e, variant=variant, out_mx=arg)
        _done(ops, variant, what)
        _check_mxq(qb, sb, qi, si, ref.quantize(_bf16_as_f64(y16)), what)

    _all_shapes(run, [(M, N, K) for M in MXQ_MS for N in MXQ_NS for K in MXQ_KS])


# ---- 6: a NaN block poisons exactly its row or column --------------------------------------------------------------------------

def _marked(pair, row, block):
    """A copy of the operand with one 32-element block marked as the quantizer marks an Inf / NaN block."""
    q, s = pair[0].copy(), pair[1].copy()
    q[row, 32 * block:32 * block + 32] = 0x7f
    s[row, block] = 0xff
    return q, s


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def _nan_runs(ops, c, a, w, variant, with_mx, **kw):
    """(fp32, bf16, (q, scales) or None) of one operand pair as host tensors, each from its own guarded launch."""
    M, N = c["want"].shape
    outs = []
    for dtype in (F32, BF):
        buf, idx, out = R.guarded(M, N, dtype, device="cuda")
        ops.gemm_mxfp8(a, w, out=out, out_fp32=dtype == F32, variant=variant, **kw)
        _done(ops, variant, "NaN containment")
        got = buf.cpu()
        mask = torch.ones_like(got, dtype=torch.bool)
        mask[idx] = False
        assert (got[mask] == SENTINEL).all(), "the guard band around C was written"
        outs.append(got[idx])
    if not with_mx:
        return outs + [None]
    arg, qb, sb, qi, si = _mxq_buffers(M, N, False)
    ops.gemm_mxfp8(a, w, variant=variant, out_mx=arg)
    _done(ops, variant, "NaN containment out_mx")
    return outs + [(qb.cpu().numpy(), sb.cpu().numpy(), qi, si)]


def _nan_containment(ops, K, variant, with_mx, **kw):
    M, N = NAN_M, NAN_N
    c = _case(M, N, K)
    base = _nan_runs(ops, c, _strided(c["a"]), _strided(c["w"]), variant, with_mx, **kw)
    assert torch.equal(base[0], _f32(c["y0"])) and torch.equal(base[1], R.epi_none(c["y0"]))
    errors = []
    marks = [("A", r, 1) for r in (0, 131, M - 1)] + [("W", col, K // 32 - 1) for col in (0, 131, N - 1)]
    for side, line, block in marks:
        try:
            am = _marked(c["a"], line, block) if side == "A" else c["a"]
            wm = _marked(c["w"], line, block) if side == "W" else c["w"]
            want_nan = torch.from_numpy(np.isnan(ref.dequantize(*am) @ ref.dequantize(*wm).T))
            hit = torch.zeros(M, N, dtype=torch.bool)
            if side == "A":
                hit[line] = True
            else:
                hit[:, line] = True
            assert torch.equal(want_nan, hit), "the fp64 reference does not confine NaN to the marked row / column"
            got = _nan_runs(ops, c, _strided(am), _strided(wm), variant, with_mx, **kw)
            for name, g, b in (("fp32", got[0], base[0]), ("bf16", got[1], base[1])):
                assert torch.equal(torch.isnan(g), hit), f"{name}: NaN in {int(torch.isnan(g).sum())} places, not exactly {side} line {line}"
                assert torch.equal(_bits(g)[~hit], _bits(b)[~hit]), f"{name}: an element outside {side} line {line} changed"
            if with_mx:
                (q, s, qi, si), (q0, s0, _, _) = got[2], base[2]
                y16 = _bf16_as_f64(base[1])
                y16[hit.numpy()] = np.nan
                wq, ws = ref.quantize(y16)
                assert np.array_equal(q[qi], wq) and np.array_equal(s[si], ws), "out_mx differs from the quantizer on the NaN result"
                qh = np.repeat(hit.numpy().reshape(M, N // 32, 32).any(-1), 32, axis=1)        # blocks that hold a NaN
                assert (q[qi][qh] == 0x7f).all() and (s[si][qh[:, ::32]] == 0xff).all()
                assert np.array_equal(q[qi][~qh], q0[qi][~qh]) and np.array_equal(s[si][~qh[:, ::32]], s0[si][~qh[:, ::32]])
                for bufm in (q, s):
                    mask = np.ones_like(bufm, dtype=bool)
                    mask[qi if bufm is q else si] = False
                    assert (bufm[mask] == Q_FILL).all(), "out_mx wrote outside its window"
        except AssertionError as e:
            errors.append(f"{side} line {line} block {block}: {e}")
    assert not errors, f"{len(errors)} of {len(marks)} marks fail:\n" + "\n".join(errors)


@pytest.mark.parametrize("variant", VARIANTS)
def test_nan_block_poisons_only_its_line(ops, variant):
    _nan_containment(ops, NAN_K, variant, with_mx=True)


def test_nan_block_poisons_only_its_line_split_k(ops):
    _nan_containment(ops, 6144, 512, with_mx=False, splitk=True)


# ---- 7: random real-valued operands against the fp64 product ------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_random_operands_against_fp64(ops, variant):
    M, N, K = RANDOM_SHAPE
    assert C_RANDOM <= K, "a bound above K * 2^-24 * sum|terms| is beyond the worst case of any fp32 summation"
    g = torch.Generator().manual_seed(7)
    a = ref.quantize((torch.randn(M, K, generator=g) * 0.5).to(BF).double().numpy())
    w = ref.quantize((torch.randn(N, K, generator=g) * 0.02).to(BF).double().numpy())
    da, dw = ref.dequantize(*a), ref.dequantize(*w)
    want, mag = da @ dw.T, np.abs(da) @ np.abs(dw).T
    buf, idx, out = R.guarded(M, N, F32, device="cuda")
    ops.gemm_mxfp8(_strided(a), _strided(w), out=out, out_fp32=True, variant=variant)
    _done(ops, variant, "random operands")
    got = buf.cpu()
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[idx] = False
    assert (got[mask] == SENTINEL).all()
    ratio = np.abs(got[idx].double().numpy() - want) / (2.0 ** -24 * mag)
    print(f"[parity] mxfp8 v{variant} M {M} N {N} K {K} vs fp64: max |got - ref| / (2^-24 |a| @ |w|^T) = {ratio.max():.4f} "
          f"(bound {C_RANDOM})", flush=True)
    assert ratio.max() <= C_RANDOM
