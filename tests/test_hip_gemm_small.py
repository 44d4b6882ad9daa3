"""Exact tests of the 128 x 128 register-staged GEMM (`gemm_bf16_kernel`, csrc/gemm_bf16.hip) and of the K-major layouts.

Which kernel runs, and how that is asserted
  A  bf16 output, M < 192: `fk_gemm_bf16` takes `gemm_bf16_kernel` for every such call -- the embedder MLPs, the modulation
     linears, the projector.  `ops.gemm_last_variant() == 0` after every call (the large-tile launcher would report 128 .. 1024).
  B  fp32 output (`out_fp32 = 1`) at any M: always `gemm_bf16_kernel<.., OUT_F32>`, so (1413, 136) also walks `map_tile`
     through a full group of 8 row tiles, a ragged group of 4 and a tile count that is no multiple of the 8 XCDs.  Variant 0.
  C  M >= 192 with operands the large-tile launcher refuses (`FK_E2BIG_STRIDES`): overlapping batches (an expanded A, batch
     stride 0) and a C / residual whose batch stride is 2^30 elements.  The call lands on `gemm_bf16_kernel` with its 64-bit
     row offsets; variant 0 again, through `ops.gemm` and through the per-problem loop of `ops.gemm_grouped`.
  D  K-major operands (layout 1: dX = dY W, layout 2: dW = dY^T X): the 256 x 256 ping-pong kernel, `gemm_last_variant() ==
     256`, on both MFMA shapes, against the fp64 product itself instead of the row-major kernel on transposed copies.

Data and why the sums are exact
  a and w are integers of [-2, 2], the bias of [-4, 4], residuals of [-64, 64] (all exact in bf16); K <= 3072.  Every partial
  sum is an integer of magnitude <= 4 K + 4 < 2^24, which fp32 holds exactly in any order, so the accumulators hold the fp64
  product (tests/gemm_small_ref.py asserts the range).  The helpers there restate each epilogue's rounding points on that
  exact value and the assertion is EQUALITY.  The gate is random bf16: gate * bf16(y) has 16 significant bits and is exact
  in fp32 too.  For GELU / SiLU, w is scaled by a power of two (still exact) so that |y| <= 8.  fp32 biases are k / 8 and
  fp32 residuals k / 4: every fp32 add stays exact.  C is a view inside a buffer filled with a sentinel (3 guard rows, 8
  guard columns, so ldc != N): the band must come back untouched and every element of C written.

GELU / SiLU: every element within 1 bf16 ulp of the once-rounded fp64 value, none excluded.  The hardware exp2 / rcp are
  good to about 1e-6 relative (fk_common.h), far below half a bf16 ulp (2^-9), so only values at a rounding boundary can move
  and only by one step.  The fp64 reference evaluates the tanh form as x * sigmoid(2 u): written with tanh it cancels to -0
  below x = -7, where the kernel (which uses the same identity) is right and would be 10^4 steps from it.
  The one recorded run (MI355X, `pytest -m gpu tests/test_hip_gemm_small.py -s`), 24 shapes = 383792 elements per K:
    GELU  K 64 / 128 / 192: exact share 1.000000 each, max 0 ulp;  expanded A (117600 elements): 1.000000, max 0 ulp
    SiLU  K 64 / 128 / 192: exact share 0.999906 / 0.999958 / 0.999872, max 1 ulp;  expanded A: 1.000000, max 0 ulp
    every normal bf16 input of 2^-24 <= |x| <= 8 (6914 values; M = 129 small kernel, M = 256 large-tile epilogue):
          GELU exact share 1.000000, max 0 ulp;  SiLU exact share 0.999939 (one value off by one step), max 1 ulp, both kernels
  The assertion is max <= 1 ulp, not these shares.

Nothing here is launched with arguments the entry point would have to survive: every refused case is rejected by
validation before a launch, and the buffers it names must come back untouched.

Time: the whole file (117 tests, no shape thinned out) ran in 3.1 s in that run; the slowest test took 0.20 s.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import gemm_small_ref as R
from conftest import bf16_ulp_diff, report
from gemm_small_ref import BF, F32, GUARD_COLS, SENTINEL

pytestmark = pytest.mark.gpu

MS, NS, KS = (1, 2, 127, 128, 129, 191), (8, 128, 136, 392), (64, 128, 192)     # 1, 2, 3 K-tiles: prologue only, even, odd exit
ALPHAS = {"scale_pow2": 0.125, "scale_rsqrt512": 512 ** -0.5}
FORMS_2D = ("none_bias", "none", "scale_pow2", "scale_rsqrt512", "res", "res_inplace", "gelu", "silu")
FORMS_GATE = ("gate_res", "gate_res_inplace")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def _problem(M, N, K, B=1, repeat=1):
    """Inputs and exact products of one shape, computed once and shared (never modified).  repeat: the M rows are `repeat`
    copies of M / repeat rows (an expanded A).  B: batches of the gate."""
    a0 = R.ints((M // repeat, K), -2, 2, 1000 + 13 * M + K)
    a = a0.repeat(repeat, 1)
    w, bias = R.ints((N, K), -2, 2, 2000 + 7 * N + K), R.ints((N,), -4, 4, 3000 + N + K)
    res = R.ints((M, N), -64, 64, 4000 + M + N)
    g = torch.Generator().manual_seed(5000 + M + N + K)
    gate_wide = (torch.randn(B, 3 * N, generator=g) * 0.7).to(BF)
    y0 = R.expected(a, w)
    # activations: the largest power of two that keeps |a w^T| s <= 4, so |y| <= 8 with the bias
    s = 2.0 ** torch.floor(torch.log2(4.0 / y0.abs().max().clamp(min=1.0))).item()
    w_act = (w.float() * s).to(BF)
    assert torch.equal(w_act.float(), w.float() * s)
    y_act = R.expected(a, w_act, bias)
    assert y_act.abs().max().item() <= 8
    return SimpleNamespace(M=M, N=N, K=K, B=B, a0=a0, a=a, w=w, bias=bias, res=res, gate_wide=gate_wide,
                           gate=gate_wide[:, N:2 * N], y0=y0, y=R.expected(a, w, bias), w_act=w_act, y_act=y_act)


def _launch(ops, form, P, a, c, res=None):
    """One call of `form` on device views a -> c.  res: the device residual for the out-of-place forms (default: a fresh
    contiguous one).  Returns (want, is_activation)."""
    w, bias = P.w.cuda(), P.bias.cuda()
    if res is None and form in ("res", "gate_res"):
        res = P.res.cuda().view(c.shape)
    if form.endswith("_inplace"):
        c.copy_(P.res.cuda().view(c.shape))
        res = c
    if form == "none_bias":
        ops.gemm(a, w, bias, out=c)
        return R.epi_none(P.y), False
    if form == "none":
        ops.gemm(a, w, out=c)
        return R.epi_none(P.y0), False
    if form in ALPHAS:
        ops.gemm(a, w, out=c, epilogue=ops.FK_EPI_SCALE, alpha=ALPHAS[form])
        return R.epi_scale(P.y0, ALPHAS[form]), False
    if form in ("res", "res_inplace"):
        ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_RES, res=res)
        return R.epi_res(P.y, P.res), False
    if form in FORMS_GATE:
        gate = P.gate_wide.cuda()[:, P.N:2 * P.N]              # a [B, N] column slice of [B, 3 N]
        ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_GATE_RES, res=res, gate=gate)
        return R.epi_gate_res(P.y, P.res, P.gate, a.shape[1]), False
    if form in ("gelu", "silu"):
        ops.gemm(a, P.w_act.cuda(), bias, out=c, epilogue=ops.FK_EPI_GELU_TANH if form == "gelu" else ops.FK_EPI_SILU)
        return (R.epi_gelu if form == "gelu" else R.epi_silu)(P.y_act), True
    raise ValueError(form)


class _UlpStats:
    def __init__(self):
        self.n = self.exact = self.worst = 0

    def add(self, buf, idx, want):
        d = bf16_ulp_diff(buf.cpu()[idx], want.reshape(buf[idx].shape))
        self.n, self.exact, self.worst = self.n + d.numel(), self.exact + int((d == 0).sum()), max(self.worst, int(d.max()))

    def line(self, what):
        return f"[ulp] {what}: {self.n} elements, exact share {self.exact / max(self.n, 1):.6f}, max {self.worst} bf16 ulp"


def _run_checked(ops, form, P, a, buf, idx, what, variant=0, stats=None, res=None):
    want, act = _launch(ops, form, P, a, buf[idx], res=res)
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == variant, f"{what}: launch form {ops.gemm_last_variant()}, expected {variant}"
    if act:
        if stats is not None:
            stats.add(buf, idx, want)
        R.check_ulp(buf, idx, want, what, max_ulp=1)
    else:
        R.check_guarded(buf, idx, want, what)


def _all_shapes(run, shapes):
    """Run every shape, then fail with all of them named (a wrong tile edge shows as a pattern over the shapes)."""
    errors = []
    for shape in shapes:
        try:
            run(*shape)
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, f"{len(errors)} of {len(shapes)} shapes fail:\n" + "\n".join(errors[:12])


# ---- A: bf16 output of the small kernel, M < 192 ----------------------------------------------------------------------------

@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("form", FORMS_2D)
def test_small_kernel_bf16_epilogues(ops, form, K):
    """The whole product M x N at this K: C a guarded 2-D view, A contiguous."""
    stats = _UlpStats()

    def run(M, N):
        P = _problem(M, N, K)
        buf, idx, _ = R.guarded(M, N, device="cuda")
        _run_checked(ops, form, P, P.a.cuda(), buf, idx, f"{form} M {M} N {N} K {K}", stats=stats)

    try:
        _all_shapes(run, [(M, N) for M in MS for N in NS])
    finally:
        if stats.n:
            print(stats.line(f"{form} K {K}, {len(MS) * len(NS)} shapes"), flush=True)


def test_small_kernel_long_k(ops):
    """48 K-tiles: the steady state of the two-stage loop, not only its first three trips."""
    M, N, K = 2, 392, 3072
    P = _problem(M, N, K)
    buf, idx, _ = R.guarded(M, N, device="cuda")
    _run_checked(ops, "none_bias", P, P.a.cuda(), buf, idx, f"none_bias M {M} N {N} K {K}")


@functools.lru_cache(maxsize=None)
def _every_bf16_value():
    """w [128, 128]: every bf16 value of 2^-24 <= |x| <= 8 (6914 values) in its first places, zeros in the rest."""
    pos = torch.arange(0, 0x8000, dtype=torch.int32).to(torch.int16).view(BF)
    pos = pos[(pos.float() >= 2.0 ** -24) & (pos.float() <= 8.0)]
    vals = torch.cat([pos, -pos])
    assert vals.numel() == 2 * (27 * 128 + 1)
    w = torch.zeros(128 * 128, dtype=BF)
    w[:vals.numel()] = vals
    return w.view(128, 128)


@pytest.mark.parametrize("M,small", [(129, True), (256, False)])
@pytest.mark.parametrize("form", ["gelu", "silu"])
def test_activation_epilogues_at_every_bf16_input(ops, form, M, small):
    """The data of the shape sweep reach a few hundred distinct activation inputs.  Here a one-hot A copies W through the
    product (y[m, n] = w[n, m % 128], exact), so the epilogue sees EVERY normal bf16 value of 2^-24 <= |x| <= 8, and 0: the
    1-ulp bound of the file's docstring at all of them, none excluded -- in the 128 x 128 kernel (M = 129, two row tiles) and,
    since gelu_tanh_f / silu_f are shared, in the large-tile epilogue the MLP-up GEMM uses (M = 256)."""
    w = _every_bf16_value()
    a = torch.zeros(M, 128, dtype=BF)
    a[torch.arange(M), torch.arange(M) % 128] = 1.0
    y = R.expected(a, w)
    assert torch.equal(y, w.double().T[torch.arange(M) % 128])
    buf, idx, c = R.guarded(M, 128, device="cuda")
    ops.gemm(a.cuda(), w.cuda(), out=c, epilogue=ops.FK_EPI_GELU_TANH if form == "gelu" else ops.FK_EPI_SILU)
    torch.cuda.synchronize()
    assert (ops.gemm_last_variant() == 0) == small
    want = (R.epi_gelu if form == "gelu" else R.epi_silu)(y)
    stats = _UlpStats()
    stats.add(buf, idx, want)
    print(stats.line(f"{form} at every bf16 input, M {M}"), flush=True)
    R.check_ulp(buf, idx, want, f"{form} at every bf16 input, M {M}", max_ulp=1)


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("form", FORMS_GATE)
def test_small_kernel_gated_residual(ops, form, B):
    """FK_EPI_GATE_RES on 3-D views, R = 70 rows per batch: with B = 2 (M = 140) batch 0 ends inside the first row tile, so
    rows 70 .. 127 must take batch 1's gate; C (and the in-place residual) is a guarded 3-D view with gaps between batches."""
    R_ = 70

    def run(N, K):
        P = _problem(B * R_, N, K, B=B)
        buf, idx, _ = R.guarded((B, R_), N, device="cuda")
        _run_checked(ops, form, P, P.a.cuda().view(B, R_, K), buf, idx, f"{form} B {B} R {R_} N {N} K {K}")

    _all_shapes(run, [(N, K) for N in NS for K in KS])


@pytest.mark.parametrize("B", [2, 1])
@pytest.mark.parametrize("form", ["none_bias", "res", "res_inplace", "gate_res", "gate_res_inplace", "silu"])
def test_small_kernel_row_slices_of_joint_buffers(ops, form, B):
    """A, the residual and C as the row slices [:, S_txt:] of joint [B, S, ld] buffers with ld wider than K or N: fk_rows
    batch strides on all three operands (B = 1: the same views are flat)."""
    S_txt, R_ = 10, 70
    S = S_txt + R_

    def run(N, K):
        P = _problem(B * R_, N, K, B=B)
        xd = torch.full((B, S, K + 8), 3.0, dtype=BF, device="cuda")          # 3: no operand value, would break equality
        xd[:, S_txt:, :K] = P.a.cuda().view(B, R_, K)
        rd = torch.full((B, S, N + 16), 99.0, dtype=BF, device="cuda")
        rd[:, S_txt:, :N] = P.res.cuda().view(B, R_, N)
        buf = torch.full((B, S + 1, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
        idx = (slice(None), slice(S_txt, S), slice(GUARD_COLS, GUARD_COLS + N))
        _run_checked(ops, form, P, xd[:, S_txt:, :K], buf, idx, f"joint {form} B {B} N {N} K {K}", res=rd[:, S_txt:, :N])
        assert (rd[:, :S_txt] == 99).all() and (rd[:, :, N:] == 99).all()

    _all_shapes(run, [(8, 128), (136, 192), (392, 64)])


# ---- B: fp32 output of the small kernel, at any M ---------------------------------------------------------------------------

F32_SHAPES = [(1413, 136, 64), (300, 77, 128), (129, 1, 64), (64, 130, 192), (77, 64, 3072)]
F32_FORMS = ("bias_bf16", "bias_f32", "res_f32", "bias_f32_res_f32_slice", "scale", "contiguous")


@functools.lru_cache(maxsize=None)
def _f32_problem(M, N, K):
    a, w = R.ints((M, K), -2, 2, 6000 + M + K), R.ints((N, K), -2, 2, 7000 + N + K)
    return SimpleNamespace(a=a, w=w, bias=R.ints((N,), -4, 4, 8000 + N), bias32=R.ints((N,), -32, 32, 8100 + N).float() / 8,
                           res32=R.ints((M, N), -64, 64, 8200 + M).float() / 4, y0=R.expected(a, w))


@pytest.mark.parametrize("form", F32_FORMS)
@pytest.mark.parametrize("M,N,K", F32_SHAPES)
def test_small_kernel_fp32_output(ops, M, N, K, form):
    P = _f32_problem(M, N, K)
    a, w = P.a.cuda(), P.w.cuda()
    buf, idx, c = R.guarded(M, N, F32, device="cuda")
    if form == "bias_bf16":
        ops.gemm(a, w, P.bias.cuda(), out=c, out_fp32=True)
        want = R.f32_none(P.y0, P.bias)
    elif form == "bias_f32":                                    # f32_flags bit 0
        ops.gemm(a, w, P.bias32.cuda(), out=c, out_fp32=True)
        want = R.f32_none(P.y0, P.bias32)
    elif form == "res_f32":                                     # f32_flags bit 1, no bias
        ops.gemm(a, w, out=c, out_fp32=True, res=P.res32.cuda())
        want = R.f32_none(P.y0, None, P.res32)
    elif form == "bias_f32_res_f32_slice":                      # both bits; the residual a column slice with a row stride of its own
        wide = torch.full((M, N + 5), 7.0, dtype=F32, device="cuda")
        wide[:, 4:4 + N] = P.res32.cuda()
        ops.gemm(a, w, P.bias32.cuda(), out=c, out_fp32=True, res=wide[:, 4:4 + N])
        want = R.f32_none(P.y0, P.bias32, P.res32)
    elif form == "scale":
        ops.gemm(a, w, out=c, out_fp32=True, epilogue=ops.FK_EPI_SCALE, alpha=512 ** -0.5)
        want = R.f32_scale(P.y0, 512 ** -0.5)
    else:                                                       # the output the entry point allocates itself
        out = ops.gemm(a, w, P.bias.cuda(), out_fp32=True)
        c.copy_(out)
        assert out.dtype == F32 and out.is_contiguous()
        want = R.f32_none(P.y0, P.bias)
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == 0
    R.check_guarded(buf, idx, want, f"fp32 {form} M {M} N {N} K {K}")


def test_unsupported_forms_are_refused_and_write_nothing(ops):
    M, N, K = 64, 136, 64
    P = _problem(M, N, K)
    a, w, bias = P.a.cuda(), P.w.cuda(), P.bias.cuda()
    buf32, _, c32 = R.guarded(M, N, F32, device="cuda")
    buf16, _, c16 = R.guarded(M, N, BF, device="cuda")
    res16 = P.res.cuda()
    gate = P.gate_wide.cuda()[:, N:2 * N]
    refused = [
        ("fp32 output supports", lambda: ops.gemm(a, w, bias, out=c32, out_fp32=True, epilogue=ops.FK_EPI_GELU_TANH)),
        ("fp32 output supports", lambda: ops.gemm(a, w, bias, out=c32, out_fp32=True, epilogue=ops.FK_EPI_SILU)),
        ("no fp32 output", lambda: ops.gemm(a, w, bias, out=c32, out_fp32=True, epilogue=ops.FK_EPI_RES, res=res16)),
        ("no fp32 output", lambda: ops.gemm(a.view(1, M, K), w, bias, out=c32, out_fp32=True, epilogue=ops.FK_EPI_GATE_RES,
                                            res=res16, gate=gate)),
        ("residual pointer", lambda: ops.gemm(a, w, bias, out=c16, epilogue=ops.FK_EPI_RES)),                   # no residual
        ("gate pointer", lambda: ops.gemm(a, w, bias, out=c16, epilogue=ops.FK_EPI_GATE_RES, res=res16)),       # no gate
        ("multiple of 8", lambda: ops.gemm(a, w[:12], out=c16[:, :12])),                                       # bf16 output, N = 12
        ("unknown epilogue", lambda: ops.gemm(a, w, bias, out=c16, epilogue=99)),
    ]
    for match, call in refused:
        with pytest.raises(RuntimeError, match=match):
            call()
    torch.cuda.synchronize()
    assert (buf32 == SENTINEL).all() and (buf16 == SENTINEL).all(), "a refused call wrote to C"


# ---- C: the fallback behind FK_E2BIG_STRIDES --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS_2D + FORMS_GATE)
def test_overlapping_batches_fall_back_to_the_small_kernel(ops, form):
    """A = x[None].expand(3, 100, K): batch stride 0, M = 300 >= 192.  The large-tile launcher refuses batches that overlap
    (its tile-relative offsets must grow), so the 128 x 128 kernel computes all 3 x 3 = 9 tiles from the same 100 rows."""
    Bx, R_, N, K = 3, 100, 392, 192
    P = _problem(Bx * R_, N, K, B=Bx, repeat=Bx)
    a = P.a0.cuda()[None].expand(Bx, R_, K)
    assert a.stride(0) == 0
    buf, idx, _ = R.guarded(Bx * R_, N, device="cuda")
    stats = _UlpStats()
    _run_checked(ops, form, P, a, buf, idx, f"expanded A, {form}", stats=stats)
    if stats.n:
        print(stats.line(f"expanded A, {form}"), flush=True)
        report(f"expanded A, {form}", buf[idx], (R.epi_gelu if form == "gelu" else R.epi_silu)(P.y_act))


@pytest.mark.parametrize("form", ["none_bias", "res_inplace", "gate_res", "gelu"])
def test_grouped_fallback_runs_every_problem(ops, form):
    """Two problems in one ops.gemm_grouped: the expanded A (refused by the large-tile launcher, which refuses the whole
    group with it) and an ordinary [2, 70, K] one -- the per-problem loop at the end of fk_gemm_bf16_grouped."""
    N, K = 392, 192
    P1, P2 = _problem(300, N, K, B=3, repeat=3), _problem(140, N, K, B=2)
    a1, a2 = P1.a0.cuda()[None].expand(3, 100, K), P2.a.cuda().view(2, 70, K)
    (buf1, idx1, c1), (buf2, idx2, c2) = R.guarded((3, 100), N, device="cuda"), R.guarded((2, 70), N, device="cuda")
    probs, wants = [], []
    for P, a, c in ((P1, a1, c1), (P2, a2, c2)):
        pr = dict(a=a, w=(P.w_act if form == "gelu" else P.w).cuda(), bias=P.bias.cuda(), out=c)
        if form == "res_inplace":
            c.copy_(P.res.cuda().view(c.shape))
            pr["res"] = c
            wants.append(R.epi_res(P.y, P.res))
        elif form == "gate_res":
            pr.update(res=P.res.cuda().view(c.shape), gate=P.gate_wide.cuda()[:, N:2 * N])
            wants.append(R.epi_gate_res(P.y, P.res, P.gate, a.shape[1]))
        elif form == "gelu":
            wants.append(R.epi_gelu(P.y_act))
        else:
            wants.append(R.epi_none(P.y))
        probs.append(pr)
    epi = dict(none_bias=ops.FK_EPI_NONE, res_inplace=ops.FK_EPI_RES, gate_res=ops.FK_EPI_GATE_RES, gelu=ops.FK_EPI_GELU_TANH)[form]
    ops.gemm_grouped(probs, epilogue=epi)
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == 0
    for buf, idx, want, name in ((buf1, idx1, wants[0], "expanded"), (buf2, idx2, wants[1], "ordinary")):
        if form == "gelu":
            R.check_ulp(buf, idx, want, f"grouped {form}, {name} problem")
        else:
            R.check_guarded(buf, idx, want, f"grouped {form}, {name} problem")


def test_batch_stride_beyond_two_gib_falls_back(ops):
    """C = res (in place), a [2, 150, 136] view with ld 144 and a batch stride of 2^30 elements inside ONE bf16 buffer of
    2^30 + 152 * 144 elements (2 GiB): a 256-row tile spans more than 2^31 bytes, the large-tile launcher answers
    FK_E2BIG_STRIDES and the 128 x 128 kernel's 64-bit row offsets carry the second batch.  Only the 152 rows at each batch's
    place are initialised and read back: 150 used ones between one sentinel row before and one after (and 8 guard columns)."""
    B, R_, N, K, ld, bs = 2, 150, 136, 192, 144, 2 ** 30
    P = _problem(B * R_, N, K, B=B)
    big = torch.empty(bs + (R_ + 2) * ld, dtype=BF, device="cuda")
    try:
        regions = [big[b * bs:b * bs + (R_ + 2) * ld].view(R_ + 2, ld) for b in range(B)]
        for b, reg in enumerate(regions):
            reg.fill_(SENTINEL)
            reg[1:R_ + 1, :N] = P.res.cuda().view(B, R_, N)[b]
        c = torch.as_strided(big, (B, R_, N), (bs, ld, 1), storage_offset=ld)
        assert c.data_ptr() == regions[0][1:].data_ptr() and c[1].data_ptr() == regions[1][1:].data_ptr()
        ops.gemm(P.a.cuda().view(B, R_, K), P.w.cuda(), P.bias.cuda(), out=c, epilogue=ops.FK_EPI_GATE_RES, res=c,
                 gate=P.gate_wide.cuda()[:, N:2 * N])
        torch.cuda.synchronize()
        assert ops.gemm_last_variant() == 0
        got = torch.stack([reg.cpu() for reg in regions])
        R.check_guarded(got, (slice(None), slice(1, R_ + 1), slice(0, N)), R.epi_gate_res(P.y, P.res, P.gate, R_),
                        "C / res with a 2^30-element batch stride")
    finally:
        del big
        regions = c = None
        torch.cuda.empty_cache()


# ---- D: K-major layouts, exact -----------------------------------------------------------------------------------------------

@pytest.fixture(params=[16, 32])
def k_major(ops, request):
    ops.gemm_set_plan(1)
    ops.gemm_set_mfma(request.param)
    try:
        yield request.param
    finally:
        ops.gemm_set_plan(3)
        ops.gemm_set_mfma(0)


@functools.lru_cache(maxsize=None)
def _layout1_problem(M, K, N, wide):
    a = R.ints((M, K), -2, 2, 9000 + M + K)
    wfull = R.ints((K, 512 + N if wide else N), -2, 2, 9100 + K + N)
    w = wfull[:, 256:256 + N] if wide else wfull
    res = R.ints((M, N), -64, 64, 9200 + M + N)
    return SimpleNamespace(a=a, wfull=wfull, res=res, y=R.expected(a, w.t()))


@pytest.mark.parametrize("wide", [False, True], ids=["whole_w", "w_column_slice"])
@pytest.mark.parametrize("M,K,N", [(300, 64, 256), (300, 192, 512), (1, 128, 256), (513, 320, 256)])
def test_layout1_against_the_fp64_product(ops, k_major, M, K, N, wide):
    """dX = dY W with W as stored, [K, N]: plain, FK_EPI_RES out of place and in place, C guarded."""
    P = _layout1_problem(M, K, N, wide)
    a, wfull = P.a.cuda(), P.wfull.cuda()
    w = wfull[:, 256:256 + N] if wide else wfull
    for form in ("plain", "res", "res_inplace"):
        buf, idx, c = R.guarded(M, N, device="cuda")
        if form == "plain":
            ops.gemm(a, w, out=c, layout=1)
            want = R.epi_none(P.y)
        else:
            res = P.res.cuda()
            if form == "res_inplace":
                c.copy_(res)
                res = c
            ops.gemm(a, w, out=c, epilogue=ops.FK_EPI_RES, res=res, layout=1)
            want = R.epi_res(P.y, P.res)
        torch.cuda.synchronize()
        assert ops.gemm_last_variant() == 256
        R.check_guarded(buf, idx, want, f"layout 1 {form} M {M} K {K} N {N} mfma {k_major}")


def test_layout1_grouped_on_row_slices(ops, k_major):
    """One grouped launch on the image / text row slices of a [2, 160, K] buffer (S_txt = 24): batched rows on A and C."""
    B, S, S_txt, K, N = 2, 160, 24, 192, 256
    x = R.ints((B, S, K), -2, 2, 9300)
    wi, wt = R.ints((K, N), -2, 2, 9301), R.ints((K, N), -2, 2, 9302)
    xd = x.cuda()
    buf = torch.full((B, S + 1, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
    ov = buf[:, :S, GUARD_COLS:GUARD_COLS + N]
    ops.gemm_grouped([dict(a=xd[:, S_txt:], w=wi.cuda(), out=ov[:, S_txt:], layout=1),
                      dict(a=xd[:, :S_txt], w=wt.cuda(), out=ov[:, :S_txt], layout=1)])
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == 256
    want = torch.cat([R.epi_none(R.expected(x[:, :S_txt].contiguous(), wt.t())).view(B, S_txt, N),
                      R.epi_none(R.expected(x[:, S_txt:].contiguous(), wi.t())).view(B, S - S_txt, N)], dim=1)
    R.check_guarded(buf, (slice(None), slice(0, S), slice(GUARD_COLS, GUARD_COLS + N)), want, f"layout 1 grouped mfma {k_major}")


@pytest.mark.parametrize("T,M,N", [(64, 256, 256), (192, 256, 512), (320, 512, 256)])
def test_layout2_against_the_fp64_product(ops, k_major, T, M, N):
    """dW = dY^T X, both operands token-major slices of wider [1, T + 64, *] buffers; |sums| <= 4 T = 1280."""
    dyb, xb = R.ints((1, T + 64, M + 128), -2, 2, 9400 + T), R.ints((1, T + 64, N + 256), -2, 2, 9500 + T)
    dy, x = dyb.cuda()[:, 64:, 128:], xb.cuda()[:, :T, 256:]
    buf, idx, c = R.guarded(M, N, device="cuda")
    ops.gemm(dy, x, out=c, layout=2)
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == 256
    want = R.epi_none(R.expected(dyb[0, 64:, 128:].t(), xb[0, :T, 256:].t()))
    R.check_guarded(buf, idx, want, f"layout 2 T {T} M {M} N {N} mfma {k_major}")


def test_k_major_refusals_write_nothing(ops, k_major):
    """What the K-major launcher documents as unsupported is refused before a launch: C keeps its sentinel."""
    a = R.ints((256, 128), -2, 2, 9600).cuda()
    buf, idx, c = R.guarded(256, 256, device="cuda")
    res = R.ints((256, 256), -64, 64, 9601).cuda()
    w200, w256 = R.ints((128, 200), -2, 2, 9602).cuda(), R.ints((128, 256), -2, 2, 9603).cuda()
    a2 = R.ints((1, 128, 384), -2, 2, 9604).cuda()                 # layout 2, M = 384
    a3 = R.ints((1, 128, 256), -2, 2, 9605).cuda()                 # layout 2, M = 256
    buf2, _, c2 = R.guarded(384, 256, device="cuda")
    refused = [
        lambda: ops.gemm(a, w200, out=c[:, :200], layout=1),                                           # N % 256
        lambda: ops.gemm(a2, w256[None], out=c2, layout=2),                                            # layout 2, M % 256
        lambda: ops.gemm(a, w256, out=c, layout=1, epilogue=ops.FK_EPI_GELU_TANH),                     # an activation
        lambda: ops.gemm(a, w256, out=c, layout=1, epilogue=ops.FK_EPI_SCALE, alpha=0.5),
        lambda: ops.gemm(a.view(1, 256, 128), w256, out=c, layout=1, epilogue=ops.FK_EPI_GATE_RES, res=res,
                         gate=res[:1]),
        lambda: ops.gemm(a3, w256[None], out=c, layout=2, epilogue=ops.FK_EPI_RES, res=res),          # layout 2 has no residual form
    ]
    for call in refused:
        with pytest.raises(RuntimeError, match="layout"):
            call()
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (buf2 == SENTINEL).all(), "a refused call wrote to C"
