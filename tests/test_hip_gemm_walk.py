"""The tile walk of the large-tile bf16 GEMMs (gemm_walk_kernel of csrc/gemm_pingpong_bf16.hip): one workgroup per CU walks
tiles g, g + G, ... of the launch and requests the next tile's first K-tile in front of the current tile's epilogue.

Every assertion is EXACT EQUALITY of the output bytes -- the whole sentinel-filled buffer around C, guard band included --
between two calls on the same inputs: the reference side carries FK_GEMM_PLAN_TILE_PER_WG (one workgroup per tile, the form
every other GEMM test holds to fp64 / integer references), the side under test FK_GEMM_PLAN_WALK with a cap G on the number of
workgroups, so that problems of 9 .. 21 tiles put 1, 2 and 3 (and up to 5) tiles on one workgroup.  `ops.gemm_last_variant()`
is asserted on both sides: the walk reports the form it walks (256 / 384).

What the shapes reach (M = 768, N = 768: 9 tiles of 256 x 256):
  cap 3 -> 3 / 3 / 3 tiles per workgroup, cap 4 -> 3 / 2 / 2 / 2, cap 2 -> 5 / 4
  K = 64, 128, 192, 3072 = 1, 2, 3, 48 K-tiles: the prefetched K-tile 0 is the tile's only one (K-tile 1's requests clamped),
    one trip, the odd exit, the production depth
  M = 700: the last row tile ragged (its epilogue's store count is not the full tile's: the conservative first wait)
  mixed grid at M = 768, N = 1024 on 256 CUs: 3 big + 18 small tiles, one big tile on each of XCDs 0 .. 2; cap 8 gives
    workgroups 0 .. 2 a big tile and then two small ones, workgroups 3 .. 7 small ones only; cap 5 mixes the XCDs
  (tests/test_gemm_walk_map.py holds the walk's places against the launch's tile order on the CPU.)
"""
import contextlib

import pytest
import torch

import gemm_small_ref as R
from gemm_small_ref import BF, GUARD_COLS, SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def launch(ops, variant, mfma, walk, cap=0):
    ops.gemm_set_variant(variant)
    ops.gemm_set_mfma(mfma)
    ops.gemm_set_walk(walk, cap)
    try:
        yield
    finally:
        ops.gemm_set_variant(0)
        ops.gemm_set_mfma(0)
        ops.gemm_set_walk("default")


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF).cuda()


def _both(ops, variant, mfma, caps, call, what, expect=None, repeat=False):
    """call() -> list of output buffers (freshly sentinel-filled inside).  Old form once, the walk under every cap."""
    expect = variant if expect is None else expect
    with launch(ops, variant, mfma, "tile_per_wg"):
        ref = call()
        assert ops.gemm_last_variant() == expect, f"{what}: old form reports {ops.gemm_last_variant()}, expected {expect}"
    torch.cuda.synchronize()
    assert all(bool((r != SENTINEL).any()) for r in ref), f"{what}: the reference side stored nothing"
    for cap in caps:
        with launch(ops, variant, mfma, "walk", cap):
            got = call()
            assert ops.gemm_last_variant() == expect, f"{what} cap {cap}: the walk reports {ops.gemm_last_variant()}, expected {expect}"
            if repeat:      # a second launch on the same buffers, nothing reset in between
                got = call(got)
        torch.cuda.synchronize()
        for i, (r, o) in enumerate(zip(ref, got)):
            bad = r.view(torch.int16) != o.view(torch.int16)
            assert not bool(bad.any()), (f"{what} cap {cap} output {i}: {int(bad.sum())} of {bad.numel()} elements differ from the "
                                         f"one-workgroup-per-tile launch, first at {bad.nonzero()[0].tolist()}")


@pytest.mark.parametrize("mfma", (16, 32))
@pytest.mark.parametrize("K", (64, 128, 192, 3072))
def test_k_tile_counts_under_caps(ops, K, mfma):
    M = N = 768
    a, w, bias = _rand((M, K), 1, 1.0), _rand((N, K), 2, 0.05), _rand((N,), 3)

    def call(bufs=None):
        buf, idx, c = R.guarded(M, N, device="cuda")
        ops.gemm(a, w, bias, out=c)
        return [buf]

    _both(ops, 256, mfma, (2, 3, 4), call, f"K {K} mfma {mfma}")


@pytest.mark.parametrize("N,expect", [(1024, 256), (1000, 128)])
def test_ragged_rows_and_a_width_the_256_kernel_declines(ops, N, expect):
    """M = 700: rows 700 .. 767 of the last row tile are never stored.  N = 1000 is no multiple of 256: neither the 256 x 256 nor
    the mixed grid takes it (the launcher answers 128 under both plans, which has no walking form) -- the walk bits must change
    nothing there."""
    M, K = 700, 192
    a, w, bias = _rand((M, K), 4), _rand((N, K), 5, 0.05), _rand((N,), 6)

    def call(bufs=None):
        buf, idx, c = R.guarded(M, N, device="cuda")
        ops.gemm(a, w, bias, out=c)
        return [buf]

    _both(ops, 256, 16, (3, 5), call, f"M {M} N {N}", expect=expect)
    if N % 256 == 0:
        _both(ops, 384, 16, (3, 5, 8), call, f"mixed M {M} N {N}")


def test_grouped_launch_hands_a_workgroup_tiles_of_both_problems(ops):
    """M = 512 and M = 256 with weights, biases and outputs of their own: 6 + 3 tiles; under caps 2 and 4 consecutive tiles
    of a workgroup belong to different problems."""
    N, K = 768, 192
    probs = [(_rand((M, K), 10 + i), _rand((N, K), 20 + i, 0.05), _rand((N,), 30 + i)) for i, M in enumerate((512, 256))]

    def call(bufs=None):
        outs = [R.guarded(a.shape[0], N, device="cuda") for a, _, _ in probs]
        ops.gemm_grouped([dict(a=a, w=w, bias=b, out=o[2]) for (a, w, b), o in zip(probs, outs)])
        return [o[0] for o in outs]

    _both(ops, 256, 16, (2, 4), call, "grouped 512 + 256")


def test_batched_rows_below_a_tile_for_output_residual_and_gate(ops):
    """B = 3 slices [:, S_txt:] of joint [B, S, ld] buffers with 192 rows per batch (below a tile): nothing flat -- A, C and the
    residual cross a batch boundary inside every tile, the gate row changes with them."""
    B, Rr, S_txt, N, K = 3, 192, 40, 768, 192
    S = S_txt + Rr
    x = torch.full((B, S, K + 16), float("nan"), dtype=BF, device="cuda")
    x[:, S_txt:, :K] = _rand((B, Rr, K), 40)
    res = torch.full((B, S, N + 16), 99.0, dtype=BF, device="cuda")
    res[:, S_txt:, :N] = _rand((B, Rr, N), 41)
    w, bias = _rand((N, K), 42, 0.05), _rand((N,), 43)
    gate = _rand((B, 3 * N), 44)

    def call(bufs=None):
        buf = torch.full((B, S + R.GUARD_ROWS, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
        c = buf[:, S_txt:S, GUARD_COLS:GUARD_COLS + N]
        ops.gemm(x[:, S_txt:, :K], w, bias, out=c, epilogue=ops.FK_EPI_GATE_RES, res=res[:, S_txt:, :N], gate=gate[:, N:2 * N])
        return [buf]

    _both(ops, 256, 16, (3, 4), call, "batched gate_res, 192 rows per batch")
    assert bool((res[:, :S_txt] == 99).all()) and bool((res[:, :, N:] == 99).all()), "the residual's buffer was written"


@pytest.mark.parametrize("variant", (256, 384))
@pytest.mark.parametrize("epi", ("none", "gelu", "silu", "gate_res", "res", "scale"))
def test_every_epilogue(ops, epi, variant):
    """M = 768 as B = 2 batches of 384 rows (per-batch gate rows), N = 1024, K = 192: 12 tiles of 256 x 256, or 3 + 18 mixed."""
    B, Rr, N, K = 2, 384, 1024, 192
    a, w, bias = _rand((B, Rr, K), 50), _rand((N, K), 51, 0.05), _rand((N,), 52)
    res, gate = _rand((B, Rr, N), 53), _rand((B, N), 54)

    def call(bufs=None):
        buf, idx, c = R.guarded((B, Rr), N, device="cuda")
        if epi == "none":
            ops.gemm(a, w, out=c)
        elif epi == "scale":
            ops.gemm(a, w, out=c, epilogue=ops.FK_EPI_SCALE, alpha=0.375)
        elif epi == "res":
            ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_RES, res=res)
        elif epi == "gate_res":
            ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_GATE_RES, res=res, gate=gate)
        else:
            ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_GELU_TANH if epi == "gelu" else ops.FK_EPI_SILU)
        return [buf]

    _both(ops, variant, 16, (5, 8), call, f"{epi} form {variant}")


@pytest.mark.parametrize("variant", (256, 384))
def test_fused_qkv_epilogue_with_a_token_offset(ops, variant):
    """H = 2 heads (N = 3 x 256), B = 2 batches of 384 tokens (a batch ends inside the second row tile) behind s_offset = 70 of
    S_total = 454: q, k and the v third of C."""
    H, B, Rr, K, s_off = 2, 2, 384, 192, 70
    D, S_total = H * 128, s_off + Rr
    a, w, bias = _rand((B, Rr, K), 60), _rand((3 * D, K), 61, 0.06), _rand((3 * D,), 62, 0.1)
    wq, wk = 1 + _rand((128,), 63, 0.1), 1 + _rand((128,), 64, 0.1)
    ang = torch.rand(S_total, 64, generator=torch.Generator().manual_seed(65)) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous().cuda()

    def call(bufs=None):
        q = torch.full((B, H, S_total, 128), SENTINEL, dtype=BF, device="cuda")
        k = torch.full_like(q, SENTINEL)
        buf, idx, c = R.guarded((B, Rr), 3 * D, device="cuda")
        ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_QKV, qkv=dict(q_out=q, k_out=k, wq=wq, wk=wk, cs=cs, s_offset=s_off))
        return [buf, q, k]

    _both(ops, variant, 16, (3, 4) if variant == 256 else (5, 8), call, f"fused QKV form {variant}")


@pytest.mark.parametrize("cap", (5, 8, 16))
def test_mixed_grid_big_then_small_on_one_workgroup(ops, cap):
    """M = 768, N = 1024 forced mixed: big and small tiles in one launch (module docstring), K = 64 and 320."""
    M, N = 768, 1024
    for K in (64, 320):
        a, w, bias = _rand((M, K), 70), _rand((N, K), 71, 0.05), _rand((N,), 72)

        def call(bufs=None):
            buf, idx, c = R.guarded(M, N, device="cuda")
            ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_GELU_TANH)
            return [buf]

        _both(ops, 384, 16, (cap,), call, f"mixed K {K}")


@pytest.mark.parametrize("variant", (256, 384))
def test_repeat_launch_on_the_same_buffers(ops, variant):
    M, N, K = 768, 1024, 192
    a, w, bias = _rand((M, K), 80), _rand((N, K), 81, 0.05), _rand((N,), 82)
    idx = R.guarded_shape(M, N)[1]

    def call(bufs=None):
        buf = R.guarded(M, N, device="cuda")[0] if bufs is None else bufs[0]
        ops.gemm(a, w, bias, out=buf[idx])
        return [buf]

    _both(ops, variant, 16, (3, 8), call, f"repeat form {variant}", repeat=True)


def test_flagship_grids_with_one_workgroup_per_cu(ops):
    """cap 0 (one workgroup per CU) at the 512^2 edit's MLP-up (2560 x 12288 x 3072, GELU: 480 tiles) and fused-QKV grid
    (2560 x 9216 x 3072, 24 heads: the launch plan's own mixed grid): the form reported stays 256 / 384, the bytes the old form's."""
    M, K = 2560, 3072
    a = _rand((M, K), 90)
    w, bias = _rand((12288, K), 91, 0.02), _rand((12288,), 92)

    def mlp_up(bufs=None):
        buf, idx, c = R.guarded(M, 12288, device="cuda")
        ops.gemm(a, w, bias, out=c, epilogue=ops.FK_EPI_GELU_TANH)
        return [buf]

    _both(ops, 0, 0, (0,), mlp_up, "MLP-up", expect=256)
    H, s_off = 24, 512
    wq, wk = 1 + _rand((128,), 93, 0.1), 1 + _rand((128,), 94, 0.1)
    ang = torch.rand(s_off + M, 64, generator=torch.Generator().manual_seed(95)) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous().cuda()

    def qkv(bufs=None):
        q = torch.full((1, H, s_off + M, 128), SENTINEL, dtype=BF, device="cuda")
        k = torch.full_like(q, SENTINEL)
        buf, idx, c = R.guarded((1, M), 9216, device="cuda")      # rows of one batch: the epilogue takes a row's token from c's batching
        ops.gemm(a.view(1, M, K), w[:9216], bias[:9216], out=c, epilogue=ops.FK_EPI_QKV, qkv=dict(q_out=q, k_out=k, wq=wq, wk=wk, cs=cs, s_offset=s_off))
        return [buf, q, k]

    _both(ops, 0, 0, (0,), qkv, "fused QKV", expect=384)
