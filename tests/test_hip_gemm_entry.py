"""The large-tile GEMMs after their workgroup entry became launch constants (csrc/gemm_tile_map.h): every launch form finds
the tiles it found before, and flat / batched row addressing reach the same elements.

Inputs are small integers in bf16, so every partial sum is an integer below 2^24 and exact in fp32 in any order; the expected
values are an fp64 matmul on the CPU (rounded once to bf16, as the kernels' store does) and the assertion is EQUALITY.  C lies
inside a larger buffer pre-filled with a sentinel: the guard rows and columns around it must come back untouched, and every
element of C must have been written (the expected values never equal the sentinel).  The two fused epilogues that cannot be
exact (RMSNorm + RoPE, gate * y) run against the unfused kernels the existing tests use, bit for bit.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = -24832.0          # a bf16 value no expected output takes: |acc + bias| <= 4 K + 4 <= 24580 in these cases
GUARD_ROWS, GUARD_COLS = 3, 8     # columns: a multiple of 8 keeps C's row starts 16-byte aligned


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


def _ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(BF)


def _expected(a, w, bias):
    """bf16(fp64 a @ w^T + bias): the sums are integers below 2^24, so the fp32 accumulators hold them exactly."""
    y = a.double().reshape(-1, a.shape[-1]) @ w.double().T + bias.double()
    assert y.abs().max().item() < 2 ** 24 and (y != SENTINEL).all()
    return y.to(torch.float32).to(BF)


class _Launch:
    """Forced launch controls for one call, restored afterwards."""

    def __init__(self, ops, variant=0, group_m=0, exchange="default"):
        self.ops, self.variant, self.group_m, self.exchange = ops, variant, group_m, exchange

    def __enter__(self):
        self.ops.gemm_set_variant(self.variant)
        self.ops.gemm_set_group_m(self.group_m)
        self.ops.gemm_set_splitk_exchange(self.exchange)

    def __exit__(self, *exc):
        self.ops.gemm_set_variant(0)
        self.ops.gemm_set_group_m(0)
        self.ops.gemm_set_splitk_exchange("default")


def _guarded(M, N):
    """(whole buffer, the [M, N] view C inside it)."""
    buf = torch.full((M + 2 * GUARD_ROWS, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
    return buf, buf[GUARD_ROWS:GUARD_ROWS + M, GUARD_COLS:GUARD_COLS + N]


def _check_guarded(buf, M, N, want, what):
    got = buf.cpu()
    inner = got[GUARD_ROWS:GUARD_ROWS + M, GUARD_COLS:GUARD_COLS + N]
    assert torch.equal(inner, want), f"{what}: {(inner != want).sum().item()} of {M * N} elements differ from the fp64 product"
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[GUARD_ROWS:GUARD_ROWS + M, GUARD_COLS:GUARD_COLS + N] = False
    assert (got[mask] == SENTINEL).all(), f"{what}: the guard band around C was written"


# (M, N, K, variant forced, the form that must report, group_m)
PLAIN = [
    (300, 384, 128, 128, 128, 0),       # 256 x 128 kernel, ragged both ways
    (520, 512, 192, 256, 256, 0),       # 256 x 256 kernel, ragged rows
    (700, 1280, 128, 128, 128, 1), (700, 1280, 128, 128, 128, 8), (700, 1280, 128, 128, 128, 64),
    (700, 1280, 128, 256, 256, 1), (700, 1280, 128, 256, 256, 8), (700, 1280, 128, 256, 256, 64),
    (512, 768, 128, 384, 384, 0),       # mixed grid: big_cols 1 (the only split of 3 column tiles that leaves >= 8 small tiles)
    (512, 512, 256, 1024, 1024, 0),     # the 4-wave hand-placed 256 x 256 kernel
]


@pytest.mark.parametrize("M,N,K,variant,reports,group_m", PLAIN)
def test_every_launch_form_finds_its_tiles(ops, M, N, K, variant, reports, group_m):
    a, w, bias = _ints((M, K), -2, 2, 1000 + M), _ints((N, K), -2, 2, 2000 + N), _ints((N,), -4, 4, 3000 + K)
    want = _expected(a, w, bias)
    buf, c = _guarded(M, N)
    with _Launch(ops, variant, group_m):
        ops.gemm(a.cuda(), w.cuda(), bias.cuda(), out=c)
        torch.cuda.synchronize()
        assert ops.gemm_last_variant() == reports
    _check_guarded(buf, M, N, want, f"M {M} N {N} K {K} variant {variant} group_m {group_m}")


@pytest.mark.parametrize("exchange", ["default", "whole", "unannounced"])
def test_splitk_pairs_find_their_tiles_and_slots(ops, exchange):
    M, N, K = 256, 512, 6144
    a, w, bias = _ints((M, K), -2, 2, 11), _ints((N, K), -2, 2, 12), _ints((N,), -4, 4, 13)
    want = _expected(a, w, bias)
    buf, c = _guarded(M, N)
    with _Launch(ops, 512, 0, exchange):
        ops.gemm(a.cuda(), w.cuda(), bias.cuda(), out=c)      # ops.gemm attaches the stream's split-K workspace at K >= 6144
        torch.cuda.synchronize()
        assert ops.gemm_last_variant() == 512
    _check_guarded(buf, M, N, want, f"split-K pairs, {exchange} exchange")


@pytest.mark.parametrize("variant", [128, 256])
@pytest.mark.parametrize("B", [2, 1])
def test_grouped_slices_of_a_joint_buffer(ops, B, variant):
    """Two problems on the text / image slices of one joint [B, S = 160, ld] buffer, S_img = 136, S_txt = 24.  B = 2: the rows
    of a batch end in the middle of a tile and the next batch starts after a gap -- the batched addressing; B = 1: the same
    views are flat.  Input and output both live in such buffers; everything outside the two C slices must stay untouched."""
    S_img, S_txt, N, K = 136, 24, 256, 128
    S = S_img + S_txt
    x = _ints((B, S, K + 8), -2, 2, 21)[:, :, :K]          # ld = K + 8: rows with a stride of their own
    w_i, w_t = _ints((N, K), -2, 2, 22), _ints((N, K), -2, 2, 23)
    b_i, b_t = _ints((N,), -4, 4, 24), _ints((N,), -4, 4, 25)
    xd = torch.zeros(B, S, K + 8, dtype=BF, device="cuda")
    xd[:, :, :K] = x.cuda()
    xv = xd[:, :, :K]
    out = torch.full((B, S + 1, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")    # one guard row per batch, guard columns
    ov = out[:, :S, GUARD_COLS:GUARD_COLS + N]
    with _Launch(ops, variant):
        ops.gemm_grouped([dict(a=xv[:, S_txt:], w=w_i.cuda(), bias=b_i.cuda(), out=ov[:, S_txt:]),
                          dict(a=xv[:, :S_txt], w=w_t.cuda(), bias=b_t.cuda(), out=ov[:, :S_txt])])
        torch.cuda.synchronize()
        assert ops.gemm_last_variant() == variant
    got = out.cpu()
    want_i = _expected(x[:, S_txt:].contiguous(), w_i, b_i).view(B, S_img, N)
    want_t = _expected(x[:, :S_txt].contiguous(), w_t, b_t).view(B, S_txt, N)
    inner = got[:, :S, GUARD_COLS:GUARD_COLS + N]
    assert torch.equal(inner[:, S_txt:], want_i), f"image slice, B {B}: {(inner[:, S_txt:] != want_i).sum().item()} elements differ"
    assert torch.equal(inner[:, :S_txt], want_t), f"text slice, B {B}: {(inner[:, :S_txt] != want_t).sum().item()} elements differ"
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[:, :S, GUARD_COLS:GUARD_COLS + N] = False
    assert (got[mask] == SENTINEL).all(), "the guard band around the C slices was written"


@pytest.mark.parametrize("B", [2, 1])
def test_fused_qkv_epilogue_against_the_unfused_kernels(ops, B):
    """FK_EPI_QKV at H = 1 (N = 384): the q / k thirds need a row's batch and token (B = 2: from the batched addressing, B = 1:
    flat rows), the v third is stored in place.  Against the projection followed by fk_qkv_post_bf16, bit for bit."""
    from oracle import mmdit
    from oracle.helpers import prepare_latent_image_ids
    H, S_txt, hh, ww, K = 1, 20, 12, 15, 128
    S, D = S_txt + hh * ww, H * 128
    g = torch.Generator().manual_seed(31 + B)
    x = torch.randn(B, S, K, generator=g).to(BF).cuda()
    w = (torch.randn(3 * D, K, generator=g) * 0.06).to(BF).cuda()
    b = (torch.randn(3 * D, generator=g) * 0.1).to(BF).cuda()
    nq, nk_ = [(1 + torch.randn(128, generator=g) * 0.1).to(BF).cuda() for _ in range(2)]
    ids = torch.cat([torch.zeros(S_txt, 3), prepare_latent_image_ids(hh, ww)])
    cos, sin = (t.cuda() for t in mmdit.rope_tables(ids))
    plain = ops.gemm(x, w, b)
    q_ref = torch.empty(B, H, S, 128, dtype=BF, device="cuda")
    k_ref = torch.empty_like(q_ref)
    ops.qkv_post(plain, q_ref, k_ref, nq, nk_, None, None, cos, sin, 0)
    q, k = torch.full_like(q_ref, SENTINEL), torch.full_like(q_ref, SENTINEL)
    fused = torch.full((B, S, 3 * D), SENTINEL, dtype=BF, device="cuda")
    ops.gemm(x, w, b, out=fused, epilogue=ops.FK_EPI_QKV, qkv=dict(q_out=q, k_out=k, wq=nq, wk=nk_, cos=cos, sin=sin, s_offset=0))
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == 128
    assert torch.equal(q, q_ref) and torch.equal(k, k_ref)
    assert torch.equal(fused[:, :, 2 * D:], plain[:, :, 2 * D:])
    assert (fused[:, :, :2 * D] == SENTINEL).all(), "the q / k thirds of C are not stored by the fused epilogue"


@pytest.mark.parametrize("variant", [128, 256])
@pytest.mark.parametrize("B", [2, 1])
def test_gated_residual_epilogue_with_a_batched_gate(ops, B, variant):
    """FK_EPI_GATE_RES on slices of joint buffers, the gate one row per batch: B = 2 -- A, C, the residual and the gate all
    take the batched addressing (a batch ends inside a tile); B = 1 -- all flat.  Against the plain GEMM followed by
    fk_gate_res_fwd_bf16, bit for bit."""
    R, S_txt, N, K = 300 // B, 10, 256, 128
    g = torch.Generator().manual_seed(41 + B)
    a = torch.randn(B, S_txt + R, K, generator=g).to(BF).cuda()[:, S_txt:]
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF).cuda()
    bias = torch.randn(N, generator=g).to(BF).cuda()
    res = (torch.randn(B, S_txt + R, N, generator=g) * 2).to(BF).cuda()[:, S_txt:]
    gate = (torch.randn(B, 3 * N, generator=g) * 0.7).to(BF).cuda()[:, N:2 * N]
    with _Launch(ops, variant):
        plain = torch.zeros(B, S_txt + R, N + 64, device="cuda", dtype=BF)[:, S_txt:, :N]
        ops.gemm(a, w, bias, out=plain)
        out = torch.full((B, S_txt + R, N + 2 * GUARD_COLS), SENTINEL, dtype=BF, device="cuda")
        ov = out[:, S_txt:, GUARD_COLS:GUARD_COLS + N]
        ops.gemm(a, w, bias, out=ov, epilogue=ops.FK_EPI_GATE_RES, res=res, gate=gate)
        torch.cuda.synchronize()
        assert ops.gemm_last_variant() == variant
    want = torch.empty(B, R, N, dtype=BF, device="cuda")
    ops.gate_res_fwd(res, plain, gate, want)
    torch.cuda.synchronize()
    assert torch.equal(ov, want), f"{(ov != want).sum().item()} elements differ from plain GEMM + gate_res_fwd"
    got = out.cpu()
    mask = torch.ones_like(got, dtype=torch.bool)
    mask[:, S_txt:, GUARD_COLS:GUARD_COLS + N] = False
    assert (got[mask] == SENTINEL).all(), "the guard band around C was written"
