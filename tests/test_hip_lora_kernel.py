"""fk_lora_merge_bf16 on the GPU against tests/lora_ref.py: the fp64 merge within the bound derived there, exact cases at
0 ulp, the in-place form, strided views with guards, untouched inputs and every refusal.

Observed worst |out - ref| / bound on an MI355X: 0.9949 over the ten shapes (N = 3072, K = 64, r = 16), 0.9893 over the
mixed-rank cases -- the bf16 rounding's half ulp, 2^-8 |ref| just above a power of two, is nearly all of it; the smallest is
0.4643 at (1, 8, 1).  The three-trip ranks: 0.9870 at (65, 136, 65), 0.9769 at (128, 64, 96), 0.9583 / 0.9762 with the ranks
(96, 5, 80, 33)."""
import ctypes

import pytest
import torch

import lora_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from gpt_image_edit_amd import ops
    return ops


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_merge_against_fp64(ops, N, K, r):
    base, terms = R.data(N, K, (r,), seed=N + K + r, device=DEV)
    keep = [t.clone() for t in (base, terms[0][0], terms[0][1])]
    out = ops.lora_merge(base, terms, out=torch.empty_like(base))
    R.check("out of place", out, base, terms)
    assert all(torch.equal(a, b) for a, b in zip(keep, (base, terms[0][0], terms[0][1]))), "an input was written"
    merged = ops.lora_merge(base, terms)               # in place: the same bits
    assert merged.data_ptr() == base.data_ptr() and torch.equal(merged, out)


@pytest.mark.parametrize("n_terms", [1, 2, 3, 4])
@pytest.mark.parametrize("N,K", [(65, 136), (128, 64)])
def test_mixed_ranks_and_negative_scales(ops, N, K, n_terms):
    base, terms = R.data(N, K, R.MIXED_RANKS[:n_terms], seed=7 * n_terms, device=DEV)
    assert n_terms < 2 or terms[1][2] < 0
    R.check(f"{n_terms} terms", ops.lora_merge(base, terms, out=torch.empty_like(base)), base, terms)


@pytest.mark.parametrize("N,K", [(65, 136), (128, 64)])
def test_mixed_ranks_with_a_rank_96_term(ops, N, K):
    """(96, 5, 80, 33): three trips of the r_pad loop, one, three again, two -- the trip count changes from term to term."""
    base, terms = R.data(N, K, R.MIXED_RANKS_96, seed=7 * 96, device=DEV)
    assert terms[1][2] < 0
    R.check("4 terms, 96 first", ops.lora_merge(base, terms, out=torch.empty_like(base)), base, terms)


@pytest.mark.parametrize("N,K,ranks", [(1, 8, (1,)), (16, 32, (32,)), (63, 72, (5,)), (65, 136, (33,)), (128, 64, (128,)),
                                       (65, 136, R.MIXED_RANKS), (130, 200, (128, 5, 33)), (64, 3072, (16, 32)),
                                       (3072, 64, (16,)), (63, 72, (80,)), (130, 200, (96, 5, 65))])
def test_exact_cases_are_0_ulp(ops, N, K, ranks):
    base, terms = R.exact_data(N, K, ranks, seed=N + K, device=DEV)
    want = R.exact_merge(base, terms)
    assert not torch.equal(want, base)
    out = ops.lora_merge(base, terms, out=torch.empty_like(base))
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(ops.lora_merge(base, terms).view(torch.int16), want.view(torch.int16))


def test_all_scales_zero_gives_base(ops):
    base, terms = R.data(65, 136, (5, 33), seed=5, device=DEV)
    base[3, 5] = -0.0
    zero = [(up, down, 0.0) for up, down, _ in terms]
    out = ops.lora_merge(base, zero, out=torch.full_like(base, 9.0))
    assert torch.equal(out, base) and torch.equal(out.view(torch.int16), base.view(torch.int16))
    keep = base.clone()
    ops.lora_merge(base, zero)
    assert torch.equal(base.view(torch.int16), keep.view(torch.int16))
    # a zero term among others adds nothing
    mixed = [terms[0], (terms[1][0], terms[1][1], 0.0)]
    assert torch.equal(ops.lora_merge(base, mixed, out=torch.empty_like(base)), ops.lora_merge(base, terms[:1], out=torch.empty_like(base)))


@pytest.mark.parametrize("pad", [8, 3])       # row strides that keep / break the 16-byte alignment of the rows
@pytest.mark.parametrize("N,K", [(63, 72), (65, 136)])
def test_strided_views_and_guards(ops, N, K, pad, ranks=(5, 33)):
    base0, terms0 = R.exact_data(N, K, ranks, seed=pad + N, device=DEV)
    want = R.exact_merge(base0, terms0)
    S = 7.0                                   # sentinel
    big_base = torch.full((N + 2, K + pad + 8), S, device=DEV, dtype=BF16)
    big_out = torch.full((N + 2, K + pad + 8), S, device=DEV, dtype=BF16)
    base = big_base[1:N + 1, 8:8 + K]
    out = big_out[1:N + 1, 8:8 + K]
    base.copy_(base0)
    terms = []
    for up0, down0, s in terms0:              # strided adapters too
        up = torch.full((N, up0.shape[1] + pad), S, device=DEV, dtype=BF16)[:, :up0.shape[1]]
        down = torch.full((down0.shape[0], K + pad), S, device=DEV, dtype=BF16)[:, :K]
        up.copy_(up0), down.copy_(down0)
        terms.append((up, down, s))
    keep_base = big_base.clone()
    ops.lora_merge(base, terms, out=out)
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(big_base, keep_base)
    guard = big_out.clone()
    guard[1:N + 1, 8:8 + K] = S
    assert bool((guard == S).all()), "a sentinel column or guard row around out was written"
    ops.lora_merge(base, terms)               # in place in the strided view
    assert torch.equal(base.view(torch.int16), want.view(torch.int16))
    keep_base[1:N + 1, 8:8 + K] = S
    chk = big_base.clone()
    chk[1:N + 1, 8:8 + K] = S
    assert torch.equal(chk, keep_base)


@pytest.mark.parametrize("pad", [8, 3])
def test_strided_views_and_guards_at_rank_80(ops, pad):
    """The same views with a three-trip term between a one-trip and a two-trip one."""
    test_strided_views_and_guards(ops, 65, 136, pad, ranks=(5, 80, 33))


def test_refusals_write_nothing(ops):
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    N, K, r = 16, 32, 8
    base, terms = R.data(N, K, (r,), seed=1, device=DEV)
    up, down, _ = terms[0]
    out = torch.full((N, K), 5.0, device=DEV, dtype=BF16)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    T = libfk.LoraTerm

    def term(up_p=up.data_ptr(), ld_up=r, down_p=down.data_ptr(), ld_down=K, rank=r, scale=1.0):
        return T(up_p, ld_up, down_p, ld_down, rank, scale)

    def call(base_p=base.data_ptr(), ld_base=K, out_p=out.data_ptr(), ld_out=K, n=N, k=K, ts=None, n_terms=None, null_terms=False):
        ts = [term()] if ts is None else ts
        arr = (T * max(len(ts), 1))(*ts)
        return lib.fk_lora_merge_bf16(ctypes.c_void_p(base_p), ld_base, ctypes.c_void_p(out_p), ld_out, n, k,
                                      None if null_terms else arr, len(ts) if n_terms is None else n_terms, st)

    EINVAL, EUNSUP = -1, -2
    cases = [
        ("N = 0", dict(n=0), EINVAL), ("K = 0", dict(k=0), EINVAL), ("K % 8", dict(k=28), EINVAL), ("K < 8", dict(k=4), EINVAL),
        ("ld_base < K", dict(ld_base=K - 8), EINVAL), ("ld_out < K", dict(ld_out=K - 1), EINVAL),
        ("null base", dict(base_p=0), EINVAL), ("null out", dict(out_p=0), EINVAL), ("null terms", dict(null_terms=True), EINVAL),
        ("null up", dict(ts=[term(up_p=0)]), EINVAL), ("null down", dict(ts=[term(down_p=0)]), EINVAL),
        ("ld_up < rank", dict(ts=[term(ld_up=r - 1)]), EINVAL), ("ld_down < K", dict(ts=[term(ld_down=K - 1)]), EINVAL),
        ("rank 0", dict(ts=[term(rank=0)]), EUNSUP), ("rank 129", dict(ts=[term(rank=129, ld_up=129)]), EUNSUP),
        ("no terms", dict(ts=[], n_terms=0), EUNSUP), ("5 terms", dict(ts=[term()] * 5), EUNSUP),
        ("out overlaps base", dict(out_p=base.data_ptr() + 16), EINVAL),
        ("second term bad", dict(ts=[term(), term(rank=0)]), EUNSUP),
    ]
    keep = base.clone()
    for name, kw, want in cases:
        code = call(**kw)
        assert code == want, (name, code)
        assert lib.fk_last_error().decode().startswith("fk_lora_merge_bf16"), name
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and torch.equal(base, keep)
    assert call() == 0                      # the same arguments, valid: it does run
    R.check("after the refusals", out, base, [(up, down, 1.0)])
    with pytest.raises(ValueError):
        ops.lora_merge(base, [(up, down[:, :K - 8], 1.0)])
    with pytest.raises(ValueError):
        ops.lora_merge(base.float(), [(up, down, 1.0)])
    with pytest.raises(RuntimeError, match="fk_lora_merge_bf16"):
        ops.lora_merge(base, [(up, down, 1.0)] * 5)
