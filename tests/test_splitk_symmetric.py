"""Split-K pairs (variant 512): the symmetric exchange -- each workgroup of a pair finishes 128 rows of the tile -- against
the one-way exchange it replaces as the default and against the unsplit 256 x 256 grid (variant 256).

What can be bit-identical, and why:
  * symmetric / its fallback ("unannounced") vs the one-way exchange: always.  Every output element is fp32 own + other
    of the same two half-K sums, and fp32 addition commutes; which workgroup forms the sum must not show.  Asserted on
    random inputs and on exact ones.
  * split vs unsplit (variant 256): the two add the same products in a different ASSOCIATION (two half-K chains joined
    once, against one chain), so with inputs whose partial sums round they differ in the last fp32 bits -- for any split-K
    whatever its exchange (include/fk.h says so of the form since it exists) -- and a small fraction of the bf16 outputs
    lands on the neighbouring value.  The comparison is therefore asserted bit for bit on inputs whose every partial sum
    is an integer below 2^24 (exact in fp32 in any association: small-integer activations and weights), where it checks
    what the exchange can get wrong -- a piece of the tile added twice, not at all, or to the wrong place --, and on the
    random inputs the distance is printed and held to 2^-5 of the output scale.
Every form runs twice per case: which workgroup of a pair finishes first differs from run to run, the result must not.
"""
import pytest
import torch

from conftest import bf16_ulp_diff

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
EXCHANGES = ("whole", "symmetric", "unannounced")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


def _inputs(B, R, N, K, exact, seed):
    g = torch.Generator().manual_seed(seed)
    if exact:       # |a|, |w| <= 2: every partial sum is an integer of magnitude <= 4 K < 2^24
        a = torch.randint(-2, 3, (B, R, K), generator=g).to(BF)
        w = torch.randint(-2, 3, (N, K), generator=g).to(BF)
        bias = torch.randint(-4, 5, (N,), generator=g).to(BF)
    else:
        a = torch.randn(B, R, K, generator=g).to(BF)
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF)
        bias = (torch.randn(N, generator=g) * 0.1).to(BF)
    gate = torch.randn(B, N, generator=g).to(BF)
    res = torch.randn(B, R, N, generator=g).to(BF)
    return [t.cuda() for t in (a, w, bias, gate, res)]


def _run(ops, variant, exchange, a, w, bias, gate, res, epi):
    ops.gemm_set_variant(variant)
    ops.gemm_set_splitk_exchange(exchange)
    try:
        if epi == "gate_res":
            out = ops.gemm(a, w, bias, epilogue=ops.FK_EPI_GATE_RES, res=res, gate=gate)
        else:
            out = ops.gemm(a, w, bias)
        torch.cuda.synchronize()
        return out, ops.gemm_last_variant()
    finally:
        ops.gemm_set_variant(0)
        ops.gemm_set_splitk_exchange("default")


# M = B * R: 2560 as the 512^2 edit runs it (both K-long classes), and a ragged one (2401 = 9 * 256 + 97)
@pytest.mark.parametrize("epi", ["gate_res", "none"])
@pytest.mark.parametrize("B,R,N,K", [(2, 1280, 3072, 12288), (2, 1280, 3072, 15360), (1, 2401, 3072, 12288)])
def test_symmetric_exchange_gives_the_bits_of_the_one_way_exchange_and_of_the_unsplit_grid(ops, B, R, N, K, epi):
    for exact in (True, False):
        t = _inputs(B, R, N, K, exact, seed=311 + K // 1024 + R)
        unsplit, v = _run(ops, 256, "default", *t, epi)
        assert v == 256
        one_way, v = _run(ops, 512, "whole", *t, epi)
        assert v == 512
        assert torch.isfinite(one_way.float()).all()
        ulp = bf16_ulp_diff(one_way.cpu(), unsplit.cpu())
        print(f"[splitk] M={B * R} K={K} {epi} {'exact' if exact else 'random'} inputs: one-way split vs unsplit: "
              f"{(ulp != 0).float().mean().item():.3e} of the elements differ, max {int(ulp.max())} bf16 ulp", flush=True)
        if exact:
            assert torch.equal(one_way, unsplit), "split-K (one-way exchange) vs the unsplit grid on exact inputs"
        else:
            # y differs by at most one bf16 ulp (2^-7 |y|); gate * y, its rounding and the rounding of res + gate * y add
            # one each: well inside 2^-5 of the output scale (an ulp count says nothing here: res + gate * y cancels)
            d = (one_way.float() - unsplit.float()).abs().max().item()
            scale = unsplit.float().abs().max().item()
            print(f"[splitk]   max |d| = {d:.3e} at output scale {scale:.3e}", flush=True)
            assert d <= 2.0 ** -5 * scale
        for exchange in EXCHANGES:
            for run in range(2):
                got, v = _run(ops, 512, exchange, *t, epi)
                assert v == 512
                same = torch.equal(got, one_way)
                print(f"[splitk] M={B * R} K={K} {epi} {'exact' if exact else 'random'} {exchange} run {run}: "
                      f"{'identical to' if same else 'DIFFERS from'} the one-way exchange", flush=True)
                assert same, f"{exchange} exchange, run {run}: not the bits of the one-way exchange"
                if exact:
                    assert torch.equal(got, unsplit), f"{exchange} exchange, run {run}: not the bits of the unsplit grid"


def test_symmetric_exchange_on_the_fp32_accumulators(ops):
    """The raw fp32 sums (out_fp32 = 2: acc + bias stored from the accumulator registers by the same main loop and the same
    rendezvous): every exchange bit for bit the one-way exchange's, on random inputs."""
    a, w, bias, _, _ = _inputs(1, 2401, 3072, 12288, False, seed=97)
    got = {}
    for exchange in EXCHANGES:
        for run in range(2):
            ops.gemm_set_variant(512)
            ops.gemm_set_splitk_exchange(exchange)
            try:
                out = ops.gemm(a[0], w, bias, out_fp32=2)
                torch.cuda.synchronize()
                assert ops.gemm_last_variant() == 512
            finally:
                ops.gemm_set_variant(0)
                ops.gemm_set_splitk_exchange("default")
            got[(exchange, run)] = out
    ref = got[("whole", 0)]
    torch.testing.assert_close(ref.cpu(), (a[0].double() @ w.double().T + bias.double()).float().cpu(), rtol=1e-3, atol=1e-4)
    for key, out in got.items():
        assert torch.equal(out, ref), key


def test_planner_keeps_its_classes(ops):
    """The launch plan with the symmetric exchange's measured price: the two K-long classes of the 512^2 edit still run as
    split-K pairs, their 1024^2 counterparts (408 tiles) never do, and the K = 3072 out-projection stays a plain grid."""
    for (M, N, K, want) in [(2560, 3072, 12288, {512}), (2560, 3072, 15360, {512}), (8704, 3072, 12288, {256, 1024}),
                            (8704, 3072, 15360, {256, 1024}), (2560, 3072, 3072, {128})]:
        g = torch.Generator().manual_seed(5)
        a, w = torch.randn(M, K, generator=g).to(BF).cuda(), (torch.randn(N, K, generator=g) * 0.05).to(BF).cuda()
        ops.gemm(a, w)
        torch.cuda.synchronize()
        assert ops.gemm_last_variant() in want, (M, N, K, ops.gemm_last_variant())


def test_two_exchanges_in_one_call_are_rejected(ops):
    a, w = torch.zeros(256, 6144, dtype=BF).cuda(), torch.zeros(256, 6144, dtype=BF).cuda()
    ops._set_launch(gemm_splitk=16 | 32)
    try:
        with pytest.raises(Exception, match="plan"):
            ops.gemm(a, w)
    finally:
        ops.gemm_set_splitk_exchange("default")
