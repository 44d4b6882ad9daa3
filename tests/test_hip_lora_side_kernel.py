"""fk_lora_side_grad_bf16 on the GPU against tests/lora_side_ref.py: the fp64 gradient within the bound derived there, integer
cases at 0 ulp, batched views whose batch stride exceeds R * ld, dY as a column block of a wider buffer with aligned and with
odd strides, accumulate onto old values and overwrite onto NaN bits, guards around both outputs and the workspace's claimed
size, two launches bit-identical, untouched inputs and every refusal.

Observed worst |out - ref| / bound on an MI355X (one run): 0.083 over the nine shapes and the production one ((1, 64, 16, 32, 32),
d_down), 4e-5 at the production shape; the rank tile of 96 (d_up / d_down): 0.0191 / 0.0165 at r = 65, 0.0259 / 0.0157 at
r = 80, 0.0228 / 0.0119 at r = 96; accumulate at r = 80: 0.0265 / 0.016."""
import ctypes

import pytest
import torch

import lora_side_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
G = 64                                        # guard floats in front of and behind an output or the workspace
S = 777.0                                     # sentinel


@pytest.fixture(scope="module")
def ops():
    from gpt_image_edit_amd import ops
    return ops


def guarded(n, shape=None):
    """(flat fp32 buffer of sentinels, its contiguous middle of n elements, viewed as ``shape``)."""
    big = torch.full((2 * G + n,), S, device=DEV, dtype=torch.float32)
    mid = big[G:G + n]
    return big, mid if shape is None else mid.view(*shape)


def guards_intact(big):
    return bool((big[:G] == S).all()) and bool((big[-G:] == S).all())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def run_guarded(ops, x, dy, up, down, s, ws_shift=0):
    """One call with guards around d_up, d_down and exactly fk_lora_side_grad_ws_floats of workspace (``ws_shift`` floats off
    the allocation's alignment); returns the outputs."""
    from gpt_image_edit_amd import libfk
    B, R_, K = x.shape if x.dim() == 3 else (1, *x.shape)
    N, r = up.shape
    need = libfk.load().fk_lora_side_grad_ws_floats(B, R_, N, K, r)
    assert need > 0
    big_u, d_up = guarded(N * r, (N, r))
    big_d, d_down = guarded(r * K, (r, K))
    big_w = torch.full((2 * G + need + ws_shift,), S, device=DEV, dtype=torch.float32)
    ws = big_w[G + ws_shift:G + ws_shift + need]
    ops.lora_side_grad(x, dy, up, down, s, d_up=d_up, d_down=d_down, ws=ws)
    assert guards_intact(big_u) and guards_intact(big_d), "a guard around an output was written"
    assert bool((big_w[:G + ws_shift] == S).all()) and bool((big_w[G + ws_shift + need:] == S).all()), "the workspace's claimed size was exceeded"
    return d_up, d_down


@pytest.mark.parametrize("shape", R.SHAPES + [R.PRODUCTION])
def test_gradient_against_fp64(ops, shape):
    x, dy, up, down, s = R.data(*shape, seed=sum(shape), device=DEV)
    keep = [t.clone() for t in (x, dy, up, down)]
    d_up, d_down = run_guarded(ops, x, dy, up, down, s)
    R.check("random", d_up, d_down, x, dy, up, down, s)
    assert all(torch.equal(a, b) for a, b in zip(keep, (x, dy, up, down))), "an input was written"
    again = ops.lora_side_grad(x, dy, up, down, s)              # fresh outputs, a fresh workspace: the same bits
    assert same_bits(again[0], d_up) and same_bits(again[1], d_down)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_integer_cases_are_0_ulp(ops, shape):
    x, dy, up, down, s = R.exact_data(*shape, seed=shape[2] + shape[3], device=DEV)
    fu, fd = R.exact_grads(x, dy, up, down, s)
    d_up, d_down = run_guarded(ops, x, dy, up, down, s, ws_shift=1)        # a workspace that is only 4-byte aligned
    assert torch.equal(d_up, fu) and torch.equal(d_down, fd)


def test_batch_stride_larger_than_the_rows(ops):
    """(2, 96, 128, 64, 128): x and dy as the image rows [32, 128) of joint [B, 128, *] buffers -- not uniformly strided."""
    B, R_, N, K, r = 2, 96, 128, 64, 128
    x0, dy0, up, down, s = R.data(B, R_, N, K, r, seed=11, device=DEV)
    xj = torch.full((B, 128, K), 3.0, device=DEV, dtype=BF16)
    yj = torch.full((B, 128, N), 3.0, device=DEV, dtype=BF16)
    x, dy = xj[:, 32:], yj[:, 32:]
    x.copy_(x0), dy.copy_(dy0)
    assert x.stride(0) > R_ * x.stride(1)
    keep = (xj.clone(), yj.clone())
    d_up, d_down = run_guarded(ops, x, dy, up, down, s)
    R.check("joint buffer", d_up, d_down, x0, dy0, up, down, s)
    assert torch.equal(xj, keep[0]) and torch.equal(yj, keep[1])
    ref = ops.lora_side_grad(x0, dy0, up, down, s)              # the same rows, contiguous: the same order, the same bits
    assert same_bits(ref[0], d_up) and same_bits(ref[1], d_down)


@pytest.mark.parametrize("shape", [(1, 65, 131, 136, 33), (2, 70, 72, 40, 16), (2, 70, 72, 40, 80)])
@pytest.mark.parametrize("pad", [8, 3])       # strides that keep / break the 16-byte alignment of the rows
def test_column_block_of_a_wider_buffer(ops, shape, pad):
    """dY as columns [N, 2N) of a [B, R + 1, 3N + pad] buffer (dqkv[:, :, D:2D] is such a block), x and the factors strided."""
    B, R_, N, K, r = shape
    x0, dy0, up0, down0, s = R.exact_data(*shape, seed=N + pad, device=DEV)
    fu, fd = R.exact_grads(x0, dy0, up0, down0, s)
    wide = torch.full((B, R_ + 1, 3 * N + pad), 3.0, device=DEV, dtype=BF16)
    dy = wide[:, :R_, N:2 * N]
    dy.copy_(dy0)
    x = torch.full((B, R_ + 2, K + pad), 3.0, device=DEV, dtype=BF16)[:, 1:R_ + 1, :K]
    up = torch.full((N, r + pad), 3.0, device=DEV, dtype=BF16)[:, :r]
    down = torch.full((r, K + pad), 3.0, device=DEV, dtype=BF16)[:, :K]
    x.copy_(x0), up.copy_(up0), down.copy_(down0)
    keep = wide.clone()
    d_up, d_down = run_guarded(ops, x, dy, up, down, s)
    assert torch.equal(d_up, fu) and torch.equal(d_down, fd)
    assert torch.equal(wide, keep)
    if pad % 8:                               # one element off a 16-byte boundary as well
        off = torch.full((B * R_ * (K + pad) + 1,), 3.0, device=DEV, dtype=BF16)[1:].view(B, R_, K + pad)[:, :, :K]
        off.copy_(x0)
        ou, od = ops.lora_side_grad(off, dy, up, down, s)
        assert torch.equal(ou, fu) and torch.equal(od, fd)


@pytest.mark.parametrize("shape", [(1, 64, 16, 32, 32), (1, 129, 16, 8, 8), (2, 96, 128, 64, 128),   # unsplit, split, batched
                                   (2, 70, 72, 40, 80)])                                              # the rank tile of 96, split
def test_accumulate_and_overwrite(ops, shape):
    x, dy, up, down, s = R.data(*shape, seed=7, device=DEV)
    N, r = up.shape
    K = down.shape[1]
    g = torch.Generator().manual_seed(8)
    old = (torch.randn(N, r, generator=g).to(DEV), torch.randn(r, K, generator=g).to(DEV))
    big_u, d_up = guarded(N * r, (N, r))
    big_d, d_down = guarded(r * K, (r, K))
    d_up.copy_(old[0]), d_down.copy_(old[1])
    ops.lora_side_grad(x, dy, up, down, s, d_up=d_up, d_down=d_down, accumulate=True)
    R.check("accumulate", d_up, d_down, x, dy, up, down, s, old=old)
    assert guards_intact(big_u) and guards_intact(big_d)
    # accumulate = 0 never reads the outputs: NaN bits are overwritten by the bits of a fresh call
    fresh = ops.lora_side_grad(x, dy, up, down, s)
    d_up.fill_(float("nan")), d_down.fill_(float("nan"))
    ops.lora_side_grad(x, dy, up, down, s, d_up=d_up, d_down=d_down, accumulate=False)
    assert same_bits(d_up, fresh[0]) and same_bits(d_down, fresh[1])
    R.check("overwrite", d_up, d_down, x, dy, up, down, s)
    # accumulate onto zeros adds +0: the value of the overwrite
    d_up.zero_(), d_down.zero_()
    ops.lora_side_grad(x, dy, up, down, s, d_up=d_up, d_down=d_down, accumulate=True)
    assert torch.equal(d_up, fresh[0]) and torch.equal(d_down, fresh[1])


def test_refusals_write_nothing(ops):
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    B, R_, N, K, r = 2, 70, 24, 40, 8                 # M = 140: both reductions split
    x, dy, up, down, s = R.data(B, R_, N, K, r, seed=1, device=DEV)
    d_up = torch.full((N, r), S, device=DEV, dtype=torch.float32)
    d_down = torch.full((r, K), S, device=DEV, dtype=torch.float32)
    need = lib.fk_lora_side_grad_ws_floats(B, R_, N, K, r)
    assert need == 2 * N * r + 2 * r * K + 3 + 2 * 32 * 192
    assert lib.fk_lora_side_grad_ws_floats(B, R_, N, K, 80) == 2 * N * 80 + 2 * 80 * K + 3 + 2 * 96 * 192     # the rank padded to 96
    ws = torch.full((need,), S, device=DEV, dtype=torch.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    V = ctypes.c_void_p

    def call(x_p=x.data_ptr(), ld_x=K, bs_x=R_ * K, dy_p=dy.data_ptr(), ld_dy=N, bs_dy=R_ * N, b=B, rows=R_, n=N, k=K,
             up_p=up.data_ptr(), ld_up=r, down_p=down.data_ptr(), ld_down=K, rank=r, scale=1.0, du_p=d_up.data_ptr(),
             dd_p=d_down.data_ptr(), acc=0, ws_p=ws.data_ptr(), ws_n=need):
        return lib.fk_lora_side_grad_bf16(V(x_p), ld_x, bs_x, V(dy_p), ld_dy, bs_dy, b, rows, n, k, V(up_p), ld_up, V(down_p), ld_down,
                                          rank, scale, V(du_p), V(dd_p), acc, V(ws_p), ws_n, st)

    EINVAL, EUNSUP = -1, -2
    cases = [
        ("B = 0", dict(b=0), EINVAL), ("R = 0", dict(rows=0), EINVAL), ("N = 0", dict(n=0), EINVAL), ("K = 0", dict(k=0), EINVAL),
        ("rank 0", dict(rank=0), EUNSUP), ("rank 129", dict(rank=129, ld_up=129), EUNSUP), ("M beyond int32", dict(b=1 << 31), EUNSUP),
        ("ld_x < K", dict(ld_x=K - 1), EINVAL), ("ld_dy < N", dict(ld_dy=N - 1), EINVAL), ("ld_up < rank", dict(ld_up=r - 1), EINVAL),
        ("ld_down < K", dict(ld_down=K - 8), EINVAL), ("bs_x < 0", dict(bs_x=-1), EINVAL), ("bs_dy < 0", dict(bs_dy=-8), EINVAL),
        ("null x", dict(x_p=0), EINVAL), ("null dy", dict(dy_p=0), EINVAL), ("null up", dict(up_p=0), EINVAL),
        ("null down", dict(down_p=0), EINVAL), ("null d_up", dict(du_p=0), EINVAL), ("null d_down", dict(dd_p=0), EINVAL),
        ("null ws", dict(ws_p=0), EINVAL), ("ws too small", dict(ws_n=need - 1), EINVAL), ("scale inf", dict(scale=float("inf")), EINVAL),
        ("scale nan", dict(scale=float("nan")), EINVAL), ("accumulate 2", dict(acc=2), EINVAL), ("accumulate -1", dict(acc=-1), EINVAL),
        ("d_up overlaps d_down", dict(dd_p=d_up.data_ptr() + 16), EINVAL), ("d_down is x", dict(dd_p=x.data_ptr()), EINVAL),
        ("d_up is dy", dict(du_p=dy.data_ptr()), EINVAL), ("ws overlaps d_up", dict(ws_p=d_up.data_ptr()), EINVAL),
        ("ws is x", dict(ws_p=x.data_ptr()), EINVAL), ("ws misaligned", dict(ws_p=ws.data_ptr() + 2, ws_n=need - 1), EINVAL),
    ]
    keep = [t.clone() for t in (x, dy, up, down)]
    for name, kw, want in cases:
        code = call(**kw)
        assert code == want, (name, code)
        assert lib.fk_last_error().decode().startswith("fk_lora_side_grad_bf16"), name
    torch.cuda.synchronize()
    assert bool((d_up == S).all()) and bool((d_down == S).all()) and bool((ws == S).all())
    assert all(torch.equal(a, b) for a, b in zip(keep, (x, dy, up, down)))
    assert call() == 0                        # the same arguments, valid: it does run
    R.check("after the refusals", d_up, d_down, x, dy, up, down, 1.0)
    d_up.fill_(S), d_down.fill_(S)
    bad = [
        (x.float(), dy, up, down),                                # wrong dtype
        (x, dy, up.float(), down),
        (x[:, :, ::2], dy, up, down[:, ::2]),                     # last dimension not contiguous
        (x, dy[:, :R_ - 1], up, down),                            # rows that do not match
        (x[0], dy, up, down),                                     # 2-D against 3-D
        (x, dy, up, down[:, :K - 8]),                             # shapes that do not fit
        (x, dy, up[:N - 1], down),
        (x, dy, up[:, :4], down),
        (x.unsqueeze(0), dy.unsqueeze(0), up, down),              # 4-D
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.lora_side_grad(*args, 1.0, d_up=d_up, d_down=d_down)
    for kw in (dict(d_up=d_up.to(BF16)), dict(d_down=d_down.t()), dict(d_up=d_up[:, :4])):
        with pytest.raises(ValueError):
            ops.lora_side_grad(x, dy, up, down, 1.0, **{**dict(d_up=d_up, d_down=d_down), **kw})
    with pytest.raises(ValueError):
        ops.lora_side_grad(x, dy, up, down, 1.0, accumulate=True)
    with pytest.raises(RuntimeError, match="fk_lora_side_grad_bf16"):
        ops.lora_side_grad(x, dy, up, down, 1.0, d_up=d_up, d_down=d_down, ws=ws[:8])
    torch.cuda.synchronize()
    assert bool((d_up == S).all()) and bool((d_down == S).all())
