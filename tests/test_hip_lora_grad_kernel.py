"""fk_lora_grad_bf16 on the GPU against tests/lora_grad_ref.py: the fp64 projection within the bound derived there, integer
cases at 0 ulp, dW as a row block of a wider buffer and with an odd row stride, guards around both outputs, two launches
bit-identical, untouched inputs and every refusal.

Observed worst |out - ref| / bound on an MI355X: 0.045 over the thirteen shapes (N = 131, K = 16, r = 8, d_up), 1e-4 at
(3072, 3072, 16) -- the bound is the worst case over every summation order, L_pad roundings all of one sign.  The rank tile of
96 (d_up / d_down): 0.0057 / 0.0087 at r = 65, 0.0135 / 0.0054 at r = 80, 0.0187 / 0.0082 at r = 96."""
import ctypes

import pytest
import torch

import lora_grad_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
G = 64                                        # guard floats in front of and behind an output
S = 777.0                                     # sentinel


@pytest.fixture(scope="module")
def ops():
    from gpt_image_edit_amd import ops
    return ops


def guarded(rows, cols):
    """(flat fp32 buffer of sentinels, its contiguous [rows, cols] middle)."""
    big = torch.full((2 * G + rows * cols,), S, device=DEV, dtype=torch.float32)
    return big, big[G:G + rows * cols].view(rows, cols)


def guards_intact(big):
    return bool((big[:G] == S).all()) and bool((big[-G:] == S).all())


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_projection_against_fp64(ops, N, K, r):
    dw, up, down, s = R.data(N, K, r, seed=N + K + r, device=DEV)
    keep = [t.clone() for t in (dw, up, down)]
    big_u, d_up = guarded(N, r)
    big_d, d_down = guarded(r, K)
    ops.lora_grad(dw, up, down, s, d_up=d_up, d_down=d_down)
    R.check("random", d_up, d_down, dw, up, down, s)
    assert guards_intact(big_u) and guards_intact(big_d), "a guard around an output was written"
    assert all(torch.equal(a, b) for a, b in zip(keep, (dw, up, down))), "an input was written"
    again = ops.lora_grad(dw, up, down, s)                      # fresh outputs, a fresh workspace: the same bits
    assert torch.equal(again[0].view(torch.int32), d_up.view(torch.int32))
    assert torch.equal(again[1].view(torch.int32), d_down.view(torch.int32))


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_integer_cases_are_0_ulp(ops, N, K, r):
    dw, up, down, s = R.exact_data(N, K, r, seed=N + K, device=DEV)
    fu, fd = R.exact_grads(dw, up, down, s)
    d_up, d_down = ops.lora_grad(dw, up, down, s)
    assert torch.equal(d_up, fu) and torch.equal(d_down, fd)


@pytest.mark.parametrize("N,K,r", [(63, 72, 5), (65, 136, 33), (131, 264, 16), (131, 72, 80)])
@pytest.mark.parametrize("pad", [8, 3])       # row strides that keep / break the 16-byte alignment of the rows
def test_row_block_of_a_wider_buffer(ops, N, K, r, pad):
    """dW as rows [N, 2N) of a [3N, K + pad] buffer (the q / k / v gradients are such row blocks), strided factors too."""
    dw0, up0, down0, s = R.exact_data(N, K, r, seed=N + pad, device=DEV)
    fu, fd = R.exact_grads(dw0, up0, down0, s)
    wide = torch.full((3 * N, K + pad), 3.0, device=DEV, dtype=BF16)
    dw = wide[N:2 * N, :K]
    dw.copy_(dw0)
    up = torch.full((N, r + pad), 3.0, device=DEV, dtype=BF16)[:, :r]
    down = torch.full((r, K + pad), 3.0, device=DEV, dtype=BF16)[:, :K]
    up.copy_(up0), down.copy_(down0)
    keep = wide.clone()
    big_u, d_up = guarded(N, r)
    big_d, d_down = guarded(r, K)
    ops.lora_grad(dw, up, down, s, d_up=d_up, d_down=d_down)
    assert torch.equal(d_up, fu) and torch.equal(d_down, fd)
    assert guards_intact(big_u) and guards_intact(big_d) and torch.equal(wide, keep)
    if pad % 8:                               # one element off a 16-byte boundary as well
        off = torch.full((N * (K + pad) + 1,), 3.0, device=DEV, dtype=BF16)[1:].view(N, K + pad)[:, :K]
        off.copy_(dw0)
        ou, od = ops.lora_grad(off, up, down, s)
        assert torch.equal(ou, fu) and torch.equal(od, fd)


def test_refusals_write_nothing(ops):
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    N, K, r = 131, 264, 8                     # both reductions split: the workspace is needed
    dw, up, down, s = R.data(N, K, r, seed=1, device=DEV)
    d_up = torch.full((N, r), S, device=DEV, dtype=torch.float32)
    d_down = torch.full((r, K), S, device=DEV, dtype=torch.float32)
    need = lib.fk_lora_grad_ws_floats(N, K, r)
    assert need == 2 * N * r + 2 * r * K and lib.fk_lora_grad_ws_floats(64, 128, 8) == 0
    ws = torch.full((need,), S, device=DEV, dtype=torch.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    V = ctypes.c_void_p

    def call(dw_p=dw.data_ptr(), ld_dw=K, up_p=up.data_ptr(), ld_up=r, down_p=down.data_ptr(), ld_down=K, n=N, k=K, rank=r,
             scale=1.0, du_p=d_up.data_ptr(), dd_p=d_down.data_ptr(), ws_p=ws.data_ptr(), ws_n=need):
        return lib.fk_lora_grad_bf16(V(dw_p), ld_dw, V(up_p), ld_up, V(down_p), ld_down, n, k, rank, scale, V(du_p), V(dd_p),
                                     V(ws_p), ws_n, st)

    EINVAL, EUNSUP = -1, -2
    cases = [
        ("N = 0", dict(n=0), EINVAL), ("K = 0", dict(k=0), EINVAL), ("rank 0", dict(rank=0), EUNSUP),
        ("rank 129", dict(rank=129, ld_up=129), EUNSUP), ("ld_dw < K", dict(ld_dw=K - 1), EINVAL),
        ("ld_up < rank", dict(ld_up=r - 1), EINVAL), ("ld_down < K", dict(ld_down=K - 8), EINVAL),
        ("null dw", dict(dw_p=0), EINVAL), ("null up", dict(up_p=0), EINVAL), ("null down", dict(down_p=0), EINVAL),
        ("null d_up", dict(du_p=0), EINVAL), ("null d_down", dict(dd_p=0), EINVAL), ("null ws", dict(ws_p=0), EINVAL),
        ("ws too small", dict(ws_n=need - 1), EINVAL), ("scale inf", dict(scale=float("inf")), EINVAL),
        ("scale nan", dict(scale=float("nan")), EINVAL), ("d_up overlaps d_down", dict(dd_p=d_up.data_ptr() + 16), EINVAL),
        ("d_down is dw", dict(dd_p=dw.data_ptr()), EINVAL), ("ws overlaps d_up", dict(ws_p=d_up.data_ptr()), EINVAL),
    ]
    keep = [t.clone() for t in (dw, up, down)]
    for name, kw, want in cases:
        code = call(**kw)
        assert code == want, (name, code)
        assert lib.fk_last_error().decode().startswith("fk_lora_grad_bf16"), name
    torch.cuda.synchronize()
    assert bool((d_up == S).all()) and bool((d_down == S).all()) and bool((ws == S).all())
    assert all(torch.equal(a, b) for a, b in zip(keep, (dw, up, down)))
    assert call() == 0                        # the same arguments, valid: it does run
    R.check("after the refusals", d_up, d_down, dw, up, down, 1.0)
    d_up.fill_(S), d_down.fill_(S)
    bad = [
        (dw.float(), up, down),                                   # wrong dtype
        (dw, up.float(), down),
        (dw[:, ::2], up, down[:, ::2]),                           # last dimension not contiguous
        (dw, up, down[:, :K - 8]),                                # shapes that do not fit
        (dw, up[:N - 1], down),
        (dw, up[:, :4], down),
        (dw.view(1, N, K), up, down),                             # not 2-D
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ops.lora_grad(*args, 1.0, d_up=d_up, d_down=d_down)
    for kw in (dict(d_up=d_up.to(BF16)), dict(d_down=d_down.t()), dict(d_up=d_up[:, :4])):
        with pytest.raises(ValueError):
            ops.lora_grad(dw, up, down, 1.0, **{**dict(d_up=d_up, d_down=d_down), **kw})
    with pytest.raises(RuntimeError, match="fk_lora_grad_bf16"):
        ops.lora_grad(dw, up, down, 1.0, d_up=d_up, d_down=d_down, ws=ws[:8])
    torch.cuda.synchronize()
    assert bool((d_up == S).all()) and bool((d_down == S).all())
