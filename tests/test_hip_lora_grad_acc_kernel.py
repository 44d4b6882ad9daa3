"""fk_lora_grad_acc_bf16 on the GPU against tests/lora_grad_acc_ref.py, at the shapes of ``lora_grad_ref.SHAPES`` (both roles
unsplit, second strips and steps with the rank padded to 64, UP split only, DOWN split only, the production weight):
``accumulate = 0`` gives the bits of fk_lora_grad_bf16 on outputs full of NaN, ``accumulate = 1`` onto zeros gives them too, a
second accumulating call lies within the derived bound, integer cases at 0 ulp, outputs as views at odd fp32 offsets of one
buffer between untouched guards, ``dW`` as a strided row block, two identical sequences bit-identical, ``accumulate = 2``
refused with nothing written; then ``zero.ShardedAdamW``'s in-place intake with the real ops, direct against staged.

Observed worst |out - ref| / bound of the second, accumulating call on an MI355X (one run): 0.054 over the thirteen shapes
(N = 131, K = 16, r = 8, d_up), 1e-4 at (3072, 3072, 16), 0.0083 / 0.0162 / 0.0244 (d_up) at the ranks 65 / 80 / 96 of the third
rank tile; the ``ShardedAdamW`` intake 0.034, direct and staged alike."""
import ctypes

import pytest
import torch

import lora_grad_acc_ref as A
import lora_grad_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda"
G = 63                                        # guard floats: odd, so the two views below start at odd fp32 offsets
S = 777.0                                     # sentinel


@pytest.fixture(scope="module")
def ops():
    from gpt_image_edit_amd import ops
    return ops


def bits(t):
    return t.contiguous().view(torch.int32)


def call_acc(dw, up, down, s, d_up, d_down, accumulate, ws=None):
    """The new entry point itself, with any value of ``accumulate``; returns the status code."""
    from gpt_image_edit_amd import libfk
    lib = libfk.load()
    N, K = dw.shape
    r = up.shape[1]
    if ws is None:
        ws = torch.empty(lib.fk_lora_grad_ws_floats(N, K, r), device=DEV, dtype=torch.float32)
    V = ctypes.c_void_p
    st = V(torch.cuda.current_stream().cuda_stream)
    return lib.fk_lora_grad_acc_bf16(V(dw.data_ptr()), dw.stride(0), V(up.data_ptr()), up.stride(0), V(down.data_ptr()), down.stride(0),
                                     N, K, r, float(s), V(d_up.data_ptr()), V(d_down.data_ptr()), int(accumulate),
                                     V(ws.data_ptr()) if ws.numel() else None, ws.numel(), st)


def views(N, K, r, fill):
    """(flat buffer, d_up view, d_down view): guard | d_up | guard | d_down | guard -- G = 63 floats in front of d_up, so it starts
    at an odd fp32 offset; d_down starts at G + N r + the middle guard, made odd too by one more guard float when N r is even."""
    mid = G + 1 - (N * r) % 2
    big = torch.full((G + N * r + mid + r * K + G,), fill, device=DEV, dtype=torch.float32)
    o_up, o_dn = G, G + N * r + mid
    assert o_up % 2 == 1 and o_dn % 2 == 1
    return big, big[o_up:o_up + N * r].view(N, r), big[o_dn:o_dn + r * K].view(r, K)


def guards(big, N, K, r):
    mid = G + 1 - (N * r) % 2
    return torch.cat([big[:G], big[G + N * r:G + N * r + mid], big[-G:]])


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_overwrite_form_is_the_old_entry_and_never_reads_the_outputs(ops, N, K, r):
    dw, up, down, s = R.data(N, K, r, seed=N + K + r, device=DEV)
    want_u, want_d = ops.lora_grad(dw, up, down, s)                         # fk_lora_grad_bf16
    d_up = torch.full((N, r), float("nan"), device=DEV)
    d_down = torch.full((r, K), float("nan"), device=DEV)
    assert call_acc(dw, up, down, s, d_up, d_down, 0) == 0
    assert torch.equal(bits(d_up), bits(want_u)) and torch.equal(bits(d_down), bits(want_d))
    # accumulate = 1 onto zeros: 0 + x = x, the same bits (a projection is never -0: it would need every product to be -0)
    z_up, z_down = torch.zeros(N, r, device=DEV), torch.zeros(r, K, device=DEV)
    ops.lora_grad(dw, up, down, s, d_up=z_up, d_down=z_down, accumulate=True)
    assert torch.equal(z_up, want_u) and torch.equal(z_down, want_d)
    assert torch.equal(bits(z_up) & 0x7fffffff, bits(want_u) & 0x7fffffff)


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_second_accumulating_call_within_the_bound_guards_and_determinism(ops, N, K, r):
    dw1, up, down, s = R.data(N, K, r, seed=N + K + r, device=DEV)
    dw2 = R.data(N, K, r, seed=N + K + r + 1, device=DEV)[0]
    keep = [t.clone() for t in (dw1, dw2, up, down)]
    ws = ops.lora_grad_ws(N, K, r, DEV)

    def sequence():
        big, d_up, d_down = views(N, K, r, S)
        ops.lora_grad(dw1, up, down, s, d_up=d_up, d_down=d_down, ws=ws)
        old = (d_up.clone(), d_down.clone())
        ops.lora_grad(dw2, up, down, s, d_up=d_up, d_down=d_down, ws=ws, accumulate=True)
        return big, d_up, d_down, old

    big, d_up, d_down, (old_u, old_d) = sequence()
    R.check("first call", old_u, old_d, dw1, up, down, s)
    A.check("second call", d_up, d_down, old_u, old_d, dw2, up, down, s)
    assert bool((guards(big, N, K, r) == S).all()), "a guard around an output was written"
    assert all(torch.equal(a, b) for a, b in zip(keep, (dw1, dw2, up, down))), "an input was written"
    big2 = sequence()[0]
    assert torch.equal(bits(big), bits(big2)), "two identical call sequences differ"


@pytest.mark.parametrize("N,K,r", R.SHAPES)
def test_integer_cases_are_0_ulp(ops, N, K, r):
    dw, up, down, s = R.exact_data(N, K, r, seed=N + K, device=DEV)
    ou, od = A.exact_old(N, K, r, seed=N + K, device=DEV)
    want_u, want_d = A.exact(ou, od, dw, up, down, s)
    big, d_up, d_down = views(N, K, r, S)
    d_up.copy_(ou), d_down.copy_(od)
    ops.lora_grad(dw, up, down, s, d_up=d_up, d_down=d_down, accumulate=True)
    assert torch.equal(d_up, want_u) and torch.equal(d_down, want_d)
    assert bool((guards(big, N, K, r) == S).all())


@pytest.mark.parametrize("N,K,r", [(65, 136, 33), (131, 264, 16), (131, 72, 80)])
@pytest.mark.parametrize("pad", [8, 3])       # row strides that keep / break the 16-byte alignment of the rows
def test_strided_row_block(ops, N, K, r, pad):
    """dW as rows [N, 2N) of a [3N, K + pad] buffer (the q / k / v gradients are such row blocks)."""
    dw0, up, down, s = R.exact_data(N, K, r, seed=N + pad, device=DEV)
    ou, od = A.exact_old(N, K, r, seed=N + pad, device=DEV)
    want_u, want_d = A.exact(ou, od, dw0, up, down, s)
    wide = torch.full((3 * N, K + pad), 3.0, device=DEV, dtype=BF16)
    dw = wide[N:2 * N, :K]
    dw.copy_(dw0)
    keep = wide.clone()
    big, d_up, d_down = views(N, K, r, S)
    d_up.copy_(ou), d_down.copy_(od)
    ops.lora_grad(dw, up, down, s, d_up=d_up, d_down=d_down, accumulate=True)
    assert torch.equal(d_up, want_u) and torch.equal(d_down, want_d)
    assert bool((guards(big, N, K, r) == S).all()) and torch.equal(wide, keep)


def test_accumulate_2_is_refused_and_writes_nothing(ops):
    from gpt_image_edit_amd import libfk
    N, K, r = 131, 264, 8                     # both reductions split: the workspace is needed
    dw, up, down, s = R.data(N, K, r, seed=1, device=DEV)
    d_up = torch.full((N, r), S, device=DEV)
    d_down = torch.full((r, K), S, device=DEV)
    ws = torch.full((libfk.load().fk_lora_grad_ws_floats(N, K, r),), S, device=DEV)
    for bad in (2, -1):
        assert call_acc(dw, up, down, s, d_up, d_down, bad, ws=ws) == -1          # FK_EINVAL
        assert libfk.load().fk_last_error().decode().startswith("fk_lora_grad_acc_bf16")
    torch.cuda.synchronize()
    assert bool((d_up == S).all()) and bool((d_down == S).all()) and bool((ws == S).all())
    with pytest.raises(ValueError, match="accumulate"):
        ops.lora_grad(dw, up, down, s, accumulate=True)                          # nothing to add to
    assert call_acc(dw, up, down, s, d_up, d_down, 1, ws=ws) == 0                # the same arguments, valid: it does run
    ou = torch.full((N, r), S, device=DEV)
    od = torch.full((r, K), S, device=DEV)
    A.check("after the refusals", d_up, d_down, ou, od, dw, up, down, s)


def test_sharded_adamw_intake_direct_against_staged(ops):
    """Factor-shaped parameters, two micro-batches through ``grad_target`` / ``written`` with the real ops: the direct intake
    (overwrite, then the kernel accumulates in the chunk) against the staged one (overwrite zeroed staging, copy, add)."""
    from gpt_image_edit_amd.zero import ShardedAdamW
    shapes = [("single_transformer_blocks.0.attn.to_q", 131, 264, 8), ("transformer_blocks.0.attn.to_k", 65, 136, 33),
              ("transformer_blocks.0.ff.net.2", 33, 17, 5)]
    g = torch.Generator().manual_seed(11)
    params = {}
    for m, N, K, r in shapes:
        params[m + ".lora_B.weight"] = (0.3 * torch.randn(N, r, generator=g)).to(BF16).to(DEV)
        params[m + ".lora_A.weight"] = (0.3 * torch.randn(r, K, generator=g)).to(BF16).to(DEV)
    dws = [[R.data(N, K, r, seed=50 + 10 * micro + i, device=DEV)[0] for i, (_, N, K, r) in enumerate(shapes)] for micro in range(2)]
    s = 0.75
    res = {}
    for mode, kw in (("direct", {}), ("staged", dict(stage_always=True))):
        opt = ShardedAdamW({k: v.clone() for k, v in params.items()}, lr=1e-3, **kw)
        asked = []
        for micro in range(2):
            opt.begin_micro_batch()
            for i, (m, N, K, r) in enumerate(shapes):
                nb, na = m + ".lora_B.weight", m + ".lora_A.weight"
                (d_up, acc), (d_down, _) = opt.grad_target(nb), opt.grad_target(na)
                asked.append(acc)
                ops.lora_grad(dws[micro][i], opt.params[nb], opt.params[na], s, d_up=d_up, d_down=d_down, accumulate=acc)
                opt.written([nb, na])
        assert asked == ([False] * 3 + [True] * 3 if mode == "direct" else [False] * 6)
        opt._flush()
        grad = opt.grad_slice.clone()
        opt.step()
        res[mode] = (opt, grad)
    (od_, gd), (os_, gs) = res["direct"], res["staged"]
    L = od_.layout
    worst = 0.0
    for i, (m, N, K, r) in enumerate(shapes):
        nb, na = m + ".lora_B.weight", m + ".lora_A.weight"
        first = ops.lora_grad(dws[0][i], params[nb], params[na], s)
        for name, old, slot in ((nb, first[0], 0), (na, first[1], 1)):
            lo, n, shape = L.offsets[name]
            ref, bound = A.bounds(first[0], first[1], dws[1][i], params[nb], params[na], s)[slot]
            # both intakes form fp32(old + p2): the direct one inside the kernel, the staged one as a torch add of the two
            # overwrite results; each is within the accumulate bound of the fp64 value, so they agree within twice it
            for got in (gd, gs):
                worst = max(worst, R.worst_ratio(got[lo:lo + n].view(shape), ref, bound))
            assert R.worst_ratio(gd[lo:lo + n].view(shape), gs[lo:lo + n].view(shape).double(), 2 * bound) <= 1.0
    print(f"[parity] ShardedAdamW intake, direct and staged against fp64: observed/bound {worst:.4f}", flush=True)
    assert worst <= 1.0
    assert not bool(gd[L.used:].any()) and not bool(gs[L.used:].any())
    for k in params:      # the tolerance of test_sharded_gradient_accumulation_and_modified_gradient_error
        a, b = od_.params[k].float(), os_.params[k].float()
        assert (a - b).abs().max().item() <= 2.0 ** -8 * a.abs().max().item() + 1e-6, k
        assert not torch.equal(od_.params[k], params[k]), f"{k} did not move"
