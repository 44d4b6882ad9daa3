"""GPU: ``fk_euler_inpaint_step_bf16`` and ``fk_scale_noise_bf16`` against the bf16 torch evaluation of the step formula on
the CPU (``inpaint_ref``, pinned by ``test_inpaint_host.py``) at 0 ulp -- the formula is exactly representable op by op, and
0 ulp is the bar ``euler`` is already held to in ``test_hip_kernels.py``."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref as R  # noqa: E402
from conftest import bf16_ulp_diff  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
C = 64
PAD_X, PAD_V = 16, 8            # rows behind S_tgt: x carries condition tokens (a sentinel here), v its own batch stride
SENTINEL = -7.75
DSIGMA = -0.0371                # not a bf16 number: the kernel has to round it first
# S_tgt = 24: 192 vectors, less than one block.  100: 800 vectors, 4 blocks, the last one partial.
# 131 096: 1 048 768 vectors, 192 past the first trip of a grid capped at 4096 blocks of 256 threads.
SHAPES = {"one_partial_block": (2, 24), "four_blocks": (2, 100), "second_grid_stride_trip": (1, 131072 + 24)}


def _data(B, S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S + PAD_X, C, generator=g).to(BF)
    x[:, S:] = SENTINEL
    v = torch.randn(B, S + PAD_V, C, generator=g).mul(3).to(BF)
    x0 = torch.randn(B, S, C, generator=g).mul(2).to(BF)
    noise = torch.randn(B, S, C, generator=g).to(BF)
    return x, v, x0, noise


def _mask(kind, Bm, S, seed):
    g = torch.Generator().manual_seed(seed + 100)
    if kind == "zeros":
        return torch.zeros(Bm, S, 4, dtype=BF)
    if kind == "ones":
        return torch.ones(Bm, S, 4, dtype=BF)
    if kind == "soft":          # not reachable from the pipeline (it binarises); the kernel's arithmetic covers it
        return torch.rand(Bm, S, 4, generator=g).to(BF)
    m = (torch.rand(Bm, S, 4, generator=g) < 0.5).to(BF)       # mixed within a token
    m[:, 0], m[:, 1], m[:, 2] = 0, 1, torch.tensor([1.0, 0.0, 0.0, 1.0]).to(BF)
    return m


@pytest.fixture(scope="module")
def cases():
    """(x, v, x0, noise) per shape, made once and never modified (the kernels work on device copies)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return {name: _data(B, S, seed) for seed, (name, (B, S)) in enumerate(SHAPES.items())}


def _check_step(data, S, mask, sigma_next):
    from gpt_image_edit_amd import ops
    x, v, x0, noise = data
    xd = x.cuda()
    ops.euler_inpaint_step(xd, v.cuda(), S, DSIGMA, sigma_next, x0.cuda(), noise.cuda(), mask.cuda())
    got = xd.cpu()
    ref = R.step(x[:, :S], v[:, :S], DSIGMA, sigma_next, x0, noise, R.expand_mask(mask, C))
    d = bf16_ulp_diff(got[:, :S], ref).max().item()
    print(f"[inpaint] S_tgt={S} mask batch {mask.shape[0]} sigma_next={sigma_next}: max ulp {d}", flush=True)
    assert d == 0
    assert torch.equal(got[:, S:], x[:, S:]), "rows behind S_tgt (the condition tokens) were written"
    return got[:, :S]


@pytest.mark.parametrize("sigma_next", [0.0, 0.7311, 1.0])
@pytest.mark.parametrize("mask_batch", [1, 2])
def test_step_base_case_matches_bf16_formula(cases, mask_batch, sigma_next):
    B, S = SHAPES["one_partial_block"]
    x, v, x0, noise = cases["one_partial_block"]
    got = _check_step(cases["one_partial_block"], S, _mask("mixed", mask_batch, S, mask_batch), sigma_next)
    # the two consequences the pipeline relies on, as values: token 0 is kept, token 1 is the Euler update
    assert torch.equal(got[:, 0], R.keep(x0, noise, sigma_next)[:, 0])
    assert torch.equal(got[:, 1], R.euler(x[:, :S], v[:, :S], DSIGMA)[:, 1])
    if sigma_next == 0.0:
        assert torch.equal(got[:, 0], x0[:, 0])


@pytest.mark.parametrize("kind", ["zeros", "ones", "soft"])
def test_step_uniform_and_soft_masks(cases, kind):
    B, S = SHAPES["one_partial_block"]
    _check_step(cases["one_partial_block"], S, _mask(kind, 2, S, 7), 0.7311)


@pytest.mark.parametrize("name", ["four_blocks", "second_grid_stride_trip"])
def test_step_beyond_one_block(cases, name):
    B, S = SHAPES[name]
    _check_step(cases[name], S, _mask("mixed", 1 if B == 1 else 2, S, 9), 0.7311)


@pytest.mark.parametrize("name", list(SHAPES))
def test_null_mask_is_the_euler_step(cases, name):
    from gpt_image_edit_amd import ops
    B, S = SHAPES[name]
    x, v, x0, noise = cases[name]
    a, b, c = x.cuda(), x.cuda(), x.cuda()
    vd = v.cuda()
    ops.euler_step(a, vd, S, DSIGMA)
    ops.euler_inpaint_step(b, vd, S, DSIGMA, 0.7311, x0.cuda(), noise.cuda(), None)
    ops.euler_inpaint_step(c, vd, S, DSIGMA, 0.7311, None, None, None)     # a mask of ones reads neither x0 nor noise
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(a[:, :S], x.cuda()[:, :S]) and torch.equal(a[:, S:].cpu(), x[:, S:])
    # ... and so is an explicit mask of ones, as values
    d = x.cuda()
    ops.euler_inpaint_step(d, vd, S, DSIGMA, 0.7311, x0.cuda(), noise.cuda(), _mask("ones", 1, S, 0).cuda())
    assert torch.equal(a, d)


@pytest.mark.parametrize("name", list(SHAPES))
def test_scale_noise_matches_bf16_formula(cases, name):
    from gpt_image_edit_amd import ops
    B, S = SHAPES[name]
    x, _, x0, noise = cases[name]
    x0d, nd = x0.cuda(), noise.cuda()
    for sigma in (0.0, 0.7311, 1.0):
        got = ops.scale_noise(x0d, nd, sigma).cpu()
        d = bf16_ulp_diff(got, R.keep(x0, noise, sigma)).max().item()
        print(f"[scale_noise] S={S} sigma={sigma}: max ulp {d}", flush=True)
        assert d == 0
    assert torch.equal(ops.scale_noise(x0d, nd, 0.0).cpu(), x0)
    # into the target rows of a token buffer (its own batch stride), as the pipeline starts an edit of strength < 1
    buf = x.cuda()
    ops.scale_noise(x0d, nd, 0.7311, out=buf[:, :S])
    assert bf16_ulp_diff(buf[:, :S].cpu(), R.keep(x0, noise, 0.7311)).max().item() == 0
    assert torch.equal(buf[:, S:].cpu(), x[:, S:])


def test_scheduler_scale_noise_looks_sigma_up_by_timestep(cases):
    import numpy as np
    from gpt_image_edit_amd import helpers
    from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler
    _, _, x0, noise = cases["one_partial_block"]
    s = FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / 6, 6), mu=helpers.calculate_shift(24), device="cpu")
    got = s.scale_noise(x0.cuda(), s.timesteps[3], noise.cuda()).cpu()
    assert bf16_ulp_diff(got, R.keep(x0, noise, float(s._sigmas_host[3]))).max().item() == 0
    s.set_begin_index(2)
    got = s.scale_noise(x0.cuda(), s.timesteps[3], noise.cuda()).cpu()       # a begin index wins, as in diffusers
    assert bf16_ulp_diff(got, R.keep(x0, noise, float(s._sigmas_host[2]))).max().item() == 0


def test_bad_alignment_and_sizes_are_errors_not_launches():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import libfk, ops
    lib = libfk.load()
    B, S = 1, 8
    n = B * S * C
    flat = [torch.full((n + 16,), 1.5, device="cuda", dtype=BF) for _ in range(4)]
    mflat = torch.ones(S * 4 + 8, device="cuda", dtype=BF)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(off=(0, 0, 0, 0), moff=0, c=C, strides=None, mstride=0):
        ptrs = [ctypes.c_void_p(t.data_ptr() + 2 * o) for t, o in zip(flat, off)]
        st = strides or [S * c] * 4
        return lib.fk_euler_inpaint_step_bf16(ptrs[0], st[0], ptrs[1], st[1], ptrs[2], st[2], ptrs[3], st[3],
                                              ctypes.c_void_p(mflat.data_ptr() + 2 * moff), mstride, B, S, c, DSIGMA, 0.5,
                                              stream)
    bad = [dict(off=(4, 0, 0, 0)), dict(off=(0, 4, 0, 0)), dict(off=(0, 0, 4, 0)), dict(off=(0, 0, 0, 4)),   # 8-byte offsets
           dict(moff=2), dict(mstride=2), dict(c=12), dict(c=4),
           dict(strides=[S * C + 4, S * C, S * C, S * C]), dict(strides=[S * C, S * C, S * C + 4, S * C])]
    for kw in bad:
        assert call(**kw) == -1, kw                       # FK_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == 1.5).all()) for t in flat), "a refused call wrote something"
    assert call() == 0                                  # the same arguments, aligned: a launch
    assert call(moff=4) == 0                            # the mask needs 8 bytes only
    out = torch.empty(n + 16, device="cuda", dtype=BF)
    sn = lambda o, c=C: lib.fk_scale_noise_bf16(ctypes.c_void_p(flat[2].data_ptr()), S * c, ctypes.c_void_p(flat[3].data_ptr()),  # noqa: E731
                                                S * c, ctypes.c_void_p(out.data_ptr() + 2 * o), S * c, B, S, c, 0.5, stream)
    assert sn(4) != 0 and sn(0, 12) != 0 and sn(0) == 0
    # through ops the error is an exception that names the entry point
    with pytest.raises(RuntimeError, match="fk_euler_inpaint_step_bf16"):
        ops.euler_inpaint_step(torch.zeros(1, 8, 12, device="cuda", dtype=BF), torch.zeros(1, 8, 12, device="cuda", dtype=BF),
                               8, DSIGMA, 0.5, torch.zeros(1, 8, 12, device="cuda", dtype=BF),
                               torch.zeros(1, 8, 12, device="cuda", dtype=BF), torch.ones(1, 8, 4, device="cuda", dtype=BF))
    torch.cuda.synchronize()
