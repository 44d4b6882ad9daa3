"""world_size-2 CPU test (gloo) of the in-place gradient intake of ``zero.ShardedAdamW`` (``grad_target`` / ``written``) as
``DenoiserTrainStep(lora=, data_parallel=True)`` drives it: three factor pairs of small odd shapes, per-rank and per-micro-batch
random bf16 ``dW``, two micro-batches, a torch stand-in for ``ops.lora_grad`` that honours ``accumulate`` and the AdamW stand-in
of tests/test_zero_gloo.py (on the GPU: csrc/lora_grad.hip, tests/test_hip_lora_grad_acc_kernel.py).

Bounds (u = 2^-24; nothing comes from the code under test):
  * gradient.  The ranks' chunks together are the fp32 sum S of four projections p_i (2 ranks x 2 micro-batches), added with three
    fp32 adds (staged: every pass is reduce-scattered, later passes added to the chunk).  Each p_i is within b_i =
    ``lora_grad_ref.bounds`` of its fp64 value r_i; every partial sum is at most sum (|r_i| + b_i), so
        |S - sum r_i| <= sum b_i + 3 u sum (|r_i| + b_i).
  * parameters.  No clipping (max_grad_norm = 1e3), so the coefficient is exactly grad_scale = 1 / 4 on the ranks and 1 on the
    single process, which is fed fp32(sum r_i / 4): the two gradients differ by dg <= (bound above) / 4 + u |mean|.  First AdamW
    step from zero moments: the update is lr f(g), f(x) = x / (|x| + eps), f' = eps / (|x| + eps)^2 decreasing in |x|, so
        |lr f(g) - lr f(g')| <= lr min(2, dg eps / (max(|g| - dg, 0) + eps)^2);
    the fp32 evaluation itself (decay, lerp, square, sqrt, two divisions, add: under 16 roundings of quantities bounded by lr and
    |master|) adds 16 u (lr + |master|) per side.  The bf16 copy of each side is within half a bf16 ulp (2^-9 |p|) of its master."""
import io
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lora_grad_ref as R
import prodigy_stub as PS
from test_zero_gloo import TorchKernels

BF = torch.bfloat16
U = R.U32
WEIGHTS = [("single_transformer_blocks.1.attn.to_q", 33, 17, 5), ("single_transformer_blocks.0.proj_mlp", 21, 35, 3),
           ("transformer_blocks.0.ff.net.2", 9, 65, 7)]                # (module, N, K, r)
SCALE = 0.75
HP = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=1e-2)
NO_CLIP = 1e3


def _names():
    return [m + s for m, _, _, _ in WEIGHTS for s in (".lora_A.weight", ".lora_B.weight")]


def _factors(seed=0):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for m, N, K, r in WEIGHTS:
        out[m + ".lora_B.weight"] = (0.3 * torch.randn(N, r, generator=g)).to(BF)       # up
        out[m + ".lora_A.weight"] = (0.3 * torch.randn(r, K, generator=g)).to(BF)       # down
    return out


def _dw(rank, micro, i):
    _, N, K, _ = WEIGHTS[i]
    g = torch.Generator().manual_seed(1000 + 100 * rank + 10 * micro + i)
    return (0.02 * torch.randn(N, K, generator=g)).to(BF)


def lora_grad(dw, up, down, scale, d_up=None, d_down=None, ws=None, accumulate=False):
    """The contract of ``ops.lora_grad`` in fp32 torch (exact bf16 products, fp32 accumulation, the scale once)."""
    sc = torch.tensor(R.f32(scale), dtype=torch.float32)
    pu, pd = sc * (dw.float() @ down.float().T), sc * (up.float().T @ dw.float())
    if accumulate:
        d_up.add_(pu), d_down.add_(pd)
    else:
        d_up.copy_(pu), d_down.copy_(pd)


def _backward_passes(opt, rank, factors):
    """Two micro-batches as ``_lora_sink`` feeds them; returns whether any call was asked to accumulate."""
    asked = []
    for micro in range(2):
        opt.begin_micro_batch()
        for i, (m, _, _, _) in enumerate(WEIGHTS):
            nb, na = m + ".lora_B.weight", m + ".lora_A.weight"
            (d_up, acc), (d_down, acc2) = opt.grad_target(nb), opt.grad_target(na)
            assert acc == acc2
            asked.append(acc)
            lora_grad(_dw(rank, micro, i), factors[nb], factors[na], SCALE, d_up=d_up, d_down=d_down, accumulate=acc)
            opt.written([nb, na])
    return asked


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gpt_image_edit_amd.zero import ShardedAdamW, backward_order
    order = backward_order(_names())
    factors = _factors()
    opt = ShardedAdamW(factors, max_grad_norm=NO_CLIP, kernels=TorchKernels, order=order, **HP)
    opt.check_ranks_agree("same seed")                         # passes: nothing raised
    asked = _backward_passes(opt, rank, opt.params)
    assert asked == [False] * 6, "with two ranks every pass is staged: the kernel overwrites zeroed staging"
    opt._flush()
    grad = opt.grad_slice.clone()
    before = opt.master.clone()
    norm = float(opt.step())
    # ranks built from different seeds: every rank raises, nobody is left in a collective
    bad = ShardedAdamW(_factors(seed=1 + rank), max_grad_norm=NO_CLIP, kernels=TorchKernels, order=order, **HP)
    try:
        bad.check_ranks_agree("different seeds")
        raised = ""
    except ValueError as e:
        raised = str(e)
    dist.barrier()                                             # ... and the next collective completes
    # one Prodigy step through the same intake
    popt = ShardedAdamW(_factors(), max_grad_norm=1.0, kernels=PS, order=order, optimizer="prodigy", weight_decay=1e-2,
                        prodigy=dict(d0=1e-3))
    _backward_passes(popt, rank, popt.params)
    popt.step()
    buf = io.BytesIO()
    torch.save(dict(rank=rank, grad=grad, before=before, master=opt.master.clone(), norm=norm, used=opt.layout.used,
                    params={n: p.clone() for n, p in opt.params.items()}, raised=raised, pstate=popt.pstate.clone(),
                    d=popt.prodigy_state()["d"], pparams={n: p.clone() for n, p in popt.params.items()}), buf)
    q.put(buf.getvalue())
    dist.barrier()
    dist.destroy_process_group()


def test_lora_dp_gloo_world2():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    r0, r1 = sorted((torch.load(io.BytesIO(q.get(timeout=180)), weights_only=False) for _ in procs), key=lambda t: t["rank"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    from gpt_image_edit_amd.zero import ShardedAdamW, backward_order
    order = backward_order(_names())
    factors = _factors()
    used = r0["used"]
    # ---- the gathered gradient against the fp64 sum of the four projections
    ref, bound = {}, {}
    for i, (m, N, K, r) in enumerate(WEIGHTS):
        nb, na = m + ".lora_B.weight", m + ".lora_A.weight"
        parts = [R.bounds(_dw(rank, micro, i), factors[nb], factors[na], SCALE) for rank in range(world) for micro in range(2)]
        for name, slot in ((nb, 0), (na, 1)):
            ref[name] = sum(p[slot][0] for p in parts)
            bound[name] = sum(p[slot][1] for p in parts) + 3 * U * sum(p[slot][0].abs() + p[slot][1] for p in parts)
    flat_ref = torch.cat([ref[n].reshape(-1) for n in order])
    flat_bound = torch.cat([bound[n].reshape(-1) for n in order])
    got = torch.cat([r0["grad"], r1["grad"]])
    assert not bool(got[used:].any()), "the padding of the chunks holds a gradient"
    ratio = R.worst_ratio(got[:used], flat_ref, flat_bound)
    print(f"[parity] lora_dp gloo gradient: observed/bound {ratio:.4f}", flush=True)
    assert ratio <= 1.0
    # ---- both ranks hold the same bits after the step
    assert r0["norm"] == r1["norm"] and all(torch.equal(r0["params"][n], r1["params"][n]) for n in order)
    # ---- one process fed the fp64 mean
    one = ShardedAdamW(factors, max_grad_norm=NO_CLIP, kernels=TorchKernels, order=order, **HP)
    mean = {n: (ref[n] / 4).to(torch.float32) for n in order}
    one.accumulate(mean)
    norm1 = float(one.step())
    assert abs(norm1 - r0["norm"]) <= 1e-5 * norm1 and norm1 < NO_CLIP
    g = flat_ref / 4
    dg = flat_bound / 4 + U * g.abs()
    lr, eps = HP["lr"], HP["eps"]
    before = torch.cat([r0["before"], r1["before"]])[:used].double()
    b_master = lr * torch.minimum(torch.full_like(dg, 2.0), dg * eps / ((g.abs() - dg).clamp_min(0) + eps) ** 2) + 2 * 16 * U * (lr + before.abs())
    master = torch.cat([r0["master"], r1["master"]])[:used]
    ratio = R.worst_ratio(master, one.master[:used].double(), b_master)
    print(f"[parity] lora_dp gloo AdamW master: observed/bound {ratio:.4f}", flush=True)
    assert ratio <= 1.0 and not torch.equal(master.double(), before)
    p_ranks = torch.cat([r0["params"][n].reshape(-1) for n in order]).double()
    p_one = torch.cat([one.params[n].reshape(-1) for n in order]).double()
    b_param = b_master + 2.0 ** -9 * (master.double().abs() + one.master[:used].double().abs())
    assert R.worst_ratio(p_ranks, p_one, b_param) <= 1.0
    # ---- different seeds: both ranks raised, with the checksums in the message
    assert "different parameters" in r0["raised"] and "different seeds" in r0["raised"] and r0["raised"] == r1["raised"]
    # ---- Prodigy: the same scalars and the same weights on both ranks
    assert r0["d"] == r1["d"] and torch.equal(r0["pstate"], r1["pstate"]) and float(r0["pstate"][PS.I["k"]]) == 1
    assert all(torch.equal(r0["pparams"][n], r1["pparams"][n]) for n in order)
    assert any(not torch.equal(r0["pparams"][n], factors[n]) for n in order)
