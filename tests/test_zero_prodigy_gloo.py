"""world_size-2 CPU test (gloo) of ``zero.ShardedAdamW(optimizer="prodigy")`` against ONE process on the same gradients, with the torch
stand-ins of tests/prodigy_stub.py for the four kernels (on the GPU they are csrc/prodigy.hip, tests/test_hip_prodigy_kernels.py).

Every step is compared from the SAME state: the single process is restarted from the state the two ranks held before the step
(gathered chunk by chunk), so the bounds are single-step ones.  Both sides run the same fp32 element arithmetic on the same
numbers (the ranks' fp32 gradient SUM times 1 / 2 is the single process's fp32 mean, bit for bit), so m, v and s must be EQUAL;
the two running sums are double sums of the same terms cut into other chunks, so they differ by the order term
2 (n + 512) 2^-53 sum |terms| (``prodigy_ref.bounds_moments``); d_hat by ``prodigy_ref.bound_d_hat`` of those; the parameters by the
element bound of ``apply`` (each side within one bound of the exact value: MARGIN = 2) plus the sensitivity of the denominator
sqrt(v) + d eps to the difference in d."""
import io
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import prodigy_ref as R
import prodigy_stub as S

BF = torch.bfloat16
SHAPES = {"blocks.0.attn.to_q.weight": (33, 17), "blocks.0.attn.to_q.bias": (33,), "blocks.1.norm.linear.weight": (50, 7),
          "blocks.1.attn.norm_q.weight": (128,)}
KW = dict(optimizer="prodigy", weight_decay=1e-2, max_grad_norm=1.0,
          prodigy=dict(d0=1e-3, use_bias_correction=False, safeguard_warmup=False))      # d leaves d0 at the third step
STEPS = 5
STATE = ("master", "p0", "exp_avg", "exp_avg_sq", "s")


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return {n: (torch.randn(s, generator=g) * 0.05).to(BF) for n, s in SHAPES.items()}


def _grads(rank, step):
    """A fixed direction plus rank- and step-dependent noise: p0 - p then points along the gradient and d grows.  Step 0 is clipped."""
    base, g = torch.Generator().manual_seed(5), torch.Generator().manual_seed(100 + 10 * step + rank)
    scale = 2.0 if step == 0 else 0.01
    return {n: scale * (torch.randn(s, generator=base) + 0.3 * torch.randn(s, generator=g)) for n, s in SHAPES.items()}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _snap(opt):
    return {k: getattr(opt, k).clone() for k in STATE + ("pstate",)}


def _worker(rank, world, port, q, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from gpt_image_edit_amd.zero import ShardedAdamW
    opt = ShardedAdamW(_params(), kernels=S, **KW)
    assert len(opt.layout.buckets) == 1
    steps = []
    for step in range(STEPS):
        before = _snap(opt)
        for n, g in _grads(rank, step).items():
            opt.grads[n].copy_(g)
        norm = float(opt.step())
        steps.append((before, _snap(opt), norm, {n: p.clone() for n, p in opt.params.items()}))
        if step == 2:
            opt.save(tmp)
    # resume after three steps: the fourth and fifth are the uninterrupted run's, bit for bit
    ropt = ShardedAdamW(_params(seed=9), kernels=S, **KW)
    ropt.load(tmp)
    resumed = all(torch.equal(ropt.params[n], steps[2][3][n]) for n in SHAPES)
    for step in range(3, STEPS):
        for n, g in _grads(rank, step).items():
            ropt.grads[n].copy_(g)
        ropt.step()
    resumed = resumed and all(torch.equal(getattr(ropt, k), getattr(opt, k)) for k in STATE + ("pstate", "flat_param"))
    # gradient accumulation: two backward passes per step, the step on their mean -- against one pass of the mean
    aopt, mopt = ShardedAdamW(_params(), kernels=S, **KW), ShardedAdamW(_params(), kernels=S, **KW)
    for step in range(1, 4):
        ga, gb = _grads(rank, step), _grads(rank + 7, step)
        aopt.begin_micro_batch()
        aopt.accumulate(ga)
        aopt.begin_micro_batch()
        aopt.accumulate(gb)
        na = float(aopt.step())
        mopt.accumulate({n: (ga[n] + gb[n]) / 2 for n in SHAPES})
        nm = float(mopt.step())
        assert abs(na - nm) <= 1e-6 * nm, (na, nm)
    micro = (aopt.prodigy_state(), mopt.prodigy_state(), {n: (aopt.params[n].clone(), mopt.params[n].clone()) for n in SHAPES})
    buf = io.BytesIO()                                      # as bytes: the queue would share tensor storage with a process that has exited
    torch.save((rank, steps, resumed, micro, opt.state_bytes(), opt.layout.slice_numel, opt.layout.used), buf)
    q.put(buf.getvalue())
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_prodigy_gloo_world2_matches_single_process(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((torch.load(io.BytesIO(q.get(timeout=180)), weights_only=False) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, st0, resumed0, micro0, bytes0, slice0, used), (_, st1, resumed1, micro1, _, _, _) = res
    assert resumed0 and resumed1, "the steps after a resume are not the uninterrupted run's"
    assert bytes0 == (slice0 * world * 6, slice0 * 24), "6 fp32 chunks per rank: master, 2 moments, gradient, s, p0"

    from gpt_image_edit_amd.zero import ShardedAdamW
    one = ShardedAdamW(_params(), kernels=S, **KW)                      # no process group: world 1
    hp = R.kernel_hp(dict(KW["prodigy"], weight_decay=KW["weight_decay"], lr=1.0))
    I = S.I
    moved = False
    for step in range(STEPS):
        (b0, a0, n0, p0_), (b1, a1, n1, p1_) = st0[step], st1[step]
        assert torch.equal(b0["pstate"], b1["pstate"]) and torch.equal(a0["pstate"], a1["pstate"]), "the ranks disagree on the scalars"
        assert n0 == n1 and all(torch.equal(p0_[n], p1_[n]) for n in SHAPES), "the ranks disagree on the weights"
        for k in STATE:                                                  # restart the single process from the ranks' state
            getattr(one, k)[:used].copy_(torch.cat([b0[k], b1[k]])[:used])
        one.pstate.copy_(b0["pstate"])
        before = {k: getattr(one, k)[:used].clone() for k in STATE}
        gs = [_grads(r, step) for r in range(world)]
        mean = {n: (gs[0][n] + gs[1][n]) / world for n in SHAPES}
        one.accumulate(mean)
        coef = R.clip_coef(float(S.sumsq(list(mean.values()))), 1.0)
        norm = float(one.step())
        assert abs(norm - n0) <= 1e-12 * norm
        assert (step == 0) == (norm > 1.0), "step 0 is the clipped one"
        after = {k: torch.cat([a0[k], a1[k]])[:used] for k in STATE}
        for k in ("exp_avg", "exp_avg_sq", "s", "p0"):
            assert torch.equal(after[k], getattr(one, k)[:used]), f"step {step}: {k} differs -- same fp32 arithmetic on the same numbers"
        sc_b, sc_w, sc_1 = b0["pstate"].tolist(), a0["pstate"].tolist(), one.pstate.tolist()
        d, dlr = sc_b[I["d"]], sc_1[I["dlr"]]
        assert sc_w[I["dlr"]] == dlr and sc_w[I["k"]] == sc_1[I["k"]] == step + 1
        flat_g = torch.cat([mean[n].reshape(-1) for n in one.layout.names])
        B = R.bounds_moments(before["master"], before["p0"], flat_g, before["exp_avg"], before["exp_avg_sq"], before["s"], d, dlr, hp, coef)
        dot_b, abs_b = 2 * B["dot_order"], 2 * B["sum_abs_order"]
        assert abs(sc_w[I["sum_dot"]] - sc_1[I["sum_dot"]]) <= dot_b and abs(sc_w[I["sum_abs"]] - sc_1[I["sum_abs"]]) <= abs_b
        bd = R.MARGIN * R.bound_d_hat(d, dlr, sc_1[I["d_numerator"]], sc_1[I["d_denom"]], dot_b, abs_b, hp)
        assert abs(sc_w[I["d_hat"]] - sc_1[I["d_hat"]]) <= bd and abs(sc_w[I["d"]] - sc_1[I["d"]]) <= bd, (step, sc_w, sc_1)
        moved = moved or sc_1[I["d"]] > d
        m64, v64 = (one.exp_avg[:used].double().numpy(), one.exp_avg_sq[:used].double().numpy())
        denom = np.sqrt(v64) + sc_1[I["d"]] * hp["eps"]
        bp = R.MARGIN * R.bounds_apply(before["master"], m64, v64, sc_1[I["d"]], dlr, hp) + np.abs(dlr * m64) * hp["eps"] * bd / denom ** 2
        diff = np.abs(after["master"].double().numpy() - one.master[:used].double().numpy())
        assert np.all(diff <= bp), (step, float(np.max(diff / bp)))
        assert not torch.equal(after["master"], before["master"])
    assert moved, "d never left d0: the scalar comparison above saw nothing"
    # micro-batch mean: (ga + gb) / 2 in one pass carries one more fp32 rounding per element than the two passes' sum times 1 / 4:
    # <= 2u relative on every gradient; d_hat is a quotient of sums that are linear in the gradients and in the state those
    # perturbed gradients built, so <= 4u per step it has been through, 16u after three; x4 for the cancellation in sum g (p0 - p)
    (sa, sm, pm) = micro0
    assert sa["k"] == sm["k"] == 3 and sa["d"] > KW["prodigy"]["d0"]
    assert abs(sa["d"] - sm["d"]) <= 64 * R.U * sm["d"], (sa["d"], sm["d"])
    assert micro1[0] == sa and micro1[1] == sm
    for n in SHAPES:
        torch.testing.assert_close(pm[n][0].float(), pm[n][1].float(), rtol=0, atol=2 ** -8 * 0.1)
