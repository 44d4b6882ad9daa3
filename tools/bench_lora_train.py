"""Timing of LoRA training on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_lora_train.py [--ranks 16,64,128] [--steps 3] [--warmup 2] [--out profiles/lora_train.json]
    python tools/bench_lora_train.py --data_parallel [--micro_batches 2] [--ranks 16] [--out profiles/lora_train_dp.json]
    python tools/bench_lora_train.py --lora_backward factored [--ranks 16,128] [--out profiles/lora_train_factored.json]

Full-size model (19 + 38 blocks, synthetic weights) at the cfg 5 shape (1024^2, batch 1: 512 text + 4096 target + 4096 condition
tokens), ready ``prompt_embeds`` (no projector on either side):

1. the full stage-2 step, ``DenoiserTrainStep(model)`` on the reference's trainable set with per-tensor fp32 state -- the code of
   the commit before LoRA training, unchanged by it -- ms per step and ``torch.cuda.max_memory_allocated``;
2. per rank, the LoRA step ``DenoiserTrainStep(model, lora=...)`` on the default targets: the same two figures;
3. per rank, the summed time of the ``fk_lora_grad_bf16`` launches of one step (one per target weight, on the q / k / v row blocks
   of a [3D, D] gradient as the step issues them) beside the wgrad GEMMs they follow (``backward.wgrad`` at the step's token
   count), both on random operands, each list timed as one bracket of events.

With ``--data_parallel`` (world 1; ``--micro_batches N`` backward passes per step, default 1) the record is the flat mode beside
the per-tensor one, to ``profiles/lora_train_dp.json``: per rank, ms per step and peak memory of ``DenoiserTrainStep(model, lora=...)``
and of ``DenoiserTrainStep(model, lora=..., data_parallel=True)`` on the same batches (with N > 1 the per-tensor step runs the same N
backward passes, each overwriting the last: the same work, not the same mathematics), and the summed time of one step's
projection launches in overwrite form (``fk_lora_grad_bf16``) and in accumulate form (``fk_lora_grad_acc_bf16``, accumulate = 1).
The full stage-2 step is left out of this record.

With ``--lora_backward factored`` the record is the factored backward beside the projected one (the step as it was before the
keyword), to ``profiles/lora_train_factored.json``: per rank, two models in ONE process, both warmed, then timed steps taken in turn
(projected, factored, projected, ...) so that clock and temperature drift hit both alike; and the summed time of one step's side
launches (``fk_lora_side_grad_bf16``: three kernels per call, on the q / k / v column blocks of a [S, 3D] gradient as the step
issues them) beside the wgrad GEMMs plus projection launches they replace.  Whichever is faster is recorded as measured.

Every phase builds its own model and frees it; peak memory is reset in between.  No threshold is asserted anywhere.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16


def batch_of(device):
    g = torch.Generator(device=device).manual_seed(7)
    B, h, w, S_txt = 1, 128, 128, 512
    return dict(model_input=torch.randn(B, 16, h, w, generator=g, device=device),
                cond_latents=torch.randn(B, 16, h, w, generator=g, device=device),
                noise=torch.randn(B, 16, h, w, generator=g, device=device),
                sigmas=torch.rand(B, generator=g, device=device) * 0.8 + 0.1,
                prompt_embeds=torch.randn(B, S_txt, 4096, generator=g, device=device).to(BF),
                pooled=torch.randn(B, 768, generator=g, device=device).to(BF)), S_txt + 2 * (h // 2) * (w // 2)


def timed_steps(ts, batch, steps, warmup, micro_batches=1):
    def one():
        for _ in range(micro_batches - 1):
            ts.forward_backward(**batch)
        return ts.step(**batch)
    for _ in range(warmup):
        out = one()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = one()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(out["loss"]).all()
    return ms


def phase(build, steps, warmup, device, micro_batches=1):
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(device)
    model = HipFluxTransformer2DModel(dict(flux_spec.FLUX_KONTEXT_CONFIG), device=device, init="synthetic", seed=0)
    ts = build(model)
    batch, _ = batch_of(device)
    ms = timed_steps(ts, batch, steps, warmup, micro_batches)
    n_train = sum(ts._param(k).numel() for k in ts.trainable_names())
    res = dict(ms_per_step_median=statistics.median(ms), ms_per_step=ms, trainable_params=n_train,
               peak_memory_gb=torch.cuda.max_memory_allocated(device) / 1e9)
    del ts, model, batch
    return res


def paired_steps(builds, steps, warmup, device):
    """ms per step of several steps objects, each on a model of its own, timed in turn within one process."""
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    gc.collect()
    torch.cuda.empty_cache()
    batch, _ = batch_of(device)
    arms = {}
    for name, build in builds.items():
        model = HipFluxTransformer2DModel(dict(flux_spec.FLUX_KONTEXT_CONFIG), device=device, init="synthetic", seed=0)
        arms[name] = build(model)
    for ts in arms.values():
        for _ in range(warmup):
            ts.step(**batch)
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    loss = {}
    for _ in range(steps):
        for name, ts in arms.items():
            t0 = time.perf_counter()
            out = ts.step(**batch)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            loss[name] = float(out["loss"])
    res = {name: dict(ms_per_step_median=statistics.median(v), ms_per_step_min=min(v), ms_per_step=v, last_loss=loss[name],
                      wgrad_set=len(arms[name].bw.trainable), side_targets=len(arms[name].bw.side)) for name, v in ms.items()}
    del arms, batch
    return res


def side_kernels(rank, S, device, reps, D=3072, n_double=19, n_single=38):
    """One step's side launches on the default targets beside the wgrad GEMMs + projections they replace, on random operands."""
    from gpt_image_edit_amd import backward, ops
    g = torch.Generator(device=device).manual_seed(rank)
    rnd = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g, device=device)).to(BF)  # noqa: E731
    dy3, dy1, x = rnd(1, S, 3 * D, s=0.02), rnd(1, S, D, s=0.02), rnd(1, S, D)
    bufs = {}

    def buf(name, shape, zero=False):
        if name not in bufs:
            bufs[name] = (torch.zeros if zero else torch.empty)(shape, device=device, dtype=BF)
        return bufs[name]
    dw3, dw1 = torch.empty(3 * D, D, device=device, dtype=BF), torch.empty(D, D, device=device, dtype=BF)
    up, down = rnd(D, rank, s=0.02), rnd(rank, D, s=0.02)
    d_up, d_down = torch.empty(D, rank, device=device), torch.empty(rank, D, device=device)
    ws, sws = ops.lora_grad_ws(D, D, rank, device), ops.lora_side_grad_ws(1, S, D, D, rank, device)

    def replaced():
        for _ in range(n_double + n_single):
            backward.wgrad(buf, dy3, x, out=dw3)
            for k in range(3):
                ops.lora_grad(dw3[k * D:(k + 1) * D], up, down, 1.0, d_up=d_up, d_down=d_down, ws=ws)
        for _ in range(n_double):
            backward.wgrad(buf, dy1, x, out=dw1)
            ops.lora_grad(dw1, up, down, 1.0, d_up=d_up, d_down=d_down, ws=ws)

    def side():
        for _ in range(n_double + n_single):
            for k in range(3):
                ops.lora_side_grad(x, dy3[:, :, k * D:(k + 1) * D], up, down, 1.0, d_up=d_up, d_down=d_down, ws=sws)
        for _ in range(n_double):
            ops.lora_side_grad(x, dy1, up, down, 1.0, d_up=d_up, d_down=d_down, ws=sws)
    n = 3 * (n_double + n_single) + n_double
    r, f = [], []
    for _ in range(reps):                      # in turn, one repetition each
        r += bracket_ms(replaced, 1)
        f += bracket_ms(side, 1)
    return dict(targets=n, rows=S, replaced_ms_median=statistics.median(r), side_ms_median=statistics.median(f),
                side_us_per_target=1e3 * statistics.median(f) / n, side_over_replaced=statistics.median(f) / statistics.median(r),
                side_gb_per_s=n * 2 * 2 * 2 * S * D / 1e9 / (statistics.median(f) / 1e3),   # X and dY read twice each, 2 B per element
                replaced_ms=r, side_ms=f, note="both brackets include the host loop (one ctypes call per launch group)")


def bracket_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def kernels(rank, S, device, reps, D=3072, n_double=19, n_single=38, accumulate_arm=False):
    """One step's projection launches beside the wgrad GEMMs in front of them, on random operands."""
    from gpt_image_edit_amd import backward, ops
    g = torch.Generator(device=device).manual_seed(rank)
    rnd = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=g, device=device)).to(BF)  # noqa: E731
    dy3, dy1, x = rnd(1, S, 3 * D, s=0.02), rnd(1, S, D, s=0.02), rnd(1, S, D)
    bufs = {}

    def buf(name, shape, zero=False):
        if name not in bufs:
            bufs[name] = (torch.zeros if zero else torch.empty)(shape, device=device, dtype=BF)
        return bufs[name]
    dw3, dw1 = torch.empty(3 * D, D, device=device, dtype=BF), torch.empty(D, D, device=device, dtype=BF)
    up, down = rnd(D, rank, s=0.02), rnd(rank, D, s=0.02)
    d_up, d_down = torch.empty(D, rank, device=device), torch.empty(rank, D, device=device)
    ws = ops.lora_grad_ws(D, D, rank, device)

    def wgrads():
        for _ in range(n_double + n_single):
            backward.wgrad(buf, dy3, x, out=dw3)
        for _ in range(n_double):
            backward.wgrad(buf, dy1, x, out=dw1)

    def projections(accumulate=False):
        for _ in range(n_double + n_single):
            for k in range(3):
                ops.lora_grad(dw3[k * D:(k + 1) * D], up, down, 1.0, d_up=d_up, d_down=d_down, ws=ws, accumulate=accumulate)
        for _ in range(n_double):
            ops.lora_grad(dw1, up, down, 1.0, d_up=d_up, d_down=d_down, ws=ws, accumulate=accumulate)
    n = 3 * (n_double + n_single) + n_double
    if accumulate_arm:
        d_up.zero_(), d_down.zero_()
        p, a = bracket_ms(projections, reps), bracket_ms(lambda: projections(True), reps)
        return dict(launches=n, overwrite_ms_median=statistics.median(p), accumulate_ms_median=statistics.median(a),
                    accumulate_over_overwrite=statistics.median(a) / statistics.median(p), overwrite_ms=p, accumulate_ms=a,
                    note="both brackets include the host loop (one ctypes call per launch)")
    w, p = bracket_ms(wgrads, reps), bracket_ms(projections, reps)
    return dict(launches=n, wgrad_ms_median=statistics.median(w), lora_grad_ms_median=statistics.median(p),
                lora_grad_us_per_launch=1e3 * statistics.median(p) / n,
                lora_grad_gb_per_s=n * 4 * D * D / 1e9 / (statistics.median(p) / 1e3),       # dW read twice: 4 B per element
                lora_grad_over_wgrad=statistics.median(p) / statistics.median(w), wgrad_ms=w, lora_grad_ms=p,
                note="projection bracket includes the host loop (one ctypes call per launch)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="16,64,128")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip_full", action="store_true", help="leave out the full stage-2 step (48 GB of optimiser state)")
    ap.add_argument("--data_parallel", action="store_true", help="record the flat data_parallel=True step beside the per-tensor one")
    ap.add_argument("--micro_batches", type=int, default=1, help="backward passes per step (with --data_parallel)")
    ap.add_argument("--lora_backward", default="projected", choices=["projected", "factored"],
                    help="factored: record the factored backward beside the projected one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.lora_backward == "factored" and args.data_parallel:
        raise SystemExit("--lora_backward factored is a record of its own")
    if args.out is None:
        args.out = ("profiles/lora_train_dp.json" if args.data_parallel else "profiles/lora_train_factored.json"
                    if args.lora_backward == "factored" else "profiles/lora_train.json")
    if args.micro_batches != 1 and not args.data_parallel:
        raise SystemExit("--micro_batches belongs to --data_parallel")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    dev = "cuda"
    _, S = batch_of(dev)
    res = dict(device=torch.cuda.get_device_name(0), shape="cfg5 1024x1024 bs1", seq_len=S, steps=args.steps, warmup=args.warmup, ranks=[])
    if args.lora_backward == "factored":
        for rank in [int(r) for r in args.ranks.split(",")]:
            def build(m, mode, rank=rank):
                m.add_lora_adapter("bench", rank=rank)
                return DenoiserTrainStep(m, lora="bench", lora_backward=mode)
            entry = dict(rank=rank, kernels=side_kernels(rank, S, dev, args.reps),
                         **paired_steps({mode: (lambda m, mode=mode: build(m, mode)) for mode in ("projected", "factored")},
                                        args.steps, args.warmup, dev))
            res["ranks"].append(entry)
            print(json.dumps({"rank": rank, **{a: {k: v for k, v in entry[a].items() if k != "ms_per_step"} for a in ("projected", "factored")},
                              "kernels": {k: v for k, v in entry["kernels"].items() if not k.endswith("_ms")}}), flush=True)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    if args.data_parallel:
        res.update(world=1, micro_batches=args.micro_batches)
        for rank in [int(r) for r in args.ranks.split(",")]:
            def build(m, dp, rank=rank):
                m.add_lora_adapter("bench", rank=rank)
                return DenoiserTrainStep(m, lora="bench", data_parallel=dp)
            entry = dict(rank=rank,
                         lora_step=phase(lambda m: build(m, False), args.steps, args.warmup, dev, args.micro_batches),
                         lora_dp_step=phase(lambda m: build(m, True), args.steps, args.warmup, dev, args.micro_batches),
                         kernels=kernels(rank, S, dev, args.reps, accumulate_arm=True))
            res["ranks"].append(entry)
            print(json.dumps({"rank": rank, **{a: {k: v for k, v in entry[a].items() if k != "ms_per_step"} for a in ("lora_step", "lora_dp_step")},
                              "kernels": {k: v for k, v in entry["kernels"].items() if not k.endswith("_ms")}}), flush=True)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    if not args.skip_full:
        res["full_step"] = phase(lambda m: DenoiserTrainStep(m), args.steps, args.warmup, dev)
        print(json.dumps({"full_step": {k: v for k, v in res["full_step"].items() if k != "ms_per_step"}}), flush=True)
    for rank in [int(r) for r in args.ranks.split(",")]:
        def build(m, rank=rank):
            m.add_lora_adapter("bench", rank=rank)
            return DenoiserTrainStep(m, lora="bench")
        entry = dict(rank=rank, lora_step=phase(build, args.steps, args.warmup, dev), kernels=kernels(rank, S, dev, args.reps))
        res["ranks"].append(entry)
        print(json.dumps({"rank": rank, "lora_step": {k: v for k, v in entry["lora_step"].items() if k != "ms_per_step"},
                          "kernels": {k: v for k, v in entry["kernels"].items() if not k.endswith("_ms")}}), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
