"""Timing and drift of the step cache on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_step_cache.py [--workloads cfg2_single_512x512_28step,single_1024x1024_28step] [--thresholds 0.05,0.1,0.2,0.4]
                                     [--out profiles/step_cache_timing.json]

Per workload (full-size model, synthetic weights, 28 steps, the inputs of bench.py):

1. plain edit: images per second, each call ended by a device synchronise (median of ``--reps`` calls after one warm-up);
2. one skipped step beside one full step: HIP events around the two-phase forward (``step_cache_begin`` +
   ``step_cache_end``) + the Euler step, ``compute=True`` and ``compute=False`` alternating, median over the repeats;
3. for each threshold of a small grid: the computed steps of the adaptive run, its images per second (eager loop: the mode
   reads 8 bytes back per step), the images per second of the same decisions replayed as a schedule (the pipeline's own route:
   the graph when FK_GRAPH=1), and cosine / max-abs of the final latents against the uncached edit.

``--measure`` is the arm that sets the two measures side by side (``StepCache(measure="input" | "first_block")``), in one process
and per workload: the plain images per second, one first-block skipped step (block 0 + the cached tail) beside one full step of
the same run, and, per measure, the uncached trajectory of the measure and for each threshold the computed steps, the images per
second (adaptive, and the decisions replayed as a schedule) and cosine / max-abs of the final latents against the uncached edit.
The two measures live on different scales, so without ``--thresholds`` each gets the three quartiles of ITS OWN uncached
trajectory: thresholds at which some steps skip and some compute, chosen for what they show about cost, not for quality.

    python tools/bench_step_cache.py --measure [--reps 2] [--out profiles/step_cache_first_block.json]

Synthetic weights make the rel-L1 trajectory unrepresentative of a real checkpoint: the figures say what a skipped step costs
and what a given number of skipped steps buys, NOT which threshold is acceptable.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpt_image_edit_amd.step_cache import StepCache  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    secs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return secs


def step_times(pipe, kw, reps, mode="input"):
    """ms of one full and one skipped step (two-phase forward + Euler step) at the call's shape, through a callback-free
    eager loop of the pipeline's own making: the loop's tensors are those of a real call, taken from a 2-step cached edit.
    ``mode="first_block"``: the skipped step runs block 0 and adds the cached residual of the blocks behind it."""
    tr = pipe.transformer
    grabbed = {}
    orig = pipe._denoise

    def grab(L, *a, **k):
        grabbed["L"] = L
        return orig(L, *a, **k)

    use_graph, pipe.use_graph, pipe._denoise = pipe.use_graph, False, grab
    try:
        pipe(**dict(kw, num_inference_steps=2), step_cache=StepCache(schedule=[0, 1]))
    finally:
        pipe.use_graph, pipe._denoise = use_graph, orig
    L = grabbed["L"]
    from gpt_image_edit_amd import ops
    st = tr.step_cache_state(measure=False, mode=mode)
    fwd = dict(hidden_states=L.model_tokens, timestep=L.t_model[0], guidance=L.guidance, pooled_projections=L.pooled,
               encoder_hidden_states=L.embeds, txt_ids=L.text_ids, img_ids=L.latent_ids, joint_attention_kwargs={})

    def one(compute):
        tr.step_cache_begin(st, **fwd)
        v = tr.step_cache_end(st, compute)
        ops.euler_step(L.tokens, v, L.S_tgt, 0.0)      # dsigma = 0: the tokens stay what they are over the repeats

    one(True), one(False)
    torch.cuda.synchronize()
    ms = {True: [], False: []}
    cur = torch.cuda.current_stream()
    for _ in range(reps):
        for compute in (True, False):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            one(compute)
            e1.record(cur)
            e1.synchronize()
            ms[compute].append(e0.elapsed_time(e1))
    return dict(full_step_ms_median=statistics.median(ms[True]), skipped_step_ms_median=statistics.median(ms[False]),
                full_step_ms=ms[True], skipped_step_ms=ms[False], mode=mode,
                note="eager two-phase forward + Euler step, HIP events")


def run_workload(bench, pipe, wl, thresholds, reps):
    inp = bench.make_inputs(wl, "cuda", 0)
    B = inp["B"]
    lat = pipe._pack_latents(inp["noise"], B, 16, inp["H"] // 8, inp["W"] // 8)
    kw = dict(image=inp["cond"], prompt_embeds=inp["emb"], pooled_prompt_embeds=inp["pooled"], height=inp["H"], width=inp["W"],
              num_inference_steps=28, guidance_scale=3.5, latents=lat, output_type="latent", max_area=inp["H"] * inp["W"],
              _auto_resize=False)
    res = dict(workload=wl, batch=B, graph=bool(pipe.use_graph), steps=28)
    plain = timed(lambda: pipe(**kw), reps)
    base = pipe(**kw).latents.float()
    res["plain"] = dict(images_per_s_median=B / statistics.median(plain), seconds=plain)
    print(json.dumps({wl: res["plain"]}), flush=True)
    res["step"] = step_times(pipe, kw, max(reps, 5))
    print(json.dumps({wl: res["step"]}), flush=True)
    probe = StepCache(threshold=0.0)
    pipe(**kw, step_cache=probe)
    res["rel_l1_uncached"] = probe.rel_l1
    res["thresholds"] = []
    for thr in thresholds:
        sc = StepCache(threshold=thr)
        adaptive = timed(lambda: pipe(**kw, step_cache=sc), reps)
        out = pipe(**kw, step_cache=sc).latents.float()
        steps = list(sc.computed_steps)
        replay = timed(lambda: pipe(**kw, step_cache=StepCache(schedule=steps)), reps)
        same = torch.equal(pipe(**kw, step_cache=StepCache(schedule=steps)).latents.float(), out)
        d = out - base
        entry = dict(threshold=thr, computed_steps=steps, block_passes=len(steps), rel_l1=sc.rel_l1,
                     adaptive_images_per_s_median=B / statistics.median(adaptive), adaptive_seconds=adaptive,
                     schedule_images_per_s_median=B / statistics.median(replay), schedule_seconds=replay,
                     schedule_replay_bit_equal=bool(same),
                     cosine_vs_uncached=torch.nn.functional.cosine_similarity(out.flatten(), base.flatten(), dim=0).item(),
                     max_abs_vs_uncached=d.abs().max().item(), max_abs_uncached=base.abs().max().item())
        res["thresholds"].append(entry)
        print(json.dumps({wl: {k: v for k, v in entry.items() if k not in ("rel_l1", "adaptive_seconds", "schedule_seconds")}}),
              flush=True)
    return res


def quartiles(xs):
    xs = sorted(xs)
    return [xs[min(len(xs) - 1, int(q * len(xs)))] for q in (0.25, 0.5, 0.75)]


def run_measures(bench, pipe, wl, thresholds, reps):
    """The ``--measure`` arm: both measures at one workload (see the module docstring)."""
    inp = bench.make_inputs(wl, "cuda", 0)
    B = inp["B"]
    lat = pipe._pack_latents(inp["noise"], B, 16, inp["H"] // 8, inp["W"] // 8)
    kw = dict(image=inp["cond"], prompt_embeds=inp["emb"], pooled_prompt_embeds=inp["pooled"], height=inp["H"], width=inp["W"],
              num_inference_steps=28, guidance_scale=3.5, latents=lat, output_type="latent", max_area=inp["H"] * inp["W"],
              _auto_resize=False)
    res = dict(workload=wl, batch=B, graph=bool(pipe.use_graph), steps=28, reps=reps)
    plain = timed(lambda: pipe(**kw), reps)
    base = pipe(**kw).latents.float()
    res["plain"] = dict(images_per_s_median=B / statistics.median(plain), seconds=plain)
    print(json.dumps({wl: res["plain"]}), flush=True)
    res["first_block_step"] = step_times(pipe, kw, max(reps, 5), mode="first_block")
    print(json.dumps({wl: {k: v for k, v in res["first_block_step"].items() if k.endswith("median")}}), flush=True)
    res["measures"] = {}
    for measure in ("input", "first_block"):
        probe = StepCache(threshold=0.0, measure=measure)
        same_as_plain = torch.equal(pipe(**kw, step_cache=probe).latents.float(), base)
        grid = thresholds if thresholds else quartiles(probe.rel_l1)
        m = dict(rel_l1_uncached=probe.rel_l1, threshold_zero_bit_equal_to_plain=bool(same_as_plain),
                 thresholds_from="--thresholds" if thresholds else "quartiles of rel_l1_uncached", thresholds=[])
        for thr in grid:
            sc = StepCache(threshold=thr, measure=measure)
            adaptive = timed(lambda: pipe(**kw, step_cache=sc), reps)
            out = pipe(**kw, step_cache=sc).latents.float()
            steps = list(sc.computed_steps)
            replay = timed(lambda: pipe(**kw, step_cache=StepCache(schedule=steps, measure=measure)), reps)
            same = torch.equal(pipe(**kw, step_cache=StepCache(schedule=steps, measure=measure)).latents.float(), out)
            d = out - base
            entry = dict(threshold=thr, computed_steps=steps, block_passes=len(steps), rel_l1=sc.rel_l1,
                         adaptive_images_per_s_median=B / statistics.median(adaptive), adaptive_seconds=adaptive,
                         schedule_images_per_s_median=B / statistics.median(replay), schedule_seconds=replay,
                         schedule_replay_bit_equal=bool(same),
                         cosine_vs_uncached=torch.nn.functional.cosine_similarity(out.flatten(), base.flatten(), dim=0).item(),
                         max_abs_vs_uncached=d.abs().max().item(), max_abs_uncached=base.abs().max().item())
            m["thresholds"].append(entry)
            print(json.dumps({wl: {measure: {k: v for k, v in entry.items()
                                             if k not in ("rel_l1", "adaptive_seconds", "schedule_seconds")}}}), flush=True)
        res["measures"][measure] = m
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg2_single_512x512_28step,single_1024x1024_28step")
    ap.add_argument("--thresholds", default=None, help="default 0.05,0.1,0.2,0.4; with --measure: each measure's own quartiles")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--measure", action="store_true", help="the two measures (input, first_block) side by side")
    ap.add_argument("--out", default=None, help="default profiles/step_cache_timing.json; with --measure profiles/step_cache_first_block.json")
    args = ap.parse_args()
    if args.out is None:
        args.out = "profiles/step_cache_first_block.json" if args.measure else "profiles/step_cache_timing.json"
    if args.thresholds is None and not args.measure:
        args.thresholds = "0.05,0.1,0.2,0.4"
    thresholds = [float(t) for t in args.thresholds.split(",")] if args.thresholds else []
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    import bench
    pipe = bench.build_pipeline("cuda")
    res = dict(device=torch.cuda.get_device_name(0), weights="synthetic: the rel-L1 trajectory is not a real checkpoint's",
               workloads=[(run_measures if args.measure else run_workload)(bench, pipe, wl, thresholds, args.reps)
                          for wl in args.workloads.split(",")])
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
