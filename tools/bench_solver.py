"""Cost and drift of the second-order multistep (AB2) solver on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_solver.py [--workloads cfg2_single_512x512_28step,single_1024x1024_28step] [--reps 3]
                                 [--out profiles/solver_ab2.json]

1. Step kernel time: HIP events around ``--launches`` back-to-back launches of ``fk_ab2_step_bf16`` (without and with a mask,
   with the history term) beside ``fk_euler_step_bf16`` and ``fk_euler_inpaint_step_bf16``, at S_tgt = 1024 and 4096
   (B = 1, C = 64); microseconds per launch, median over ``--reps`` repeats.
2. Per workload (full-size model, synthetic weights, the inputs of bench.py): images per second of the Euler edit at 28 steps
   and of the AB2 edit at 28, 20, 16 and 14 steps (each call ended by a device synchronise, median of ``--reps`` calls after one
   warm-up), and cosine / max-abs of each one's final latents against a 224-step Euler edit of the same noise.

``--latent_state`` runs another arm instead and writes ``profiles/solver_f32_state.json``: the step launch of
``fk_solver_step_f32`` (Euler and AB2 form, without and with a mask) beside ``fk_euler_step_bf16`` and ``fk_ab2_step_bf16`` in the
same run, and per workload the Euler and the AB2 edit at 28, 20, 16 and 14 steps with the bf16 and with the float32 latent state:
images per second, and cosine / max-abs of the final latents against a 224-step Euler edit run WITH the float32 state.

Synthetic weights make the velocity field unrepresentative of a real checkpoint: the figures say what a step costs and how far
the latents of a shorter schedule land from a long Euler run of THIS field, NOT what a picture looks like.  No step count is
recommended and nothing here is a threshold.
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
from gpt_image_edit_amd import ops  # noqa: E402
from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler  # noqa: E402

BF = torch.bfloat16
REFERENCE_STEPS = 224
AB2_STEPS = (28, 20, 16, 14)


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


def launch_times(arms, s_tgt, launches, reps):
    """us per launch of each arm: HIP events around ``launches`` back-to-back calls, ``reps`` repeats after one warm-up call."""
    cur = torch.cuda.current_stream()
    out = {}
    for name, fn in arms.items():
        fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            for _ in range(launches):
                fn()
            e1.record(cur)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / launches)
        out[name] = dict(us_per_launch_median=statistics.median(us), us_per_launch=us)
    return dict(S_tgt=s_tgt, B=1, C=64, launches=launches,
                note="HIP events around back-to-back eager launches: launch overhead of the ctypes call included", kernels=out)


def kernel_times(s_tgt, launches, reps):
    """us per launch of the four step entry points at [1, s_tgt, 64]; coefficients of 0 keep the tokens what they are."""
    g = torch.Generator().manual_seed(0)
    x, v, hist, x0, noise = (torch.randn(1, s_tgt, 64, generator=g).to(BF).cuda() for _ in range(5))
    mask = (torch.rand(1, s_tgt, 4, generator=g) < 0.5).to(BF).cuda()
    arms = {
        "fk_euler_step_bf16": lambda: ops.euler_step(x, v, s_tgt, 0.0),
        "fk_euler_inpaint_step_bf16 (mask)": lambda: ops.euler_inpaint_step(x, v, s_tgt, 0.0, 0.5, x0, noise, mask),
        "fk_ab2_step_bf16": lambda: ops.ab2_step(x, v, hist, s_tgt, 0.0, 0.0, 1),
        "fk_ab2_step_bf16 (mask)": lambda: ops.ab2_step(x, v, hist, s_tgt, 0.0, 0.0, 1, 0.5, x0, noise, mask),
    }
    return launch_times(arms, s_tgt, launches, reps)


def state_kernel_times(s_tgt, launches, reps):
    """us per launch of the float32-state step beside the two bf16 steps, measured the same way in the same process."""
    g = torch.Generator().manual_seed(0)
    x, v, hist, x0, noise = (torch.randn(1, s_tgt, 64, generator=g).to(BF).cuda() for _ in range(5))
    state = x.float()
    mask = (torch.rand(1, s_tgt, 4, generator=g) < 0.5).to(BF).cuda()
    arms = {
        "fk_euler_step_bf16": lambda: ops.euler_step(x, v, s_tgt, 0.0),
        "fk_ab2_step_bf16": lambda: ops.ab2_step(x, v, hist, s_tgt, 0.0, 0.0, 1),
        "fk_solver_step_f32 (euler)": lambda: ops.solver_step_f32(state, x, v, s_tgt, 0.0),
        "fk_solver_step_f32 (ab2)": lambda: ops.solver_step_f32(state, x, v, s_tgt, 0.0, 0.0, 1, 1, hist),
        "fk_solver_step_f32 (euler, seeding step)": lambda: ops.solver_step_f32(state, x, v, s_tgt, 0.0, load_state=0),
        "fk_solver_step_f32 (ab2, mask)": lambda: ops.solver_step_f32(state, x, v, s_tgt, 0.0, 0.0, 1, 1, hist, 0.5, x0, noise, mask),
    }
    return launch_times(arms, s_tgt, launches, reps)


def run_state_workload(bench, pipe, wl, reps):
    """Both solvers at every step count with both latent states, against a 224-step Euler edit on the float32 state."""
    inp = bench.make_inputs(wl, "cuda", 0)
    B = inp["B"]
    lat = pipe._pack_latents(inp["noise"], B, 16, inp["H"] // 8, inp["W"] // 8)
    kw = dict(image=inp["cond"], prompt_embeds=inp["emb"], pooled_prompt_embeds=inp["pooled"], height=inp["H"], width=inp["W"],
              guidance_scale=3.5, latents=lat, output_type="latent", max_area=inp["H"] * inp["W"], _auto_resize=False)
    scheds = {"euler": FlowMatchEulerDiscreteScheduler(), "ab2": FlowMatchMultistepScheduler()}
    res = dict(workload=wl, batch=B, graph=bool(pipe.use_graph), reps=reps, reference_steps=REFERENCE_STEPS,
               reference="euler, latent_state=fp32", runs=[])
    pipe.scheduler = scheds["euler"]
    base = pipe(**kw, num_inference_steps=REFERENCE_STEPS, latent_state="fp32").latents.float()
    res["max_abs_reference"] = base.abs().max().item()
    for solver in ("euler", "ab2"):
        pipe.scheduler = scheds[solver]
        for n in AB2_STEPS:
            for state in ("bf16", "fp32"):
                secs = timed(lambda: pipe(**kw, num_inference_steps=n, latent_state=state), reps)
                out = pipe(**kw, num_inference_steps=n, latent_state=state).latents.float()
                entry = dict(solver=solver, steps=n, latent_state=state, images_per_s_median=B / statistics.median(secs),
                             seconds=secs,
                             cosine_vs_reference=torch.nn.functional.cosine_similarity(out.flatten(), base.flatten(), dim=0).item(),
                             max_abs_vs_reference=(out - base).abs().max().item(), finite=bool(torch.isfinite(out).all()))
                res["runs"].append(entry)
                print(json.dumps({wl: {k: v for k, v in entry.items() if k != "seconds"}}), flush=True)
    pipe.scheduler = scheds["euler"]
    return res


def run_workload(bench, pipe, wl, reps):
    inp = bench.make_inputs(wl, "cuda", 0)
    B = inp["B"]
    lat = pipe._pack_latents(inp["noise"], B, 16, inp["H"] // 8, inp["W"] // 8)
    kw = dict(image=inp["cond"], prompt_embeds=inp["emb"], pooled_prompt_embeds=inp["pooled"], height=inp["H"], width=inp["W"],
              guidance_scale=3.5, latents=lat, output_type="latent", max_area=inp["H"] * inp["W"], _auto_resize=False)
    euler, ab2 = FlowMatchEulerDiscreteScheduler(), FlowMatchMultistepScheduler()
    res = dict(workload=wl, batch=B, graph=bool(pipe.use_graph), reps=reps, reference_steps=REFERENCE_STEPS, runs=[])
    pipe.scheduler = euler
    base = pipe(**kw, num_inference_steps=REFERENCE_STEPS).latents.float()
    res["max_abs_reference"] = base.abs().max().item()
    for solver, sched, n in [("euler", euler, 28)] + [("ab2", ab2, n) for n in AB2_STEPS]:
        pipe.scheduler = sched
        secs = timed(lambda: pipe(**kw, num_inference_steps=n), reps)
        out = pipe(**kw, num_inference_steps=n).latents.float()
        entry = dict(solver=solver, steps=n, images_per_s_median=B / statistics.median(secs), seconds=secs,
                     cosine_vs_reference=torch.nn.functional.cosine_similarity(out.flatten(), base.flatten(), dim=0).item(),
                     max_abs_vs_reference=(out - base).abs().max().item(), finite=bool(torch.isfinite(out).all()))
        res["runs"].append(entry)
        print(json.dumps({wl: {k: v for k, v in entry.items() if k != "seconds"}}), flush=True)
    pipe.scheduler = euler
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg2_single_512x512_28step,single_1024x1024_28step")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None, help="default: profiles/solver_ab2.json, or profiles/solver_f32_state.json with --latent_state")
    ap.add_argument("--latent_state", action="store_true",
                    help="the float32-latent-state arm instead: both solvers, both states, fk_solver_step_f32's launch time")
    args = ap.parse_args()
    if args.out is None:
        args.out = "profiles/solver_f32_state.json" if args.latent_state else "profiles/solver_ab2.json"
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    import bench
    times, workload = (state_kernel_times, run_state_workload) if args.latent_state else (kernel_times, run_workload)
    res = dict(device=torch.cuda.get_device_name(0),
               weights="synthetic: the velocity field is not a real checkpoint's, the drift figures say nothing about pictures",
               step_kernels=[times(s, args.launches, max(args.reps, 5)) for s in (1024, 4096)])
    print(json.dumps({"step_kernels": [{k["S_tgt"]: {n: round(v["us_per_launch_median"], 2) for n, v in k["kernels"].items()}}
                                       for k in res["step_kernels"]]}), flush=True)
    pipe = bench.build_pipeline("cuda")
    res["workloads"] = [workload(bench, pipe, wl, args.reps) for wl in args.workloads.split(",") if wl]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
