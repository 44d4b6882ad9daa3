"""Timing of the masked-edit step on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_inpaint.py [--no-edit] [--out profiles/inpaint_timing.json]

1. ``fk_euler_inpaint_step_bf16`` (with a mask) beside ``fk_euler_step_bf16`` per launch at the 512^2 and 1024^2 edit shapes
   (S_tgt = 1024 / 4096 target rows in a [1, 2 S_tgt, 64] token buffer, C = 64): HIP events around windows of back-to-back
   launches, the two kernels alternating window by window, median over the windows.  Back-to-back launches of a
   microsecond kernel measure the launch rate as much as the kernel: the figure is time per launch, not kernel time.
2. Edited images per second of a masked edit (half the picture repainted) beside the plain edit, full-size model, the
   flagship 512^2 workload of bench.py, alternating, each call ended by a device synchronise.
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

BF = torch.bfloat16


def window(fn, launches):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(launches):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3        # us per launch


def step_timing(S, launches=2000, windows=7):
    C = 64
    g = torch.Generator(device="cuda").manual_seed(S)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda").to(BF)  # noqa: E731
    x, v, x0, noise = rnd(1, 2 * S, C), rnd(1, 2 * S, C), rnd(1, S, C), rnd(1, S, C)
    mask = (torch.rand(1, S, 4, generator=g, device="cuda") < 0.5).to(BF)
    # dsigma = 0 keeps x finite over thousands of in-place launches; the kernels do the same work for any value
    fns = {"fk_euler_step_bf16": lambda: ops.euler_step(x, v, S, 0.0),
           "fk_euler_inpaint_step_bf16": lambda: ops.euler_inpaint_step(x, v, S, 0.0, 0.5, x0, noise, mask)}
    for fn in fns.values():
        window(fn, 200)
    samples = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            samples[k].append(window(fn, launches))
    bytes_ = {"fk_euler_step_bf16": 3 * S * C * 2, "fk_euler_inpaint_step_bf16": 5 * S * C * 2 + 8 * S}
    return {k: dict(S_tgt=S, C=C, us_per_launch_median=statistics.median(v_), us_per_launch_min=min(v_),
                    us_per_launch_max=max(v_), launches_per_window=launches, windows=windows,
                    algorithmic_bytes=bytes_[k]) for k, v_ in samples.items()}


def edit_timing(reps=3):
    import bench
    wl = "cfg2_single_512x512_28step"
    pipe = bench.build_pipeline("cuda")
    inp = bench.make_inputs(wl, "cuda", 0)
    lat = pipe._pack_latents(inp["noise"], inp["B"], 16, inp["H"] // 8, inp["W"] // 8)
    mask = torch.zeros(1, 1, inp["H"], inp["W"])
    mask[..., : inp["W"] // 2] = 1
    kw = dict(image=inp["cond"], prompt_embeds=inp["emb"], pooled_prompt_embeds=inp["pooled"], height=inp["H"],
              width=inp["W"], num_inference_steps=28, guidance_scale=3.5, latents=lat, output_type="pt_raw",
              max_area=inp["H"] * inp["W"], _auto_resize=False)
    calls = {"plain_edit": lambda: pipe(**kw), "masked_edit_half": lambda: pipe(mask_image=mask, **kw)}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    secs = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
    return {k: dict(workload=wl, batch=inp["B"], images_per_s_median=inp["B"] / statistics.median(v), seconds=v,
                    graph=bool(pipe.use_graph)) for k, v in secs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-edit", action="store_true")
    ap.add_argument("--out", default="profiles/inpaint_timing.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    res = {"step": [step_timing(S) for S in (1024, 4096)]}
    print(json.dumps(res["step"], indent=1), flush=True)
    if not args.no_edit:
        res["edit"] = edit_timing()
        print(json.dumps(res["edit"], indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
