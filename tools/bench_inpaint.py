"""Timing of the masked-edit step on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_inpaint.py [--no-edit] [--out profiles/inpaint_timing.json]
    python tools/bench_inpaint.py --overlay [--no-edit] [--out profiles/inpaint_overlay.json]

1. ``fk_euler_inpaint_step_bf16`` (with a mask) beside ``fk_euler_step_bf16`` per launch at the 512^2 and 1024^2 edit shapes
   (S_tgt = 1024 / 4096 target rows in a [1, 2 S_tgt, 64] token buffer, C = 64): HIP events around windows of back-to-back
   launches, the two kernels alternating window by window, median over the windows.  Back-to-back launches of a
   microsecond kernel measure the launch rate as much as the kernel: the figure is time per launch, not kernel time.
2. Edited images per second of a masked edit (half the picture repainted) beside the plain edit, full-size model, the
   flagship 512^2 workload of bench.py, alternating, each call ended by a device synchronise.

``--overlay``: the same two measurements for the crop / feather / overlay kernels -- per-launch time of ``fk_mask_bbox_u8``,
``fk_mask_blur_u8`` (sigma 4), ``fk_pixels_u8_box_to_nhwc_bf16`` and ``fk_image_overlay_u8`` at a 1024^2 picture with a 512^2 box,
beside ``fk_pixels_u8_to_nhwc_bf16`` and ``fk_image_to_u8_nhwc`` at 512^2 in the same run, and images per second of a crop +
overlay edit beside the plain masked edit (both return uint8 pixels).

``--resample`` (``python tools/bench_inpaint.py --resample [--out profiles/resample.json]``): per-launch time of the two passes of
``fk_resample_pass_u8`` and of ``ops.resample_u8`` as a whole, three filters, 3000 x 4000 -> 768 x 1024 and 1024^2 -> 512^2, beside
``fk_pixels_u8_to_nhwc_bf16`` at the same sizes and Pillow's own time for the same call on the host CPU.
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


def overlay_kernel_timing(launches=500, windows=7):
    P, S, box = 1024, 512, (256, 256, 768, 768)
    g = torch.Generator(device="cuda").manual_seed(P)
    pic = torch.randint(0, 256, (1, P, P, 3), generator=g, device="cuda", dtype=torch.uint8)
    small = pic[:, :S, :S].contiguous()
    mask = torch.zeros(1, P, P, device="cuda", dtype=torch.uint8)
    mask[:, box[1]:box[3], box[0]:box[2]] = 255
    img = (torch.rand(1, 3, S, S, generator=g, device="cuda") * 2 - 1).to(BF)
    out4, ws = torch.empty(4, device="cuda", dtype=torch.int32), torch.empty(16384, device="cuda", dtype=torch.int32)
    blurred, crop, over = torch.empty_like(mask), torch.empty(1, S, S, 32, device="cuda", dtype=BF), torch.empty_like(pic)
    fns = {"fk_mask_bbox_u8": lambda: ops.mask_bbox(mask, 1, out=out4, ws=ws),
           "fk_mask_blur_u8(sigma=4)": lambda: ops.mask_blur(mask, 4.0, out=blurred),        # + its tap upload and plane allocation
           "fk_pixels_u8_box_to_nhwc_bf16": lambda: ops.pixels_box_to_nhwc(pic, box, S, S, 32, False, out=crop),
           "fk_image_overlay_u8": lambda: ops.image_overlay(img, pic, mask, box, out=over),
           "fk_pixels_u8_to_nhwc_bf16": lambda: ops.pixels_to_nhwc(small, S, S, 32, False),
           "fk_image_to_u8_nhwc": lambda: ops.image_to_u8(img)}
    bytes_ = {"fk_mask_bbox_u8": P * P, "fk_mask_blur_u8(sigma=4)": P * P * (1 + 4 + 4 + 1),
              "fk_pixels_u8_box_to_nhwc_bf16": S * S * 3 + S * S * 32 * 2, "fk_image_overlay_u8": S * S * 3 * 2 + P * P * (3 + 1 + 3),
              "fk_pixels_u8_to_nhwc_bf16": S * S * 3 + S * S * 32 * 2, "fk_image_to_u8_nhwc": S * S * 3 * (2 + 1)}
    for fn in fns.values():
        window(fn, 50)
    samples = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            samples[k].append(window(fn, launches))
    return {k: dict(picture=P, box=S, us_per_launch_median=statistics.median(v_), us_per_launch_min=min(v_),
                    us_per_launch_max=max(v_), launches_per_window=launches, windows=windows, algorithmic_bytes=bytes_[k])
            for k, v_ in samples.items()}


def overlay_edit_timing(reps=3):
    import bench
    wl = "cfg2_single_512x512_28step"
    pipe = bench.build_pipeline("cuda")
    inp = bench.make_inputs(wl, "cuda", 0)
    H, W = inp["H"], inp["W"]
    lat = pipe._pack_latents(inp["noise"], inp["B"], 16, H // 8, W // 8)
    g = torch.Generator().manual_seed(0)
    pic = torch.randint(0, 256, (1, 2 * H, 2 * W, 3), generator=g, dtype=torch.uint8)     # a picture four times the model's area
    mask = torch.zeros(2 * H, 2 * W, dtype=torch.uint8)
    mask[H // 2:H // 2 + H, W // 2:W // 2 + W] = 255                                      # the box is the model's resolution
    kw = dict(image=pic, mask_image=mask, prompt_embeds=inp["emb"], pooled_prompt_embeds=inp["pooled"], height=H, width=W,
              num_inference_steps=28, guidance_scale=3.5, latents=lat, output_type="np_uint8", max_area=H * W, _auto_resize=False)
    calls = {"masked_edit": lambda: pipe(**kw), "crop_overlay_edit": lambda: pipe(padding_mask_crop=0, **kw),
             "crop_blur_overlay_edit": lambda: pipe(padding_mask_crop=32, mask_blur=4.0, **kw)}
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
    return {k: dict(workload=wl, picture=[2 * H, 2 * W], batch=inp["B"], images_per_s_median=inp["B"] / statistics.median(v),
                    seconds=v, graph=bool(pipe.use_graph)) for k, v in secs.items()}


def resample_timing(launches=50, windows=5):
    """Per launch: the horizontal pass, the vertical pass and ``resample_u8`` as a whole (both launches, the intermediate's
    allocation, the cached tables) for the three filters at 3000 x 4000 -> 768 x 1024 and 1024^2 -> 512^2, beside the nearest
    gather ``fk_pixels_u8_to_nhwc_bf16`` at the same sizes, and Pillow's time for the same call on this host's CPU (one thread)."""
    import numpy as np
    res = []
    for (Hin, Win), (Hout, Wout) in (((3000, 4000), (768, 1024)), ((1024, 1024), (512, 512))):
        g = torch.Generator(device="cuda").manual_seed(Hin)
        pic = torch.randint(0, 256, (1, Hin, Win, 3), generator=g, device="cuda", dtype=torch.uint8)
        mid = torch.empty(1, Hin, Wout, 3, device="cuda", dtype=torch.uint8)
        out = torch.empty(1, Hout, Wout, 3, device="cuda", dtype=torch.uint8)
        fns = {"fk_pixels_u8_to_nhwc_bf16": lambda: ops.pixels_to_nhwc(pic, Hout, Wout, 32, False)}
        for f in ("bilinear", "bicubic", "lanczos"):
            ops.resample_pass_u8(pic, 1, Wout, f, out=mid)
            fns[f"fk_resample_pass_u8(horizontal, {f})"] = lambda f=f: ops.resample_pass_u8(pic, 1, Wout, f, out=mid)
            fns[f"fk_resample_pass_u8(vertical, {f})"] = lambda f=f: ops.resample_pass_u8(mid, 0, Hout, f, out=out)
            fns[f"resample_u8({f})"] = lambda f=f: ops.resample_u8(pic, Hout, Wout, f)
        for fn in fns.values():
            window(fn, 5)
        samples = {k: [] for k in fns}
        for _ in range(windows):
            for k, fn in fns.items():
                samples[k].append(window(fn, launches))
        entry = {k: dict(us_per_launch_median=statistics.median(v), us_per_launch_min=min(v), us_per_launch_max=max(v),
                         launches_per_window=launches, windows=windows) for k, v in samples.items()}
        try:
            from PIL import Image
            im = Image.fromarray(pic[0].cpu().numpy())
            for f, flt in (("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC), ("lanczos", Image.LANCZOS)):
                secs = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    ref = im.resize((Wout, Hout), flt)
                    secs.append(time.perf_counter() - t0)
                same = bool(np.array_equal(np.asarray(ref), ops.resample_u8(pic, Hout, Wout, f)[0].cpu().numpy()))
                entry[f"PIL.Image.resize({f}) on the host CPU"] = dict(us_per_call_median=statistics.median(secs) * 1e6,
                                                                        equal_to_the_kernel=same)
        except ImportError:
            entry["PIL.Image.resize"] = "Pillow is not installed"
        res.append(dict(source=[Hin, Win], target=[Hout, Wout], channels=3, timings=entry))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-edit", action="store_true")
    ap.add_argument("--overlay", action="store_true", help="time the crop / feather / overlay kernels and edits instead")
    ap.add_argument("--resample", action="store_true", help="time the antialiased byte resize (fk_resample_pass_u8) instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or ("profiles/resample.json" if args.resample else
                            "profiles/inpaint_overlay.json" if args.overlay else "profiles/inpaint_timing.json")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    if args.resample:
        res = {"resample": resample_timing()}
        print(json.dumps(res, indent=1), flush=True)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    if args.overlay:
        res = {"kernels": overlay_kernel_timing()}
        print(json.dumps(res["kernels"], indent=1), flush=True)
        if not args.no_edit:
            res["edit"] = overlay_edit_timing()
            print(json.dumps(res["edit"], indent=1), flush=True)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
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
