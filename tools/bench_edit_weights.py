"""Timing of the edit-region weight stages on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_edit_weights.py [--out profiles/edit_weights.json]

For one 448^2 and one 1024^2 (reference, target) pair -- the target is the reference with one repainted rectangle, speckles and
pinholes (tests/edit_weights_ref.py: edit_pair) -- it records
  * the time per launch of each stage (``ops.edit_diff_mask`` .. ``ops.mask_weight_fill``) from HIP events around windows of
    back-to-back launches, median over the windows.  Back-to-back launches of a short kernel measure the launch rate as much as
    the kernel: the figure is time per launch, not kernel time;
  * ``edit_region_weights`` as a whole, its one read-back included, each call timed on the host between device synchronises;
  * the numpy restatement of the same chain on this host's CPU (its labelling is a plain Python BFS: the figure says what the
    tests' reference costs, not what OpenCV would).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import edit_weights_ref as R  # noqa: E402
from gpt_image_edit_amd import edit_weights, ops  # noqa: E402


def window(fn, launches):
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(launches):
        fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3        # us per launch


def timing(side, launches=100, windows=5, reps=5):
    ref_np, tgt_np = R.edit_pair(side, side, seed=side, speckles=40, pinholes=40)
    ref, tgt = torch.from_numpy(ref_np)[None].cuda(), torch.from_numpy(tgt_np)[None].cuda()
    diff = ops.edit_diff_mask(ref, tgt)
    closed = ops.mask_close5(diff)
    ws = ops.mask_components_ws(1, side, side, "cuda")
    kept = ops.mask_filter_components(closed, ws=ws)
    mask_ds, counts = ops.mask_and_pool8(kept[None], status=ws)
    wvec = torch.tensor([2.0], device="cuda")
    out_d, out_c, out_k, out_w = torch.empty_like(diff), torch.empty_like(diff), torch.empty_like(diff), None
    fns = {"edit_diff_mask": lambda: ops.edit_diff_mask(ref, tgt, out=out_d),
           "mask_close5": lambda: ops.mask_close5(diff, out=out_c),
           "mask_filter_components (5 launches)": lambda: ops.mask_filter_components(closed, out=out_k, ws=ws, check=False),
           "mask_and_pool8 (4 launches, 2 buffers)": lambda: ops.mask_and_pool8(kept[None], status=ws),
           "mask_weight_fill": lambda: ops.mask_weight_fill(mask_ds, wvec, out=out_w)}
    for fn in fns.values():
        window(fn, 10)
    samples = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            samples[k].append(window(fn, launches))
    entry = {k: dict(us_per_launch_median=statistics.median(v), us_per_launch_min=min(v), us_per_launch_max=max(v),
                     launches_per_window=launches, windows=windows) for k, v in samples.items()}
    refs5 = ref[:, None]
    edit_weights.edit_region_weights(refs5, tgt)
    secs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = edit_weights.edit_region_weights(refs5, tgt)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    entry["edit_region_weights (whole call, one read-back)"] = dict(us_per_call_median=statistics.median(secs) * 1e6,
                                                                    us_per_call_min=min(secs) * 1e6, calls=reps)
    t0 = time.perf_counter()
    want = R.chain(ref_np[None, None], tgt_np[None])
    cpu = time.perf_counter() - t0
    same = bool(np.array_equal(got[0].cpu().numpy(), want[0]) and torch.equal(got[1].cpu(), want[1]))
    entry["numpy restatement on the host CPU (Python BFS labelling)"] = dict(us_per_call=cpu * 1e6, equal_to_the_kernels=same)
    return dict(picture=[side, side], references=1, white_pixels_of_the_intersection=int(counts[0, 0]), timings=entry)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/edit_weights.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    res = {"device": torch.cuda.get_device_name(0), "edit_weights": [timing(448), timing(1024)]}
    print(json.dumps(res, indent=1), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
