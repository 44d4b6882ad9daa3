"""Timing of the optimiser step alone, Prodigy beside AdamW, on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_prodigy.py [--steps 5] [--warmup 2] [--layers 57] [--out profiles/prodigy.json]

The cfg 5 trainable set (``training.trainable_names`` over the full-size denoiser's shapes: 4.04 B parameters) as bf16 tensors with
random bf16 gradients -- no model, no forward or backward.  Four phases, each with its own tensors, freed before the next:

  per-tensor   ``optim.PerTensorState.step``, the optimiser of ``DenoiserTrainStep.optimizer_step`` (``fk_sumsq`` + ``fk_adamw_step`` per
               tensor | ``fk_sumsq``, ``fk_prodigy_begin``, ``fk_prodigy_moments`` per tensor, ``fk_prodigy_update_d``, ``fk_prodigy_apply``
               per tensor) around the bare parameters;
  sharded      ``zero.ShardedAdamW(...).step()`` at world 1; the cast of the gradients into its fp32 chunks (``accumulate``) is
               outside the bracket, as it runs during the backward pass.

Each timed step is one bracket of HIP events around the call (``--warmup`` steps first); per phase the median, every sample, the
peak of ``torch.cuda.max_memory_allocated`` and the bytes per parameter the median implies at the kernels' nominal traffic.
No threshold is asserted anywhere.
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BF = torch.bfloat16
# nominal HBM bytes per parameter of one optimiser step (reads + writes; fp32 state, bf16 copy; + the gradient norm's read of g)
NOMINAL = {("adamw", "per_tensor"): 28 + 2 + 2, ("adamw", "sharded"): 28 + 4 + 4,
           ("prodigy", "per_tensor"): 32 + 2 + 18 + 2, ("prodigy", "sharded"): 32 + 4 + 18 + 4}


def trainable_shapes(layers):
    from gpt_image_edit_amd import flux_spec, training
    shapes = flux_spec.flux_param_shapes(dict(flux_spec.FLUX_KONTEXT_CONFIG))
    names = training.trainable_names(list(shapes), layers_to_train=tuple(range(layers)))
    return {k: tuple(shapes[k]) for k in names}


def make(shapes, device, seed, scale):
    g = torch.Generator(device=device).manual_seed(seed)
    return {k: (scale * torch.randn(s, generator=g, device=device)).to(BF) for k, s in shapes.items()}


def bracket(fn, before, steps, warmup):
    ms = []
    for i in range(warmup + steps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return ms


def per_tensor(optimizer, params, grads):
    """The unsharded optimiser of ``DenoiserTrainStep`` around bare parameters."""
    from gpt_image_edit_amd.optim import PerTensorState
    st = PerTensorState(params.__getitem__, optimizer, weight_decay=0.01)
    return (lambda: st.step(grads)), (lambda: None), st


def sharded(optimizer, params, grads):
    from gpt_image_edit_amd.zero import ShardedAdamW, backward_order
    opt = ShardedAdamW(params, weight_decay=0.01, optimizer=optimizer, order=backward_order(list(params)))
    return opt.step, (lambda: opt.accumulate(grads)), opt


def phase(optimizer, path, shapes, args, device):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(device)
    params, grads = make(shapes, device, 0, 0.02), make(shapes, device, 1, 1e-3)
    n = sum(p.numel() for p in params.values())
    fn, before, keep = (per_tensor if path == "per_tensor" else sharded)(optimizer, params, grads)
    ms = bracket(fn, before, args.steps, args.warmup)
    med = statistics.median(ms)
    res = dict(optimizer=optimizer, path=path, params=n, tensors=len(params), ms_median=med, ms=ms,
               peak_memory_gb=torch.cuda.max_memory_allocated(device) / 1e9, nominal_bytes_per_param=NOMINAL[optimizer, path],
               nominal_tb_per_s=NOMINAL[optimizer, path] * n / 1e12 / (med / 1e3))
    if optimizer == "prodigy":
        res["scalars"] = keep.prodigy_state()
    del fn, before, keep, params, grads
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=57, help="train the first N of the 57 blocks (57 = the cfg 5 set)")
    ap.add_argument("--out", default="profiles/prodigy.json")
    args = ap.parse_args()
    if args.steps < 3 or args.warmup < 2:
        raise SystemExit("at least 2 warm-up and 3 timed steps")
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    dev = "cuda"
    shapes = trainable_shapes(args.layers)
    res = dict(device=torch.cuda.get_device_name(0), what="optimiser step alone on the cfg 5 trainable set", layers=args.layers,
               steps=args.steps, warmup=args.warmup, phases=[])
    for path in ("per_tensor", "sharded"):
        for optimizer in ("adamw", "prodigy"):
            r = phase(optimizer, path, shapes, args, dev)
            res["phases"].append(r)
            print(json.dumps({k: v for k, v in r.items() if k not in ("ms", "scalars")}), flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
