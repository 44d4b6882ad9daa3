"""Timing of the LoRA merge on one MI355X (development aid; bench.py is the contract benchmark).

    python tools/bench_lora_merge.py [--ranks 16,64,128] [--reps 5] [--workload cfg2_single_512x512_28step]
                                     [--out profiles/lora_merge.json]

Full-size model (19 + 38 blocks, synthetic weights), one synthetic adapter per rank on EVERY 2-D weight of the blocks:

1. the memory floor measured on the same box: a plain ``copy_`` of each touched weight from its saved base (2 B read + 2 B
   written per element, what the merge moves), ms and GB/s over all of them;
2. the merge: ``set_lora_scale`` alternating between two scales, so every touched weight is re-merged from its base by one
   ``fk_lora_merge_bf16`` launch -- ms and GB/s (weight bytes read + written; the adapters are not counted);
3. the edit's images per second without an adapter and with one merged (the same launches: the figures should agree), and
   the first call after a scale change (merge + re-pack of the fused copies + the edit).

No threshold is asserted anywhere.
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


def ms_of(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    cur = torch.cuda.current_stream()
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(cur)
        fn()
        e1.record(cur)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def seconds_of(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def synthetic_adapter(tr, rank, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    st = {}
    for name, p in tr.named_parameters():
        if p.dim() == 2 and name.endswith(".weight") and ("transformer_blocks." in name):
            mod = name[:-len(".weight")]
            n, k = p.shape
            st[f"transformer.{mod}.lora_A.weight"] = (0.01 * torch.randn(rank, k, generator=g, device="cuda")).to(torch.bfloat16)
            st[f"transformer.{mod}.lora_B.weight"] = (0.01 * torch.randn(n, rank, generator=g, device="cuda")).to(torch.bfloat16)
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="16,64,128")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workload", default="cfg2_single_512x512_28step")
    ap.add_argument("--out", default="profiles/lora_merge.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: a timing from anything else says nothing")
    import bench
    pipe = bench.build_pipeline("cuda")
    tr = pipe.transformer
    inp = bench.make_inputs(args.workload, "cuda", 0)
    B = inp["B"]
    lat = pipe._pack_latents(inp["noise"], B, 16, inp["H"] // 8, inp["W"] // 8)
    kw = dict(image=inp["cond"], prompt_embeds=inp["emb"], pooled_prompt_embeds=inp["pooled"], height=inp["H"], width=inp["W"],
              num_inference_steps=28, guidance_scale=3.5, latents=lat, output_type="latent", max_area=inp["H"] * inp["W"],
              _auto_resize=False)
    res = dict(device=torch.cuda.get_device_name(0), workload=args.workload, graph=bool(pipe.use_graph), ranks=[])
    plain = seconds_of(lambda: pipe(**kw), args.reps)
    res["plain_images_per_s_median"] = B / statistics.median(plain)
    print(json.dumps({"plain_images_per_s_median": res["plain_images_per_s_median"]}), flush=True)
    for rank in [int(r) for r in args.ranks.split(",")]:
        pipe.load_lora_weights(synthetic_adapter(tr, rank, seed=rank), adapter_name="bench")
        names = sorted(tr._lora_base)
        elems = sum(tr._lora_base[n].numel() for n in names)
        gbytes = 4 * elems / 1e9                                   # 2 B read + 2 B written per weight element
        scratch = {n: torch.empty_like(tr._lora_base[n]) for n in names}
        copy_ms = ms_of(lambda: [scratch[n].copy_(tr._lora_base[n]) for n in names], args.reps)
        scales = [0.5, 1.0]
        state = {"i": 0}

        def remerge():
            state["i"] += 1
            tr.set_lora_scale(scales[state["i"] % 2])

        merge_ms = ms_of(remerge, args.reps)
        tr.set_lora_scale(1.0)
        with_adapter = seconds_of(lambda: pipe(**kw), args.reps)

        def rescaled_edit():
            state["i"] += 1
            pipe(**kw, joint_attention_kwargs={"scale": scales[state["i"] % 2]})

        first_call = seconds_of(rescaled_edit, args.reps)
        entry = dict(rank=rank, weights=len(names), weight_elements=elems,
                     copy_ms_median=statistics.median(copy_ms), copy_gb_per_s=gbytes / (statistics.median(copy_ms) / 1e3),
                     merge_ms_median=statistics.median(merge_ms), merge_gb_per_s=gbytes / (statistics.median(merge_ms) / 1e3),
                     copy_ms=copy_ms, merge_ms=merge_ms,
                     adapter_images_per_s_median=B / statistics.median(with_adapter),
                     rescaled_call_images_per_s_median=B / statistics.median(first_call),
                     note="merge_ms includes the host loop over the weights (one launch each); rescaled call = merge + re-pack + edit")
        res["ranks"].append(entry)
        print(json.dumps({k: v for k, v in entry.items() if k not in ("copy_ms", "merge_ms")}), flush=True)
        pipe.unload_lora_weights()
        del scratch
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
