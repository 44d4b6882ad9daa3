"""MXFP8 vs bf16 weight format, interleaved in one process on one GPU.

Edits (default): the cfg 2 edit (BASELINE.json configs[1]: 512^2, S = 2560) and the 1024^2 edit with bench.py's synthetic
full-depth pipeline, bench.py's protocol per arm (warm-up edits, then timed edits between synchronizes), the arms alternating
bf16 / mxfp8 round by round on ONE model (``set_weight_format``).  Prints images/s per arm.

GEMMs (--gemms, also after the edits unless --no-gemms): every block GEMM shape of the cfg 2 forward, the bf16 launch against
quantize_mxfp8 (activation) + gemm_mxfp8 (pre-quantized weight): median us, TF/s, the quantizer's share.

One mxfp8 edit for a kernel trace: ``rocprofv3 --kernel-trace --stats -d DIR -o ab -- python tools/mxfp8_ab.py --one-edit``.

    python tools/mxfp8_ab.py [--rounds 2] [--steps 3] [--warmup 1] [--gemms | --no-gemms]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gpt_image_edit_amd import ops  # noqa: E402

# (name, M, N, K, epilogue): the block GEMMs of the cfg 2 edit (B = 1, S_txt = 512, S_img = 2560 incl. the condition tokens)
SHAPES = [("double img qkv", 2560, 9216, 3072), ("double txt qkv", 512, 9216, 3072),
          ("double img to_out", 2560, 3072, 3072), ("double txt to_add_out", 512, 3072, 3072),
          ("double img ff.0", 2560, 12288, 3072), ("double txt ff.0", 512, 12288, 3072),
          ("double img ff.2", 2560, 3072, 12288), ("double txt ff.2", 512, 3072, 12288),
          ("single qkv+mlp", 3072, 21504, 3072), ("single proj_out", 3072, 3072, 15360)]


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / iters


def edits(args):
    import time

    import bench
    pipe = bench.build_pipeline("cuda")
    tr = pipe.transformer
    print(f"# mxfp8_ab edits: {torch.cuda.get_device_name(0)}, full depth, per arm {args.warmup} warm-up + {args.steps} timed "
          f"edits, {args.rounds} interleaved rounds", flush=True)
    for workload in ("cfg2_single_512x512_28step", "single_1024x1024_28step"):
        inp = bench.make_inputs(workload, "cuda", seed=0)
        res = {"bf16": [], "mxfp8": []}
        for _ in range(args.rounds):
            for fmt in ("bf16", "mxfp8"):
                tr.set_weight_format(fmt)
                for _ in range(args.warmup):
                    out = bench.run_edit(pipe, inp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    out = bench.run_edit(pipe, inp)
                torch.cuda.synchronize()
                assert torch.isfinite(out.images.float()).all()
                res[fmt].append(args.steps * inp["B"] / (time.perf_counter() - t0))
        bf, mx = statistics.median(res["bf16"]), statistics.median(res["mxfp8"])
        print(f"{workload:28s} bf16 {bf:.4f} images/s  mxfp8 {mx:.4f} images/s  ratio {mx / bf:.3f}   "
              f"(rounds bf16 {' '.join(f'{x:.4f}' for x in res['bf16'])} | mxfp8 {' '.join(f'{x:.4f}' for x in res['mxfp8'])})",
              flush=True)
    tr.set_weight_format("bf16")


def one_edit():
    import bench
    pipe = bench.build_pipeline("cuda")
    pipe.transformer.set_weight_format("mxfp8")
    inp = bench.make_inputs("cfg2_single_512x512_28step", "cuda", seed=0)
    bench.run_edit(pipe, inp)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2, help="interleaved rounds (edits); GEMMs use 5")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--gemms", action="store_true", help="GEMM table only")
    ap.add_argument("--no-gemms", action="store_true")
    ap.add_argument("--one-edit", action="store_true", help="one mxfp8 cfg 2 edit (for a kernel trace)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    if args.one_edit:
        return one_edit()
    if not args.gemms:
        edits(args)
    if not args.no_gemms:
        gemms(args)


def gemms(args):
    g = torch.Generator().manual_seed(0)
    rounds = 5
    print(f"# mxfp8_ab gemms: {torch.cuda.get_device_name(0)}, {rounds} interleaved rounds x {args.iters} launches, median per launch")
    print(f"{'shape':20s} {'M':>5s} {'N':>6s} {'K':>6s} | {'bf16 us':>9s} {'TF/s':>6s} | {'quant us':>8s} {'mx gemm us':>10s} "
          f"{'TF/s':>6s} {'mx total':>9s} | {'speedup':>7s} {'gemm only':>9s} {'tile':>4s}")
    tot_bf = tot_mx = tot_q = 0.0
    for name, M, N, K in SHAPES:
        a = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).cuda()
        w = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda()
        b = (torch.randn(N, generator=g) * 0.1).to(torch.bfloat16).cuda()
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        wq = ops.quantize_mxfp8(w)
        aq = ops.quantize_mxfp8(a)
        f_bf = lambda: ops.gemm(a, w, b, out=out)                       # noqa: E731
        f_q = lambda: ops.quantize_mxfp8(a, q=aq[0], scales=aq[1])      # noqa: E731
        f_mx = lambda: ops.gemm_mxfp8(aq, wq, b, out=out)               # noqa: E731
        for f in (f_bf, f_q, f_mx):
            timed(f, 3)
        t_bf, t_q, t_mx = [], [], []
        for _ in range(rounds):
            t_bf.append(timed(f_bf, args.iters))
            t_q.append(timed(f_q, args.iters))
            t_mx.append(timed(f_mx, args.iters))
        tile = ops.gemm_last_variant()
        bf, q, mx = statistics.median(t_bf), statistics.median(t_q), statistics.median(t_mx)
        fl = 2.0 * M * N * K
        tot_bf, tot_mx, tot_q = tot_bf + bf, tot_mx + mx + q, tot_q + q
        print(f"{name:20s} {M:5d} {N:6d} {K:6d} | {bf:9.1f} {fl / bf / 1e6:6.0f} | {q:8.1f} {mx:10.1f} {fl / mx / 1e6:6.0f} "
              f"{mx + q:9.1f} | {bf / (mx + q):7.3f} {bf / mx:9.3f} {tile:4d}")
    print(f"{'sum (one of each)':20s} {'':5s} {'':6s} {'':6s} | {tot_bf:9.1f} {'':6s} | {tot_q:8.1f} {tot_mx - tot_q:10.1f} {'':6s} "
          f"{tot_mx:9.1f} | {tot_bf / tot_mx:7.3f} {tot_bf / (tot_mx - tot_q):9.3f}")


if __name__ == "__main__":
    main()
