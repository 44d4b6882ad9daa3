"""Fused vs unfused MXFP8 activation quantization, and both against the bf16 edit -- and, with --parent-tree, against another
checkout's MXFP8 edit (the commit this schedule is judged against).

A third MXFP8 arm, "mxfp8 fused+attn" (FK_MX_FUSED_QUANT=1 FK_MX_FUSED_ATTN=1), adds the attention forward that emits its consumer's
quantized operand itself: no standalone quantizer launch is left in a forward.  Its record belongs in profiles/ beside the fused
A/B's; until one exists the switch's gain is unmeasured and its default stays 0.

FK_MX_FUSED_QUANT / FK_MX_FUSED_ATTN are read at import and a parent tree is other code, so every arm of every round is a FRESH child process;
the arms alternate round by round on one GPU (interleaved: box drift hits all arms alike).  A child builds bench.py's synthetic
full-depth pipeline, then per workload runs warm-up edits and times each following edit with HIP events; it prints the median.

    python tools/mxfp8_fused_ab.py [--rounds 3] [--steps 3] [--warmup 1] [--parent-tree DIR] [--sizes cfg2,1024]
    rocprofv3 --kernel-trace --stats -d DIR -o fused -- python tools/mxfp8_fused_ab.py --child mxfp8 --one-edit   (FK_MX_FUSED_QUANT=1)

The verdict line applies the repository's bar for keeping a default: the fused arm's WORST round must beat the reference arm's
BEST round (the parent tree's when given, else this tree's unfused switch) at cfg 2; for the fused+attn arm the reference is the
fused arm (what the switch is added to)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"cfg2": "cfg2_single_512x512_28step", "1024": "single_1024x1024_28step"}


def child(args):
    sys.path.insert(0, args.tree)
    os.chdir(args.tree)
    import torch
    import bench
    torch.cuda.set_device(0)
    pipe = bench.build_pipeline("cuda")
    pipe.transformer.set_weight_format(args.child)
    out = {}
    for size in args.sizes.split(","):
        inp = bench.make_inputs(WORKLOADS[size], "cuda", seed=0)
        for _ in range(args.warmup):
            res = bench.run_edit(pipe, inp)
        torch.cuda.synchronize()
        if args.one_edit:
            return
        ms = []
        for _ in range(args.steps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            res = bench.run_edit(pipe, inp)
            e.record()
            e.synchronize()
            ms.append(s.elapsed_time(e))
        assert torch.isfinite(res.images.float()).all()
        out[size] = inp["B"] * 1e3 / statistics.median(ms)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", default="cfg2,1024")
    ap.add_argument("--parent-tree", help="a built checkout of the commit to compare against")
    ap.add_argument("--child", choices=("bf16", "mxfp8"), help="(internal) run one arm in this process")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--one-edit", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    # (name, tree, weight format, FK_MX_FUSED_QUANT, FK_MX_FUSED_ATTN)
    arms = [("mxfp8 unfused", ROOT, "mxfp8", "0", "0"), ("mxfp8 fused", ROOT, "mxfp8", "1", "0"),
            ("mxfp8 fused+attn", ROOT, "mxfp8", "1", "1"), ("bf16", ROOT, "bf16", "1", "0")]
    if args.parent_tree:
        arms.insert(0, ("mxfp8 parent", os.path.abspath(args.parent_tree), "mxfp8", "1", "0"))
    sizes = args.sizes.split(",")
    res = {a[0]: {s: [] for s in sizes} for a in arms}
    print(f"# mxfp8_fused_ab: {args.rounds} interleaved rounds, a fresh process per arm and round, per workload {args.warmup} warm-up + "
          f"{args.steps} timed edits (HIP events, median); images/s", flush=True)
    for r in range(args.rounds):
        for name, tree, fmt, fused, fused_attn in arms:
            env = dict(os.environ, FK_MX_FUSED_QUANT=fused, FK_MX_FUSED_ATTN=fused_attn)
            env.pop("FK_LIB_PATH", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", fmt, "--tree", tree, "--steps", str(args.steps),
                                "--warmup", str(args.warmup), "--sizes", args.sizes], env=env, capture_output=True, text=True, timeout=900)
            line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(f"arm {name!r} failed in round {r} (exit {p.returncode}):\n{p.stderr[-2000:]}", flush=True)
                return 1                       # nothing more is started on the GPU after a failed arm
            got = json.loads(line[-1][7:])
            for s in sizes:
                res[name][s].append(got[s])
            print(f"round {r} {name:16s} " + "  ".join(f"{s} {got[s]:.4f}" for s in sizes), flush=True)
    for s in sizes:
        print(f"## {WORKLOADS[s]}")
        for name, *_ in arms:
            v = res[name][s]
            print(f"{name:16s} median {statistics.median(v):.4f}  best {max(v):.4f}  worst {min(v):.4f}   ({' '.join(f'{x:.4f}' for x in v)})")
        bf = statistics.median(res["bf16"][s])
        print("ratios to bf16: " + "  ".join(f"{name} {statistics.median(res[name][s]) / bf:.3f}" for name, *_ in arms if name != "bf16"))
    ref = "mxfp8 parent" if args.parent_tree else "mxfp8 unfused"
    if "cfg2" in sizes:
        worst, best = min(res["mxfp8 fused"]["cfg2"]), max(res[ref]["cfg2"])
        print(f"verdict (cfg 2): fused worst {worst:.4f} vs {ref} best {best:.4f}: the fused default "
              f"{'meets' if worst > best else 'does NOT meet'} the bar")
        worst, best = min(res["mxfp8 fused+attn"]["cfg2"]), max(res["mxfp8 fused"]["cfg2"])
        print(f"verdict (cfg 2): fused+attn worst {worst:.4f} vs mxfp8 fused best {best:.4f}: the FK_MX_FUSED_ATTN default "
              f"{'meets' if worst > best else 'does NOT meet'} the bar")
    return 0


if __name__ == "__main__":
    sys.exit(main())
