"""Child process of tests/test_hip_mxfp8_fused.py: FK_MX_FUSED_QUANT and FK_BLOCK_API are read when the package is imported, so
every setting gets a fresh interpreter.  Runs a 2 + 4-block mxfp8 model forward (B = 2, ragged rows), counts the standalone
quantizer launches of that forward, then a short edit eagerly and through the captured graph, and saves the results.

usage: python mxfp8_fused_child.py OUT.pt      (settings come from the environment)"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out_path):
    from gpt_image_edit_amd import flux_spec, ops, transformer
    from test_hip_mxfp8_model import _edit, _edit_setup, _kw
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=2, num_single_layers=4)
    model = transformer.HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=31, weight_format="mxfp8")
    kw = _kw(2, 77, 10, 12, cfg, seed=4)
    model(**kw)                                   # packs the weights (their quantizer launches are not the forward's)
    torch.cuda.synchronize()
    n0 = ops.quantize_launch_count()
    fwd = model(**kw)[0].clone()
    torch.cuda.synchronize()
    launches = ops.quantize_launch_count() - n0
    tr, (eager, graphed) = _edit_setup((False, True))
    tr.set_weight_format("mxfp8")
    res = dict(fused=int(transformer.MX_FUSED_QUANT), api=int(transformer.BLOCK_API), launches=launches, fwd=fwd.cpu())
    for seed in (2, 3):                           # the graphed pipeline captures with seed 2 and replays with seed 3
        res[f"eager{seed}"] = _edit(eager, seed, 4).cpu()
        res[f"graph{seed}"] = _edit(graphed, seed, 4).cpu()
    torch.cuda.synchronize()
    torch.save(res, out_path)
    print(f"[child] fused={res['fused']} api={res['api']} quantizer launches per forward: {launches}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
