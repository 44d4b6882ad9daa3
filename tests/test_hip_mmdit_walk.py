"""The tile walk of the large-tile GEMMs through the MMDiT block schedule: the walk bits of the launch plan must reach every
block GEMM on all three block APIs (per-kernel calls, one C call per block, one per forward: fk_block_ws.gemm_plan), and the
blocks' own launch shapes -- grouped image + text launches with the fused QKV epilogue and a token offset, gated residuals in
place, batches that end inside a row tile -- must give the bits of the one-workgroup-per-tile launch.

Small shapes never exceed the CU count, so nothing else in the suite runs a model-level GEMM under the walk; here a cap on the
workgroups forces it.  Full width, one double and one single block, B = 2, S_txt = 77, 2 x 16 x 16 image tokens (S = 589 rows per
batch in the single block: the batch ends inside a row tile).  With the forced form every block GEMM of N % 256 == 0 has more
tiles than the caps 1 and 5 and therefore walks:
  double block, image (M = 1024) + text (M = 154) grouped:  fused QKV N = 9216 (180 tiles of 256 x 256), out-proj N = 3072 (60),
      MLP-up N = 12288 (240), MLP-down N = 3072 (60)
  single block (M = 1178, 5 row tiles):  fused QKV N = 9216 (180), MLP-up N = 12288 with GELU (240), out-proj N = 3072 over
      K = 15360 with the gated residual (60)
(the mixed form 384 cuts the same launches into more, smaller tiles).  The embedders' GEMMs in front of the blocks have a
handful of rows and keep the small kernel.

One MI355X run: both tests pass, 0.9 s and 0.3 s.  Control, on the copy of the library described in
tests/test_hip_gemm_walk_exact.py (the walk's bias quads taken from the next tile's columns): both tests fail, and the six walk
forwards of each -- caps 1 and 5 on each of the three block APIs -- all differ from the reference in 98.8 % of the output
elements while the tile_per_wg forwards of the two C routes still equal it: the walk bits reach the block GEMMs on every route.
"""
import pytest
import torch

from test_hip_mmdit import _inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("variant", (256, 384))
def test_walk_through_the_block_schedule_gives_the_same_bits(variant):
    """One reference forward (tile_per_wg, BLOCK_API 0) and six under the walk (caps 1 and 5 x BLOCK_API 0, 1, 2), and the
    tile_per_wg forward on the two C routes: all outputs equal and finite."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import flux_spec, ops, transformer
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=1)
    model = transformer.HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=29)
    B, S_txt, h, w = 2, 77, 16, 16
    assert (S_txt + 2 * h * w) % 256 != 0
    hs, enc, pooled, t, gd, img_ids, txt_ids = _inputs(B, S_txt, h, w, cfg, seed=13)
    kw = dict(hidden_states=hs.cuda(), timestep=t.cuda(), guidance=gd.cuda(), pooled_projections=pooled.cuda(),
              encoder_hidden_states=enc.cuda(), txt_ids=txt_ids.cuda(), img_ids=img_ids.cuda(), return_dict=False)
    saved = transformer.BLOCK_API
    try:
        ops.gemm_set_variant(variant)
        outs = {}
        for api in (0, 1, 2):
            transformer.BLOCK_API = api
            ops.gemm_set_walk("tile_per_wg")
            outs[("tile_per_wg", 0, api)] = model(**kw)[0].clone()
            for cap in (1, 5):
                ops.gemm_set_walk("walk", cap)
                outs[("walk", cap, api)] = model(**kw)[0].clone()
        torch.cuda.synchronize()
        ref = outs[("tile_per_wg", 0, 0)]
        assert ref.shape == (B, 2 * h * w, 64) and torch.isfinite(ref.float()).all()
        bad = [f"{key[0]} cap {key[1]} BLOCK_API {key[2]}: {int((o != ref).sum())} of {ref.numel()} elements"
               for key, o in outs.items() if not torch.equal(o, ref)]
        assert not bad, f"form {variant}: outputs differ from the one-workgroup-per-tile forward of BLOCK_API 0 -- " + "; ".join(bad)
    finally:
        transformer.BLOCK_API = saved
        ops.gemm_set_variant(0)
        ops.gemm_set_walk("default")
