"""GPU: edit_region_weights against the CPU chain (tests/edit_weights_ref.py), mask and weights equal, and one training step whose
``area_mask_weights`` come from the GPU call: loss and gradient bits equal those with the CPU-made map."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_weights_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def erw():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gpt_image_edit_amd
    return gpt_image_edit_amd.edit_region_weights


@pytest.fixture(scope="module")
def pairs():
    """(refs [2, 1, H, W, 3], target [2, H, W, 3]) per size: two edit pairs each, made once."""
    out = {}
    for H, W in ((96, 128), (100, 76)):
        two = [R.edit_pair(H, W, seed=H + s) for s in (0, 1)]
        out[H, W] = (np.stack([p[0] for p in two])[:, None], np.stack([p[1] for p in two]))
    return out


def _run(erw, refs, tgt, *args, **kw):
    mask_ds, weights = erw(torch.from_numpy(refs).cuda(), torch.from_numpy(tgt).cuda(), *args, **kw)
    torch.cuda.synchronize()
    assert mask_ds.is_cuda and weights.is_cuda and mask_ds.dtype == torch.uint8 and weights.dtype == torch.float32
    return mask_ds.cpu().numpy(), weights.cpu()


@pytest.mark.parametrize("H, W", [(96, 128), (100, 76)])
@pytest.mark.parametrize("kind", ["log", "exp"])
def test_repainted_rectangle(erw, pairs, H, W, kind):
    refs, tgt = pairs[H, W]
    mask_ds, weights = _run(erw, refs, tgt, kind)
    want_mask, want_w = R.chain(refs, tgt, kind)
    assert np.array_equal(mask_ds, want_mask) and torch.equal(weights, want_w)
    box = np.zeros((1, 1, H, W), dtype=np.uint8)                                 # speckles dropped, pinholes closed: the rectangle
    box[0, 0, H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = 255
    assert np.array_equal(mask_ds[0], R.and_pool8(box)[0][0]) and np.array_equal(mask_ds[1], mask_ds[0])
    assert float(weights.max()) == float(R.weight_scalar(mask_ds[0].size, int((mask_ds[0] == 255).sum()), kind)) > 1.0
    assert float(weights.min()) == 1.0


def test_identical_pictures_next_to_an_edit(erw, pairs):
    refs, tgt = pairs[96, 128]
    tgt = tgt.copy()
    tgt[0] = refs[0, 0]                                                           # sample 0: reconstruction data
    mask_ds, weights = _run(erw, refs, tgt)
    want_mask, want_w = R.chain(refs, tgt)
    assert np.array_equal(mask_ds, want_mask) and torch.equal(weights, want_w)
    assert mask_ds[0].min() == 255 and torch.equal(weights[0], torch.ones(1, 12, 16)) and float(weights[1].max()) > 1.0


def test_a_three_pixel_change_raises(erw, pairs):
    refs, tgt = pairs[96, 128]
    tgt = tgt.copy()
    tgt[1] = refs[1, 0]
    tgt[1, 40, 50:53] ^= 0x80
    with pytest.raises(ValueError, match="TOO SMALL mask_intersect_area_ratio: 0.000244140625, sample 1"):
        _run(erw, refs, tgt)
    with pytest.raises(ValueError, match="TOO SMALL"):
        R.chain(refs, tgt)


def test_two_references(erw, pairs):
    refs, tgt = pairs[100, 76]
    H, W = 100, 76
    other = np.random.default_rng(9).integers(0, 256, refs.shape, dtype=np.uint8)
    second = np.where(np.arange(W)[None, None, None, :, None] < W // 2, other, refs)   # differs from the target on the left half too
    both = np.concatenate([refs, second], 1)
    mask_ds, weights = _run(erw, both, tgt)
    want_mask, want_w = R.chain(both, tgt)
    assert np.array_equal(mask_ds, want_mask) and torch.equal(weights, want_w)
    assert np.array_equal(mask_ds, R.chain(refs, tgt)[0])                         # the intersection is the rectangle again
    with pytest.raises(ValueError, match="sample 0: an empty intersection"):      # two references, nothing edited
        _run(erw, np.concatenate([refs, refs], 1), refs[:, 0].copy())


@pytest.mark.parametrize("kind", ["log", "exp"])
def test_shortcuts(erw, pairs, kind):
    refs, tgt = pairs[100, 76]
    for r, kw in ((refs, dict(need_weight=False)), (refs[:, :0], {})):
        mask_ds, weights = _run(erw, r, tgt, kind, **kw)
        assert mask_ds.shape == (2, 12, 9) and mask_ds.min() == 255 and torch.equal(weights, torch.ones(2, 1, 12, 9))
    with pytest.raises(NotImplementedError, match="found lin"):
        _run(erw, refs, tgt, "lin")


def test_train_step_takes_the_map_from_the_gpu_call(erw, pairs):
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    refs, tgt = pairs[96, 128]
    _, made = erw(torch.from_numpy(refs).cuda(), torch.from_numpy(tgt).cuda())
    _, want = R.chain(refs, tgt)
    assert torch.equal(made.cpu(), want)
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=1)
    model = HipFluxTransformer2DModel(cfg, device="cuda", init="synthetic", seed=11)
    B, h, w, S_txt = 2, 12, 16, 32
    g = torch.Generator().manual_seed(21)
    batch = dict(model_input=torch.randn(B, 16, h, w, generator=g).cuda(), cond_latents=torch.randn(B, 16, h, w, generator=g).cuda(),
                 noise=torch.randn(B, 16, h, w, generator=g).cuda(), sigmas=torch.tensor([0.6, 0.3]).cuda(),
                 prompt_embeds=torch.randn(B, S_txt, 4096, generator=g).to(BF).cuda(),
                 pooled=torch.randn(B, 768, generator=g).to(BF).cuda())
    ts = DenoiserTrainStep(model)
    runs = []
    for area in (made, want.cuda(), None):
        loss, grads, _ = ts.forward_backward(**batch, area_mask_weights=area)
        torch.cuda.synchronize()
        runs.append((loss.clone(), {k: v.clone() for k, v in grads.items()}))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
    assert not torch.equal(runs[0][0], runs[2][0])                                # and the map does weigh the loss
