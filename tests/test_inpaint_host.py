"""Host side of masked (inpaint) edits and ``strength``: where the loop starts, the scheduler's per-step scalars, the compact
token mask against ``_pack_latents``, and the identities of the bf16 step formula that the GPU tests use as their reference.
No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref as R  # noqa: E402

from gpt_image_edit_amd import helpers, ops  # noqa: E402
from gpt_image_edit_amd.scheduler import FlowMatchEulerDiscreteScheduler  # noqa: E402

BF = torch.bfloat16


@pytest.mark.parametrize("n, strength, t_start", [(28, 1.0, 0), (28, 0.5, 14), (6, 0.5, 3), (3, 0.1, 2)])
def test_t_start_table(n, strength, t_start):
    assert helpers.strength_t_start(n, strength) == t_start
    assert n - helpers.strength_t_start(n, strength) >= 1          # (3, 0.1): one step is left


@pytest.mark.parametrize("strength", [0, 0.0, -0.25, 1.0001, 2, float("nan")])
def test_strength_outside_the_half_open_unit_interval_is_refused(strength):
    with pytest.raises(ValueError, match="strength"):
        helpers.strength_t_start(28, strength)


def _shifted(n, s_tgt):
    s = FlowMatchEulerDiscreteScheduler()
    s.set_timesteps(sigmas=np.linspace(1.0, 1 / n, n), mu=helpers.calculate_shift(s_tgt), device="cpu")
    return s


def test_sigma_next_and_dsigma_follow_the_sigma_table():
    for n, s_tgt in ((6, 24), (28, 1024), (3, 4096)):
        s = _shifted(n, s_tgt)
        tab = s._sigmas_host
        assert tab.dtype == np.float32 and len(tab) == n + 1 and tab[-1] == 0.0
        assert abs(tab[n // 2] - np.linspace(1.0, 1 / n, n)[n // 2]) > 1e-3                  # the schedule is shifted
        for i in range(n):
            assert s.sigma_next(i) == float(tab[i + 1])
            assert s.dsigma(i) == float(np.float32(tab[i + 1]) - np.float32(tab[i]))
            assert np.float32(tab[i]) + np.float32(s.dsigma(i)) == pytest.approx(s.sigma_next(i), abs=1e-7)
        assert s.sigma_next(n - 1) == 0.0
        assert torch.equal(s.sigmas, torch.from_numpy(tab))
        # the timestep -> sigma lookup scale_noise uses
        for i in (0, n // 2, n - 1):
            assert s.index_for_timestep(s.timesteps[i]) == i


def _via_pack_latents(mask):
    """The mask a torch implementation would use: repeated over the 16 channels and packed like the latents."""
    B, _, h, w = mask.shape
    return helpers._pack_latents(mask.repeat(1, 16, 1, 1).contiguous(), B, 16, h, w)


def test_compact_mask_is_pack_latents_indexed_by_sub_pixel():
    g = torch.Generator().manual_seed(3)
    rnd = (torch.rand(2, 1, 6, 10, generator=g) < 0.5).float()
    edge = torch.zeros(2, 1, 6, 10)
    edge[:, :, :, :3] = 1                       # the edge sits on odd latent column 3: tokens of column pair (2, 3) are mixed
    edge[1, :, :3] = 0                          # and, in sample 1, on odd row 3
    edge[1, :, 3:, :] = 1
    for mask in (rnd, edge, torch.zeros(1, 1, 6, 10), torch.ones(1, 1, 6, 10)):
        compact = ops.pack_inpaint_mask(mask, 6, 10)
        full = _via_pack_latents(mask)
        assert compact.shape == (mask.shape[0], 15, 4) and compact.dtype == BF and compact.is_contiguous()
        assert full.shape == (mask.shape[0], 15, 64)
        for j in range(64):
            assert torch.equal(full[:, :, j], compact[:, :, j % 4].float()), j
        assert torch.equal(R.expand_mask(compact, 64).float(), full)
    compact = ops.pack_inpaint_mask(edge, 6, 10)
    per_token = compact.float().sum(-1)
    assert ((per_token > 0) & (per_token < 4)).any(), "no token carries mixed sub-pixels: the case tests nothing"
    assert compact[0, 1].tolist() == [1.0, 0.0, 1.0, 0.0]          # token (0, 1): columns 2 (repaint) and 3 (keep)


def test_mask_nearest_resize_and_binarisation_at_one_half():
    g = torch.Generator().manual_seed(4)
    px = torch.rand(1, 1, 48, 80, generator=g)
    px[0, 0, 0, 0], px[0, 0, 0, 8], px[0, 0, 8, 0] = 0.5, 0.49999, 0.50001
    compact = ops.pack_inpaint_mask(px, 6, 10)
    # nearest: latent (y, x) reads pixel (floor(y * 48 / 6), floor(x * 80 / 10)) = (8 y, 8 x); >= 0.5 -> 1
    want = (px[:, :, ::8, ::8] >= 0.5).float()
    assert want[0, 0, 0, 0] == 1 and want[0, 0, 0, 1] == 0 and want[0, 0, 1, 0] == 1
    assert torch.equal(R.expand_mask(compact, 64).float(), _via_pack_latents(want))
    # a mask already at the latent size is only binarised; uint8-style values in [0, 1] after / 255
    lat = torch.tensor([127 / 255, 128 / 255, 0.0, 1.0]).view(1, 1, 2, 2)
    assert ops.pack_inpaint_mask(lat, 2, 2).view(-1).tolist() == [0.0, 1.0, 0.0, 1.0]
    with pytest.raises(ValueError):
        ops.pack_inpaint_mask(torch.zeros(1, 3, 8, 8), 2, 2)
    with pytest.raises(ValueError):
        ops.pack_inpaint_mask(torch.zeros(1, 1, 8, 8), 3, 2)


def test_bf16_step_formula_identities():
    """m = 1 is the Euler update, m = 0 is ``keep``, and sigma_next = 0 makes ``keep`` the preserved picture -- as values
    (``torch.equal``), for finite inputs.  This is the reference the GPU tests compare the HIP kernels with."""
    g = torch.Generator().manual_seed(5)
    x, v, x0, noise = (torch.randn(2, 24, 64, generator=g).mul(s).to(BF) for s in (1.0, 3.0, 2.0, 1.0))
    ones, zeros = torch.ones(1, 24, 64, dtype=BF), torch.zeros(1, 24, 64, dtype=BF)
    dsigma = -0.0371                          # not a bf16 number
    assert R.bf_scalar(dsigma).float().item() != np.float32(dsigma)
    for sn in (0.0, 0.7311, 1.0):
        assert torch.equal(R.step(x, v, dsigma, sn, x0, noise, ones), R.euler(x, v, dsigma))
        assert torch.equal(R.step(x, v, dsigma, sn, x0, noise, zeros), R.keep(x0, noise, sn))
    assert torch.equal(R.keep(x0, noise, 0.0), x0)
    assert torch.equal(R.keep(x0, noise, 1.0), noise)
    assert torch.equal(R.step(x, v, dsigma, 0.0, x0, noise, zeros), x0)
    # the Euler update is the scheduler step of the plain edit: bf16(x + bf16(bf16(dsigma) * v))
    want = (x.float() + (R.bf_scalar(dsigma).float() * v.float()).to(BF).float()).to(BF)
    assert torch.equal(R.euler(x, v, dsigma), want)
    # a mixed token takes each element from its own side
    m = R.expand_mask(torch.tensor([1.0, 0.0, 0.0, 1.0]).to(BF).view(1, 1, 4).expand(1, 24, 4), 64)
    out = R.step(x, v, dsigma, 0.7311, x0, noise, m)
    sel = m.expand(2, 24, 64) == 1
    assert torch.equal(out[sel], R.euler(x, v, dsigma)[sel]) and torch.equal(out[~sel], R.keep(x0, noise, 0.7311)[~sel])


def test_cli_mask_and_strength_reach_the_pipeline(tmp_path, monkeypatch):
    from PIL import Image
    from gpt_image_edit_amd.serve import cli
    base = ["--model_path", "m", "--flux_path", "f"]
    a = cli.build_parser().parse_args(base)
    assert a.mask is None and a.strength == 1.0 and cli.inpaint_kwargs(a) == {}          # the plain edit: nothing is passed
    arr = np.zeros((32, 48), dtype=np.uint8)
    arr[:, :24] = 255
    Image.fromarray(arr).convert("RGB").save(tmp_path / "mask.png")                        # any mode: read as greyscale
    a = cli.build_parser().parse_args(base + ["--mask", str(tmp_path / "mask.png"), "--strength", "0.6"])
    kw = cli.inpaint_kwargs(a)
    assert kw["strength"] == 0.6 and kw["mask_image"].mode == "L" and kw["mask_image"].size == (48, 32)
    assert np.array_equal(np.asarray(kw["mask_image"]), arr)
    seen = {}
    monkeypatch.setattr(cli.torch, "Generator", lambda device=None: type("G", (), {"manual_seed": lambda self, s: self})())

    class Pipe:
        device = "cpu"

        def __call__(self, **kwargs):
            seen.update(kwargs)
            return type("O", (), {"images": [None]})()
    cli.generate_image(Pipe(), torch.zeros(1, 4, 4096), torch.zeros(1, 768), [], 64, 64, a)
    assert seen["strength"] == 0.6 and seen["mask_image"].mode == "L"
    with pytest.raises(SystemExit, match="--mask / --strength"):
        cli.main(a)                                     # the chat route has no mask input
