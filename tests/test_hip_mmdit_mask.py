"""The MMDiT with ``joint_attention_kwargs["attention_mask"]``: a padded batch of samples of different sizes must compute, at
every sample's real tokens, what the sample computes alone and unpadded -- forward (against the fp32 / bf16 CPU oracle run per
sample), training gradients (against the sum of the per-sample HIP runs), the train step's loss, and the error paths.

Batch: B = 2, 32 text tokens, an 8 x 12 token grid (the batch maximum); sample 0 fills it, sample 1 is real in the top-left
6 x 8 corner, its padded latents zero.  Top-left padding keeps every real token's (row, col) id.  Full-width model, one double
and two single blocks (FLUX_KONTEXT_CONFIG with num_layers = 1, num_single_layers = 2), as tests/test_hip_mmdit.py builds them.

Measured on an MI355X: see RECORDED below.
"""
import pytest
import torch

from conftest import report

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, S_TXT, ROWS, COLS = 2, 32, 8, 12
VALID = ((8, 12), (6, 8))

# figures of one MI355X run (`pytest -s`): the forward test's distances and the gradient test's worst ratios
RECORDED = """
forward    masked batch vs per-sample fp32-oracle: max 4.768e-02, mean 9.552e-03; bf16-oracle vs fp32-oracle (the floor): max
           4.882e-02, mean 9.553e-03 -> 0.98 / 1.00 of the floor (bounds 1.25 / 1.1).  Control, sample 1 of the UNMASKED padded batch:
           max 2.524, mean 0.488 = 51.7 x / 49.6 x its floor.
gradients  masked batch vs sum of the per-sample runs over 32 tensors: worst max error 1.650e-02 of max|ref|
           (single_transformer_blocks.1.attn.to_k.weight; its mean 3.1e-04; bounds 2e-2 / 4e-3), typical 5e-03 .. 9e-03;
           UNMASKED padded batch: 1.775 of max|ref|.  Checkpointing on / off: same bits.
step       loss 3.17962746 vs the oracle's loss on the per-sample predictions 3.17975140: rel 3.9e-05 (bound 4e-4);
           without attention_mask 3.20477830 (7.9e-03 away).  The same comparison with the data seeded 5 .. 12: rel 3.9e-05,
           7.7e-05, 9.2e-05, 6.9e-06, 1.1e-05, 8.5e-07, 5.6e-05, 3.6e-05.  While the RoPE of q, k still held an fma (one product
           unrounded) the same eight gave 1.5e-07, 4.1e-05, 6.0e-06, 2.3e-05, 4.8e-06, 3.0e-05, 2.5e-05, 1.5e-05: the 1e-5 this
           test asked for then was met by the committed seed alone, not by the code.
"""

# test_train_step_takes_the_attention_mask: the padded batch and the per-sample runs are two bf16 executions of the same model,
# not the same sums (the attention visits sample 1's keys in other 64-key tiles, the GEMMs see other row counts): where a float32
# sum lands on the other side of a bf16 boundary the two part, and the following blocks spread it.  Two executions that were
# INDEPENDENT at the bf16 floor of the forward test above (mean 9.55e-3, rms 1.2e-2 against the exact prediction) would differ in
# the loss mean(e^2), rms(e) = sqrt(3.18), over N = 64 x (96 + 48) weighted entries by 2 x 1.2e-2 / (1.78 sqrt(N)) = 1.4e-4
# relative (one sigma); the bound is three of those.  A step that ignored the mask is 7.9e-3 away, twenty bounds.
STEP_LOSS_REL = 4e-4


def _grid_mask():
    m = torch.zeros(B, ROWS, COLS, dtype=torch.bool)
    for b, (r, c) in enumerate(VALID):
        m[b, :r, :c] = True
    return m.reshape(B, ROWS * COLS)


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import flux_spec
    from gpt_image_edit_amd.transformer import HipFluxTransformer2DModel
    from oracle.helpers import prepare_latent_image_ids
    cfg = dict(flux_spec.FLUX_KONTEXT_CONFIG, num_layers=1, num_single_layers=2)
    sd_bf = {k: v.to(BF) for k, v in flux_spec.synthetic_state(flux_spec.flux_param_shapes(cfg), seed=1).items()}
    model = HipFluxTransformer2DModel(cfg, device="cuda")
    model.load_state_dict(sd_bf)
    g = torch.Generator().manual_seed(0)
    mask = _grid_mask()
    hs = torch.randn(B, ROWS * COLS, cfg["in_channels"], generator=g).to(BF)
    hs[~mask] = 0                                                  # padded latents are zero
    enc = torch.randn(B, S_TXT, cfg["joint_attention_dim"], generator=g).to(BF)
    pooled = torch.randn(B, cfg["pooled_projection_dim"], generator=g).to(BF)
    t = torch.tensor([0.5, 0.25]).to(BF)                           # t * 1000 exact in bf16 (tests/test_hip_mmdit.py)
    gd = torch.full((B,), 4.0)
    img_ids = prepare_latent_image_ids(ROWS, COLS)
    txt_ids = torch.zeros(S_TXT, 3)
    return dict(cfg=cfg, sd_bf=sd_bf, model=model, mask=mask, hs=hs, enc=enc, pooled=pooled, t=t, gd=gd, img_ids=img_ids, txt_ids=txt_ids)


def _call(s, mask=None, sample=None, **over):
    """The model on the padded batch (``mask``: the attention mask or None) or on sample ``sample`` alone, unpadded."""
    hs, enc, pooled, t, gd, ids = s["hs"], s["enc"], s["pooled"], s["t"], s["gd"], s["img_ids"]
    if sample is not None:
        b, idx = sample, s["mask"][sample].nonzero()[:, 0]
        hs, enc, pooled, t, gd, ids = hs[b:b + 1, idx], enc[b:b + 1], pooled[b:b + 1], t[b:b + 1], gd[b:b + 1], ids[idx]
    kw = dict(hidden_states=hs.cuda(), timestep=t.cuda(), guidance=gd.cuda(), pooled_projections=pooled.cuda(),
              encoder_hidden_states=enc.cuda(), txt_ids=s["txt_ids"].cuda(), img_ids=ids.cuda(),
              joint_attention_kwargs={} if mask is None else {"attention_mask": mask}, return_dict=False)
    kw.update(over)
    return s["model"](**kw)[0]


def test_padded_batch_equals_the_per_sample_runs(setup):
    """Masked forward of the padded batch at each sample's real tokens against the fp32 oracle run PER SAMPLE, unpadded, on the
    gathered tokens and ids, in the form of tests/test_hip_mmdit.py::test_mmdit_forward_matches_oracle: HIP - fp32-oracle max
    <= 1.25 x (bf16-oracle - fp32-oracle max), mean <= 1.1 x that mean.  Control: the UNMASKED forward of the same padded batch
    must break that bound on sample 1 (48 of its 128 keys are padding) -- otherwise the test would show nothing."""
    from oracle import mmdit
    s = setup
    with torch.no_grad():
        out = _call(s, s["mask"].cuda()).cpu()
        out_nomask = _call(s, None).cpu()
    assert out.shape == (B, ROWS * COLS, 64) and torch.isfinite(out.float()).all()
    sd_bf, cfg = s["sd_bf"], s["cfg"]
    sd_r = {k: v.float() for k, v in sd_bf.items()}
    got, got_nomask, ref_bf, ref32 = [], [], [], []
    for b in range(B):
        idx = s["mask"][b].nonzero()[:, 0]
        args = (s["hs"][b:b + 1, idx], s["enc"][b:b + 1], s["pooled"][b:b + 1])
        rest = (s["t"][b:b + 1], s["img_ids"][idx], s["txt_ids"], s["gd"][b:b + 1])
        ref_bf.append(mmdit.flux_forward(sd_bf, *args, *rest, config=cfg)[0])
        ref32.append(mmdit.flux_forward(sd_r, *(a.float() for a in args), *rest, config=cfg)[0])
        got.append(out[b, idx])
        got_nomask.append(out_nomask[b, idx])
    cat = lambda xs: torch.cat([x.float() for x in xs])      # noqa: E731
    d_32 = report("masked padded batch vs per-sample fp32-oracle", cat(got), cat(ref32))
    d_bf = report("masked padded batch vs per-sample bf16-oracle", cat(got), cat(ref_bf))
    d_ref = report("per-sample bf16-oracle vs fp32-oracle (round-off floor)", cat(ref_bf), cat(ref32))
    assert d_32.max().item() <= 1.25 * d_ref.max().item()
    assert d_32.mean().item() <= 1.1 * d_ref.mean().item()
    # control, sample 1 alone
    c_32 = report("UNMASKED padded batch, sample 1 vs fp32-oracle", got_nomask[1], ref32[1])
    f_1 = report("sample 1 bf16-oracle vs fp32-oracle", ref_bf[1], ref32[1])
    assert c_32.max().item() > 1.25 * f_1.max().item() and c_32.mean().item() > 1.1 * f_1.mean().item(), \
        "the unmasked forward passes the bound: the padding does not matter at this latent scale and the test shows nothing"
    # sample 0 has no padding: its unmasked rows still differ from the masked call's only through the kernel, not the mask
    print(f"[mask] sample 1: unmasked / floor max {c_32.max().item() / f_1.max().item():.1f}, mean {c_32.mean().item() / f_1.mean().item():.1f}", flush=True)


def _close_bf16(name, got, ref, tol=2e-2):
    """tests/test_hip_backward.py::close_bf16, the bound it holds the attention backward to against autograd: max error <= tol x
    max |ref| (+ 1e-6), mean <= 0.2 tol x max |ref| (+ 1e-7); tol = 2e-2 there and here."""
    d = (got.float() - ref.float()).abs()
    scale = ref.float().abs().max().item()
    print(f"[grad] {name:55s} max {d.max().item() / max(scale, 1e-30):.3e} mean {d.mean().item() / max(scale, 1e-30):.3e} of max|ref| "
          f"(bounds {tol:.0e} / {0.2 * tol:.0e})", flush=True)
    assert torch.isfinite(got.float()).all()
    assert d.max().item() <= tol * scale + 1e-6, f"{name}: {d.max().item():.3e} vs scale {scale:.3e}"
    assert d.mean().item() <= 0.2 * tol * scale + 1e-7, name
    return d.max().item() / max(scale, 1e-30)


def test_training_gradients_equal_the_sum_of_the_per_sample_runs(setup):
    """loss = sum over the real tokens of w * sample, `only_tune_image_branch` parameter selection, loss.backward(): the
    gradients of the masked padded batch against the SUM of the two per-sample unpadded HIP runs' gradients (fp32 sum of their
    bf16 gradients), at the bound tests/test_hip_backward.py holds HIP gradients to against autograd (close_bf16, tol 2e-2).
    Padding tokens carry no loss weight and are no keys, so no gradient reaches or leaves them.  Gradient checkpointing on / off
    (recompute / stored-activation policy) gives the same bits."""
    from gpt_image_edit_amd import training
    s = setup
    model = s["model"]
    trainable = training.trainable_names(list(s["sd_bf"].keys()))
    assert trainable
    model.requires_grad_(False)
    for k in trainable:
        model.p(k).requires_grad_(True)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(B, ROWS * COLS, 64, generator=g)
    w[~s["mask"]] = 0
    w = w.cuda()

    def grads_of(run):
        for k in trainable:
            model.p(k).grad = None
        run()
        torch.cuda.synchronize()
        return {k: model.p(k).grad.detach().clone() for k in trainable}

    def batch_run():
        with torch.enable_grad():
            (_call(s, s["mask"].cuda()).float() * w).sum().backward()

    try:
        model.enable_gradient_checkpointing()
        g_ckpt = grads_of(batch_run)
        model.disable_gradient_checkpointing()
        g_store = grads_of(batch_run)
        for k in trainable:
            assert torch.equal(g_ckpt[k], g_store[k]), f"{k}: recompute and stored-activation policies differ"
        per = {k: torch.zeros_like(g_store[k], dtype=torch.float32) for k in trainable}
        for b in range(B):
            one = grads_of(lambda b=b: _one(s, b, w))
            for k in trainable:
                per[k] += one[k].float()
        worst = max(_close_bf16(k, g_store[k], per[k]) for k in trainable)
        print(f"[grad] masked padded batch vs sum of per-sample runs: worst max error {worst:.3e} of max|ref| over {len(trainable)} tensors", flush=True)
        # and the mask matters: without it the padded batch's gradients leave the bound somewhere
        def nomask_run():
            with torch.enable_grad():
                (_call(s, None).float() * w).sum().backward()
        g_no = grads_of(nomask_run)
        far = max(((g_no[k].float() - per[k]).abs().max() / per[k].abs().max().clamp_min(1e-30)).item() for k in trainable)
        print(f"[grad] UNMASKED padded batch vs sum of per-sample runs: worst max error {far:.3e} of max|ref|", flush=True)
        assert far > 2e-2, "the unmasked batch passes too: the test shows nothing"
    finally:
        model.disable_gradient_checkpointing()
        model.requires_grad_(False)
        for k in trainable:
            model.p(k).grad = None


def _one(s, b, w):
    idx = s["mask"][b].nonzero()[:, 0].cuda()
    with torch.enable_grad():
        (_call(s, None, sample=b).float() * w[b:b + 1, idx]).sum().backward()


def test_train_step_takes_the_attention_mask(setup):
    """DenoiserTrainStep.forward_backward(..., weight_mask=, attention_mask=) on the padded batch (latents 16 x 24, sample 1
    real in 12 x 16; model_input and noise zero on the padding): the loss equals oracle.train.flow_matching_loss with
    weight_mask on the PER-SAMPLE predictions -- each sample's prediction computed alone and unpadded by the HIP model, scattered
    into the padded layout (the padding's entries do not count: weight 0) -- to STEP_LOSS_REL, what two bf16 executions of the
    model can differ by (derived above; the rel 1e-5 of tests/test_hip_train_step.py::test_step_takes_the_stage2_loss_weights
    belongs to one set of predictions through two loss codes, which this is not).  Without attention_mask the same call gives
    another loss, at least five bounds away: weight_mask alone stays loss-only."""
    from gpt_image_edit_amd.train_step import DenoiserTrainStep
    from oracle import helpers, train as otrain
    s = setup
    model = s["model"]
    h, w = 2 * ROWS, 2 * COLS
    g = torch.Generator().manual_seed(5)
    wm = torch.zeros(B, 1, h, w)
    for b, (r, c) in enumerate(VALID):
        wm[b, :, :2 * r, :2 * c] = 1.0
    x = torch.randn(B, 16, h, w, generator=g) * wm
    noise = torch.randn(B, 16, h, w, generator=g) * wm
    sigmas = torch.tensor([0.25, 0.75])
    ts = DenoiserTrainStep(model)
    common = dict(prompt_embeds=s["enc"].cuda(), pooled=s["pooled"].cuda())
    loss, grads, _ = ts.forward_backward(x.cuda(), None, noise.cuda(), sigmas.cuda(), weight_mask=wm.cuda(),
                                         attention_mask=s["mask"].cuda(), **common)
    loss_nomask, _, _ = ts.forward_backward(x.cuda(), None, noise.cuda(), sigmas.cuda(), weight_mask=wm.cuda(), **common)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and all(torch.isfinite(v.float()).all() for v in grads.values())
    # per-sample predictions: the sample's real latent window alone through the same step's forward
    pred = torch.zeros(B, ROWS * COLS, 64)
    for b, (r, c) in enumerate(VALID):
        xb, nb = x[b:b + 1, :, :2 * r, :2 * c].contiguous(), noise[b:b + 1, :, :2 * r, :2 * c].contiguous()
        inp, S_tgt = ts.prepare_inputs(xb.cuda(), None, nb.cuda(), sigmas[b:b + 1].cuda(), s["enc"][b:b + 1].cuda(), s["pooled"][b:b + 1].cuda())
        pb = ts.bw.forward(inp["hidden_states"], inp["encoder_hidden_states"], inp["pooled_projections"], inp["timestep"],
                           inp["img_ids"], inp["txt_ids"], inp["guidance"])[:, :S_tgt].float().cpu()
        pred[b, s["mask"][b]] = pb[0]
    ref = otrain.flow_matching_loss(helpers.unpack_latents(pred, h * 8, w * 8), x, noise, wm.float(), weight_mask=wm)
    print(f"[step] loss masked {float(loss):.8f}  oracle loss on per-sample predictions {float(ref):.8f}  rel "
          f"{abs(float(loss) - float(ref)) / float(ref):.2e} (bound {STEP_LOSS_REL:.0e});  without attention_mask {float(loss_nomask):.8f}",
          flush=True)
    assert float(loss) == pytest.approx(float(ref), rel=STEP_LOSS_REL)
    assert abs(float(loss_nomask) - float(ref)) > 5 * STEP_LOSS_REL * float(ref), "the unmasked step gives the same loss: the test shows nothing"


def test_error_paths_and_the_pooled_mask_shape(setup):
    s = setup
    model = s["model"]
    m = s["mask"].cuda()
    with torch.no_grad():
        base = _call(s, m)
        pooled_form = _call(s, m[:, None, :].expand(B, 16, -1).to(torch.float32))      # max_pool2d(...).flatten(-2): [B, 16, S_img] of 0 / 1
        assert torch.equal(base, pooled_form)
        one_channel = torch.zeros(B, 16, ROWS * COLS, device="cuda")
        one_channel[:, 3] = m.float()                                                # reduced over C with any()
        assert torch.equal(base, _call(s, one_channel))
        for bad in (m[:, :-1], m[:1], m[:, None, None, :], m.reshape(-1)):
            with pytest.raises(ValueError, match="attention_mask"):
                _call(s, bad)
        with pytest.raises(ValueError, match="S_txt"):
            _call(s, m, encoder_hidden_states=s["enc"][:, :0].cuda(), txt_ids=s["txt_ids"][:0].cuda())
        model.set_weight_format("mxfp8")
        try:
            with pytest.raises(ValueError, match="mxfp8"):
                _call(s, m)
        finally:
            model.set_weight_format("bf16")
        assert torch.equal(base, _call(s, m))
