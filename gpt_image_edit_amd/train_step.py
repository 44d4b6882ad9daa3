"""One optimisation step of the denoiser on the HIP path (BASELINE.json configs[4]).

Counterpart of the body of the reference's training loop, ``train_denoiser.py:935-1181``, for the shipped FLUX-Kontext
configuration (continuous timesteps, unit loss weights, guidance 1.0, AdamW, global-norm clipping at 1.0,
``only_tune_image_branch``): noisy input mixed and packed (``fk_flow_noisy_tokens_bf16``), MMDiT forward with one
checkpoint per block and backward (``backward.FluxBackward``), flow-matching loss fused with its gradient
(``fk_flow_loss_bf16``), squared gradient norm (``fk_sumsq``) and AdamW with the clipping coefficient folded in and the
bf16 parameter copy written in the same pass (``fk_adamw_step``).  The step's scalars (which parameters train, sigma
sampling, shift) are ``training.py``; the optimiser pass and the unsharded state are ``optim.py``; the data-parallel exchange
is ``zero.py``.  No torch arithmetic touches an
activation, gradient or parameter.

With ``projector=`` the ``denoise_projector`` trains along (it is in the reference's trainable set,
``train_denoiser.py:71-119``): ``vlm_hidden`` -- the frozen VLM's last hidden states -- goes through
``HipDenoiseProjector.forward_train``, the optional T5 ``prefix_prompt_embeds`` are appended as the reference's
``UnivaDenoiseTower.forward`` does (``modeling_univa_denoise_tower.py:62-70``), and the gradient of ``prompt_embeds``
that the MMDiT backward returns is carried through both Linears.  Its parameters appear as ``denoise_projector.*``.
For padded multi-resolution batches the reference pads every latent to the batch's maximum size, max-pools the ones /
zeros map to token resolution and passes it as ``joint_attention_kwargs['attention_mask']`` (``train_denoiser.py:907-916``);
``UnivaDenoiseTower.forward`` then pops it without passing it on (``modeling_univa_denoise_tower.py:77``; the code that would
have joined it with the text mask is commented out, ``:77-99``), so in the reference no mask ever reaches the attention and
the padding tokens act as keys of every real token -- a bug, not a specification.  Here ``forward_backward(...,
attention_mask=...)`` hands the mask to the attention kernels as a key-padding mask (text keys always valid, broadcast over
heads and queries; ``HipFluxTransformer2DModel.forward`` has the forms).  Without ``attention_mask``, ``weight_mask`` weighs
the loss only and the attention runs unmasked, as before.

With ``lora=adapter_name`` the step trains a LoRA adapter's factors instead of the weights (``lora.py``, "Training"): the same
forward and backward on the merged weights, each target weight's ``dW`` projected onto ``up`` / ``down`` as its block emits it
(``fk_lora_grad_bf16``), AdamW on fp32 masters of the factors, then one re-merge per touched weight from its saved base.  The
optimiser state is 12 bytes per ADAPTER parameter and only one block's ``dW`` is alive at a time.  With ``data_parallel=True`` as well
the factors live in a ``zero.ShardedAdamW``: every ``dW`` is projected straight into the optimiser's fp32 gradient views
(``fk_lora_grad_acc_bf16``, which can add to what is there), so the adapter has micro-batch accumulation and the data-parallel exchange.
With ``lora_backward="factored"`` the adapter gradient of every linear whose backward operands survive (``FluxBackward.SIDE_LEAVES``)
is taken from those operands, ``d_up = s dY^T (X down^T)``, ``d_down = s (dY up)^T X`` (``fk_lora_side_grad_bf16``): its wgrad GEMM and
its ``dW`` do not exist, and the gradient does not pass through ``dW``'s bf16 rounding.  The other targets stay projected.

With ``optimizer="prodigy"`` the optimiser pass is Prodigy instead of AdamW (the reference's ``optimizer: 'prodigy'``,
``train_denoiser.py:603-624``; ``csrc/prodigy.hip``): ``fk_sumsq``, ``fk_prodigy_begin``, ``fk_prodigy_moments`` over the sorted names,
``fk_prodigy_update_d``, ``fk_prodigy_apply`` over the same names.  The step size ``d`` and every other scalar stay on the device;
the state per tensor is ``(master, m, v, s, p0)``.  The same code serves ``lora=`` and ``sharded=True``.
"""
import torch

from . import helpers, ops
from .backward import FluxBackward
from .optim import PerTensorState
from .zero import DEFAULT_BUCKET, ShardedAdamW, backward_order

BF16 = torch.bfloat16


class DenoiserTrainStep:
    def __init__(self, model, lr=None, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, trainable=None,
                 sharded=False, group=None, store_activations="auto", projector=None, keep_grads=True, bucket_numel=None,
                 lora=None, optimizer="adamw", prodigy=None, data_parallel=False, lora_backward="projected"):
        """sharded=True: the optimiser state lives in ``zero.ShardedAdamW`` (ZeRO-2: one flat bf16 parameter buffer the
        model's trainable tensors become views of, fp32 gradients reduce-scattered over the data-parallel ranks, this
        rank's slice of master + moments updated, parameters all-gathered); works unchanged with one process.
        keep_grads=False (sharded only): ``forward_backward`` hands every block's gradients to the optimiser's buckets and
        does not keep them (saves the 8 GB of bf16 gradients; ``step()['grads']`` is then empty).
        lora=adapter_name: train that adapter's factors instead of the weights (``lora.py``; created by ``add_lora_adapter`` or
        loaded from a file -- the same code).  The forward and backward are launch for launch the ones above on the merged
        weights, with only the adapter's target weights in the wgrad set; each block's ``dW`` is projected onto the factors as it is
        emitted (``fk_lora_grad_bf16``) and dropped.  The trainable parameters are ``<module>.lora_A.weight`` (down) and
        ``<module>.lora_B.weight`` (up); other active adapters stay merged and frozen.  Not with ``sharded=True``.
        data_parallel=True (with ``lora=``; ``group=`` / ``bucket_numel=`` as for ``sharded``): the factors (and any ``projector=``
        parameters) become views of the flat bf16 buffer of a ``zero.ShardedAdamW`` in ``backward_order``; every ``dW`` is projected
        STRAIGHT into the optimiser's fp32 gradient views (``fk_lora_grad_acc_bf16``: overwritten by the first micro-batch, added
        to by later ones on one rank; staged and reduce-scattered with more ranks), so a second ``forward_backward`` before
        ``optimizer_step`` is a further micro-batch and the step uses the mean over micro-batches and ranks.  All ranks must start
        from the same factors (checked once, collectively).  Works unchanged with one process.
        optimizer="adamw" | "prodigy" (the reference's ``optimizer`` key, train_denoiser.py:595-624): Prodigy estimates its step
        size ``d`` on the fly (``csrc/prodigy.hip``; two more fp32 state tensors, ``s`` and the initial point ``p0``);
        ``prodigy=dict(beta3=, d0=, d_coef=, growth_rate=, use_bias_correction=, safeguard_warmup=, decouple=)`` overrides its
        defaults (the reference config's: the three flags True).  ``lr=None`` is 1e-6 for AdamW and 1.0 for Prodigy; Prodigy
        with ``lr <= 0.1`` is refused as the reference refuses it (:609-612).
        lora_backward="projected" | "factored" (with ``lora=``): "projected" is the step above, launch for launch.  "factored": every
        target of the adapter that ``FluxBackward.side_routable`` leaves the wgrad set; the backward hands its two operand views to a
        side sink that asks the optimiser for the same two fp32 targets as the projection does (``grad_target``, then ``written``)
        and makes one ``ops.lora_side_grad`` call -- so ``data_parallel=True``, ``optimizer="prodigy"``, ``projector=``, frozen
        second adapters, ``discard()`` and save / resume work as before.  The optimiser state is the same in both modes and
        ``state_dict()`` does not record the mode: a state saved in one loads in the other."""
        if lora_backward not in ("projected", "factored"):
            raise ValueError(f"DenoiserTrainStep: lora_backward={lora_backward!r}, it is \"projected\" or \"factored\"")
        if lora_backward == "factored" and lora is None:
            raise ValueError("DenoiserTrainStep: lora_backward=\"factored\" is the adapter's backward and needs lora=")
        self.lora_backward = lora_backward
        # the unsharded optimiser (its refusals come before the model is touched); unused once `opt` below is set
        self.local = PerTensorState(self._param, optimizer, lr, betas, eps, weight_decay, max_grad_norm, prodigy)
        self.optimizer, self.lr, self.prodigy = self.local.optimizer, self.local.hp["lr"], self.local.prodigy
        self.model = model
        self.projector = projector
        self.lora = lora
        self.data_parallel = bool(data_parallel)
        if data_parallel and lora is None:
            raise ValueError("DenoiserTrainStep: data_parallel=True is the adapter's gradient accumulation / data-parallel mode and "
                             "needs lora=; the full-weight step has both with sharded=True")
        if lora is not None:
            if sharded:
                raise ValueError("DenoiserTrainStep: lora= with sharded=True is not built (sharded=True lays out the full weights); "
                                 "data_parallel=True gives an adapter gradient accumulation and the data-parallel exchange")
            if trainable is not None:
                raise ValueError("DenoiserTrainStep: lora= trains the adapter's factors; trainable= selects full weights")
            if lora not in model._lora_adapters or lora not in model._lora_active:
                raise ValueError(f"DenoiserTrainStep: adapter {lora!r} is not loaded and active (add_lora_adapter / "
                                 "load_lora_adapter / set_adapters before the train step is built)")
            model.set_lora_scale(1.0)          # the scale of the projection is the one the weights were merged with
            self._lora_entries = model._lora_adapters[lora]
            self._lora_ws = None
            self._side_ws = None
        side = None
        if lora_backward == "factored":
            side = {k for k in self._lora_entries if FluxBackward.side_routable(k)}
        self.bw = FluxBackward(model, trainable, store_activations=store_activations, lora=lora, side=side)
        self.betas, self.eps, self.weight_decay, self.max_grad_norm = betas, eps, weight_decay, max_grad_norm
        self.opt = None     # the zero.ShardedAdamW of sharded=True / data_parallel=True
        self.keep_grads = keep_grads
        self._sunk = {}     # name -> (data_ptr, version) of the gradients already handed to the sharded optimiser
        if sharded or data_parallel:
            self.opt = self._flat_optimizer(group, bucket_numel)
        if sharded:
            model._packed = None
        if data_parallel:        # ONE all-reduce: all ranks raise together or none does
            self.opt.check_ranks_agree(f"DenoiserTrainStep(lora={self.lora!r}, data_parallel=True): create or load the adapter "
                                       "identically on every rank, e.g. the same add_lora_adapter(seed=)")

    # the optimiser's own state, under the names it had when it was kept here
    state = property(lambda self: self.local.state)              # name -> (fp32 master, exp_avg, exp_avg_sq) (+ s, p0: Prodigy)
    pstate = property(lambda self: self.local.pstate)
    _optim = property(lambda self: self.opt or self.local)       # the optimiser in use: both have the same calls
    step_count = property(lambda self: self._optim.step_count)

    def _flat_optimizer(self, group, bucket_numel):
        """The ``ShardedAdamW`` of ``sharded=True`` and ``data_parallel=True``: every trainable tensor (with ``lora=``: ``e.up`` /
        ``e.down``, so the merge and ``lora_state_dict`` read the trained values with no copy) becomes a view of its flat bf16 buffer.
        Buckets in the order the backward pass finishes the gradients: a bucket's reduce-scatter is issued the moment its last block
        is done and runs under the backward of the earlier blocks (zero2.json: overlap_comm)."""
        names = sorted(self.trainable_names())
        opt = ShardedAdamW({k: self._param(k).data for k in names}, lr=self.lr, betas=self.betas, eps=self.eps,
                           weight_decay=self.weight_decay, max_grad_norm=self.max_grad_norm, group=group,
                           order=backward_order(names), bucket_numel=bucket_numel or DEFAULT_BUCKET,
                           **({} if self.optimizer == "adamw" else dict(optimizer=self.optimizer, prodigy=self.prodigy)))
        for k in names:          # the forward now reads views of the flat buffer
            if self.lora is not None and not k.startswith(self.PROJ):
                setattr(*self._factor(k), opt.params[k])
            else:
                self._param(k).data = opt.params[k]
        return opt

    PROJ = "denoise_projector."

    LORA_A, LORA_B = ".lora_A.weight", ".lora_B.weight"

    def _factor(self, name):
        """(adapter entry, "up" | "down") of the factor ``name``."""
        for sfx, slot in ((self.LORA_A, "down"), (self.LORA_B, "up")):
            if name.endswith(sfx):
                return self._lora_entries[name[:-len(sfx)] + ".weight"], slot
        raise KeyError(f"{name} is no factor of adapter {self.lora!r}")

    def _factor_names(self, pname):
        """(name of up, name of down) for the target weight ``pname``: the inverse of ``_factor``."""
        return pname[:-len(".weight")] + self.LORA_B, pname[:-len(".weight")] + self.LORA_A

    def trainable_names(self):
        if self.lora is not None:
            names = {n for k in self._lora_entries for n in self._factor_names(k)}
        else:
            names = set(self.bw.trainable)
        if self.projector is not None:
            names |= {self.PROJ + k for k in self.projector.state_dict()}
        return names

    def _param(self, name):
        if name.startswith(self.PROJ):
            return self.projector.p(name[len(self.PROJ):])
        if self.lora is not None:
            return getattr(*self._factor(name))
        return self.model.p(name)

    def _lora_sink(self, out):
        """The sink of ``FluxBackward.backward`` under ``lora=``: every emitted ``dW`` of a target weight is projected onto its two
        factors (one ``fk_lora_grad_bf16`` / ``fk_lora_grad_acc_bf16`` call) into the optimiser's two fp32 targets -- persistent buffers
        of ``PerTensorState``, the gradient views of ``ShardedAdamW`` (no buffer of this step's, no copy); ``out`` collects them by name."""
        scales = self._lora_scales()
        if self._lora_ws is None:
            dev = self.model.device
            need = max(ops.lora_grad_ws(e.up.shape[0], e.down.shape[1], e.rank, dev).numel() for e in self._lora_entries.values())
            self._lora_ws = torch.empty(need, device=dev, dtype=torch.float32)
        optim = self._optim

        def sink(block_grads):
            for pname, dw in block_grads.items():
                e = self._lora_entries.get(pname)
                if e is None:                  # the rest of a q / k / v group, a bias: not this adapter's
                    continue
                up, down = self._factor_names(pname)
                (d_up, acc), (d_down, _) = optim.grad_target(up), optim.grad_target(down)
                ops.lora_grad(dw, e.up, e.down, scales[pname], d_up=d_up, d_down=d_down, ws=self._lora_ws, accumulate=acc)
                optim.written([up, down])
                out[up], out[down] = d_up, d_down
        return sink

    def _lora_scales(self):
        """target weight -> the scale the trained adapter was merged with."""
        return {p: next(s for a, s, _ in ts if a == self.lora) for p, ts in self.model._lora_wanted().items()
                if any(a == self.lora for a, _, _ in ts)}

    def _lora_side_sink(self, out):
        """The side sink of ``FluxBackward.backward`` under ``lora_backward="factored"``: the two operand views of a side target's
        linear go through one ``fk_lora_side_grad_bf16`` call into the optimiser's two fp32 targets, by the protocol of
        ``_lora_sink`` (``grad_target``, then ``written``).  One workspace, grown to the largest (rows, target) seen."""
        scales = self._lora_scales()
        optim = self._optim

        def side_sink(pname, dy, x):
            e = self._lora_entries[pname]
            B, R = (1, dy.shape[0]) if dy.dim() == 2 else dy.shape[:2]
            need = ops.lora_side_grad_ws_floats(B, R, e.up.shape[0], e.down.shape[1], e.rank)
            if self._side_ws is None or self._side_ws.numel() < need:
                big = max(ops.lora_side_grad_ws_floats(B, R, f.up.shape[0], f.down.shape[1], f.rank)
                          for k, f in self._lora_entries.items() if k in self.bw.side)
                self._side_ws = torch.empty(max(big, need), device=self.model.device, dtype=torch.float32)
            up, down = self._factor_names(pname)
            (d_up, acc), (d_down, _) = optim.grad_target(up), optim.grad_target(down)
            ops.lora_side_grad(x, dy, e.up, e.down, scales[pname], d_up=d_up, d_down=d_down, ws=self._side_ws, accumulate=acc)
            optim.written([up, down])
            out[up], out[down] = d_up, d_down
        return side_sink

    @torch.no_grad()
    def prepare_inputs(self, model_input, cond_latents, noise, sigmas, prompt_embeds, pooled, guidance_scale=1.0):
        """The denoiser's keyword arguments for one batch, as the reference assembles them (``train_denoiser.py:996-1059,
        1064-1104``): noisy target tokens (mix + 2x2 packing in ONE kernel) followed by the condition tokens, ids with the
        condition's first coordinate set to 1, zero ``txt_ids``, ``timesteps / 1000`` in bf16, the guidance vector.
        Returns (kwargs of ``HipFluxTransformer2DModel.forward``, number of target tokens)."""
        dev = self.model.device
        B, C, h, w = model_input.shape
        S_tgt = (h // 2) * (w // 2)
        S_cond = 0 if cond_latents is None else (cond_latents.shape[2] // 2) * (cond_latents.shape[3] // 2)
        tokens = torch.empty(B, S_tgt + S_cond, 4 * C, device=dev, dtype=BF16)
        ops.flow_noisy_tokens(model_input.contiguous(), noise.contiguous(), sigmas.contiguous(), out=tokens[:, :S_tgt])
        ids = helpers._prepare_latent_image_ids(B, h // 2, w // 2, dev, BF16)
        if cond_latents is not None:
            ch, cw = cond_latents.shape[2], cond_latents.shape[3]
            tokens[:, S_tgt:].copy_(helpers._pack_latents(cond_latents.to(BF16), B, C, ch, cw))
            cids = helpers._prepare_latent_image_ids(B, ch // 2, cw // 2, dev, BF16)
            cids[..., 0] = 1
            ids = torch.cat([ids, cids], dim=0)
        txt_ids = torch.zeros(prompt_embeds.shape[1], 3, device=dev, dtype=BF16)
        guidance = torch.full([B], guidance_scale, device=dev, dtype=torch.float32)
        timestep = (sigmas * 1000.0).to(BF16) / 1000            # `timesteps / 1000` as the model receives it (:1073)
        return dict(hidden_states=tokens, encoder_hidden_states=prompt_embeds, pooled_projections=pooled, timestep=timestep,
                    img_ids=ids, txt_ids=txt_ids, guidance=guidance), S_tgt

    @staticmethod
    def _latent_map(m, B, h, w, dev):
        """A per-pixel weight map as the loss kernel reads it: fp32 [B, 1, h, w] on the device, nearest-resized to the latent
        size when it comes at another resolution (``F.interpolate(..., mode='nearest')``, train_denoiser.py:1131-1148)."""
        if m is None:
            return None
        m = m.to(device=dev, dtype=torch.float32)
        if m.dim() != 4 or m.shape[0] != B or m.shape[1] != 1:
            raise ValueError("area_mask_weights / weight_mask must be [B, 1, H, W]")
        if tuple(m.shape[-2:]) != (h, w):
            m = torch.nn.functional.interpolate(m, size=(h, w), mode="nearest")
        return m.contiguous()

    @torch.no_grad()
    def forward_backward(self, model_input, cond_latents, noise, sigmas, prompt_embeds=None, pooled=None, guidance_scale=1.0,
                         vlm_hidden=None, prefix_prompt_embeds=None, weighting=None, area_mask_weights=None, weight_mask=None,
                         attention_mask=None):
        """(loss fp64 [1], grads, d_prompt_embeds) for one batch of equally sized samples; model_input / noise fp32
        [B,16,h,w] (VAE latents already shifted and scaled), cond_latents the same or None, sigmas fp32 [B].
        Either ``prompt_embeds`` (projector frozen / absent) or ``vlm_hidden`` [B,L,3584] (+ optional T5 prefix).
        The loss as the stage-2 config sets it up (``mask_weight_type: 'log'``; train_denoiser.py:1106-1166): ``weighting``
        fp32 [B] (``compute_loss_weighting_for_sd3`` / ``sigmas_as_weight``; None = ones), ``area_mask_weights`` [B,1,H,W]
        (the dataset's per-pixel area weights; ``edit_weights.edit_region_weights`` makes them on the device from the reference
        and target bytes), ``weight_mask`` [B,1,H,W] (1 inside a padded sample's true extent; with it
        the sum is divided by ``weight_mask.sum() * C`` instead of the element count).  ``attention_mask``: bool / 0-1
        [B, S_img] or [B, C, S_img] over the image tokens (target tokens, then condition tokens), non-zero = a real token
        -- the attention then runs under that key mask; None: unmasked."""
        n_proj = 0
        if vlm_hidden is not None:
            if self.projector is None or prompt_embeds is not None:
                raise ValueError("vlm_hidden needs projector= at construction and excludes prompt_embeds")
            prompt_embeds = self.projector.forward_train(vlm_hidden)
            n_proj = prompt_embeds.shape[1]
            if prefix_prompt_embeds is not None:
                prompt_embeds = torch.cat([prompt_embeds, prefix_prompt_embeds.to(BF16)], dim=1)
        elif prompt_embeds is None:
            raise ValueError("one of prompt_embeds / vlm_hidden is required")
        inp, S_tgt = self.prepare_inputs(model_input, cond_latents, noise, sigmas, prompt_embeds, pooled, guidance_scale)
        key_mask = None
        if attention_mask is not None:
            key_mask = self.model._joint_key_mask(attention_mask, inp["hidden_states"], inp["encoder_hidden_states"])
        pred = self.bw.forward(inp["hidden_states"], inp["encoder_hidden_states"], inp["pooled_projections"], inp["timestep"],
                               inp["img_ids"], inp["txt_ids"], inp["guidance"], key_mask=key_mask)
        B, _, h, w = model_input.shape
        dev = pred.device
        if weighting is not None:
            weighting = weighting.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        loss, grad = ops.flow_loss(pred[:, :S_tgt], model_input.contiguous(), noise.contiguous(), weight=weighting,
                                   area_mask_weights=self._latent_map(area_mask_weights, B, h, w, dev),
                                   weight_mask=self._latent_map(weight_mask, B, h, w, dev))
        dsample = torch.zeros_like(pred)
        dsample[:, :S_tgt].copy_(grad)
        sink = None
        if self.opt is not None:
            # a second forward_backward before optimizer_step is a further micro-batch of the same step (the reference's
            # gradient_accumulation_steps): its gradients are ADDED to the optimiser's chunks, the step uses their mean
            self.opt.begin_micro_batch()

            def sink(block_grads):
                self.opt.accumulate(block_grads)
                for k, g in block_grads.items():
                    self._sunk[k] = (g.data_ptr(), g._version)
        if self.lora is not None:
            lora_grads = {}
            side_sink = self._lora_side_sink(lora_grads) if self.bw.side else None
            _, d_enc = self.bw.backward(dsample, sink=self._lora_sink(lora_grads), keep=False, side_sink=side_sink)
            missing = sorted(k for k in self.trainable_names() if not k.startswith(self.PROJ) and k not in lora_grads)
            if missing:
                raise RuntimeError("the backward emitted no weight gradient for " + ", ".join(missing[:4]))
            # data_parallel: the live running sums on one rank (valid until optimizer_step); staged gradients are not kept
            grads = lora_grads if self.opt is None or self.opt.direct else {}
        else:
            grads, d_enc = self.bw.backward(dsample, sink=sink, keep=self.keep_grads or self.opt is None)
        if n_proj:
            pg = {self.PROJ + k: g for k, g in self.projector.backward(d_enc[:, :n_proj]).items()}
            if sink is not None:
                sink(pg)
            if (self.keep_grads and not self.data_parallel) or self.opt is None:
                grads.update(pg)
        return loss, grads, d_enc

    @torch.no_grad()
    def optimizer_step(self, grads):
        """Global-norm clipping + the optimiser pass on fp32 masters (``optim.optimizer_pass``); the bf16 parameters of the model
        are rewritten in the same pass.  Returns the squared gradient norm."""
        # whatever forward_backward has not already handed to the flat optimiser's buckets (gradients from another source;
        # without one: all of them); tensors without a gradient this step -- e.g. the projector on a batch that came with ready
        # prompt_embeds -- count as 0 there
        rest = {}
        for k, g in grads.items():
            if self.data_parallel and not k.startswith(self.PROJ):
                continue                  # a factor's gradient is already where the optimiser reads it
            stamp = self._sunk.get(k)
            if stamp is None:
                rest[k] = g
            elif stamp != (g.data_ptr(), g._version):
                raise RuntimeError(f"optimizer_step: the gradient passed for {k} is not the one forward_backward already "
                                   "handed to the sharded optimiser (it was replaced or modified in place afterwards) and "
                                   "would be ignored: with sharded=True accumulate by calling forward_backward again, and "
                                   "scale through lr / max_grad_norm, not on the returned tensors")
        self._sunk = {}
        if self.opt is None:
            sumsq = self.local.step(rest)
        else:
            if rest:
                self.opt.accumulate(rest)
            norm = self.opt.step()
            sumsq = norm * norm
        self._lora_remerge()              # data_parallel: every rank holds the same factors after the all-gather
        self.bw.refresh()
        return sumsq

    def prodigy_state(self):
        """The Prodigy scalars (``d``, ``dlr``, ``k``, ...; ``ops.prodigy_state``) as python numbers -- this synchronises; log
        ``d * lr`` from it as the reference does (train_denoiser.py:1364-1373)."""
        if self.optimizer != "prodigy":
            raise RuntimeError("prodigy_state(): the optimiser is " + self.optimizer)
        return self._optim.prodigy_state()

    def _lora_remerge(self):
        """The factors changed: re-merge exactly the weights the trained adapter touches, one launch each, from their bases.  The
        model's packs are kept -- ``bw.refresh()`` re-copies, in place, the fused operands built from those weights."""
        if self.lora is None:
            return
        pk = self.model._packed
        self.model.lora_mark_stale(self.lora)
        self.model._lora_sync()
        self.model._packed = pk

    def discard(self):
        """Drop the gradients of the backward passes since the last optimiser step (a step that is deliberately skipped, e.g.
        a non-finite loss; the reference's ``optimizer.zero_grad()``, train_denoiser.py:1180).  With ``sharded=True`` it finishes
        the reduce-scatters already in flight and starts none; the decision to skip must be the same on every rank (take it
        on an all-reduced loss or flag).  Without it a skipped backward pass would be summed into the
        next step as a further micro-batch."""
        if self.opt is not None:
            self.opt.zero_grad()
        self._sunk = {}

    KINDS = dict(per_tensor="sharded=False, lora=None (kind 'per_tensor')", lora="lora= without data_parallel (kind 'lora')",
                 sharded="sharded=True, lora=None (kind 'sharded')", lora_dp="lora= with data_parallel=True (kind 'lora_dp')")

    def _kind(self):
        if self.data_parallel:
            return "lora_dp"
        return "sharded" if self.opt is not None else "lora" if self.lora is not None else "per_tensor"

    def state_dict(self):
        """Optimiser state for ``accelerator.save_state``-style checkpoints (train_denoiser.py:1229): the ZeRO-2 shard of
        this rank (``zero.ShardedAdamW.state_dict``) or, unsharded, the per-tensor fp32 masters and moments."""
        if self.opt is not None:
            return dict(kind=self._kind(), opt=self.opt.state_dict())
        return dict(kind=self._kind(), **self.local.state_dict())

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Resume (train_denoiser.py:349-367, 769): restores the state and rewrites the model's trainable bf16 parameters from
        the fp32 masters, so the next step continues bit for bit."""
        kind = sd.get("kind", "per_tensor")
        if kind != self._kind():
            raise ValueError(f"optimiser state was saved with {self.KINDS.get(kind, repr(kind))}, this step runs with "
                             f"{self.KINDS[self._kind()]}")
        inner = sd["opt"] if self.opt is not None else sd
        saved_opt = inner.get("optimizer", "adamw")
        if saved_opt != self.optimizer:
            raise ValueError(f"optimiser state was saved by optimizer={saved_opt!r}, this step runs optimizer={self.optimizer!r}")
        self._sunk = {}
        self._optim.load_state_dict(inner)
        self._lora_remerge()
        self.bw.refresh()
        self.model._packed = None

    def step(self, **batch):
        loss, grads, d_enc = self.forward_backward(**batch)
        sumsq = self.optimizer_step(grads)
        return dict(loss=loss, grad_sumsq=sumsq, d_prompt_embeds=d_enc, grads=grads)
