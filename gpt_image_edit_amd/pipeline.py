"""FluxKontextPipeline -- MI355X-native counterpart of the reference's pipeline driver.

Mirrors the call surface and semantics of ``univa/utils/flux_pipeline.py::FluxKontextPipeline.__call__``
(:732-1138) for the embeds-driven path every reference caller uses (``univa/serve/cli.py:239-248``,
``univa/eval/gedit/step1_gen_samples.py:194-203``, ``train_denoiser.py:1587-1600``):
same argument names and defaults, the ``max_area`` / preferred-resolution quirks, the same
latent packing, ids, sigma schedule, 28-step Euler loop and VAE decode -- but the loop body is

    transformer (HIP MMDiT)  ->  fused slice + Euler update (one HIP kernel, in place; for a masked edit the same launch
                                 also puts the re-noised preserved picture back outside the mask)

over ONE persistent token buffer [B, S_tgt + S_cond, 64] (target tokens first, condition tokens after:
the reference's per-step ``torch.cat([latents, image_latents], dim=1)`` disappears), with all per-step
scalars prepared before the loop so the 28 steps enqueue without a host sync.

Pixels either side of the path: ``image_processor.VaeImageProcessor`` restates the
diffusers helper the reference pipeline calls; uint8 pixels (PIL / numpy / uint8 tensors) take two fused HIP kernels
(normalise + nearest resize + cast in front of the VAE encoder, clamp + quantise behind the decoder); ``resample=`` puts Pillow's
antialiased byte resize (``fk_resample_pass_u8``) in front of the first and behind the second.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import helpers, image_processor, ops
from .scheduler import FlowMatchEulerDiscreteScheduler

BF16 = torch.bfloat16


class FluxPipelineOutput(SimpleNamespace):
    pass


class FluxKontextPipeline:
    def __init__(self, transformer, vae, scheduler=None, text_encoder=None, tokenizer=None,
                 text_encoder_2=None, tokenizer_2=None, use_graph=None):
        """use_graph (default: FK_GRAPH=1 in the environment): run the conditioning pass + the whole denoise loop of an
        edit as ONE hipGraph launch (captured once per call shape, replayed afterwards; bit-identical to the eager loop).
        The loop allocates nothing and never synchronises, so the capture is a plain stream capture; what it buys is the
        host: ~5 400 ctypes launches per edit become one graph launch -- insurance for 8 ranks sharing one host."""
        self.use_graph = (os.environ.get("FK_GRAPH", "0") == "1") if use_graph is None else bool(use_graph)
        self._loop_graph = None       # (key, static tensors, torch.cuda.CUDAGraph) of the latest call shape
        self.transformer = transformer
        self.vae = vae
        self.scheduler = scheduler or FlowMatchEulerDiscreteScheduler()
        self.text_encoder, self.tokenizer = text_encoder, tokenizer
        self.text_encoder_2, self.tokenizer_2 = text_encoder_2, tokenizer_2
        self.vae_scale_factor = 2 ** (len(vae.config.block_out_channels) - 1)
        self.latent_channels = vae.config.latent_channels
        self.default_sample_size = 128
        self.tokenizer_max_length = tokenizer.model_max_length if tokenizer is not None else 77   # :253-255
        self.image_processor = image_processor.VaeImageProcessor(vae_scale_factor=self.vae_scale_factor * 2)
        self._interrupt = False
        self._guidance_scale = None
        self._num_timesteps = 0
        self._cache_state = None      # eager step-cache buffers of the latest call shape (transformer.step_cache_state)
        self._said_adaptive_is_eager = False

    # static helpers the training script reaches for directly (train_denoiser.py:925,1009,1021,1098)
    _pack_latents = staticmethod(helpers._pack_latents)
    _unpack_latents = staticmethod(helpers._unpack_latents)
    _prepare_latent_image_ids = staticmethod(helpers._prepare_latent_image_ids)

    def to(self, device):
        self.transformer.to(device)
        self.vae.to(device)
        return self

    @property
    def device(self):
        return self.transformer.device

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def num_timesteps(self):
        return self._num_timesteps

    def enable_vae_slicing(self): self.vae.enable_slicing()
    def disable_vae_slicing(self): self.vae.disable_slicing()
    def enable_vae_tiling(self): self.vae.enable_tiling()
    def disable_vae_tiling(self): self.vae.disable_tiling()
    def maybe_free_model_hooks(self): pass

    # ---- input validation: the cases that can still occur with embeds-only input ----------------------
    def check_inputs(self, height, width, prompt_embeds, pooled_prompt_embeds, max_sequence_length=512):
        m = self.vae_scale_factor * 2
        if height % m != 0 or width % m != 0:
            print(f"`height` and `width` have to be divisible by {m} but are {height} and {width}. "
                  f"Dimensions will be resized accordingly")
        if prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and "
                             "`prompt_embeds` undefined.")
        if pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed. Make "
                             "sure to generate `pooled_prompt_embeds` from the same text encoder that was used to "
                             "generate `prompt_embeds`.")
        if max_sequence_length is not None and max_sequence_length > 512:
            raise ValueError(f"`max_sequence_length` cannot be greater than 512 but is {max_sequence_length}")

    # flux_pipeline.py:266-438 (the encoders are transformers' CLIPTextModel / T5EncoderModel, reused as they are)
    def _get_t5_prompt_embeds(self, prompt, num_images_per_prompt=1, max_sequence_length=512, device=None, dtype=None):
        if self.text_encoder_2 is None or self.tokenizer_2 is None:
            raise ValueError("string prompts need `text_encoder_2` / `tokenizer_2` (T5); pass `prompt_embeds` instead")
        device = device or self.device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        ids = self.tokenizer_2(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                               return_length=False, return_overflowing_tokens=False, return_tensors="pt").input_ids
        untruncated = self.tokenizer_2(prompt, padding="longest", return_tensors="pt").input_ids
        if untruncated.shape[-1] >= ids.shape[-1] and not torch.equal(ids, untruncated):
            removed = self.tokenizer_2.batch_decode(untruncated[:, self.tokenizer_max_length - 1:-1])
            print(f"The following part of your input was truncated because `max_sequence_length` is set to "
                  f" {max_sequence_length} tokens: {removed}")
        enc_device = next(self.text_encoder_2.parameters()).device
        embeds = self.text_encoder_2(ids.to(enc_device), output_hidden_states=False)[0]
        embeds = embeds.to(dtype=self.text_encoder_2.dtype, device=device)
        n, seq_len, _ = embeds.shape
        return embeds.repeat(1, num_images_per_prompt, 1).view(n * num_images_per_prompt, seq_len, -1)

    def _get_clip_prompt_embeds(self, prompt, num_images_per_prompt=1, device=None):
        if self.text_encoder is None or self.tokenizer is None:
            raise ValueError("string prompts need `text_encoder` / `tokenizer` (CLIP); pass `pooled_prompt_embeds` "
                             "instead")
        device = device or self.device
        prompt = [prompt] if isinstance(prompt, str) else prompt
        ids = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer_max_length, truncation=True,
                             return_overflowing_tokens=False, return_length=False, return_tensors="pt").input_ids
        untruncated = self.tokenizer(prompt, padding="longest", return_tensors="pt").input_ids
        if untruncated.shape[-1] >= ids.shape[-1] and not torch.equal(ids, untruncated):
            removed = self.tokenizer.batch_decode(untruncated[:, self.tokenizer_max_length - 1:-1])
            print(f"The following part of your input was truncated because CLIP can only handle sequences up to"
                  f" {self.tokenizer_max_length} tokens: {removed}")
        enc_device = next(self.text_encoder.parameters()).device
        pooled = self.text_encoder(ids.to(enc_device), output_hidden_states=False).pooler_output
        pooled = pooled.to(dtype=self.text_encoder.dtype, device=device)
        n = pooled.shape[0]
        return pooled.repeat(1, num_images_per_prompt).view(n * num_images_per_prompt, -1)

    def encode_prompt(self, prompt, prompt_2=None, device=None, num_images_per_prompt=1, prompt_embeds=None,
                      pooled_prompt_embeds=None, max_sequence_length=512, lora_scale=None):
        """(prompt_embeds, pooled_prompt_embeds, text_ids): CLIP pooled output of ``prompt``, T5 last hidden state of
        ``prompt_2 or prompt``; given embeddings pass through untouched (flux_pipeline.py:361-438)."""
        device = device or self.device
        if prompt_embeds is None:
            prompt = [prompt] if isinstance(prompt, str) else prompt
            prompt_2 = prompt_2 or prompt
            prompt_2 = [prompt_2] if isinstance(prompt_2, str) else prompt_2
            pooled_prompt_embeds = self._get_clip_prompt_embeds(prompt, num_images_per_prompt, device)
            prompt_embeds = self._get_t5_prompt_embeds(prompt_2, num_images_per_prompt, max_sequence_length, device)
        dtype = self.text_encoder.dtype if self.text_encoder is not None else self.transformer.dtype
        text_ids = torch.zeros(prompt_embeds.shape[1], 3).to(device=device, dtype=dtype)
        return prompt_embeds, pooled_prompt_embeds, text_ids

    # ---- LoRA adapters for the denoiser (diffusers' FluxLoraLoaderMixin names; lora.py: merged into the weights) -----------
    def _lora_model(self):
        if not hasattr(self.transformer, "load_lora_adapter"):
            raise ValueError("LoRA adapters need a transformer with the adapter API (HipFluxTransformer2DModel)")
        return self.transformer

    def load_lora_weights(self, path_or_dict, adapter_name="default", weight=1.0):
        """A diffusers / PEFT LoRA (``transformer.<module>.lora_A.weight`` ...) merged into the denoiser.  Text-encoder keys
        are ignored (returned); any other unknown key is a ``ValueError``."""
        return self._lora_model().load_lora_adapter(path_or_dict, adapter_name=adapter_name, weight=weight)

    def set_adapters(self, adapter_names, adapter_weights=None):
        self._lora_model().set_adapters(adapter_names, adapter_weights)

    def delete_adapters(self, adapter_names):
        self._lora_model().delete_adapters(adapter_names)

    def save_lora_weights(self, path, adapter_name="default"):
        """Write adapter ``adapter_name`` (trained through ``DenoiserTrainStep(lora=...)``, or loaded) as one safetensors file
        in the layout ``load_lora_weights`` reads.  ``path``: the file, or a directory (then
        ``pytorch_lora_weights.safetensors`` in it, diffusers' name).  Returns the file's path."""
        import os
        from .checkpoint import _safetensors
        st, _ = _safetensors()
        path = os.fspath(path)
        if os.path.isdir(path) or not path.endswith(".safetensors"):
            os.makedirs(path, exist_ok=True)
            path = os.path.join(path, "pytorch_lora_weights.safetensors")
        sd = self._lora_model().lora_state_dict(adapter_name)
        st.save_file({k: v.contiguous() for k, v in sd.items()}, path, metadata={"format": "pt"})
        return path

    def unload_lora_weights(self):
        self._lora_model().unload_lora()

    def get_active_adapters(self):
        return self._lora_model().active_adapters()

    def _encode_vae_image(self, image, nhwc=False):
        """(mode(vae.encode(image)) - shift) * scale, the affine fused into the layout kernel (:600-613)."""
        cfg = self.vae.config
        return self.vae.encode(image, post_add=-cfg.shift_factor, post_mul=cfg.scaling_factor,
                               nhwc=nhwc).latent_dist.mode()

    def prepare_latents(self, image, batch_size, num_channels_latents, height, width, dtype, device,
                        generator=None, latents=None):
        """Same contract as flux_pipeline.py:648-708 -> (latents, image_latents, latent_ids, image_ids)."""
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an "
                             f"effective batch size of {batch_size}. Make sure the batch size matches the length "
                             f"of the generators.")
        height = 2 * (int(height) // (self.vae_scale_factor * 2))
        width = 2 * (int(width) // (self.vae_scale_factor * 2))
        image_latents = image_ids = None
        if image is not None:
            image = image.to(device=device)
            if isinstance(image, image_processor.NhwcPixels):  # fused pixel route (explicit marker, not a shape test)
                image_latents = self._encode_vae_image(image.tensor, nhwc=True)
            elif image.shape[1] != self.latent_channels:
                image_latents = self._encode_vae_image(image)
            else:
                image_latents = image.to(dtype)
            n = image_latents.shape[0]
            if batch_size > n and batch_size % n == 0:
                image_latents = torch.cat([image_latents] * (batch_size // n), dim=0)
            elif batch_size > n:
                raise ValueError(f"Cannot duplicate `image` of batch size {n} to {batch_size} text prompts.")
            ih, iw = image_latents.shape[2:]
            image_latents = self._pack_latents(image_latents, batch_size, num_channels_latents, ih, iw)
            image_ids = self._prepare_latent_image_ids(batch_size, ih // 2, iw // 2, device, dtype)
            image_ids[..., 0] = 1  # condition tokens: first id = 1
        latent_ids = self._prepare_latent_image_ids(batch_size, height // 2, width // 2, device, dtype)
        if latents is None:
            shape = (batch_size, num_channels_latents, height, width)
            if isinstance(generator, list):
                # diffusers' randn_tensor: sample i comes from its own generator (on that generator's device)
                noise = torch.cat([torch.randn((1, *shape[1:]), generator=g, device=g.device, dtype=dtype).to(device)
                                   for g in generator], dim=0)
            else:
                gdev = generator.device if isinstance(generator, torch.Generator) else device
                noise = torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)
            latents = self._pack_latents(noise, batch_size, num_channels_latents, height, width)
        else:
            latents = latents.to(device=device, dtype=dtype)
        return latents, image_latents, latent_ids, image_ids

    def _prepare_mask(self, mask_image, batch_size, height, width, device, edit=None):
        """``mask_image`` (float [1 or B, 1, Hm, Wm] in [0, 1]; uint8 tensor / numpy / PIL greyscale, 255 = repaint) -> the
        compact token mask [1 or B, S_tgt, 4] of the fused step: binarised at 0.5, nearest-resized to the latent size.

        ``edit`` (``_check_pixel_edit``; None: today's path): the mask as bytes on the device, feathered (``fk_mask_blur_u8``) when
        ``mask_blur`` > 0, and from then on THE mask -- the overlay's alpha, the source of the crop box (``fk_mask_bbox_u8`` on
        alpha >= 1, the call's one read-back, then ``helpers.mask_crop_box``) and, sliced to that box, of the token mask
        (``_prepare_edit_mask``)."""
        m = mask_image
        if hasattr(m, "convert"):
            m = [m]
        if isinstance(m, (list, tuple)) and m and hasattr(m[0], "convert"):
            arrs = [np.asarray(im.convert("L"), dtype=np.uint8) for im in m]
            if any(a.shape != arrs[0].shape for a in arrs):
                raise ValueError("mask images must share one size")
            m = np.stack(arrs)
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(np.ascontiguousarray(m))
        if not torch.is_tensor(m):
            raise ValueError("pass `mask_image` as a [1 or B, 1, H, W] tensor in [0, 1], or as uint8 / PIL greyscale")
        if edit is not None:
            return self._prepare_edit_mask(m, edit, batch_size, height, width, device)
        m = m.float() / 255.0 if m.dtype == torch.uint8 else m.float()
        if m.dim() == 2:
            m = m[None]
        if m.dim() == 3:
            m = m[:, None]
        if m.dim() != 4 or m.shape[1] != 1:
            raise ValueError(f"`mask_image` must be [1 or B, 1, H, W], got {tuple(m.shape)}")
        if m.shape[0] not in (1, batch_size):
            raise ValueError(f"`mask_image` has batch {m.shape[0]}: must be 1 or the batch size {batch_size}")
        sf = self.vae_scale_factor * 2
        return ops.pack_inpaint_mask(m, 2 * (int(height) // sf), 2 * (int(width) // sf)).to(device)

    def _prepare_edit_mask(self, m, edit, batch_size, height, width, device):
        """``_prepare_mask`` of a call with ``padding_mask_crop`` / ``mask_blur`` / ``overlay``: fills ``edit.alpha`` (uint8
        [1 or B, Hm, Wm] on the device), ``edit.box`` and ``edit.renorm``, returns the token mask of the box."""
        if m.dtype != torch.uint8:          # a float mask's bytes: rint(255 m)
            m = m.float().clamp(0, 1).mul(255).round().to(torch.uint8)
        if m.dim() == 4 and m.shape[1] == 1:
            m = m[:, 0]
        if m.dim() == 2:
            m = m[None]
        if m.dim() != 3:
            raise ValueError(f"`mask_image` must be [1 or B, 1, H, W], got {tuple(m.shape)}")
        if m.shape[0] not in (1, batch_size):
            raise ValueError(f"`mask_image` has batch {m.shape[0]}: must be 1 or the batch size {batch_size}")
        Hm, Wm = m.shape[1:]
        if edit.pic is not None and tuple(edit.pic.shape[1:3]) != (Hm, Wm):
            raise ValueError(f"`mask_image` is {Hm} x {Wm}, the preserved picture {edit.pic.shape[1]} x {edit.pic.shape[2]}: "
                             "a crop or an overlay needs both at one size")
        a = m.to(device).contiguous()
        if edit.sigma > 0:
            a = ops.mask_blur(a, edit.sigma)
        edit.alpha, edit.box = a, (0, 0, Wm, Hm)
        if edit.crop:
            bbox = ops.mask_bbox(a, 1).tolist()             # 16 bytes: the call's one read-back
            if bbox[2] <= bbox[0] or bbox[3] <= bbox[1]:
                raise ValueError("`mask_image` is empty: `padding_mask_crop` has no box to crop to")
            x0, y0, x1, y1 = edit.box = helpers.mask_crop_box(bbox, Wm, Hm, edit.pad, width, height)
            # the existing quirk, stated for the box: a second normalisation iff no normalised value of it is negative
            # (with `resample` the resized bytes decide instead: _crop_pixels)
            edit.renorm = edit.resample is None and bool(edit.pic[:, y0:y1, x0:x1].min() >= 128)
            a = a[:, y0:y1, x0:x1]
        if edit.pic is not None:
            edit.pic = edit.pic.to(device).contiguous()
        sf = self.vae_scale_factor * 2
        return ops.pack_inpaint_mask(a[:, None].float() / 255.0, 2 * (int(height) // sf), 2 * (int(width) // sf)).to(device)

    def _check_pixel_edit(self, image, init_image, mask_image, padding_mask_crop, mask_blur, overlay, output_type):
        """The refusals of ``padding_mask_crop`` / ``mask_blur`` / ``overlay``, before any work, and what the call carries from
        here on: sigma, pad, whether it crops and overlays, and the preserved picture's bytes (``pic``, uint8 [N, H, W, 3])."""
        sigma = float(mask_blur)
        if not 0.0 <= sigma <= helpers.MASK_BLUR_MAX_SIGMA:
            raise ValueError(f"`mask_blur` is a sigma in [0, {helpers.MASK_BLUR_MAX_SIGMA:g}] pixels, not {mask_blur!r}")
        crop = padding_mask_crop is not None
        if crop and (isinstance(padding_mask_crop, bool) or not isinstance(padding_mask_crop, (int, np.integer))
                     or padding_mask_crop < 0):
            raise ValueError(f"`padding_mask_crop` is an int >= 0 or None, not {padding_mask_crop!r}")
        if mask_image is None:
            raise ValueError("`padding_mask_crop` / `mask_blur` / `overlay` need `mask_image`")
        if overlay is None:                 # a crop is pasted back, except where the caller asks for the crop's latents
            overlay = crop and output_type != "latent"
        if overlay and output_type not in ("pil", "np_uint8"):
            raise ValueError(f'`overlay` returns uint8 pixels: `output_type` is "pil" or "np_uint8", not {output_type!r}')
        pic = None
        if crop or overlay:
            pic = image_processor.as_uint8_nhwc(image if init_image is None else init_image)
            if pic is None:
                raise ValueError("`padding_mask_crop` / `overlay` need the preserved picture as uint8 pixels (PIL / numpy / uint8 "
                                 "tensor [N,H,W,3]): a float tensor or latents have no bytes to keep")
        return SimpleNamespace(sigma=sigma, pad=None if not crop else int(padding_mask_crop), crop=crop, overlay=bool(overlay),
                               pic=pic, alpha=None, box=None, renorm=False, resample=None)

    def _encode_init_image(self, init_image, batch_size, num_channels_latents, height, width, device, edit=None, resample=None):
        """Packed latents [B, S_tgt, 64] of the picture a masked edit preserves, at the target size: the condition image's
        own routes (uint8 pixels through the fused gather, float tensors through resize + preprocess) without the
        preferred-resolution snap; pre-encoded latents must already have the target's latent size.  A cropped edit
        (``edit.crop``) samples the picture's box instead (``fk_pixels_u8_box_to_nhwc_bf16``, bilinear).  ``resample`` (a filter
        name): uint8 pixels are resized with ``ops.resample_u8`` first, and the gather is an identity."""
        h_lat, w_lat = height // self.vae_scale_factor, width // self.vae_scale_factor
        u8 = image_processor.as_uint8_nhwc(init_image)
        if edit is not None and edit.crop:
            lat = self._encode_vae_image(self._crop_pixels(edit, height, width).tensor, nhwc=True)
        elif u8 is not None:
            if resample is not None:
                u8 = ops.resample_u8(u8.to(device), height, width, resample)
            px = image_processor.pixels_to_latent_input(u8, height, width, device)
            lat = self._encode_vae_image(px.tensor, nhwc=True)
        elif isinstance(init_image, torch.Tensor) and init_image.dim() == 4 and init_image.size(1) == self.latent_channels:
            lat = init_image.to(device=device, dtype=BF16)
        elif isinstance(init_image, torch.Tensor) and init_image.dim() == 4:
            img = init_image
            if tuple(img.shape[2:]) != (height, width):
                img = self.image_processor.resize(img.float(), height, width)
            lat = self._encode_vae_image(self.image_processor.preprocess(img, height, width).to(device=device))
        else:
            raise NotImplementedError("pass the picture to preserve as a [N,3,H,W] tensor in [-1,1], as uint8 pixels "
                                      "(PIL / numpy / uint8 tensor [N,H,W,3]) or as latents [N,16,h,w]")
        if tuple(lat.shape[2:]) != (h_lat, w_lat):
            raise ValueError(f"the preserved picture's latents are {tuple(lat.shape[2:])}, the target's ({h_lat}, {w_lat})")
        n = lat.shape[0]
        if batch_size > n and batch_size % n == 0:
            lat = torch.cat([lat] * (batch_size // n), dim=0)
        elif batch_size != n:
            raise ValueError(f"Cannot duplicate the preserved picture of batch size {n} to batch size {batch_size}.")
        return self._pack_latents(lat, batch_size, num_channels_latents, h_lat, w_lat).contiguous()

    @staticmethod
    def _crop_pixels(edit, height, width):
        """The preserved picture's box at height x width, as the VAE encoder's input: point-sampled bilinear, or with
        ``edit.resample`` the box's view resized byte for byte and passed through the whole-picture gather at equal size (which
        decides the second normalisation on the resized bytes)."""
        if edit.resample is not None:
            x0, y0, x1, y1 = edit.box
            resized = ops.resample_u8(edit.pic[:, y0:y1, x0:x1], height, width, edit.resample)
            return image_processor.pixels_to_latent_input(resized, height, width, resized.device)
        return image_processor.NhwcPixels(ops.pixels_box_to_nhwc(edit.pic, edit.box, height, width, 32, edit.renorm))

    @torch.no_grad()
    def __call__(self, image=None, prompt=None, prompt_2=None, negative_prompt=None, negative_prompt_2=None,
                 true_cfg_scale=1.0, height=None, width=None, num_inference_steps=28, sigmas=None,
                 guidance_scale=3.5, num_images_per_prompt=1, generator=None, latents=None, prompt_embeds=None,
                 pooled_prompt_embeds=None, negative_prompt_embeds=None, negative_pooled_prompt_embeds=None,
                 output_type="pil", return_dict=True, joint_attention_kwargs=None, callback_on_step_end=None,
                 callback_on_step_end_tensor_inputs=("latents",), max_sequence_length=512,
                 max_area=1024 ** 2, _auto_resize=True, mask_image=None, strength=1.0, init_image=None, step_cache=None,
                 padding_mask_crop=None, mask_blur=0.0, overlay=None, resample=None, latent_state="bf16"):
        """``mask_image`` / ``strength`` / ``init_image`` (diffusers' ``FluxKontextInpaintPipeline``): repaint only where the
        mask is 1 and keep ``init_image`` (default: ``image``, resized to the target size) elsewhere; ``strength`` < 1 starts
        the loop inside the schedule from the re-noised ``init_image`` instead of from noise.  ``image`` stays the Kontext
        condition.  Without the three the call is the plain edit, launch for launch.

        ``step_cache`` (a ``step_cache.StepCache``): skip the MMDiT blocks on the steps its rule or schedule says, adding the
        residual kept at the last computed step instead (one decision per step for the whole model batch).  A schedule is
        sync-free and graph-capturable; the adaptive rule reads 8 bytes back per step and therefore runs the eager loop.
        ``StepCache(..., measure="first_block")`` runs block 0 at every step, measures what it added to the image stream and
        skips only the blocks behind it.  ``None`` is today's call, launch for launch.

        ``latent_state``: "bf16" is today's call, launch for launch -- the latents are rounded to bf16 at every step, as the
        reference's loop rounds them.  "fp32" carries them in a float32 buffer of the call's own ([B, S_tgt, 64], seeded from
        the bf16 start tokens) through ``fk_solver_step_f32``, for whichever scheduler is installed; the model still reads the
        bf16 token rows, which receive the state's one rounding per step, and the returned latents are those rows.

        ``padding_mask_crop`` / ``mask_blur`` / ``overlay`` (diffusers' ``padding_mask_crop`` + ``apply_overlay``; parity with PIL's
        GaussianBlur unpinned): work on the masked box and paste the result back.  They need ``mask_image``;
        a crop or an overlay also needs the preserved picture (``init_image``, else ``image``) as uint8 pixels of the mask's size.
        ``mask_blur`` (sigma in pixels of the mask image, at most 64) feathers the mask, which from then on is the mask everywhere.
        ``padding_mask_crop`` (int >= 0): one box per call -- the bounding box over the mask batch of alpha >= 1, padded and grown
        to the target's aspect (``helpers.mask_crop_box``) -- is sampled bilinearly at ``height`` x ``width`` and edited in place
        of the picture; without ``init_image`` the Kontext condition is the same crop.  ``overlay`` (None: on with a crop, except
        for ``output_type="latent"``, which returns the crop's latents): the returned image has the preserved picture's size and
        its own bytes outside the box and wherever alpha is 0, the alpha blend of the resampled result elsewhere; without a crop
        the box is the whole picture.  The output carries ``crop_box``.  With all three at their defaults the call is today's
        call, launch for launch.  Without ``resample`` the box is point-sampled in both directions.

        ``resample`` (None | "nearest" | "bilinear" | "bicubic" | "lanczos"): how pictures that arrive as bytes (PIL / numpy uint8 /
        uint8 tensor) are resized.  ``None`` and ``"nearest"`` are today's call, launch for launch.  A filter name is Pillow's
        antialiased 8-bit ``Image.resize`` with that filter, byte for byte (``ops.resample_u8``; diffusers resizes PIL inputs with
        lanczos): the condition image is resized to its snapped size and ``init_image`` to the target's, then each takes today's
        gather at equal size, whose second-normalisation rule therefore reads the resized bytes.  With ``padding_mask_crop`` the
        box ``pic[:, y0:y1, x0:x1]`` is resized the same way (crop, then resize: windows clamp at the box), and the second
        normalisation is decided on the RESIZED bytes -- a lanczos or bicubic overshoot can take a byte below 128 where every byte
        of the box is >= 128, so this can differ from the point-sampled crop's decision; the token mask stays the binarised nearest
        one.  With ``overlay`` the decoded result becomes bytes (``fk_image_to_u8_nhwc``), is resized to the box's size and blended
        over the picture's bytes in integers (``fk_bytes_overlay_u8``); at equal size with alpha in {0, 255} these are today's
        overlay bytes.  A filter name with a float-tensor or latent picture is a ``ValueError`` (there are no bytes to filter), and
        so is an unknown name.  All of it is in front of the first step or behind the decode.

        ``joint_attention_kwargs["scale"]`` (default 1.0): the call scale of the loaded LoRA adapters (``load_lora_weights``)."""
        device = self.device
        if latent_state not in ("bf16", "fp32"):
            raise ValueError(f'`latent_state` is "bf16" or "fp32", not {latent_state!r}')
        if joint_attention_kwargs and "scale" in joint_attention_kwargs:
            # the LoRA call scale: merged into the weights before the loop and left there until another scale is asked for;
            # without adapters it is ignored.  It is no argument of the transformer call, so it leaves the kwargs here
            joint_attention_kwargs = dict(joint_attention_kwargs)
            scale = joint_attention_kwargs.pop("scale")
            if getattr(self.transformer, "lora_loaded", None) is not None and self.transformer.lora_loaded():
                self.transformer.set_lora_scale(1.0 if scale is None else scale)
        elif getattr(self.transformer, "lora_loaded", None) is not None and self.transformer.lora_loaded():
            self.transformer.set_lora_scale(1.0)
        if resample is not None and resample != "nearest" and resample not in helpers.RESAMPLE_FILTERS:
            raise ValueError(f'`resample` is None, "nearest", "bilinear", "bicubic" or "lanczos", not {resample!r}')
        resample = None if resample == "nearest" else resample
        if resample is not None:
            for name, pic in (("image", image), ("init_image", init_image)):
                if pic is not None and image_processor.as_uint8_nhwc(pic) is None:
                    raise ValueError(f'`resample="{resample}"` filters bytes: `{name}` is a float tensor or latents, which have none '
                                     "(pass PIL / numpy uint8 / a uint8 tensor [N,H,W,3], or leave `resample` out)")
        helpers.strength_t_start(num_inference_steps, strength)     # validates strength before any work
        if step_cache is not None:                                  # ... and the schedule against the executed step count
            n_all = num_inference_steps if sigmas is None else len(sigmas)
            step_cache.validate(n_all - helpers.strength_t_start(n_all, strength))
        inpaint = mask_image is not None or init_image is not None or strength < 1.0
        if (mask_image is not None or strength < 1.0) and image is None and init_image is None:
            raise ValueError("`mask_image` / `strength` < 1 need a picture to preserve: pass `image` or `init_image`")
        edit = None
        if padding_mask_crop is not None or mask_blur or overlay:
            edit = self._check_pixel_edit(image, init_image, mask_image, padding_mask_crop, mask_blur, overlay, output_type)
            edit.resample = resample
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make "
                             "sure to only forward one of the two.")   # :510-514
        if prompt is not None:
            # string prompts: the pipeline's own CLIP / T5 encoders (:899-906); every caller in the reference passes
            # embeddings instead (VLM tokens and/or T5), which skip this
            prompt_embeds, pooled_prompt_embeds, _ = self.encode_prompt(
                prompt, prompt_2, device=device, max_sequence_length=max_sequence_length)
        if negative_prompt is not None and negative_prompt_embeds is None and true_cfg_scale > 1:
            negative_prompt_embeds, negative_pooled_prompt_embeds, _ = self.encode_prompt(
                negative_prompt, negative_prompt_2, device=device, max_sequence_length=max_sequence_length)
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        multiple_of = self.vae_scale_factor * 2
        oh, ow = height, width
        height, width = helpers.fit_to_max_area(height, width, max_area, multiple_of)
        if (height, width) != (oh, ow):
            print(f"Generation `height` and `width` have been adjusted to {height} and {width} to fit the model "
                  f"requirements.")
        self.check_inputs(height, width, prompt_embeds, pooled_prompt_embeds, max_sequence_length)
        self._guidance_scale = guidance_scale
        self._interrupt = False
        has_neg = negative_prompt_embeds is not None and negative_pooled_prompt_embeds is not None
        do_true_cfg = true_cfg_scale > 1 and has_neg  # :928
        batch_size = prompt_embeds.shape[0] * num_images_per_prompt
        prompt_embeds = prompt_embeds.to(device=device, dtype=BF16)
        pooled_prompt_embeds = pooled_prompt_embeds.to(device=device, dtype=BF16)
        if num_images_per_prompt > 1:
            prompt_embeds = prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0)
            pooled_prompt_embeds = pooled_prompt_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        text_ids = torch.zeros(prompt_embeds.shape[1], 3, device=device, dtype=BF16)  # :436
        if do_true_cfg:
            # The reference runs a second transformer call per step on the negative embeddings (:1080-1095).  Samples
            # are independent in the MMDiT, so here the positive and the negative pass are ONE call on a batch of 2B
            # (twice the GEMM rows per weight read), followed by the fused combine kernel.
            neg_e = negative_prompt_embeds.to(device=device, dtype=BF16)
            neg_p = negative_pooled_prompt_embeds.to(device=device, dtype=BF16)
            if num_images_per_prompt > 1:
                neg_e = neg_e.repeat_interleave(num_images_per_prompt, dim=0)
                neg_p = neg_p.repeat_interleave(num_images_per_prompt, dim=0)
            if neg_e.shape != prompt_embeds.shape:
                raise NotImplementedError("true CFG needs negative_prompt_embeds of the positive embeddings' shape "
                                          "(pad the shorter prompt; the joint pass shares one text length)")
            model_embeds = torch.cat([prompt_embeds, neg_e], dim=0)
            model_pooled = torch.cat([pooled_prompt_embeds, neg_p], dim=0)
        else:
            model_embeds, model_pooled = prompt_embeds, pooled_prompt_embeds
        model_batch = model_embeds.shape[0]

        if edit is None:
            mask = None if mask_image is None else self._prepare_mask(mask_image, batch_size, height, width, device)
        else:
            if edit.pic is not None and edit.pic.shape[0] not in (1, batch_size):
                raise ValueError(f"the preserved picture has batch {edit.pic.shape[0]}: must be 1 or the batch size {batch_size}")
            mask = self._prepare_mask(mask_image, batch_size, height, width, device, edit)

        # 3. condition image: preferred-resolution snap + nearest resize (VaeImageProcessor tensor path)
        image_in, cond_hw = image, None             # cond_hw: pixel size the condition latents stand for
        u8 = image_processor.as_uint8_nhwc(image) if image is not None else None
        if edit is not None and edit.crop and init_image is None:
            # `image` stands in as the preserved picture: the condition is the same crop, at the size the box snaps to
            ih, iw = self.image_processor.get_default_height_width(None, edit.box[3] - edit.box[1], edit.box[2] - edit.box[0])
            ih, iw = helpers.preferred_condition_size(ih, iw, multiple_of, _auto_resize) if min(ih, iw) > 0 else (0, 0)
            if min(ih, iw) <= 0:
                raise ValueError(f"the crop box {edit.box} is smaller than one {multiple_of}-pixel token: raise `padding_mask_crop`")
            image = self._crop_pixels(edit, ih, iw)
            cond_hw = (ih, iw)
        elif u8 is not None:
            # uint8 pixels: cli.prepare_condition_images + resize + preprocess + .to(bf16) as ONE HIP gather
            ih, iw = self.image_processor.get_default_height_width(u8.permute(0, 3, 1, 2))
            ih, iw = helpers.preferred_condition_size(ih, iw, multiple_of, _auto_resize)
            if resample is not None:                # antialiased to the snapped size; the gather below is then an identity
                u8 = ops.resample_u8(u8.to(device), ih, iw, resample)
            image = image_processor.pixels_to_latent_input(u8, ih, iw, device)
            cond_hw = (ih, iw)
        elif image is not None and not (isinstance(image, torch.Tensor) and image.size(1) == self.latent_channels):
            if not isinstance(image, torch.Tensor) or image.dim() != 4:
                raise NotImplementedError("pass the condition image as a [N,3,H,W] tensor in [-1,1] (cli.py:99-116) "
                                          "or as uint8 pixels (PIL / numpy / uint8 tensor [N,H,W,3])")
            ih, iw = self.image_processor.get_default_height_width(image)
            ih, iw = helpers.preferred_condition_size(ih, iw, multiple_of, _auto_resize)
            image = self.image_processor.resize(image.float(), ih, iw) if (ih, iw) != tuple(image.shape[2:]) else image
            image = self.image_processor.preprocess(image, ih, iw)
            cond_hw = (ih, iw)
        elif image is not None:
            cond_hw = (image.shape[2] * self.vae_scale_factor, image.shape[3] * self.vae_scale_factor)

        # 4. latents
        num_channels_latents = self.transformer.config.in_channels // 4
        latents, image_latents, latent_ids, image_ids = self.prepare_latents(
            image, batch_size, num_channels_latents, height, width, BF16, device, generator, latents)
        S_tgt = latents.shape[1]
        if image_ids is not None:
            latent_ids = torch.cat([latent_ids, image_ids], dim=0)
            tokens = torch.cat([latents, image_latents], dim=1).contiguous()  # built ONCE, updated in place
        else:
            tokens = latents.contiguous().clone()
        x0 = noise = None
        if mask is not None or strength < 1.0:
            # the preserved picture at the target size: the condition latents when they already are that, else one more encode
            if init_image is None and cond_hw == (height, width):
                x0 = image_latents
            else:
                x0 = self._encode_init_image(image_in if init_image is None else init_image, batch_size,
                                             num_channels_latents, height, width, device, edit, resample)
            noise = latents.contiguous()            # a caller-supplied `latents` serves as the noise, as in diffusers

        # 5. timesteps (host float32 arithmetic, like diffusers' numpy path)
        sig = np.linspace(1.0, 1 / num_inference_steps, num_inference_steps) if sigmas is None else sigmas
        cfg = self.scheduler.config
        mu = helpers.calculate_shift(S_tgt, cfg.get("base_image_seq_len", 256), cfg.get("max_image_seq_len", 4096),
                                     cfg.get("base_shift", 0.5), cfg.get("max_shift", 1.15))
        self.scheduler.set_timesteps(sigmas=sig, mu=mu, device="cpu")
        t_start = helpers.strength_t_start(len(self.scheduler.timesteps), strength)
        timesteps = self.scheduler.timesteps[t_start:]
        self._num_timesteps = len(timesteps)
        # `t.expand(B).to(bf16)` then `/ 1000` (flux_pipeline.py:1065,1069): all steps prepared up front
        t_model = (timesteps.to(BF16) / 1000)[:, None].expand(-1, model_batch).contiguous().to(device)
        guidance = None
        if self.transformer.config.guidance_embeds:
            guidance = torch.full([model_batch], guidance_scale, device=device, dtype=torch.float32)
        self.scheduler.set_begin_index(t_start)
        if t_start > 0:                             # start inside the schedule: the picture re-noised to sigma[t_start]
            ops.scale_noise(x0, noise, float(self.scheduler._sigmas_host[t_start]), out=tokens[:, :S_tgt])
        steps = range(t_start, t_start + len(timesteps))
        model_tokens = torch.empty((model_batch, *tokens.shape[1:]), device=device, dtype=BF16) if do_true_cfg else tokens
        # a second-order multistep scheduler: every step's (c_v, c_h, use_hist) and the previous velocity's buffer, once per call
        solver_order = getattr(self.scheduler, "solver_order", 1)
        if solver_order not in (1, 2):
            raise NotImplementedError(f"the denoise loop has a first- and a second-order step, not solver_order={solver_order}")
        ab2 = [self.scheduler.coefficients(i, i > t_start) for i in steps] if solver_order == 2 else None
        hist = torch.empty((batch_size, S_tgt, tokens.shape[2]), device=device, dtype=BF16) if ab2 is not None else None
        # a float32 latent state: one buffer per call, never an input -- the first executed step seeds it from the start tokens
        state = torch.empty((batch_size, S_tgt, tokens.shape[2]), device=device, dtype=torch.float32) \
            if latent_state == "fp32" else None

        # 6. denoising loop: no allocation, no host sync
        L = SimpleNamespace(tokens=tokens, model_tokens=model_tokens, t_model=t_model, guidance=guidance, pooled=model_pooled,
                            embeds=model_embeds, text_ids=text_ids, latent_ids=latent_ids, S_tgt=S_tgt, batch_size=batch_size,
                            do_true_cfg=do_true_cfg, true_cfg_scale=true_cfg_scale, jak=joint_attention_kwargs or {},
                            geom=(height, width, None if image is None else tuple(image.shape[-2:])),
                            dsigma=[self.scheduler.dsigma(i) for i in steps], inpaint=inpaint,
                            sigma_next=[self.scheduler.sigma_next(i) for i in steps] if inpaint else [],
                            # without a mask the fused step is the Euler update alone and reads neither x0 nor noise
                            x0=x0 if mask is not None else None, noise=noise if mask is not None else None, mask=mask,
                            step_cache=step_cache, cache_state=None, ab2=ab2, hist=hist, latent_state=latent_state, state=state)
        graphable = self.use_graph and callback_on_step_end is None and not joint_attention_kwargs and not self._interrupt
        if graphable and step_cache is not None and step_cache.adaptive:
            # the adaptive rule needs the step's two sums on the host before it can choose the step's launches
            if not self._said_adaptive_is_eager:
                print("step cache: the adaptive mode reads its measure back once per step, so this call runs the eager loop; "
                      "replay its decisions through the graph with StepCache(schedule=step_cache.computed_steps)")
                self._said_adaptive_is_eager = True
            graphable = False
        if graphable:
            tokens = self._denoise_graph(L)
        else:
            self._denoise(L, callback_on_step_end, timesteps)

        latents = tokens[:, :S_tgt]
        if output_type == "latent":
            image_out = latents.contiguous()
        else:
            z = self._unpack_latents(latents, height, width, self.vae_scale_factor).contiguous()
            vcfg = self.vae.config
            img = self.vae.decode(z, return_dict=False, pre_div=vcfg.scaling_factor, pre_add=vcfg.shift_factor)[0]
            if edit is not None and edit.overlay:
                # the result resampled into the box and blended over the picture's own bytes: they are kept, not decoded
                if edit.resample is not None:       # decode -> bytes -> antialiased to the box's size -> integer blend
                    x0, y0, x1, y1 = edit.box
                    res = ops.resample_u8(ops.image_to_u8(img.contiguous()), y1 - y0, x1 - x0, edit.resample)
                    image_out = ops.bytes_overlay(res, edit.pic, edit.alpha, edit.box).cpu().numpy()
                else:
                    image_out = ops.image_overlay(img.contiguous(), edit.pic, edit.alpha, edit.box).cpu().numpy()
                if output_type == "pil":
                    from PIL import Image
                    image_out = [Image.fromarray(a) for a in image_out]
            else:
                image_out = self.postprocess(img, output_type)
        if not return_dict:
            return (image_out,)
        # .latents: packed final latents (DP gather); .crop_box: (x0, y0, x1, y1) of a cropped masked edit, else None
        return FluxPipelineOutput(images=image_out, latents=latents, crop_box=edit.box if edit is not None and edit.crop else None)

    def _denoise(self, L, callback_on_step_end=None, timesteps=None):
        """Conditioning of all steps in one pass, then the loop (flux_pipeline.py:1052-1120) over the persistent buffers."""
        if hasattr(self.transformer, "prepare_conditioning"):  # all steps' modulation vectors in one pass
            self.transformer.prepare_conditioning(L.t_model, L.guidance, L.pooled)
        tokens, B = L.tokens, L.batch_size
        sc, st = L.step_cache, None
        if sc is not None:
            st = self._step_cache_state(L)
            sc.begin(len(L.dsigma))
        seed = True     # float32 state: the next step widens the bf16 token rows instead of reading the state
        for i in range(len(L.dsigma)):
            if self._interrupt:
                continue
            if L.do_true_cfg:
                L.model_tokens[:B].copy_(tokens)
                L.model_tokens[B:].copy_(tokens)
            fwd = dict(hidden_states=L.model_tokens, timestep=L.t_model[i], guidance=L.guidance,
                       pooled_projections=L.pooled, encoder_hidden_states=L.embeds,
                       txt_ids=L.text_ids, img_ids=L.latent_ids, joint_attention_kwargs=L.jak)
            if sc is None:
                noise_pred = self.transformer(**fwd, return_dict=False)[0]
            else:
                # two phases: embed (+ the measure), then the blocks or the cached residual; the adaptive rule's read of
                # state.sums (8 bytes) is the one host sync per step the mode needs
                self.transformer.step_cache_begin(st, **fwd)
                compute = sc.step(i, st.sums.tolist() if sc.adaptive and i > 0 else None)
                noise_pred = self.transformer.step_cache_end(st, compute)
            if L.do_true_cfg:
                noise_pred = ops.true_cfg(noise_pred[:B], noise_pred[B:], L.true_cfg_scale)
            self._solver_step(L, i, noise_pred, seed)
            seed = False
            if callback_on_step_end is not None:
                out = callback_on_step_end(self, i, timesteps[i], {"latents": tokens[:, :L.S_tgt]})
                if out and "latents" in out:
                    tokens[:, :L.S_tgt].copy_(out["latents"])
                    seed = True     # the callback's bf16 latents become the state at the next step
        if sc is not None:
            sc.block_passes = st.block_passes

    def _solver_step(self, L, i, noise_pred, seed):
        """Step i of the loop on the token rows, one launch: the rule (Euler or AB2) on the state type (bf16 rows or the float32
        state) the call chose, blended with the keep region of a masked edit.  ``seed``: the float32 state is not yet valid, and
        the step widens the bf16 token rows instead of reading it."""
        sigma_next = L.sigma_next[i] if L.inpaint else 0.0     # the keep region's noise level after the step
        c_v, c_h, use_hist = L.ab2[i] if L.ab2 is not None else (L.dsigma[i], 0.0, 0)
        if L.state is not None:   # either rule on the float32 state; the token rows receive its rounding to bf16
            ops.solver_step_f32(L.state, L.tokens, noise_pred, L.S_tgt, c_v, c_h, use_hist, 0 if seed else 1, L.hist, sigma_next,
                                L.x0, L.noise, L.mask)
        elif L.ab2 is not None:   # second-order multistep update (and hist <- this velocity), blended like the Euler one
            ops.ab2_step(L.tokens, noise_pred, L.hist, L.S_tgt, c_v, c_h, use_hist, sigma_next, L.x0, L.noise, L.mask)
        elif L.inpaint:           # Euler update where the mask is 1, the preserved picture at sigma[i+1] where it is 0
            ops.euler_inpaint_step(L.tokens, noise_pred, L.S_tgt, c_v, sigma_next, L.x0, L.noise, L.mask)
        else:
            ops.euler_step(L.tokens, noise_pred, L.S_tgt, c_v)

    def _step_cache_state(self, L):
        """The loop's cache state, reset for a new call: the graph route keeps one among the graph's own buffers
        (``L.cache_state``), the eager loop one per pipeline whose buffers last while the call shape does."""
        tr = self.transformer
        if not hasattr(tr, "step_cache_begin"):
            raise ValueError("`step_cache` needs a transformer with the two-phase forward (HipFluxTransformer2DModel)")
        st = L.cache_state if L.cache_state is not None else self._cache_state
        sc = L.step_cache
        if st is None or st.measure != sc.adaptive or st.mode != sc.measure:
            st = tr.step_cache_state(measure=sc.adaptive, mode=sc.measure)
        if L.cache_state is None:
            self._cache_state = st
        st.steps, st.block_passes, st.have_residual, st.f = 0, 0, False, None
        return st

    _GRAPH_INPUTS = ("tokens", "t_model", "guidance", "pooled", "embeds", "text_ids", "latent_ids", "x0", "noise", "mask")

    def _graph_key(self, L):
        """Everything a captured loop freezes: a call whose key differs captures anew."""
        # weights rewritten in place since the last forward (load_state_dict, a LoRA merge, an optimiser step): packed() checks
        # the source parameters' version stamps, re-packs the fused copies if needed and bumps the serial the key carries --
        # a replay never mixes fresh unfused weights with stale fused ones
        if hasattr(self.transformer, "packed"):
            self.transformer.packed()
        key = (tuple(L.tokens.shape), tuple(L.embeds.shape), tuple(L.latent_ids.shape), L.geom, L.do_true_cfg,
               float(L.true_cfg_scale), tuple(L.dsigma), L.guidance is None, L.S_tgt,
               getattr(self.transformer, "_pack_serial", 0), ops.launch_config_epoch(),
               # masked edits: the preserved picture, the noise and the mask are inputs (a new mask of the same shape replays);
               # their presence, the mask's batch form and the keep region's noise levels are frozen into the graph
               L.inpaint, None if L.mask is None else tuple(L.mask.shape), tuple(L.sigma_next),
               # step cache: which steps run the blocks, and which blocks a skipped step still runs, is frozen into the graph
               None if L.step_cache is None else (L.step_cache.schedule, L.step_cache.measure),
               # the latent state's type selects the step kernel
               L.latent_state,
               # the solver: its order and every step's coefficients are frozen into the graph's step launches
               1 if L.ab2 is None else 2, None if L.ab2 is None else tuple(L.ab2))
        return key

    def _denoise_graph(self, L):
        """The same work as ONE graph launch.  The captured kernels read and write fixed buffers, so the call's tensors
        are copied into the graph's own (a few MB); everything the host decides during an eager pass -- launch plans,
        cached RoPE tables, the rows of the prepared conditioning, the Euler step sizes -- is frozen into the graph and
        therefore part of its key.  Returns the token buffer the graph updates."""
        key = self._graph_key(L)
        cur = torch.cuda.current_stream()
        if self._loop_graph is None or self._loop_graph[0] != key:
            self._loop_graph = None
            G = SimpleNamespace(**vars(L))
            for n in self._GRAPH_INPUTS:
                t = getattr(L, n)
                setattr(G, n, None if t is None else t.clone())
            G.model_tokens = torch.empty_like(L.model_tokens) if L.do_true_cfg else G.tokens
            if L.hist is not None:          # the previous velocity is the graph's own buffer, not an input: step 0 never reads it
                G.hist = torch.empty_like(L.hist)
            if L.state is not None:         # so is the float32 state: every replay's first step seeds it from the tokens
                G.state = torch.empty_like(L.state)
            if L.step_cache is not None:    # the cache state (h0, the residual) belongs to the graph's own buffers
                G.cache_state = self.transformer.step_cache_state(measure=False, mode=L.step_cache.measure)
            side = torch.cuda.Stream(device=L.tokens.device)
            side.wait_stream(cur)
            with torch.cuda.stream(side):       # eager warm-up off the capture: kernel attributes, workspaces, RoPE cache
                self._denoise(G)
            cur.wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self._denoise(G)
            self._loop_graph = (key, G, graph)
        _, G, graph = self._loop_graph
        if L.step_cache is not None:        # a replay makes the decisions the capture froze: record them for this call's cache
            L.step_cache.begin(len(L.dsigma))
            L.step_cache.computed_steps = list(L.step_cache.schedule)
            L.step_cache.block_passes = G.cache_state.block_passes = len(L.step_cache.schedule)
        for n in self._GRAPH_INPUTS:
            t = getattr(L, n)
            if t is not None:
                getattr(G, n).copy_(t)
        graph.replay()
        # the graph's own buffer is overwritten by the next same-shape call: hand out a copy, as the eager path hands out
        # fresh tensors (results of consecutive calls -- a list of latents, the DP gather -- must stay distinct)
        return G.tokens.clone()

    @staticmethod
    def postprocess(image, output_type="pil"):
        """VaeImageProcessor.postprocess (flux_pipeline.py:1130); 'pil' / 'np_uint8' quantise on the GPU."""
        return image_processor.VaeImageProcessor.postprocess(image, output_type)
