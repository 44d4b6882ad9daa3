"""Command-line front end of the HIP path -- counterpart of the reference's ``univa/serve/cli.py``.

Same flags and defaults (``cli.py:271-283``), same helper names and semantics (``update_size`` :82-97,
``prepare_condition_images`` :99-116, ``load_pipe`` :58-76) and the same generation call (:239-248); what changes
is what sits behind ``pipe``: ``HipFluxTransformer2DModel`` + ``HipAutoencoderKL`` filled from the same checkpoints
(``gpt_image_edit_amd.checkpoint``).

Prompt understanding: the Qwen2.5-VL backbone and T5 / CLIP come from the installed
``transformers`` (reused as-is), wrapped by ``gpt_image_edit_amd.qwen_adaptor`` (task head, ``denoise_embeds`` forward,
HIP ``denoise_projector``) -- nothing is imported from the reference package.  ``--prompt_embeds FILE`` feeds the
generation half from saved embeddings instead (a ``torch.save``d dict with ``prompt_embeds`` [1,L,4096] and
``pooled_prompt_embeds`` [1,768]), which is also how the parity tests drive it offline.
"""
import argparse
import os

import numpy as np
import torch

from .. import checkpoint, flux_spec, lora
from ..anyres_util import dynamic_resize
from ..pipeline import FluxKontextPipeline
from ..scheduler import FlowMatchEulerDiscreteScheduler, FlowMatchMultistepScheduler
from .. import transformer
from ..transformer import HipFluxTransformer2DModel
from ..vae import HipAutoencoderKL

seed = 42  # cli.py:20-26 seeds everything with 42 and draws the edit's noise from Generator("cuda").manual_seed(seed)
generate_image_temp = "./generate_image_{}.png"


SOLVERS = {"euler": FlowMatchEulerDiscreteScheduler, "ab2": FlowMatchMultistepScheduler}


def add_solver_argument(parser):
    parser.add_argument("--solver", choices=tuple(SOLVERS), default="euler",
                        help="integrator of the denoise loop: euler -- the reference's first-order step; ab2 -- second-order "
                             "Adams-Bashforth on the same sigma schedule (one model call per step, fp32 sum, one bf16 rounding)")
    parser.add_argument("--latent_state", choices=("bf16", "fp32"), default="bf16",
                        help="the loop's latents between steps: bf16 -- rounded at every step, as the reference's loop does; "
                             "fp32 -- carried in a float32 buffer by either solver, the model still reads their bf16 rounding")


def solver_kwargs(args):
    """``--solver`` as ``load_pipe``'s ``solver`` (nothing for the default: the call ``load_pipe`` always got)."""
    solver = getattr(args, "solver", None) or "euler"
    return {} if solver == "euler" else {"solver": solver}


def latent_state_kwargs(args):
    """``--latent_state`` as the pipeline's ``latent_state`` (nothing for the default: the call the pipeline always got)."""
    state = getattr(args, "latent_state", None) or "bf16"
    return {} if state == "bf16" else {"latent_state": state}


RESAMPLE_CHOICES = ("nearest", "bilinear", "bicubic", "lanczos")


def add_resample_argument(parser):
    parser.add_argument("--resample", choices=RESAMPLE_CHOICES, default="nearest",
                        help="how input images (and, with --mask_crop_padding / --overlay, the result on its way back) are "
                             "resized: nearest -- the reference's tensor resize, point-sampled; bilinear / bicubic / lanczos -- "
                             "Pillow's antialiased 8-bit resize with that filter, byte for byte, in HIP (diffusers resizes PIL "
                             "inputs with lanczos)")


def resample_kwargs(args):
    """``--resample`` as the pipeline's ``resample`` (nothing for the default: the call the pipeline always got)."""
    name = getattr(args, "resample", None) or "nearest"
    return {} if name == "nearest" else {"resample": name}


def load_pipe(denoiser, flux_path, device, weight_format="bf16", solver="euler"):
    """``FluxKontextPipeline.from_pretrained(flux_path, transformer=denoiser, torch_dtype=bf16).to(device)``.

    ``denoiser``: a ``HipFluxTransformer2DModel``, or a checkpoint directory (a UniWorld model directory with
    ``denoise_tower.denoiser.*`` keys, cli.py:127, or a diffusers FLUX directory), or None = ``flux_path``'s own
    transformer.  Returns (pipe, tokenizers, text_encoders) like the reference; the T5/CLIP encoders are loaded
    with ``transformers`` when ``flux_path`` holds them, else the two lists contain None.  ``weight_format``: "bf16" or
    "mxfp8" (``HipFluxTransformer2DModel.set_weight_format``: opt-in MXFP8 block GEMMs, inference only).  ``solver``: "euler"
    or "ab2" -- the scheduler class the pipeline is built with (``SOLVERS``)."""
    if not isinstance(denoiser, HipFluxTransformer2DModel):
        src = denoiser or flux_path
        cfg = checkpoint.flux_transformer_config(flux_path) if os.path.isdir(os.path.join(flux_path, "transformer")) else None
        model = HipFluxTransformer2DModel(cfg, device=device)
        checkpoint.load_flux_transformer(model, src)
        denoiser = model
    denoiser.set_weight_format(weight_format)
    vae = HipAutoencoderKL(device=device)
    checkpoint.load_vae(vae, flux_path)
    sched = SOLVERS[solver](**checkpoint.scheduler_config(flux_path))
    tokenizers, text_encoders = [None, None], [None, None]
    try:  # reused as-is; absent offline
        from transformers import CLIPTextModel, CLIPTokenizer, T5EncoderModel, T5TokenizerFast
        if os.path.isdir(os.path.join(flux_path, "text_encoder")):
            tokenizers = [CLIPTokenizer.from_pretrained(flux_path, subfolder="tokenizer"),
                          T5TokenizerFast.from_pretrained(flux_path, subfolder="tokenizer_2")]
            text_encoders = [CLIPTextModel.from_pretrained(flux_path, subfolder="text_encoder", torch_dtype=torch.bfloat16).to(device),
                             T5EncoderModel.from_pretrained(flux_path, subfolder="text_encoder_2", torch_dtype=torch.bfloat16).to(device)]
    except Exception as e:  # pragma: no cover
        print(f"text encoders not loaded ({type(e).__name__}: {e}); pass --prompt_embeds")
    pipe = FluxKontextPipeline(denoiser, vae, sched, text_encoder=text_encoders[0], tokenizer=tokenizers[0],
                               text_encoder_2=text_encoders[1], tokenizer_2=tokenizers[1])
    return pipe, tokenizers, text_encoders


def update_size(i1, i2, anyres="any_11ratio", anchor_pixels=1024 * 1024):
    """Edit size for a turn (reference cli.py:82-97): with no input image a square of ``anchor_pixels``; otherwise the
    ``anyres`` bucket of the input's size -- of the MEAN width / height when two images are given."""
    from PIL import Image
    sizes = [Image.open(path).size for path in (i1, i2) if path]        # PIL: (width, height)
    if not sizes:
        side = int(anchor_pixels ** 0.5)
        return side, side
    mean_w = sizes[0][0] if len(sizes) == 1 else sum(w for w, _ in sizes) / len(sizes)
    mean_h = sizes[0][1] if len(sizes) == 1 else sum(h for _, h in sizes) / len(sizes)
    return dynamic_resize(int(mean_h), int(mean_w), anyres, anchor_pixels=anchor_pixels)


def prepare_condition_images(image_paths, device):
    """float32 [-1,1] condition tensor [N,3,H,W] exactly as the reference builds it (cli.py:99-116)."""
    from PIL import Image
    if not image_paths:
        return None
    cond = []
    for p in image_paths:
        img = Image.open(p).convert("RGB")
        t = torch.tensor(np.array(img), dtype=torch.float32) / 255.0
        cond.append((t.permute(2, 0, 1) - 0.5) / 0.5)
    return torch.stack(cond).to(device, dtype=torch.float32)


def prepare_condition_pixels(image_paths):
    """The same images as uint8 [N,H,W,3]: the pipeline then normalises / resizes / casts them in one HIP kernel
    (bit-identical to the float route; tests/test_hip_pixels.py)."""
    from PIL import Image
    if not image_paths:
        return None
    arrs = [np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8) for p in image_paths]
    return torch.from_numpy(np.stack(arrs))


def inpaint_kwargs(args):
    """``--mask`` / ``--strength`` as the pipeline's ``mask_image`` / ``strength`` (nothing when neither is given: the plain
    edit).  The mask is read as greyscale, white = repaint; the pipeline binarises it at 0.5 and resizes it."""
    from PIL import Image
    kw = {}
    if getattr(args, "mask", None):
        kw["mask_image"] = Image.open(args.mask).convert("L")
    if getattr(args, "strength", None) is not None and args.strength != 1.0:
        kw["strength"] = args.strength
    # the masked box at full model resolution, a feathered mask, the input's own bytes outside the repainted region: each is
    # passed only when asked for, so without them the call is the one the pipeline always got
    if getattr(args, "mask_crop_padding", None) is not None:
        kw["padding_mask_crop"] = args.mask_crop_padding
    if getattr(args, "mask_blur", None):
        kw["mask_blur"] = args.mask_blur
    if getattr(args, "overlay", False):
        kw["overlay"] = True
    return kw


def step_cache_kwargs(args):
    """``--step_cache_threshold`` / ``--step_cache_schedule`` / ``--step_cache_coefficients`` / ``--step_cache_measure`` as the
    pipeline's ``step_cache``
    (nothing when neither mode is given: every step runs the blocks).  A fresh ``StepCache`` per call."""
    from ..step_cache import from_args
    sc = from_args(getattr(args, "step_cache_threshold", None), getattr(args, "step_cache_schedule", None),
                   getattr(args, "step_cache_coefficients", None), getattr(args, "step_cache_measure", None))
    return {} if sc is None else {"step_cache": sc}


def lora_kwargs(args):
    """``--lora_scale`` as the pipeline's ``joint_attention_kwargs["scale"]`` (nothing without ``--lora``: the plain edit)."""
    if not getattr(args, "lora", None):
        return {}
    return {"joint_attention_kwargs": {"scale": getattr(args, "lora_scale", 1.0)}}


def add_step_cache_arguments(parser):
    parser.add_argument("--step_cache_threshold", type=float, default=None, metavar="F",
                        help="adaptive step cache: skip the MMDiT blocks while the accumulated relative L1 change of the first "
                             "block's modulated input stays below F (no default: which F is acceptable depends on the checkpoint)")
    parser.add_argument("--step_cache_schedule", type=str, default=None, metavar="0,1,3,...",
                        help="fixed step cache: the executed-step indices that run the blocks (must start with 0); sync-free, "
                             "goes through the graph route")
    parser.add_argument("--step_cache_coefficients", type=str, default=None, metavar="a0,a1,...",
                        help="with --step_cache_threshold: rescaling polynomial of the measure, lowest order first (default 0,1)")
    parser.add_argument("--step_cache_measure", choices=("input", "first_block"), default=None,
                        help="what the step cache measures and skips (default input): input -- the first block's modulated "
                             "input, every block skipped; first_block -- block 0 runs at every step, the change of what it adds "
                             "to the image stream is compared with F directly and the blocks behind it are skipped")


def generate_image(pipe, prompt_embeds, pooled_prompt_embeds, history_image_paths, new_h, new_w, args, fused_pixels=True):
    """The generation call of cli.py:236-248."""
    cond = prepare_condition_pixels(history_image_paths) if fused_pixels else prepare_condition_images(history_image_paths, pipe.device)
    return pipe(
        image=cond,
        prompt_embeds=prompt_embeds,
        pooled_prompt_embeds=pooled_prompt_embeds,
        height=new_h,
        width=new_w,
        num_inference_steps=args.num_inference_steps,
        guidance_scale=args.guidance_scale,
        generator=torch.Generator(device="cuda").manual_seed(seed),
        **inpaint_kwargs(args),
        **step_cache_kwargs(args),
        **lora_kwargs(args),
        **latent_state_kwargs(args),
        **resample_kwargs(args),
    ).images[0]


def run_t5_only(pipe, text_encoders, tokenizers, text, image1=None, image2=None, args=None):
    """One edit conditioned on T5 (256 tokens) + CLIP only, no VLM -- ``run_model_and_return_samples`` of the
    reference's ``univa/eval/imgedit/step1_gen_samples_T5_only.py:140-183``: size from ``update_size`` with
    ``anchor_pixels = height * width``, the first image resized to that size (PIL bilinear, which is what
    torchvision's ``Resize`` does for a PIL input) and normalised to [-1, 1], ``encode_prompt(..., 256, device, 1)``,
    then the pipeline call with its default generator."""
    from PIL import Image

    from ..prompt_embedding import encode_prompt
    new_h, new_w = update_size(image1, image2, "any_11ratio", anchor_pixels=args.height * args.width)
    pipeline_image = None
    if image1:
        cond = Image.open(image1).convert("RGB").resize((new_w, new_h), Image.BILINEAR)
        pipeline_image = torch.from_numpy(np.asarray(cond).copy()).unsqueeze(0)      # uint8 [1, H, W, 3]: fused HIP route
    with torch.no_grad():
        t5_prompt_embeds, pooled_prompt_embeds = encode_prompt(text_encoders, tokenizers, text, 256, pipe.device, 1)
    return pipe(
        image=pipeline_image,
        prompt_embeds=t5_prompt_embeds,
        pooled_prompt_embeds=pooled_prompt_embeds,
        height=new_h,
        width=new_w,
        num_inference_steps=args.num_inference_steps,
        guidance_scale=args.guidance_scale,
        num_images_per_prompt=getattr(args, "num_images_per_prompt", 1),
        **inpaint_kwargs(args),
        **step_cache_kwargs(args),
        **lora_kwargs(args),
        **latent_state_kwargs(args),
        **resample_kwargs(args),
    ).images


def build_parser():
    parser = argparse.ArgumentParser(description="Model and component paths")
    parser.add_argument("--model_path", type=str, required=True)
    parser.add_argument("--flux_path", type=str, required=True)
    parser.add_argument("--no_auto_hw", action="store_true")
    parser.add_argument("--height", type=int, default=1024)
    parser.add_argument("--width", type=int, default=1024)
    parser.add_argument("--num_inference_steps", type=int, default=28)
    parser.add_argument("--guidance_scale", type=float, default=3.5)
    parser.add_argument("--ocr_enhancer", action="store_true")
    parser.add_argument("--no_joint_with_t5", action="store_true")
    # additions of this front end
    parser.add_argument("--prompt_embeds", type=str, default=None,
                        help="torch-saved dict(prompt_embeds, pooled_prompt_embeds): skip the VLM / T5 / CLIP stage")
    parser.add_argument("--images", type=str, default="", help="comma-separated condition images (with --prompt_embeds)")
    parser.add_argument("--output", type=str, default=generate_image_temp.format(0))
    parser.add_argument("--t5_only", type=str, default=None, metavar="INSTRUCTION",
                        help="one edit from T5 + CLIP embeddings of INSTRUCTION only (no VLM), with --images")
    parser.add_argument("--weight_format", choices=("bf16", "mxfp8"), default="bf16",
                        help="block GEMM weights: bf16, or opt-in OCP MXFP8 (e4m3 + E8M0 per 32; inference only)")
    parser.add_argument("--mx_splitk", action="store_true",
                        help="mxfp8 only: let the long-K block GEMMs run as split-K pairs (FK_MX_SPLITK=1; default off)")
    parser.add_argument("--mx_fused_attn", action="store_true",
                        help="mxfp8 with FK_MX_FUSED_QUANT=1 only: the attention emits MXFP8 itself (FK_MX_FUSED_ATTN=1; default off)")
    parser.add_argument("--mask", type=str, default=None, metavar="PATH",
                        help="greyscale mask image, white = repaint, black = keep the first of --images bit for bit in "
                             "latent space (with --prompt_embeds / --t5_only)")
    parser.add_argument("--strength", type=float, default=1.0, metavar="F",
                        help="in (0, 1]: below 1 the edit starts from the re-noised input image instead of from noise and "
                             "runs the last F of the steps (with --prompt_embeds / --t5_only)")
    parser.add_argument("--mask_crop_padding", type=int, default=None, metavar="N",
                        help="with --mask: edit only the mask's bounding box, padded by N pixels and grown to the target's aspect, "
                             "at the full model resolution, and paste the result back into the input image")
    parser.add_argument("--mask_blur", type=float, default=0.0, metavar="F",
                        help="with --mask: feather the mask with a Gaussian of sigma F pixels (at most 64) before it is used")
    parser.add_argument("--overlay", action="store_true",
                        help="with --mask: return the input image's own bytes wherever the mask is black (implied by "
                             "--mask_crop_padding)")
    add_resample_argument(parser)
    add_step_cache_arguments(parser)
    add_solver_argument(parser)
    lora.add_cli_arguments(parser)
    return parser


def main(args):
    device = torch.device("cuda")
    if getattr(args, "mx_splitk", False):
        transformer.set_mx_splitk(True)
    if getattr(args, "mx_fused_attn", False):
        transformer.set_mx_fused_attn(True)
    if (getattr(args, "mask", None) or getattr(args, "strength", 1.0) != 1.0) and not (args.prompt_embeds or args.t5_only):
        raise SystemExit("--mask / --strength go with --prompt_embeds or --t5_only")
    if (getattr(args, "mask_crop_padding", None) is not None or getattr(args, "mask_blur", 0.0) or getattr(args, "overlay", False)) \
            and not getattr(args, "mask", None):
        raise SystemExit("--mask_crop_padding / --mask_blur / --overlay go with --mask")
    step_cache_kwargs(args)      # a bad threshold / schedule / coefficient list fails before the weights load
    pipe, tokenizers, text_encoders = load_pipe(args.model_path, args.flux_path, device,
                                                weight_format=getattr(args, "weight_format", "bf16"),
                                                **solver_kwargs(args))
    lora.load_cli_adapters(pipe, getattr(args, "lora", None))
    if args.prompt_embeds:
        blob = torch.load(args.prompt_embeds, map_location="cpu", weights_only=True)
        urls = [u.strip() for u in args.images.split(",") if u.strip()]
        new_h, new_w = args.height, args.width
        if urls and not args.no_auto_hw:
            new_h, new_w = update_size(urls[0], urls[1] if len(urls) > 1 else None, "any_11ratio",
                                       anchor_pixels=args.height * args.width)
        img = generate_image(pipe, blob["prompt_embeds"], blob["pooled_prompt_embeds"], urls, new_h, new_w, args)
        img.save(args.output)
        print(f"Assistant: generate image at {args.output}")
        return
    if args.t5_only:
        if text_encoders[0] is None or text_encoders[1] is None:
            raise SystemExit(f"--t5_only needs the text_encoder / text_encoder_2 folders under {args.flux_path}")
        urls = [u.strip() for u in args.images.split(",") if u.strip()] + [None, None]
        imgs = run_t5_only(pipe, text_encoders, tokenizers, args.t5_only, urls[0], urls[1], args)
        imgs[0].save(args.output)
        print(f"Assistant: generate image at {args.output}")
        return
    chat(args, pipe, tokenizers, text_encoders, device)


def smart_resize(height, width, factor=28, min_pixels=4 * 28 * 28, max_pixels=16384 * 28 * 28):
    """(height, width) the Qwen2-VL front end resizes an image to: both multiples of ``factor`` (= 2 x 14-pixel patches
    merged 2 x 2), area within [min_pixels, max_pixels], aspect kept as far as the rounding allows.  Restated from the
    published algorithm of ``qwen-vl-utils`` (``vision_process.smart_resize``; un-pinned third-party dependency of the
    reference, ``requirements.txt:34``, not installed here), which the reference applies through
    ``process_vision_info(conversation)`` (``univa/serve/cli.py:189``) with the per-image ``min_pixels = max_pixels =
    448 * 448`` of ``cli.py:172``."""
    import math
    if max(height, width) / min(height, width) > 200:
        raise ValueError(f"absolute aspect ratio must be smaller than 200, got {max(height, width) / min(height, width)}")
    h_bar = max(factor, round(height / factor) * factor)
    w_bar = max(factor, round(width / factor) * factor)
    if h_bar * w_bar > max_pixels:
        beta = math.sqrt((height * width) / max_pixels)
        h_bar = math.floor(height / beta / factor) * factor
        w_bar = math.floor(width / beta / factor) * factor
    elif h_bar * w_bar < min_pixels:
        beta = math.sqrt(min_pixels / (height * width))
        h_bar = math.ceil(height * beta / factor) * factor
        w_bar = math.ceil(width * beta / factor) * factor
    return h_bar, w_bar


def vision_inputs(conversation):
    """``process_vision_info(conversation)[0]`` of the reference's cli (:189): every image entry of the conversation, in
    order, opened as RGB and resized (PIL's default filter, bicubic) to ``smart_resize`` of its own size under the
    entry's ``min_pixels`` / ``max_pixels`` (or of the entry's ``resized_height`` x ``resized_width`` when it names them:
    ``univa/eval/gedit/step1_gen_samples.py:119-124``) -- so that a 448 x 448-pixel budget yields the 16 x 16 merged-patch grid
    (256 image tokens for a square image) whatever the processor's own defaults are.  None when there is no image."""
    from PIL import Image
    out = []
    for message in conversation:
        for c in message["content"]:
            if c.get("type") != "image":
                continue
            img = c["image"] if isinstance(c["image"], Image.Image) else Image.open(c["image"])
            img = img.convert("RGB")
            w, h = img.size
            if "resized_height" in c and "resized_width" in c:      # a forced size wins over the pixel budget (gedit generator)
                h, w = c["resized_height"], c["resized_width"]
            rh, rw = smart_resize(h, w, 28, c.get("min_pixels", 4 * 28 * 28), c.get("max_pixels", 16384 * 28 * 28))
            out.append(img.resize((rw, rh)))
    return out or None


def load_main_model_and_processor(model_path, device, min_pixels=448 * 448, max_pixels=448 * 448):
    """(model, task_head, processor) like reference cli.py:30-55, built from this package's adaptor: the stock
    Qwen2.5-VL weights of the UniWorld directory, its ``denoise_tower.denoise_projector.*`` on the HIP projector and
    ``task_head_final.pt``."""
    from transformers import AutoProcessor

    from ..projector import HipDenoiseProjector
    from ..qwen_adaptor import TaskHead, UnivaQwen2p5VL, load_vlm
    proj = HipDenoiseProjector(device=device)
    proj.load_state_dict(checkpoint.read_projector(model_path))
    model = UnivaQwen2p5VL(load_vlm(model_path, device), proj)
    task_head = TaskHead().to(device)
    task_head.load_state_dict(checkpoint.read_task_head(model_path))
    processor = AutoProcessor.from_pretrained(model_path, min_pixels=min_pixels, max_pixels=max_pixels)
    return model, task_head, processor


def chat(args, pipe, tokenizers, text_encoders, device):
    """The interactive loop of reference cli.py:118-267 (text and / or image URLs per turn; empty turn exits)."""
    from ..prompt_embedding import encode_prompt
    from ..qwen_adaptor import encode_edit_prompt
    model, task_head, processor = load_main_model_and_processor(args.model_path, device)
    conversation, history_image_paths, n_generated = [], [], 0
    print("Interactive UniWorld-V1 Chat (Exit if input is empty)")
    while True:
        txt = input("Text prompt (or press Enter to skip): ").strip()
        img_input = input("Image URLs (comma-separated, or press Enter to skip): ").strip()
        if not img_input and not txt:
            print("Exit.")
            return
        if args.ocr_enhancer:
            raise SystemExit("--ocr_enhancer needs the reference's OCR service (out of scope, SURVEY.md section 2)")
        content = [{"type": "text", "text": txt}] if txt else []
        urls = [u.strip() for u in img_input.split(",") if u.strip()]
        new_h, new_w = args.height, args.width
        for url in urls:
            content.append({"type": "image", "image": url, "min_pixels": 448 * 448, "max_pixels": 448 * 448})
            history_image_paths.append(url)
        if urls:
            new_h, new_w = update_size(urls[0], urls[1] if len(urls) > 1 else None, "any_11ratio",
                                       anchor_pixels=args.height * args.width)
        conversation.append({"role": "user", "content": content})
        chat_text = processor.apply_chat_template(conversation, tokenize=False, add_generation_prompt=True)
        chat_text = "<|im_end|>\n".join(chat_text.split("<|im_end|>\n")[1:])      # drop the system turn (cli.py:186)
        images = vision_inputs(conversation)                                        # process_vision_info (cli.py:189)
        inputs = processor(text=[chat_text], images=images, padding=True, return_tensors="pt").to(device)
        # The processor applies its own smart_resize to what process_vision_info already resized (a 600 x 800 input becomes
        # 364 x 504, below min_pixels, and is scaled up again to 392 x 532): the reference does exactly this double resize
        # silently (cli.py:189-196) and so does this loop -- the grid the model sees is the processor's.
        t5_embeds, pooled = encode_prompt(text_encoders, tokenizers, txt if not args.no_joint_with_t5 else "", 256, device, 1)
        turn = encode_edit_prompt(model, task_head, inputs, t5_embeds, joint_with_t5=not args.no_joint_with_t5)
        if turn["generate"]:
            image = generate_image(pipe, turn["prompt_embeds"], pooled, history_image_paths, new_h, new_w, args)
            img_url = generate_image_temp.format(n_generated)
            n_generated += 1
            image.save(img_url)
            conversation.append({"role": "assistant", "content": [{"type": "image", "image": img_url}]})
            history_image_paths.append(img_url)
            print(f"Assistant: generate image at {img_url}\n")
        else:
            generated = model.vlm.generate(**inputs, max_new_tokens=128)
            reply = processor.batch_decode([o[len(i):] for i, o in zip(inputs.input_ids, generated)],
                                           skip_special_tokens=True, clean_up_tokenization_spaces=False)[0]
            print(f"Assistant: {reply}\n")
            conversation.append({"role": "assistant", "content": [{"type": "text", "text": reply}]})


if __name__ == "__main__":
    main(build_parser().parse_args())
