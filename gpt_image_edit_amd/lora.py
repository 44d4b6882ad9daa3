"""LoRA adapters for the denoiser: parse, merge into the bf16 weights (one HIP launch per touched weight), rescale, unload.

The reference's ``FluxKontextPipeline`` is a ``FluxLoraLoaderMixin`` (``univa/utils/flux_pipeline.py:30,195``).  Here an
adapter is MERGED, never run as a side branch: ``W = bf16(W_base + sum_a s_a * B_a A_a)`` (``ops.lora_merge``,
``fk_lora_merge_bf16``), so an edit with adapters runs exactly the launches of a plain edit -- fused QKV, MXFP8, graph replay
and the step cache see ordinary weights.

Exactness rules
  * every merge computes from a bf16 clone of the untouched weight (``model._lora_base``), never from a merged one: rescaling,
    re-ordering, deleting and unloading are exact and idempotent; ``unload_lora()`` copies the clones back bit for bit;
  * a term's scale is ``weight x call scale x alpha / r`` (host doubles, rounded once to fp32); terms are added in the order
    of ``set_adapters`` (default: load order);
  * a weight is re-merged only when its tuple of (adapter, effective scale) changed since its last merge.

Training (``train_step.DenoiserTrainStep(model, lora=adapter_name)``) keeps that function: the forward and backward over a
model with a trainable adapter are launch for launch the training forward and backward on the merged weights, and the chain
rule through the merge, straight through its one bf16 rounding, gives the factors' gradients from the ``dW`` the backward
already computes: ``d_up = s dW down^T``, ``d_down = s up^T dW`` (``ops.lora_grad``, ``fk_lora_grad_bf16``), block by block, so
one block's ``dW`` is alive at a time.  AdamW runs on fp32 masters of the factors and rewrites the bf16 factors; the touched
weights are then marked stale (``lora_mark_stale``) and re-merged from their bases, one launch each.  ``add_lora_adapter``
creates an adapter (``up = 0``: the model is unchanged until the first step), ``lora_state_dict`` /
``pipe.save_lora_weights`` write it in the layout ``parse_lora_state`` reads.  The merged design still pays for the full wgrad
GEMM; it saves the fp32 optimiser state and the kept gradients of the full step and changes no forward or backward kernel.

Not built: text-encoder LoRA (the encoders are stock transformers models; such keys are reported as ignored), BFL / kohya
fused-qkv key formats, bias / norm deltas, more than ``FK_LORA_MAX_TERMS`` active adapters on one weight, ranks above
``FK_LORA_MAX_RANK`` = 128.  Training, not built: the ZeRO / data-parallel exchange of adapter gradients (``sharded=True``
with ``lora=`` is refused), micro-batch accumulation (every ``forward_backward`` overwrites the adapter gradients), a
side-branch backward that never forms ``dW`` (it would save the wgrad flops as well), an fp32-output wgrad in front of the
projection (``dW`` is rounded to bf16 first, as in the full step), bias / norm deltas, text-encoder adapters.

``state_dict()`` / ``save_pretrained`` of a model with active adapters hold the MERGED weights (diffusers after
``fuse_lora``); ``unload_lora()`` first to save the plain ones.
"""
import os
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import ops, param_tree
from .libfk import FK_LORA_MAX_RANK, FK_LORA_MAX_TERMS

BF16 = torch.bfloat16
IGNORED_PREFIXES = ("text_encoder.", "text_encoder_2.")


def _name_some(keys):
    keys = sorted(keys)
    return ", ".join(keys[:5]) + (f" ... ({len(keys)} keys)" if len(keys) > 5 else "")


def parse_lora_state(state_or_path, prefix="transformer."):
    """A diffusers / PEFT LoRA state (a dict, or the path of a safetensors file) -> ``(modules, ignored)``.

    ``modules``: ``{module name: SimpleNamespace(down=lora_A [r, in], up=lora_B [out, r], alpha=float, rank=r)}`` from
    ``<prefix><module>.lora_A.weight`` / ``.lora_B.weight`` and an optional scalar ``<prefix><module>.alpha`` (default: r).
    ``ignored``: the keys under ``text_encoder.`` / ``text_encoder_2.``.  Anything else -- a ``lora_B.bias``, norm or bias
    deltas, BFL / kohya key formats, a key outside ``prefix`` -- raises a ``ValueError`` naming up to five offending keys."""
    if isinstance(state_or_path, (str, os.PathLike)):
        from .checkpoint import _safetensors
        _, safe_open = _safetensors()
        state = OrderedDict()
        with safe_open(os.fspath(state_or_path), framework="pt", device="cpu") as f:
            for k in f.keys():
                state[k] = f.get_tensor(k)
    else:
        state = state_or_path
    ignored, bad, parts = [], [], {}
    for key, t in state.items():
        if key.startswith(IGNORED_PREFIXES):
            ignored.append(key)
            continue
        if not key.startswith(prefix):
            bad.append(key)
            continue
        name = key[len(prefix):]
        for suffix, slot in ((".lora_A.weight", "down"), (".lora_B.weight", "up"), (".alpha", "alpha")):
            if name.endswith(suffix):
                parts.setdefault(name[:-len(suffix)], {})[slot] = (key, t)
                break
        else:
            bad.append(key)
    if bad:
        raise ValueError("unsupported LoRA keys (supported: <prefix><module>.lora_A.weight / .lora_B.weight / .alpha with prefix "
                         f"{prefix!r}; no bias or norm deltas, no fused-qkv key formats): " + _name_some(bad))
    modules = OrderedDict()
    for mod, p in parts.items():
        if "down" not in p or "up" not in p:
            bad += [k for k, _ in p.values()]
            continue
        (kd, down), (ku, up) = p["down"], p["up"]
        if down.dim() != 2 or up.dim() != 2 or up.shape[1] != down.shape[0]:
            bad += [kd, ku]
            continue
        rank = down.shape[0]
        alpha = float(rank)
        if "alpha" in p:
            ka, a = p["alpha"]
            if torch.is_tensor(a) and a.numel() != 1:
                bad.append(ka)
                continue
            alpha = float(a)
        modules[mod] = SimpleNamespace(down=down, up=up, alpha=alpha, rank=rank)
    if bad:
        raise ValueError("incomplete or malformed LoRA entries (a module needs lora_A [r, in] and lora_B [out, r]; alpha is a "
                         "scalar): " + _name_some(bad))
    return modules, ignored


def parse_lora_arg(text):
    """``PATH[:WEIGHT]`` of the ``--lora`` command-line flag -> (path, weight)."""
    path, sep, w = text.rpartition(":")
    if sep and path:
        try:
            return path, float(w)
        except ValueError:
            pass
    return text, 1.0


def add_cli_arguments(parser):
    parser.add_argument("--lora", action="append", default=[], metavar="PATH[:WEIGHT]",
                        help="a diffusers / PEFT LoRA safetensors file for the denoiser, merged into its weights (repeatable)")
    parser.add_argument("--lora_scale", type=float, default=1.0, help="joint_attention_kwargs['scale'] of every call")


def load_cli_adapters(pipe, lora_args):
    """Load every ``--lora PATH[:WEIGHT]`` into ``pipe`` (adapter names lora0, lora1, ...) and activate them all."""
    names, weights = [], []
    for i, arg in enumerate(lora_args or []):
        path, w = parse_lora_arg(arg)
        pipe.load_lora_weights(path, adapter_name=f"lora{i}")
        names.append(f"lora{i}")
        weights.append(w)
    if names:
        pipe.set_adapters(names, weights)
    return names


class LoraMixin:
    """The adapter API of ``HipFluxTransformer2DModel`` (state: ``_lora_adapters``, ``_lora_active``, ``_lora_scale``,
    ``_lora_base``, ``_lora_merged`` -- plain attributes, no parameters, nothing in ``state_dict()``)."""

    def _lora_init(self):
        self._lora_adapters = OrderedDict()    # adapter name -> {parameter name: SimpleNamespace(up, down, alpha, rank)}
        self._lora_active = OrderedDict()      # adapter name -> weight, in merge order
        self._lora_scale = 1.0
        self._lora_base = {}                   # parameter name -> bf16 clone of the untouched weight (kept from its first merge)
        self._lora_merged = {}                 # parameter name -> ((adapter, effective scale), ...) of its last merge

    def load_lora_adapter(self, state, adapter_name="default", weight=1.0, prefix="transformer."):
        """Parse ``state`` (dict or safetensors path), check it against this model and activate it after the current
        adapters.  Returns the ignored (text-encoder) keys."""
        if self._train_packs:
            raise RuntimeError("load_lora_adapter: the model is under training (FluxBackward owns its packs); LoRA adapters "
                               "are an inference feature")
        if adapter_name in self._lora_adapters:
            raise ValueError(f"adapter {adapter_name!r} is already loaded: delete_adapters([{adapter_name!r}]) first")
        modules, ignored = parse_lora_state(state, prefix=prefix)
        bad, entries = [], {}
        for mod, e in modules.items():
            pname = mod + ".weight"
            if not self.has(pname) or self.p(pname).dim() != 2:
                bad.append(prefix + mod + ".lora_A.weight")
                continue
            N, K = self.p(pname).shape
            if tuple(e.up.shape) != (N, e.rank) or tuple(e.down.shape) != (e.rank, K) or not 1 <= e.rank <= FK_LORA_MAX_RANK:
                bad.append(prefix + mod + ".lora_B.weight")
                continue
            dev = self.p(pname).device
            entries[pname] = SimpleNamespace(up=e.up.to(device=dev, dtype=BF16).contiguous(),
                                             down=e.down.to(device=dev, dtype=BF16).contiguous(), alpha=e.alpha, rank=e.rank)
        if bad:
            raise ValueError(f"LoRA entries that do not fit the model (no such Linear, a shape other than the weight's [N, K], or "
                             f"a rank above {FK_LORA_MAX_RANK}): " + _name_some(bad))
        self._lora_adapters[adapter_name] = entries
        self._lora_active[adapter_name] = float(weight)
        try:
            self._lora_sync()
        except Exception:
            del self._lora_adapters[adapter_name], self._lora_active[adapter_name]
            raise
        return ignored

    # ---- training (train_step.DenoiserTrainStep(model, lora=adapter_name)) ---------------------------------------------------
    QKV_GROUPS = (("to_q", "to_k", "to_v"), ("add_q_proj", "add_k_proj", "add_v_proj"))

    def _lora_default_targets(self):
        """The Linear weights among ``training.trainable_names``: image-stream ``attn.to_q / to_k / to_v / to_out.0`` of the
        double blocks, ``attn.to_q / to_k / to_v`` of the single blocks."""
        from . import training
        leaves = ("attn.to_q.weight", "attn.to_k.weight", "attn.to_v.weight", "attn.to_out.0.weight")
        return [k[:-len(".weight")] for k in training.trainable_names(list(self._pmap.keys())) if k.endswith(leaves)]

    def _lora_resolve_targets(self, target_modules):
        """Module names (no ``.weight``) of ``target_modules``: full names or PEFT-style suffixes (``"to_q"``, ``"ff.net.2"``);
        the q / k / v of an attention named in part are completed to the three."""
        from .backward import FluxBackward
        mods = [k[:-len(".weight")] for k in self._pmap if k.endswith(".weight")]
        chosen, bad = [], []
        for t in target_modules:
            t = t[:-len(".weight")] if t.endswith(".weight") else t
            hit = [m for m in mods if m == t or m.endswith("." + t)]
            if not hit:
                bad.append(t)
            for m in hit:
                if not FluxBackward.producible(m + ".weight") or self.p(m + ".weight").dim() != 2:
                    bad.append(m + ".weight")
                elif m not in chosen:
                    chosen.append(m)
        if bad:
            raise ValueError("LoRA targets must be 2-D weights of transformer_blocks.* / single_transformer_blocks.* (the "
                             "backward produces no other weight gradient): " + _name_some(set(bad)))
        for m in list(chosen):
            stem, _, leaf = m.rpartition(".")
            for group in self.QKV_GROUPS:
                if leaf in group:
                    chosen += [f"{stem}.{g}" for g in group if f"{stem}.{g}" not in chosen]
        return sorted(chosen)

    def add_lora_adapter(self, adapter_name="default", rank=16, alpha=None, target_modules=None, seed=0, weight=1.0):
        """Create a trainable adapter instead of loading one and activate it after the current adapters: ``up`` (lora_B) = 0,
        ``down`` (lora_A) uniform in +-1/sqrt(K) (PEFT's ``kaiming_uniform_(a=sqrt(5))``) from a generator seeded with ``seed``,
        stored bf16 -- the merged weights stay the base weights bit for bit until the first optimiser step.  ``alpha``
        defaults to ``rank``.  ``target_modules``: module names or PEFT-style suffixes (``"to_q"``, ``"ff.net.2"``,
        ``"proj_mlp"``); default: the Linear weights among ``training.trainable_names``.  Every target must be a 2-D weight of
        ``transformer_blocks.*`` / ``single_transformer_blocks.*``.  ``to_q / to_k / to_v`` (and ``add_q_proj / add_k_proj /
        add_v_proj``) of one attention come as a group -- the backward computes their gradient as one [3D, D] GEMM -- so naming
        one of them selects the three.  Returns the parameter names touched."""
        if self._train_packs:
            raise RuntimeError("add_lora_adapter: the model is under training (FluxBackward owns its packs); add or load adapters "
                               "before the train step is built")
        if adapter_name in self._lora_adapters:
            raise ValueError(f"adapter {adapter_name!r} is already loaded: delete_adapters([{adapter_name!r}]) first")
        rank = int(rank)
        if not 1 <= rank <= FK_LORA_MAX_RANK:
            raise ValueError(f"rank {rank}: supported 1 to {FK_LORA_MAX_RANK}")
        mods = self._lora_default_targets() if target_modules is None else self._lora_resolve_targets(
            [target_modules] if isinstance(target_modules, str) else list(target_modules))
        if not mods:
            raise ValueError("add_lora_adapter: no target modules")
        alpha = float(rank if alpha is None else alpha)
        g = torch.Generator().manual_seed(int(seed))
        entries = OrderedDict()
        for mod in sorted(mods):
            w = self.p(mod + ".weight")
            N, K = w.shape
            lim = torch.tensor(K ** -0.5, dtype=torch.float32).to(BF16)
            if float(lim) > K ** -0.5:          # the largest bf16 number inside the interval: the rounding stays within +-1/sqrt(K)
                lim = (lim.view(torch.int16) - 1).view(BF16)
            down = ((torch.rand(rank, K, generator=g, dtype=torch.float32) * 2 - 1) / K ** 0.5).to(BF16).clamp(-lim, lim)
            entries[mod + ".weight"] = SimpleNamespace(up=torch.zeros(N, rank, device=w.device, dtype=BF16),
                                                       down=down.to(w.device).contiguous(), alpha=alpha, rank=rank)
        self._lora_adapters[adapter_name] = entries
        self._lora_active[adapter_name] = float(weight)
        try:
            self._lora_sync()
        except Exception:
            del self._lora_adapters[adapter_name], self._lora_active[adapter_name]
            raise
        return list(entries)

    def lora_mark_stale(self, adapter_name):
        """The factors of ``adapter_name`` were rewritten (an optimiser step): forget the last merge of the weights it touches, so
        the next ``_lora_sync()`` re-merges exactly those, one launch each, from their saved bases."""
        for pname in self._lora_adapters[adapter_name]:
            self._lora_merged.pop(pname, None)

    def lora_state_dict(self, adapter_name="default", prefix="transformer."):
        """The adapter in the diffusers / PEFT layout ``parse_lora_state`` reads: ``<prefix><module>.lora_A.weight`` (down),
        ``.lora_B.weight`` (up), ``.alpha`` -- the bf16 factors the model runs with, on the CPU."""
        if adapter_name not in self._lora_adapters:
            raise ValueError(f"lora_state_dict: not loaded: {adapter_name!r}")
        sd = OrderedDict()
        for pname, e in self._lora_adapters[adapter_name].items():
            mod = prefix + pname[:-len(".weight")]
            sd[mod + ".lora_A.weight"] = e.down.detach().cpu().clone()
            sd[mod + ".lora_B.weight"] = e.up.detach().cpu().clone()
            sd[mod + ".alpha"] = torch.tensor(float(e.alpha))
        return sd

    def lora_backward_weights(self, adapter_name):
        """The weights whose wgrad GEMMs a backward for ``adapter_name`` has to run: its targets, the q / k / v of an attention
        completed to the three (their gradient is gated on the first of them)."""
        names = set(self._lora_adapters[adapter_name])
        for pname in list(names):
            stem, _, leaf = pname[:-len(".weight")].rpartition(".")
            for group in self.QKV_GROUPS:
                if leaf in group:
                    names |= {f"{stem}.{g}.weight" for g in group}
        return names

    def set_adapters(self, names, weights=None):
        """Activate exactly ``names`` (a name or a list), in this order, with ``weights`` (default 1.0 each)."""
        names = [names] if isinstance(names, str) else list(names)
        if weights is None:
            weights = [1.0] * len(names)
        weights = [weights] * len(names) if isinstance(weights, (int, float)) else list(weights)
        if len(weights) != len(names) or len(set(names)) != len(names):
            raise ValueError("set_adapters: one weight per adapter name, names unique")
        missing = [n for n in names if n not in self._lora_adapters]
        if missing:
            raise ValueError(f"set_adapters: not loaded: {missing}")
        before = self._lora_active
        self._lora_active = OrderedDict((n, float(w)) for n, w in zip(names, weights))
        try:
            self._lora_sync()
        except Exception:
            self._lora_active = before
            raise

    def set_lora_scale(self, scale):
        """The call scale (``joint_attention_kwargs["scale"]``) of every active adapter; merged until another is asked for."""
        scale = float(scale)
        if scale != self._lora_scale:
            self._lora_scale = scale
            self._lora_sync()

    def delete_adapters(self, names):
        names = [names] if isinstance(names, str) else list(names)
        missing = [n for n in names if n not in self._lora_adapters]
        if missing:
            raise ValueError(f"delete_adapters: not loaded: {missing}")
        for n in names:
            del self._lora_adapters[n]
            self._lora_active.pop(n, None)
        self._lora_sync()
        if not self._lora_adapters:
            self._lora_base.clear()            # everything is back at its base (the sync above restored it)
            self._lora_merged.clear()

    def unload_lora(self):
        """Every touched weight back to its saved bits; adapters and clones freed."""
        self._lora_adapters.clear()
        self._lora_active.clear()
        self._lora_sync()
        self._lora_base.clear()
        self._lora_merged.clear()
        self._lora_scale = 1.0

    def active_adapters(self):
        return list(self._lora_active)

    def lora_loaded(self):
        return bool(self._lora_adapters)

    def _lora_wanted(self):
        """parameter name -> ((adapter, effective scale, entry), ...) of the active adapters, in merge order."""
        want = {}
        for name, weight in self._lora_active.items():
            for pname, e in self._lora_adapters[name].items():
                s = float(torch.tensor(weight * self._lora_scale * e.alpha / e.rank, dtype=torch.float32))
                want.setdefault(pname, []).append((name, s, e))
        over = sorted(p for p, ts in want.items() if len(ts) > FK_LORA_MAX_TERMS)
        if over:
            raise ValueError(f"more than {FK_LORA_MAX_TERMS} active adapters on one weight: " + _name_some(over))
        return want

    @torch.no_grad()
    def _lora_sync(self):
        """Bring every touched weight to the wanted (adapter, scale) tuple: one merge launch per weight whose tuple changed,
        each from the saved base.  Returns the number of launches."""
        want = self._lora_wanted()
        merges = 0
        for pname in sorted(set(want) | set(self._lora_merged)):
            terms = want.get(pname, ())
            key = tuple((a, s) for a, s, _ in terms)
            if self._lora_merged.get(pname, ()) == key:
                continue
            w = self.p(pname).data
            if pname not in self._lora_base:
                self._lora_base[pname] = w.detach().clone()
            base = self._lora_base[pname]
            if terms:
                ops.lora_merge(base, [(e.up, e.down, s) for _, s, e in terms], out=w)
                self._lora_merged[pname] = key
            else:
                w.copy_(base)
                self._lora_merged.pop(pname, None)
            merges += 1
        if merges:
            # the kernel writes through raw pointers: no torch version counter moves.  Every cache keyed on the parameters
            # (prepared conditioning, W^T copies) sees the epoch; the packs (fused QKV / modulation copies, MXFP8 copies)
            # are rebuilt by the next forward, which bumps _pack_serial: a captured loop graph is re-made
            param_tree.note_raw_write()
            self._packed = None
        return merges
