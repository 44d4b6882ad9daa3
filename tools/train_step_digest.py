"""sha256 digests of a fixed training sequence in all eight combinations of state kind and optimiser (development aid).

    python tools/train_step_digest.py --out digests.json [--package DIR]

For a change that must leave every launch of the training step as it was: run it on both trees and compare the files.  The
configuration is the one of tests/test_hip_lora_train_step.py (its ``_model``, ``_batch`` and ``_random_adapter``: full width, one
double + one single block, 16 x 16 latents, 64 text tokens).  Per kind (``per_tensor``, ``lora``, ``sharded``, ``lora_dp``) and
optimiser (``adamw``, ``prodigy``):

  1. one step;  2. two ``forward_backward`` calls, then the optimiser step (a further micro-batch where the kind accumulates, else
  the second call replaces the first);  3. one ``forward_backward`` and ``discard()``;  4. a third step;  5. ``state_dict()`` loaded
  into a freshly built step on a freshly built model, and one more step there.

Digested: every loss and returned ``grad_sumsq``, every trainable parameter at the end, every tensor of the final ``state_dict()``
in sorted key order, and the Prodigy scalars.  ``--package DIR``: import ``gpt_image_edit_amd`` from DIR instead of this tree (a copy
of another commit's python files; ``FK_LIB_PATH`` then names the built library).
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
KINDS = dict(per_tensor={}, lora=dict(lora="t"), sharded=dict(sharded=True), lora_dp=dict(lora="t", data_parallel=True))


def sha(t):
    t = t.detach().cpu().contiguous()
    return hashlib.sha256(str((t.dtype, tuple(t.shape))).encode() + t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def flatten(x, prefix, out):
    """Every tensor below ``x`` (dicts in sorted key order, tuples and lists by index); other leaves by their ``repr``."""
    if isinstance(x, torch.Tensor):
        out[prefix] = sha(x)
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            flatten(x[k], f"{prefix}/{k}", out)
    elif isinstance(x, (tuple, list)) and any(isinstance(v, (torch.Tensor, dict, tuple, list)) for v in x):
        for i, v in enumerate(x):
            flatten(v, f"{prefix}/{i}", out)
    else:
        out[prefix] = repr(x)
    return out


def run(kind, optimizer, T):
    from gpt_image_edit_amd.train_step import DenoiserTrainStep

    def build():
        model = T._model()
        if "lora" in KINDS[kind]:
            mods = [p[:-len(".weight")] for p in T.DEFAULT_TARGETS]
            model.load_lora_adapter(T._random_adapter(model, mods, 5, 10, seed=6), adapter_name="t")
        kw = dict(KINDS[kind], optimizer=optimizer, weight_decay=0.01)
        return DenoiserTrainStep(model, lr=LR if optimizer == "adamw" else None, **kw)
    out = {}

    def note(tag, res):
        out[f"{tag}/loss"], out[f"{tag}/grad_sumsq"] = sha(res["loss"]), sha(res["grad_sumsq"])
    ts = build()
    note("1", ts.step(**T._batch(seed=0)))
    ts.forward_backward(**T._batch(seed=1))
    loss, grads, _ = ts.forward_backward(**T._batch(seed=2))
    note("2", dict(loss=loss, grad_sumsq=ts.optimizer_step(grads)))
    out["3/loss"] = sha(ts.forward_backward(**T._batch(seed=3))[0])
    ts.discard()
    note("4", ts.step(**T._batch(seed=4)))
    sd = ts.state_dict()
    ts2 = build()
    ts2.load_state_dict(sd)
    note("5", ts2.step(**T._batch(seed=5)))
    for k in sorted(ts2.trainable_names()):
        out[f"param/{k}"] = sha(ts2._param(k).data)
    flatten(ts2.state_dict(), "state_dict", out)
    if optimizer == "prodigy":
        out["prodigy_state"] = json.dumps(ts2.prodigy_state(), sort_keys=True)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--package", default=ROOT, help="directory that holds the gpt_image_edit_amd package to run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    sys.path[:0] = [os.path.abspath(args.package), os.path.join(ROOT, "tests"), ROOT]
    import gpt_image_edit_amd
    import test_hip_lora_train_step as T
    print("package:", os.path.dirname(os.path.abspath(gpt_image_edit_amd.__file__)), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), runs={})
    for kind in KINDS:
        for optimizer in ("adamw", "prodigy"):
            res["runs"][f"{kind}/{optimizer}"] = run(kind, optimizer, T)
            print(kind, optimizer, len(res["runs"][f"{kind}/{optimizer}"]), "digests", flush=True)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
