"""The optimiser pass of the training step and its unsharded state.

``optimizer_pass`` is the ONE place that knows the kernel sequences (``csrc/train_kernels.hip``, ``csrc/prodigy.hip``): AdamW is
``adamw_step`` per segment; Prodigy is ``prodigy_begin``, ``prodigy_moments`` per segment, ``prodigy_update_d``, ``prodigy_apply`` per
segment.  A segment is whatever the caller updates in one launch: a tensor (``PerTensorState``, sorted names) or a rank's chunk of
a bucket (``zero.ShardedAdamW``, layout order, with the all-reduce between Prodigy's passes and the all-gather after every write
as hooks).  ``PerTensorState`` is the optimiser of ``DenoiserTrainStep`` without ``sharded=`` / ``data_parallel=``; it offers the
gradient intake of ``ShardedAdamW`` (``grad_target`` / ``written``) so that the LoRA projection has one sink.
"""
import torch

from . import ops

PRODIGY_SLOTS = ("d", "d_max", "d_numerator", "d_denom", "d_hat", "dlr", "k", "skipped", "sum_dot", "sum_abs")   # include/fk.h
PRODIGY_DEFAULTS = dict(beta3=None, d0=1e-6, d_coef=1.0, growth_rate=float("inf"), use_bias_correction=True,
                        safeguard_warmup=True, decouple=True)     # the reference config's (configuration_denoise.py:49-55)


def resolve_optimizer(optimizer, lr, prodigy):
    """(optimizer, lr, Prodigy hyper-parameters or None) after the defaults and refusals of the training seam
    (train_denoiser.py:595-624): ``lr=None`` is 1e-6 for AdamW and 1.0 for Prodigy, Prodigy wants ``lr`` around 1."""
    if optimizer not in ("adamw", "prodigy"):
        raise ValueError(f"optimizer must be 'adamw' or 'prodigy', got {optimizer!r}")
    if optimizer == "adamw":
        if prodigy is not None:
            raise ValueError("prodigy= holds Prodigy's hyper-parameters; the optimiser is 'adamw'")
        return optimizer, (1e-6 if lr is None else lr), None
    lr = 1.0 if lr is None else lr
    if lr <= 0.1:
        raise ValueError(f"optimizer='prodigy' estimates the step size itself and wants lr around 1.0; lr = {lr} (<= 0.1) would "
                         "scale that estimate down")
    hp = dict(PRODIGY_DEFAULTS)
    unknown = sorted(set(prodigy or {}) - set(hp))
    if unknown:
        raise ValueError("prodigy=: unknown keys " + ", ".join(unknown) + "; known: " + ", ".join(sorted(hp)))
    hp.update(prodigy or {})
    if not hp["d0"] > 0 or not hp["d_coef"] > 0 or not hp["growth_rate"] > 1.0:
        raise ValueError("prodigy=: d0 and d_coef must be positive and growth_rate above 1")
    if hp["beta3"] is not None and not 0.0 <= hp["beta3"] < 1.0:
        raise ValueError("prodigy=: beta3 must lie in [0, 1)")
    return optimizer, lr, hp


def optimizer_pass(k, segments, step, hp, prodigy, pstate, pws, sumsq, max_grad_norm, grad_scale=1.0, reduce_sums=None,
                   after_write=None):
    """One optimiser step over the segments ``(master, grad, exp_avg, exp_avg_sq, s, p0, param_bf16)`` (``s`` / ``p0`` None for
    AdamW), with the kernels of ``k`` looked up at call time.  ``segments()`` returns an iterator over them -- a generator function,
    so that a segment is put together right before its launch and that host work hides under the kernels already queued (a list
    built up front cost the per-tensor AdamW pass about 1 ms at 608 tensors, profiles/train_step_refactor_ab.json); Prodigy walks it twice.  ``hp``: lr, betas, eps, weight_decay; ``prodigy``: Prodigy's
    hyper-parameters, None = AdamW; ``pstate`` / ``pws``: its scalar buffer and workspace.  ``sumsq`` is the squared norm of the
    gradient SUMS and ``grad_scale`` what still multiplies them; ``max_grad_norm=None``: no clipping.  Prodigy's two running sums
    accumulate on the device in segment order.  ``reduce_sums(two fp64 sums)`` runs between the moments pass and
    ``prodigy_update_d`` (the sum over the ranks); ``after_write(i)`` right after segment i's parameters were written."""
    clip = dict(grad_sumsq=sumsq if max_grad_norm is not None else None,
                max_grad_norm=max_grad_norm if max_grad_norm is not None else 0.0, grad_scale=grad_scale)
    if prodigy is not None:
        k.prodigy_begin(pstate, hp["lr"], hp["betas"], prodigy["beta3"], prodigy["use_bias_correction"])
        for master, grad, m, v, s, p0, _ in segments():
            k.prodigy_moments(master, p0, grad, m, v, s, pstate, betas=hp["betas"], beta3=prodigy["beta3"],
                              weight_decay=hp["weight_decay"], d0=prodigy["d0"], decouple=prodigy["decouple"],
                              safeguard_warmup=prodigy["safeguard_warmup"], ws=pws, **clip)
        if reduce_sums is not None:
            reduce_sums(pstate[PRODIGY_SLOTS.index("sum_dot"): PRODIGY_SLOTS.index("sum_abs") + 1])
        k.prodigy_update_d(pstate, prodigy["d0"], prodigy["d_coef"], prodigy["growth_rate"])
    for i, (master, grad, m, v, _, _, param) in enumerate(segments()):
        if prodigy is not None:
            k.prodigy_apply(master, m, v, pstate, eps=hp["eps"], weight_decay=hp["weight_decay"], decouple=prodigy["decouple"],
                            param_bf16=param)
        else:
            k.adamw_step(master, grad, m, v, step, param_bf16=param, **clip, **hp)
        if after_write is not None:
            after_write(i)


class PerTensorState:
    """AdamW / Prodigy on fp32 masters, one launch per tensor over the sorted names; everything is created lazily.

    ``param``: name -> bf16 parameter (anything with ``.data``, ``.shape``, ``.device``; a bare tensor will do).  ``state[name]`` is
    ``(master, exp_avg, exp_avg_sq)``, for Prodigy ``(master, m, v, s, p0)``, created at the first step that sees ``name`` from the
    parameter's value at that moment.  ``pstate`` (Prodigy: the fp64 scalar buffer on the device, include/fk.h FK_PRODIGY_*) does
    not exist before the first step."""

    def __init__(self, param, optimizer="adamw", lr=None, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0,
                 prodigy=None):
        self.param = param
        self.optimizer, lr, self.prodigy = resolve_optimizer(optimizer, lr, prodigy)
        self.hp = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.max_grad_norm = max_grad_norm
        self.state, self.pstate, self._pws, self.step_count = {}, None, None, 0
        self._grads = {}       # name -> persistent fp32 gradient buffer (``grad_target``)

    def _state(self, name):
        st = self.state.get(name)
        if st is None:
            p = self.param(name)
            st = (p.detach().float().contiguous(), torch.zeros(p.shape, device=p.device, dtype=torch.float32),
                  torch.zeros(p.shape, device=p.device, dtype=torch.float32))
            if self.prodigy is not None:        # + s and the point the distance estimate is measured from
                st = st + (torch.zeros(p.shape, device=p.device, dtype=torch.float32), st[0].clone())
            self.state[name] = st
        return st

    def grad_target(self, name):
        """(fp32 buffer of the parameter's shape, False): the intake of ``zero.ShardedAdamW.grad_target`` without accumulation --
        the kernel overwrites the buffer, which persists over the steps."""
        buf = self._grads.get(name)
        if buf is None:
            p = self.param(name)
            buf = self._grads[name] = torch.empty(p.shape, device=p.device, dtype=torch.float32)
        return buf, False

    def written(self, names):
        pass

    @torch.no_grad()
    def step(self, grads):
        """Global-norm clipping + the optimiser pass over the sorted names of ``grads``; returns the squared norm (fp64 [1]).
        Nothing is read back: Prodigy's ``d``, the step count of its bias correction and the zero-gradient rule are device-side."""
        names = sorted(grads)
        gs = [grads[k].contiguous() for k in names]
        sumsq = ops.sumsq(gs)
        self.step_count += 1
        if self.prodigy is not None and self.pstate is None:
            self.pstate = ops.prodigy_init_state(self.prodigy["d0"], gs[0].device)
        if self.prodigy is not None and self._pws is None:
            self._pws = ops.prodigy_ws(gs[0].device)

        def segments():
            for k, g in zip(names, gs):
                master, m, v, *sp = self._state(k)
                yield (master, g, m, v, *(sp or (None, None)), self.param(k).data)
        optimizer_pass(ops, segments, self.step_count, self.hp, self.prodigy, self.pstate, self._pws, sumsq, self.max_grad_norm)
        return sumsq

    def prodigy_state(self):
        if self.pstate is None:                 # before the first step: no buffer yet
            d0 = float(self.prodigy["d0"])
            return dict(zip(PRODIGY_SLOTS, [d0, d0] + [0.0] * 4 + [0, False, 0.0, 0.0]))
        return ops.prodigy_state(self.pstate)

    def state_dict(self):
        sd = dict(step=self.step_count, state={k: tuple(t.detach().cpu().clone() for t in st) for k, st in self.state.items()})
        if self.prodigy is not None:            # an AdamW state keeps exactly the keys it had
            hp = self.hp
            sd.update(optimizer="prodigy", hp=dict(self.prodigy, lr=hp["lr"], betas=tuple(hp["betas"]), eps=hp["eps"],
                                                   weight_decay=hp["weight_decay"]),
                      scalars=None if self.pstate is None else self.pstate.detach().cpu().clone())
        return sd

    @torch.no_grad()
    def load_state_dict(self, sd):
        """Restores the state and rewrites the bf16 parameters from the fp32 masters."""
        self.step_count = int(sd["step"])
        self.state = {}
        for k, st in sd["state"].items():
            p = self.param(k)
            if len(st) != (3 if self.prodigy is None else 5):
                raise ValueError(f"{k}: {len(st)} state tensors do not fit optimizer={self.optimizer!r}")
            self.state[k] = tuple(t.to(p.device) for t in st)
            p.data.copy_(self.state[k][0])
        if self.prodigy is not None:
            self.pstate = None if sd["scalars"] is None else sd["scalars"].to(p.device)     # scalars exist only after a step, so does a state
