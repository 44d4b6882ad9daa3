"""Reference, fp32 emulation and error bounds of the Prodigy step (include/fk.h "Prodigy", csrc/prodigy.hip).

``Ref``: the step of the issue's specification in float64 over a dict of tensors, in the four phases the kernels have
(``begin`` / ``moments`` / ``update_d`` / ``apply``), so a test can hand the same scalars to the phase it checks.
``Emu``: the same phases with the element arithmetic in float32, every operation rounded on its own, in the kernels' order --
and, on request, with one of six deliberate mistakes.
``bounds_*``: what separates the two, derived from the operation order alone (u = 2^-24 per fp32 rounding; fma contraction only
removes roundings) and never from a kernel's output.  Hyper-parameters that cross the C ABI as ``float`` (betas, eps, weight
decay) are rounded to fp32 FIRST by ``kernel_hp``: reference and kernel then compute with the same numbers.
"""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53
TINY = 8 * 2.0 ** -149  # a few fp32 denormal spacings: an operation whose result underflows loses absolute, not relative, accuracy
MARGIN = 2.0            # the project's margin on derived bounds

DEFAULTS = dict(lr=1.0, betas=(0.9, 0.99), beta3=None, eps=1e-8, weight_decay=0.0, d0=1e-6, d_coef=1.0, growth_rate=float("inf"),
                decouple=True, use_bias_correction=True, safeguard_warmup=True)
MISTAKES = ("new_d_for_dlr", "no_beta3_decay", "abs_s_old", "dot_sign", "safeguard_swapped", "eps_unscaled")


def f32(x):
    return float(np.float32(x))


def resolve(hp=None):
    out = dict(DEFAULTS)
    out.update(hp or {})
    if out["beta3"] is None:
        out["beta3"] = math.sqrt(out["betas"][1])
    return out


def kernel_hp(hp=None):
    """The hyper-parameters as the kernels receive them: betas, eps and weight decay rounded to fp32 (beta3 after its sqrt)."""
    out = resolve(hp)
    out["betas"] = (f32(out["betas"][0]), f32(out["betas"][1]))
    for k in ("beta3", "eps", "weight_decay"):
        out[k] = f32(out[k])
    return out


def clip_coef(sumsq, max_grad_norm, grad_scale=1.0):
    """``adamw_kernel``'s coefficient arithmetic in fp32: grad_scale * min(1, max_norm / (grad_scale * sqrt(sumsq) + 1e-6))."""
    gs = np.float32(grad_scale)
    if sumsq is None:
        return float(gs)
    total = np.float32(math.sqrt(float(sumsq))) * gs
    return float(np.minimum(np.float32(max_grad_norm) / (total + np.float32(1e-6)), np.float32(1.0)) * gs)


class Ref:
    """float64.  ``params`` / gradients: dict name -> array-like; scalars are python floats."""
    dtype = np.float64

    def __init__(self, params, hp=None, mistake=None):
        self.hp = resolve(hp)
        self.mistake = mistake
        self.p = {k: np.array(v, dtype=self.dtype) for k, v in params.items()}
        self.p0 = {k: v.copy() for k, v in self.p.items()}
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.s = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.d = self.d_max = float(self.hp["d0"])
        self.d_numerator = self.d_denom = self.d_hat = self.dlr = 0.0
        self.k, self.skipped = 0, False
        self.sum_dot = self.sum_abs = 0.0

    def scalars(self):
        return dict(d=self.d, d_max=self.d_max, d_numerator=self.d_numerator, d_denom=self.d_denom, d_hat=self.d_hat, dlr=self.dlr,
                    k=self.k, skipped=self.skipped, sum_dot=self.sum_dot, sum_abs=self.sum_abs)

    def set_scalars(self, **kw):
        for k, v in kw.items():
            setattr(self, k, int(v) if k == "k" else (bool(v) if k == "skipped" else float(v)))

    # -- phases -------------------------------------------------------------------------------------------------------------
    def begin(self):
        hp = self.hp
        b1, b2 = hp["betas"]
        bc = math.sqrt(1.0 - b2 ** (self.k + 1)) / (1.0 - b1 ** (self.k + 1)) if hp["use_bias_correction"] else 1.0
        self.dlr = self.d * hp["lr"] * bc
        self._bc = bc
        if self.mistake != "no_beta3_decay":
            self.d_numerator *= hp["beta3"]
        self.sum_dot = self.sum_abs = 0.0
        self.skipped = False

    def _moment_factors(self):
        hp = self.hp
        b1, b2 = hp["betas"]
        safeguard = hp["safeguard_warmup"] != (self.mistake == "safeguard_swapped")
        return (self.d * (1.0 - b1), self.d * self.d * (1.0 - b2), (self.d / hp["d0"]) * (self.d if safeguard else self.dlr))

    def moments_one(self, name, graw, coef=1.0):
        """Step 2 for one tensor; ``graw`` the stored gradient, ``coef`` the clipping / grad_scale coefficient (``clip_coef``)."""
        hp = self.hp
        b1, b2 = hp["betas"]
        cm, cv, cs = self._moment_factors()
        p = self.p[name]
        g = np.asarray(graw, dtype=np.float64).reshape(p.shape) * coef
        if not hp["decouple"]:
            g = g + hp["weight_decay"] * p
        diff = self.p0[name] - p
        if self.mistake == "dot_sign":
            diff = -diff
        s_old = self.s[name]
        self.sum_dot += float(np.sum(g * diff))
        self.m[name] = b1 * self.m[name] + cm * g
        self.v[name] = b2 * self.v[name] + cv * g * g
        self.s[name] = hp["beta3"] * s_old + cs * g
        self.sum_abs += float(np.sum(np.abs(s_old if self.mistake == "abs_s_old" else self.s[name])))

    def moments(self, grads, coef=1.0):
        for name in sorted(grads):
            self.moments_one(name, grads[name], coef)

    def update_d(self):
        hp = self.hp
        d, d0 = self.d, hp["d0"]
        self.d_numerator += (d / d0) * self.dlr * self.sum_dot
        self.d_denom = self.sum_abs
        if self.d_denom == 0.0:
            self.skipped = True
            return
        self.d_hat = hp["d_coef"] * self.d_numerator / self.d_denom
        if d == d0:
            d = max(d, self.d_hat)
        self.d_max = max(self.d_max, self.d_hat)
        self.d = min(self.d_max, d * hp["growth_rate"])
        self.k += 1

    def apply_one(self, name):
        if self.skipped:
            return
        hp = self.hp
        dlr = self.dlr
        if self.mistake == "new_d_for_dlr":
            dlr = self.d * hp["lr"] * self._bc
        p = self.p[name]
        if hp["decouple"]:
            p = p + p * (-hp["weight_decay"] * dlr)
        deps = hp["eps"] if self.mistake == "eps_unscaled" else self.d * hp["eps"]
        self.p[name] = p - dlr * (self.m[name] / (np.sqrt(self.v[name]) + deps))

    def apply(self):
        for name in sorted(self.p):
            self.apply_one(name)

    def step(self, grads, coef=1.0):
        self.begin()
        self.moments(grads, coef)
        self.update_d()
        self.apply()


class Emu(Ref):
    """The kernels' arithmetic: scalars in python floats (= the device's double), per-tensor factors rounded to fp32 once, element
    operations in fp32 one rounding each, sums in double over the fp32 values (the order of a double sum is inside its bound)."""
    dtype = np.float32

    def moments_one(self, name, graw, coef=1.0):
        hp = self.hp
        F = np.float32
        b1, b2, b3, wd = F(hp["betas"][0]), F(hp["betas"][1]), F(hp["beta3"]), F(hp["weight_decay"])
        cm, cv, cs = (F(x) for x in self._moment_factors())
        p = self.p[name]
        g = np.asarray(graw, dtype=np.float32).reshape(p.shape) * F(coef)
        if not hp["decouple"]:
            g = g + wd * p
        diff = self.p0[name] - p
        if self.mistake == "dot_sign":
            diff = -diff
        s_old = self.s[name]
        self.sum_dot += float(np.sum(g.astype(np.float64) * diff.astype(np.float64)))
        self.m[name] = b1 * self.m[name] + cm * g
        self.v[name] = b2 * self.v[name] + (cv * g) * g
        self.s[name] = b3 * s_old + cs * g
        self.sum_abs += float(np.sum(np.abs(s_old if self.mistake == "abs_s_old" else self.s[name]).astype(np.float64)))

    def apply_one(self, name):
        if self.skipped:
            return
        hp = self.hp
        F = np.float32
        dlr = self.dlr
        if self.mistake == "new_d_for_dlr":
            dlr = self.d * hp["lr"] * self._bc
        p = self.p[name]
        if hp["decouple"]:
            p = p + p * F(-float(F(hp["weight_decay"])) * dlr)
        deps = F(float(F(hp["eps"])) if self.mistake == "eps_unscaled" else self.d * float(F(hp["eps"])))
        self.p[name] = p - F(dlr) * (self.m[name] / (np.sqrt(self.v[name]) + deps))


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def bounds_moments(p, p0, graw, m, v, s, d, dlr, hp, coef=1.0):
    """Per-element bounds of fp32 ``moments`` against float64 on the SAME inputs and scalars, and of the two sums.

    g = fl(graw * coef): 1 rounding, e_g = u |g|; not decoupled, g + fl(wd p): + u |wd p| (product) + u |g'| (sum).
    m = fl(fl(b1 m) + fl(fl32(cm) g)): u |b1 m| + 2u |cm g| + |cm| e_g + u |m'|   <=  u (2 |b1 m| + 3 |cm g|) + |cm| e_g
    v = fl(fl(b2 v) + fl(fl(fl32(cv) g) g)): u |b2 v| + 3u |cv g^2| + 2 |cv g| e_g + u |v'|  <=  u (2 |b2 v| + 4 |cv g^2|) + 2 |cv g| e_g
    s like m with cs.   The e_g^2 term of v is below u^2 |cv g^2| and is covered by the slack between 3 and 4.
    dot: the kernel multiplies in double the fp32 g by fl(p0 - p): per element |p0 - p| e_g + u |g| |p0 - p|, then the double
    accumulation n 2^-53 sum |terms|.  |s|: the kernel's double sum over ITS fp32 s against the same sum in float64:
    n 2^-53 sum |s| (``sum_abs_order``); against the float64 reference's s the per-element bounds of s add up (``sum_abs``)."""
    hp = resolve(hp)
    b1, b2 = hp["betas"]
    b3, wd = hp["beta3"], hp["weight_decay"]
    A = lambda x: np.asarray(x, dtype=np.float64).ravel()       # noqa: E731
    p, p0, graw, m, v, s = A(p), A(p0), A(graw), A(m), A(v), A(s)
    n = p.size
    cm, cv = d * (1.0 - b1), d * d * (1.0 - b2)
    cs = (d / hp["d0"]) * (d if hp["safeguard_warmup"] else dlr)
    g = graw * coef
    eg = U * np.abs(g)
    if not hp["decouple"]:
        eg = eg + U * np.abs(wd * p) + U * (np.abs(g) + np.abs(wd * p))
        g = g + wd * p
    eg = eg + TINY
    bm = U * (2 * np.abs(b1 * m) + 3 * np.abs(cm * g)) + abs(cm) * eg + TINY
    bv = U * (2 * np.abs(b2 * v) + 4 * np.abs(cv * g * g)) + 2 * np.abs(cv * g) * eg + TINY
    bs = U * (2 * np.abs(b3 * s) + 3 * np.abs(cs * g)) + abs(cs) * eg + TINY
    diff = p0 - p
    terms = np.abs(g * diff)
    s_new = np.abs(b3 * s + cs * g)
    dot = float(np.sum(np.abs(diff) * eg + U * terms) + (n + 512) * U64 * np.sum(terms))
    sum_abs_order = float((n + 512) * U64 * np.sum(s_new + bs))
    dot_order = float((n + 512) * U64 * np.sum(terms))          # two double sums of the SAME terms in different orders: twice this
    return dict(m=bm, v=bv, s=bs, dot=dot, dot_order=dot_order, sum_abs_order=sum_abs_order, sum_abs=float(np.sum(bs)) + sum_abs_order)


def bounds_apply(p, m, v, d_new, dlr, hp):
    """p1 = fl(p + fl(p fl32(wdf))): u |p wdf| (factor) + u |p wdf| (product) + u |p1|;  denom = fl(fl(sqrt v) + fl32(d eps)): every term
    positive, relative error <= 3u;  q = fl(m / denom): 4u;  t = fl(fl32(dlr) q): 6u;  p' = fl(p1 - t): + u |p'|, |p'| <= |p1| + |t|:
    u (2 |p wdf| + 2 |p1| + 8 |t|), the 8 leaving one u |t| for the second-order terms."""
    hp = resolve(hp)
    A = lambda x: np.asarray(x, dtype=np.float64).ravel()       # noqa: E731
    p, m, v = A(p), A(m), A(v)
    pw = np.zeros_like(p)
    p1 = p
    if hp["decouple"]:
        pw = p * (-hp["weight_decay"] * dlr)
        p1 = p + pw
    t = dlr * (m / (np.sqrt(v) + d_new * hp["eps"]))
    return U * (2 * np.abs(pw) + 2 * np.abs(p1) + 8 * np.abs(t)) + TINY


def bound_d_hat(d, dlr, d_numerator, d_denom, dot_bound, abs_bound, hp):
    """d_hat = d_coef N / D with N = N_prev + (d / d0) dlr dot and D = sum |s|: an error e_N = (d / d0) dlr dot_bound in the numerator and
    e_D = abs_bound in the denominator move the quotient by at most d_coef (e_N + |N / D| e_D) / (D - e_D) (plus a few double roundings)."""
    hp = resolve(hp)
    e_n = (d / hp["d0"]) * dlr * dot_bound
    if d_denom <= abs_bound:
        return float("inf")
    q = abs(d_numerator / d_denom)
    return hp["d_coef"] * (e_n + q * abs_bound) / (d_denom - abs_bound) + 8 * U64 * hp["d_coef"] * q
