"""CPU: the Prodigy reference of tests/prodigy_ref.py -- the pinned float64 table of the specification, the behaviour on a
quadratic, the fp32 emulation of the kernels' operation order inside the derived bounds, six deliberate mistakes outside them,
and the zero-gradient rule."""
import numpy as np
import pytest

import prodigy_ref as R

PIN_HP = dict(lr=1.0, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
P_START, TARGET = [0.5, -1.0, 0.25, 2.0], np.array([1.0, 1.0, -1.0, 0.0])
PINS = {
    "defaults": (dict(), [1e-6] * 4 + [1.197223943056e-06, 1.513531931796e-06, 1.940868238091e-06, 2.508317315680e-06],
                 [5.000096745485e-01, -9.999902381844e-01, 2.499902818174e-01, 1.999990180008e+00], (1.779963252172e-10, 7.096244327005e-05)),
    "no safeguard, no bias correction": (
        dict(safeguard_warmup=False, use_bias_correction=False),
        [1e-6] * 2 + [1.130134451123e-06, 1.978402654954e-06, 3.877048838221e-06, 7.569064214046e-06, 1.394341189182e-05, 2.496302731348e-05],
        [5.000524778958e-01, -9.999470498428e-01, 2.499472860363e-01, 1.999946734862e+00], None),
    "coupled decay": (dict(decouple=False),
                      [1e-6] * 4 + [1.187016950964e-06, 1.497186235811e-06, 1.916169123153e-06, 2.472833126892e-06], None, None),
}


def _close(a, b, rel=1e-9):
    return abs(a - b) <= rel * abs(b)


@pytest.mark.parametrize("name", sorted(PINS))
def test_pinned_table(name):
    flags, ds, p_end, num_den = PINS[name]
    ref = R.Ref({"w": P_START}, dict(PIN_HP, **flags))
    got = []
    for _ in range(8):
        ref.step({"w": ref.p["w"] - TARGET})
        got.append(ref.d)
    assert all(_close(a, b) for a, b in zip(got, ds)), got
    if p_end is not None:
        assert all(_close(a, b) for a, b in zip(ref.p["w"], p_end)), ref.p["w"]
    if num_den is not None:
        assert _close(ref.d_numerator, num_den[0]) and _close(ref.d_denom, num_den[1])
    assert ref.k == 8 and not ref.skipped


def test_quadratic_d_grows_and_the_loss_vanishes():
    """f = |w - t|^2 / 2 over 64 elements, start and target standard normal, with the Prodigy package's own settings (betas (0.9, 0.999),
    no bias correction, no safeguard): the run the specification describes (d from 1e-6 to about a third of the distance scale, loss
    to 0).  Why beta2 = 0.999 and not the project's 0.99: near the minimum the step is dlr * m / sqrt(v), and sqrt(v) forgets at
    beta2^(1/2) per step.  Over 300 steps 0.999^300 = 0.74 of the early, large gradients is still in v, so the steps shrink with the
    gradient and the loss falls geometrically; with 0.99 v forgets within ~100 steps, m / sqrt(v) returns to O(1) and the iterate
    rattles at a floor of ~1e-5 of the start -- Adam's constant-lr behaviour, not a property of the distance estimate under test.
    Bias correction multiplies dlr by sqrt(1 - beta2^k) / (1 - beta1^k) ~ 0.05 in the first steps, which alone keeps d at d0 past
    step 10."""
    rng = np.random.default_rng(0)
    target, start = rng.standard_normal(64), rng.standard_normal(64)
    ref = R.Ref({"w": start}, dict(lr=1.0, betas=(0.9, 0.999), use_bias_correction=False, safeguard_warmup=False))
    loss = lambda: 0.5 * float(np.sum((ref.p["w"] - target) ** 2))      # noqa: E731
    first, ds = loss(), [ref.d]
    for _ in range(300):
        ref.step({"w": ref.p["w"] - target})
        ds.append(ref.d)
    assert all(b >= a for a, b in zip(ds, ds[1:])), "d decreased"
    assert ds[10] > ds[0] == 1e-6, "d is still d0 after 10 steps"
    assert loss() < 1e-6 * first, (loss(), first)


def _pair(n, flags, seed, steps=6, mistake=None):
    """Reference and emulation run ``steps - 1`` steps together on the emulation's fp32 state, then the checked step: returns the inputs
    of that step, both results, and the scalars."""
    rng = np.random.default_rng(seed)
    hp = R.kernel_hp(dict(lr=1.0, weight_decay=0.01, d0=1e-3, **flags))          # d0 = 1e-3, six steps: d has left d0 in the checked step
    names = ("a", "b")
    start = {k: rng.standard_normal(n).astype(np.float32) for k in names}
    target = {k: rng.standard_normal(n).astype(np.float32) for k in names}
    emu = R.Emu(start, hp)
    grads = lambda e: {k: (e.p[k] - target[k]).astype(np.float32) for k in names}      # noqa: E731
    for _ in range(steps - 1):
        emu.step(grads(emu), coef=0.5)
    g = grads(emu)
    ref = R.Ref({k: emu.p[k] for k in names}, hp)
    for k in names:
        ref.p0[k], ref.m[k], ref.v[k], ref.s[k] = (x[k].astype(np.float64) for x in (emu.p0, emu.m, emu.v, emu.s))
    ref.set_scalars(**emu.scalars())
    before = {k: {a: getattr(emu, a)[k].copy() for a in ("p", "p0", "m", "v", "s")} for k in names}
    emu.mistake = mistake
    return hp, names, g, before, ref, emu


def _check(n, flags, seed, mistake=None):
    """True when the emulation's step lies inside every bound; the apply phase is compared on the emulation's scalars."""
    hp, names, g, before, ref, emu = _pair(n, flags, seed, mistake=mistake)
    ok = True
    ref.begin(), emu.begin()
    ok &= _close(emu.d_numerator, ref.d_numerator, 1e-12) if ref.d_numerator else emu.d_numerator == 0.0
    d, dlr = ref.d, ref.dlr
    ref.moments(g, 0.5), emu.moments(g, 0.5)
    dot_b = abs_b = 0.0
    for k in names:
        b = before[k]
        B = R.bounds_moments(b["p"], b["p0"], g[k], b["m"], b["v"], b["s"], d, dlr, hp, 0.5)
        for a in ("m", "v", "s"):
            ok &= bool(np.all(np.abs(getattr(emu, a)[k].astype(np.float64) - getattr(ref, a)[k]) <= R.MARGIN * B[a]))
        dot_b, abs_b = dot_b + B["dot"], abs_b + B["sum_abs"]
    ok &= abs(emu.sum_dot - ref.sum_dot) <= R.MARGIN * dot_b and abs(emu.sum_abs - ref.sum_abs) <= R.MARGIN * abs_b
    ref.update_d(), emu.update_d()
    ok &= abs(emu.d_hat - ref.d_hat) <= R.MARGIN * R.bound_d_hat(d, dlr, ref.d_numerator, ref.d_denom, dot_b, abs_b, hp)
    ok &= emu.k == ref.k
    ref.set_scalars(d=emu.d)                      # the same scalars for the second pass
    m_v = {k: (emu.m[k].copy(), emu.v[k].copy()) for k in names}
    for k in names:
        ref.m[k], ref.v[k] = (x.astype(np.float64) for x in m_v[k])
    ref.apply(), emu.apply()
    for k in names:
        Bp = R.bounds_apply(before[k]["p"], m_v[k][0], m_v[k][1], ref.d, ref.dlr, hp)
        ok &= bool(np.all(np.abs(emu.p[k].astype(np.float64) - ref.p[k]) <= R.MARGIN * Bp))
    return bool(ok)


FLAGS = [dict(), dict(decouple=False), dict(safeguard_warmup=False, use_bias_correction=False)]


@pytest.mark.parametrize("n", [1, 257, 4099])
@pytest.mark.parametrize("fi", range(len(FLAGS)))
def test_fp32_emulation_sits_inside_the_bounds(n, fi):
    assert _check(n, FLAGS[fi], seed=n + fi)


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_mistakes_sit_outside_the_bounds(mistake):
    assert len(R.MISTAKES) == 6
    # without bias correction and safeguard d moves in every step from the third on (the pinned table's second row), so the old and
    # the new d differ in the checked step; the swapped safeguard needs dlr != d, i.e. the bias correction
    flags = dict(safeguard_warmup=False, use_bias_correction=False) if mistake == "new_d_for_dlr" else {}
    assert _check(257, flags, seed=11), "the correct step must pass with these inputs"
    assert not _check(257, flags, seed=11, mistake=mistake), f"{mistake} went unnoticed"


def test_zero_gradient_leaves_p_d_and_k_alone():
    for cls in (R.Ref, R.Emu):
        opt = cls({"w": np.array(P_START, dtype=np.float32)}, R.kernel_hp(dict(PIN_HP)))
        zero = {"w": np.zeros(4, dtype=np.float32)}
        opt.step(zero)
        assert opt.skipped and opt.k == 0 and opt.d == 1e-6 and np.array_equal(opt.p["w"], np.array(P_START, dtype=opt.dtype))
        opt.step({"w": opt.p["w"] - TARGET.astype(opt.dtype)})
        assert not opt.skipped and opt.k == 1
        m = opt.m["w"].copy()
        p, d = opt.p["w"].copy(), opt.d
        opt.step(zero)                       # the moments keep their decay; |s| is non-zero now, so this step is NOT skipped
        assert not opt.skipped and opt.k == 2 and np.all(np.abs(opt.m["w"]) < np.abs(m))
        assert d == opt.d and not np.array_equal(p, opt.p["w"])


def test_reference_and_package_agree_on_slots_defaults_and_beta3():
    """The reference's scalar names are the state buffer's slots, its defaults the host's, and ``kernel_hp`` rounds beta3 as ``ops`` does."""
    from gpt_image_edit_amd import libfk, ops, zero
    assert tuple(R.Ref({}, None).scalars()) == libfk.FK_PRODIGY_SLOTS == zero.PRODIGY_SLOTS
    assert all(R.DEFAULTS[k] == v for k, v in zero.PRODIGY_DEFAULTS.items())
    for betas, beta3 in (((0.9, 0.99), None), ((0.9, 0.999), None), ((0.8, 0.95), 0.9)):
        assert R.kernel_hp(dict(betas=betas, beta3=beta3))["beta3"] == ops.prodigy_beta3(betas, beta3)
