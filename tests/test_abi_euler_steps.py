"""CPU test of the boundary of the three Euler-side step entries (the pattern of tests/test_abi_solver_state.py):
fk_euler_step_bf16, fk_euler_inpaint_step_bf16 and fk_scale_noise_bf16 are declared in include/fk.h, exported, and bound argument
by argument -- and every refusal is made on the host before anything is launched, so its error string, and the order in which the
conditions are tested, can be read here, without a GPU, from calls that pass made-up addresses."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fk_euler_step_bf16": ["x", "x_batch_stride", "v", "v_batch_stride", "B", "S_tgt", "C", "dsigma", "stream"],
    "fk_euler_inpaint_step_bf16": ["x", "x_batch_stride", "v", "v_batch_stride", "x0", "x0_batch_stride", "noise",
                                   "noise_batch_stride", "mask", "mask_batch_stride", "B", "S_tgt", "C", "dsigma", "sigma_next",
                                   "stream"],
    "fk_scale_noise_bf16": ["x0", "x0_batch_stride", "noise", "noise_batch_stride", "out", "out_batch_stride", "B", "S_tgt", "C",
                            "sigma", "stream"],
}
POINTERS = ("x", "v", "x0", "noise", "mask", "out", "stream")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def _lib():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return libfk.load()


@pytest.mark.parametrize("name", list(ARGS))
def test_symbol_is_declared_exported_and_bound(name):
    from gpt_image_edit_amd import libfk
    lib = _lib()
    declared = set(re.findall(r"\b(fk_[a-z0-9_]+)\s*\(", _header()))
    assert name in declared, f"{name} is not declared in include/fk.h"
    assert hasattr(lib, name), f"{name} is not exported by libfk"
    assert name in libfk.SIGNATURES, f"{name} has no ctypes signature"


@pytest.mark.parametrize("name", list(ARGS))
def test_signature_is_the_declared_one(name):
    """Argument by argument: the C declaration's parameter types against the ctypes prototype."""
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "fk_stream_t": libfk.c_vp, "int64_t": libfk.c_i64,
             "int32_t": libfk.c_i32, "float": libfk.c_f32}
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", _header())
    assert m, name
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(re.search(r"\b(\w+)$", arg).group(1))
        want.append(kinds[re.sub(r"\s*\b\w+$", "", arg)])              # drop the parameter's name
    res, args = libfk.SIGNATURES[name]
    assert res is libfk.c_i32 and args == want, (args, want)
    assert names == ARGS[name]


# ---- the refusals: host checks before any launch ----------------------------------------------------------------------------------
A = 0x10000          # made-up addresses, 16-byte aligned and distinct; a refused call dereferences none of them
GOOD = dict(x=A, x_batch_stride=1024, v=2 * A, v_batch_stride=1024, x0=3 * A, x0_batch_stride=512, noise=4 * A,
            noise_batch_stride=512, mask=5 * A, mask_batch_stride=32, out=6 * A, out_batch_stride=512, B=2, S_tgt=8, C=64,
            dsigma=-0.05, sigma_next=0.5, sigma=0.5, stream=0)
SIZES, ALIGN = "bad sizes", "alignment"
NEEDS, ALIGN_ROWS, ALIGN_MASK = "a mask needs x0 and noise", "alignment of x0 / noise", "alignment of the mask"
_BAD_DIMS = [dict(B=0), dict(S_tgt=0), dict(C=0), dict(B=-1), dict(S_tgt=-3), dict(C=-8), dict(C=4), dict(C=12)]
_XV = [(dict(x=0), SIZES), (dict(v=0), SIZES)] + [(d, SIZES) for d in _BAD_DIMS] + [
    (dict(x=A + 8), ALIGN), (dict(v=2 * A + 8), ALIGN), (dict(x_batch_stride=1028), ALIGN), (dict(v_batch_stride=1028), ALIGN),
    # two violations: the sizes are tested before the alignment
    (dict(C=12, x=A + 8), SIZES), (dict(B=0, v_batch_stride=1028), SIZES), (dict(v=0, x=A + 8), SIZES)]
REFUSALS = {
    "fk_euler_step_bf16": _XV,
    "fk_euler_inpaint_step_bf16": _XV + [
        (dict(x0=0), NEEDS), (dict(noise=0), NEEDS), (dict(x0=0, noise=0), NEEDS),
        (dict(x0=3 * A + 8), ALIGN_ROWS), (dict(noise=4 * A + 8), ALIGN_ROWS), (dict(x0_batch_stride=516), ALIGN_ROWS),
        (dict(noise_batch_stride=516), ALIGN_ROWS), (dict(mask=5 * A + 4), ALIGN_MASK), (dict(mask_batch_stride=2), ALIGN_MASK),
        # two violations: sizes, then x / v, then the presence of x0 / noise, then their alignment, then the mask's;
        # x and v are tested before the mask is looked at, so they are refused without one too
        (dict(C=12, x0=0), SIZES), (dict(C=4, mask=5 * A + 4), SIZES), (dict(x=A + 8, x0=0), ALIGN),
        (dict(v_batch_stride=1028, mask=5 * A + 4), ALIGN), (dict(x=A + 8, x0_batch_stride=516), ALIGN),
        (dict(x0=0, noise=4 * A + 8), NEEDS), (dict(noise=0, mask=5 * A + 4), NEEDS), (dict(x0=0, mask_batch_stride=2), NEEDS),
        (dict(x0=3 * A + 8, mask=5 * A + 4), ALIGN_ROWS), (dict(noise_batch_stride=516, mask_batch_stride=2), ALIGN_ROWS),
        (dict(mask=0, x0=0, noise=0, C=12), SIZES), (dict(mask=0, x0=0, noise=0, x=A + 8), ALIGN),
        (dict(mask=0, v_batch_stride=1028), ALIGN)],
    "fk_scale_noise_bf16": [(dict(x0=0), SIZES), (dict(noise=0), SIZES), (dict(out=0), SIZES)] + [(d, SIZES) for d in _BAD_DIMS] + [
        (dict(x0=3 * A + 8), ALIGN), (dict(noise=4 * A + 8), ALIGN), (dict(out=6 * A + 8), ALIGN),
        (dict(x0_batch_stride=516), ALIGN), (dict(noise_batch_stride=516), ALIGN), (dict(out_batch_stride=516), ALIGN),
        (dict(C=12, x0=3 * A + 8), SIZES), (dict(out=0, noise_batch_stride=516), SIZES), (dict(S_tgt=0, out=6 * A + 8), SIZES)],
}
CASES = [(name, change, message) for name, table in REFUSALS.items() for change, message in table]


def _call(lib, name, **change):
    kw = dict(GOOD, **change)
    return getattr(lib, name)(*[ctypes.c_void_p(kw[n] or None) if n in POINTERS else kw[n] for n in ARGS[name]])


@pytest.mark.parametrize("name,change,message", CASES,
                         ids=[name + "-" + ",".join(f"{k}={v}" for k, v in c.items()) for name, c, _ in CASES])
def test_refusal_and_its_error_string(name, change, message):
    lib = _lib()
    assert _call(lib, name, **change) == -1                          # FK_EINVAL
    assert lib.fk_last_error().decode() == f"{name}: {message}"      # the entry's own name, and this condition's text alone


def test_without_a_mask_x0_and_noise_are_not_looked_at():
    """mask NULL = a mask of ones: the call goes to the Euler launch whatever x0 and noise are.  Without a GPU the launch fails
    (or does nothing) and the made-up addresses are never used; with one, x and v are real rows and the step runs."""
    import torch
    lib, name = _lib(), "fk_euler_inpaint_step_bf16"
    rows = {}
    if torch.cuda.is_available():
        t = torch.zeros(2, 2, 8, 64, device="cuda", dtype=torch.bfloat16)
        rows = dict(x=t[0].data_ptr(), v=t[1].data_ptr(), x_batch_stride=512, v_batch_stride=512)
    for change in (dict(x0=0, noise=0), dict(x0=3 * A + 8, noise=0, x0_batch_stride=516, noise_batch_stride=3)):
        rc = _call(lib, name, mask=0, mask_batch_stride=2, **rows, **change)
        if rows:
            torch.cuda.synchronize()
            assert rc == 0
        else:
            assert rc == 0 or lib.fk_last_error().decode().startswith(name + ": launch failed"), lib.fk_last_error().decode()
