"""CPU test of the float32-state step's boundary (the pattern of tests/test_abi_solver.py): include/fk.h declares it, the library
exports it, libfk.py has its prototype argument by argument, ops wraps it -- and every refusal is made on the host before
anything is launched, so its error string can be read here, without a GPU, from calls that pass made-up addresses."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fk_solver_step_f32"
ARGS = ["state", "state_batch_stride", "x", "x_batch_stride", "v", "v_batch_stride", "hist", "hist_batch_stride", "x0",
        "x0_batch_stride", "noise", "noise_batch_stride", "mask", "mask_batch_stride", "B", "S_tgt", "C", "c_v", "c_h", "use_hist",
        "load_state", "sigma_next", "stream"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def _lib():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return libfk.load()


def test_symbol_is_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    lib = _lib()
    declared = set(re.findall(r"\b(fk_[a-z0-9_]+)\s*\(", _header()))
    assert NAME in declared, f"{NAME} is not declared in include/fk.h"
    assert hasattr(lib, NAME), f"{NAME} is not exported by libfk"
    assert NAME in libfk.SIGNATURES, f"{NAME} has no ctypes signature"


def test_signature_is_the_declared_one():
    """Argument by argument: the C declaration's parameter types against the ctypes prototype."""
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "float*": libfk.c_vp, "fk_stream_t": libfk.c_vp,
             "int64_t": libfk.c_i64, "int32_t": libfk.c_i32, "float": libfk.c_f32}
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", _header())
    assert m, NAME
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(re.search(r"\b(\w+)$", arg).group(1))
        want.append(kinds[re.sub(r"\s*\b\w+$", "", arg)])              # drop the parameter's name
    res, args = libfk.SIGNATURES[NAME]
    assert res is libfk.c_i32 and args == want, (args, want)
    assert names == ARGS and len(args) == 23
    # fk_ab2_step_bf16's arguments behind the state's two, with load_state behind use_hist
    ab2 = libfk.SIGNATURES["fk_ab2_step_bf16"][1]
    assert args[2:20] == ab2[:18] and args[21:] == ab2[18:] and args[20] is libfk.c_i32


def test_the_rule_is_the_declarations_comment():
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    comment = text[:text.index("int " + NAME)].rsplit("/*", 1)[1]
    for words in ("load_state ? state : float(x)", "s + c_h * hist", "sigma_next * noise + om * x0", "never an fma",
                  "x <- bf16(out)", "hist <- v", "FK_EINVAL"):
        assert words in comment, words


def test_ops_wrapper():
    from gpt_image_edit_amd import ops
    p = inspect.signature(ops.solver_step_f32).parameters
    assert list(p) == ["state", "x", "v", "s_tgt", "c_v", "c_h", "use_hist", "load_state", "hist", "sigma_next", "x0", "noise",
                       "mask"]
    assert all(p[n].default is inspect.Parameter.empty for n in ("state", "x", "v", "s_tgt", "c_v"))
    assert (p["c_h"].default, p["use_hist"].default, p["load_state"].default, p["sigma_next"].default) == (0.0, 0, 1, 0.0)
    import torch
    z = torch.zeros(1, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # a missing GPU is an error, not another path
        ops.solver_step_f32(torch.zeros(1, 8, 64), z, z, 8, -0.1)


def test_it_lives_in_the_file_that_is_built_without_contraction():
    mk = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "solver_step.hip")).read()
    assert re.search(r"^solver_step\.o:\s*EXTRA\s*:=.*-ffp-contract=off", mk, flags=re.M)
    assert 'extern "C" int ' + NAME in src
    common = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "step_common.h")).read()
    # the kernel's arithmetic is its own text plus the step_common.h helpers it calls, and the ones those call: each must be one
    # this test knows, and the float32 rule holds over all of that text together
    helpers = {m.group(1): m.group(0) for m in re.finditer(r"^FK_DEV [^\n(]*?\b(\w+)\([^\n]*\{\n.*?^\}\n", common, flags=re.M | re.S)}
    assert {"widen8", "pack8", "axpy8_rn", "load_keep8", "blend8_bf16", "blend8_f32", "keep_f"} <= set(helpers)
    body = src[src.index("void state_kernel"):src.index('extern "C" int ' + NAME)]
    called, todo = set(), [body]
    while todo:
        text = todo.pop()
        for name in helpers:
            if name not in called and re.search(r"\b" + name + r"\(", text.split("{", 1)[1]):
                called.add(name)
                todo.append(helpers[name])
    assert called == {"widen8", "axpy8_rn", "blend8_f32", "load_keep8", "pack8"}, called
    body += "".join(helpers[name] for name in sorted(called))
    assert "__fmul_rn" in body and "__fadd_rn" in body and "fmaf" not in body and "keep_f" not in body and "round_bf" not in body
    assert "ew_grid" in common and "ew_grid(nvec)" in src[src.index('extern "C" int ' + NAME):]


# ---- the refusals: host checks before any launch ----------------------------------------------------------------------------------
A = 0x10000          # made-up addresses, 16-byte aligned and distinct; a refused call dereferences none of them
GOOD = dict(state=A, state_batch_stride=512, x=2 * A, x_batch_stride=1024, v=3 * A, v_batch_stride=1024, hist=4 * A,
            hist_batch_stride=512, x0=5 * A, x0_batch_stride=512, noise=6 * A, noise_batch_stride=512, mask=7 * A,
            mask_batch_stride=32, B=2, S_tgt=8, C=64, c_v=-0.05, c_h=0.01, use_hist=1, load_state=1, sigma_next=0.5, stream=0)
REFUSALS = [
    (dict(state=0), "bad sizes"), (dict(x=0), "bad sizes"), (dict(v=0), "bad sizes"),
    (dict(B=0), "bad sizes"), (dict(S_tgt=0), "bad sizes"), (dict(C=0), "bad sizes"), (dict(B=-1), "bad sizes"),
    (dict(S_tgt=-3), "bad sizes"), (dict(C=-8), "bad sizes"), (dict(C=12), "bad sizes"), (dict(C=4), "bad sizes"),
    (dict(use_hist=2), "use_hist=2 is neither 0 nor 1"), (dict(use_hist=-1), "use_hist=-1 is neither 0 nor 1"),
    (dict(load_state=2), "load_state=2 is neither 0 nor 1"), (dict(load_state=-1), "load_state=-1 is neither 0 nor 1"),
    (dict(load_state=2, mask=0), "load_state=2"),
    (dict(hist=0), "use_hist=1 needs a history buffer"), (dict(hist=0, mask=0), "use_hist=1 needs a history buffer"),
    (dict(hist=2 * A), "hist must be a buffer of its own"), (dict(hist=3 * A), "hist must be a buffer of its own"),
    (dict(hist=A), "hist must be a buffer of its own"), (dict(hist=3 * A, use_hist=0), "hist must be a buffer of its own"),
    (dict(state=2 * A), "state must be a buffer of its own"), (dict(x=A), "state must be a buffer of its own"),
    (dict(x=2 * A + 8), ": alignment"), (dict(v=3 * A + 8), ": alignment"), (dict(hist=4 * A + 8), ": alignment"),
    (dict(x_batch_stride=1028), ": alignment"), (dict(v_batch_stride=1028), ": alignment"),
    (dict(hist_batch_stride=516), ": alignment"),
    (dict(state=A + 8), "alignment of the state"), (dict(state=A + 4), "alignment of the state"),
    (dict(state_batch_stride=514), "alignment of the state"), (dict(state_batch_stride=513), "alignment of the state"),
    (dict(x0=0), "a mask needs x0 and noise"), (dict(noise=0), "a mask needs x0 and noise"),
    (dict(x0=0, noise=0), "a mask needs x0 and noise"),
    (dict(x0=5 * A + 8), "alignment of x0 / noise"), (dict(noise=6 * A + 8), "alignment of x0 / noise"),
    (dict(x0_batch_stride=516), "alignment of x0 / noise"), (dict(noise_batch_stride=516), "alignment of x0 / noise"),
    (dict(mask=7 * A + 4), "alignment of the mask"), (dict(mask_batch_stride=2), "alignment of the mask"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_refusal_and_its_error_string(change, message):
    lib = _lib()
    kw = dict(GOOD, **change)
    args = [kw[n] if n not in ("state", "x", "v", "hist", "x0", "noise", "mask", "stream") else ctypes.c_void_p(kw[n] or None)
            for n in ARGS]
    assert lib.fk_solver_step_f32(*args) == -1                       # FK_EINVAL
    err = lib.fk_last_error().decode()
    assert err.startswith(NAME + ":") and message in err, err
