"""CPU test of the first-block measure's boundary (the pattern of tests/test_abi_step_cache.py): include/fk.h declares
fk_residual_absdiff_sums_bf16, the library exports it, libfk.py has its prototype, and ops wraps it."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fk_residual_absdiff_sums_bf16"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def test_symbol_is_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    declared = set(re.findall(r"\b(fk_[a-z0-9_]+)\s*\(", _header()))
    lib = libfk.load()
    assert NAME in declared, f"{NAME} is not declared in include/fk.h"
    assert hasattr(lib, NAME), f"{NAME} is not exported by libfk"
    assert NAME in libfk.SIGNATURES, f"{NAME} has no ctypes signature"


def test_signature_is_the_declared_one():
    """Argument by argument: the C declaration's parameter types against the ctypes prototype."""
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "float*": libfk.c_vp, "fk_stream_t": libfk.c_vp,
             "fk_rows": libfk.Rows, "int64_t": libfk.c_i64, "int32_t": libfk.c_i32}
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", _header())
    assert m, NAME
    want, names = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(re.search(r"\b(\w+)$", arg).group(1))
        want.append(kinds[re.sub(r"\s*\b\w+$", "", arg)])          # drop the parameter's name
    res, args = libfk.SIGNATURES[NAME]
    assert res is libfk.c_i32 and args == want, (args, want)
    assert names == ["h1", "r1", "h0", "r0", "ref", "rf", "r_out", "rr", "M", "D", "is_bf16", "out", "ws", "ws_floats", "stream"]
    # the three inputs and r_out each travel with an fk_rows of their own; the tail is fk_absdiff_sums_bf16's
    assert args[:8] == [libfk.c_vp, libfk.Rows] * 4 and args[8:] == libfk.SIGNATURES["fk_absdiff_sums_bf16"][1][4:]


def test_ops_wrapper():
    from gpt_image_edit_amd import ops
    sig = inspect.signature(ops.residual_absdiff_sums)
    assert list(sig.parameters) == ["h1", "h0", "ref", "r_out", "out", "ws"]
    assert all(sig.parameters[k].default is None for k in ("r_out", "out", "ws"))


def test_the_measure_shares_the_sums_workspace_and_file():
    src = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "step_cache.hip")).read()
    assert NAME in src and "fk_absdiff_ws_floats" in src
    assert "atomic" not in src.replace("No floating-point atomics", "")
