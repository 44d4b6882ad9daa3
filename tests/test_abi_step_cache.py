"""CPU test of the step-cache boundary (the pattern of tests/test_abi_attention_mask.py): include/fk.h declares the three
kernels and the workspace size, the library exports them, libfk.py has their prototypes, and ops wraps them."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fk_absdiff_sums_bf16", "fk_residual_save_bf16", "fk_residual_apply_bf16", "fk_absdiff_ws_floats")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def test_step_cache_symbols_are_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    declared = set(re.findall(r"\b(fk_[a-z0-9_]+)\s*\(", _header()))
    lib = libfk.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/fk.h"
        assert hasattr(lib, name), f"{name} is not exported by libfk"
        assert name in libfk.SIGNATURES, f"{name} has no ctypes signature"
    assert lib.fk_absdiff_ws_floats() == 2 * 1024


def test_signatures_are_the_declared_ones():
    """Argument by argument: the C declaration's parameter types against the ctypes prototype."""
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "float*": libfk.c_vp, "fk_stream_t": libfk.c_vp,
             "fk_rows": libfk.Rows, "int64_t": libfk.c_i64, "int32_t": libfk.c_i32}
    src = _header()
    for name in NEW[:3]:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            typ = re.sub(r"\s*\b\w+$", "", " ".join(arg.split()))          # drop the parameter's name
            want.append(kinds[typ])
        res, args = libfk.SIGNATURES[name]
        assert res is libfk.c_i32 and args == want, (name, args, want)
    assert libfk.SIGNATURES["fk_absdiff_ws_floats"] == (libfk.c_i64, [])
    assert len(libfk.SIGNATURES["fk_absdiff_sums_bf16"][1]) == 11
    assert len(libfk.SIGNATURES["fk_residual_save_bf16"][1]) == len(libfk.SIGNATURES["fk_residual_apply_bf16"][1]) == 10
    assert ctypes.sizeof(libfk.Rows) == 24


def test_ops_wrappers():
    from gpt_image_edit_amd import ops
    assert list(inspect.signature(ops.absdiff_sums).parameters)[:3] == ["a", "b", "out"]
    assert inspect.signature(ops.absdiff_sums).parameters["out"].default is None
    assert list(inspect.signature(ops.residual_save).parameters) == ["h_out", "h0", "r"]
    assert list(inspect.signature(ops.residual_apply).parameters) == ["h0", "r", "out"]


def test_new_file_is_built_by_the_makefile():
    mk = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "step_cache.hip"))
    assert "$(wildcard *.hip)" in mk or "step_cache.hip" in mk
