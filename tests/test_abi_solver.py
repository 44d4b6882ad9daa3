"""CPU test of the multistep solver's boundary (the pattern of tests/test_abi_step_cache.py): include/fk.h declares the step,
the library exports it, libfk.py has its prototype argument by argument, and ops wraps it."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fk_ab2_step_bf16"


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
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "fk_stream_t": libfk.c_vp, "int64_t": libfk.c_i64,
             "int32_t": libfk.c_i32, "float": libfk.c_f32}
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", _header())
    assert m, NAME
    names, want = [], []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        names.append(re.search(r"\b(\w+)$", arg).group(1))
        want.append(kinds[re.sub(r"\s*\b\w+$", "", arg)])              # drop the parameter's name
    res, args = libfk.SIGNATURES[NAME]
    assert res is libfk.c_i32 and args == want, (args, want)
    assert names == ["x", "x_batch_stride", "v", "v_batch_stride", "hist", "hist_batch_stride", "x0", "x0_batch_stride", "noise",
                     "noise_batch_stride", "mask", "mask_batch_stride", "B", "S_tgt", "C", "c_v", "c_h", "use_hist", "sigma_next",
                     "stream"]
    assert len(args) == 20


def test_ops_wrapper():
    from gpt_image_edit_amd import ops
    p = inspect.signature(ops.ab2_step).parameters
    assert list(p) == ["x", "v", "hist", "s_tgt", "c_v", "c_h", "use_hist", "sigma_next", "x0", "noise", "mask"]
    assert p["sigma_next"].default == 0.0 and all(p[n].default is None for n in ("x0", "noise", "mask"))
    assert all(p[n].default is inspect.Parameter.empty for n in ("x", "v", "hist", "s_tgt", "c_v", "c_h", "use_hist"))


def test_new_file_is_built_by_the_makefile_without_contraction():
    mk = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "solver_step.hip"))
    assert "$(wildcard *.hip)" in mk
    # the step is specified product by product: hipcc's default contraction would fuse them
    assert re.search(r"^solver_step\.o:\s*EXTRA\s*:=.*-ffp-contract=off", mk, flags=re.M)
