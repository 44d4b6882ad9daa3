"""CPU test of the LoRA gradient boundary (the pattern of tests/test_abi_lora.py): include/fk.h declares the two entry
points, the library exports them, libfk.py has prototypes of the declared argument layout, and ops wraps them."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def _types(name):
    m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)", _header())
    assert m, f"{name} is not declared in include/fk.h"
    return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]


def test_symbols_are_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = libfk.load()
    for name in ("fk_lora_grad_bf16", "fk_lora_grad_ws_floats"):
        assert hasattr(lib, name), f"{name} is not exported by libfk"
        assert name in libfk.SIGNATURES, f"{name} has no ctypes signature"
    # the split plan csrc/lora_grad.hip's header states: nothing split below 257 k / 129 n, two partials just above
    assert lib.fk_lora_grad_ws_floats(64, 128, 8) == 0 and lib.fk_lora_grad_ws_floats(128, 256, 128) == 0
    assert lib.fk_lora_grad_ws_floats(16, 264, 8) == 2 * 16 * 8 and lib.fk_lora_grad_ws_floats(131, 16, 8) == 2 * 8 * 16
    assert lib.fk_lora_grad_ws_floats(3072, 3072, 16) == 6 * 3072 * 16 + 8 * 16 * 3072
    assert lib.fk_lora_grad_ws_floats(0, 8, 8) == 0 and lib.fk_lora_grad_ws_floats(8, 8, 129) == 0


def test_argument_layout_matches_the_header():
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "float*": libfk.c_vp, "int64_t": libfk.c_i64, "int32_t": libfk.c_i32,
             "float": libfk.c_f32, "fk_stream_t": libfk.c_vp}
    types = _types("fk_lora_grad_bf16")
    assert types == ["const void*", "int64_t", "const void*", "int64_t", "const void*", "int64_t", "int32_t", "int32_t", "int32_t",
                     "float", "float*", "float*", "float*", "int64_t", "fk_stream_t"]
    res, args = libfk.SIGNATURES["fk_lora_grad_bf16"]
    assert res is libfk.c_i32 and args == [kinds[t] for t in types]
    assert _types("fk_lora_grad_ws_floats") == ["int32_t", "int32_t", "int32_t"]
    assert libfk.SIGNATURES["fk_lora_grad_ws_floats"] == (libfk.c_i64, [libfk.c_i32] * 3)


def test_ops_wrapper_and_makefile():
    from gpt_image_edit_amd import ops
    ps = inspect.signature(ops.lora_grad).parameters
    assert list(ps)[:6] == ["dw", "up", "down", "scale", "d_up", "d_down"] and ps["d_up"].default is None and ps["d_down"].default is None
    mk = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "lora_grad.hip")) and "$(wildcard *.hip)" in mk
