"""CPU test of the factored LoRA gradient's boundary (the pattern of tests/test_abi_lora_grad.py): include/fk.h declares the two
entry points, the library exports them, libfk.py has prototypes of the declared argument layout, and ops wraps them."""
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
    for name in ("fk_lora_side_grad_bf16", "fk_lora_side_grad_ws_floats"):
        assert hasattr(lib, name), f"{name} is not exported by libfk"
        assert name in libfk.SIGNATURES, f"{name} has no ctypes signature"
    ws = lib.fk_lora_side_grad_ws_floats
    # the plan csrc/lora_side_grad.hip's header states: 3 floats of alignment slack + four bf16 [r_pad][M_pad] matrices, and the
    # partials of a split m reduction -- nothing split up to M = 128, two chunks from M = 129, 10 per role at the production shape
    assert ws(1, 64, 16, 32, 32) == 3 + 2 * 32 * 64 and ws(2, 64, 16, 32, 33) == 3 + 2 * 64 * 128
    assert ws(1, 129, 16, 8, 8) == 2 * 16 * 8 + 2 * 8 * 8 + 3 + 2 * 32 * 192 == ws(3, 43, 16, 8, 8)
    assert ws(1, 8704, 3072, 3072, 16) == 2 * 10 * 3072 * 16 + 3 + 2 * 32 * 8704
    assert ws(0, 8, 8, 8, 8) == 0 and ws(1, 8, 8, 8, 129) == 0 and ws(1, 8, 8, 8, 0) == 0 and ws(1 << 20, 1 << 20, 8, 8, 8) == 0


def test_argument_layout_matches_the_header():
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "float*": libfk.c_vp, "int64_t": libfk.c_i64, "int": libfk.c_i32, "float": libfk.c_f32,
             "fk_stream_t": libfk.c_vp}
    types = _types("fk_lora_side_grad_bf16")
    assert types == ["const void*", "int64_t", "int64_t", "const void*", "int64_t", "int64_t", "int64_t", "int64_t", "int64_t", "int64_t",
                     "const void*", "int64_t", "const void*", "int64_t", "int64_t", "float", "float*", "float*", "int", "float*",
                     "int64_t", "fk_stream_t"]
    res, args = libfk.SIGNATURES["fk_lora_side_grad_bf16"]
    assert res is libfk.c_i32 and args == [kinds[t] for t in types]
    assert _types("fk_lora_side_grad_ws_floats") == ["int64_t"] * 5
    assert libfk.SIGNATURES["fk_lora_side_grad_ws_floats"] == (libfk.c_i64, [libfk.c_i64] * 5)


def test_ops_wrapper_and_makefile():
    from gpt_image_edit_amd import ops
    ps = inspect.signature(ops.lora_side_grad).parameters
    assert list(ps) == ["x", "dy", "up", "down", "scale", "d_up", "d_down", "ws", "accumulate"]
    assert ps["d_up"].default is None and ps["d_down"].default is None and ps["ws"].default is None and ps["accumulate"].default is False
    assert list(inspect.signature(ops.lora_side_grad_ws).parameters) == ["B", "R", "N", "K", "rank", "device"]
    mk = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "lora_side_grad.hip")) and "$(wildcard *.hip)" in mk
