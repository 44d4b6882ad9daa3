"""CPU test of the boundary of the accumulating LoRA gradient projection (the pattern of tests/test_abi_lora_grad.py):
include/fk.h declares ``fk_lora_grad_acc_bf16``, the library exports it, libfk.py has a prototype of the declared argument layout --
``fk_lora_grad_bf16``'s with one ``int32_t`` in front of the workspace pointer -- and ``ops.lora_grad`` has the keyword."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _types(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)
    m = re.search(r"\b(?:int|int64_t)\s+" + name + r"\s*\(([^)]*)\)", header)
    assert m, f"{name} is not declared in include/fk.h"
    return [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]


def test_symbol_is_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = libfk.load()
    assert hasattr(lib, "fk_lora_grad_acc_bf16"), "fk_lora_grad_acc_bf16 is not exported by libfk"
    assert "fk_lora_grad_acc_bf16" in libfk.SIGNATURES, "fk_lora_grad_acc_bf16 has no ctypes signature"


def test_argument_list_is_the_overwrite_forms_plus_one_int32():
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "float*": libfk.c_vp, "int64_t": libfk.c_i64, "int32_t": libfk.c_i32, "float": libfk.c_f32,
             "fk_stream_t": libfk.c_vp}
    plain, acc = _types("fk_lora_grad_bf16"), _types("fk_lora_grad_acc_bf16")
    at = len(plain) - 3                          # in front of (float* ws, int64_t ws_floats, fk_stream_t stream)
    assert plain[at:] == ["float*", "int64_t", "fk_stream_t"]
    assert acc == plain[:at] + ["int32_t"] + plain[at:]
    res, args = libfk.SIGNATURES["fk_lora_grad_acc_bf16"]
    assert res is libfk.c_i32 and args == [kinds[t] for t in acc]
    res0, args0 = libfk.SIGNATURES["fk_lora_grad_bf16"]
    assert args == args0[:at] + [libfk.c_i32] + args0[at:]


def test_ops_keyword():
    from gpt_image_edit_amd import ops
    ps = inspect.signature(ops.lora_grad).parameters
    assert list(ps)[:6] == ["dw", "up", "down", "scale", "d_up", "d_down"]
    assert ps["accumulate"].default is False and ps["ws"].default is None
