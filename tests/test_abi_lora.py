"""CPU test of the LoRA merge boundary (the pattern of tests/test_abi_step_cache.py): include/fk.h declares the entry point
and its term struct, the library exports it, libfk.py has the prototype and a struct of the C compiler's layout, and ops
wraps it."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def test_symbol_is_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = libfk.load()
    assert re.search(r"\bint\s+fk_lora_merge_bf16\s*\(", _header())
    assert hasattr(lib, "fk_lora_merge_bf16") and "fk_lora_merge_bf16" in libfk.SIGNATURES
    res, args = libfk.SIGNATURES["fk_lora_merge_bf16"]
    V, I64, I32 = libfk.c_vp, libfk.c_i64, libfk.c_i32
    assert res is I32 and args == [V, I64, V, I64, I32, I32, ctypes.POINTER(libfk.LoraTerm), I32, V]
    m = re.search(r"\bint\s+fk_lora_merge_bf16\s*\(([^)]*)\)", _header())
    types = [re.sub(r"\s*\b\w+$", "", " ".join(a.split())) for a in m.group(1).split(",")]
    assert types == ["const void*", "int64_t", "void*", "int64_t", "int32_t", "int32_t", "const fk_lora_term*", "int32_t", "fk_stream_t"]


def test_term_struct_layout_matches_the_header(tmp_path):
    from gpt_image_edit_amd import libfk
    fields = [f for f, _ in libfk.LoraTerm._fields_]
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "fk.h"\nint main(){printf("%zu", sizeof(fk_lora_term));\n'
            + "".join(f'printf(" %zu", offsetof(fk_lora_term, {f}));\n' for f in fields)
            + 'printf(" %d %d\\n", FK_LORA_MAX_TERMS, FK_LORA_MAX_RANK);return 0;}\n')
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(code)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(libfk.LoraTerm)] + [getattr(libfk.LoraTerm, f).offset for f in fields]
    assert got[:-2] == want and want[0] == 40
    assert got[-2:] == [libfk.FK_LORA_MAX_TERMS, libfk.FK_LORA_MAX_RANK] == [4, 128]


def test_ops_wrapper_and_makefile():
    from gpt_image_edit_amd import ops
    ps = inspect.signature(ops.lora_merge).parameters
    assert list(ps) == ["base", "terms", "out"] and ps["out"].default is None
    mk = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "lora_merge.hip")) and "$(wildcard *.hip)" in mk
