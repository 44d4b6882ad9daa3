"""CPU test of the key-mask boundary (the pattern of tests/test_abi.py): include/fk.h declares the packer and the masked
attention entry points, the library exports them, libfk.py has their prototypes, and the ops wrappers take the packed mask."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fk_pack_key_mask", "fk_attention_fwd_masked_bf16", "fk_attention_fwd_masked_f32_debug", "fk_attention_bwd_masked_bf16")


def test_masked_attention_symbols_are_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fk_[a-z0-9_]+)\s*\(", src))
    lib = libfk.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/fk.h"
        assert hasattr(lib, name), f"{name} is not exported by libfk"
        assert name in libfk.SIGNATURES, f"{name} has no ctypes signature"
    # argument counts as fk.h states them
    assert len(libfk.SIGNATURES["fk_pack_key_mask"][1]) == 6
    assert len(libfk.SIGNATURES["fk_attention_fwd_masked_bf16"][1]) == 15
    assert len(libfk.SIGNATURES["fk_attention_fwd_masked_f32_debug"][1]) == 14
    assert len(libfk.SIGNATURES["fk_attention_bwd_masked_bf16"][1]) == 16


def test_ops_wrappers_take_the_packed_mask():
    from gpt_image_edit_amd import ops
    assert callable(ops.pack_key_mask)
    for fn in (ops.attention, ops.attention_lse, ops.attention_bwd, ops.attention_f32_debug):
        p = inspect.signature(fn).parameters
        assert "key_mask" in p and p["key_mask"].default is None, fn.__name__


def test_the_precondition_is_stated_in_the_header():
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    assert "PRECONDITION" in text and "at least one valid key" in text and "finite" in text
