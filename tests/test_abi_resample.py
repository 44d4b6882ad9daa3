"""CPU test of the resample entries' boundary (the pattern of tests/test_abi_mask_ops.py): include/fk.h declares them with their
rule, the library exports them, libfk.py has their prototypes argument by argument, ops wraps them -- and every refusal is made on
the host before anything is launched, so its error string can be read here, without a GPU, from calls that pass made-up addresses."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fk_resample_pass_u8": ["src", "src_batch_stride", "src_row_stride", "dst", "B", "Hin", "Win", "C", "axis", "n_out", "bounds", "kk",
                            "ksize", "stream"],
    "fk_bytes_overlay_u8": ["res", "orig", "orig_batch", "alpha", "alpha_batch", "dst", "B", "H", "W", "x0", "y0", "x1", "y1", "stream"],
}
POINTERS = {"src", "dst", "bounds", "kk", "res", "orig", "alpha", "stream"}


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
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "const int32_t*": libfk.c_vp, "fk_stream_t": libfk.c_vp,
             "int64_t": libfk.c_i64, "int32_t": libfk.c_i32}
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


def test_the_cap_is_one_constant():
    from gpt_image_edit_amd import helpers, libfk
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    cap = int(re.search(r"#define FK_RESAMPLE_MAX_KSIZE (\d+)", text).group(1))
    assert cap == 513 == helpers.FK_RESAMPLE_MAX_KSIZE == libfk.FK_RESAMPLE_MAX_KSIZE
    assert helpers.resample_coeffs(512, 2, "bilinear")[2] == cap             # 1/256 is the last bilinear scale under it
    assert helpers.resample_coeffs(255, 3, "lanczos")[2] == 511              # 1/85 the last lanczos one
    with pytest.raises(ValueError, match="FK_RESAMPLE_MAX_KSIZE"):
        helpers.resample_coeffs(258, 3, "lanczos")


def test_the_rules_are_the_declarations_comments():
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    block = text[text.index("Antialiased byte resize and byte paste-back"):text.index("int fk_bytes_overlay_u8")]
    for words in ("Pillow's 8-bit resize", "EQUALITY", "bilinear 1 - |x| on |x| < 1, support 1", "a = -0.5, support 2",
                  "sinc(x) sinc(x / 3)", "-3 <= x < 3", "scale = n_in / n_out", "fs = max(scale, 1)", "support = filter_support * fs",
                  "ksize = ceil(support) * 2 + 1", "center = (i + 0.5) * scale", "xmin = max(int(center - support + 0.5), 0)",
                  "xmax = min(int(center + support + 0.5), n_in)", "summed in ascending t", "kk_t = int(w_t * 2^22 + 0.5) for w_t >= 0",
                  "int(w_t * 2^22 - 0.5) otherwise", "out = clip((2^21 + sum_t kk_t * src[xmin + t]) >> 22, 0, 255)",
                  "int32 accumulator", "arithmetic shift", "uint8 intermediate [B, Hin, Wout, C]", "is skipped", "crop-then-resize",
                  "TAP-MAJOR", "255 * sum_t |kk_t| + 2^21 < 2^31", "FK_EINVAL", "nothing written", "a == 0: o, taken",
                  "a == 255: r, taken", "(2 * (a * r + (255 - a) * o) + 255) / 510", "a tie cannot occur",
                  "Parity with PIL's compositing is not"):
        assert words in block, words
    # the stated gap is closed where it was stated; the blur's parity stays open
    old = text[text.index("Masked edits on the masked box"):text.index("int64_t fk_mask_bbox_ws_ints")]
    assert "lanczos resize is unpinned" not in old and "GaussianBlur is unpinned" in old and "pinned byte for byte" in old


def test_ops_wrappers():
    import torch
    from gpt_image_edit_amd import ops
    sig = {n: list(inspect.signature(getattr(ops, n)).parameters) for n in ("resample_u8", "resample_pass_u8", "bytes_overlay")}
    assert sig["resample_u8"] == ["src_view", "out_h", "out_w", "filter", "out"]
    assert sig["resample_pass_u8"] == ["src_view", "axis", "n_out", "filter", "out"]
    assert sig["bytes_overlay"] == ["res", "orig_u8", "alpha_u8", "box", "out"]
    pic = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for call in (lambda: ops.resample_u8(pic, 4, 4, "lanczos"), lambda: ops.resample_pass_u8(pic, 1, 4, "bilinear"),
                 lambda: ops.bytes_overlay(pic[:, :4, :4].contiguous(), pic, None, (0, 0, 4, 4))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):        # a missing GPU is an error, not another path
            call()
    with pytest.raises(ValueError, match="filter"):
        ops.resample_u8(pic, 4, 4, "nearest")


def test_the_kernels_are_integer_and_take_no_box():
    src = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "resample.hip")).read()
    for name in ARGS:
        assert 'extern "C" int ' + name in src
    assert "float" not in src and "double" not in src
    assert "__shared__" in src and "kkT" in src


# ---- the refusals: host checks before any launch ----------------------------------------------------------------------------------
A = 0x10000          # made-up addresses, 16-byte aligned and distinct; a refused call dereferences none of them
GOOD = {
    "fk_resample_pass_u8": dict(src=A, src_batch_stride=37 * 300, src_row_stride=300, dst=2 * A, B=2, Hin=37, Win=67, C=3, axis=1,
                                n_out=20, bounds=3 * A, kk=4 * A, ksize=23, stream=0),
    "fk_bytes_overlay_u8": dict(res=A, orig=2 * A, orig_batch=1, alpha=3 * A, alpha_batch=3, dst=4 * A, B=3, H=37, W=67, x0=5, y0=3,
                                x1=67, y1=37, stream=0),
}
REFUSALS = [
    ("fk_resample_pass_u8", dict(src=0), "null pointer"), ("fk_resample_pass_u8", dict(dst=0), "null pointer"),
    ("fk_resample_pass_u8", dict(bounds=0), "null pointer"), ("fk_resample_pass_u8", dict(kk=0), "null pointer"),
    ("fk_resample_pass_u8", dict(C=2), "C=2 is neither 1 nor 3"), ("fk_resample_pass_u8", dict(C=4), "C=4 is neither 1 nor 3"),
    ("fk_resample_pass_u8", dict(C=0), "C=0 is neither 1 nor 3"),
    ("fk_resample_pass_u8", dict(B=0), "sizes must be positive (B=0, Hin=37, Win=67, n_out=20)"),
    ("fk_resample_pass_u8", dict(Hin=0), "sizes must be positive"), ("fk_resample_pass_u8", dict(Win=-1), "sizes must be positive"),
    ("fk_resample_pass_u8", dict(n_out=0), "sizes must be positive"),
    ("fk_resample_pass_u8", dict(axis=2), "axis=2 is neither 0 (vertical) nor 1 (horizontal)"),
    ("fk_resample_pass_u8", dict(axis=-1), "axis=-1 is neither 0"),
    ("fk_resample_pass_u8", dict(ksize=0), "ksize=0 is below 1"), ("fk_resample_pass_u8", dict(ksize=-3), "ksize=-3 is below 1"),
    ("fk_resample_pass_u8", dict(ksize=514), "ksize=514 is above FK_RESAMPLE_MAX_KSIZE = 513"),
    ("fk_resample_pass_u8", dict(src_row_stride=200), "rows of 201 bytes overlap at a row stride of 200"),
    ("fk_resample_pass_u8", dict(src_batch_stride=-1), "batch stride -1"),
    ("fk_resample_pass_u8", dict(bounds=3 * A + 2), ": alignment"), ("fk_resample_pass_u8", dict(kk=4 * A + 1), ": alignment"),
    ("fk_resample_pass_u8", dict(dst=A), "dst must be a buffer of its own"),
    ("fk_bytes_overlay_u8", dict(res=0), "bad arguments"), ("fk_bytes_overlay_u8", dict(orig=0), "bad arguments"),
    ("fk_bytes_overlay_u8", dict(dst=0), "bad arguments"), ("fk_bytes_overlay_u8", dict(B=0), "bad arguments"),
    ("fk_bytes_overlay_u8", dict(H=0), "bad arguments"), ("fk_bytes_overlay_u8", dict(W=0), "bad arguments"),
    ("fk_bytes_overlay_u8", dict(orig_batch=2), "2 original pictures for a batch of 3"),
    ("fk_bytes_overlay_u8", dict(orig_batch=0), "0 original pictures for a batch of 3"),
    ("fk_bytes_overlay_u8", dict(alpha_batch=2), "alpha_batch=2 is neither 1 nor the batch 3"),
    ("fk_bytes_overlay_u8", dict(alpha_batch=0), "alpha_batch=0 is neither 1 nor the batch 3"),
    ("fk_bytes_overlay_u8", dict(alpha=0), "alpha_batch=3 is neither 1 nor the batch 3 (0 without alpha)"),
    ("fk_bytes_overlay_u8", dict(x1=68), "box (5, 3, 68, 37) is empty or outside the 67 x 37 picture"),
    ("fk_bytes_overlay_u8", dict(x0=67), "box (67, 3, 67, 37) is empty or outside"),
    ("fk_bytes_overlay_u8", dict(y0=-2), "box (5, -2, 67, 37) is empty or outside"),
    ("fk_bytes_overlay_u8", dict(y1=38), "box (5, 3, 67, 38) is empty or outside"),
    ("fk_bytes_overlay_u8", dict(dst=2 * A), "dst must be a buffer of its own"),
    ("fk_bytes_overlay_u8", dict(dst=3 * A), "dst must be a buffer of its own"),
    ("fk_bytes_overlay_u8", dict(dst=A), "dst must be a buffer of its own"),
]


@pytest.mark.parametrize("name,change,message", REFUSALS,
                         ids=[n[3:15] + ":" + ",".join(f"{k}={v}" for k, v in c.items()) for n, c, _ in REFUSALS])
def test_refusal_and_its_error_string(name, change, message):
    lib = _lib()
    kw = dict(GOOD[name], **change)
    args = [ctypes.c_void_p(kw[n] or None) if n in POINTERS else kw[n] for n in ARGS[name]]
    assert getattr(lib, name)(*args) == -1                               # FK_EINVAL
    err = lib.fk_last_error().decode()
    assert err.startswith(name + ":") and message in err, err
