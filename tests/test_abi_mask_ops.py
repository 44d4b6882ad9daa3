"""CPU test of the mask-box entries' boundary (the pattern of tests/test_abi_solver_state.py): include/fk.h declares them, the
library exports them, libfk.py has their prototypes argument by argument, ops wraps them -- and every refusal is made on the host
before anything is launched, so its error string can be read here, without a GPU, from calls that pass made-up addresses."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fk_mask_bbox_u8": ["mask", "Bm", "H", "W", "threshold", "out4", "ws", "ws_ints", "stream"],
    "fk_mask_blur_u8": ["src", "dst", "plane", "taps", "R", "Bm", "H", "W", "stream"],
    "fk_pixels_u8_box_to_nhwc_bf16": ["src", "dst", "B", "Hin", "Win", "x0", "y0", "x1", "y1", "Hout", "Wout", "Cpad", "renorm", "stream"],
    "fk_image_overlay_u8": ["img", "img_is_fp32", "h", "w", "orig", "orig_batch", "alpha", "alpha_batch", "dst", "B", "H", "W", "x0",
                            "y0", "x1", "y1", "stream"],
}
POINTERS = {"mask", "out4", "ws", "src", "dst", "plane", "taps", "img", "orig", "alpha", "stream"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def _lib():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return libfk.load()


@pytest.mark.parametrize("name", list(ARGS) + ["fk_mask_bbox_ws_ints"])
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
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "float*": libfk.c_vp, "const float*": libfk.c_vp,
             "int32_t*": libfk.c_vp, "fk_stream_t": libfk.c_vp, "int64_t": libfk.c_i64, "int32_t": libfk.c_i32}
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


def test_workspace_size_and_blur_radius():
    from gpt_image_edit_amd import helpers, libfk
    lib = _lib()
    assert libfk.SIGNATURES["fk_mask_bbox_ws_ints"] == (libfk.c_i64, [])
    assert lib.fk_mask_bbox_ws_ints() == 4 * 4096                       # four ints per block of the elementwise grid's cap
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    radius = int(re.search(r"#define FK_MASK_BLUR_MAX_RADIUS (\d+)", text).group(1))
    assert radius == 192 and helpers.gaussian_taps(helpers.MASK_BLUR_MAX_SIGMA).numel() == 2 * radius + 1


def test_the_rules_are_the_declarations_comments():
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    block = text[text.index("Masked edits on the masked box"):text.index("int fk_image_overlay_u8")]
    for words in ("parity with PIL's", "unpinned", "one fp32 operation", "clamped before its load", "no atomics", "FK_EINVAL",
                  "writes nothing", "antialiased", "s = clamp((X + 0.5) * (n_in / n_out) - 0.5, 0, n_in - 1)",
                  "i1 = min(i0 + 1, n_in - 1)", "(1-fy) * ((1-fx) * p00 + fx * p01) + fy * ((1-fx) * p10 + fx * p11)",
                  "(W, H, 0, 0)", "one-block finish", "R = ceil(3 sigma)", "acc = acc + w[k] * float(src[y, clamp(x + k, 0, W-1)])",
                  "uint8(rint(clamp(v, 0, 255)))", "every byte of the box is >= 128", "a == 0: o, taken", "a == 255: c, taken",
                  "(a * c + (255 - a) * o) / 255", "fk_image_to_u8_nhwc's bits"):
        assert words in block, words


def test_ops_wrappers():
    import torch
    from gpt_image_edit_amd import ops
    sig = {n: list(inspect.signature(getattr(ops, n)).parameters) for n in ("mask_bbox", "mask_blur", "pixels_box_to_nhwc", "image_overlay")}
    assert sig["mask_bbox"][:2] == ["mask_u8", "threshold"] and sig["mask_blur"][:2] == ["mask_u8", "sigma"]
    assert sig["pixels_box_to_nhwc"][:6] == ["u8", "box", "out_h", "out_w", "cpad", "renorm"]
    assert sig["image_overlay"][:4] == ["img", "orig_u8", "alpha_u8", "box"]
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    for call in (lambda: ops.mask_bbox(m, 1), lambda: ops.mask_blur(m, 1.0),
                 lambda: ops.pixels_box_to_nhwc(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (0, 0, 4, 4), 8, 8),
                 lambda: ops.image_overlay(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, 3, dtype=torch.uint8), m, (0, 0, 4, 4))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):        # a missing GPU is an error, not another path
            call()


def test_they_live_in_the_file_that_is_built_without_contraction():
    csrc = os.path.join(ROOT, "gpt_image_edit_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    src = open(os.path.join(csrc, "mask_ops.hip")).read()
    assert re.search(r"^mask_ops\.o:\s*EXTRA\s*:=.*-ffp-contract=off", mk, flags=re.M)
    for name in ARGS:
        assert 'extern "C" int ' + name in src
    assert "fmaf" not in src and "atomic" not in src.replace("no atomics", "").replace("uses atomics", "")
    assert src.count("ew_grid(") >= 5 and '#include "step_common.h"' in src


# ---- the refusals: host checks before any launch ----------------------------------------------------------------------------------
A = 0x10000          # made-up addresses, 16-byte aligned and distinct; a refused call dereferences none of them
GOOD = {
    "fk_mask_bbox_u8": dict(mask=A, Bm=2, H=37, W=67, threshold=1, out4=2 * A, ws=3 * A, ws_ints=4 * 4096, stream=0),
    "fk_mask_blur_u8": dict(src=A, dst=2 * A, plane=3 * A, taps=4 * A, R=6, Bm=2, H=37, W=67, stream=0),
    "fk_pixels_u8_box_to_nhwc_bf16": dict(src=A, dst=2 * A, B=2, Hin=37, Win=67, x0=5, y0=3, x1=67, y1=37, Hout=64, Wout=96, Cpad=32,
                                          renorm=0, stream=0),
    "fk_image_overlay_u8": dict(img=A, img_is_fp32=0, h=64, w=96, orig=2 * A, orig_batch=1, alpha=3 * A, alpha_batch=3, dst=4 * A, B=3,
                                H=37, W=67, x0=5, y0=3, x1=67, y1=37, stream=0),
}
REFUSALS = [
    ("fk_mask_bbox_u8", dict(mask=0), "bad arguments"), ("fk_mask_bbox_u8", dict(out4=0), "bad arguments"),
    ("fk_mask_bbox_u8", dict(ws=0), "bad arguments"), ("fk_mask_bbox_u8", dict(Bm=0), "bad arguments"),
    ("fk_mask_bbox_u8", dict(H=0), "bad arguments"), ("fk_mask_bbox_u8", dict(W=-1), "bad arguments"),
    ("fk_mask_bbox_u8", dict(threshold=256), "threshold=256 is no byte value"),
    ("fk_mask_bbox_u8", dict(threshold=-1), "threshold=-1 is no byte value"),
    ("fk_mask_bbox_u8", dict(ws_ints=4 * 4096 - 1), "workspace of 16383 ints, needs fk_mask_bbox_ws_ints() = 16384"),
    ("fk_mask_bbox_u8", dict(ws_ints=0), "workspace of 0 ints"),
    ("fk_mask_bbox_u8", dict(out4=2 * A + 2), ": alignment"), ("fk_mask_bbox_u8", dict(ws=3 * A + 1), ": alignment"),
    ("fk_mask_bbox_u8", dict(ws=2 * A), ": alignment"),
    ("fk_mask_blur_u8", dict(src=0), "bad arguments"), ("fk_mask_blur_u8", dict(dst=0), "bad arguments"),
    ("fk_mask_blur_u8", dict(plane=0), "bad arguments"), ("fk_mask_blur_u8", dict(taps=0), "bad arguments"),
    ("fk_mask_blur_u8", dict(Bm=0), "bad arguments"), ("fk_mask_blur_u8", dict(H=0), "bad arguments"),
    ("fk_mask_blur_u8", dict(W=0), "bad arguments"),
    ("fk_mask_blur_u8", dict(R=-1), "R=-1 is outside [0, 192]"), ("fk_mask_blur_u8", dict(R=193), "R=193 is outside [0, 192]"),
    ("fk_mask_blur_u8", dict(plane=3 * A + 2), ": alignment"), ("fk_mask_blur_u8", dict(taps=4 * A + 2), ": alignment"),
    ("fk_mask_blur_u8", dict(plane=A), "the plane must be a buffer of its own"),
    ("fk_mask_blur_u8", dict(plane=2 * A), "the plane must be a buffer of its own"),
    ("fk_mask_blur_u8", dict(taps=3 * A), "the plane must be a buffer of its own"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(src=0), "bad arguments"), ("fk_pixels_u8_box_to_nhwc_bf16", dict(dst=0), "bad arguments"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(B=0), "bad arguments"), ("fk_pixels_u8_box_to_nhwc_bf16", dict(Hin=0), "bad arguments"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(Win=0), "bad arguments"), ("fk_pixels_u8_box_to_nhwc_bf16", dict(Hout=0), "bad arguments"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(Wout=0), "bad arguments"), ("fk_pixels_u8_box_to_nhwc_bf16", dict(Cpad=2), "bad arguments"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(x0=-1), "box (-1, 3, 67, 37) is empty or outside the 67 x 37 picture"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(y0=-1), "box (5, -1, 67, 37) is empty or outside"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(x1=68), "box (5, 3, 68, 37) is empty or outside"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(y1=38), "box (5, 3, 67, 38) is empty or outside"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(x1=5), "box (5, 3, 5, 37) is empty or outside"),
    ("fk_pixels_u8_box_to_nhwc_bf16", dict(y0=37), "box (5, 37, 67, 37) is empty or outside"),
    ("fk_image_overlay_u8", dict(img=0), "bad arguments"), ("fk_image_overlay_u8", dict(orig=0), "bad arguments"),
    ("fk_image_overlay_u8", dict(dst=0), "bad arguments"), ("fk_image_overlay_u8", dict(B=0), "bad arguments"),
    ("fk_image_overlay_u8", dict(h=0), "bad arguments"), ("fk_image_overlay_u8", dict(w=0), "bad arguments"),
    ("fk_image_overlay_u8", dict(H=0), "bad arguments"), ("fk_image_overlay_u8", dict(W=0), "bad arguments"),
    ("fk_image_overlay_u8", dict(orig_batch=2), "2 original pictures for a batch of 3"),
    ("fk_image_overlay_u8", dict(orig_batch=0), "0 original pictures for a batch of 3"),
    ("fk_image_overlay_u8", dict(alpha_batch=2), "alpha_batch=2 is neither 1 nor the batch 3"),
    ("fk_image_overlay_u8", dict(alpha_batch=0), "alpha_batch=0 is neither 1 nor the batch 3"),
    ("fk_image_overlay_u8", dict(alpha=0), "alpha_batch=3 is neither 1 nor the batch 3 (0 without alpha)"),
    ("fk_image_overlay_u8", dict(x1=68), "box (5, 3, 68, 37) is empty or outside the 67 x 37 picture"),
    ("fk_image_overlay_u8", dict(x0=67), "box (67, 3, 67, 37) is empty or outside"),
    ("fk_image_overlay_u8", dict(y0=-2), "box (5, -2, 67, 37) is empty or outside"),
    ("fk_image_overlay_u8", dict(y1=38), "box (5, 3, 67, 38) is empty or outside"),
    ("fk_image_overlay_u8", dict(dst=2 * A), "dst must be a buffer of its own"),
    ("fk_image_overlay_u8", dict(dst=3 * A), "dst must be a buffer of its own"),
    ("fk_image_overlay_u8", dict(dst=A), "dst must be a buffer of its own"),
    ("fk_image_overlay_u8", dict(img=A + 1), ": alignment"), ("fk_image_overlay_u8", dict(img=A + 2, img_is_fp32=1), ": alignment"),
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
