"""CPU test of the edit-weight entries' boundary (the pattern of tests/test_abi_mask_ops.py): include/fk.h declares them, the library
exports them, libfk.py has their prototypes argument by argument, ops wraps them -- and every refusal is made on the host before
anything is launched, so its error string can be read here, without a GPU, from calls that pass made-up addresses."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {
    "fk_edit_diff_mask_u8": ["ref", "ref_batch_stride", "tgt", "dst", "N", "H", "W", "threshold", "stream"],
    "fk_mask_close5_u8": ["src", "dst", "N", "H", "W", "stream"],
    "fk_mask_filter_components_u8": ["src", "dst", "N", "H", "W", "keep_num", "keep_den", "ws", "ws_bytes", "stream"],
    "fk_mask_components_status": ["ws", "stream"],
    "fk_mask_and_pool8_u8": ["masks", "B", "R", "H", "W", "pooled", "mask_ds", "counts", "status", "stream"],
    "fk_mask_weight_fill_f32": ["mask_ds", "w", "dst", "B", "h", "wd", "stream"],
}
POINTERS = {"ref", "tgt", "dst", "src", "ws", "masks", "pooled", "mask_ds", "counts", "status", "w", "stream"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def _lib():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return libfk.load()


@pytest.mark.parametrize("name", list(ARGS) + ["fk_mask_components_ws_bytes"])
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
             "int32_t*": libfk.c_vp, "const int32_t*": libfk.c_vp, "fk_stream_t": libfk.c_vp, "int64_t": libfk.c_i64,
             "int32_t": libfk.c_i32}
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


def test_workspace_size_limits_and_the_bound_code():
    from gpt_image_edit_amd import libfk
    lib = _lib()
    assert libfk.SIGNATURES["fk_mask_components_ws_bytes"] == (libfk.c_i64, [libfk.c_i32] * 3)
    assert lib.fk_mask_components_ws_bytes(3, 37, 53) == 4 * (1 + 3 + 2 * 3 * 37 * 53)     # status, white counts, labels, areas
    assert lib.fk_mask_components_ws_bytes(127, 4096, 4096) == 4 * (1 + 127 + 2 * 127 * 4096 * 4096)
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 4097), (128, 4096, 4096)):
        assert lib.fk_mask_components_ws_bytes(*bad) == 0
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    assert re.search(r"#define FK_EDIT_MASK_MAX_SIDE 4096\b", text) and re.search(r"#define FK_MASK_CLOSE_TILE 32\b", text)
    assert re.search(r"FK_EBOUND = -4,", text)


def test_the_documents_carry_the_parity_statement_and_a_timing_status():
    for name in ("README.md", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "parity with OpenCV is unpinned" in text and "TIMING_STATUS" not in text, name
        recorded = os.path.exists(os.path.join(ROOT, "profiles", "edit_weights.json"))
        assert recorded or "Timing: unmeasured" in text, name                # no figure without a recorded run


def test_the_rules_are_the_declarations_comments():
    text = open(os.path.join(ROOT, "include", "fk.h")).read()
    block = text[text.index("Edit-region loss weights"):text.index("int fk_mask_weight_fill_f32")]
    for words in ("parity with OpenCV is unpinned", "pinned to the installed Pillow", "cross-checked against scipy",
                  "grey = (19595 d_R + 38470 d_G + 7471 d_B + 32768) >> 16", "255 iff grey >= threshold",
                  "00100 / 11111 / 11111 / 11111 / 00100", "dilation first", "never dilates and never erodes", "8-connectivity",
                  "planes never connect", "keep_den * area >= keep_num * (white pixels of its plane)", "not H * W",
                  "the component is kept", "atomicMin", "Two launches give the same bytes", "Every loop has a bound",
                  "never a hang", "FK_EBOUND", "white iff it is >= 128", "the all-white plane takes its place", "floor sizes",
                  "counts[b, 1]", "1.0f elsewhere", "FK_EINVAL", "writes nothing", "N * H * W < 2^31"):
        assert words in block, words


def test_ops_wrappers_and_the_export():
    import torch
    import gpt_image_edit_amd
    from gpt_image_edit_amd import edit_weights, ops
    assert gpt_image_edit_amd.edit_region_weights is edit_weights.edit_region_weights
    sig = {n: list(inspect.signature(getattr(ops, n)).parameters)
           for n in ("edit_diff_mask", "mask_close5", "mask_filter_components", "mask_and_pool8", "mask_weight_fill")}
    assert sig["edit_diff_mask"][:3] == ["ref_u8", "tgt_u8", "threshold"] and sig["mask_close5"][:1] == ["mask"]
    assert sig["mask_filter_components"][:3] == ["mask", "keep_num", "keep_den"] and sig["mask_and_pool8"][:1] == ["masks"]
    assert sig["mask_weight_fill"][:2] == ["mask_ds", "w"]
    assert inspect.signature(ops.edit_diff_mask).parameters["threshold"].default == 18
    assert [inspect.signature(ops.mask_filter_components).parameters[k].default for k in ("keep_num", "keep_den")] == [3, 10]
    pic, m = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda: ops.edit_diff_mask(pic, pic), lambda: ops.mask_close5(m), lambda: ops.mask_filter_components(m),
                 lambda: ops.mask_and_pool8(m[None]), lambda: ops.mask_weight_fill(m, torch.ones(1))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):        # a missing GPU is an error, not another path
            call()


def test_the_kernels_are_integer_and_every_loop_is_bounded():
    src = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "edit_weights.hip")).read()
    for name in ARGS:
        assert 'extern "C" int ' + name in src
    kernels = src[src.index("namespace {"):src.index("}  // namespace")]
    assert "while" not in kernels and "for (;;" not in kernels and "goto" not in kernels
    heads = re.findall(r"\bfor \((.*)\) ?\{?$", kernels, flags=re.M)
    assert len(heads) >= 20 and all(re.search(r"; [^;]*<[^;]*;", h) for h in heads), heads   # every for compares with its bound
    device = kernels[:kernels.index("inline bool sizes_ok")]
    assert "double" not in device and "fmul" not in device and device.count("float") == 2     # E5's w, dst and nothing else


# ---- the refusals: host checks before any launch ----------------------------------------------------------------------------------
A = 0x10000          # made-up addresses, 16-byte aligned and distinct; a refused call dereferences none of them
GOOD = {
    "fk_edit_diff_mask_u8": dict(ref=A, ref_batch_stride=2 * 37 * 53 * 3, tgt=2 * A, dst=3 * A, N=2, H=37, W=53, threshold=18, stream=0),
    "fk_mask_close5_u8": dict(src=A, dst=2 * A, N=2, H=37, W=53, stream=0),
    "fk_mask_filter_components_u8": dict(src=A, dst=2 * A, N=2, H=37, W=53, keep_num=3, keep_den=10, ws=3 * A,
                                         ws_bytes=4 * (1 + 2 + 4 * 37 * 53), stream=0),
    "fk_mask_components_status": dict(ws=A, stream=0),
    "fk_mask_and_pool8_u8": dict(masks=A, B=2, R=2, H=37, W=53, pooled=2 * A, mask_ds=3 * A, counts=4 * A, status=5 * A, stream=0),
    "fk_mask_weight_fill_f32": dict(mask_ds=A, w=2 * A, dst=3 * A, B=2, h=4, wd=6, stream=0),
}
SIDES = "sides are 1..4096 and N * H * W < 2^31"
REFUSALS = [
    ("fk_edit_diff_mask_u8", dict(ref=0), "bad arguments"), ("fk_edit_diff_mask_u8", dict(tgt=0), "bad arguments"),
    ("fk_edit_diff_mask_u8", dict(dst=0), "bad arguments"),
    ("fk_edit_diff_mask_u8", dict(N=0), "0 planes of 37 x 53: " + SIDES), ("fk_edit_diff_mask_u8", dict(H=0), "2 planes of 0 x 53"),
    ("fk_edit_diff_mask_u8", dict(W=4097), "2 planes of 37 x 4097"), ("fk_edit_diff_mask_u8", dict(H=4097), "2 planes of 4097 x 53"),
    ("fk_edit_diff_mask_u8", dict(N=128, H=4096, W=4096), "128 planes of 4096 x 4096"),
    ("fk_edit_diff_mask_u8", dict(threshold=-1), "threshold=-1 is outside [0, 256]"),
    ("fk_edit_diff_mask_u8", dict(threshold=257), "threshold=257 is outside [0, 256]"),
    ("fk_edit_diff_mask_u8", dict(ref_batch_stride=37 * 53 * 3 - 1), "ref_batch_stride=5882 is less than a picture's 5883 bytes"),
    ("fk_edit_diff_mask_u8", dict(ref_batch_stride=0), "ref_batch_stride=0 is less than"),
    ("fk_edit_diff_mask_u8", dict(dst=A), "dst must be a buffer of its own"),
    ("fk_edit_diff_mask_u8", dict(dst=2 * A), "dst must be a buffer of its own"),
    ("fk_mask_close5_u8", dict(src=0), "bad arguments"), ("fk_mask_close5_u8", dict(dst=0), "bad arguments"),
    ("fk_mask_close5_u8", dict(N=0), "0 planes of 37 x 53: " + SIDES), ("fk_mask_close5_u8", dict(H=-1), "2 planes of -1 x 53"),
    ("fk_mask_close5_u8", dict(W=4097), "2 planes of 37 x 4097"),
    ("fk_mask_close5_u8", dict(N=128, H=4096, W=4096), "128 planes of 4096 x 4096"),
    ("fk_mask_close5_u8", dict(dst=A), "dst must be a buffer of its own"),
    ("fk_mask_filter_components_u8", dict(src=0), "bad arguments"), ("fk_mask_filter_components_u8", dict(dst=0), "bad arguments"),
    ("fk_mask_filter_components_u8", dict(ws=0), "bad arguments"),
    ("fk_mask_filter_components_u8", dict(N=0), "0 planes of 37 x 53: " + SIDES),
    ("fk_mask_filter_components_u8", dict(H=4097), "2 planes of 4097 x 53"),
    ("fk_mask_filter_components_u8", dict(W=0), "2 planes of 37 x 0"),
    ("fk_mask_filter_components_u8", dict(N=128, H=4096, W=4096), "128 planes of 4096 x 4096"),
    ("fk_mask_filter_components_u8", dict(keep_num=-1), "keep -1 / 10 is no fraction >= 0"),
    ("fk_mask_filter_components_u8", dict(keep_den=0), "keep 3 / 0 is no fraction >= 0"),
    ("fk_mask_filter_components_u8", dict(ws_bytes=4 * (1 + 2 + 4 * 37 * 53) - 1),
     "workspace of 31387 bytes, needs fk_mask_components_ws_bytes() = 31388"),
    ("fk_mask_filter_components_u8", dict(ws_bytes=0), "workspace of 0 bytes"),
    ("fk_mask_filter_components_u8", dict(ws=3 * A + 2), ": alignment"), ("fk_mask_filter_components_u8", dict(ws=A), "ws must be a buffer of its own"),
    ("fk_mask_filter_components_u8", dict(ws=2 * A), "ws must be a buffer of its own"),
    ("fk_mask_components_status", dict(ws=0), "bad arguments"), ("fk_mask_components_status", dict(ws=A + 2), "bad arguments"),
    ("fk_mask_and_pool8_u8", dict(masks=0), "bad arguments"), ("fk_mask_and_pool8_u8", dict(pooled=0), "bad arguments"),
    ("fk_mask_and_pool8_u8", dict(mask_ds=0), "bad arguments"), ("fk_mask_and_pool8_u8", dict(counts=0), "bad arguments"),
    ("fk_mask_and_pool8_u8", dict(R=0), "bad arguments"),
    ("fk_mask_and_pool8_u8", dict(B=0), "0 x 2 planes of 37 x 53: sides are 8..4096 and B * R * H * W < 2^31"),
    ("fk_mask_and_pool8_u8", dict(H=7), "2 x 2 planes of 7 x 53"), ("fk_mask_and_pool8_u8", dict(W=7), "2 x 2 planes of 37 x 7"),
    ("fk_mask_and_pool8_u8", dict(H=4097), "2 x 2 planes of 4097 x 53"),
    ("fk_mask_and_pool8_u8", dict(B=16, R=8, H=4096, W=4096), "16 x 8 planes of 4096 x 4096"),
    ("fk_mask_and_pool8_u8", dict(B=65536, H=8, W=8), "a batch of 65536 is more than 65535"),
    ("fk_mask_and_pool8_u8", dict(counts=4 * A + 2), ": alignment"), ("fk_mask_and_pool8_u8", dict(status=5 * A + 1), ": alignment"),
    ("fk_mask_and_pool8_u8", dict(pooled=3 * A), "pooled and mask_ds must be buffers of their own"),
    ("fk_mask_and_pool8_u8", dict(pooled=A), "pooled and mask_ds must be buffers of their own"),
    ("fk_mask_and_pool8_u8", dict(mask_ds=A), "pooled and mask_ds must be buffers of their own"),
    ("fk_mask_and_pool8_u8", dict(counts=2 * A), "pooled and mask_ds must be buffers of their own"),
    ("fk_mask_weight_fill_f32", dict(mask_ds=0), "bad arguments"), ("fk_mask_weight_fill_f32", dict(w=0), "bad arguments"),
    ("fk_mask_weight_fill_f32", dict(dst=0), "bad arguments"),
    ("fk_mask_weight_fill_f32", dict(B=0), "0 planes of 4 x 6: sides are 1..4096 and B * h * w < 2^31"),
    ("fk_mask_weight_fill_f32", dict(h=0), "2 planes of 0 x 6"), ("fk_mask_weight_fill_f32", dict(wd=4097), "2 planes of 4 x 4097"),
    ("fk_mask_weight_fill_f32", dict(w=2 * A + 2), ": alignment"), ("fk_mask_weight_fill_f32", dict(dst=3 * A + 1), ": alignment"),
    ("fk_mask_weight_fill_f32", dict(dst=A), "dst must be a buffer of its own"),
    ("fk_mask_weight_fill_f32", dict(dst=2 * A), "dst must be a buffer of its own"),
]


@pytest.mark.parametrize("name,change,message", REFUSALS,
                         ids=[n[3:18] + ":" + ",".join(f"{k}={v}" for k, v in c.items()) for n, c, _ in REFUSALS])
def test_refusal_and_its_error_string(name, change, message):
    lib = _lib()
    kw = dict(GOOD[name], **change)
    args = [ctypes.c_void_p(kw[n] or None) if n in POINTERS else kw[n] for n in ARGS[name]]
    assert getattr(lib, name)(*args) == -1                               # FK_EINVAL
    err = lib.fk_last_error().decode()
    assert err.startswith(name + ":") and message in err, err
