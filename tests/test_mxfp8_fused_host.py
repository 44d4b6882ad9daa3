"""CPU checks of the MXFP8 producers that emit quantized activations (fk_ln_modulate(2)_mxfp8, fk_gemm_mxfp8_q): the ABI
boundary, and the code hipcc generates for gfx950 -- the new kernels keep everything in registers, and the kernels that share
headers with them did not change."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpt_image_edit_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = {"fk_ln_modulate_mxfp8": 14, "fk_ln_modulate2_mxfp8": 19, "fk_gemm_mxfp8_q": 2, "fk_gemm_mxfp8_q_grouped": 3}


def test_new_entry_points_are_declared_bound_and_exported():
    from gpt_image_edit_amd import libfk
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = libfk.load()
    exported = subprocess.run(["nm", "-D", "--defined-only", libfk.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, arity in NEW.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/fk.h"
        assert len(m.group(1).split(",")) == arity, f"{name}: {len(m.group(1).split(','))} parameters declared"
        assert name in libfk.SIGNATURES and len(libfk.SIGNATURES[name][1]) == arity, f"{name}: ctypes signature"
        assert hasattr(lib, name) and re.search(r" T " + name + r"$", exported, flags=re.M), f"{name} is not exported"


def test_new_struct_layouts_match_header():
    from gpt_image_edit_amd import libfk
    qf = ["a", "Q", "ldq", "Q_scale", "ldq_scale", "col_offset"]
    wf = ["q", "s", "q_bytes", "s_bytes", "fused", "quantize_launches"]
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "fk.h"\nint main(){printf("%zu %zu", sizeof(fk_gemm_mxfp8_q_args), sizeof(fk_mx_ws));'
            + "".join(f'printf(" %zu", offsetof(fk_gemm_mxfp8_q_args, {f}));' for f in qf)
            + "".join(f'printf(" %zu", offsetof(fk_mx_ws, {f}));' for f in wf) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")], check=True)
        got = [int(x) for x in subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()]
    Q, W = libfk.GemmMxfp8QArgs, libfk.MxWs
    assert got == [ctypes.sizeof(Q), ctypes.sizeof(W)] + [getattr(Q, f).offset for f in qf] + [getattr(W, f).offset for f in wf]
    # a workspace struct built the way callers of the unfused entry points always built it selects the unfused schedule
    assert libfk.MxWs(1, 2, 3, 4).fused == 0


def test_ops_and_switch_exist_without_a_gpu():
    import torch
    from gpt_image_edit_amd import ops, transformer
    assert isinstance(transformer.MX_FUSED_QUANT, bool)
    assert ops.quantize_launch_count() >= 0
    x = torch.zeros(1, 4, 3072, dtype=torch.bfloat16)
    m = torch.zeros(1, 3072, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ln_modulate_mxfp8(x, m, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ln_modulate2_mxfp8(x, m, m, m, m, 2)
    q = (torch.zeros(4, 128, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gemm_mxfp8(q, q, out_mx=True)


def _metadata(src, tmp_path, extra=()):
    out = tmp_path / (src + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-unused-result", "-S",
                    "--cuda-device-only", *extra, os.path.join(CSRC, src), "-o", str(out)], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                      r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    return text, {n: (int(s), int(v), int(sp)) for n, s, v, sp in meta}


def test_new_kernels_stay_in_registers_and_the_existing_mxfp8_kernels_keep_their_budget(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    _, meta = _metadata("gemm_mxfp8.hip", tmp_path)
    mxq = {n: m for n, m in meta.items() if "gemm_mxq_kernel" in n}
    assert len(mxq) == 4, f"expected NONE / GELU x two tile widths of gemm_mxq_kernel, got {sorted(mxq)}"
    for n, (scratch, vgprs, spills) in mxq.items():
        assert scratch == 0 and spills == 0 and vgprs <= 256, f"{n}: {scratch} B scratch, {spills} spills, {vgprs} VGPRs"
    old = {n: m for n, m in meta.items() if "gemm_mxfp8_kernel" in n}
    assert len(old) == 10
    for n, (scratch, vgprs, spills) in old.items():
        # the fused-QKV 256 x 128 form took 144 while its RoPE was a product and an fma; 142 with both products rounded (mul2_add)
        want = 220 if "ELi256EEE" in n else (142 if "ILi6ELi128" in n else 132)
        assert (scratch, spills, vgprs) == (0, 0, want), f"{n}: {scratch} B scratch, {spills} spills, {vgprs} VGPRs (was {want})"
    _, ln = _metadata("norm_kernels.hip", tmp_path)
    lnmx = {n: m for n, m in ln.items() if "ln_modulate_mx_kernel" in n}
    assert len(lnmx) == 3 and len([n for n in ln if "ln_modulate_kernel" in n]) == 3
    for n, (scratch, vgprs, spills) in {**lnmx, **{n: m for n, m in ln.items() if "ln_modulate_kernel" in n}}.items():
        assert scratch == 0 and spills == 0 and vgprs <= 128, f"{n}: {scratch} B scratch, {spills} spills, {vgprs} VGPRs"


@pytest.mark.timeout(1800)
def test_bf16_gemm_kernels_compile_to_the_parent_commits_code(tmp_path):
    """gemm_epilogue.h gained store_tile_mxq and an include: gemm_pingpong_bf16.hip / gemm_bf16.hip must generate the same
    assembly as in the commit before the quantizer header existed (tools/codeobj_parent_diff.py builds that commit's sources in
    a scratch directory).  Without git history (an exported tree) the comparison is against gemm_epilogue.h with the addition
    cut out again, which is the same text."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("codeobj_parent_diff", os.path.join(ROOT, "tools", "codeobj_parent_diff.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    files = ["gemm_pingpong_bf16.hip", "gemm_bf16.hip"]
    res = tool.compare(tool.default_rev(), files, str(tmp_path)) if os.path.exists(os.path.join(ROOT, ".git")) else None
    if res is None:
        parent = tmp_path / "cut"
        shutil.copytree(os.path.join(ROOT, "include"), parent / "include")
        shutil.copytree(CSRC, parent / "gpt_image_edit_amd" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.s"))
        hdr = parent / "gpt_image_edit_amd" / "csrc" / "gemm_epilogue.h"
        text = hdr.read_text()
        cut = re.sub(r'#include "mxfp8_quant.h".*\n', "", text[:text.index("// Quantized-output epilogue")])
        assert "store_tile_mxq" not in cut and "mxfp8_quant" not in cut
        hdr.write_text(cut)
        res = {}
        for name in files[:1]:
            a = tool.assembly(str(parent), name, str(tmp_path / ("cut_" + name + ".s")))
            b = tool.assembly(ROOT, name, str(tmp_path / ("tree_" + name + ".s")))
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
            res[name] = (first, 0, a, b)
    for name, (first, _, a, b) in res.items():
        assert first is None, f"{name}: generated code changed at assembly line {first + 1}: {a[first][:100]!r} -> {b[first][:100]!r}"
        assert len(b) > 1000
