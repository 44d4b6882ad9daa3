"""Host-side checks (no GPU) of the MXFP8-output attention forward: the generated code of its kernels, the hazard census that the
build runs over them, the ctypes view of its destination struct and the transformer's switch."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpt_image_edit_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _census():
    spec = importlib.util.spec_from_file_location("a4_census", os.path.join(ROOT, "tools", "a4_census.py"))
    census = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(census)
    return census


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("a4") / "attention_fwd4.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-Wno-unused-value", "-Wno-unused-result",
           "-S", "--cuda-device-only", os.path.join(CSRC, "attention_fwd4.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return str(out)


def test_census_walks_the_mx_kernels_and_names_a_missing_one(assembly, tmp_path, capsys):
    census = _census()
    names = [n for _, n in census.KERNELS]
    assert len(names) == 4 and sum("attention_fwd4_mx_kernel" in n for n in names) == 2
    assert census.check(assembly) == 0
    # the same file without the stream-K mx kernel: the check fails and says which kernel it could not find (no exception)
    text = open(assembly).read()
    gone = [n for n in names if "mx_kernelILb1E" in n][0]
    cut = tmp_path / "cut.s"
    cut.write_text(text.replace(gone + ":", "removed:"))
    capsys.readouterr()
    assert census.check(str(cut)) == 1
    err = capsys.readouterr().err
    assert gone in err and "is not in" in err


def test_mx_kernels_keep_the_bf16_kernels_resources_and_steady_loop(assembly):
    """The MXFP8 form differs from the bf16 kernel in `finalize` only: its tile loop must be as clean (64-MFMA bodies without AGPR
    copies, scratch traffic or a wait for all vector-memory requests), every asm chain >= 12 states from its reader, and registers /
    scratch / spills within what the bf16 kernel of the same grid form has."""
    census = _census()
    text = open(assembly).read()
    meta = {name: (int(scratch), int(vgprs), int(spills)) for name, scratch, vgprs, spills in re.findall(
        r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)}
    by_tag = dict(census.KERNELS)
    for tag in ("ILb0E", "ILb1E"):
        bf, mx = meta[by_tag[tag]], meta[by_tag["mx " + tag]]
        assert mx[1] <= 512 and mx[0] <= bf[0] and mx[2] <= bf[2], f"{tag}: (scratch, VGPRs, spills) mx {mx} against bf16 {bf}"
        body = census.kernel_body(text, by_tag["mx " + tag])
        chains = steady = 0
        for lab, ins in census.blocks_of(body):
            n_mfma = sum(x.startswith("v_mfma") for x in ins)
            if n_mfma < 32:
                continue
            for at, states, reader in census.hazard_distances(ins):
                chains += 1
                assert states >= 12, f"mx {tag} {lab}: {states} states between the chain's last MFMA (#{at}) and `{reader}`"
            if n_mfma == 64 and not any("accvgpr" in x or "scratch_" in x or "vmcnt(0)" in x for x in ins):
                steady += 1
        assert chains >= 8 and steady >= 1, f"mx {tag}: {chains} asm chains, {steady} clean 64-MFMA tile bodies"


def test_destination_struct_matches_the_header(tmp_path):
    from gpt_image_edit_amd import libfk
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fk.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(fk_attn_mx_out), '
                   'offsetof(fk_attn_mx_out, q_b), offsetof(fk_attn_mx_out, split), offsetof(fk_attn_mx_out, ldq_scale));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A = libfk.AttnMxOut
    assert got == [ctypes.sizeof(A), A.q_b.offset, A.split.offset, A.ldq_scale.offset]


def test_switch_travels_as_bit_1_only_with_the_fused_schedule():
    from gpt_image_edit_amd import ops, transformer
    saved = transformer.MX_FUSED_QUANT, transformer.MX_FUSED_ATTN
    try:
        e0 = ops.launch_config_epoch()
        transformer.set_mx_fused_attn(True)
        assert ops.launch_config_epoch() == e0 + 1
        transformer.MX_FUSED_QUANT = False
        assert transformer._mx_fused_bits() == 0          # no effect without the fused schedule
        transformer.MX_FUSED_QUANT = True
        assert transformer._mx_fused_bits() == 3
        transformer.set_mx_fused_attn(False)
        assert transformer._mx_fused_bits() == 1 and ops.launch_config_epoch() == e0 + 2
    finally:
        transformer.MX_FUSED_QUANT, transformer.MX_FUSED_ATTN = saved
