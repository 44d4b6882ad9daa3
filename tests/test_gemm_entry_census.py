"""Workgroup entry of the large-tile GEMM kernels, read from the code hipcc generates for gfx950 (no GPU needed).

tools/gemm_entry_census.py counts what the four flagship instantiations execute in front of their first LDS-DMA request.
Held here: at most two groups of scalar loads that end in a wait (the entry record, then the tile's problem record) and
no reciprocal division sequence.  The instruction counts are printed, not capped (DESIGN.md section 4 keeps them beside
the tool's counts for the kernels before the entry record existed: 7 - 8 dependent waits, 6 divisions, 492 - 498 instructions).
The counts follow the text up to the first request: the path hipcc lays out first, which is the flat-rows one (the batched
addressing is a cold block behind it) and, in the mixed kernel, the branch that comes first.
"""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpt_image_edit_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _census_module():
    spec = importlib.util.spec_from_file_location("gemm_entry_census", os.path.join(ROOT, "tools", "gemm_entry_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_census_counts_wait_groups_and_divisions():
    """The counting itself, on a hand-written entry: loads that share a wait are one group, a wait with nothing pending is
    none, everything behind the first LDS-DMA request is ignored."""
    census = _census_module()
    ins = ["s_load_dwordx4 s[4:7], s[0:1], 0x0", "s_load_dword s8, s[0:1], 0x10", "s_waitcnt lgkmcnt(0)", "s_mul_hi_u32 s9, s4, s5",
           "s_waitcnt lgkmcnt(0)", "s_load_dwordx8 s[12:19], s[0:1], s9 offset:0x110", "s_cbranch_scc1 .LBB0_2",
           "s_waitcnt vmcnt(0) lgkmcnt(0)", "v_rcp_iflag_f32_e32 v1, v2", "buffer_load_dwordx4 v3, s[8:11], s30 offen lds",
           "s_load_dword s20, s[0:1], 0x20", "s_waitcnt lgkmcnt(0)", "v_rcp_f32_e32 v1, v2"]
    c = census.entry_census(ins)
    assert c == {"instructions": 9, "s_load": 3, "wait_groups": 2, "v_rcp": 1, "branches": 1}


def test_flagship_kernels_reach_their_first_request_in_two_fetches(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    census = _census_module()
    out = tmp_path / "gemm_pingpong_bf16.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-unused-result", "-S",
           "--cuda-device-only", os.path.join(CSRC, "gemm_pingpong_bf16.hip"), "-o", str(out)]     # csrc/Makefile's flags
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    rows = census.census(out.read_text())
    assert len(rows) == 4
    for label, c in rows:
        assert c is not None, f"{label}: not in the generated code"
        print(f"[census] {label}: {c}", flush=True)
        assert c["wait_groups"] <= census.MAX_WAIT_GROUPS, f"{label}: {c['wait_groups']} dependent scalar-load waits before the first request"
        assert c["v_rcp"] == 0, f"{label}: a division sequence before the first request"
