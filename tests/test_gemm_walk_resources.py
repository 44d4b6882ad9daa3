"""Register / scratch budget of the tile-walk GEMM kernels (gemm_walk_kernel of csrc/gemm_pingpong_bf16.hip), read from the
code hipcc generates for gfx950 (no GPU needed), the way tests/test_kernel_resources.py reads the other large-tile kernels.

The walk holds a tile's K loop, the next tile's address arithmetic and the epilogue inside ONE loop.  Whatever hipcc hoists out
of that loop lives across all of it, and the epilogue's batches already fill the 256 registers of two waves per SIMD: the
kernels derive every per-lane value from an opaque thread id and recompute the next tile's request offsets behind the epilogue
so that NOTHING goes through scratch -- no private segment, no spilled VGPR, in any of the 28 instantiations (7 epilogues x
pure / mixed grid x two MFMA shapes).  The K loops must also keep their counted waits: no wait for ALL vector-memory requests
inside them (the LDS-DMA prefetch is in flight there), and the tile hand-over must not wait for them either (the next tile's
K-tile 0 and this tile's stores are in flight): where the epilogue reads nothing but the bias, the whole kernel holds exactly
the waits for all requests that its source names.
"""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpt_image_edit_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_walk_kernels_use_no_scratch_and_keep_counted_waits(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "gemm_pingpong_bf16.s"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-unused-result", "-S",
           "--cuda-device-only", os.path.join(CSRC, "gemm_pingpong_bf16.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900)
    text = out.read_text()
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                      r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    walk = [(n, int(s), int(v), int(sp)) for n, s, v, sp in meta if "gemm_walk_kernel" in n]
    assert len(walk) == 28, f"expected 7 epilogues x pure / mixed x 2 MFMA shapes, got {len(walk)}"
    for name, scratch, vgprs, spills in walk:
        assert vgprs <= 256, f"{name}: {vgprs} VGPRs"      # two waves per SIMD
        assert scratch == 0 and spills == 0, f"{name}: {scratch} B of scratch per lane, {spills} spilled VGPRs"
    lines = text.split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_ZN12_GLOBAL__N_116gemm_walk_kernel\w+:", l)]
    assert len(starts) == 28
    for a in starts:
        e = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        body = lines[a:e]
        assert not any("scratch_" in l for l in body), f"{lines[a][:80]}: scratch traffic"
        labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
        loops = []
        for i, l in enumerate(body):
            m = re.search(r"(?:s_cbranch_\w+|s_branch) (\.LBB\d+_\d+)", l)
            if m and m.group(1) in labels and labels[m.group(1)] < i:
                n_mfma = sum("v_mfma" in x for x in body[labels[m.group(1)]:i])
                if n_mfma >= 32:
                    loops.append((labels[m.group(1)], i, n_mfma))
        assert loops, f"{lines[a][:80]}: no loop with MFMAs found"
        # the K loops: the multiplying loops that store nothing to global memory (every back edge of the tile loop around them
        # spans an epilogue, i.e. stores)
        k_loops = [t for t in loops if not any(re.search(r"\b(global|buffer|flat)_store", x) for x in body[t[0]:t[1]])]
        mixed = "ELb1ELb" in lines[a]          # <EPI, MIX, M16>
        assert len(k_loops) >= (2 if mixed else 1) and len(k_loops) < len(loops), f"{lines[a][:80]}: K loops {k_loops} of {loops}"
        for lo, hi, _ in k_loops:
            assert not any("vmcnt(0)" in x for x in body[lo:hi]), f"{lines[a][:80]}: s_waitcnt vmcnt(0) inside a K loop"
        # The hand-over must not wait for the next tile's requests before the epilogue's arithmetic has covered their latency.
        # Epilogues that read global memory only for the bias (none, GELU, SiLU, scale: template argument EPI = 0, 1, 2, 5) load
        # it IN FRONT of those requests, so hipcc's waits for it count past them; the kernel then holds exactly the waits for ALL
        # vector-memory requests that its source names: one behind each K loop (the surplus requests), one in each epilogue's
        # first pass in front of its first store (the next tile's K-tile 0 has landed before a store is in flight, so no later
        # wait counts past stores), one at the kernel's end (the last tile's repeated requests).  One more would be a wait hipcc
        # added -- what it does when the requests sit under a branch (it happened twice while this kernel was written).  The
        # residual, gate and rotary-table loads of the other epilogues are younger than the requests and wait for them anyway.
        if re.search(r"gemm_walk_kernelILi[0125]E", lines[a]):
            n_all = sum(1 for x in body if re.search(r"s_waitcnt.*vmcnt\(0\)", x))
            assert n_all == (5 if mixed else 3), f"{lines[a][:80]}: {n_all} waits for all vector-memory requests"
        # and no wait of the kernel counts past a store: the furthest any counts is hipcc's own wait for the first of the 8 bias
        # loads with the other 7 and the 8 requests behind it (15); nothing depends on how many stores hipcc emits
        counts = [int(m.group(1)) for x in body for m in [re.search(r"s_waitcnt.*vmcnt\((\d+)\)", x)] if m]
        assert max(counts) <= 15, f"{lines[a][:80]}: a wait for all but {max(counts)} requests"
