"""The large-tile GEMMs' tile order as launch constants (csrc/gemm_tile_map.h), checked on the CPU: no GPU, no hipcc.

tests/gemm_tile_map_main.cpp is a stand-alone program (its own main) that includes the header the kernels and the launcher
share and holds it against the device code it replaced, kept verbatim there:
  * the multiply-shift quotients equal `/` for every divisor 1 .. 4096 and every t < 65536 (and at the edge of the range the
    launcher accepts);
  * the (problem, m0, n0) of every workgroup equals the old tile_of / xcd_chunk_index formulas on the flagship grids
    (M = 2560 and grouped 2048 + 512 at N = 3072 / 9216 / 12288: both tile widths, split-K pairs, mixed grids with every
    big_cols) and on ragged ones (M = 300 / 520 / 700, N = 384 / 1280, group_m 1 / 8 / 64, 1 - 4 problems), and every tile
    is covered;
  * rows the launcher marks flat lie at m * ld for every m, against fk_row_offset, for batched and unbatched views.
Built with -fsanitize=address,undefined where the host compiler links them.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gemm_tile_map_main.cpp")
HEADER = os.path.join(os.path.dirname(HERE), "gpt_image_edit_amd", "csrc", "gemm_tile_map.h")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def _build(cxx, out, sanitize):
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", SRC, "-o", out]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
        if "clang" not in os.path.basename(cxx):      # g++: runtimes linked in, so the program starts in any environment
            cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_header_has_no_hip_dependency():
    text = open(HEADER).read()
    assert "#include <stdint.h>" in text and text.count("#include") == 1, "the header includes <stdint.h> and nothing else"
    assert "hip_runtime" not in text and "__device__" not in text and "threadIdx" not in text and "blockIdx" not in text


def test_tile_map_matches_the_division_forms(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found (g++ / clang++ / $CXX)"
    exe = str(tmp_path / "gemm_tile_map_check")
    r = _build(cxx, exe, sanitize=True)
    sanitized = r.returncode == 0 and subprocess.run([exe, "--self-test"], capture_output=True, timeout=60).returncode == 0
    if not sanitized:      # no sanitizer runtimes, or a sanitized program cannot start here: the plain program checks the same things
        r = _build(cxx, exe, sanitize=False)
    assert r.returncode == 0, r.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print("sanitized build:", sanitized)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert " 0 failures" in run.stdout
