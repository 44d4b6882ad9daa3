"""The tile walk of the large-tile GEMMs (csrc/gemm_tile_map.h: tm_walk_count, tm_walk_place, tm_mix_place, tm_fill_mix),
checked on the CPU: no GPU, no hipcc.

tests/gemm_walk_main.cpp is a stand-alone program (its own main).  For every (grid, G) of a sweep -- the flagship MLP-up and
fused-QKV grids, the small grids of tests/test_hip_gemm_walk.py, ragged and grouped ones; G from 1 to beyond the tile count,
multiples of 8 and not -- the lists of the G workgroups together hold every place of the launch exactly once, place b is entry
b / G of workgroup b % G (the order list scheduling gives a CU on the one-workgroup-per-tile launch), every place names the
tile that launch computes from blockIdx.x = place, the tiles named are all tiles of the problems, each once, and on a mixed
grid a workgroup whose places stay on one XCD never meets a 256 x 256 tile behind a 256 x 128 one -- nor does any other: no place
behind a small tile names a big one, so for every G a workgroup's list changes shape at most once.
`--places` prints a mixed launch's places for tests/test_gemm_large_host.py.
Built with -fsanitize=address,undefined where the host compiler links them.
"""
import os
import subprocess

from test_gemm_tile_map import _compiler

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gemm_walk_main.cpp")


def _build(cxx, out, sanitize):
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", SRC, "-o", out]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
        if "clang" not in os.path.basename(cxx):      # g++: runtimes linked in, so the program starts in any environment
            cmd[1:1] = ["-static-libasan", "-static-libubsan"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def test_walk_covers_every_tile_once_in_launch_order(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found (g++ / clang++ / $CXX)"
    exe = str(tmp_path / "gemm_walk_check")
    r = _build(cxx, exe, sanitize=True)
    # the start probe alone decides about the fallback: a sanitized program that starts is the one whose verdict counts, so a
    # sanitizer report in the real run fails the test instead of being replaced by the plain build's result
    sanitized = r.returncode == 0 and subprocess.run([exe, "--self-test"], capture_output=True, timeout=60).returncode == 0
    if not sanitized:      # no sanitizer runtimes, or a sanitized program cannot start here: the plain program checks the same things
        r = _build(cxx, exe, sanitize=False)
    assert r.returncode == 0, r.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print("sanitized build:", sanitized)
    print(run.stdout[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert " 0 failures" in run.stdout
