"""Do kernel files still compile to the same gfx950 code as in an earlier commit?

Extracts gpt_image_edit_amd/csrc and include/ of a git revision into a scratch directory, compiles the named .hip files from
that tree and from the working tree with the build's flags (-S, device only) and compares the generated assembly, ignoring the
per-compilation `__hip_cuid_*` symbol.  Used when a shared header moves or grows (gemm_epilogue.h): the bf16 GEMM kernels must
not notice.  Without --rev: the parent of the commit that added csrc/mxfp8_quant.h (HEAD while that file is uncommitted).

    python tools/codeobj_parent_diff.py [--rev REV] [gemm_pingpong_bf16.hip gemm_bf16.hip]

Exit status 0: every file identical; 1: differences (first differing lines are printed); 2: no git history to compare with."""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("gpt_image_edit_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-unused-result", "-S", "--cuda-device-only"]


def git(*args):
    return subprocess.run(["git", "-C", ROOT] + list(args), capture_output=True, text=True)


def default_rev():
    added = git("log", "--diff-filter=A", "--format=%H", "--", os.path.join(CSRC, "mxfp8_quant.h")).stdout.split()
    return added[-1] + "^" if added else "HEAD"


def extract(rev, dest):
    """csrc/ and include/ of `rev` under dest (same relative layout: the sources include ../../include/fk.h)."""
    r = git("ls-tree", "-r", "--name-only", rev, CSRC, "include")
    if r.returncode != 0 or not r.stdout.strip():
        return False
    for path in r.stdout.split():
        out = os.path.join(dest, path)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "wb") as f:
            f.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{path}"], capture_output=True, check=True).stdout)
    return True


def assembly(tree, name, out):
    subprocess.run([HIPCC] + FLAGS + [os.path.join(tree, CSRC, name), "-o", out], check=True, capture_output=True, timeout=900)
    return [l for l in open(out).read().split("\n") if "__hip_cuid_" not in l]


def compare(rev, files, scratch):
    if not extract(rev, os.path.join(scratch, "parent")):
        return None
    jobs = {}
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        for name in files:
            for which, tree in (("parent", os.path.join(scratch, "parent")), ("tree", ROOT)):
                jobs[(name, which)] = ex.submit(assembly, tree, name, os.path.join(scratch, f"{which}_{name}.s"))
    result = {}
    for name in files:
        a, b = jobs[(name, "parent")].result(), jobs[(name, "tree")].result()
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
        kernels = sum(bool(re.match(r"\s+\.amdhsa_kernel ", l)) for l in b)
        result[name] = (first, kernels, a, b)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev")
    ap.add_argument("files", nargs="*", default=["gemm_pingpong_bf16.hip", "gemm_bf16.hip"])
    args = ap.parse_args()
    rev = args.rev or default_rev()
    with tempfile.TemporaryDirectory() as scratch:
        res = compare(rev, args.files, scratch)
        if res is None:
            print(f"no git revision {rev} to compare with")
            return 2
        bad = 0
        for name, (first, kernels, a, b) in res.items():
            if first is None:
                print(f"{name}: {kernels} kernels, {len(b)} lines of assembly identical to {rev}")
            else:
                bad = 1
                print(f"{name}: differs from {rev} at line {first + 1}:\n  - {a[first] if first < len(a) else '<end>'}\n"
                      f"  + {b[first] if first < len(b) else '<end>'}")
        return bad


if __name__ == "__main__":
    sys.exit(main())
