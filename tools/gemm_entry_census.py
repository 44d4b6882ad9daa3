"""Census of the workgroup entry of the large-tile GEMM kernels from hipcc -S output (no GPU): what executes between a
kernel's first instruction and its first LDS-DMA request (`buffer_load_dwordx4 ... lds`), in the order of the text --
instructions, scalar loads, groups of scalar loads that end in an `s_waitcnt lgkmcnt(0)` (each group depends on the one
before it: a serial round trip through the kernel arguments), reciprocal division sequences (`v_rcp*`) and branches.
  python tools/gemm_entry_census.py gemm.s            the table for the four flagship instantiations
  python tools/gemm_entry_census.py --check gemm.s    exit status 1 unless every one of them has <= 2 wait groups and no v_rcp*
The counts follow the TEXT: they describe the path hipcc lays out first.  For these kernels that is the flat-rows path -- the
batched addressing of A (one 32-bit division, a reciprocal and a further fetch of p[pi].a) is a cold block placed behind the
first request's block and is not counted -- and in gemm_mix_kernel the branch (256 x 256 or 256 x 128 body) that comes first.
"<= 2 wait groups, no v_rcp*" is therefore a statement about the flat path; a change of block layout by the compiler shows up
as a changed count, which is what the test that runs this is for.
The assembly: hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only csrc/gemm_pingpong_bf16.hip (csrc/Makefile's flags)."""
import re
import sys

# (label, fragment of the mangled name): template arguments <EPI, BN, SPLITK, LAY, M16> / <EPI, M16> / <EPI, BN, M16>
KERNELS = [
    ("gemm8_kernel<1,256,false,0,true> (MLP-up)", "12gemm8_kernelILi1ELi256ELb0ELi0ELb1EE"),
    ("gemm8_kernel<3,256,true,0,true> (split-K pairs)", "12gemm8_kernelILi3ELi256ELb1ELi0ELb1EE"),
    ("gemm_mix_kernel<6,true> (fused QKV)", "15gemm_mix_kernelILi6ELb1EE"),
    ("gemm9_kernel<3,128,true> (out-projection)", "12gemm9_kernelILi3ELi128ELb1EE"),
]
MAX_WAIT_GROUPS = 2


def kernel_body(text, frag):
    """Instructions of the kernel whose mangled name contains `frag`, or None when the file does not define it."""
    m = re.search(r"^(_ZN12_GLOBAL__N_1%s\w*):.*\n" % re.escape(frag), text, re.M)
    if not m:
        return None
    body = text[m.end():text.index(".Lfunc_end", m.end())]
    return [l.strip() for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]


def entry_census(ins):
    """Counts over the instructions in front of the first LDS-DMA request."""
    c = {"instructions": 0, "s_load": 0, "wait_groups": 0, "v_rcp": 0, "branches": 0}
    pending = False      # a scalar load was issued since the last lgkmcnt(0)
    for x in ins:
        if x.startswith("buffer_load_dword") and x.endswith(" lds"):
            return c
        c["instructions"] += 1
        if x.startswith("s_load_") or x.startswith("s_buffer_load_"):
            c["s_load"] += 1
            pending = True
        elif x.startswith("s_waitcnt") and ("lgkmcnt(0)" in x or re.match(r"s_waitcnt \d+$", x)):
            if pending:
                c["wait_groups"] += 1
            pending = False
        elif x.startswith("v_rcp"):
            c["v_rcp"] += 1
        elif x.startswith(("s_cbranch", "s_branch")):
            c["branches"] += 1
    raise ValueError("no LDS-DMA request in the kernel")


def census(text):
    out = []
    for label, frag in KERNELS:
        ins = kernel_body(text, frag)
        out.append((label, None if ins is None else entry_census(ins)))
    return out


def main(argv):
    check = "--check" in argv
    paths = [a for a in argv if not a.startswith("--")]
    if len(paths) != 1:
        print(__doc__)
        return 2
    rows = census(open(paths[0]).read())
    bad = 0
    print("%-52s %6s %7s %6s %6s %8s" % ("kernel", "instr", "s_load", "waits", "v_rcp", "branches"))
    for label, c in rows:
        if c is None:
            print("%-52s not found" % label)
            bad += 1
            continue
        print("%-52s %6d %7d %6d %6d %8d" % (label, c["instructions"], c["s_load"], c["wait_groups"], c["v_rcp"], c["branches"]))
        if c["wait_groups"] > MAX_WAIT_GROUPS or c["v_rcp"]:
            bad += 1
    return 1 if (check and bad) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
