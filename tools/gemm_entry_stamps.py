"""Where a large-tile GEMM workgroup's cycles go outside its K loop, from s_memtime stamps (diagnostic build only).

Needs a library built with -DFK_ENTRY_STAMPS (csrc/gemm_pingpong_bf16.hip: EntryStamps; never the shipped one):
    hipcc <the Makefile's flags> -DFK_ENTRY_STAMPS -c gemm_pingpong_bf16.hip -o pp_stamps.o, linked with the other objects
    FK_LIB_PATH=/path/to/libfk_stamps.so python tools/gemm_entry_stamps.py [label]
Wave 0 of every workgroup stamps (0) the kernel's first instruction, (1) behind its first LDS-DMA request, (2) in front of its
first MFMA phase, (3) the K loop's exit, (4) behind its last store.  The four flagship launch classes run at M = 2560 over a
ring of NRING weights (far beyond the 256 MiB Infinity Cache: every launch streams weights nobody touched, the method of
tools/cold_weights_gemm.py); medians over workgroups and launches, first-round workgroups (index < CUs) and later ones apart."""
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpt_image_edit_amd import libfk, ops  # noqa: E402

BF = torch.bfloat16
NRING = int(os.environ.get("NRING", "12"))
label = sys.argv[1] if len(sys.argv) > 1 else os.path.basename(libfk.LIB_PATH)
lib = libfk.load()
lib.fk_entry_stamps_set.argtypes = [ctypes.c_void_p]
lib.fk_entry_stamps_set.restype = ctypes.c_int
CUS = torch.cuda.get_device_properties(0).multi_processor_count
MAXWG = 4096
buf = torch.zeros(MAXWG * 8, dtype=torch.int64, device="cuda")
assert lib.fk_entry_stamps_set(ctypes.c_void_p(buf.data_ptr())) == 0
M = 2560
CLASSES = [("MLP-up gemm8<1,256> N 12288 K 3072", 12288, 3072, "gelu", 256),
           ("fused-QKV grid gemm_mix N 9216 K 3072", 9216, 3072, "none", 384),
           ("out-projection gemm9<3,128> N 3072 K 3072", 3072, 3072, "gate_res", 128),
           ("split-K pairs gemm8<3,256,true> N 3072 K 12288", 3072, 12288, "gate_res", 512)]
SPANS = [("entry -> first request", 0, 1), ("first request -> first MFMA phase", 1, 2), ("entry -> first MFMA phase", 0, 2),
         ("K loop", 2, 3), ("loop exit -> last store", 3, 4)]
print(f"# {label}: s_memtime deltas, medians over workgroups x {NRING} cold launches; M = {M}, {CUS} CUs")
for name, N, K, epi, want in CLASSES:
    a = (torch.rand(1, M, K, device="cuda") * 2 - 1).to(BF)
    ws = [((torch.rand(N, K, device="cuda") * 2 - 1) * 0.05).to(BF) for _ in range(NRING)]
    b = (torch.rand(N, device="cuda") * 2 - 1).to(BF)
    res = torch.zeros(1, M, N, device="cuda", dtype=BF)
    gate = torch.ones(1, N, device="cuda", dtype=BF)
    out = torch.empty(1, M, N, device="cuda", dtype=BF)

    def launch(i):
        if epi == "gelu":
            ops.gemm(a, ws[i], b, out=out, epilogue=ops.FK_EPI_GELU_TANH)
        elif epi == "gate_res":
            ops.gemm(a, ws[i], b, out=out, epilogue=ops.FK_EPI_GATE_RES, res=res, gate=gate)
        else:
            ops.gemm(a, ws[i], b, out=out)

    for i in range(NRING):
        launch(i)
    torch.cuda.synchronize()
    assert ops.gemm_last_variant() == want, (name, ops.gemm_last_variant())
    rows = {"first round": {s[0]: [] for s in SPANS}, "later rounds": {s[0]: [] for s in SPANS}}
    nwg = 0
    for i in range(NRING):
        buf.zero_()
        launch(i)
        torch.cuda.synchronize()
        t = buf.view(MAXWG, 8).cpu()
        live = (t[:, 0] != 0).nonzero().flatten().tolist()
        nwg = len(live)
        for w in live:
            which = "first round" if w < CUS else "later rounds"
            for sname, i0, i1 in SPANS:
                rows[which][sname].append(int(t[w, i1] - t[w, i0]))
    print(f"\n## {name}: {nwg} workgroups")
    for which, spans in rows.items():
        if not spans[SPANS[0][0]]:
            continue
        print(f"  {which} ({len(spans[SPANS[0][0]]) // NRING} workgroups per launch)")
        for sname, _, _ in SPANS:
            v = sorted(spans[sname])
            print(f"    {sname:36s} median {statistics.median(v):9.0f}   p10 {v[len(v) // 10]:9d}   p90 {v[len(v) * 9 // 10]:9d}")
    del ws
lib.fk_entry_stamps_set(None)
