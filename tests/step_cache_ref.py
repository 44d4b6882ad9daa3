"""Host reference for the step-cache kernels (plain module: tests/test_step_cache_ref.py checks it on the CPU,
tests/test_hip_step_cache_kernels.py holds the HIP kernels to it).

The two sums -- the bound
-------------------------
csrc/step_cache.hip sums the terms t = |a - b| (and |b|) of M rows of D elements in four fp32 stages.  With cpr = ceil(D / 8)
chunks per row, N = M * cpr work items, nblk = min(ceil(N / 256), 1024) blocks and T = 256 * nblk threads:

  chunk    ((t0 + t1) + (t2 + t3)) + ((t4 + t5) + (t6 + t7)), terms beyond D are 0            a term passes 3 additions
  thread   acc += chunk sum over its items g, g + T, ...                                      iters = ceil(N / T) additions
  block    halving tree over the block's 256 accumulators                                     n_tree = 8
  final    one block: thread t adds partials t, t + 256, ... in order, then the same tree     n_final = ceil(nblk / 256) + 8

so a term passes at most n_serial + n_tree + n_final fp32 additions with n_serial = 3 + iters, and forming the term costs one
more rounding (the difference of two bf16 numbers is not always an fp32 number; |b| is exact).  With u = 2^-24 the first-order
bound of any such summation tree is

    |S - sum t| <= (n_serial + n_tree + n_final + 1) * u * sum |t|

Nothing in it comes from a kernel's output.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
THREADS, MAX_BLOCKS = 256, 1024
ONE_TRIP_ITEMS = THREADS * MAX_BLOCKS        # work items (8-element chunks) the grid covers in its first trip


def layout(M, D):
    cpr = (D + 7) // 8
    N = M * cpr
    nblk = min((N + THREADS - 1) // THREADS, MAX_BLOCKS)
    T = nblk * THREADS
    iters = (N + T - 1) // T
    nf = (nblk + THREADS - 1) // THREADS
    return dict(cpr=cpr, N=N, nblk=nblk, T=T, iters=iters, n_serial=3 + iters, n_tree=8, n_final=nf + 8, nf=nf)


def sums64(a, b):
    """fp64 (sum |a - b|, sum |b|) over two tensors of one shape (their values are the truth)."""
    a64, b64 = a.to(torch.float64), b.to(torch.float64)
    return float((a64 - b64).abs().sum()), float(b64.abs().sum())


def bound(a, b):
    """(bound on |out[0] - sum|a - b||, bound on |out[1] - sum|b||) for [..., D] inputs: the module docstring's derivation."""
    D = a.shape[-1]
    lay = layout(a.numel() // D, D)
    gamma = (lay["n_serial"] + lay["n_tree"] + lay["n_final"] + 1) * U32
    s0, s1 = sums64(a, b)
    return gamma * s0, gamma * s1


def _tree256(v):
    """Halving tree over axis -1 of length 256 (offsets 128 .. 1), fp32."""
    v = v.copy()
    off = THREADS // 2
    while off >= 1:
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def emulate(a, b, drop_last_partial=False, drop_row=None):
    """The kernels' summation order in numpy fp32.  a, b: [..., D] tensors (bf16 values).  Returns fp32 (out0, out1).
    ``drop_last_partial`` / ``drop_row``: deliberately wrong variants (the finaliser misses the last block's partial / the
    partials miss one row), for showing that the bound catches them."""
    D = a.shape[-1]
    M = a.numel() // D
    lay = layout(M, D)
    cpr, N, nblk, T, iters, nf = (lay[k] for k in ("cpr", "N", "nblk", "T", "iters", "nf"))
    af = a.reshape(M, D).to(torch.float32).numpy()
    bfl = b.reshape(M, D).to(torch.float32).numpy()
    out = []
    for term in (np.abs(af - bfl), np.abs(bfl)):          # fp32 subtraction: one rounding, as on the device
        term = term.astype(np.float32)
        if drop_row is not None:
            term = term.copy()
            term[drop_row] = 0
        t = np.zeros((M, cpr * 8), np.float32)
        t[:, :D] = term
        t = t.reshape(N, 8)
        chunk = ((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])) + ((t[:, 4] + t[:, 5]) + (t[:, 6] + t[:, 7]))
        items = np.zeros(iters * T, np.float32)           # an absent item adds nothing; + 0 is exact
        items[:N] = chunk
        items = items.reshape(iters, T)
        acc = np.zeros(T, np.float32)
        for k in range(iters):
            acc = acc + items[k]
        part = _tree256(acc.reshape(nblk, THREADS))
        if drop_last_partial:
            part = part[:-1]
        pad = np.zeros(nf * THREADS, np.float32)
        pad[:len(part)] = part
        pad = pad.reshape(nf, THREADS)
        facc = np.zeros(THREADS, np.float32)
        for k in range(nf):
            facc = facc + pad[k]
        out.append(np.float32(_tree256(facc)))
    return out[0], out[1]


def check(name, got, a, b):
    """got: (out0, out1) floats against fp64 on a, b within `bound`; prints and returns the observed / bound ratios."""
    s0, s1 = sums64(a, b)
    b0, b1 = bound(a, b)
    r0 = abs(float(got[0]) - s0) / b0 if b0 > 0 else (0.0 if float(got[0]) == 0.0 else float("inf"))
    r1 = abs(float(got[1]) - s1) / b1 if b1 > 0 else (0.0 if float(got[1]) == 0.0 else float("inf"))
    lay = layout(a.numel() // a.shape[-1], a.shape[-1])
    print(f"[parity] {name}: M={a.numel() // a.shape[-1]} D={a.shape[-1]} nblk={lay['nblk']} iters={lay['iters']} "
          f"observed/bound diff={r0:.4f} ref={r1:.4f}", flush=True)
    assert r0 <= 1.0, f"{name}: sum|a-b| is {r0:.3f} x the derived bound"
    assert r1 <= 1.0, f"{name}: sum|b| is {r1:.3f} x the derived bound"
    return r0, r1


def data(shape, seed, spread=0.05):
    """(a, b) bf16: b ~ N(0, 1), a = b + spread * N(0, 1): a step's modulated input beside the previous step's."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(shape, generator=g)
    a = b + spread * torch.randn(shape, generator=g)
    return a.to(torch.bfloat16), b.to(torch.bfloat16)
