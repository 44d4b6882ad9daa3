"""fp64 reference of the joint attention (forward + backward), a model of the backward's bf16 rounding points, and the
row-wise checker the attention tests share (plain module: tests/test_attention_ref.py checks the checker on the CPU,
tests/test_hip_attention_grids.py holds the HIP kernels to it).

    P = exp2(Q K^T c log2(e) - lse)     O = P V      D = sum_d dO O
    dV = P^T dO     dP = dO V^T     dS = P o (dP - D) c     dQ = dS K     dK = dS^T Q

Everything here is head-major [B, H, S, 128]; `token_major` / `head_major` convert to and from the kernels' [B, S, H*128] views.
The reference takes the bf16-rounded inputs and, when given, the lse / D tensors the GPU backward was actually fed: the backward
kernel is a pure function of (q, k, v, dO, lse, D, c) and is checked as that function; lse and D have their own checks.

The model is the same sums in fp64 with the rounding points csrc/attention_bwd.hip documents and no others (a model of bf16,
not of the kernel): the weights enter the accumulating MFMA as bf16 -- dV from bf16(p); dQ pass and three-pass dK from
bf16(p (dP - D)); paired pass dK from bf16(bf16(p) (dP - D)) -- and each gradient is rounded to bf16 once.  Its row errors
against the reference are what bf16 costs; `assert_rows_close` derives the bound from them, never from a kernel.
"""
import math

import torch

LOG2E = 1.4426950408889634
MARGIN = 2.0            # allowance for what the fp64 rounding model leaves out (fp32 accumulation order, the hardware exp2)
MAX_MARGIN = 4.0        # a case may go up to here with the cause named in its docstring; beyond is a finding
PROJ_TOL = 2.0 ** -8    # |<got, ref> / <ref, ref> - 1| per (b, h): rounding averages out over S x 128 elements, a wrong factor does not
BF = torch.bfloat16
F64 = torch.float64


def bf16r(x):
    """Round an fp64 tensor to bf16 and back."""
    return x.to(BF).to(F64)


def token_major(x):
    """[B, H, S, 128] -> contiguous [B, S, H*128]."""
    B, H, S, hd = x.shape
    return x.transpose(1, 2).reshape(B, S, H * hd).contiguous()


def head_major(x, H):
    """[B, S, H*128] view -> [B, H, S, 128] view."""
    B, S, _ = x.shape
    return x.reshape(B, S, H, -1).transpose(1, 2)


def make_inputs(B, H, S, seed, matched=True):
    """q, k, v, dout as bf16 [B, H, S, 128], built on the host.  q, k, v ~ N(0, 1); for a third of the queries a matched key
    k[pi(i)] += 0.9 q[i], pi a permutation of the WHOLE sequence (the dominant term of such a row sits anywhere: it crosses item,
    tile and seam boundaries, and lse / D differ from row to row); dO rows scaled by 2^U{-4..4} per (b, h, s), so that a row- or
    head-permuted result cannot hide under a global absmax."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, S, 128, generator=g)
    k = torch.randn(B, H, S, 128, generator=g)
    v = torch.randn(B, H, S, 128, generator=g)
    dout = torch.randn(B, H, S, 128, generator=g)
    if matched:
        for b in range(B):
            for h in range(H):
                pi = torch.randperm(S, generator=g)
                src = torch.arange(0, S, 3)
                k[b, h, pi[src]] += 0.9 * q[b, h, src]
    dout *= torch.exp2(torch.randint(-4, 5, (B, H, S, 1), generator=g).float())
    return q.to(BF), k.to(BF), v.to(BF), dout.to(BF)


def _sweep(q, k, v, dout, scale, lse, dsum, want_ref, want_model, weight=None, chunk=256):
    """One pass over every (b, h), chunked over query rows (S = 8704: 18 MB per [chunk, S] fp64 temporary, well under 1 GB in all).
    weight(r0, r1) -> [r1 - r0, S] multiplier of the MODEL's weights (test hook: a dropped or doubled tile)."""
    B, H, S, hd = q.shape
    c2 = scale * LOG2E
    z = lambda: torch.zeros(B, H, S, hd, dtype=F64)   # noqa: E731
    ref = dict(o=z(), lse=torch.zeros(B, H, S, dtype=F64), dq=z(), dk=z(), dv=z()) if want_ref else None
    mod = dict(dq=z(), dk=z(), dk3=z(), dv=z()) if want_model else None
    for b in range(B):
        for h in range(H):
            Q, K, V, dO = (t[b, h].to(F64) for t in (q, k, v, dout))
            for r0 in range(0, S, chunk):
                r1 = min(S, r0 + chunk)
                s2 = (Q[r0:r1] @ K.t()) * c2
                m = s2.max(dim=1, keepdim=True).values
                P = torch.exp2(s2.sub_(m))                 # one exponential per score; normalised below
                l = P.sum(dim=1)
                lse_own = m[:, 0] + torch.log2(l)
                P /= l[:, None]
                del s2
                if want_ref or dsum is None:
                    o_own = P @ V
                if want_ref:
                    ref["o"][b, h, r0:r1] = o_own
                    ref["lse"][b, h, r0:r1] = lse_own
                D = (dO[r0:r1] * o_own).sum(dim=1) if dsum is None else dsum[b, h, r0:r1].to(F64)
                if lse is not None:                        # exp2(s - lse) = exp2(s - lse_own) * exp2(lse_own - lse)
                    P *= torch.exp2(lse_own - lse[b, h, r0:r1].to(F64))[:, None]
                G = dO[r0:r1] @ V.t()
                G -= D[:, None]                       # dP - D
                if want_ref:
                    dS = P * G
                    ref["dv"][b, h] += P.t() @ dO[r0:r1]
                    ref["dq"][b, h, r0:r1] = (dS @ K) * scale
                    ref["dk"][b, h] += (dS.t() @ Q[r0:r1]) * scale
                    del dS
                if want_model:
                    W = weight(r0, r1) if weight is not None else None
                    wf = lambda x: x if W is None else x * W    # noqa: E731
                    pb = bf16r(P)
                    mod["dv"][b, h] += wf(pb).t() @ dO[r0:r1]
                    w2 = wf(bf16r(pb * G))                    # paired pass: bf16(bf16(p) (dP - D))
                    mod["dk"][b, h] += w2.t() @ Q[r0:r1]
                    del pb, w2
                    w3 = wf(bf16r(P * G))                     # dQ pass, three-pass dK: bf16(p (dP - D))
                    mod["dq"][b, h, r0:r1] = w3 @ K
                    mod["dk3"][b, h] += w3.t() @ Q[r0:r1]
                    del w3
    if want_model:
        for n in ("dq", "dk", "dk3"):
            mod[n] = bf16r(mod[n] * scale)
        mod["dv"] = bf16r(mod["dv"])
    return ref, mod


def attention_ref64(q, k, v, dout, scale, lse=None, dsum=None):
    """o, lse2 (log2 domain), dq, dk, dv in fp64 from the bf16-rounded inputs.  o and lse2 are always the reference's own; the
    gradients use `lse` / `dsum` ([B, H, S]) when given."""
    ref, _ = _sweep(q, k, v, dout, scale, lse, dsum, True, False)
    return ref["o"], ref["lse"], ref["dq"], ref["dk"], ref["dv"]


def attention_bwd_model(q, k, v, dout, scale, lse=None, dsum=None, weight=None):
    """dq, dk (paired pass), dv, dk3 (three-pass form): fp64 sums with the kernel's documented bf16 rounding points."""
    _, mod = _sweep(q, k, v, dout, scale, lse, dsum, False, True, weight=weight)
    return mod["dq"], mod["dk"], mod["dv"], mod["dk3"]


def attention_ref_and_model(q, k, v, dout, scale, lse=None, dsum=None):
    """Both of the above from one sweep (the scores and exponentials are formed once): dicts ref{o, lse, dq, dk, dv} and
    model{dq, dk, dk3, dv}."""
    return _sweep(q, k, v, dout, scale, lse, dsum, True, True)


def row_errors(got, ref):
    """Per row (last dimension): ||got - ref||_2 and ||ref||_2, in fp64."""
    g, r = got.to(F64), ref.to(F64)
    return (g - r).norm(dim=-1), r.norm(dim=-1)


def _worst(ratio, n=3):
    """The n largest entries of a [B, H, S] tensor as ((b, h, s), value)."""
    vals, idx = torch.topk(ratio.flatten(), min(n, ratio.numel()))
    _, H, S = ratio.shape
    return [((i // (H * S), i // S % H, i % S), v) for i, v in zip(idx.tolist(), vals.tolist())]


def assert_rows_close(name, got, ref, model, margin=MARGIN):
    """Every row r of `got` ([B, H, S, 128]) within margin * max(rho ||ref_r||, floor) of `ref`, and per (b, h) the projection
    <got, ref> / <ref, ref> within 2^-8 of 1.

    floor = 2^-9 rms(ref) sqrt(128): half a bf16 ulp at the tensor's scale over a row (for rows whose gradient is ~0);
    rho   = the largest row-relative error of the rounding MODEL over rows with ||ref_r|| above the floor.
    No row is excluded.  Prints rho, the worst rows with their (b, h, s), and the largest observed / model ratio (= the margin
    the result would have needed); returns dict(ratio=that ratio, rho, proj=max |projection - 1|, proj_model=the model's own)."""
    assert 1.0 <= margin <= MAX_MARGIN
    got, ref, model = got.to(F64).cpu(), ref.to(F64), model.to(F64)
    assert got.shape == ref.shape == model.shape and got.dim() == 4
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    floor = 2.0 ** -9 * ref.pow(2).mean().sqrt().item() * math.sqrt(ref.shape[-1])
    e_m, n_r = row_errors(model, ref)
    above = n_r > floor
    rho = (e_m[above] / n_r[above]).max().item() if above.any() else 0.0
    e_g, _ = row_errors(got, ref)
    unit = torch.clamp(rho * n_r, min=floor) if floor > 0 else rho * n_r
    ratio = torch.where(unit > 0, e_g / unit, torch.where(e_g > 0, torch.full_like(e_g, math.inf), torch.zeros_like(e_g)))
    ratio_m = torch.where(unit > 0, e_m / unit, torch.zeros_like(e_m))
    worst = _worst(ratio)
    # the systematic part, per (b, h)
    rr = (ref * ref).sum(dim=(-1, -2))
    ok_h = rr > 0
    proj_g = torch.where(ok_h, (got * ref).sum(dim=(-1, -2)) / rr.clamp(min=1e-300) - 1, torch.zeros_like(rr))
    proj_m = torch.where(ok_h, (model * ref).sum(dim=(-1, -2)) / rr.clamp(min=1e-300) - 1, torch.zeros_like(rr))
    bh = int(proj_g.abs().argmax())
    rows = "; ".join(f"(b,h,s)={p} {r / margin:.3f} of the bound" for p, r in worst)
    print(f"[rows] {name}: rho={rho:.3e} floor={floor:.3e} rows_below_floor={int((~above).sum())} "
          f"observed/model max={ratio.max().item():.3f} (margin {margin:g}; model's own max {ratio_m.max().item():.3f}) "
          f"worst: {rows} | projection-1: got max {proj_g.abs().max().item():.2e} at (b,h)=({bh // ref.shape[1]},{bh % ref.shape[1]}), "
          f"model max {proj_m.abs().max().item():.2e}, bound {PROJ_TOL:.2e}", flush=True)
    p, r = worst[0]      # (1 + 1e-9): the fp64 round-off of the ratio itself, so that the model sits AT margin 1, not above it
    assert r <= margin * (1 + 1e-9), (f"{name}: row (b,h,s)={p} is {r:.3f} x max(rho ||ref_r||, floor), allowed {margin:g} "
                         f"(rho={rho:.3e}, floor={floor:.3e})")
    assert proj_g.abs().max().item() <= PROJ_TOL, (f"{name}: projection <got,ref>/<ref,ref> - 1 = {proj_g.flatten()[bh].item():.3e} "
                                                   f"at (b,h)=({bh // ref.shape[1]},{bh % ref.shape[1]}), allowed {PROJ_TOL:.3e}")
    return dict(ratio=ratio.max().item(), rho=rho, proj=proj_g.abs().max().item(), proj_model=proj_m.abs().max().item())
