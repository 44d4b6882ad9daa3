"""fp64 reference of the KEY-MASKED joint attention (forward + backward), built on tests/attention_ref.py, and the CPU checks
of it: against torch autograd through fp64 scaled_dot_product_attention(attn_mask=...), of the row-wise checker's power to
reject a wrong mask, and of the packed mask's bit layout.  tests/test_hip_attention_mask.py holds the HIP kernels to it.

How the mask reaches attention_ref.py without editing it: its sweep is square (queries and keys of one length; dK / dV are
accumulated over all query rows, masked tokens' rows included, so gathering the valid KEYS alone would make it rectangular).
The head dimension is free, though: one extra column -- q: 1, k: 0 at a valid key and -BIG at a masked one, v / dO: 0 -- adds
exactly 0 to a valid key's score and -BIG to a masked key's, whose probability exp2(-BIG c) underflows to exactly 0 in fp64.
Every sum of attention_ref.py then runs over the valid keys only, a masked key's dK / dV rows are sums of exact zeros, and the
extra column of every result is dropped.  The rounding model (attention_bwd_model) comes along unchanged.  The forward's
rounding model is formed here: o = bf16(bf16(P) V), the probabilities entering the PV product as bf16, one rounding of the result.
"""
import numpy as np
import pytest
import torch

import attention_ref as ar

F64 = torch.float64
BIG = 1.0e9          # exp2(-BIG * scale * log2 e) == 0.0 in fp64 for any scale the tests use (>= 1e-3)


def pack(mask):
    """[B, S] bool -> int64 [B, ceil(S / 64)]: bit j of word (b, t) = mask[b, 64 t + j]; bits at positions >= S are 0.  Pure
    Python: the layout fk.h documents, written down a second time."""
    mask = torch.as_tensor(mask).bool()
    B, S = mask.shape
    nw = (S + 63) // 64
    out = torch.zeros(B, nw, dtype=torch.int64)
    for b in range(B):
        for t in range(nw):
            w = 0
            for j in range(min(64, S - 64 * t)):
                if mask[b, 64 * t + j]:
                    w |= 1 << j
            out[b, t] = w - (1 << 64) if w >= (1 << 63) else w      # the same 64 bits as a signed word
    return out


def _augment(q, k, v, dout, mask):
    B, H, S, _ = q.shape
    col = lambda x: x[:, None, :, None].expand(B, H, S, 1)      # noqa: E731
    one, zero = torch.ones(B, S, dtype=F64), torch.zeros(B, S, dtype=F64)
    kcol = torch.where(mask.bool(), zero, torch.full_like(zero, -BIG))
    return (torch.cat([q.to(F64), col(one)], -1), torch.cat([k.to(F64), col(kcol)], -1), torch.cat([v.to(F64), col(zero)], -1),
            torch.cat([dout.to(F64), col(zero)], -1))


def masked_ref_and_model(q, k, v, dout, scale, mask, lse=None, dsum=None):
    """attention_ref.attention_ref_and_model under the key mask `mask` ([B, S] bool, True = valid): dicts
    ref{o, lse, dq, dk, dv} and model{o, dq, dk, dk3, dv}, [B, H, S, 128] fp64.  dK / dV rows of masked keys are exactly 0."""
    qa, ka, va, da = _augment(q, k, v, dout, mask)
    ref, mod = ar.attention_ref_and_model(qa, ka, va, da, scale, lse=lse, dsum=dsum)
    ref = {n: (t if n == "lse" else t[..., :-1].contiguous()) for n, t in ref.items()}
    mod = {n: t[..., :-1].contiguous() for n, t in mod.items()}
    # forward rounding model: bf16 probabilities into the PV product, the result rounded once
    c2 = scale * ar.LOG2E
    s2 = torch.einsum("bhqd,bhkd->bhqk", q.to(F64), k.to(F64)) * c2
    s2 = s2.masked_fill(~mask.bool()[:, None, None, :], -float("inf"))
    P = torch.exp2(s2 - ref["lse"][..., None])
    mod["o"] = ar.bf16r(ar.bf16r(P) @ v.to(F64))
    return ref, mod


def pattern_2d(S_txt=37, rows=16, cols=20, valid=((16, 20), (12, 16))):
    """The reference's padded batch as a key mask: S_txt text keys (always valid), then a rows x cols token grid per sample of
    which the top-left valid[b] = (r, c) corner is real.  [B, S_txt + rows * cols] bool."""
    m = torch.zeros(len(valid), S_txt + rows * cols, dtype=torch.bool)
    m[:, :S_txt] = True
    for b, (r, c) in enumerate(valid):
        g = torch.zeros(rows, cols, dtype=torch.bool)
        g[:r, :c] = True
        m[b, S_txt:] = g.flatten()
    return m


# ---- the checks -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    B, H, S = 2, 2, 70
    q, k, v, dout = ar.make_inputs(B, H, S, seed=4242)
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(B, S, generator=g) > 0.35
    mask[1, :64] = False                      # a whole 64-key tile without a valid key
    mask[1, 66] = True
    scale = 128 ** -0.5
    ref, mod = masked_ref_and_model(q, k, v, dout, scale, mask)
    return dict(q=q, k=k, v=v, dout=dout, mask=mask, scale=scale, ref=ref, mod=mod)


def test_masked_reference_matches_autograd_through_sdpa(small):
    q, k, v, dout = (small[n].to(F64).clone().requires_grad_(n != "dout") for n in ("q", "k", "v", "dout"))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=small["mask"][:, None, None, :], scale=small["scale"])
    o.backward(dout)
    ref = small["ref"]
    for name, got in (("o", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        torch.testing.assert_close(ref[name], got, rtol=1e-10, atol=1e-12, msg=lambda m, n=name: f"{n}: {m}")
    s = torch.einsum("bhqd,bhkd->bhqk", small["q"].to(F64), small["k"].to(F64)) * small["scale"]
    s = s.masked_fill(~small["mask"][:, None, None, :], -float("inf"))
    torch.testing.assert_close(ref["lse"], torch.logsumexp(s, -1) * ar.LOG2E, rtol=1e-12, atol=1e-12)
    masked = ~small["mask"]
    for n in ("dk", "dv"):
        assert (ref[n].transpose(1, 2)[masked] == 0).all() and (small["mod"][n].transpose(1, 2)[masked] == 0).all()


def test_rounding_model_passes_its_own_bound(small):
    ref, mod = small["ref"], small["mod"]
    for n, m in (("o", "o"), ("dq", "dq"), ("dk", "dk"), ("dk", "dk3"), ("dv", "dv")):
        assert ar.assert_rows_close(f"model {m}", mod[m], ref[n], mod[m], margin=1.0)["ratio"] <= 1.0 + 1e-9


def test_checker_rejects_a_result_that_ignores_the_mask(small):
    s = small
    _, wrong = masked_ref_and_model(s["q"], s["k"], s["v"], s["dout"], s["scale"], torch.ones_like(s["mask"]))
    for n in ("o", "dq", "dk", "dv"):
        with pytest.raises(AssertionError):
            ar.assert_rows_close(f"unmasked {n}", wrong[n], s["ref"][n], s["mod"][n])


def test_checker_rejects_one_key_too_many_masked(small):
    s = small
    for b, key in ((0, int(s["mask"][0].nonzero()[3])), (1, 66)):
        m2 = s["mask"].clone()
        m2[b, key] = False
        if not m2[b].any():
            m2[b, 65] = True               # (sample 1 has few valid keys: swap instead of emptying it)
        _, wrong = masked_ref_and_model(s["q"], s["k"], s["v"], s["dout"], s["scale"], m2)
        for n in ("o", "dq", "dk", "dv"):
            with pytest.raises(AssertionError):
                ar.assert_rows_close(f"one key too many {n}", wrong[n], s["ref"][n], s["mod"][n])


def test_checker_rejects_a_gradient_at_a_masked_key(small):
    s = small
    _, unmasked = masked_ref_and_model(s["q"], s["k"], s["v"], s["dout"], s["scale"], torch.ones_like(s["mask"]))
    key = int((~s["mask"][0]).nonzero()[0])
    for n in ("dk", "dv"):
        wrong = s["mod"][n].clone()
        wrong[0, :, key] = unmasked[n][0, :, key]          # what an unmasked kernel would have left there
        with pytest.raises(AssertionError):
            ar.assert_rows_close(f"{n} at a masked key", wrong, s["ref"][n], s["mod"][n])


@pytest.mark.parametrize("S", [1, 63, 64, 65, 200, 357])
def test_pack_layout_against_numpy(S):
    g = torch.Generator().manual_seed(S)
    mask = torch.rand(3, S, generator=g) > 0.4
    mask[2] = True
    nw = (S + 63) // 64
    padded = np.zeros((3, nw * 64), dtype=np.uint8)
    padded[:, :S] = mask.numpy()
    want = np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(3, nw)      # byte i of a word = keys 8 i .. 8 i + 7
    got = pack(mask)
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, nw)
    assert np.array_equal(got.numpy().view(np.uint64), want)
    for b, key in ((0, 0), (1, S - 1), (2, S // 2)):            # the documented layout, bit by bit
        assert bool((int(got[b, key // 64]) >> (key % 64)) & 1) == bool(mask[b, key])
    if S % 64:
        assert (int(got[2, -1]) & ((1 << 64) - 1)) >> (S % 64) == 0, "bits at positions >= S must be 0"


def test_pattern_2d_is_the_padded_batch():
    m = pattern_2d()
    assert tuple(m.shape) == (2, 357) and m[0].all() and int(m[1].sum()) == 37 + 12 * 16
    words = pack(m)
    assert (words[0, :5] == -1).all() and int(words[0, 5]) == (1 << 37) - 1           # 357 = 5 * 64 + 37
    kinds = {"full" if int(w) == -1 else "empty" if int(w) == 0 else "partial" for w in words[1]}
    assert "partial" in kinds
