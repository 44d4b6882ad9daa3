"""Key-padding mask in the attention forward and backward (fk_attention_fwd_masked_bf16 / fk_attention_bwd_masked_bf16 /
fk_pack_key_mask) against the unmasked kernels, bit for bit, where the two must agree, and against the masked fp64 reference of
tests/test_attention_mask_ref.py everywhere else.  B = 2, H = 2; every output sits inside a sentinel-filled allocation (guard
rows and columns, as tests/test_hip_attention_grids.py has them), checked after every run.

Bounds: o, dq, dk, dv by attention_ref.assert_rows_close at MARGIN = 2 (rho from the bf16 rounding model, never from a kernel);
lse against the fp64 log-sum-exp at rtol 1e-4 / atol 3e-4 (log2 units), the bound of tests/test_hip_attention_grids.py; the
fp32-output form at rtol 1e-3 / atol 1e-4.  dK / dV rows of masked keys are compared with == 0.

Observed on an MI355X (largest observed / model ratio per tensor, bound 2.0): see RECORDED below.
"""
import pytest
import torch

import attention_ref as ar
import test_attention_mask_ref as mr
from attention_ref import MARGIN

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCALE = 128 ** -0.5
B, H = 2, 2
D = H * 128
PAD = 40

# `[rows]` lines of one MI355X run of this file (observed / model, the margin each result would have needed; bound MARGIN = 2.0)
RECORDED = """
case                 o      dq     dk     dv     dk three-pass   lse max |d| (log2 units; bound rtol 1e-4 / atol 3e-4)
2-D padding S357     1.196  0.876  1.000  0.912  1.000           3.45e-06
first-empty          0.974  0.957  1.000  0.903  1.000           3.61e-06
last-empty           1.044  0.852  1.000  1.000  1.000           3.57e-06
first-block-empty    1.324  0.968  1.000  0.792  1.000           3.29e-06
single key           0.000  -      -      1.000  -               1.16e-06
q x 8, first-empty   lse max |d| 2.67e-05 with lse up to 163.6; o max 3.98e-03, mean 2.16e-04 of absmax (bounds 3e-2 / 1e-3)
(the gradients' worst rows sit exactly at the rounding model's own; o, whose model knows nothing of the kernel's exponent
reference, needed at most 1.32 of the allowed 2.0.)  The bit-for-bit cases (all ones, prefix) and the fp32-output form passed.
"""


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


class Run:
    """Forward with lse, rowdot and backward of one case, every output a window of a larger allocation filled with 5.0 (lse / D:
    12345).  mask: [B, S] bool (packed with ops.pack_key_mask) or None = the UNMASKED kernels on the plain grid (grid = -1)."""

    def __init__(self, ops, q, k, v, dout, mask=None, passes=1, scale=SCALE, lse=None, dsum=None):
        S = q.shape[2]
        self.S = S
        self.qd, self.kd = q.cuda().contiguous(), k.cuda().contiguous()
        self.qkv = torch.zeros(B, S, 3 * D, device="cuda", dtype=BF)
        self.qkv[:, :, 2 * D:] = ar.token_major(v).cuda()
        vd = self.qkv[:, :, 2 * D:]
        self.doutd = ar.token_major(dout).cuda()
        n = B * H * S
        self.stats = torch.full((2, n + 128), 12345.0, device="cuda", dtype=torch.float32)
        self.lse, self.dsum = self.stats[0, 64:64 + n].view(B, H, S), self.stats[1, 64:64 + n].view(B, H, S)
        self.o_wide = torch.full((B, S + 3, D + 64), 5.0, device="cuda", dtype=BF)
        self.dq_big = torch.full((B, H, S + PAD, 128), 5.0, device="cuda", dtype=BF)
        self.dk_big = torch.full((B, H, S + PAD, 128), 5.0, device="cuda", dtype=BF)
        self.dv_wide = torch.full((B, S + 3, 3 * D + 64), 5.0, device="cuda", dtype=BF)
        self.o, self.dv = self.o_wide[:, :S, :D], self.dv_wide[:, :S, 2 * D:3 * D]
        self.dq, self.dk = self.dq_big[:, :, :S], self.dk_big[:, :, :S]
        km = None
        if mask is not None:
            km = ops.pack_key_mask(mask.cuda())
            assert torch.equal(km.cpu(), mr.pack(mask)), "fk_pack_key_mask against the pure-Python packer"
        ops.attention_set_split(0)             # unmasked calls: the plain grid; masked calls know no other
        ops.attention_bwd_set_mode(passes)
        try:
            ops.attention_lse(self.qd, self.kd, vd, self.o, self.lse, scale=scale, key_mask=km)
            ops.rowdot(self.doutd, self.o, H, out=self.dsum)
            ops.attention_bwd(self.qd, self.kd, vd, self.doutd, self.lse if lse is None else lse, self.dsum if dsum is None else dsum,
                              self.dq, self.dk, self.dv, scale=scale, key_mask=km)
            torch.cuda.synchronize()
        finally:
            ops.attention_set_split(1)
            ops.attention_bwd_set_mode(1)
        self.km = km
        self.check_guards()

    def check_guards(self):
        S, n = self.S, B * H * self.S
        assert (self.stats[:, :64] == 12345.0).all() and (self.stats[:, 64 + n:] == 12345.0).all(), "lse / D: written outside [B, H, S]"
        assert (self.o_wide[:, S:] == 5.0).all() and (self.o_wide[:, :, D:] == 5.0).all(), "o: written outside its view"
        assert (self.dq_big[:, :, S:] == 5.0).all(), "dq: rows beyond S written"
        assert (self.dk_big[:, :, S:] == 5.0).all(), "dk: rows beyond S written"
        assert ((self.dv_wide[:, S:] == 5.0).all() and (self.dv_wide[:, :, :2 * D] == 5.0).all()
                and (self.dv_wide[:, :, 3 * D:] == 5.0).all()), "dv: written outside its view"

    def host(self):
        return dict(o=ar.head_major(self.o.cpu(), H), lse=self.lse.cpu(), dq=self.dq.cpu(), dk=self.dk.cpu(),
                    dv=ar.head_major(self.dv.cpu(), H))


ALL_GRADS = ("dq", "dk", "dv", "dk three-pass")


def check_against_reference(ops, tag, q, k, v, dout, mask, scale=SCALE, grads=ALL_GRADS):
    """Paired and three-pass backward of one masked case against the masked fp64 reference formed from the lse and D the kernels
    were fed; returns the default run and the observed / model ratios."""
    run = Run(ops, q, k, v, dout, mask, scale=scale)
    three = Run(ops, q, k, v, dout, mask, passes=0, scale=scale)
    assert torch.equal(run.o, three.o) and torch.equal(run.lse, three.lse)
    assert torch.equal(run.dq, three.dq) and torch.equal(run.dv, three.dv), f"{tag}: three-pass dQ / dV differ from the paired form"
    got = run.host()
    ref, mod = mr.masked_ref_and_model(q, k, v, dout, scale, mask, lse=got["lse"], dsum=run.dsum.cpu())
    lse = got["lse"].double()
    print(f"[fwd] {tag}: lse max |d| {(lse - ref['lse']).abs().max().item():.2e} (lse in [{ref['lse'].min().item():.1f}, "
          f"{ref['lse'].max().item():.1f}])", flush=True)
    assert torch.isfinite(lse).all()
    torch.testing.assert_close(lse, ref["lse"], rtol=1e-4, atol=3e-4)
    ratios = {}
    ratios["o"] = ar.assert_rows_close(f"{tag} o", got["o"], ref["o"], mod["o"], margin=MARGIN)["ratio"]
    torch.testing.assert_close(run.dsum.cpu().double(), (dout.double() * got["o"].double()).sum(-1), rtol=1e-3, atol=1e-3)
    masked = ~mask                                  # [B, S] -> rows of [B, S, H, 128]
    for name, t in (("dk", run.dk), ("dv", ar.head_major(run.dv, H)), ("dk three-pass", three.dk)):
        assert (t.transpose(1, 2)[masked.cuda()] == 0).all(), f"{tag}: {name} rows of masked keys must be exact zeros"
    for name, g, r, m in (("dq", got["dq"], ref["dq"], mod["dq"]), ("dk", got["dk"], ref["dk"], mod["dk"]),
                          ("dv", got["dv"], ref["dv"], mod["dv"]), ("dk three-pass", three.dk.cpu(), ref["dk"], mod["dk3"])):
        if name in grads:
            ratios[name] = ar.assert_rows_close(f"{tag} {name}", g, r, m, margin=MARGIN)["ratio"]
    print(f"[rows] {tag}: observed / model " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()) + f" (margin {MARGIN:g})", flush=True)
    return run, three, ref, ratios


# ---- 1. all ones == unmasked ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 200, 257, 320])
def test_all_ones_mask_is_the_unmasked_call_bit_for_bit(ops, S):
    """A word of ones (within S) takes the unmasked tile body, the ragged last tile the select it always had: o, lse, dq, dk, dv
    equal the unmasked kernels' on the plain grid, in both `passes` forms."""
    q, k, v, dout = ar.make_inputs(B, H, S, seed=21000 + S)
    ones = torch.ones(B, S, dtype=torch.bool)
    for passes in (1, 0):
        plain = Run(ops, q, k, v, dout, None, passes=passes)
        masked = Run(ops, q, k, v, dout, ones, passes=passes)
        for n in ("o", "lse", "dsum", "dq", "dk", "dv"):
            assert torch.equal(getattr(plain, n), getattr(masked, n)), f"S{S} passes {passes}: {n} differs from the unmasked call"


# ---- 2. prefix mask == shorter S ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,L", [(320, 200), (320, 256), (200, 65)])
def test_prefix_mask_is_the_shorter_sequence_bit_for_bit(ops, S, L):
    """Keys [0, L) valid in a length-S call against the unmasked call on contiguous copies of the first L tokens: o, lse and dq
    of the rows < L, and -- with the masked call's dout rows >= L zero -- dk / dv of the rows < L, bit for bit.  A masked key's
    numerator is exp2(-1e30 c - m) = 0 exactly, an all-masked tile adds nothing, and a query row >= L whose dout (hence D) is
    zero adds p * 0 to dV and bf16(p * (0 - 0)) = 0 to dK: the same sums in the same order."""
    q, k, v, dout = ar.make_inputs(B, H, S, seed=22000 + S + L)
    dout[:, :, L:] = 0
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[:, :L] = True
    cut = lambda t: t[:, :, :L].contiguous()      # noqa: E731
    for passes in (1, 0):
        long = Run(ops, q, k, v, dout, mask, passes=passes)
        short = Run(ops, cut(q), cut(k), cut(v), cut(dout), None, passes=passes)
        assert torch.equal(long.o[:, :L], short.o) and torch.equal(long.lse[:, :, :L], short.lse), f"forward rows < {L}"
        assert torch.equal(long.dq[:, :, :L], short.dq), "dq rows < L"
        assert torch.equal(long.dk[:, :, :L], short.dk), "dk rows < L"
        assert torch.equal(long.dv[:, :L], short.dv), "dv rows < L"
        assert (long.dk[:, :, L:] == 0).all() and (long.dv[:, L:] == 0).all(), "dk / dv rows of masked keys"
        assert (long.dsum[:, :, L:] == 0).all()


# ---- 3. + 6. the reference's 2-D padding pattern, both `passes` forms -----------------------------------------------------------
def test_2d_padding_pattern_against_fp64(ops):
    """S_txt = 37 text keys, then a 16 x 20 token grid: sample 0 fills it, sample 1 is real in rows < 12, cols < 16 -- S = 357,
    ragged, sample 1 with partial tiles throughout and an all-masked last tile.  o, dq, dk, dv (paired and three-pass) by
    assert_rows_close at MARGIN; lse at the grids file's bound; masked keys' dK / dV rows exact zeros; masked tokens' QUERY rows
    are compared like any others."""
    mask = mr.pattern_2d()
    S = mask.shape[1]
    q, k, v, dout = ar.make_inputs(B, H, S, seed=23000, matched=True)
    check_against_reference(ops, "2-D padding S357", q, k, v, dout, mask)


# ---- 4. whole-tile cases --------------------------------------------------------------------------------------------------------
def _whole_tile_mask(case, S=320):
    m = torch.ones(B, S, dtype=torch.bool)
    if case == "first-empty":
        m[:, :64] = False
    elif case == "last-empty":
        m[:, 256:] = False
    elif case == "first-block-empty":       # keys 0..31 masked: the reference comes from the tile's second 32-key block
        m[:, :32] = False
        m[1, :47] = False
    return m


@pytest.mark.parametrize("case", ["first-empty", "last-empty", "first-block-empty"])
def test_whole_tile_cases(ops, case):
    """S = 320.  first-empty: keys 0..63 masked -- the forward's exponent reference must come from tile 1; last-empty: tile 4
    masked; first-block-empty: the first 32-key block of tile 0 (and in sample 1 half of the second) masked -- the reference
    comes from the tile's second block."""
    S = 320
    q, k, v, dout = ar.make_inputs(B, H, S, seed=24000 + len(case))
    check_against_reference(ops, case, q, k, v, dout, _whole_tile_mask(case, S))


def test_single_valid_key(ops):
    """Only key 130 valid in S = 320: the softmax is 1 at that key, so o = v[130] (reference and rounding model agree: the row
    bound is the half-ulp floor), lse = q.k[130] c log2 e, dV[130] =
    sum of the dO rows and every other dK / dV row is zero.  dQ and dK[130] are exactly 0 in exact arithmetic; the kernels return
    c k (D - dO.v) p, fp32 summation noise (tests/test_hip_attention_grids.py::assert_single_key_noise_only derives the bound
    per element: |D - dO.v| <= |sum dO (o - v)| + 3 * 129 * 2^-23 sum |dO_d v_d|, times 1.01 for p and the two bf16 roundings)."""
    S, key = 320, 130
    q, k, v, dout = ar.make_inputs(B, H, S, seed=24500)
    mask = torch.zeros(B, S, dtype=torch.bool)
    mask[:, key] = True
    run, three, ref, _ = check_against_reference(ops, "single key", q, k, v, dout, mask, grads=("dv",))
    got = run.host()
    dO, V, o = dout.double(), v.double(), got["o"].double()
    slack = ((dO * (o - V[:, :, key:key + 1])).sum(-1).abs() + 3 * 129 * 2.0 ** -23 * (dO * V[:, :, key:key + 1]).abs().sum(-1))[..., None] * SCALE * 1.01
    bound_dq = slack * k[:, :, key:key + 1].double().abs()
    bound_dk = (slack * q.double().abs()).sum(2)                       # every query row adds its noise term to dK[130]
    for name, g in (("dq", got["dq"]), ("dq three-pass", three.dq.cpu())):
        assert torch.isfinite(g).all() and (g.double().abs() <= bound_dq).all(), f"{name}: more than fp32 summation noise"
    for name, g in (("dk", got["dk"]), ("dk three-pass", three.dk.cpu())):
        assert torch.isfinite(g).all() and (g[:, :, key].double().abs() <= bound_dk * (1 + 2.0 ** -8)).all(), f"{name}[130]: more than noise"


def test_masked_first_tile_with_large_logits(ops):
    """first-empty with q scaled by 8: the matched rows' logits sit ~117 log2 units above the typical score, at the edge of the
    exponent window around a reference that must come from tile 1 -- rows that outgrow it send the workgroup through the
    restart (exact maxima from the K-only pre-pass, which has to skip the masked tile as well).  Whether it ran is not asserted
    (tests/test_hip_attention_orders.py, M6 / M7, has inputs for which it must);
    that lse of every row is the fp64 log-sum-exp over the valid keys is (and o at the restart test's bound, 3e-2 / 1e-3 of absmax)."""
    S = 320
    q, k, v, dout = ar.make_inputs(B, H, S, seed=24800)
    q = (q.float() * 8).to(BF)
    mask = _whole_tile_mask("first-empty", S)
    run = Run(ops, q, k, v, dout, mask)
    got = run.host()
    ref, _ = mr.masked_ref_and_model(q, k, v, dout, SCALE, mask, lse=got["lse"], dsum=run.dsum.cpu())
    d = (got["o"].double() - ref["o"]).abs()
    amax = ref["o"].abs().max().item()
    print(f"[fwd] q x 8, first tile masked: lse max |d| {(got['lse'].double() - ref['lse']).abs().max().item():.2e} "
          f"(lse up to {ref['lse'].max().item():.1f}); o max {d.max().item() / amax:.2e} mean {d.mean().item() / amax:.2e} of absmax", flush=True)
    torch.testing.assert_close(got["lse"].double(), ref["lse"], rtol=1e-4, atol=3e-4)
    assert d.max().item() <= 3e-2 * amax and d.mean().item() <= 1e-3 * amax
    for n in ("dq", "dk", "dv"):
        assert torch.isfinite(got[n]).all()


# ---- 5. the fp32-output form ----------------------------------------------------------------------------------------------------
def test_f32_debug_form_with_the_2d_pattern(ops):
    """fk_attention_fwd_masked_f32_debug against the fp32 masked softmax(Q K^T c) V at the project's rtol 1e-3 / atol 1e-4."""
    mask = mr.pattern_2d()
    S = mask.shape[1]
    q, k, v, _ = ar.make_inputs(B, H, S, seed=25000)
    qkv = torch.zeros(B, S, 3 * D, device="cuda", dtype=BF)
    qkv[:, :, 2 * D:] = ar.token_major(v).cuda()
    out = ops.attention_f32_debug(q.cuda(), k.cuda(), qkv[:, :, 2 * D:], key_mask=ops.pack_key_mask(mask.cuda()))
    torch.cuda.synchronize()
    s = torch.einsum("bhqd,bhkd->bhqk", q.float(), k.float()) * SCALE
    s = s.masked_fill(~mask[:, None, None, :], -float("inf"))
    ref = ar.token_major(torch.softmax(s, -1) @ v.float())
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-3, atol=1e-4)
