"""Attention forward + backward (csrc/attention_fwd4.hip, csrc/attention_bwd.hip) against fp64 at the launches training
actually makes, at the S edges of every tile size, at other softmax scales, with guard rows around every output, and from an
lse that the forward's restart pass wrote.

Reference, rounding model and the row-wise bound live in tests/attention_ref.py (tests/test_attention_ref.py proves on the CPU
that the bound rejects a 1 % scale error, shifted lse / D rows, a dropped key or tile, swapped rows and a seam added twice).
Every case runs forward-with-lse, rowdot and the backward (paired and three-pass form, twice for determinism) and checks
  o     max <= 1e-2, mean <= 1e-3 of the reference's absmax (the forward test's bound; max 3e-2 in the restart case, as its test has),
  lse   against the fp64 log-sum-exp, rtol 1e-4 / atol 3e-4 (log2 units),
  D     against the fp64 row dot of dO and the bf16 o, rtol 1e-3 / atol 1e-3,
  dq, dk, dv (and the three-pass dk)  by assert_rows_close: every row within MARGIN x max(rho ||ref_r||, floor), rho from the
        bf16 rounding model, plus the per-(b, h) projection within 2^-8 -- against the fp64 gradients formed from the lse and D
        the kernel was fed.
The `[rows]` lines of a `-s` run say where the worst rows are and how much of the bound they use.
"""
import pytest
import torch

import attention_ref as ar
from attention_ref import MARGIN

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCALE = 128 ** -0.5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


class Run:
    """One forward + rowdot + backward on the device; tensors stay there until asked for."""

    def __init__(self, ops, q, k, v, dout, scale, lse=None, dsum=None, passes=1):
        B, H, S, _ = q.shape
        D = H * 128
        self.H = H
        self.qd, self.kd = q.cuda(), k.cuda()
        self.qkv = torch.zeros(B, S, 3 * D, device="cuda", dtype=BF)       # V is read in place from the fused projection buffer
        self.qkv[:, :, 2 * D:] = ar.token_major(v).cuda()
        self.doutd = ar.token_major(dout).cuda()
        vd = self.qkv[:, :, 2 * D:]
        self.o = torch.empty(B, S, D, device="cuda", dtype=BF)
        self.lse = torch.empty(B, H, S, device="cuda", dtype=torch.float32)
        ops.attention_lse(self.qd, self.kd, vd, self.o, self.lse, scale=scale)
        self.dsum = ops.rowdot(self.doutd, self.o, H)
        lse = self.lse if lse is None else lse
        dsum = self.dsum if dsum is None else dsum
        self.dq, self.dk = torch.full_like(self.qd, 5.0), torch.full_like(self.kd, 5.0)
        self.dqkv = torch.full_like(self.qkv, 5.0)
        ops.attention_bwd_set_mode(passes)
        try:
            ops.attention_bwd(self.qd, self.kd, vd, self.doutd, lse, dsum, self.dq, self.dk, self.dqkv[:, :, 2 * D:], scale=scale)
            torch.cuda.synchronize()
        finally:
            ops.attention_bwd_set_mode(1)
        assert (self.dqkv[:, :, :2 * D] == 5.0).all()                        # the q | k thirds belong to qkv_post_bwd

    def grads(self):
        return self.dq.cpu(), self.dk.cpu(), ar.head_major(self.dqkv[:, :, 2 * self.H * 128:].cpu(), self.H)

    def same_grads(self, other):
        return torch.equal(self.dq, other.dq) and torch.equal(self.dk, other.dk) and torch.equal(self.dqkv, other.dqkv)


def check_forward(tag, run, ref, dout, o_tol=(1e-2, 1e-3)):
    H = run.H
    o = ar.head_major(run.o.cpu(), H).double()
    d = (o - ref["o"]).abs()
    amax = ref["o"].abs().max().item()
    lse = run.lse.cpu().double()
    print(f"[fwd] {tag}: o max {d.max().item() / amax:.2e} mean {d.mean().item() / amax:.2e} of absmax; "
          f"lse max |d| {(lse - ref['lse']).abs().max().item():.2e} (lse in [{ref['lse'].min().item():.1f}, {ref['lse'].max().item():.1f}])", flush=True)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    assert d.max().item() <= o_tol[0] * amax and d.mean().item() <= o_tol[1] * amax, tag
    torch.testing.assert_close(lse, ref["lse"], rtol=1e-4, atol=3e-4)
    torch.testing.assert_close(run.dsum.cpu().double(), (dout.double() * o).sum(-1), rtol=1e-3, atol=1e-3)


def assert_single_key_noise_only(tag, run, three, q, k, v, dout, scale):
    """S = 1: softmax over one key is 1 whatever q and k are, so dQ = dK = 0 exactly and the row-relative bound has nothing to
    be relative to.  What the kernel returns is c k (D - dO.v) p (dK: q for k): D is rowdot's fp32 sum of the 128 products
    dO_d o_d, dO.v the MFMA chain's fp32 sum of dO_d v_d on top of D (bf16 x bf16 products are exact in fp32).  Any order of
    n fp32 additions is within n u sum|x| of the exact sum; u = 2^-23 here, since the matrix core's adders need not round to
    nearest.  rowdot: 128 terms; the chain: 129 terms, D among them, |D| <= sum |dO_d o_d|.  So
    |D - dO.v| <= |sum dO (o - v)| + 3 * 129 * 2^-23 * sum |dO_d v_d| (o = v here, up to the first term); p <= 1 + 3e-4 (the lse
    tolerance) and the two bf16 roundings (of the weight, of the result) add 2^-8 -- together a factor 1.01.  Element-wise,
    from the number formats alone; a real gradient term would be ~1e4 times larger."""
    H = run.H
    o = ar.head_major(run.o.cpu(), H).double()
    dO, V = dout.double(), v.double()
    slack = ((dO * (o - V)).sum(-1).abs() + 3 * 129 * 2.0 ** -23 * (dO * V).abs().sum(-1))[..., None] * scale * 1.01
    for name, got, other in (("dq", run.dq, k), ("dk", run.dk, q), ("dk three-pass", three.dk, q)):
        got, bound = got.cpu().double().abs(), slack * other.double().abs()
        print(f"[rows] {tag} {name}: exact gradient 0; max |got| {got.max().item():.3e}, largest share of the fp32 summation bound "
              f"{(got / bound.clamp(min=1e-300)).max().item():.3f}", flush=True)
        assert torch.isfinite(got).all() and (got <= bound).all(), f"{tag} {name}: more than fp32 summation noise where the gradient is 0"


def check_case(ops, tag, q, k, v, dout, scale, margin=MARGIN, o_tol=(1e-2, 1e-3)):
    """The whole check of one case on the launcher's current grid mode; returns the default run and the largest
    observed / model ratio of any gradient."""
    run = Run(ops, q, k, v, dout, scale)
    again = Run(ops, q, k, v, dout, scale)
    assert torch.equal(run.o, again.o) and torch.equal(run.lse, again.lse) and torch.equal(run.dsum, again.dsum), f"{tag}: forward not deterministic"
    assert run.same_grads(again), f"{tag}: backward not deterministic"
    three = Run(ops, q, k, v, dout, scale, passes=0)
    assert torch.equal(run.dq, three.dq) and torch.equal(run.dqkv, three.dqkv), f"{tag}: three-pass dQ / dV differ from the paired form"
    ref, mod = ar.attention_ref_and_model(q, k, v, dout, scale, lse=run.lse.cpu(), dsum=run.dsum.cpu())
    check_forward(tag, run, ref, dout, o_tol)
    dq, dk, dv = run.grads()
    worst = 0.0
    checks = (("dq", dq, ref["dq"], mod["dq"]), ("dk", dk, ref["dk"], mod["dk"]), ("dv", dv, ref["dv"], mod["dv"]),
              ("dk three-pass", three.dk.cpu(), ref["dk"], mod["dk3"]))
    if q.shape[2] == 1:
        assert_single_key_noise_only(tag, run, three, q, k, v, dout, scale)
        checks = checks[2:3]
    for name, got, r, m in checks:
        worst = max(worst, ar.assert_rows_close(f"{tag} {name}", got, r, m, margin=margin)["ratio"])
    print(f"[rows] {tag}: largest observed / model ratio over all gradients {worst:.3f} (margin {margin:g})", flush=True)
    return run, worst


# ---- 1. the grids training launches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,S", [(1, 24, 8704), (2, 24, 2560), (4, 24, 2560), (2, 24, 2597), (1, 24, 5632)])
def test_production_grids_against_fp64(ops, B, H, S):
    """Default launch controls at the cfg 5 shapes: the forward and the dQ pass take the stream-K grid (whole rounds + a dealt-out
    tail with up to G - 1 seams), the paired dK / dV pass B * H * ceil(S / 128) workgroups.  All 24 heads against fp64.  Then the
    same inputs on the plain grid (attention_set_split(0)): (i) the default must differ from it somewhere -- it really was the
    stream-K grid --, (ii) at most G - 1 items of 256 rows may differ, for dQ and for the forward's o / lse alike, and dK / dV
    (plain grid in both) must not differ at all.

    MARGIN = 2, from the rounding model (tests/attention_ref.py).  The observed / model ratios of an MI355X run are printed by
    the `[rows]` lines; none has been recorded here yet."""
    q, k, v, dout = ar.make_inputs(B, H, S, seed=7000 + 10 * S + B)
    run, _ = check_case(ops, f"B{B} H{H} S{S}", q, k, v, dout, SCALE)
    G = torch.cuda.get_device_properties(0).multi_processor_count
    ops.attention_set_split(0)
    try:
        plain = Run(ops, q, k, v, dout, SCALE, lse=run.lse, dsum=run.dsum)     # the backward from the SAME lse / D: only the grid differs
    finally:
        ops.attention_set_split(1)
    assert torch.equal(run.dk, plain.dk) and torch.equal(run.dqkv, plain.dqkv), "dK / dV: plain grid in both launches"
    allowed = (G - 1) * 256 / (B * H * S)
    same_dq = (run.dq == plain.dq).all(dim=-1)
    same_o = (ar.head_major(run.o, H) == ar.head_major(plain.o, H)).all(dim=-1) & (run.lse == plain.lse)
    for name, same in (("dQ", same_dq), ("forward o / lse", same_o)):
        frac = same.float().mean().item()
        pairs = int((~same).any(dim=-1).sum())
        print(f"[grid] B{B} H{H} S{S} {name}: rows bit-identical to the plain grid {frac:.5f} (bound {1 - allowed:.5f}, G = {G}), "
              f"{int((~same).sum())} rows differ, in {pairs} (b, h) pairs", flush=True)
        assert frac < 1.0, f"{name}: identical to the plain grid -- the default launch did not take the stream-K grid"
        assert frac >= 1.0 - allowed - 1e-9, f"{name}: more rows differ from the plain grid than {G - 1} cut items hold"
    # a cut item's rows differ by fp32 summation order only
    dmax = (run.dq.float() - plain.dq.float()).abs().max().item()
    assert dmax <= 2.0 ** -7 * plain.dq.float().abs().max().item()


# ---- 2. S edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 31, 32, 33, 63, 65, 127, 128, 129, 255, 256, 257, 511, 513])
def test_sequence_length_edges(ops, S):
    """S below and around every tile size: 32 (rows per wave, the forward's first-block exponent reference), 64 (streamed
    tile), 128 (dK / dV rows per item), 256 (dQ / forward rows per item).  Read before run: both forwards mask the ragged tile
    BEFORE the first-block maximum, clamp row reads to S - 1 and size their buffer descriptors to S rows; the backward kernels
    re-read the last valid row for the rows beyond S, zero their weights and store under `row < S` -- every S >= 1 is supported,
    none is refused.  S = 1 has dQ = dK = 0 exactly and is held to fp32 summation noise instead of the
    row-relative bound (assert_single_key_noise_only).  Forced grids 2 and 3 (taken where the launcher's stream_k() accepts them): with fewer than 16 tiles a cut
    snaps onto an item boundary, so there is no seam and every gradient must equal the plain grid's bit for bit."""
    B, H = 2, 3
    q, k, v, dout = ar.make_inputs(B, H, S, seed=9000 + S)
    run, _ = check_case(ops, f"edge S{S}", q, k, v, dout, SCALE)
    for grid in (2, 3):
        ops.attention_set_split(grid)
        try:
            forced = Run(ops, q, k, v, dout, SCALE, lse=run.lse, dsum=run.dsum)
            forced3 = Run(ops, q, k, v, dout, SCALE, lse=run.lse, dsum=run.dsum, passes=0)
        finally:
            ops.attention_set_split(1)
        assert torch.equal(forced.o, run.o) and torch.equal(forced.lse, run.lse), f"forward on {grid} workgroups"
        assert forced.same_grads(run), f"backward on {grid} workgroups"
        assert torch.equal(forced3.dq, run.dq) and torch.equal(forced3.dqkv, run.dqkv), f"three-pass backward on {grid} workgroups"


# ---- 3. softmax scale ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.03, 128 ** -0.5, 0.25])
@pytest.mark.parametrize("B,H,S", [(1, 2, 300), (2, 3, 1000)])
def test_softmax_scale(ops, B, H, S, scale):
    """`scale` enters the exponent (scale * log2 e) and the store (dQ, dK) separately; 0.03 is nearly uniform attention, 0.25
    one-hot on the matched rows (logit ~ 29 nats, inside the forward's exponent window: no restart)."""
    q, k, v, dout = ar.make_inputs(B, H, S, seed=11000 + S)
    check_case(ops, f"scale {scale:.4f} B{B} H{H} S{S}", q, k, v, dout, scale)


# ---- 4. guard rows and strided views ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [75, 257, 1000])
def test_guard_rows_and_strided_views(ops, S):
    """Every output inside a larger sentinel-filled allocation: dq / dk as [:, :, :S] of [B, H, S + 40, 128] (head stride !=
    S * 128), dv / dout / o as column slices of wider token-major buffers, lse and D exact-size windows of longer fp32 buffers.
    Same bits as the contiguous run, sentinels intact."""
    B, H, PAD = 2, 3, 40
    D = H * 128
    q, k, v, dout = ar.make_inputs(B, H, S, seed=13000 + S)
    base, _ = check_case(ops, f"guard S{S}", q, k, v, dout, SCALE)
    n = B * H * S
    stats = torch.full((2, n + 128), 12345.0, device="cuda", dtype=torch.float32)
    lse, dsum = stats[0, 64:64 + n].view(B, H, S), stats[1, 64:64 + n].view(B, H, S)
    o_wide = torch.full((B, S + 3, D + 64), 5.0, device="cuda", dtype=BF)
    dout_wide = torch.full((B, S, D + 64), 5.0, device="cuda", dtype=BF)
    dout_wide[:, :, 64:] = base.doutd
    dq_big = torch.full((B, H, S + PAD, 128), 5.0, device="cuda", dtype=BF)
    dk_big = torch.full((B, H, S + PAD, 128), 5.0, device="cuda", dtype=BF)
    dv_wide = torch.full((B, S + 3, 3 * D + 64), 5.0, device="cuda", dtype=BF)
    vd = base.qkv[:, :, 2 * D:]
    o, dv = o_wide[:, :S, :D], dv_wide[:, :S, 2 * D:3 * D]
    ops.attention_lse(base.qd, base.kd, vd, o, lse)
    ops.rowdot(dout_wide[:, :, 64:], o, H, out=dsum)
    ops.attention_bwd(base.qd, base.kd, vd, dout_wide[:, :, 64:], lse, dsum, dq_big[:, :, :S], dk_big[:, :, :S], dv)
    torch.cuda.synchronize()
    assert torch.equal(o, base.o) and torch.equal(lse, base.lse) and torch.equal(dsum, base.dsum)
    assert torch.equal(dq_big[:, :, :S], base.dq) and torch.equal(dk_big[:, :, :S], base.dk) and torch.equal(dv, base.dqkv[:, :, 2 * D:])
    assert (stats[:, :64] == 12345.0).all() and (stats[:, 64 + n:] == 12345.0).all(), "lse / D: written outside [B, H, S]"
    assert (o_wide[:, S:] == 5.0).all() and (o_wide[:, :, D:] == 5.0).all(), "o: written outside its view"
    assert (dq_big[:, :, S:] == 5.0).all(), "dq: rows beyond S written"
    assert (dk_big[:, :, S:] == 5.0).all(), "dk: rows beyond S written"
    assert (dv_wide[:, S:] == 5.0).all() and (dv_wide[:, :, :2 * D] == 5.0).all() and (dv_wide[:, :, 3 * D:] == 5.0).all(), "dv: written outside its view"
    assert (dout_wide[:, :, :64] == 5.0).all()


# ---- 5. the restart pass's lse feeds the backward -----------------------------------------------------------------------------
def test_backward_from_the_restart_pass_lse(ops):
    """The inputs of test_hip_kernels.py::test_attention_restart_on_late_large_logit at gain 12 (a logit ~196 log2 units above
    the first block's reference turns the first pass's sums into inf; the forward repeats the pass with exact row maxima).
    lse of EVERY row, the two hit rows included, against the fp64 log-sum-exp; then the backward from that lse: finite, and
    within the row bound."""
    B, H, S, gain = 1, 2, 640, 12.0
    g = torch.Generator().manual_seed(77)
    q = torch.randn(B, H, S, 128, generator=g).to(BF)
    k = torch.randn(B, H, S, 128, generator=g).to(BF)
    qkv = torch.randn(B, S, 3 * H * 128, generator=g).to(BF)
    k[0, 0, 600] = q[0, 0, 5] * gain
    k[0, 1, 321] = q[0, 1, 400] * (gain - 1.0)
    v = ar.head_major(qkv[:, :, 2 * H * 128:], H).contiguous()
    dout = ar.make_inputs(B, H, S, seed=78)[3]
    # o: the existing restart test's bound (3e-2 of absmax), with the usual bound on the mean
    run, _ = check_case(ops, "restart gain 12", q, k, v, dout, SCALE, o_tol=(3e-2, 1e-3))
    lse = run.lse.cpu()
    assert lse[0, 0, 5].item() > 150 and lse[0, 1, 400].item() > 150       # the hit rows really carry the large logit
