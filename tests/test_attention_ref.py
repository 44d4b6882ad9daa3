"""CPU tests of the attention checker (tests/attention_ref.py): the reference agrees with torch, the rounding model passes
its own bound, and every subtle defect a kernel could have is REJECTED -- which is what makes a green
tests/test_hip_attention_grids.py mean something.

The defects are built on the reference side: the rounding model is run with the mutation and plays the wrong kernel
(`got`); reference and bound come from the unmutated computation.  Each must fail at MAX_MARGIN = 4, the loosest margin a
GPU case may ever use, and the gradients a defect does not touch must still pass at MARGIN = 2.
"""
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar

SCALE = 128 ** -0.5


class Case:
    def __init__(self, S):
        self.S = S
        self.q, self.k, self.v, self.dout = ar.make_inputs(1, 1, S, seed=500 + S)
        ref, mod = ar.attention_ref_and_model(self.q, self.k, self.v, self.dout, SCALE)
        self.ref, self.mod = ref, mod
        self.D = (self.dout.double() * ref["o"]).sum(-1)

    def model(self, scale=SCALE, lse=None, dsum=None, weight=None):
        lse = self.ref["lse"] if lse is None else lse
        dsum = self.D if dsum is None else dsum
        dq, dk, dv, _ = ar.attention_bwd_model(self.q, self.k, self.v, self.dout, scale, lse, dsum, weight=weight)
        return dict(dq=dq, dk=dk, dv=dv)

    def block(self, rows, cols, value):
        """weight hook: `value` on rows x cols of the [S, S] weight matrix, 1 elsewhere."""
        def weight(r0, r1):
            w = torch.ones(r1 - r0, self.S, dtype=torch.float64)
            lo, hi = max(rows[0], r0), min(rows[1], r1)
            if lo < hi:
                w[lo - r0:hi - r0, cols[0]:cols[1]] = value
            return w
        return weight

    def verdicts(self, got, margin):
        out = {}
        for n in ("dq", "dk", "dv"):
            try:
                ar.assert_rows_close(f"S{self.S} {n}", got[n], self.ref[n], self.mod[n], margin=margin)
                out[n] = None
            except AssertionError as e:
                out[n] = str(e)
        return out


@pytest.fixture(scope="module", params=[333, 1000])
def case(request):
    return Case(request.param)


def test_inputs_are_peaked_and_rows_differ(case):
    """The builder's claims: matched rows are dominated by one key, and lse varies from row to row (so a row shift is visible)."""
    s = (case.q.double()[0, 0] @ case.k.double()[0, 0].t()) * SCALE
    pmax = torch.softmax(s, -1).max(-1).values
    assert pmax[::3].mean().item() > 0.5 and pmax[1::3].mean().item() < 0.5
    assert torch.logsumexp(s, -1).std().item() > 0.5
    norms = case.dout.double().norm(dim=-1)
    assert norms.max().item() / norms.min().item() > 64


def test_reference_agrees_with_torch_autograd(case):
    """attention_ref64 against an independent fp32 autograd SDPA gradient: 1e-5 of each tensor's scale."""
    o, lse, dq, dk, dv = ar.attention_ref64(case.q, case.k, case.v, case.dout, SCALE)
    qr, kr, vr = (t.float().requires_grad_(True) for t in (case.q, case.k, case.v))
    out = F.scaled_dot_product_attention(qr, kr, vr)
    out.backward(case.dout.float())
    for name, mine, theirs in (("o", o, out.detach()), ("dq", dq, qr.grad), ("dk", dk, kr.grad), ("dv", dv, vr.grad)):
        err = (mine - theirs.double()).abs().max().item()
        assert err <= 1e-5 * mine.abs().max().item(), f"{name}: {err:.3e}"
    s = (case.q.double() @ case.k.double().transpose(-1, -2)) * SCALE
    torch.testing.assert_close(lse, torch.logsumexp(s, -1) * ar.LOG2E, rtol=1e-12, atol=1e-12)
    # and the single-sweep form is the same computation
    for n, t in zip(("o", "lse", "dq", "dk", "dv"), (o, lse, dq, dk, dv)):
        assert torch.equal(case.ref[n], t)


def test_model_passes_its_own_bound(case):
    """MARGIN = 1 by construction; rho is a few 1e-3 (bf16: 2^-9 per rounding); the model's systematic part is well below the
    projection bound.  How far below: a peaked row is dominated by ONE bf16 weight whose relative rounding error (uniform in
    +-2^-9, rms 2^-9 / sqrt(3) = 1.1e-3) is shared by the row's 128 elements; the projection averages the S / 3 such rows
    weighted by their squared norm, and with dO scaled by 2^-4..2^4 the ninth of them at the top scale carries the sum:
    a sigma of ~1.1e-3 / sqrt(S / 27) = 2 to 3e-4 at these S, less at the training sizes -- held to a quarter of the bound here."""
    for n, m in (("dq", "dq"), ("dk", "dk"), ("dv", "dv"), ("dk", "dk3")):
        r = ar.assert_rows_close(f"S{case.S} model {m}", case.mod[m], case.ref[n], case.mod[m], margin=1.0)
        assert r["ratio"] <= 1.0 + 1e-9 and 1e-3 <= r["rho"] <= 1e-2, r
        assert r["proj_model"] <= ar.PROJ_TOL / 4 and r["proj"] == r["proj_model"], r
    # the three-pass dK (w from the fp32 p) within the paired pass's bound as well
    ar.assert_rows_close(f"S{case.S} dk3 under the paired bound", case.mod["dk3"], case.ref["dk"], case.mod["dk"])


def test_model_with_the_given_lse_and_dsum_is_the_same_function(case):
    got = case.model()
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], case.mod[n])


def _expect(case, got, rejected, why=None):
    v4 = case.verdicts(got, ar.MAX_MARGIN)
    for n in rejected:
        assert v4[n] is not None, f"{n} was accepted"
        if why:
            assert why in v4[n], v4[n]
    v2 = case.verdicts(got, ar.MARGIN)
    for n in ("dq", "dk", "dv"):
        if n not in rejected:
            assert v2[n] is None, f"{n} is untouched by this defect but was rejected: {v2[n]}"


def test_rejects_uniform_one_percent_scale_error(case):
    """What the absmax check lets through: every gradient 1 % too large.  The row bound (2 rho ~ 1e-2) cannot see it; the
    per-head projection must."""
    got = {n: ar.bf16r(case.mod[n] * 1.01) for n in ("dq", "dk", "dv")}
    _expect(case, got, ("dq", "dk", "dv"), why="projection")


def test_rejects_store_scale_off_by_one_percent(case):
    """p.scale at the store 1 % off while the exponent's scale is right: dQ and dK 1 % too large, dV untouched."""
    got = dict(case.mod)
    got["dq"], got["dk"] = ar.bf16r(case.mod["dq"] * 1.01), ar.bf16r(case.mod["dk"] * 1.01)
    _expect(case, got, ("dq", "dk"), why="projection")


def test_rejects_scale_times_1_01_in_both_places(case):
    _expect(case, case.model(scale=SCALE * 1.01), ("dq", "dk", "dv"))


@pytest.mark.parametrize("shift", [1, 64])
def test_rejects_lse_taken_from_another_row(case, shift):
    _expect(case, case.model(lse=torch.roll(case.ref["lse"], -shift, dims=-1)), ("dq", "dk", "dv"))


def test_rejects_dsum_zeroed_for_one_head(case):
    _expect(case, case.model(dsum=torch.zeros_like(case.D)), ("dq", "dk"))


def test_rejects_last_key_dropped(case):
    S = case.S
    _expect(case, case.model(weight=case.block((0, S), (S - 1, S), 0.0)), ("dq", "dk", "dv"))


def test_rejects_one_dropped_tile_of_one_item(case):
    """One 64-column tile missing from one 256-row item."""
    _expect(case, case.model(weight=case.block((256, 512), (64, 128), 0.0)), ("dq", "dk", "dv"))


def test_rejects_two_adjacent_dk_rows_swapped(case):
    got = dict(case.mod)
    dk = case.mod["dk"].clone()
    dk[0, 0, [200, 201]] = dk[0, 0, [201, 200]]
    got["dk"] = dk
    _expect(case, got, ("dk",))


def test_rejects_a_seam_partial_added_twice(case):
    """The rows of one 256-row item counted twice over 8 column tiles."""
    got = case.model(weight=case.block((256, 512), (0, 512), 2.0))
    got["dk"], got["dv"] = case.mod["dk"], case.mod["dv"]          # the dQ pass's seam
    _expect(case, got, ("dq",))


def test_rows_below_the_floor_are_held_to_the_floor():
    """A row whose reference is ~0 is not excluded: garbage there fails, half-ulp noise at the tensor's scale passes."""
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(1, 2, 40, 128, generator=g, dtype=torch.float64)
    ref[0, 1, 7] = 0
    model = ar.bf16r(ref)
    ar.assert_rows_close("zero row", model, ref, model, margin=1.0)
    bad = model.clone()
    bad[0, 1, 7] = 0.05
    with pytest.raises(AssertionError, match=r"\(0, 1, 7\)"):
        ar.assert_rows_close("zero row, garbage", bad, ref, model, margin=ar.MAX_MARGIN)
    nan = model.clone()
    nan[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError, match="non-finite"):
        ar.assert_rows_close("nan", nan, ref, model)
