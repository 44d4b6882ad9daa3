"""The two instruction orders of the 8-wave attention forward (csrc/attention_fwd.hip: `do_tile`, ILV = false / true), run
against each other bit for bit and against fp64 -- key-masked forms, the masked restart pass and a forced stream-K grid
included.  "Bit-identical results", says the kernel's comment of the two orders; this file holds it to that.

Which instantiation runs where
------------------------------
The library reads FK_ATTN_KERNEL and FK_ATTN_ILV once per process.  tests/attention_orders_child.py is started twice, one
fresh process after the other (the second only if the first succeeded):

    child 0   FK_ATTN_KERNEL=8 FK_ATTN_ILV=0     child 1   FK_ATTN_KERNEL=8 FK_ATTN_ILV=1

so that in child c every call is FORCED to attention_fwd_kernel<8, false, ILV = c, STREAMK, KMASK>:

    M1 .. M7  key_mask given             <8, false, c, false, true>    the masked copy; no test reached it with ILV = true
    U1, U2    plain grid                 <8, false, c, false>
    U3        attention_set_split(0)     <8, false, c, false>
              attention_set_split(7)     <8, false, c, true>           20 items x 18 tiles on 7 workgroups: cut items, seams

The masked cases (B = 2, H = 2, inputs from attention_ref.make_inputs, outputs in the sentinel-guarded windows of
test_hip_attention_mask.Run, forward with lse + rowdot + paired backward):
    M1  the 2-D padding pattern, S = 357: partial tiles throughout, an all-masked last tile
    M2  first-empty, M3 last-empty, S = 320
    M4  first-block-empty: block 0 of the first valid tile is empty, so the ILV copy issues block 0's exponentials against
        the initial reference and takes the real one from block 1 (`if ((uint32_t)kw == 0) m_ref = block_max(s1) + ...`)
    M5  a single valid key (130)
    M6  the restart under a mask: two valid hits 197.2 / 127.2 log2 units above their rows' first-pass reference (fp32 ends at
        2^128: the first row's sum, and both rows' O, are inf), so only the repeated pass gives finite rows; two masked decoys
        at gain 14
    M7  M6 plus four masked decoys on rows of the two items that DO restart, one per kind of tile the K-only pre-pass tells
        apart (whole / partial / empty word).  M6's own decoys lie in items (b, h) = (0, 1) and (1, 0), which never run the
        pre-pass; these are the keys that tell a pre-pass that forgot the mask from one that did not: it would leave the row
        with l = 0 and lse = -inf (attention_orders_child.restart_case).

In the parent process (default environment: the 4-wave kernel for unmasked calls, the launcher's own choice of order):
    U1 .. U3 again, for "the two kernels give the same bits" at the interleaved order, the restart and the forced grid;
    test_launcher_rule_picks_the_interleaved_copy: B = 4, H = 128, S = 200 is n_items = 512, the first count at which
    `use_interleaved` (csrc/attention_fwd.hip) says yes without FK_ATTN_ILV.  That threshold is read from the source; the
    children, not that test, guarantee that both copies run.

Bounds (the project's own, none new): child 0 == child 1 with torch.equal, everything finite; masked cases of child 1 against
test_attention_mask_ref.masked_ref_and_model formed from the lse and D the backward was fed: lse rtol 1e-4 / atol 3e-4 (log2
units), o / dq / dk / dv by attention_ref.assert_rows_close at MARGIN = 2, dK / dV rows of masked keys == 0; M5 the
single-key fp32 summation noise bound of test_hip_attention_mask.py::test_single_valid_key; M6 / M7 o at the restart bound of
test_hip_attention_grids.py (max 3e-2, mean 1e-3 of absmax), gradients at MARGIN.

Observed on an MI355X: see RECORDED below.
"""
import os
import subprocess
import sys

import pytest
import torch

import attention_orders_child as cases
import attention_ref as ar
import test_attention_mask_ref as mr
from attention_ref import MARGIN

gpu = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
SCALE = cases.SCALE

# `[rows]` / `[fwd]` lines of one MI355X run of this file (observed / model, the margin each result would have needed; bound 2.0)
RECORDED = """
child 1 (ILV = 1)               o      dq     dk     dv      lse max |d| (log2 units; bound rtol 1e-4 / atol 3e-4)
M1 2-D padding S357             1.196  0.876  1.000  0.912   3.45e-06
M2 first-empty                  0.974  0.957  1.000  0.903   3.61e-06
M3 last-empty                   1.044  0.852  1.000  1.000   3.57e-06
M4 first-block-empty            1.324  0.968  1.000  0.792   3.29e-06
M5 single key                   0.000  -      -      1.000   1.16e-06
M6 restart, masked decoys       -      0.930  1.000  0.942   1.43e-05 with lse in [7.6, 225.5]; o max 4.25e-03, mean 1.19e-04 of absmax
M7 restart, pre-pass decoys     -      0.930  1.000  0.942   1.43e-05 with lse in [7.6, 225.5]; o max 4.25e-03, mean 1.19e-04 of absmax
launcher rule B4 H128 S200      1.190  -      -      -       5.68e-06 with lse in [7.0, 24.3]
(M1 .. M5 are the figures tests/test_hip_attention_mask.py records for the non-interleaved order, digit for digit: the two
orders gave the same bits in all 50 tensors, and U1 .. U3 the bits of the 4-wave kernel.  M6 and M7 share every valid
quantity; o needed at most 1.32 of the allowed 2.0.)
"""


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from gpt_image_edit_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def masked():
    return cases.masked_cases()


@pytest.fixture(scope="module")
def plain():
    return cases.plain_cases()


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """The saved results of child 0 (ILV = 0) and child 1 (ILV = 1).  One after the other; check=True: if the first fails or
    runs into the time limit (the bound for a hung child, not an expected duration) the second is never started."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    out = tmp_path_factory.mktemp("attention_orders")
    res = []
    for ilv in ("0", "1"):
        path = out / f"ilv{ilv}.pt"
        env = dict(os.environ, FK_ATTN_KERNEL="8", FK_ATTN_ILV=ilv)
        subprocess.run([sys.executable, os.path.join(tests, "attention_orders_child.py"), root, str(path)], env=env, check=True, timeout=600)
        res.append(torch.load(path))
        assert res[-1].pop("env") == ("8", ilv)
    return res


# ---- CPU: the cases are what the docstring says -----------------------------------------------------------------------------------
def masked_forward_ref(q, k, v, scale, mask):
    """Forward only, one sample at a time: (o, lse, model o) as masked_ref_and_model forms them -- fp64 softmax over the valid
    keys, lse in log2 units, model = bf16(bf16(P) V)."""
    Bq, Hq, S, _ = q.shape
    o = torch.empty(Bq, Hq, S, 128, dtype=F64)
    mod = torch.empty_like(o)
    lse = torch.empty(Bq, Hq, S, dtype=F64)
    for b in range(Bq):
        s2 = torch.einsum("hqd,hkd->hqk", q[b].to(F64), k[b].to(F64)) * (scale * ar.LOG2E)
        s2 = s2.masked_fill(~mask[b].bool()[None, None, :], -float("inf"))
        m = s2.max(dim=-1, keepdim=True).values
        P = torch.exp2(s2 - m)
        l = P.sum(-1, keepdim=True)
        P /= l
        lse[b] = (m + torch.log2(l))[..., 0]
        o[b] = P @ v[b].to(F64)
        mod[b] = ar.bf16r(ar.bf16r(P) @ v[b].to(F64))
    return o, lse, mod


def test_forward_only_reference_is_the_masked_reference(masked):
    q, k, v, dout, mask = masked["M4 first-block-empty"]
    ref, model = mr.masked_ref_and_model(q, k, v, dout, SCALE, mask)
    o, lse, mod = masked_forward_ref(q, k, v, SCALE, mask)
    torch.testing.assert_close(o, ref["o"], rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(lse, ref["lse"], rtol=1e-12, atol=1e-12)
    # the same roundings; the two fp64 score sums differ in their last bits, which moves a bf16 tie now and then
    assert (mod != model["o"]).double().mean().item() < 1e-3
    assert (mod - model["o"]).abs().max().item() <= 2.0 ** -7 * ref["o"].abs().max().item()


def test_restart_case_needs_the_restart_and_its_decoys_tell(masked):
    """M6 / M7 in fp64: each hit overflows the first pass (the row's reference is REF_BIAS = 24 above the maximum of the first
    32-key block with a valid key; fp32 ends at 2^128): row (0, 0, 5) sits 197.2 log2 units above its reference -- numerator
    and row sum inf --, row (1, 1, 260) 127.2 -- the numerator 2^127.2 is still finite, its product with v[170] (largest entry
    2.98 = 2^1.58) is not, which the kernel's check of O sees as well.  The decoy rows' lse is small with the mask and ~150 or
    more without it, and the two forms have one reference."""
    for name in ("M6 restart, masked decoys", "M7 restart, decoys in the pre-pass"):
        q, k, v, _, mask = masked[name]
        _, lse, _ = masked_forward_ref(q, k, v, SCALE, mask)
        _, lse_all, _ = masked_forward_ref(q, k, v, SCALE, torch.ones_like(mask))
        s2 = torch.einsum("bhqd,bhkd->bhqk", q.to(F64), k.to(F64)) * (SCALE * ar.LOG2E)
        for (b, h, row), key, least in zip(cases.HITS, cases.HIT_KEYS, (190.0, 127.0)):
            first = int(mask[b].nonzero()[0]) // 32 * 32              # the first 32-key block with a valid key
            block = s2[b, h, row, first:first + 32][mask[b, first:first + 32]]
            excess = (s2[b, h, row, key] - (block.max() + 24.0)).item()
            assert mask[b, key] and lse[b, h, row] > 150 and excess > least, (name, b, h, row, excess)
            assert excess + torch.log2(v[b, h, key].double().abs().max()).item() > 128.5, (name, b, h, row, excess)
        assert abs(lse[0, 0, 5].item() - 225.5) < 0.1
        rows = list(cases.DECOYS) + ([(b, h, r) for b, h, _, r in cases.PREPASS_DECOYS] if name.startswith("M7") else [])
        for (b, h, row) in rows:
            assert lse[b, h, row] < 20 and lse_all[b, h, row] > 145, (name, b, h, row, lse[b, h, row], lse_all[b, h, row])
    assert abs(lse_all[0, 1, 7].item() - 152.0) < 0.1
    a, c = masked["M6 restart, masked decoys"], masked["M7 restart, decoys in the pre-pass"]
    valid = a[4]
    assert torch.equal(a[4], c[4]) and torch.equal(a[1].transpose(1, 2)[valid], c[1].transpose(1, 2)[valid])      # only masked keys differ
    # a restarting item is a (b, h, 256-row block): the pre-pass decoys share one with a hit, the plain decoys do not
    items = {(b, h, r // 256) for b, h, r in cases.HITS}
    assert {(b, h, r // 256) for b, h, _, r in cases.PREPASS_DECOYS} == items
    assert not {(b, h, r // 256) for b, h, r in cases.DECOYS} & items


def test_launcher_rule_masks_are_what_the_docstring_says():
    m = launcher_rule_masks()
    words = mr.pack(m)
    assert tuple(m.shape) == (4, 200) and m.any(dim=1).all()
    assert int(m[0].sum()) == 40 + 7 * 11 and m[0, :40].all() and int(words[0, 0]) not in (0, -1)      # 2-D padding: partial tiles
    assert int(words[1, 0]) == 0 and (words[1, 1:3] == -1).all()                         # first tile empty
    assert int(words[2, 0]) & 0xFFFFFFFF == 0 and int(words[2, 0]) != 0                  # first block empty + half of the second
    assert int(words[3, 3]) == 0 and (words[3, :3] == -1).all()                          # last (ragged) tile empty


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_orders_agree_bit_for_bit(children):
    """Every saved tensor of child 0 (ILV = 0) equals child 1's (ILV = 1) and is finite: masked forward and lse, the backward
    run from them, the plain grid, the restart and the forced stream-K grid."""
    a, b = children
    assert a.keys() == b.keys() and len(a) == 7 * 6 + 4 * 2
    for name in a:
        assert torch.isfinite(a[name].float()).all() and torch.isfinite(b[name].float()).all(), f"{name}: non-finite"
        assert torch.equal(a[name], b[name]), f"{name}: {(a[name].float() - b[name].float()).abs().max().item()} max difference between the orders"
        assert not name.endswith(("/o", "/lse")) or a[name].float().abs().max().item() > 0


def _masked_keys_are_zero(tag, got, mask):
    for n in ("dk", "dv"):
        assert (got[n].transpose(1, 2)[~mask] == 0).all(), f"{tag}: {n} rows of masked keys must be exact zeros"


def _lse_check(tag, got, ref):
    lse = got["lse"].double()
    print(f"[fwd] {tag}: lse max |d| {(lse - ref['lse']).abs().max().item():.2e} (lse in [{ref['lse'].min().item():.1f}, "
          f"{ref['lse'].max().item():.1f}])", flush=True)
    assert torch.isfinite(lse).all()
    torch.testing.assert_close(lse, ref["lse"], rtol=1e-4, atol=3e-4)


def _case_of(children, name):
    return {n: children[1][f"{name}/{n}"] for n in ("o", "lse", "dq", "dk", "dv", "dsum")}


@gpu
@pytest.mark.parametrize("name", ["M1 2-D padding S357", "M2 first-empty", "M3 last-empty", "M4 first-block-empty"])
def test_interleaved_masked_cases_against_fp64(children, masked, name):
    """Child 1's tensors as test_hip_attention_mask.check_against_reference holds them (the guards and the packed mask were
    asserted in the child by test_hip_attention_mask.Run)."""
    q, k, v, dout, mask = masked[name]
    got = _case_of(children, name)
    ref, mod = mr.masked_ref_and_model(q, k, v, dout, SCALE, mask, lse=got["lse"], dsum=got["dsum"])
    _lse_check(name, got, ref)
    torch.testing.assert_close(got["dsum"].double(), (dout.double() * got["o"].double()).sum(-1), rtol=1e-3, atol=1e-3)
    _masked_keys_are_zero(name, got, mask)
    ratios = {n: ar.assert_rows_close(f"{name} {n}", got[n], ref[n], mod[n], margin=MARGIN)["ratio"] for n in ("o", "dq", "dk", "dv")}
    print(f"[rows] {name}: observed / model " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()) + f" (margin {MARGIN:g})", flush=True)


@gpu
def test_interleaved_single_valid_key(children, masked):
    """M5: o = v[130], dV[130] = the sum of the dO rows, by the row bound; dQ and dK[130] are 0 in exact arithmetic and held
    to the fp32 summation noise bound of test_hip_attention_mask.py::test_single_valid_key."""
    name, key = "M5 single key", 130
    q, k, v, dout, mask = masked[name]
    got = _case_of(children, name)
    ref, mod = mr.masked_ref_and_model(q, k, v, dout, SCALE, mask, lse=got["lse"], dsum=got["dsum"])
    _lse_check(name, got, ref)
    _masked_keys_are_zero(name, got, mask)
    ratios = {n: ar.assert_rows_close(f"{name} {n}", got[n], ref[n], mod[n], margin=MARGIN)["ratio"] for n in ("o", "dv")}
    print(f"[rows] {name}: observed / model " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()) + f" (margin {MARGIN:g})", flush=True)
    dO, V, o = dout.double(), v.double(), got["o"].double()
    slack = ((dO * (o - V[:, :, key:key + 1])).sum(-1).abs() + 3 * 129 * 2.0 ** -23 * (dO * V[:, :, key:key + 1]).abs().sum(-1))[..., None] * SCALE * 1.01
    bound_dq = slack * k[:, :, key:key + 1].double().abs()
    bound_dk = (slack * q.double().abs()).sum(2)
    assert torch.isfinite(got["dq"]).all() and (got["dq"].double().abs() <= bound_dq).all(), "dq: more than fp32 summation noise"
    assert torch.isfinite(got["dk"]).all() and (got["dk"][:, :, key].double().abs() <= bound_dk * (1 + 2.0 ** -8)).all(), "dk[130]: more than noise"


@gpu
@pytest.mark.parametrize("name", ["M6 restart, masked decoys", "M7 restart, decoys in the pre-pass"])
def test_interleaved_masked_restart(children, masked, name):
    """lse of every row against fp64 (the hits are real: > 150; no masked key's logit reached a sum, a first-pass reference or
    the pre-pass maximum: the decoy rows < 20), o at the restart bound, the backward from the restart pass's lse at MARGIN."""
    q, k, v, dout, mask = masked[name]
    got = _case_of(children, name)
    ref, mod = mr.masked_ref_and_model(q, k, v, dout, SCALE, mask, lse=got["lse"], dsum=got["dsum"])
    _lse_check(name, got, ref)
    d = (got["o"].double() - ref["o"]).abs()
    amax = ref["o"].abs().max().item()
    print(f"[fwd] {name}: o max {d.max().item() / amax:.2e} mean {d.mean().item() / amax:.2e} of absmax (bounds 3e-2 / 1e-3)", flush=True)
    assert d.max().item() <= 3e-2 * amax and d.mean().item() <= 1e-3 * amax
    lse = got["lse"]
    assert lse[0, 0, 5].item() > 150 and lse[1, 1, 260].item() > 150
    assert lse[0, 1, 7].item() < 20 and lse[1, 0, 33].item() < 20
    if name.startswith("M7"):
        for b, h, _, row in cases.PREPASS_DECOYS:
            assert lse[b, h, row].item() < 20, (b, h, row)
    torch.testing.assert_close(got["dsum"].double(), (dout.double() * got["o"].double()).sum(-1), rtol=1e-3, atol=1e-3)
    _masked_keys_are_zero(name, got, mask)
    ratios = {n: ar.assert_rows_close(f"{name} {n}", got[n], ref[n], mod[n], margin=MARGIN)["ratio"] for n in ("dq", "dk", "dv")}
    print(f"[rows] {name}: observed / model " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()) + f" (margin {MARGIN:g})", flush=True)


@gpu
def test_unmasked_forms_equal_the_parent_process_bit_for_bit(ops, children, plain):
    """U1 .. U3 in this process (default environment: the 4-wave kernel unless FK_ATTN_KERNEL says otherwise) on the same grid
    setting, against both children: the two kernels' same bits at the interleaved order, the restart and a 7-workgroup grid."""
    for name, (q, k, v, grids) in plain.items():
        for grid in grids:
            o, lse = cases.run_plain(ops, q, k, v, grid)
            assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
            for c, child in enumerate(children):
                assert torch.equal(child[f"{name}/grid {grid}/o"], o), f"{name} grid {grid}: o of child {c} differs from this process"
                assert torch.equal(child[f"{name}/grid {grid}/lse"], lse), f"{name} grid {grid}: lse of child {c} differs from this process"
    name = "U3 B1 H4 S1100"                                    # the forced grid did cut items: it differs from the plain grid somewhere
    assert not torch.equal(children[1][f"{name}/grid 7/o"], children[1][f"{name}/grid 0/o"])
    lse = children[1]["U2 B1 H2 S640 restart/grid 1/lse"]
    assert lse[0, 0, 5].item() > 150 and lse[0, 1, 400].item() > 150        # U2's hit rows carry the large logit: the restart ran


def launcher_rule_masks(S=200):
    """Four samples: 2-D-style padding (40 text keys, then a 10 x 16 grid of which the 7 x 11 corner is real); first tile
    empty; first block empty plus half of the second; last (ragged) tile empty."""
    m = torch.ones(4, S, dtype=torch.bool)
    g = torch.zeros(10, 16, dtype=torch.bool)
    g[:7, :11] = True
    m[0, 40:] = g.flatten()
    m[1, :64] = False
    m[2, :48] = False
    m[3, 192:] = False
    return m


@gpu
def test_launcher_rule_picks_the_interleaved_copy(ops):
    """No forced order: B = 4, H = 128, S = 200 gives n_items = B * H * ceil(S / 256) = 512, the first count at which
    `use_interleaved` in csrc/attention_fwd.hip answers yes (`p.n_items >= 512`, read from the source, not observable from
    here -- the children above, not this test, guarantee that both copies run).  Four different sample masks; forward with
    lse against the masked fp64 reference at the bounds of the cases above; V its own [B, S, H * 128] buffer; o and lse in
    sentinel-guarded windows."""
    if "FK_ATTN_ILV" in os.environ:
        pytest.skip("FK_ATTN_ILV is set: the launcher's own rule is not what picks the order")
    Bq, Hq, S = 4, 128, 200
    D = Hq * 128
    q, k, v, _ = ar.make_inputs(Bq, Hq, S, seed=29000)
    mask = launcher_rule_masks(S)
    n = Bq * Hq * S
    stats = torch.full((n + 128,), 12345.0, device="cuda", dtype=torch.float32)
    lse = stats[64:64 + n].view(Bq, Hq, S)
    o_wide = torch.full((Bq, S + 3, D + 64), 5.0, device="cuda", dtype=BF)
    o = o_wide[:, :S, :D]
    km = ops.pack_key_mask(mask.cuda())
    assert torch.equal(km.cpu(), mr.pack(mask))
    ops.attention_lse(q.cuda(), k.cuda(), ar.token_major(v).cuda(), o, lse, scale=SCALE, key_mask=km)
    torch.cuda.synchronize()
    assert (stats[:64] == 12345.0).all() and (stats[64 + n:] == 12345.0).all(), "lse: written outside [B, H, S]"
    assert (o_wide[:, S:] == 5.0).all() and (o_wide[:, :, D:] == 5.0).all(), "o: written outside its view"
    ref_o, ref_lse, mod_o = masked_forward_ref(q, k, v, SCALE, mask)
    tag = "launcher rule B4 H128 S200"
    _lse_check(tag, dict(lse=lse.cpu()), dict(lse=ref_lse))
    r = ar.assert_rows_close(f"{tag} o", ar.head_major(o.cpu(), Hq), ref_o, mod_o, margin=MARGIN)["ratio"]
    print(f"[rows] {tag}: observed / model o {r:.3f} (margin {MARGIN:g})", flush=True)
