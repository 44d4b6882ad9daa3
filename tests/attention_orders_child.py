"""The cases of tests/test_hip_attention_orders.py and the child process that runs them (plain module, not collected).

The library reads FK_ATTN_KERNEL and FK_ATTN_ILV once per process, so each instruction order of the 8-wave forward
(csrc/attention_fwd.hip) needs a process of its own:

    python attention_orders_child.py <repository root> <output file>

builds every case below from its seed on the CPU, runs it through `ops` under whatever FK_ATTN_* the environment holds and
saves the results with torch.save as {"<case>/<tensor>": CPU tensor}.  The parent imports this module too: `masked_cases`
and `plain_cases` give it the very same tensors for the references, `run_plain` its own default-environment results.
"""
import os
import sys

import torch

import attention_ref as ar
import test_attention_mask_ref as mr

BF = torch.bfloat16
SCALE = 128 ** -0.5
B, H = 2, 2                      # every masked case (test_hip_attention_mask.Run is built for these)


def whole_tile_mask(case, S=320):
    """tests/test_hip_attention_mask.py::_whole_tile_mask (imported lazily: that module needs nothing of the GPU to import)."""
    import test_hip_attention_mask as tm
    return tm._whole_tile_mask(case, S)


def restart_case(decoys_in_the_restarting_items):
    """S = 320, seed 26000.  Tile 0 and tile 3 empty, tile 1 partial in sample 0, tile 2 partial in sample 1.  Two VALID hits
    (a key = gain x its query) lift rows (0, 0, 5) and (1, 1, 260) to lse 225.5 and 155.8 (log2 units): 197.2 and 127.2 above
    the row's first-pass reference (first valid block's maximum + 24), where fp32 ends at 2^128 -- the first row's sum is inf,
    the second row's numerator 2^127.2 is finite but its product with v (up to 2.98) is not.  Either way the first pass's O is
    inf and the two workgroups, items (b, h, rows) = (0, 0, 0..255) and (1, 1, 256..319), repeat the pass after the K-only
    pre-pass (tests/test_hip_attention_orders.py checks these figures on the CPU).  Two MASKED decoys at gain 14 sit on rows
    (0, 1, 7) and (1, 0, 33): with the mask their lse is 7.9 and 13.6, without it 152.0 and 228.3.

    Those two rows belong to items that never restart, so they hold the main loop's mask, not the pre-pass's.  With
    `decoys_in_the_restarting_items` four more masked decoys are placed on rows OF the two restarting items, one per kind of
    tile the pre-pass tells apart: key 200 (empty tile 3) for row (0, 0, 9), key 70 (partial tile 1 of sample 0) for row
    (0, 0, 11), key 140 (partial tile 2 of sample 1) for row (1, 1, 270), key 10 (empty tile 0) for row (1, 1, 300).  A pre-pass
    that took its maximum before the mask would hand such a row a reference ~150 log2 units above every valid score: all its
    numerators flush to 0, l = 0, lse = -inf.  Masked keys add nothing to any sum, so the fp64 reference of every valid quantity
    is the same in both forms."""
    S = 320
    q, k, v, dout = ar.make_inputs(B, H, S, seed=26000)
    mask = torch.ones(B, S, dtype=torch.bool)
    mask[:, :64] = False
    mask[0, 64:96] = False
    mask[1, 130:150] = False
    mask[:, 192:256] = False
    put = lambda b, h, key, gain, row: k[b, h, key].copy_((gain * q[b, h, row].float()).to(BF))   # noqa: E731
    put(0, 0, 300, 12.0, 5)            # valid hits
    put(1, 1, 170, 11.0, 260)
    put(0, 1, 200, 14.0, 7)            # masked decoys
    put(1, 0, 10, 14.0, 33)
    assert mask[0, 300] and mask[1, 170] and not mask[0, 200] and not mask[1, 10]
    if decoys_in_the_restarting_items:
        for b, h, key, row in PREPASS_DECOYS:
            assert not mask[b, key]
            put(b, h, key, 14.0, row)
    return q, k, v, dout, mask


HITS = ((0, 0, 5), (1, 1, 260))
HIT_KEYS = (300, 170)
DECOYS = ((0, 1, 7), (1, 0, 33))
PREPASS_DECOYS = ((0, 0, 200, 9), (0, 0, 70, 11), (1, 1, 140, 270), (1, 1, 10, 300))       # (b, h, masked key, its query row)


def masked_cases():
    """name -> (q, k, v, dout, mask), in the order M1 .. M6 (+ M7: M6 with the decoys the pre-pass itself meets)."""
    cases = {}
    mask = mr.pattern_2d()
    cases["M1 2-D padding S357"] = (*ar.make_inputs(B, H, mask.shape[1], seed=23000, matched=True), mask)
    for i, case in enumerate(("first-empty", "last-empty", "first-block-empty")):
        cases[f"M{2 + i} {case}"] = (*ar.make_inputs(B, H, 320, seed=24000 + len(case)), whole_tile_mask(case))
    mask = torch.zeros(B, 320, dtype=torch.bool)
    mask[:, 130] = True
    cases["M5 single key"] = (*ar.make_inputs(B, H, 320, seed=24500), mask)
    cases["M6 restart, masked decoys"] = restart_case(False)
    cases["M7 restart, decoys in the pre-pass"] = restart_case(True)
    return cases


def plain_cases():
    """name -> (q, k, v [B, H, S, 128], grids): `grids` are the attention_set_split modes to run (1 = the launcher's default,
    0 = plain grid, 7 = a persistent stream-K grid of 7 workgroups)."""
    cases = {"U1 B2 H3 S75": (*ar.make_inputs(2, 3, 75, seed=27075)[:3], (1,))}
    g = torch.Generator().manual_seed(77)                       # tests/test_hip_kernels.py::test_attention_restart_on_late_large_logit, gain 12
    q = torch.randn(1, 2, 640, 128, generator=g).to(BF)
    k = torch.randn(1, 2, 640, 128, generator=g).to(BF)
    qkv = torch.randn(1, 640, 3 * 2 * 128, generator=g).to(BF)
    k[0, 0, 600] = q[0, 0, 5] * 12.0
    k[0, 1, 321] = q[0, 1, 400] * 11.0
    cases["U2 B1 H2 S640 restart"] = (q, k, ar.head_major(qkv[:, :, 2 * 2 * 128:], 2).contiguous(), (1,))
    # 20 items x 18 KV tiles: a 7-workgroup grid cuts items (tests/test_hip_mxfp8_attention.py)
    cases["U3 B1 H4 S1100"] = (*ar.make_inputs(1, 4, 1100, seed=28100)[:3], (0, 7))
    return cases


def run_plain(ops, q, k, v, grid):
    """Unmasked forward with lse under attention_set_split(grid): (o [B, S, H * 128], lse [B, H, S]) on the CPU."""
    Bq, Hq, S, _ = q.shape
    D = Hq * 128
    qkv = torch.zeros(Bq, S, 3 * D, device="cuda", dtype=BF)      # V read in place from the fused projection buffer
    qkv[:, :, 2 * D:] = ar.token_major(v).cuda()
    o = torch.full((Bq, S, D), 5.0, device="cuda", dtype=BF)
    lse = torch.full((Bq, Hq, S), 12345.0, device="cuda", dtype=torch.float32)
    ops.attention_set_split(grid)
    try:
        ops.attention_lse(q.cuda(), k.cuda(), qkv[:, :, 2 * D:], o, lse, scale=SCALE)
        torch.cuda.synchronize()
    finally:
        ops.attention_set_split(1)
    return o.cpu(), lse.cpu()


def main(root, out_path):
    sys.path.insert(0, root)
    from gpt_image_edit_amd import ops
    import test_hip_attention_mask as tm
    outs = {}
    for name, (q, k, v, dout, mask) in masked_cases().items():
        run = tm.Run(ops, q, k, v, dout, mask)          # sentinel-guarded windows; asserts the guards and the packed mask
        for n, t in run.host().items():
            outs[f"{name}/{n}"] = t.contiguous()
        outs[f"{name}/dsum"] = run.dsum.cpu().contiguous()
    for name, (q, k, v, grids) in plain_cases().items():
        for grid in grids:
            o, lse = run_plain(ops, q, k, v, grid)
            outs[f"{name}/grid {grid}/o"], outs[f"{name}/grid {grid}/lse"] = o, lse
    outs["env"] = (os.environ.get("FK_ATTN_KERNEL"), os.environ.get("FK_ATTN_ILV"))
    torch.save(outs, out_path)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
