"""CPU: the host half of edit_region_weights with ``ops`` stubbed by the numpy restatement -- the order of the stages, the one
read-back, the three raises, the shortcuts (R == 0, need_weight=False), both weight types and the list / PIL inputs."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_weights_ref as R  # noqa: E402

from gpt_image_edit_amd import edit_weights as EW  # noqa: E402


class StubOps:
    """The five wrappers on CPU tensors, each stage the numpy rule; ``calls`` records (name, leading sizes)."""

    def __init__(self, poison=False):
        self.calls, self.poison = [], poison

    def edit_diff_mask(self, ref_u8, tgt_u8, threshold=18, out=None):
        self.calls.append(("edit_diff_mask", tuple(ref_u8.shape), threshold))
        assert ref_u8[0].is_contiguous() and tgt_u8.is_contiguous() and out.is_contiguous()
        assert ref_u8._base is not None or ref_u8.shape[0] == 1              # a view of refs, not a copy of it
        out.copy_(torch.from_numpy(R.diff_mask(ref_u8.numpy(), tgt_u8.numpy(), threshold)))
        return out

    def mask_close5(self, mask, out=None):
        self.calls.append(("mask_close5", tuple(mask.shape)))
        return torch.from_numpy(R.close5(mask.numpy()))

    def mask_components_ws(self, N, H, W, device):
        return torch.zeros(1 + N + 2 * N * H * W, dtype=torch.int32)

    def mask_filter_components(self, mask, keep_num=3, keep_den=10, out=None, ws=None, check=True):
        self.calls.append(("mask_filter_components", tuple(mask.shape), keep_num, keep_den, check))
        assert ws is not None and ws.numel() == 1 + mask.shape[0] + 2 * mask.numel()
        res = torch.from_numpy(R.filter_components(mask.numpy(), keep_num, keep_den))
        return res if out is None else out.copy_(res)

    def mask_and_pool8(self, masks, status=None, out=None):
        self.calls.append(("mask_and_pool8", tuple(masks.shape), status is not None))
        assert masks.is_contiguous()
        mask_ds, counts = R.and_pool8(masks.numpy())
        if self.poison:
            counts[:] = -1
        return torch.from_numpy(mask_ds), torch.from_numpy(counts)

    def mask_weight_fill(self, mask_ds, w, out=None):
        self.calls.append(("mask_weight_fill", tuple(mask_ds.shape)))
        assert w.dtype == torch.float32 and tuple(w.shape) == (mask_ds.shape[0],)
        return R.weight_fill(mask_ds.numpy(), w)


@pytest.fixture
def stub(monkeypatch):
    s = StubOps()
    reads = []
    monkeypatch.setattr(EW, "ops", s)
    real = EW._read_back
    monkeypatch.setattr(EW, "_read_back", lambda c: (reads.append(tuple(c.shape) + (c.dtype,)), real(c))[1])
    s.reads = reads
    return s


def _batch(H=96, W=128, refs_per=1):
    pairs = [R.edit_pair(H, W, seed=s) for s in (1, 2)]
    tgt = np.stack([p[1] for p in pairs])
    refs = np.stack([np.stack([p[0]] * refs_per) for p in pairs])
    return refs, tgt


@pytest.mark.parametrize("kind", ["log", "exp"])
@pytest.mark.parametrize("refs_per", [1, 2])
def test_order_one_read_back_and_the_result(stub, kind, refs_per):
    refs, tgt = _batch(refs_per=refs_per)
    mask_ds, weights = EW.edit_region_weights(torch.from_numpy(refs), torch.from_numpy(tgt), kind, device="cpu")
    want_mask, want_w = R.chain(refs, tgt, kind)
    assert np.array_equal(mask_ds.numpy(), want_mask) and torch.equal(weights, want_w)
    assert weights.dtype == torch.float32 and tuple(weights.shape) == (2, 1, 12, 16) and mask_ds.dtype == torch.uint8
    names = [c[0] for c in stub.calls]
    assert names == ["edit_diff_mask"] * refs_per + ["mask_close5", "mask_filter_components", "mask_and_pool8", "mask_weight_fill"]
    assert all(c == ("edit_diff_mask", (2, 96, 128, 3), 18) for c in stub.calls[:refs_per])
    assert stub.calls[refs_per] == ("mask_close5", (2 * refs_per, 96, 128))
    assert stub.calls[refs_per + 1] == ("mask_filter_components", (2 * refs_per, 96, 128), 3, 10, False)   # no read-back in it
    assert stub.calls[refs_per + 2] == ("mask_and_pool8", (2, refs_per, 96, 128), True)                    # the status rides along
    assert stub.reads == [(2, 2, torch.int32)]                                                            # 8 B bytes, once
    # the scalars are the reference's torch expressions
    for b in range(2):
        t = torch.from_numpy(want_mask[b]).float().bool()
        x = t.numel() / t.sum()
        s = torch.round(torch.log2(x) + 1 if kind == "log" else 2 ** (x ** 0.5 - 1), decimals=6)
        assert float(weights[b].max()) == float(s) > 1.0 and float(weights[b].min()) == 1.0


def test_the_three_raises(stub):
    refs, tgt = _batch()
    small = tgt.copy()
    small[1] = refs[1, 0]
    small[1, 40, 50:53] ^= 0x80                                                   # sample 1: 3 pixels of 12288
    with pytest.raises(ValueError, match=r"TOO SMALL mask_intersect_area_ratio: 0\.000244\d*, sample 1"):
        EW.edit_region_weights(torch.from_numpy(refs), torch.from_numpy(small), device="cpu")
    assert len(stub.reads) == 1 and stub.calls[-1][0] == "mask_and_pool8"          # nothing is filled after a raise
    two = np.concatenate([refs, refs], 1)
    same = tgt.copy()
    same[0] = refs[0, 0]
    with pytest.raises(ValueError, match="sample 0: an empty intersection is reconstruction data"):
        EW.edit_region_weights(torch.from_numpy(two), torch.from_numpy(same), device="cpu")
    before = len(stub.calls)
    with pytest.raises(NotImplementedError, match=r"Support log \| exp, but found lin"):
        EW.edit_region_weights(torch.from_numpy(refs), torch.from_numpy(tgt), "lin", device="cpu")
    assert len(stub.calls) == before                                               # refused before any stage
    # one reference and identical pictures: reconstruction data, no raise, weights 1
    mask_ds, weights = EW.edit_region_weights(torch.from_numpy(refs), torch.from_numpy(same), device="cpu")
    assert int(mask_ds[0].min()) == 255 and torch.equal(weights[0], torch.ones(1, 12, 16)) and float(weights[1].max()) > 1


def test_a_labelling_bound_is_an_error(monkeypatch):
    monkeypatch.setattr(EW, "ops", StubOps(poison=True))
    refs, tgt = _batch()
    with pytest.raises(RuntimeError, match="FK_EBOUND"):
        EW.edit_region_weights(torch.from_numpy(refs), torch.from_numpy(tgt), device="cpu")


@pytest.mark.parametrize("kind", ["log", "exp"])
def test_no_reference_and_need_weight_false(stub, kind):
    refs, tgt = _batch(H=100, W=76)
    for r, kw in ((torch.from_numpy(refs[:, :0]), {}), (torch.from_numpy(refs), dict(need_weight=False))):
        mask_ds, weights = EW.edit_region_weights(r, torch.from_numpy(tgt), kind, device="cpu", **kw)
        assert tuple(mask_ds.shape) == (2, 12, 9) and int(mask_ds.min()) == 255 and mask_ds.dtype == torch.uint8
        assert torch.equal(weights, torch.ones(2, 1, 12, 9)) and weights.dtype == torch.float32
    assert stub.calls == [] and stub.reads == []


def test_lists_of_pil_and_numpy_pictures(stub):
    refs, tgt = _batch(refs_per=2)
    want = EW.edit_region_weights(torch.from_numpy(refs), torch.from_numpy(tgt), device="cpu")
    as_pil = EW.edit_region_weights([[Image.fromarray(p) for p in s] for s in refs], [Image.fromarray(t) for t in tgt], device="cpu")
    as_np = EW.edit_region_weights([list(s) for s in refs], list(tgt), device="cpu")
    for got in (as_pil, as_np):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    none = EW.edit_region_weights([[], []], list(tgt), device="cpu")                # text-to-image: R == 0
    assert int(none[0].min()) == 255 and torch.equal(none[1], torch.ones(2, 1, 12, 16))
    for bad_refs, bad_tgt in (([[refs[0, 0]], []], list(tgt)),                       # unequal numbers of references
                              ([[refs[0, 0][:90]], [refs[1, 0]]], list(tgt)),       # unequal sizes
                              ([[refs[0, 0]]], list(tgt)),                          # one list shorter than the other
                              ([[refs[0, 0].astype(np.float32)], [refs[1, 0]]], list(tgt)),
                              ([[refs[0, 0][..., 0]], [refs[1, 0][..., 0]]], list(tgt)),
                              ("refs", list(tgt))):
        with pytest.raises(ValueError):
            EW.edit_region_weights(bad_refs, bad_tgt, device="cpu")
    for bad in (torch.from_numpy(refs).float(), torch.from_numpy(refs)[:, :, :90], torch.from_numpy(refs)[0]):
        with pytest.raises(ValueError):
            EW.edit_region_weights(bad, torch.from_numpy(tgt), device="cpu")
    with pytest.raises(ValueError, match="sides are 8..4096"):
        EW.edit_region_weights(torch.zeros(1, 1, 7, 8, 3, dtype=torch.uint8), torch.zeros(1, 7, 8, 3, dtype=torch.uint8), device="cpu")
