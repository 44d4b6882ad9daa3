"""The reference helpers of tests/gemm_small_ref.py (CPU): each epilogue helper is the obvious torch bf16 graph on exact
inputs, and the comparison functions the GPU tests call reject four deliberate mistakes of the kind a tiled kernel makes."""
import pytest
import torch
import torch.nn.functional as F

import gemm_small_ref as R
from gemm_small_ref import BF, F32, F64

B, ROWS, N, K = 2, 70, 136, 192        # M = 140: a batch ends inside the first 128-row tile
M = B * ROWS


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(7)
    a, w, bias = R.ints((B, ROWS, K), -2, 2, 1), R.ints((N, K), -2, 2, 2), R.ints((N,), -4, 4, 3)
    res = R.ints((B, ROWS, N), -64, 64, 4)
    gate = (torch.randn(B, 3 * N, generator=g) * 0.7).to(BF)[:, N:2 * N]
    return dict(a=a, w=w, bias=bias, res=res, gate=gate, y=R.expected(a, w, bias), acc32=a.reshape(M, K).float() @ w.float().T)


def test_ints_and_expected(data):
    v = R.ints((1000,), -2, 2, 5)
    assert v.dtype == BF and set(v.float().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert torch.equal(v, R.ints((1000,), -2, 2, 5))
    assert data["y"].dtype == F64 and data["y"].shape == (M, N)
    assert torch.equal(data["y"], (data["acc32"] + data["bias"].float()).double())     # the fp32 matmul is exact on these data
    with pytest.raises(AssertionError):                    # sums beyond 2^24
        R.expected(torch.full((1, 64), 2.0 ** 12), torch.full((8, 64), 2.0 ** 12))
    with pytest.raises(AssertionError):                    # a value that is the sentinel
        R.expected(torch.full((1, 64), 1.0), torch.full((8, 64), R.SENTINEL / 64))
    with pytest.raises(AssertionError):                    # not representable in fp32
        R.expected(torch.full((1, 64), 1.0, dtype=F64), torch.full((8, 64), 1.0 + 2.0 ** -40, dtype=F64))


def test_none_scale_res_are_the_torch_graphs(data):
    lin = (data["acc32"] + data["bias"].float()).to(BF)
    assert torch.equal(R.epi_none(data["y"]), lin)
    y0 = R.expected(data["a"], data["w"])
    for alpha in (0.125, 512 ** -0.5):
        assert torch.equal(R.epi_scale(y0, alpha), (data["acc32"] * torch.tensor(alpha, dtype=F32)).to(BF))
    assert not torch.equal(R.epi_scale(y0, 512 ** -0.5), R.epi_scale(y0, 0.0625))
    assert torch.equal(R.epi_res(data["y"], data["res"]), lin + data["res"].reshape(M, N))      # one bf16 add


def test_gate_res_is_the_torch_graph(data):
    lin = (data["acc32"] + data["bias"].float()).to(BF).view(B, ROWS, N)
    want = data["res"] + data["gate"][:, None] * lin                                             # evaluated in bf16
    assert torch.equal(R.epi_gate_res(data["y"], data["res"], data["gate"], ROWS), want.reshape(M, N))
    one = R.epi_gate_res(data["y"][:ROWS], data["res"][:1], data["gate"][:1], ROWS)               # B = 1
    assert torch.equal(one, want[0])


@pytest.mark.parametrize("name", ["gelu", "silu"])
def test_activations_are_the_torch_graphs_within_a_step(data, name):
    y = R.expected(data["a"], data["w"] * 2.0 ** -5, data["bias"])
    assert y.abs().max().item() <= 8
    x = R.bf16_of(y)
    got = (R.epi_gelu if name == "gelu" else R.epi_silu)(y)
    ref32 = (F.gelu(x.float(), approximate="tanh") if name == "gelu" else F.silu(x.float())).to(BF)
    # torch's GELU forms 1 + tanh(u), which cancels for negative x: its fp32 graph is good to a bf16 step only above -3 or
    # so, its fp64 graph to 1e-9 above -4 (and is -0 below -7).  The helper's form (x * sigmoid(2 u)) has no such range.
    near = x.float() >= -3 if name == "gelu" else torch.ones_like(x, dtype=torch.bool)
    assert near.float().mean() > 0.8 and (~near).any() == (name == "gelu")
    d = R.bf16_ulp_diff(got, ref32)[near]
    assert int(d.max()) <= 1 and float((d == 0).float().mean()) > 0.99        # fp32 against fp64 evaluation: boundaries only
    torch_ref = F.gelu(x.double(), approximate="tanh") if name == "gelu" else F.silu(x.double())
    ref64 = R.gelu_tanh64(x.double()) if name == "gelu" else x.double() / (1 + torch.exp(-x.double()))
    mid = x.double() >= -4
    assert ((ref64 - torch_ref).abs()[mid] <= 1e-9 * torch_ref.abs()[mid]).all()
    if name == "gelu":
        deep = torch.tensor([-8.0], dtype=F64)
        assert F.gelu(deep, approximate="tanh").item() == 0.0 and -4e-21 < R.gelu_tanh64(deep).item() < -3e-21
    # rounded ONCE: the result is the bf16 value nearest the fp64 one
    err = (got.double() - ref64).abs()
    for step in (-1, 1):
        bits = got.view(torch.int16).to(torch.int32)
        mono = torch.where(bits < 0, -(bits & 0x7FFF), bits) + step
        raw = torch.where(mono < 0, (-mono) | 0x8000, mono)
        nb = torch.where(raw >= 0x8000, raw - 0x10000, raw).to(torch.int16).view(BF)
        assert (err <= (nb.double() - ref64).abs()).all()


def test_round_once_differs_from_the_double_rounding_where_it_must():
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -30, 1.0 + 2.0 ** -8 - 2.0 ** -30, -(1.0 + 2.0 ** -8 + 2.0 ** -30), 3.0], dtype=F64)
    # through fp32 the first lands on the tie 1 + 2^-8 and goes to even (1.0); rounded once it is above the tie
    assert x.to(F32).to(BF).tolist() == [1.0, 1.0, -1.0, 3.0]
    assert R.round_once_bf16(x).tolist() == [1.0 + 2.0 ** -7, 1.0, -(1.0 + 2.0 ** -7), 3.0]


def test_fp32_forms(data):
    y0 = R.expected(data["a"], data["w"])
    bias32 = torch.arange(N, dtype=F32) / 8 - 5
    res32 = R.ints((M, N), -64, 64, 9).float() / 4
    assert torch.equal(R.f32_none(y0, data["bias"]), data["acc32"] + data["bias"].float())
    assert torch.equal(R.f32_none(y0, bias32, res32), data["acc32"] + bias32 + res32)
    assert torch.equal(R.f32_scale(y0, 512 ** -0.5), data["acc32"] * torch.tensor(512 ** -0.5, dtype=F32))
    with pytest.raises(AssertionError):                    # a bias the fp32 add would round
        R.f32_none(y0 + 2.0 ** 20, torch.full((N,), 2.0 ** -10))


def test_guarded_views():
    for rows, n, dtype in [(5, 8, BF), ((2, 5), 136, BF), (5, 77, F32), (5, 1, F32)]:
        buf, idx, c = R.guarded(rows, n, dtype)
        assert c.shape[-1] == n and c.stride(-1) == 1 and c.stride(-2) != n
        assert (c.data_ptr() - buf.data_ptr()) % 16 == 0 and c.data_ptr() % 16 == buf.data_ptr() % 16
        assert (buf == R.SENTINEL).all()


# ---- the comparison functions see the mistakes a tiled kernel makes --------------------------------------------------------

MISTAKES = R.MISTAKES


def _in_buffer(out):
    buf, idx, c = R.guarded(M, N, out.dtype)
    c.copy_(out)
    return buf, idx


@pytest.mark.parametrize("mistake", MISTAKES, ids=lambda f: f.__name__.strip("_"))
def test_equality_check_sees_each_mistake(data, mistake):
    finish = lambda y: R.epi_gate_res(y, data["res"], data["gate"], ROWS)      # noqa: E731
    want = finish(data["y"])
    buf, idx = _in_buffer(want)
    R.check_guarded(buf, idx, want, "correct")
    buf, idx = _in_buffer(mistake(data, finish))
    with pytest.raises(AssertionError, match="differ"):
        R.check_guarded(buf, idx, want, mistake.__name__)


@pytest.mark.parametrize("mistake", MISTAKES[:3], ids=lambda f: f.__name__.strip("_"))
def test_fp32_equality_check_sees_each_mistake(data, mistake):
    finish = lambda y: R.f32_none(y)      # noqa: E731
    want = finish(data["y"])
    buf, idx = _in_buffer(want)
    R.check_guarded(buf, idx, want, "correct")
    buf, idx = _in_buffer(mistake(data, finish))
    with pytest.raises(AssertionError, match="differ"):
        R.check_guarded(buf, idx, want, mistake.__name__)


@pytest.mark.parametrize("name", ["gelu", "silu"])
@pytest.mark.parametrize("mistake", MISTAKES[:3], ids=lambda f: f.__name__.strip("_"))
def test_ulp_check_sees_each_mistake(data, mistake, name):
    d = dict(data, w=data["w"] * 2.0 ** -5)
    d["y"] = R.expected(d["a"], d["w"], d["bias"])
    finish = R.epi_gelu if name == "gelu" else R.epi_silu
    want = finish(d["y"])
    buf, idx = _in_buffer(want)
    assert R.check_ulp(buf, idx, want, "correct") == (1.0, 0)
    buf, idx = _in_buffer(mistake(d, finish))
    with pytest.raises(AssertionError, match="ulp"):
        R.check_ulp(buf, idx, want, mistake.__name__)


def test_checks_see_a_written_guard_band_and_an_unwritten_element(data):
    want = R.epi_none(data["y"])
    buf, idx = _in_buffer(want)
    buf[R.GUARD_ROWS + M, R.GUARD_COLS] = 0.0                # the row after C
    with pytest.raises(AssertionError, match="guard band"):
        R.check_guarded(buf, idx, want, "row after")
    with pytest.raises(AssertionError, match="guard band"):
        R.check_ulp(buf, idx, want, "row after")
    buf, idx = _in_buffer(want)
    buf[idx][M - 1, N - 1] = R.SENTINEL                      # an element no workgroup stored
    with pytest.raises(AssertionError, match="differ"):
        R.check_guarded(buf, idx, want, "unwritten")
