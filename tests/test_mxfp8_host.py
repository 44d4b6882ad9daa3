"""MXFP8 path, host side (no GPU): the reference quantizer against hand-computed codes and torch's e4m3fn, the ctypes
mirrors of the new fk.h structs, the new kernels' register / scratch budget on hipcc's gfx950 assembly."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mxfp8_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpt_image_edit_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def block(vals, fill=0.0):
    """One [1, 32] row: vals first, then fill."""
    v = list(vals) + [fill] * (32 - len(vals))
    return np.array([v], dtype=np.float64)


def test_e4m3_table():
    v = ref.e4m3_values()
    assert v[0] == 0 and v[1] == 2.0 ** -9 and v[8] == 2.0 ** -6 and v[0x38] == 1.0 and v[126] == 448.0
    assert np.all(np.diff(v) > 0)


def test_round_to_nearest_even_ties():
    # amax 256 -> e = 0 (scale byte 127); 1.0625 lies halfway between 1.0 (code 0x38) and 1.125 (0x39): even 0x38;
    # 1.1875 between 1.125 (0x39) and 1.25 (0x3a): even 0x3a; 1.03125 is below the midpoint: 0x38
    q, s = ref.quantize(block([256.0, 1.0625, 1.1875, 1.03125, -1.0625]))
    assert s[0, 0] == 127
    assert list(q[0, :5]) == [0x78, 0x38, 0x3a, 0x38, 0xb8]


def test_saturation_edge():
    # amax 480: floor(log2) = 8 -> e = 0; 480 > 448 saturates to 448 (0x7e), as do 464 (rounds past 448) and 508;
    # 448 itself and 416 (0x7d) are exact
    q, s = ref.quantize(block([480.0, 464.0, 508.0, 448.0, 416.0, -480.0]))
    assert s[0, 0] == 127
    assert list(q[0, :6]) == [0x7e, 0x7e, 0x7e, 0x7e, 0x7d, 0xfe]
    # the same at another scale: x 2^-20 everywhere -> byte 107, same codes
    q2, s2 = ref.quantize(block([v * 2.0 ** -20 for v in (480.0, 464.0, 508.0, 448.0, 416.0, -480.0)]))
    assert s2[0, 0] == 107 and np.array_equal(q2, q)


def test_scale_exponent_at_powers_of_two():
    # amax = 2^k: e = k - 8 and amax maps to 256 (0x78); just below 2^k (1.9921875 * 2^(k-1)) e = k - 9 and amax saturates
    for k in (-20, -1, 0, 1, 8, 30):
        q, s = ref.quantize(block([2.0 ** k]))
        assert s[0, 0] == k - 8 + 127 and q[0, 0] == 0x78
        q, s = ref.quantize(block([1.9921875 * 2.0 ** (k - 1)]))
        assert s[0, 0] == k - 9 + 127 and q[0, 0] == 0x7e
    # the exponent clamps at -127 (byte 0) for tiny blocks
    q, s = ref.quantize(block([2.0 ** -130]))
    assert s[0, 0] == 0 and q[0, 0] == 0x20      # 2^-130 / 2^-127 = 2^-3: exp field -3 + 7 = 4, code 4 << 3


def test_zero_block():
    q, s = ref.quantize(np.zeros((2, 64)))
    assert np.all(s == 127) and np.all(q == 0)
    q, s = ref.quantize(block([-0.0]))
    assert s[0, 0] == 127 and q[0, 0] == 0x80


def test_subnormal_outputs():
    # amax 256 (e = 0): 2^-7 = 4 * 2^-9 (code 4), 2^-9 (1), 0.75 * 2^-9 -> 1, 2^-10 = 0.5 * 2^-9 -> tie to even 0,
    # 1.5 * 2^-9 -> tie to even 2, 7.5 * 2^-9 -> tie to 8 = the smallest normal (0x08), 2^-11 -> 0
    vals = [256.0, 2.0 ** -7, 2.0 ** -9, 0.75 * 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -9, 7.5 * 2.0 ** -9, 2.0 ** -11, -(2.0 ** -9)]
    q, s = ref.quantize(block(vals))
    assert list(q[0, :9]) == [0x78, 4, 1, 1, 0, 2, 8, 0, 0x81]


def test_inf_nan_blocks():
    x = np.concatenate([block([1.0, np.inf]), block([np.nan]), block([-np.inf, 3.0]), block([2.0])], axis=1)
    q, s = ref.quantize(x)
    assert list(s[0]) == [0xff, 0xff, 0xff, 127 - 7]
    assert np.all(q[0, :96] == 0x7f)
    d = ref.dequantize(q, s)
    assert np.isnan(d[0, :96]).all() and d[0, 96] == 2.0


def test_dequantize_error_bound():
    """Unsaturated elements: |deq - x| <= max(2^-4 |x|, 2^-10 * 2^e) (half an ulp of 3 mantissa bits, or half the smallest
    subnormal step 2^-9 * 2^e); saturated ones (|x| / 2^e > 448) land on 448 * 2^e."""
    g = np.random.default_rng(0)
    x = torch.from_numpy(g.standard_normal((64, 256)) * 10.0 ** g.uniform(-3, 3, (64, 1))).to(torch.bfloat16).double().numpy()
    q, s = ref.quantize(x)
    d = ref.dequantize(q, s)
    scale = np.repeat(ref.e8m0_decode(s), 32, axis=1)
    sat = np.abs(x) / scale > 448.0
    assert np.all(np.abs(d - x)[~sat] <= np.maximum(2.0 ** -4 * np.abs(x), 2.0 ** -10 * scale)[~sat])
    assert np.all(np.abs(d[sat]) == 448.0 * scale[sat])


@pytest.mark.skipif(not hasattr(torch, "float8_e4m3fn"), reason="torch without float8_e4m3fn")
def test_reference_matches_torch_e4m3fn():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(128, 512, generator=g) * torch.logspace(-6, 6, 128).unsqueeze(1)).to(torch.bfloat16)
    x[0, :32] = 0
    x[1, 5] = 3.0e38
    xd = x.double().numpy()
    q, s = ref.quantize(xd)
    e = (s.astype(np.int64) - 127).repeat(32, axis=1)
    v = np.clip(np.ldexp(xd, -e), -448.0, 448.0)
    tq = torch.from_numpy(v).float().to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(q, tq)


def test_struct_layouts_match_header():
    from gpt_image_edit_amd import libfk
    fields = ["g", "A8", "lda8", "A_scale", "lda_scale", "W8", "ldw8", "W_scale", "ldw_scale"]
    code = ('#include <stdio.h>\n#include <stddef.h>\n#include "fk.h"\nint main(){printf("%zu", sizeof(fk_gemm_mxfp8_args));' +
            "".join(f'printf(" %zu", offsetof(fk_gemm_mxfp8_args, {f}));' for f in fields) + 'return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(code)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    M = libfk.GemmMxfp8Args
    assert got == [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields]
    for name in ("fk_quantize_mxfp8", "fk_gemm_mxfp8", "fk_gemm_mxfp8_grouped"):
        assert name in libfk.SIGNATURES


def test_mxfp8_kernels_register_budget(tmp_path):
    """Every kernel of gemm_mxfp8.hip: <= 256 VGPRs (two waves per SIMD), no scratch, no spills; scaled MFMAs present."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path / "mx.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-value", "-Wno-unused-result", "-S",
                    "--cuda-device-only", os.path.join(CSRC, "gemm_mxfp8.hip"), "-o", str(out)], check=True,
                   capture_output=True, timeout=600)
    text = out.read_text()
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                      r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    names = [m[0] for m in meta]
    assert any("quantize_mxfp8_kernel" in n for n in names)
    assert sum("gemm_mxfp8_kernel" in n for n in names) == 10      # 5 epilogues x 2 tile widths
    for name, scratch, vgprs, spills in meta:
        assert int(vgprs) <= 256, f"{name}: {vgprs} VGPRs"
        assert int(scratch) == 0 and int(spills) == 0, f"{name}: {scratch} B scratch, {spills} spills"
    assert "v_mfma_scale_f32_16x16x128_f8f6f4" in text


def test_cli_and_gen_samples_pass_weight_format(monkeypatch):
    from gpt_image_edit_amd.eval import gen_samples
    from gpt_image_edit_amd.serve import cli
    seen = []

    class Stop(Exception):
        pass

    def fake_load_pipe(model_path, flux_path, device, weight_format="bf16"):
        seen.append(weight_format)
        raise Stop

    monkeypatch.setattr(cli, "load_pipe", fake_load_pipe)
    args = cli.build_parser().parse_args(["--model_path", "m", "--flux_path", "f", "--weight_format", "mxfp8"])
    assert args.weight_format == "mxfp8"
    assert cli.build_parser().parse_args(["--model_path", "m", "--flux_path", "f"]).weight_format == "bf16"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--model_path", "m", "--flux_path", "f", "--weight_format", "fp8"])
    with pytest.raises(Stop):
        cli.main(args)
    gargs = gen_samples.build_parser().parse_args(["--model_path", "m", "--flux_path", "f", "--gedit_prompt_path", "p",
                                                   "--output_dir", "o", "--weight_format", "mxfp8"])
    monkeypatch.setattr(gen_samples.dp, "init_from_env", lambda: (0, 0, 1))
    monkeypatch.setattr(gen_samples.torch.cuda, "set_device", lambda d: None)
    with pytest.raises(Stop):
        gen_samples.main(gargs)
    assert seen == ["mxfp8", "mxfp8"]


def test_block_level_mx_structs_match_header():
    from gpt_image_edit_amd import libfk
    names = ["fk_mx_pair", "fk_double_block_weights_mx", "fk_single_block_weights_mx", "fk_mx_ws"]
    code = ('#include <stdio.h>\n#include "fk.h"\nint main(){' + "".join(f'printf("%zu ", sizeof({n}));' for n in names) +
            'return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(code)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(c) for c in (libfk.MxPair, libfk.DoubleBlockWeightsMx, libfk.SingleBlockWeightsMx, libfk.MxWs)]
