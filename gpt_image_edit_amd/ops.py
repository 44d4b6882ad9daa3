"""Tensor-level wrappers over the C ABI (include/fk.h): tensors in, tensors out.

Only plumbing lives here: argument checking, stride extraction, raw pointers and the current HIP
stream.  All arithmetic happens in libfk.so; nothing falls back to torch ops.
"""
import ctypes
import threading
from types import SimpleNamespace
import os

import torch

from . import helpers, libfk, param_tree
from .libfk import (FK_EPI_GATE_RES, FK_EPI_GELU_TANH, FK_EPI_NONE, FK_EPI_QKV, FK_EPI_RES, FK_EPI_SCALE,  # noqa: F401
                    FK_EPI_SILU, GemmArgs, GemmMxfp8Args, GemmMxfp8QArgs, Rows)

BF16 = torch.bfloat16


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("gpt_image_edit_amd ops need GPU tensors: the HIP path has no CPU fallback")


def pack_rope(cos, sin, check=True):
    """FluxPosEmbed's cos / sin [S, 128] (each value repeated over the two columns of its rotary pair) -> the
    [S, 64, 2] (cos, sin)-per-pair table the fused QKV epilogue reads.  Step-invariant: callers on the hot path
    pack once (transformer._rope) and pass ``cs``; passing cos / sin packs per call and checks the repetition."""
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != 128:
        raise ValueError("cos / sin must be [S, 128]")
    # check=False: tables that come straight from transformer.rope_tables (torch.equal on device tensors is a host sync)
    if check and not (torch.equal(cos[:, 0::2], cos[:, 1::2]) and torch.equal(sin[:, 0::2], sin[:, 1::2])):
        raise ValueError("cos / sin do not repeat over the columns of a rotary pair: not FluxPosEmbed tables")
    return torch.stack([cos[:, 0::2], sin[:, 0::2]], dim=-1).to(torch.float32).contiguous()


def rows_of(t):
    """(M, Rows) for a [M, K] or [B, R, K] tensor (or view) whose last dimension is contiguous."""
    if t.stride(-1) != 1:
        raise ValueError("last dimension must be contiguous")
    if t.dim() == 2:
        return t.shape[0], Rows(t.stride(0), 0, 0)
    if t.dim() == 3:
        b, r, _ = t.shape
        return b * r, Rows(t.stride(1), r, t.stride(0))
    raise ValueError(f"expected a 2-D or 3-D tensor, got {t.dim()}-D")


# Split-K workspace (fk.h: fk_gemm_args.splitk_ws): one per (device, stream) -- launches that share one must be ordered.
# 128 slots cover every grid the planner splits (two half-K workgroups per tile on at most all 256 CUs); 32 MiB each.
SPLITK_SLOTS = 256      # one per cut of a stream-K launch (= CUs) / per tile of a split-K pair launch
_SPLITK_WS = {}


def splitk_workspace(device):
    """(uint8 buffer, slots) for the current stream of ``device``; control words zeroed once (monotonic tickets after)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        ws = torch.zeros(SPLITK_SLOTS * libfk.FK_SPLITK_SLOT_BYTES, device=device, dtype=torch.uint8)
        _SPLITK_WS[key] = ws
    return ws, SPLITK_SLOTS


_VARIANT_USED = threading.local()


def _variant_slot():
    """This thread's int32 that every GEMM call of this module hands to the library as fk_gemm_args.variant_used (OUT)."""
    slot = getattr(_VARIANT_USED, "slot", None)
    if slot is None:
        slot = _VARIANT_USED.slot = ctypes.c_int32(0)
    return slot


def gemm_last_variant():
    """Launch form of this thread's last ``gemm`` / ``gemm_grouped`` / block-level call: 128 = 256 x 128 tiles, 256 = 256 x 256,
    384 = mixed grid, 512 = split-K pairs, 640 = stream-K ranges, 0 = the 128 x 128 kernel (tests, profiling).  The value is
    the call's own OUT field (fk_gemm_args.variant_used): the library keeps no record."""
    return int(_variant_slot().value)


def _check_splitk_ws(splitk_ws):
    """(buffer, slots) of a caller-owned split-K workspace: a contiguous uint8 tensor of at least ``slots`` x
    FK_SPLITK_SLOT_BYTES bytes, 16-byte aligned.  The caller zeroes it once and keeps ``slots`` fixed for its lifetime (the
    control words lie behind ``slots`` partial tiles and are never reset)."""
    ws, slots = splitk_ws
    _need_cuda(ws)
    if (ws.dtype != torch.uint8 or not ws.is_contiguous() or int(slots) < 1 or ws.numel() < int(slots) * libfk.FK_SPLITK_SLOT_BYTES
            or ws.data_ptr() % 16 != 0):
        raise ValueError("splitk_ws: (contiguous 16-byte aligned uint8 tensor of >= slots * FK_SPLITK_SLOT_BYTES bytes, slots >= 1)")
    return ws, int(slots)


def _gemm_args(a, w, bias, out, epilogue, res, gate, out_fp32, alpha, qkv=None, layout=0, splitk_ws=None):
    _need_cuda(a, w, bias, out, res, gate)
    if a.dtype != BF16 or w.dtype != BF16:
        raise TypeError("fk_gemm_bf16 takes bf16 operands")
    if layout == 0:
        M, ra = rows_of(a)
        N, K = w.shape
        if a.shape[-1] != K:
            raise ValueError(f"K mismatch: a {tuple(a.shape)} vs w {tuple(w.shape)}")
        out_shape = (*a.shape[:-1], N)
    elif layout == 1:     # w is [K, N]: out = a @ w
        M, ra = rows_of(a)
        K, N = w.shape
        if a.shape[-1] != K or w.stride(1) != 1:
            raise ValueError(f"layout 1: a {tuple(a.shape)} @ w {tuple(w.shape)} (w rows contiguous)")
        out_shape = (*a.shape[:-1], N)
    elif layout == 2:     # a is [K, M] (or [B, R, M] rows = K), w is [K, N]: out = a^T @ w
        a = a[0] if a.dim() == 3 and a.shape[0] == 1 else a      # one batch: any batch stride
        w = w[0] if w.dim() == 3 and w.shape[0] == 1 else w
        K, ra = rows_of(a)
        M, N = a.shape[-1], w.shape[-1]
        Kw, rw = rows_of(w)
        if Kw != K or w.stride(-1) != 1 or (rw.rows_per_batch > 0 and rw.batch_stride != rw.rows_per_batch * rw.ld):
            raise ValueError(f"layout 2: a {tuple(a.shape)} ^T @ w {tuple(w.shape)} (uniformly strided w rows)")
        out_shape = (M, N)
    else:
        raise ValueError(f"layout {layout}")
    if out is None:
        out = torch.empty(out_shape, device=a.device, dtype=torch.float32 if out_fp32 else BF16)
    Mo, rc = rows_of(out)
    if Mo != M or out.shape[-1] != N:
        raise ValueError(f"output shape {tuple(out.shape)} does not match M={M}, N={N}")
    args = GemmArgs()
    args.layout = layout
    args.A, args.a = a.data_ptr(), ra
    args.W, args.ldw = w.data_ptr(), (w.stride(0) if layout != 2 else rw.ld)
    args.bias = bias.data_ptr() if bias is not None else None
    args.C, args.c = out.data_ptr(), rc
    if res is not None:
        Mr, rr = rows_of(res)
        if Mr != M:
            raise ValueError("residual rows mismatch")
        args.res, args.r = res.data_ptr(), rr
    if gate is not None:
        if a.dim() != 3 or gate.dim() != 2 or gate.shape[0] != a.shape[0] or gate.stride(1) != 1:
            raise ValueError("gate must be a [B, N] view matching a 3-D activation")
        args.gate = gate.data_ptr()
        args.gate_batch_stride = gate.stride(0)
        args.gate_rows_per_batch = a.shape[1]
    args.M, args.N, args.K = M, N, K
    _apply_gemm_launch(args)
    args.variant_used = ctypes.pointer(_variant_slot())
    args.epilogue, args.out_fp32, args.alpha = epilogue, int(out_fp32), float(alpha)
    if int(out_fp32) == 1:       # fp32-class VAE encoder: fp32 bias / fp32 residual added to the fp32 output
        args.f32_flags = ((1 if bias is not None and bias.dtype == torch.float32 else 0) |
                          (2 if res is not None and res.dtype == torch.float32 and epilogue == FK_EPI_NONE else 0))
    if splitk_ws is not None:    # the caller's own workspace instead of the stream's (any K: forced pairs / ranges below 6144)
        ws, slots = _check_splitk_ws(splitk_ws)
        args.splitk_ws, args.splitk_slots = ws.data_ptr(), slots
    elif K >= 6144 and N % 256 == 0 and M <= 256 * SPLITK_SLOTS and int(out_fp32) != 1 and layout == 0:   # the only shapes the planner may split
        ws, slots = splitk_workspace(a.device)
        args.splitk_ws, args.splitk_slots = ws.data_ptr(), slots
    if epilogue == FK_EPI_QKV:
        _set_qkv(args, qkv)
    return args, out


def _set_qkv(args, qkv):
    """The FK_EPI_QKV fields of a GemmArgs from gemm()'s ``qkv`` dict."""
    cs = qkv["cs"] if "cs" in qkv else pack_rope(qkv["cos"], qkv["sin"])
    _need_cuda(qkv["q_out"], qkv["k_out"], qkv["wq"], qkv["wk"], cs)
    if cs.dtype != torch.float32 or not cs.is_contiguous() or tuple(cs.shape) != (qkv["q_out"].shape[2], 64, 2):
        raise ValueError("cs must be a contiguous fp32 [S_total, 64, 2] table (see pack_rope)")
    args.q_out, args.k_out = qkv["q_out"].data_ptr(), qkv["k_out"].data_ptr()
    args.wq, args.wk = qkv["wq"].data_ptr(), qkv["wk"].data_ptr()
    args.rope_cs = cs.data_ptr()
    args.qkv_s_offset, args.qkv_s_total, args.qkv_heads = qkv["s_offset"], qkv["q_out"].shape[2], qkv["q_out"].shape[1]


def gemm(a, w, bias=None, out=None, epilogue=FK_EPI_NONE, res=None, gate=None, out_fp32=False, alpha=1.0, qkv=None, layout=0,
         splitk_ws=None):
    """out = epilogue(a @ w.T + bias).  a: [M,K] / [B,R,K] view; w: [N,K]; out likewise (may alias res).

    out_fp32: True / 1 = fp32(acc + bias) by the 128 x 128 register-staged kernel; 2 = the same from the LARGE-TILE kernels'
    own main loops (256 x 256 / 256 x 128 / mixed / split-K, whichever the launch plan or ``gemm_set_variant`` selects) --
    the parity build that holds the kernels carrying the FLOPs to rtol 1e-3 / atol 1e-4.

    layout (fk_gemm_args.layout): 1 = ``w`` is [K, N] and out = a @ w (the data gradient reads the weight as stored);
    2 = ``a`` is [K, M] / [B, R, M] and ``w`` [K, N] / [B, R, N], out [M, N] = a^T @ w (the weight gradient reads both
    operands token-major).  N % 256 == 0 (2: M % 256 == 0), K % 64 == 0, no epilogue (1: FK_EPI_RES allowed).

    gate: [B, N] view (row stride = batch stride); used with FK_EPI_GATE_RES and a 3-D ``a``.
    qkv (FK_EPI_QKV): dict(q_out, k_out [B,H,S_total,128], wq, wk [128], cs fp32 [S_total,64,2] (pack_rope; or cos, sin
    fp32 [S_total,128], packed per call), s_offset)
    -- the fused QKV projection: q / k thirds get RMSNorm + RoPE + head-major layout, the v third lands in out.
    splitk_ws: ``(uint8 tensor, slots)`` -- a split-K workspace of the caller's own (zeroed once, >= slots x
    FK_SPLITK_SLOT_BYTES bytes, ``slots`` fixed for its lifetime) instead of this stream's; None = the stream's at K >= 6144.
    """
    args, out = _gemm_args(a, w, bias, out, epilogue, res, gate, out_fp32, alpha, qkv, layout, splitk_ws)
    libfk.check(libfk.load().fk_gemm_bf16(ctypes.byref(args), _stream()), "fk_gemm_bf16")
    return out


# ---- launch controls --------------------------------------------------------------------------------------------------------
# The C library keeps NO mutable launch state (round 5): every call carries its launch form (fk_gemm_args.variant / plan /
# group_m / mfma, the `grid` / `passes` arguments of the attention entry points, fk_block_ws.gemm_* / attn_grid).  What the
# HOST wants as its defaults lives here, in the application layer: the setters below change this module's defaults (and only
# this process's Python callers see them); the environment variables FK_GEMM_PLAN, FK_GEMM_BN, FK_GEMM_GROUP_M, FK_GEMM_MFMA,
# FK_ATTN_SPLIT, FK_ATTN_BWD of rounds 2-4 are read once, here.
FK_GEMM_PLAN_EXPLICIT = 8
FK_GEMM_PLAN_SPLITK = {"default": 0, "whole": 16, "symmetric": 32, "unannounced": 64}   # include/fk.h: FK_GEMM_PLAN_SPLITK_*
FK_GEMM_PLAN_WALK = {"default": 0, "tile_per_wg": 128, "walk": 256}                       # include/fk.h: FK_GEMM_PLAN_TILE_PER_WG / _WALK
FK_GEMM_PLAN_WALK_CAP_SHIFT = 16


def _env_int(name, default):
    v = os.environ.get(name)
    return default if v is None or v == "" else int(v)


LAUNCH = SimpleNamespace(
    gemm_variant=_env_int("FK_GEMM_BN", 0),         # 0 = launch plan; 128 / 256 / 384 / 512 / 640 force a form where it applies
    gemm_plan=(FK_GEMM_PLAN_EXPLICIT | (_env_int("FK_GEMM_PLAN", 3) & 7)) if os.environ.get("FK_GEMM_PLAN") else 0,
    gemm_splitk=0,                                  # exchange of the split-K pairs: 0 = built default, or a FK_GEMM_PLAN_SPLITK bit
    # tile walk of the 256 x 256 / mixed grids (plan bits): FK_GEMM_WALK=0 never, 1 wherever tiles > CUs, unset = the built rule
    gemm_walk={"0": 128, "1": 256}.get(os.environ.get("FK_GEMM_WALK", ""), 0),
    gemm_group_m=_env_int("FK_GEMM_GROUP_M", 0),
    gemm_mfma=_env_int("FK_GEMM_MFMA", 0),          # 0 = built default (16); 16 / 32
    attn_grid={0: -1, 1: 0}.get(_env_int("FK_ATTN_SPLIT", 1), _env_int("FK_ATTN_SPLIT", 1)),   # 0 default, -1 plain grid, >= 2 forced
    attn_bwd_passes=0 if _env_int("FK_ATTN_BWD", 1) else 3)
_LAUNCH_CFG_EPOCH = [0]


def launch_config_epoch():
    """Bumped by every launch-control setter of this module: anything that froze host-side launch decisions (a captured
    hipGraph of the denoise loop) keys on it."""
    return _LAUNCH_CFG_EPOCH[0]


def _set_launch(**kw):
    for k, v in kw.items():
        setattr(LAUNCH, k, v)
    _LAUNCH_CFG_EPOCH[0] += 1


def gemm_set_variant(variant):
    """Force the launch form of the large-tile GEMMs where it applies: 128 = 256 x 128 tiles, 256 = 256 x 256 tiles, 384 =
    mixed grid, 512 = split-K pairs, 640 = stream-K ranges, 1024 = the 4-wave hand-placed 256 x 256 kernel (gemm10_kernel);
    0 = the launch plan chooses per problem.  (fk_gemm_args.variant)"""
    if int(variant) not in (0, 128, 256, 384, 512, 640, 1024):
        raise ValueError(f"gemm_set_variant: {variant} is not one of 0, 128, 256, 384, 512, 640, 1024")
    _set_launch(gemm_variant=int(variant))


def gemm_set_plan(allow):
    """Which launch forms the plan may use (fk_gemm_args.plan): bit 0 = mixed grids (bit-identical results), bit 1 = split-K
    pairs (last-bit differences against the unsplit sum, so a sample's result then depends on how full the grid is), bit 2 =
    stream-K ranges.  ``gemm_set_plan(1)`` = batch-invariant; ``gemm_set_plan(3)`` = the default."""
    if not 0 <= int(allow) <= 7:
        raise ValueError(f"gemm_set_plan: {allow} is not in 0..7")
    _set_launch(gemm_plan=FK_GEMM_PLAN_EXPLICIT | int(allow))


def gemm_set_splitk_exchange(mode):
    """How the two workgroups of a split-K pair exchange their partial tiles (fk_gemm_args.plan, FK_GEMM_PLAN_SPLITK_*):
    "whole" = the first to finish hands its whole tile over, "symmetric" = each finishes 128 rows of it, "unannounced" = the
    symmetric form's fallback taken always (tests), "default" = what the library was built with.  Same bits every way."""
    _set_launch(gemm_splitk=FK_GEMM_PLAN_SPLITK[mode])


def gemm_set_walk(form="default", cap=0):
    """Tile walk of the large-tile GEMMs (fk_gemm_args.plan): a 256 x 256 or mixed grid with more tiles than workgroups runs as
    one workgroup per CU, each walking its tiles with the next tile's first operands requested in front of the epilogue.
    "default" = the library's built rule, "tile_per_wg" = never (one workgroup per tile), "walk" = wherever it applies;
    ``cap`` > 0 (implies "walk"): at most that many workgroups (tests).  Same bits every way."""
    if not 0 <= int(cap) <= 0x7fff or (cap and form == "tile_per_wg"):
        raise ValueError(f"gemm_set_walk: cap {cap} is not in 0..32767, or given with 'tile_per_wg'")
    _set_launch(gemm_walk=FK_GEMM_PLAN_WALK[form] | (int(cap) << FK_GEMM_PLAN_WALK_CAP_SHIFT))


def launch_plan():
    """fk_gemm_args.plan / fk_block_ws.gemm_plan of this module's launch defaults."""
    extra = LAUNCH.gemm_splitk | LAUNCH.gemm_walk
    if not extra:
        return LAUNCH.gemm_plan
    return (LAUNCH.gemm_plan or (FK_GEMM_PLAN_EXPLICIT | 3)) | extra


def gemm_set_group_m(depth):
    """Depth (in 256-row tiles) of the grouped tile order (fk_gemm_args.group_m; results do not depend on it); 0 = default."""
    if not 0 <= int(depth) <= 4096:
        raise ValueError(f"gemm_set_group_m: {depth} is not 0 (default) or 1..4096 row tiles")
    _set_launch(gemm_group_m=int(depth))


def gemm_set_mfma(shape):
    """MFMA shape of the layout-0 large-tile GEMM kernels (fk_gemm_args.mfma): 32 (v_mfma_f32_32x32x16_bf16), 16
    (v_mfma_f32_16x16x32_bf16) or 0 = the built default (16).  The two differ in the last bits; see include/fk.h."""
    if int(shape) not in (0, 16, 32):
        raise ValueError(f"gemm_set_mfma: {shape} is not 0, 16 or 32")
    _set_launch(gemm_mfma=int(shape))


def _apply_gemm_launch(args):
    args.variant, args.plan, args.group_m, args.mfma = LAUNCH.gemm_variant, launch_plan(), LAUNCH.gemm_group_m, LAUNCH.gemm_mfma


def gemm_grouped(problems, epilogue=FK_EPI_NONE, splitk_ws=None):
    """Several independent GEMMs sharing (N, K, epilogue) in ONE launch.  ``problems`` is a list of dicts
    with the keyword arguments of :func:`gemm` (a, w, bias, out, res, gate); returns the outputs.  splitk_ws: as :func:`gemm`."""
    n = len(problems)
    arr = (GemmArgs * n)()
    outs = []
    for i, pr in enumerate(problems):
        args, out = _gemm_args(pr["a"], pr["w"], pr.get("bias"), pr.get("out"), epilogue, pr.get("res"),
                               pr.get("gate"), False, 1.0, pr.get("qkv"), pr.get("layout", 0), splitk_ws)
        arr[i] = args
        outs.append(out)
    libfk.check(libfk.load().fk_gemm_bf16_grouped(arr, n, _stream()), "fk_gemm_bf16_grouped")
    return outs


# ---- MXFP8 (opt-in inference format of the block GEMMs; include/fk.h) --------------------------------------------------------
MXFP8_BLOCK = 32
# launches of the standalone quantizer since import: those of quantize_mxfp8() below, and those the block-level C entry points
# enqueue (they count into the int32 that fk_mx_ws.quantize_launches names).  Tests read the difference around a forward: the
# fused schedule leaves 2 per double block and 1 per single block.
QUANTIZE_LAUNCHES = [0]
_QUANTIZE_SLOT = ctypes.c_int32(0)


def quantize_launch_count():
    return QUANTIZE_LAUNCHES[0] + int(_QUANTIZE_SLOT.value)


def quantize_mxfp8(x, q=None, scales=None):
    """OCP MXFP8 of a bf16 [M, K] / [B, R, K] view (last dimension contiguous, K % 32 == 0): returns (q, scales), q uint8
    [M, K] holding e4m3fn codes of x / 2^e (round-to-nearest-even, saturated to +-448) and scales uint8 [M, K / 32] holding
    the E8M0 byte e + 127 of every block of 32 consecutive elements, e = max(floor(log2(amax)) - 8, -127).  An all-zero block
    has scale byte 127; a block holding Inf / NaN has scale 0xFF and elements 0x7F (NaN).  Weights [N, K] go through the
    same call once at pack time."""
    _need_cuda(x, q, scales)
    if x.dtype != BF16:
        raise TypeError("quantize_mxfp8 takes a bf16 tensor")
    M, rx = rows_of(x)
    K = x.shape[-1]
    if q is None:
        q = torch.empty((M, K), device=x.device, dtype=torch.uint8)
    if scales is None:
        scales = torch.empty((M, K // MXFP8_BLOCK), device=x.device, dtype=torch.uint8)
    if (q.dtype != torch.uint8 or scales.dtype != torch.uint8 or q.dim() != 2 or scales.dim() != 2 or tuple(q.shape) != (M, K)
            or tuple(scales.shape) != (M, K // MXFP8_BLOCK) or q.stride(1) != 1 or scales.stride(1) != 1):
        raise ValueError(f"quantize_mxfp8: q must be uint8 [{M}, {K}] and scales uint8 [{M}, {K // MXFP8_BLOCK}], rows contiguous")
    libfk.check(libfk.load().fk_quantize_mxfp8(x.data_ptr(), rx, M, K, q.data_ptr(), q.stride(0), scales.data_ptr(),
                                                scales.stride(0), _stream()), "fk_quantize_mxfp8")
    QUANTIZE_LAUNCHES[0] += 1
    return q, scales


def _mx_pair_out(out, M, K, device, what):
    """(q, scales) uint8 [M, >= K] / [M, >= K / 32] row-strided views for a producer's quantized output (allocated when None)."""
    if out is None:
        return (torch.empty((M, K), device=device, dtype=torch.uint8),
                torch.empty((M, K // MXFP8_BLOCK), device=device, dtype=torch.uint8))
    q, sc = out
    _need_cuda(q, sc)
    if (q.dtype != torch.uint8 or sc.dtype != torch.uint8 or q.dim() != 2 or sc.dim() != 2 or tuple(q.shape) != (M, K)
            or tuple(sc.shape) != (M, K // MXFP8_BLOCK) or q.stride(1) != 1 or sc.stride(1) != 1):
        raise ValueError(f"{what}: the output is a (uint8 [{M}, {K}], uint8 [{M}, {K // MXFP8_BLOCK}]) pair, rows contiguous")
    return q, sc


def ln_modulate_mxfp8(x, shift, scale, out=None, eps=1e-6):
    """:func:`ln_modulate` with its result stored as MXFP8: returns the (q [B * R, D], scales [B * R, D / 32]) pair that
    :func:`quantize_mxfp8` gives for ``ln_modulate(x, shift, scale)``, bit for bit; the bf16 rows are never written.  ``out``: such
    a pair (row-strided views of wider buffers are fine)."""
    _need_cuda(x, shift, scale)
    if x.dim() != 3 or x.dtype != BF16:
        raise ValueError("x must be bf16 [B, R, D]")
    B, R, D = x.shape
    M, rx = rows_of(x)
    if shift.stride(0) != scale.stride(0) or shift.stride(1) != 1 or scale.stride(1) != 1:
        raise ValueError("shift/scale must be [B, D] views with a common batch stride")
    q, sc = _mx_pair_out(out, M, D, x.device, "ln_modulate_mxfp8")
    libfk.check(libfk.load().fk_ln_modulate_mxfp8(_ptr(x), rx, _ptr(q), q.stride(0), _ptr(sc), sc.stride(0), _ptr(shift), _ptr(scale),
                                                   shift.stride(0), R, M, D, eps, _stream()), "fk_ln_modulate_mxfp8")
    return q, sc


def ln_modulate2_mxfp8(x, shift, scale, shift_b, scale_b, split, out=None, out_b=None, eps=1e-6):
    """:func:`ln_modulate2` with its result stored as MXFP8, each stream in its own dense pair: returns (first, second) where
    ``first`` = quantize_mxfp8(n[:, :split]) ([B * split, D] rows, batch-major) and ``second`` = quantize_mxfp8(n[:, split:]) for
    n = ln_modulate2(...), bit for bit.  ``out`` / ``out_b``: such pairs with a common row stride."""
    _need_cuda(x, shift, scale, shift_b, scale_b)
    if x.dim() != 3 or x.dtype != BF16:
        raise ValueError("x must be bf16 [B, R, D]")
    B, R, D = x.shape
    M, rx = rows_of(x)
    strides = {t.stride(0) for t in (shift, scale, shift_b, scale_b)}
    if len(strides) != 1 or any(t.stride(1) != 1 for t in (shift, scale, shift_b, scale_b)):
        raise ValueError("shift/scale vectors must be [B, D] views with a common batch stride")
    if not 0 <= split <= R:
        raise ValueError(f"split {split} outside [0, {R}]")
    qa, sa = _mx_pair_out(out, B * split, D, x.device, "ln_modulate2_mxfp8")
    qb, sb = _mx_pair_out(out_b, B * (R - split), D, x.device, "ln_modulate2_mxfp8")
    ldq = {t.stride(0) for t in (qa, qb) if t.shape[0] > 1} or {D}
    lds = {t.stride(0) for t in (sa, sb) if t.shape[0] > 1} or {D // MXFP8_BLOCK}
    if len(ldq) != 1 or len(lds) != 1:
        raise ValueError("ln_modulate2_mxfp8: both streams' outputs must share their row strides")
    libfk.check(libfk.load().fk_ln_modulate2_mxfp8(_ptr(x), rx, _ptr(qa), _ptr(sa), _ptr(qb), _ptr(sb), ldq.pop(), lds.pop(),
                                                    _ptr(shift), _ptr(scale), _ptr(shift_b), _ptr(scale_b), split, shift.stride(0), R,
                                                    M, D, eps, _stream()), "fk_ln_modulate2_mxfp8")
    return (qa, sa), (qb, sb)


def _mx_args(a, w, bias, out, epilogue, res, gate, out_fp32, qkv, variant, splitk=False):
    """fk_gemm_mxfp8_args of one problem; ``out`` False: no bf16 output (the quantized-output form fills its own fields).
    ``splitk``: hand the call this stream's split-K workspace and the module's launch plan (fk.h: the opt-in to variant 512)."""
    (aq, asc), (wq, wsc) = a, w
    _need_cuda(aq, asc, wq, wsc, bias, None if out is False else out, res, gate)
    for t in (aq, asc, wq, wsc):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.stride(1) != 1:
            raise TypeError("gemm_mxfp8 operands are (uint8 e4m3 [rows, K], uint8 E8M0 [rows, K / 32]) pairs (quantize_mxfp8)")
    M, K = aq.shape
    N = wq.shape[0]
    if wq.shape[1] != K or tuple(asc.shape) != (M, K // MXFP8_BLOCK) or tuple(wsc.shape) != (N, K // MXFP8_BLOCK):
        raise ValueError(f"gemm_mxfp8: a {tuple(aq.shape)} / {tuple(asc.shape)} vs w {tuple(wq.shape)} / {tuple(wsc.shape)}")
    args = GemmMxfp8Args()
    g = args.g
    if out is not False:
        if out is None:
            out = torch.empty((M, N), device=aq.device, dtype=torch.float32 if out_fp32 else BF16)
        Mo, rc = rows_of(out)
        if Mo != M or out.shape[-1] != N:
            raise ValueError(f"output shape {tuple(out.shape)} does not match M={M}, N={N}")
        g.C, g.c = out.data_ptr(), rc
    g.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        Mr, rr = rows_of(res)
        if Mr != M:
            raise ValueError("residual rows mismatch")
        g.res, g.r = res.data_ptr(), rr
    if gate is not None:
        if out.dim() != 3 or gate.dim() != 2 or gate.shape[0] != out.shape[0] or gate.stride(1) != 1:
            raise ValueError("gate must be a [B, N] view matching a 3-D output")
        g.gate, g.gate_batch_stride, g.gate_rows_per_batch = gate.data_ptr(), gate.stride(0), out.shape[1]
    g.M, g.N, g.K = M, N, K
    g.epilogue, g.out_fp32 = epilogue, 2 if out_fp32 else 0
    g.variant = int(variant)
    g.variant_used = ctypes.pointer(_variant_slot())
    if splitk:
        ws, slots = splitk_workspace(aq.device)
        g.splitk_ws, g.splitk_slots, g.plan = ws.data_ptr(), slots, launch_plan()
    if epilogue == FK_EPI_QKV:
        _set_qkv(g, qkv)
    args.A8, args.lda8, args.A_scale, args.lda_scale = aq.data_ptr(), aq.stride(0), asc.data_ptr(), asc.stride(0)
    args.W8, args.ldw8, args.W_scale, args.ldw_scale = wq.data_ptr(), wq.stride(0), wsc.data_ptr(), wsc.stride(0)
    return args, out


def _mx_q_args(a, w, bias, epilogue, variant, out_mx):
    """fk_gemm_mxfp8_q_args of one problem.  ``out_mx``: True = a fresh dense pair; (q, scales) = uint8 [M, N] / [M, N / 32]
    views (row-strided is fine); (q, scales, col_offset) = WHOLE uint8 [M, ld] / [M, ld / 32] buffers of which columns
    [col_offset, col_offset + N) (scales: / 32) are written.  Returns (args, (q, scales))."""
    M, N = a[0].shape[0], w[0].shape[0]
    col = 0
    if out_mx is True or len(out_mx) == 2:
        q, sc = _mx_pair_out(None if out_mx is True else out_mx, M, N, a[0].device, "gemm_mxfp8")
    else:
        q, sc, col = out_mx
        _need_cuda(q, sc)
        if (q.dtype != torch.uint8 or sc.dtype != torch.uint8 or q.dim() != 2 or sc.dim() != 2 or q.shape[0] != M
                or sc.shape[0] != M or q.stride(1) != 1 or sc.stride(1) != 1):
            raise ValueError(f"gemm_mxfp8: out_mx buffers must be uint8 [{M}, ld] / [{M}, ld / 32], rows contiguous")
    qa = GemmMxfp8QArgs()
    qa.a, _ = _mx_args(a, w, bias, False, epilogue, None, None, False, None, variant)
    qa.Q, qa.ldq, qa.Q_scale, qa.ldq_scale, qa.col_offset = q.data_ptr(), q.stride(0), sc.data_ptr(), sc.stride(0), int(col)
    return qa, (q, sc)


def gemm_mxfp8(a, w, bias=None, out=None, epilogue=FK_EPI_NONE, res=None, gate=None, out_fp32=False, qkv=None, variant=0,
               out_mx=None, splitk=False):
    """out = epilogue(deq(a) @ deq(w).T + bias) on the block-scaled MFMA, fp32 accumulation; the epilogues (FK_EPI_NONE,
    GELU_TANH, GATE_RES, QKV) round exactly like :func:`gemm`'s.  ``a`` / ``w``: the (q, scales) pairs of
    :func:`quantize_mxfp8` ([M, K] / [N, K]); out [M, N] or a [B, R, N] view (may alias res; with ``gate`` it must be 3-D).
    out_fp32: fp32(acc + bias) from the same main loop (parity build).  variant: 0 = launch plan, 128 / 256 = 256 x 128 /
    256 x 256 tiles, 512 = split-K pairs (needs ``splitk``).  K % 128 == 0, N % 256 == 0.

    splitk: the call gets this stream's split-K workspace and the module's launch plan (``gemm_set_plan``,
    ``gemm_set_splitk_exchange``), so the library may run a K >= 6144 launch that fills at most half the CUs as two half-K
    workgroups per 256 x 256 tile (``gemm_last_variant() == 512``; FK_EPI_NONE / GATE_RES, last-bit differences against the
    unsplit sum).  False (default): never split.

    out_mx (FK_EPI_NONE / FK_EPI_GELU_TANH): the result leaves as MXFP8 instead of bf16 -- the (q, scales) pair that
    ``quantize_mxfp8(gemm_mxfp8(...))`` gives, bit for bit, with no bf16 output stored.  True = a fresh pair, (q, scales) =
    uint8 [M, N] / [M, N / 32] views, (q, scales, col_offset) = whole [M, ld] / [M, ld / 32] buffers and the first column of
    the window to fill.  Returns the pair."""
    if out_mx is not None:
        if out is not None or res is not None or gate is not None or out_fp32 or qkv is not None:
            raise ValueError("gemm_mxfp8: out_mx replaces out; it takes no res / gate / qkv / out_fp32")
        qa, pair = _mx_q_args(a, w, bias, epilogue, variant, out_mx)
        libfk.check(libfk.load().fk_gemm_mxfp8_q(ctypes.byref(qa), _stream()), "fk_gemm_mxfp8_q")
        return pair
    args, out = _mx_args(a, w, bias, out, epilogue, res, gate, out_fp32, qkv, variant, splitk)
    libfk.check(libfk.load().fk_gemm_mxfp8(ctypes.byref(args), _stream()), "fk_gemm_mxfp8")
    return out


def gemm_mxfp8_grouped(problems, epilogue=FK_EPI_NONE, out_fp32=False, variant=0, splitk=False):
    """Up to 4 MXFP8 GEMMs sharing (N, K, epilogue) in ONE launch; ``problems``: dicts with the keyword arguments of
    :func:`gemm_mxfp8` (a, w, bias, out, res, gate, qkv).  Returns the outputs.  With ``out_mx`` in every problem (see
    :func:`gemm_mxfp8`) the launch is the quantized-output form and the (q, scales) pairs are returned.  ``splitk``: as
    :func:`gemm_mxfp8` (one workspace slot per tile of the whole launch; not for the quantized-output form)."""
    n = len(problems)
    if any(pr.get("out_mx") is not None for pr in problems):
        if not all(pr.get("out_mx") is not None for pr in problems) or out_fp32:
            raise ValueError("gemm_mxfp8_grouped: out_mx must be given for every problem of a launch (and no out_fp32)")
        qarr = (GemmMxfp8QArgs * n)()
        pairs = []
        for i, pr in enumerate(problems):
            qarr[i], pair = _mx_q_args(pr["a"], pr["w"], pr.get("bias"), epilogue, variant, pr["out_mx"])
            pairs.append(pair)
        libfk.check(libfk.load().fk_gemm_mxfp8_q_grouped(qarr, n, _stream()), "fk_gemm_mxfp8_q_grouped")
        return pairs
    arr = (GemmMxfp8Args * n)()
    outs = []
    for i, pr in enumerate(problems):
        args, out = _mx_args(pr["a"], pr["w"], pr.get("bias"), pr.get("out"), epilogue, pr.get("res"), pr.get("gate"),
                             out_fp32, pr.get("qkv"), variant, splitk)
        arr[i] = args
        outs.append(out)
    libfk.check(libfk.load().fk_gemm_mxfp8_grouped(arr, n, _stream()), "fk_gemm_mxfp8_grouped")
    return outs


def ln_modulate(x, shift, scale, out=None, eps=1e-6):
    """out = LN(x) * (1 + scale[b]) + shift[b]; x/out: [B,R,D] views, shift/scale: [B,D] views."""
    _need_cuda(x, shift, scale, out)
    if x.dim() != 3:
        raise ValueError("x must be [B, R, D]")
    B, R, D = x.shape
    if out is None:
        out = torch.empty((B, R, D), device=x.device, dtype=BF16)
    M, rx = rows_of(x)
    _, ro = rows_of(out)
    if shift.stride(0) != scale.stride(0) or shift.stride(1) != 1 or scale.stride(1) != 1:
        raise ValueError("shift/scale must be [B, D] views with a common batch stride")
    lib = libfk.load()
    libfk.check(lib.fk_ln_modulate_bf16(_ptr(x), rx, _ptr(out), ro, _ptr(shift), _ptr(scale),
                                        shift.stride(0), R, M, D, eps, _stream()), "fk_ln_modulate_bf16")
    return out


def ln_modulate2(x, shift_a, scale_a, shift_b, scale_b, split, out=None, eps=1e-6):
    """Joint-sequence LN+modulate: rows [0, split) of every batch use (shift_a, scale_a), the rest (b)."""
    _need_cuda(x, shift_a, scale_a, shift_b, scale_b, out)
    B, R, D = x.shape
    if out is None:
        out = torch.empty((B, R, D), device=x.device, dtype=BF16)
    M, rx = rows_of(x)
    _, ro = rows_of(out)
    st = shift_a.stride(0)
    if any(t.stride(0) != st or t.stride(1) != 1 for t in (scale_a, shift_b, scale_b)):
        raise ValueError("modulation views must share one batch stride")
    libfk.check(libfk.load().fk_ln_modulate2_bf16(_ptr(x), rx, _ptr(out), ro, _ptr(shift_a), _ptr(scale_a),
                                                  _ptr(shift_b), _ptr(scale_b), split, st, R, M, D, eps, _stream()),
                "fk_ln_modulate2_bf16")
    return out


def qkv_post(qkv, q_out, k_out, wq_img, wk_img, wq_txt, wk_txt, cos, sin, s_txt, eps=1e-6):
    """RMSNorm + RoPE + re-layout of q, k: qkv [B,S,3*H*128] -> q/k [B,H,S,128] (V stays in qkv)."""
    _need_cuda(qkv, q_out, k_out, cos, sin)
    B, S, D3 = qkv.shape
    H = D3 // 384
    if not qkv.is_contiguous():
        raise ValueError("qkv must be contiguous")
    lib = libfk.load()
    libfk.check(lib.fk_qkv_post_bf16(_ptr(qkv), _ptr(q_out), _ptr(k_out), _ptr(wq_img), _ptr(wk_img), _ptr(wq_txt),
                                     _ptr(wk_txt), _ptr(cos), _ptr(sin), B, S, s_txt, H, eps, _stream()),
                "fk_qkv_post_bf16")


_ATTN_WS = {}


def attention_workspace(device):
    """Stream-K workspace of the attention forward for the current stream of ``device`` (fk_attention_ws_bytes(), zeroed
    once: monotonic tickets afterwards)."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(device).cuda_stream)
    ws = _ATTN_WS.get(key)
    if ws is None:
        ws = torch.zeros(libfk.load().fk_attention_ws_bytes(), device=device, dtype=torch.uint8)
        _ATTN_WS[key] = ws
    return ws


def attention_set_split(mode):
    """Grid of the attention forward and of the backward's dQ pass (the `grid` argument of fk_attention_fwd_ws_bf16 /
    fk_attention_bwd_ws_bf16): 1 = stream-K grids where the plain grid wastes a round (default), 0 = never (batch-invariant),
    >= 2 = a persistent grid of that many workgroups wherever every block is cut at most once (test hook)."""
    mode = int(mode)
    if mode < 0:
        raise ValueError(f"attention_set_split: {mode} is not 0, 1 or a workgroup count >= 2")
    _set_launch(attn_grid={0: -1, 1: 0}.get(mode, mode))


def pack_key_mask(mask):
    """Key-padding mask of the attention kernels (fk_pack_key_mask): bool / 0-1 ``mask`` [B, S], True = valid key, ->
    int64 [B, ceil(S / 64)]; bit j of word (b, t) is key 64 t + j of sample b (bits at positions >= S are 0).  Every sample
    needs at least one valid key, and the K / V rows of masked keys must be finite (fk.h has the precondition)."""
    _need_cuda(mask)
    if mask.dim() != 2:
        raise ValueError("pack_key_mask takes a [B, S] mask")
    m = (mask != 0).to(torch.uint8).contiguous()
    B, S = m.shape
    out = torch.empty((B, (S + 63) // 64), device=m.device, dtype=torch.int64)
    libfk.check(libfk.load().fk_pack_key_mask(_ptr(m), m.stride(0), B, S, _ptr(out), _stream()), "fk_pack_key_mask")
    return out


def _check_key_mask(key_mask, B, S):
    if key_mask.dtype != torch.int64 or key_mask.shape != (B, (S + 63) // 64) or not key_mask.is_contiguous():
        raise ValueError(f"key_mask must be the contiguous int64 [{B}, {(S + 63) // 64}] tensor pack_key_mask gives")


def attention(q, k, v, out, scale=None, lse=None, key_mask=None):
    """out[b, s, h*128:(h+1)*128] = softmax(q k^T * scale) v.

    q, k: [B,H,S,128] contiguous; v: [B,S,H*128] view with contiguous last dim (e.g. qkv[:, :, 2D:]);
    out: [B,S,>=H*128] view; lse: optional fp32 [B,H,S] (log2 domain, for :func:`attention_bwd`);
    key_mask: optional :func:`pack_key_mask` tensor -- only valid keys take part (fk_attention_fwd_masked_bf16: the 8-wave
    kernel on the plain grid)."""
    _need_cuda(q, k, v, out, lse, key_mask)
    B, H, S, hd = q.shape
    if hd != 128:
        raise ValueError("head_dim must be 128")
    if v.dim() != 3 or v.shape[-1] != H * 128 or v.stride(2) != 1:
        raise ValueError("v must be a [B, S, H*128] view with a contiguous last dimension")
    if lse is not None and (lse.dtype != torch.float32 or lse.shape != (B, H, S) or not lse.is_contiguous()):
        raise ValueError("lse must be a contiguous fp32 [B,H,S] tensor")
    if scale is None:
        scale = hd ** -0.5
    if key_mask is not None:
        _check_key_mask(key_mask, B, S)
        libfk.check(libfk.load().fk_attention_fwd_masked_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), _ptr(key_mask), B, H, S,
                                                             v.stride(1), v.stride(0), out.stride(1), out.stride(0), scale,
                                                             _stream()), "fk_attention_fwd_masked_bf16")
        return out
    ws = attention_workspace(q.device)
    libfk.check(libfk.load().fk_attention_fwd_ws_bf16(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), B, H, S, v.stride(1),
                                                     v.stride(0), out.stride(1), out.stride(0), scale, _ptr(ws), ws.numel(),
                                                     LAUNCH.attn_grid, _stream()), "fk_attention_fwd_bf16")
    return out


def attention_mxfp8(q, k, v, out, out_b=None, split=0, scale=None, lse=None):
    """:func:`attention` with its result stored as MXFP8 (fk_attention_fwd_ws_mxfp8): the bytes :func:`quantize_mxfp8` gives for
    the bf16 output, which is never written.  ``out`` = (codes uint8 [rows, >= H*128], scales uint8 [rows, >= H*4]) row-strided
    views; head h fills columns [128 h, 128 h + 128) / [4 h, 4 h + 4) of a row.  Tokens [0, split) of batch b are the rows
    b * split + s of ``out``, tokens [split, S) the rows b * (S - split) + s - split of ``out_b`` (same row strides);
    ``split`` 0 or S: everything goes to ``out``.  Same grid choice (``LAUNCH.attn_grid``) and workspace as :func:`attention`."""
    _need_cuda(q, k, v, lse, *out, *(out_b or ()))
    B, H, S, hd = q.shape
    if hd != 128:
        raise ValueError("head_dim must be 128")
    if v.dim() != 3 or v.shape[-1] != H * 128 or v.stride(2) != 1:
        raise ValueError("v must be a [B, S, H*128] view with a contiguous last dimension")
    if lse is not None and (lse.dtype != torch.float32 or lse.shape != (B, H, S) or not lse.is_contiguous()):
        raise ValueError("lse must be a contiguous fp32 [B,H,S] tensor")
    pairs = [out] + ([out_b] if out_b is not None else [])
    for qt, st in pairs:
        if qt.dtype != torch.uint8 or st.dtype != torch.uint8 or qt.dim() != 2 or st.dim() != 2 or qt.stride(1) != 1 or st.stride(1) != 1:
            raise ValueError("attention_mxfp8: an output is a (uint8 [rows, cols], uint8 [rows, cols / 32]) pair, rows contiguous")
    if len({pr[0].stride(0) for pr in pairs}) != 1 or len({pr[1].stride(0) for pr in pairs}) != 1:
        raise ValueError("attention_mxfp8: both streams' outputs must share their row strides")
    dst = libfk.AttnMxOut(_ptr(out[0]), _ptr(out[1]), _ptr(out_b[0]) if out_b is not None else None,
                          _ptr(out_b[1]) if out_b is not None else None, int(split), out[0].stride(0), out[1].stride(0))
    ws = attention_workspace(q.device)
    libfk.check(libfk.load().fk_attention_fwd_ws_mxfp8(_ptr(q), _ptr(k), _ptr(v), _ptr(lse), B, H, S, v.stride(1), v.stride(0),
                                                      hd ** -0.5 if scale is None else scale, ctypes.byref(dst), _ptr(ws),
                                                      ws.numel(), LAUNCH.attn_grid, _stream()), "fk_attention_fwd_ws_mxfp8")
    return out if out_b is None else (out, out_b)


def attention_f32_debug(q, k, v, scale=None, key_mask=None):
    """Parity build of :func:`attention` (fk_attention_fwd_f32_debug): fp32 [B, S, H*128] output, P as hi + lo bf16;
    with ``key_mask`` (:func:`pack_key_mask`) fk_attention_fwd_masked_f32_debug."""
    _need_cuda(q, k, v, key_mask)
    B, H, S, hd = q.shape
    if hd != 128 or v.dim() != 3 or v.shape[-1] != H * 128 or v.stride(2) != 1:
        raise ValueError("q, k: [B,H,S,128]; v: [B,S,H*128] view with a contiguous last dimension")
    out = torch.empty((B, S, H * 128), device=q.device, dtype=torch.float32)
    if key_mask is not None:
        _check_key_mask(key_mask, B, S)
        libfk.check(libfk.load().fk_attention_fwd_masked_f32_debug(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(key_mask), B, H, S,
                                                                  v.stride(1), v.stride(0), out.stride(1), out.stride(0),
                                                                  hd ** -0.5 if scale is None else scale, _stream()),
                    "fk_attention_fwd_masked_f32_debug")
        return out
    libfk.check(libfk.load().fk_attention_fwd_f32_debug(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, H, S, v.stride(1),
                                                       v.stride(0), out.stride(1), out.stride(0),
                                                       hd ** -0.5 if scale is None else scale, _stream()),
                "fk_attention_fwd_f32_debug")
    return out


def silu(x, out=None):
    _need_cuda(x)
    if out is None:
        out = torch.empty_like(x)
    libfk.check(libfk.load().fk_silu_bf16(_ptr(x), _ptr(out), x.numel(), _stream()), "fk_silu_bf16")
    return out


def add3(a, b, c, out=None):
    _need_cuda(a, b, c)
    if out is None:
        out = torch.empty_like(a)
    libfk.check(libfk.load().fk_add3_bf16(_ptr(a), _ptr(b), _ptr(c), _ptr(out), a.numel(), _stream()),
                "fk_add3_bf16")
    return out


def true_cfg(pos, neg, scale, out=None):
    """out = neg + scale * (pos - neg) with the reference's bf16 rounding points (flux_pipeline.py:1095)."""
    _need_cuda(pos, neg, out)
    if pos.shape != neg.shape or pos.dtype != BF16 or neg.dtype != BF16 or not (pos.is_contiguous() and neg.is_contiguous()):
        raise ValueError("true_cfg takes two contiguous bf16 tensors of one shape")
    if out is None:
        out = torch.empty_like(pos)
    libfk.check(libfk.load().fk_true_cfg_bf16(_ptr(pos), _ptr(neg), _ptr(out), float(scale), pos.numel(), _stream()),
                "fk_true_cfg_bf16")
    return out


def timestep_proj(v, freqs, out=None):
    """[B] (bf16 or fp32) -> [B,256] bf16 sinusoid of bf16(v)*1000 (cos first)."""
    _need_cuda(v, freqs)
    B = v.shape[0]
    if v.dtype not in (BF16, torch.float32):
        raise TypeError("timestep must be bf16 or fp32")
    if out is None:
        out = torch.empty((B, 256), device=v.device, dtype=BF16)
    libfk.check(libfk.load().fk_timestep_proj(_ptr(v), int(v.dtype == torch.float32), _ptr(freqs), _ptr(out),
                                              B, _stream()), "fk_timestep_proj")
    return out


def euler_step(x, v, s_tgt, dsigma):
    """In place: x[:, :s_tgt] += bf16(bf16(dsigma) * v[:, :s_tgt]) with the reference's rounding."""
    _need_cuda(x, v)
    B, _, C = x.shape
    libfk.check(libfk.load().fk_euler_step_bf16(_ptr(x), x.stride(0), _ptr(v), v.stride(0), B, s_tgt, C,
                                                float(dsigma), _stream()), "fk_euler_step_bf16")
    return x


def _token_rows(B, s_tgt, C, mask=True, **rows):
    """Checks that every given row tensor is bf16 [B, >= s_tgt, C] with contiguous rows; returns their [pointer, batch stride, ...]
    as the C ABI takes them.  None = an operand the call does not have (NULL, 0), and so are x0 / noise when ``mask`` is None."""
    args = []
    for name, t in rows.items():
        if t is None or (mask is None and name in ("x0", "noise")):
            args += (None, 0)
            continue
        if t.dtype != BF16 or t.dim() != 3 or t.shape[0] != B or t.shape[1] < s_tgt or t.shape[2] != C or \
                t.stride(2) != 1 or t.stride(1) != C:
            raise ValueError(f"{name} must be bf16 [{B}, >= {s_tgt}, {C}] with contiguous rows, got {tuple(t.shape)} {t.dtype}")
        args += (ctypes.c_void_p(t.data_ptr()), t.stride(0))
    return args


def _mask_args(mask, B, s_tgt):
    """[pointer, batch stride] of the compact mask of :func:`pack_inpaint_mask`, checked; stride 0 = one mask for the batch."""
    if mask is None:
        return None, 0
    if mask.dtype != BF16 or mask.dim() != 3 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (s_tgt, 4) \
            or not mask.is_contiguous():
        raise ValueError(f"mask must be contiguous bf16 [1 or {B}, {s_tgt}, 4], got {tuple(mask.shape)} {mask.dtype}")
    return ctypes.c_void_p(mask.data_ptr()), mask.stride(0) if mask.shape[0] == B and B > 1 else 0


def euler_inpaint_step(x, v, s_tgt, dsigma, sigma_next, x0, noise, mask=None):
    """In place on x[:, :s_tgt]: the Euler update where ``mask`` is 1, the preserved picture ``x0`` re-noised to
    ``sigma_next`` with the call's ``noise`` where it is 0 (include/fk.h: fk_euler_inpaint_step_bf16).  ``mask``: the compact
    [1 or B, s_tgt, 4] bf16 mask of :func:`pack_inpaint_mask`; None = ones, the values of :func:`euler_step`."""
    _need_cuda(x, v, x0, noise, mask)
    B, _, C = x.shape
    rows = _token_rows(B, s_tgt, C, mask, x=x, v=v, x0=x0, noise=noise)
    libfk.check(libfk.load().fk_euler_inpaint_step_bf16(*rows, *_mask_args(mask, B, s_tgt), B, s_tgt, C, float(dsigma),
                                                        float(sigma_next), _stream()), "fk_euler_inpaint_step_bf16")
    return x


def ab2_step(x, v, hist, s_tgt, c_v, c_h, use_hist, sigma_next=0.0, x0=None, noise=None, mask=None):
    """In place on x[:, :s_tgt]: the second-order multistep update bf16(x + c_v * v [+ c_h * hist]), summed in fp32 with the
    coefficients as the fp32 numbers they are, and hist <- v[:, :s_tgt] in the same pass (include/fk.h: fk_ab2_step_bf16).
    ``use_hist`` 0: a first-order step that does not read ``hist`` (the first step, whose history is whatever the buffer held).
    ``mask``: as in :func:`euler_inpaint_step`, with this update where it is 1; None = ones, and ``x0`` / ``noise`` /
    ``sigma_next`` are not used."""
    _need_cuda(x, v, hist, x0, noise, mask)
    B, _, C = x.shape
    rows = _token_rows(B, s_tgt, C, mask, x=x, v=v, hist=hist, x0=x0, noise=noise)
    libfk.check(libfk.load().fk_ab2_step_bf16(*rows, *_mask_args(mask, B, s_tgt), B, s_tgt, C, float(c_v), float(c_h),
                                              int(use_hist), float(sigma_next), _stream()), "fk_ab2_step_bf16")
    return x


def solver_step_f32(state, x, v, s_tgt, c_v, c_h=0.0, use_hist=0, load_state=1, hist=None, sigma_next=0.0, x0=None, noise=None,
                    mask=None):
    """The loop's step on a float32 latent state, in place on ``state`` (fp32 [B, s_tgt, C]) and on x[:, :s_tgt], which receives
    the state's one rounding to bf16 (include/fk.h: fk_solver_step_f32): state + c_v * v [+ c_h * hist] in float32, from
    float(x) instead of ``state`` when ``load_state`` is 0 (the first step: ``state`` is then not read).  Euler: ``use_hist`` 0,
    ``hist`` None, ``c_v`` the unrounded float32 step size; AB2: :func:`ab2_step`'s coefficients and ``hist``, which receives
    v[:, :s_tgt] in the same pass.  ``mask``: as in :func:`euler_inpaint_step`, blended in float32; None = ones."""
    _need_cuda(state, x, v, hist, x0, noise, mask)
    B, _, C = x.shape
    rows = _token_rows(B, s_tgt, C, mask, x=x, v=v, hist=hist, x0=x0, noise=noise)
    if state.dtype != torch.float32 or tuple(state.shape) != (B, s_tgt, C) or state.stride(2) != 1 or state.stride(1) != C:
        raise ValueError(f"state must be fp32 [{B}, {s_tgt}, {C}] with contiguous rows, got {tuple(state.shape)} {state.dtype}")
    libfk.check(libfk.load().fk_solver_step_f32(
        _ptr(state), state.stride(0), *rows, *_mask_args(mask, B, s_tgt), B, s_tgt, C, float(c_v), float(c_h), int(use_hist),
        int(load_state), float(sigma_next), _stream()), "fk_solver_step_f32")
    return x


def scale_noise(x0, noise, sigma, out=None):
    """bf16(bf16(sigma) * noise) + bf16(1 - bf16(sigma)) * x0 with one rounding per bf16 tensor op
    (FlowMatchEulerDiscreteScheduler.scale_noise): the start tokens of an edit that begins inside the schedule."""
    _need_cuda(x0, noise, out)
    B, S, C = x0.shape
    if out is None:
        out = torch.empty((B, S, C), device=x0.device, dtype=BF16)
    rows = _token_rows(B, S, C, x0=x0, noise=noise, out=out)
    libfk.check(libfk.load().fk_scale_noise_bf16(*rows, B, S, C, float(sigma), _stream()), "fk_scale_noise_bf16")
    return out


def pack_inpaint_mask(mask, h_lat, w_lat):
    """[Bm, 1, Hm, Wm] mask in [0, 1] (1 = repaint) -> the compact [Bm, (h_lat/2) * (w_lat/2), 4] bf16 token mask of
    fk_euler_inpaint_step_bf16: binarised at 0.5 (>= 0.5 -> 1), nearest-resized to the latent size, packed 2 x 2 like
    ``_pack_latents`` packs one channel -- element k of a token's four is the sub-pixel every latent element j with
    j % 4 == k lies on.  Host-side torch on a few KB, once per call; runs on any device."""
    if not torch.is_tensor(mask) or mask.dim() != 4 or mask.shape[1] != 1:
        raise ValueError("mask must be a [B, 1, H, W] tensor")
    if h_lat % 2 or w_lat % 2:
        raise ValueError("the latent size must be even (2 x 2 packing)")
    m = (mask.to(torch.float32) >= 0.5).to(torch.float32)
    if tuple(m.shape[2:]) != (h_lat, w_lat):
        m = torch.nn.functional.interpolate(m, size=(h_lat, w_lat), mode="nearest")
    m = m.view(m.shape[0], h_lat // 2, 2, w_lat // 2, 2).permute(0, 1, 3, 2, 4)
    return m.reshape(m.shape[0], (h_lat // 2) * (w_lat // 2), 4).to(BF16).contiguous()


# ---- step cache (include/fk.h: fk_absdiff_sums_bf16, fk_residual_absdiff_sums_bf16, fk_residual_save_bf16, fk_residual_apply_bf16)
def _step_cache_views(what, *ts):
    """(M, D, is_bf16, [Rows]) of [B, R, D] (or [M, D]) views of one shape and dtype with contiguous rows.  The dtype travels
    with the call: the library refuses anything but bf16 (FK_EUNSUPPORTED)."""
    _need_cuda(*ts)
    t0 = ts[0]
    for t in ts:
        if t.dim() not in (2, 3) or t.shape != t0.shape or t.dtype != t0.dtype:
            raise ValueError(f"{what} takes [B, R, D] views of one shape and dtype, got "
                             f"{[(tuple(t.shape), t.dtype) for t in ts]}")
    rows = [rows_of(t) for t in ts]
    return rows[0][0], t0.shape[-1], int(t0.dtype == BF16), [r for _, r in rows]


def absdiff_ws(device):
    """The partials workspace of :func:`absdiff_sums` (fp32): one per stream of ordered launches."""
    return torch.empty(libfk.load().fk_absdiff_ws_floats(), device=device, dtype=torch.float32)


def absdiff_sums(a, b, out=None, ws=None):
    """fp32 [2]: (sum |a - b|, sum |b|) over two bf16 [B, R, D] views with contiguous rows (a row and a batch stride of their
    own), fixed summation order: two calls on the same data give the same bits.  ``ws``: :func:`absdiff_ws` (allocated per call
    when None -- the hot path owns one)."""
    M, D, eb, (ra, rb) = _step_cache_views("absdiff_sums", a, b)
    if out is None:
        out = torch.empty(2, device=a.device, dtype=torch.float32)
    if ws is None:
        ws = absdiff_ws(a.device)
    _need_cuda(out, ws)
    if out.dtype != torch.float32 or out.numel() < 2 or not out.is_contiguous() or ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("out must be fp32 [2], ws a contiguous fp32 workspace")
    libfk.check(libfk.load().fk_absdiff_sums_bf16(_ptr(a), ra, _ptr(b), rb, M, D, eb, _ptr(out), _ptr(ws), ws.numel(), _stream()),
                "fk_absdiff_sums_bf16")
    return out


def residual_absdiff_sums(h1, h0, ref, r_out=None, out=None, ws=None):
    """The first-block measure in one pass: ``r = bf16(float(h1) - float(h0))`` (:func:`residual_save`'s value, written to
    ``r_out`` when given) and fp32 [2] ``(sum |r - ref|, sum |ref|)`` in :func:`absdiff_sums`' order -- the bits of
    ``residual_save(h1, h0, r)`` followed by ``absdiff_sums(r, ref)``.  bf16 [B, R, D] views with contiguous rows; ``r_out`` may
    overlap no input."""
    views = (h1, h0, ref) if r_out is None else (h1, h0, ref, r_out)
    M, D, eb, rows = _step_cache_views("residual_absdiff_sums", *views)
    if out is None:
        out = torch.empty(2, device=h1.device, dtype=torch.float32)
    if ws is None:
        ws = absdiff_ws(h1.device)
    _need_cuda(out, ws)
    if out.dtype != torch.float32 or out.numel() < 2 or not out.is_contiguous() or ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("out must be fp32 [2], ws a contiguous fp32 workspace")
    rr = rows[3] if r_out is not None else Rows(0, 0, 0)
    libfk.check(libfk.load().fk_residual_absdiff_sums_bf16(_ptr(h1), rows[0], _ptr(h0), rows[1], _ptr(ref), rows[2], _ptr(r_out), rr,
                                                           M, D, eb, _ptr(out), _ptr(ws), ws.numel(), _stream()),
                "fk_residual_absdiff_sums_bf16")
    return out


def residual_save(h_out, h0, r):
    """r = bf16(float(h_out) - float(h0)) over bf16 [B, R, D] views with contiguous rows; no two may overlap."""
    M, D, eb, (ro, r0, rr) = _step_cache_views("residual_save", h_out, h0, r)
    libfk.check(libfk.load().fk_residual_save_bf16(_ptr(h_out), ro, _ptr(h0), r0, _ptr(r), rr, M, D, eb, _stream()),
                "fk_residual_save_bf16")
    return r


def residual_apply(h0, r, out):
    """out = bf16(float(h0) + float(r)) over bf16 [B, R, D] views with contiguous rows; ``out`` may be ``h0`` itself."""
    M, D, eb, (r0, rr, ro) = _step_cache_views("residual_apply", h0, r, out)
    libfk.check(libfk.load().fk_residual_apply_bf16(_ptr(h0), r0, _ptr(r), rr, _ptr(out), ro, M, D, eb, _stream()),
                "fk_residual_apply_bf16")
    return out


# ---- LoRA merge (include/fk.h: fk_lora_merge_bf16) ---------------------------------------------------------------------
def lora_merge(base, terms, out=None):
    """out = bf16(float(base) + sum_t scale_t * (up_t @ down_t)) over a bf16 weight [N, K] (fp32 accumulation, terms added in
    order).  ``terms``: a list of ``(up [N, r], down [r, K], scale)``.  ``out=None`` merges in place.  2-D views with a
    contiguous last dimension; every refusal comes from the library."""
    if out is None:
        out = base
    terms = list(terms)
    ts = [base, out] + [t for up, down, _ in terms for t in (up, down)]
    _need_cuda(*ts)
    for t in ts:
        if t.dim() != 2 or t.stride(-1) != 1 or t.dtype != BF16:
            raise ValueError(f"lora_merge takes 2-D bf16 views with a contiguous last dimension, got {tuple(t.shape)} {t.dtype} "
                             f"strides {t.stride()}")
    N, K = base.shape
    if out.shape != base.shape:
        raise ValueError(f"out is {tuple(out.shape)}, base {tuple(base.shape)}")
    arr = (libfk.LoraTerm * max(len(terms), 1))()
    for i, (up, down, scale) in enumerate(terms):
        if up.shape[0] != N or down.shape[1] != K or up.shape[1] != down.shape[0]:
            raise ValueError(f"term {i}: up {tuple(up.shape)} / down {tuple(down.shape)} do not fit the weight [{N}, {K}]")
        arr[i] = libfk.LoraTerm(up.data_ptr(), up.stride(0), down.data_ptr(), down.stride(0), up.shape[1], float(scale))
    libfk.check(libfk.load().fk_lora_merge_bf16(_ptr(base), base.stride(0), _ptr(out), out.stride(0), N, K, arr, len(terms),
                                                _stream()), "fk_lora_merge_bf16")
    return out


# ---- LoRA gradient projection (include/fk.h: fk_lora_grad_bf16) ----------------------------------------------------------
def lora_grad_ws(N, K, rank, device):
    """The partials workspace of :func:`lora_grad` for a weight [N, K] at ``rank`` (fp32; empty when the kernel splits
    nothing): one per stream of ordered launches."""
    return torch.empty(libfk.load().fk_lora_grad_ws_floats(N, K, rank), device=device, dtype=torch.float32)


def lora_grad(dw, up, down, scale, d_up=None, d_down=None, ws=None, accumulate=False):
    """(d_up [N, r], d_down [r, K]) in fp32: ``scale * dw @ down^T`` and ``scale * up^T @ dw`` for the weight gradient
    ``dw`` bf16 [N, K] of a weight merged as ``base + scale * up @ down`` (fp32 accumulation, fixed summation order: two calls
    give the same bits).  ``dw``, ``up`` [N, r], ``down`` [r, K]: 2-D bf16 views with a contiguous last dimension; the
    outputs contiguous fp32 (views at any 4-byte offset of a larger buffer will do).  ``ws``: :func:`lora_grad_ws` (allocated per
    call when None -- the hot path owns one).  ``accumulate=True`` (``fk_lora_grad_acc_bf16``): the projection is ADDED to what
    ``d_up`` / ``d_down`` hold -- a further micro-batch -- each element read once and written once, the order still fixed."""
    ins = [dw, up, down]
    if accumulate and (d_up is None or d_down is None):
        raise ValueError("lora_grad(accumulate=True) adds to d_up / d_down: pass both")
    _need_cuda(*ins)
    for t in ins:
        if t.dim() != 2 or t.stride(-1) != 1 or t.dtype != BF16:
            raise ValueError(f"lora_grad takes 2-D bf16 views with a contiguous last dimension, got {tuple(t.shape)} {t.dtype} "
                             f"strides {t.stride()}")
    N, K = dw.shape
    r = up.shape[1]
    if up.shape[0] != N or down.shape[1] != K or down.shape[0] != r:
        raise ValueError(f"up {tuple(up.shape)} / down {tuple(down.shape)} do not fit the gradient [{N}, {K}]")
    if d_up is None:
        d_up = torch.empty(N, r, device=dw.device, dtype=torch.float32)
    if d_down is None:
        d_down = torch.empty(r, K, device=dw.device, dtype=torch.float32)
    need = libfk.load().fk_lora_grad_ws_floats(N, K, r)
    if ws is None:
        ws = torch.empty(need, device=dw.device, dtype=torch.float32)
    _need_cuda(d_up, d_down, ws)
    for t, shape in ((d_up, (N, r)), (d_down, (r, K))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"lora_grad writes contiguous fp32 {shape}, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
    if ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("ws must be a contiguous fp32 workspace")
    if accumulate:
        libfk.check(libfk.load().fk_lora_grad_acc_bf16(_ptr(dw), dw.stride(0), _ptr(up), up.stride(0), _ptr(down), down.stride(0), N, K,
                                                       r, float(scale), _ptr(d_up), _ptr(d_down), int(accumulate),
                                                       _ptr(ws) if ws.numel() else None, ws.numel(), _stream()),
                    "fk_lora_grad_acc_bf16")
        return d_up, d_down
    libfk.check(libfk.load().fk_lora_grad_bf16(_ptr(dw), dw.stride(0), _ptr(up), up.stride(0), _ptr(down), down.stride(0), N, K, r,
                                               float(scale), _ptr(d_up), _ptr(d_down), _ptr(ws) if ws.numel() else None,
                                               ws.numel(), _stream()), "fk_lora_grad_bf16")
    return d_up, d_down


# ---- factored LoRA gradient (include/fk.h: fk_lora_side_grad_bf16) -------------------------------------------------------
def _side_view(t, what):
    """(B, R, cols, row stride, batch stride) of a 2-D [R, cols] or 3-D [B, R, cols] bf16 view with a contiguous last dimension."""
    if t.dim() not in (2, 3) or t.stride(-1) != 1 or t.dtype != BF16:
        raise ValueError(f"lora_side_grad takes {what} as a 2-D or 3-D bf16 view with a contiguous last dimension, got "
                         f"{tuple(t.shape)} {t.dtype} strides {t.stride()}")
    if t.dim() == 2:
        return 1, t.shape[0], t.shape[1], t.stride(0), 0
    return t.shape[0], t.shape[1], t.shape[2], t.stride(1), t.stride(0)


def lora_side_grad_ws_floats(B, R, N, K, rank):
    """fp32 elements of :func:`lora_side_grad`'s workspace."""
    return libfk.load().fk_lora_side_grad_ws_floats(B, R, N, K, rank)


def lora_side_grad_ws(B, R, N, K, rank, device):
    """The workspace of :func:`lora_side_grad` for ``B * R`` rows of a linear [N, K] at ``rank`` (fp32 elements: the split-bf16
    intermediates and the partials of the split reduction): one per stream of ordered launches."""
    return torch.empty(lora_side_grad_ws_floats(B, R, N, K, rank), device=device, dtype=torch.float32)


def lora_side_grad(x, dy, up, down, scale, d_up=None, d_down=None, ws=None, accumulate=False):
    """(d_up [N, r], d_down [r, K]) in fp32 for a linear ``y = x W^T`` whose weight was merged as ``base + scale * up @ down``:
    ``scale * dy^T (x down^T)`` and ``scale * (dy up)^T x``, from the linear's own backward operands ``x`` [B, R, K] and ``dy``
    [B, R, N] -- the weight gradient ``dy^T x`` is never formed (fp32 accumulation, split-bf16 intermediates, fixed summation order:
    two calls give the same bits).  ``x`` / ``dy``: bf16 views with a contiguous last dimension and any row and batch stride (2-D
    means B = 1); ``up`` [N, r], ``down`` [r, K]: 2-D bf16 views with a contiguous last dimension; the outputs contiguous fp32
    (views at any 4-byte offset of a larger buffer will do).  ``ws``: :func:`lora_side_grad_ws` (allocated per call when None --
    the hot path owns one).  ``accumulate=True``: the result is ADDED to what ``d_up`` / ``d_down`` hold."""
    if accumulate and (d_up is None or d_down is None):
        raise ValueError("lora_side_grad(accumulate=True) adds to d_up / d_down: pass both")
    _need_cuda(x, dy, up, down)
    B, R, K, ld_x, bs_x = _side_view(x, "x")
    B2, R2, N, ld_dy, bs_dy = _side_view(dy, "dy")
    if (B, R) != (B2, R2):
        raise ValueError(f"x {tuple(x.shape)} and dy {tuple(dy.shape)} do not have the same rows")
    for t in (up, down):
        if t.dim() != 2 or t.stride(-1) != 1 or t.dtype != BF16:
            raise ValueError(f"lora_side_grad takes up / down as 2-D bf16 views with a contiguous last dimension, got "
                             f"{tuple(t.shape)} {t.dtype} strides {t.stride()}")
    r = up.shape[1]
    if up.shape[0] != N or down.shape[1] != K or down.shape[0] != r:
        raise ValueError(f"up {tuple(up.shape)} / down {tuple(down.shape)} do not fit the linear [{N}, {K}]")
    if d_up is None:
        d_up = torch.empty(N, r, device=x.device, dtype=torch.float32)
    if d_down is None:
        d_down = torch.empty(r, K, device=x.device, dtype=torch.float32)
    if ws is None:
        ws = lora_side_grad_ws(B, R, N, K, r, x.device)
    _need_cuda(d_up, d_down, ws)
    for t, shape in ((d_up, (N, r)), (d_down, (r, K))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"lora_side_grad writes contiguous fp32 {shape}, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
    if ws.dtype != torch.float32 or not ws.is_contiguous():
        raise ValueError("ws must be a contiguous fp32 workspace")
    libfk.check(libfk.load().fk_lora_side_grad_bf16(_ptr(x), ld_x, bs_x, _ptr(dy), ld_dy, bs_dy, B, R, N, K, _ptr(up), up.stride(0),
                                                    _ptr(down), down.stride(0), r, float(scale), _ptr(d_up), _ptr(d_down),
                                                    int(accumulate), _ptr(ws) if ws.numel() else None, ws.numel(), _stream()),
                "fk_lora_side_grad_bf16")
    return d_up, d_down


def transpose(src, dst):
    """dst[b, c, r] = src[b, r, c] for 3-D views with contiguous last dims."""
    _need_cuda(src, dst)
    Bn, R, C = src.shape
    libfk.check(libfk.load().fk_transpose_bf16(_ptr(src), src.stride(1), src.stride(0), _ptr(dst),
                                               dst.stride(1), dst.stride(0), R, C, Bn, _stream()),
                "fk_transpose_bf16")
    return dst


def attention_hd512(q, k, v, out=None, scale=None):
    """Fused single-head attention with head dimension 512 (the VAE mid block): q, k, v bf16 [B, S, 512] views with a common
    row / batch stride (column blocks of one fused projection), out [B, S, 512]; nothing of size S x S is allocated."""
    _need_cuda(q, k, v, out)
    B, S, C = q.shape
    if C != 512 or k.shape != q.shape or v.shape != q.shape or q.dtype != BF16:
        raise ValueError("attention_hd512 takes bf16 [B, S, 512] q, k, v")
    if not (q.stride() == k.stride() == v.stride()) or q.stride(2) != 1:
        raise ValueError("attention_hd512: q, k, v must share their strides (views of one projection buffer)")
    if out is None:
        out = torch.empty((B, S, C), device=q.device, dtype=BF16)
    if out.stride(2) != 1:
        raise ValueError("attention_hd512: out rows must be contiguous")
    libfk.check(libfk.load().fk_attention_hd512_bf16(_ptr(q), _ptr(k), _ptr(v), q.stride(1), q.stride(0), _ptr(out), out.stride(1),
                                                     out.stride(0), B, S, float(scale if scale is not None else C ** -0.5), _stream()),
                "fk_attention_hd512_bf16")
    return out


def softmax_rows(x, out=None):
    """fp32 [rows, n] -> bf16 softmax rows."""
    _need_cuda(x)
    rows, n = x.shape
    if out is None:
        out = torch.empty((rows, n), device=x.device, dtype=BF16)
    libfk.check(libfk.load().fk_softmax_rows(_ptr(x), x.stride(0), _ptr(out), out.stride(0), rows, n,
                                             _stream()), "fk_softmax_rows")
    return out



# ---- fp32-class VAE encoder (include/fk.h "fp32-class encoder"; reference train_denoiser.py:458,887-918) ---------------
F32 = torch.float32


def split_f32_rows(x, out, parts=3, weight_order=False):
    """fp32 [rows, n] view -> bf16 parts in ``out`` [rows, parts * n]-like view: part p of x[r, c] at out[r, p*ps + c] with
    ps = out.shape[1] // parts.  Order (hi, lo, hi), or (hi, hi, lo) for the weight side of a product."""
    _need_cuda(x, out)
    rows, n = x.shape
    ps = out.shape[1] // parts
    if x.dtype != F32 or out.dtype != BF16 or out.shape[0] != rows or ps < n or x.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("split_f32_rows: fp32 [rows, n] -> bf16 [rows, parts * ps], ps >= n")
    libfk.check(libfk.load().fk_split_f32_rows(_ptr(x), x.stride(0), _ptr(out), out.stride(0), ps, rows, n, parts,
                                               int(weight_order), _stream()), "fk_split_f32_rows")
    return out


def group_norm_f32_parts(x, gamma, beta, silu, parts, eps=1e-6):
    """GroupNorm(32) (+ SiLU) of fp32 NHWC x (fp32 gamma / beta) -> bf16 parts [B, ..., parts * C]."""
    _need_cuda(x, gamma, beta)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    if x.dtype != F32 or gamma.dtype != F32 or beta.dtype != F32 or not x.is_contiguous():
        raise TypeError("group_norm_f32_parts takes contiguous fp32 tensors")
    lib = libfk.load()
    ws, stats = _gn_workspace(lib, B, HW, C, x.device)
    out = torch.empty((*x.shape[:-1], parts * C), device=x.device, dtype=BF16)
    libfk.check(lib.fk_groupnorm_f32_nhwc(_ptr(x), _ptr(out), _ptr(stats), _ptr(ws), _ptr(gamma), _ptr(beta), B, HW, C, 32,
                                          eps, int(silu), parts, _stream()), "fk_groupnorm_f32_nhwc")
    return out


def conv2d_nhwc_f32out(x_parts, w_packed, bias, cout, ksize=3, stride=1, pad=1, res=None, halo=False):
    """x_parts: [B,H,W,parts*C] bf16 operand parts; w_packed [cout, Kpad] bf16 over the same channel layout; bias / res /
    result fp32.  ``halo=True`` (3 x 3, stride 1, pad 1, parts*C % 64 == 0): the LDS halo-tiled kernel instead of the
    implicit GEMM."""
    _need_cuda(x_parts, w_packed, bias, res)
    B, Hin, Win, Cin = x_parts.shape
    if stride == 1:
        Hout, Wout = Hin, Win
    else:
        Hout, Wout = (Hin + 1 - 3) // 2 + 1, (Win + 1 - 3) // 2 + 1
    if x_parts.dtype != BF16 or bias.dtype != F32 or (res is not None and (res.dtype != F32 or not res.is_contiguous())) \
            or not x_parts.is_contiguous():
        raise TypeError("conv2d_nhwc_f32out: bf16 parts in, fp32 bias / residual")
    out = torch.empty((B, Hout, Wout, cout), device=x_parts.device, dtype=F32)
    a = libfk.ConvArgs()
    a.x, a.w, a.bias, a.y = x_parts.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr()
    a.res = res.data_ptr() if res is not None else None
    a.B, a.Hin, a.Win, a.Cin, a.Cout = B, Hin, Win, Cin, cout
    a.ksize, a.stride, a.pad, a.upsample2x = ksize, stride, pad, 0
    a.Hout, a.Wout = Hout, Wout
    if halo:
        libfk.check(libfk.load().fk_conv3x3_halo_f32out(ctypes.byref(a), _stream()), "fk_conv3x3_halo_f32out")
    else:
        libfk.check(libfk.load().fk_conv2d_nhwc_f32out(ctypes.byref(a), _stream()), "fk_conv2d_nhwc_f32out")
    return out


def nchw_f32_to_nhwc_parts(x, cpad, parts):
    _need_cuda(x)
    B, C, H, W = x.shape
    if x.dtype != F32 or not x.is_contiguous():
        raise TypeError("nchw_f32_to_nhwc_parts takes contiguous fp32 NCHW")
    out = torch.empty((B, H, W, parts * cpad), device=x.device, dtype=BF16)
    libfk.check(libfk.load().fk_nchw_f32_to_nhwc_parts(_ptr(x), _ptr(out), B, C, cpad, H, W, parts, _stream()),
                "fk_nchw_f32_to_nhwc_parts")
    return out


def nhwc_f32_to_nchw(x, c, add=0.0, mul=1.0):
    _need_cuda(x)
    B, H, W, cpad = x.shape
    if x.dtype != F32 or not x.is_contiguous():
        raise TypeError("nhwc_f32_to_nchw takes contiguous fp32 NHWC")
    out = torch.empty((B, c, H, W), device=x.device, dtype=F32)
    libfk.check(libfk.load().fk_nhwc_f32_to_nchw(_ptr(x), _ptr(out), B, c, cpad, H, W, float(add), float(mul), _stream()),
                "fk_nhwc_f32_to_nchw")
    return out


def softmax_rows_parts(x, out):
    """fp32 [rows, n] -> the bf16 parts (hi, lo, hi) of the fp32 softmax in ``out`` [rows, 3 * ps]."""
    _need_cuda(x, out)
    rows, n = x.shape
    ps = out.shape[1] // 3
    libfk.check(libfk.load().fk_softmax_rows_parts(_ptr(x), x.stride(0), _ptr(out), out.stride(0), ps, rows, n, _stream()),
                "fk_softmax_rows_parts")
    return out


# ---- backward pass of the MMDiT (include/fk.h "backward pass"; reference: autograd, train_denoiser.py:1172) -----------
_BWD_WS = {}


def bwd_workspace(device):
    """fp32 scratch of the two-stage reductions (one per device; kernels on one stream are ordered)."""
    key = str(device)
    ws = _BWD_WS.get(key)
    if ws is None:
        ws = torch.empty(libfk.load().fk_bwd_ws_floats(), device=device, dtype=torch.float32)
        _BWD_WS[key] = ws
    return ws


def attn_view(t, head_major):
    """fk_attn_view of a bf16 tensor: head-major [B,H,S,128] (contiguous rows) or token-major [B,S,H*128] view."""
    v = libfk.AttnView()
    v.p = t.data_ptr()
    if head_major:
        if t.dim() != 4 or t.shape[3] != 128 or t.stride(3) != 1:
            raise ValueError("head-major view must be [B,H,S,128] with a contiguous last dimension")
        v.ld, v.head_stride, v.batch_stride = t.stride(2), t.stride(1), t.stride(0)
    else:
        if t.dim() != 3 or t.stride(2) != 1:
            raise ValueError("token-major view must be [B,S,H*128] with a contiguous last dimension")
        v.ld, v.head_stride, v.batch_stride = t.stride(1), 128, t.stride(0)
    return v


def attention_lse(q, k, v, out, lse, scale=None, key_mask=None):
    """:func:`attention` that also writes lse [B,H,S] fp32 (log2 domain) for :func:`attention_bwd`."""
    if lse is None:
        raise ValueError("attention_lse needs an lse tensor")
    return attention(q, k, v, out, scale=scale, lse=lse, key_mask=key_mask)


def rowdot(a, c, heads, out=None):
    """out[b,h,s] = sum_d a[b,s,h*128+d] * c[b,s,h*128+d]; a, c: [B,S,heads*128] views."""
    _need_cuda(a, c)
    B, S, _ = a.shape
    if out is None:
        out = torch.empty((B, heads, S), device=a.device, dtype=torch.float32)
    libfk.check(libfk.load().fk_rowdot_bf16(_ptr(a), a.stride(1), a.stride(0), _ptr(c), c.stride(1), c.stride(0), _ptr(out),
                                            B, S, heads, _stream()), "fk_rowdot_bf16")
    return out


def attention_bwd_set_mode(mode):
    """`passes` of fk_attention_bwd_ws_bf16: 1 = dQ pass + paired dK / dV pass (default), 0 = three passes."""
    if int(mode) not in (0, 1):
        raise ValueError(f"attention_bwd_set_mode: {mode} is not 0 (three passes) or 1 (dQ pass + paired dK / dV pass)")
    _set_launch(attn_bwd_passes=0 if int(mode) else 3)


def attention_bwd(q, k, v, dout, lse, dsum, dq, dk, dv, scale=None, key_mask=None):
    """dq, dk [B,H,S,128] and dv ([B,S,H*128] view) of softmax(q k^T scale) v given dout ([B,S,H*128] view), lse, dsum.
    key_mask: the :func:`pack_key_mask` tensor the forward ran with (fk_attention_bwd_masked_bf16: plain grids; dk / dv rows
    of masked keys are written as zeros)."""
    _need_cuda(q, k, v, dout, lse, dsum, dq, dk, dv, key_mask)
    B, H, S, hd = q.shape
    views = [attn_view(q, True), attn_view(k, True), attn_view(v, False), attn_view(dout, False),
             attn_view(dq, True), attn_view(dk, True), attn_view(dv, False)]
    r = [ctypes.byref(x) for x in views]
    if key_mask is not None:
        _check_key_mask(key_mask, B, S)
        libfk.check(libfk.load().fk_attention_bwd_masked_bf16(r[0], r[1], r[2], r[3], _ptr(lse), _ptr(dsum), r[4], r[5], r[6],
                                                             _ptr(key_mask), B, H, S, hd ** -0.5 if scale is None else scale,
                                                             LAUNCH.attn_bwd_passes, _stream()), "fk_attention_bwd_masked_bf16")
        return
    ws = attention_workspace(q.device)      # the forward's stream-K workspace: the dQ pass uses the same scheme
    libfk.check(libfk.load().fk_attention_bwd_ws_bf16(r[0], r[1], r[2], r[3], _ptr(lse), _ptr(dsum), r[4], r[5], r[6], B, H, S,
                                                     hd ** -0.5 if scale is None else scale, _ptr(ws), ws.numel(), LAUNCH.attn_grid,
                                                     LAUNCH.attn_bwd_passes, _stream()),
                "fk_attention_bwd_bf16")


def ln_modulate_bwd(x, dn, scale, dx_out, dmod_shift, dx_in=None, eps=1e-6):
    """Adjoint of :func:`ln_modulate` for one stream view x / dn / dx [B,R,D]; scale: [B,D] view of the modulation
    vector; dmod_shift: fp32 [B, >=2D] view whose columns [0,D) receive dshift and [D,2D) dscale."""
    _need_cuda(x, dn, scale, dx_out, dmod_shift, dx_in)
    B, R, D = x.shape
    M, rx = rows_of(x)
    _, rg = rows_of(dn)
    _, ro = rows_of(dx_out)
    ri = rows_of(dx_in)[1] if dx_in is not None else Rows(0, 0, 0)
    if dmod_shift.dtype != torch.float32 or dmod_shift.stride(1) != 1 or dmod_shift.shape[1] < 2 * D:
        raise ValueError("dmod_shift must be an fp32 [B, >= 2D] view")
    base = dmod_shift.data_ptr()
    libfk.check(libfk.load().fk_ln_modulate_bwd_bf16(_ptr(x), rx, _ptr(dn), rg, _ptr(scale), scale.stride(0), R, _ptr(dx_in), ri,
                                                    _ptr(dx_out), ro, ctypes.c_void_p(base), ctypes.c_void_p(base + 4 * D),
                                                    dmod_shift.stride(0), _ptr(bwd_workspace(x.device)), B, D, eps, _stream()),
                "fk_ln_modulate_bwd_bf16")
    return dx_out


def gate_res_bwd(dout, y, gate, dy, dgate):
    """dy = dout * gate[b]; dgate[b] = sum_s dout * y.  dout / y / dy: [B,R,N] views; gate: [B,N] view; dgate fp32 [B,N] view."""
    _need_cuda(dout, y, gate, dy, dgate)
    B, R, N = dout.shape
    _, r0 = rows_of(dout)
    _, r1 = rows_of(y)
    _, r2 = rows_of(dy)
    libfk.check(libfk.load().fk_gate_res_bwd_bf16(_ptr(dout), r0, _ptr(y), r1, _ptr(gate), gate.stride(0), R, _ptr(dy), r2,
                                                 _ptr(dgate), dgate.stride(0), _ptr(bwd_workspace(dout.device)), B, N, _stream()),
                "fk_gate_res_bwd_bf16")
    return dy


def gelu_bwd(h, df, out=None):
    """out = df * gelu_tanh'(h) (contiguous tensors of one shape)."""
    _need_cuda(h, df)
    if not (h.is_contiguous() and df.is_contiguous()):
        raise ValueError("gelu_bwd takes contiguous tensors")
    if out is None:
        out = torch.empty_like(df)
    libfk.check(libfk.load().fk_gelu_bwd_bf16(_ptr(h), _ptr(df), _ptr(out), h.numel(), _stream()), "fk_gelu_bwd_bf16")
    return out


def silu_bwd(h, df, out=None):
    """out = df * silu'(h) (contiguous tensors of one shape)."""
    _need_cuda(h, df)
    if not (h.is_contiguous() and df.is_contiguous()):
        raise ValueError("silu_bwd takes contiguous tensors")
    if out is None:
        out = torch.empty_like(df)
    libfk.check(libfk.load().fk_silu_bwd_bf16(_ptr(h), _ptr(df), _ptr(out), h.numel(), _stream()), "fk_silu_bwd_bf16")
    return out


def qkv_post_bwd(dq, dk, qkv, dqkv, wq_img, wk_img, wq_txt, wk_txt, cos, sin, s_txt, eps=1e-6):
    """Adjoint of :func:`qkv_post`; returns dw fp32 [2 (q,k)][2 (image,text)][128]."""
    _need_cuda(dq, dk, qkv, dqkv, cos, sin)
    B, S, D3 = qkv.shape
    H = D3 // 384
    if not (qkv.is_contiguous() and dqkv.is_contiguous() and dq.is_contiguous() and dk.is_contiguous()):
        raise ValueError("qkv_post_bwd takes contiguous tensors")
    dw = torch.empty((2, 2, 128), device=qkv.device, dtype=torch.float32)
    libfk.check(libfk.load().fk_qkv_post_bwd_bf16(_ptr(dq), _ptr(dk), _ptr(qkv), _ptr(dqkv), _ptr(wq_img), _ptr(wk_img),
                                                 _ptr(wq_txt), _ptr(wk_txt), _ptr(cos), _ptr(sin), _ptr(dw),
                                                 _ptr(bwd_workspace(qkv.device)), B, S, s_txt, H, eps, _stream()),
                "fk_qkv_post_bwd_bf16")
    return dw


def gate_res_fwd(res, y, gate, out):
    """out = res + gate[b] * y with the fused epilogue's rounding; res / y / out: [B,R,N] views, gate: [B,N] view."""
    _need_cuda(res, y, gate, out)
    B, R, N = y.shape
    M, r1 = rows_of(y)
    _, r0 = rows_of(res)
    _, r2 = rows_of(out)
    libfk.check(libfk.load().fk_gate_res_fwd_bf16(_ptr(res), r0, _ptr(y), r1, _ptr(gate), gate.stride(0), R, _ptr(out), r2, M, N,
                                                 _stream()), "fk_gate_res_fwd_bf16")
    return out


def gelu_tanh(x, out):
    """out = gelu_tanh(x) (bf16, the GEMM epilogue's function); x / out: [M,N] or [B,R,N] views."""
    _need_cuda(x, out)
    M, r0 = rows_of(x)
    _, r1 = rows_of(out)
    libfk.check(libfk.load().fk_gelu_tanh_bf16(_ptr(x), r0, _ptr(out), r1, M, x.shape[-1], _stream()), "fk_gelu_tanh_bf16")
    return out


def f32_to_bf16_transposed(src, dst):
    """dst[c, r] = bf16(src[r, c]) for an fp32 [R,C] view and a bf16 [C, ld >= R] buffer (extra columns zeroed)."""
    _need_cuda(src, dst)
    R, C = src.shape
    if src.dtype != torch.float32 or src.stride(1) != 1 or dst.dtype != BF16 or not dst.is_contiguous() or dst.shape[0] != C:
        raise ValueError("f32_to_bf16_transposed: fp32 [R,C] view -> contiguous bf16 [C, ld]")
    libfk.check(libfk.load().fk_f32_to_bf16_transposed(_ptr(src), src.stride(0), _ptr(dst), dst.shape[1], R, C, _stream()),
                "fk_f32_to_bf16_transposed")
    return dst


def colsum(x, out=None):
    """fp32 [N] = sum over the rows of a [M,N] / [B,R,N] view (bias gradients)."""
    _need_cuda(x)
    M, rx = rows_of(x)
    N = x.shape[-1]
    if out is None:
        out = torch.empty(N, device=x.device, dtype=torch.float32)
    libfk.check(libfk.load().fk_colsum_bf16(_ptr(x), rx, M, N, _ptr(out), _ptr(bwd_workspace(x.device)), _stream()),
                "fk_colsum_bf16")
    return out


# ---- FLUX AutoencoderKL pieces (NHWC bf16 activations) -------------------------------------------------
def conv2d_nhwc(x, w_packed, bias, cout, ksize=3, stride=1, pad=1, upsample2x=False, res=None, out=None):
    """x: [B,H,W,Cin] bf16; w_packed: [cout, Kpad] (k = (kh*ks+kw)*Cin + ci, zero padded to 64)."""
    _need_cuda(x, w_packed, bias, res)
    B, Hin, Win, Cin = x.shape
    He, We = (Hin * 2, Win * 2) if upsample2x else (Hin, Win)
    if stride == 1:
        Hout, Wout = He, We
    else:  # F.pad(x, (0,1,0,1)) + 3x3 stride-2 valid conv
        Hout, Wout = (He + 1 - 3) // 2 + 1, (We + 1 - 3) // 2 + 1
    if out is None:
        out = torch.empty((B, Hout, Wout, cout), device=x.device, dtype=BF16)
    a = libfk.ConvArgs()
    a.x, a.w, a.bias, a.y = x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr()
    a.res = res.data_ptr() if res is not None else None
    a.B, a.Hin, a.Win, a.Cin, a.Cout = B, Hin, Win, Cin, cout
    a.ksize, a.stride, a.pad, a.upsample2x = ksize, stride, pad, int(upsample2x)
    a.Hout, a.Wout = Hout, Wout
    if not x.is_contiguous() or (res is not None and not res.is_contiguous()):
        raise ValueError("conv2d_nhwc needs contiguous NHWC tensors")
    libfk.check(libfk.load().fk_conv2d_nhwc_bf16(ctypes.byref(a), _stream()), "fk_conv2d_nhwc_bf16")
    return out


_GN_WS = {}


def _gn_workspace(lib, B, HW, C, device):
    """Partial-sum workspace + statistics of one GroupNorm shape, allocated once per (device, shape): calls on one
    stream are ordered, so consecutive GroupNorms may share it."""
    key = (str(device), B, HW, C)
    hit = _GN_WS.get(key)
    if hit is None:
        if len(_GN_WS) > 64:
            _GN_WS.clear()
        hit = (torch.empty(lib.fk_groupnorm_ws_floats(B, HW, C), device=device, dtype=torch.float32),
               torch.empty((B, 32, 2), device=device, dtype=torch.float32))
        _GN_WS[key] = hit
    return hit


def group_norm_stats(x, eps=1e-6):
    """(mean, rstd) fp32 [B, 32, 2] of GroupNorm(32) over [B, ..., C] NHWC bf16.  The buffer is shared by every call of
    one shape on the device: consume it (``group_norm_nhwc`` / ``conv3x3_halo(gn=...)``) before the next call."""
    _need_cuda(x)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    lib = libfk.load()
    ws, stats = _gn_workspace(lib, B, HW, C, x.device)
    libfk.check(lib.fk_groupnorm_stats_nhwc_bf16(_ptr(x), _ptr(stats), _ptr(ws), B, HW, C, 32, eps, _stream()),
                "fk_groupnorm_stats_nhwc_bf16")
    return stats


def conv3x3_halo(x, w_packed, bias, cout, upsample2x=False, res=None, gn=None, out=None, out_fp32=False):
    """3 x 3 / stride 1 / pad 1 convolution over NHWC bf16 by the LDS halo-tiled kernel (csrc/conv_halo.hip), optionally
    with GroupNorm(32) (+ SiLU) of the INPUT applied while the halo tile is staged: ``gn = (stats, gamma, beta, silu)``
    with ``stats`` from :func:`group_norm_stats`.  Cin % 64 == 0."""
    _need_cuda(x, w_packed, bias, res)
    B, Hin, Win, Cin = x.shape
    Hout, Wout = (Hin * 2, Win * 2) if upsample2x else (Hin, Win)
    if out is None:
        out = torch.empty((B, Hout, Wout, cout), device=x.device, dtype=torch.float32 if out_fp32 else BF16)
    if out.dtype != (torch.float32 if out_fp32 else BF16) or not out.is_contiguous():
        raise TypeError("conv3x3_halo: out must be a contiguous bf16 tensor (fp32 with out_fp32: the parity build)")
    if not x.is_contiguous() or (res is not None and not res.is_contiguous()):
        raise ValueError("conv3x3_halo needs contiguous NHWC tensors")
    a = libfk.ConvArgs()
    a.x, a.w, a.bias, a.y = x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), out.data_ptr()
    a.res = res.data_ptr() if res is not None else None
    a.B, a.Hin, a.Win, a.Cin, a.Cout = B, Hin, Win, Cin, cout
    a.ksize, a.stride, a.pad, a.upsample2x = 3, 1, 1, int(upsample2x)
    a.Hout, a.Wout = Hout, Wout
    stats, gamma, beta, silu = gn if gn is not None else (None, None, None, False)
    _need_cuda(stats, gamma, beta)
    fn = libfk.load().fk_conv3x3_halo_f32_debug if out_fp32 else libfk.load().fk_conv3x3_halo_bf16
    libfk.check(fn(ctypes.byref(a), _ptr(stats), _ptr(gamma), _ptr(beta), 32, int(bool(silu)), _stream()), "fk_conv3x3_halo_bf16")
    return out


def group_norm_nhwc(x, gamma, beta, silu, eps=1e-6, out=None):
    """GroupNorm(32) (+SiLU) over [B, ..., C] NHWC bf16."""
    _need_cuda(x, gamma, beta)
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    lib = libfk.load()
    stats = group_norm_stats(x, eps)
    if out is None:
        out = torch.empty_like(x)
    libfk.check(lib.fk_groupnorm_apply_nhwc_bf16(_ptr(x), _ptr(out), _ptr(stats), _ptr(gamma), _ptr(beta), B, HW,
                                                 C, 32, int(silu), _stream()), "fk_groupnorm_apply_nhwc_bf16")
    return out


def nchw_to_nhwc(x, cpad, div=1.0, add=0.0):
    _need_cuda(x)
    B, C, H, W = x.shape
    if x.dtype not in (BF16, torch.float32) or not x.is_contiguous():
        raise TypeError("nchw_to_nhwc takes contiguous fp32/bf16 NCHW")
    out = torch.empty((B, H, W, cpad), device=x.device, dtype=BF16)
    libfk.check(libfk.load().fk_nchw_to_nhwc_bf16(_ptr(x), int(x.dtype == torch.float32), _ptr(out), B, C, cpad,
                                                  H, W, float(div), float(add), _stream()), "fk_nchw_to_nhwc_bf16")
    return out


def nhwc_to_nchw(x, c, add=0.0, mul=1.0, dtype=BF16):
    _need_cuda(x)
    B, H, W, cpad = x.shape
    out = torch.empty((B, c, H, W), device=x.device, dtype=dtype)
    libfk.check(libfk.load().fk_nhwc_to_nchw(_ptr(x), _ptr(out), int(dtype == torch.float32), B, c, cpad, H, W,
                                             float(add), float(mul), _stream()), "fk_nhwc_to_nchw")
    return out


def pixels_to_nhwc(u8, out_h, out_w, cpad=32, renorm=False):
    """uint8 NHWC pixels [B,Hin,Win,3] -> NHWC bf16 [B,out_h,out_w,cpad] in [-1,1]: cli.py:106-109 normalisation,
    VaeImageProcessor tensor resize (nearest) and the bf16 cast, one gather kernel."""
    _need_cuda(u8)
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3 or not u8.is_contiguous():
        raise TypeError("pixels_to_nhwc takes a contiguous uint8 [B, H, W, 3] tensor")
    B, Hin, Win, _ = u8.shape
    out = torch.empty((B, out_h, out_w, cpad), device=u8.device, dtype=BF16)
    libfk.check(libfk.load().fk_pixels_u8_to_nhwc_bf16(_ptr(u8), _ptr(out), B, Hin, Win, out_h, out_w, cpad,
                                                       int(bool(renorm)), _stream()), "fk_pixels_u8_to_nhwc_bf16")
    return out


def image_to_u8(img):
    """decoder output [B,C,H,W] (bf16/fp32, [-1,1]) -> uint8 [B,H,W,C] (VaeImageProcessor.postprocess, 'pil' array)."""
    _need_cuda(img)
    if img.dtype not in (BF16, torch.float32) or img.dim() != 4 or not img.is_contiguous():
        raise TypeError("image_to_u8 takes a contiguous fp32/bf16 NCHW tensor")
    B, C, H, W = img.shape
    out = torch.empty((B, H, W, C), device=img.device, dtype=torch.uint8)
    libfk.check(libfk.load().fk_image_to_u8_nhwc(_ptr(img), int(img.dtype == torch.float32), _ptr(out), B, C, H, W,
                                                 _stream()), "fk_image_to_u8_nhwc")
    return out


# ---- masked edits on the masked box (include/fk.h: fk_mask_bbox_u8, fk_mask_blur_u8, fk_pixels_u8_box_to_nhwc_bf16,
# fk_image_overlay_u8) -----------------------------------------------------------------------------------------------
def _mask_u8(mask, what):
    _need_cuda(mask)
    if mask.dtype != torch.uint8 or mask.dim() != 3 or not mask.is_contiguous():
        raise TypeError(f"{what} takes a contiguous uint8 [Bm, H, W] mask")
    return mask.shape


def _box(box):
    x0, y0, x1, y1 = (int(v) for v in box)
    return x0, y0, x1, y1


def mask_bbox(mask_u8, threshold=1, out=None, ws=None):
    """int32 [4] on the device: (min x, min y, max x + 1, max y + 1) over all samples of the pixels with byte >= ``threshold``;
    (W, H, 0, 0) when there are none.  ``ws``: the partials workspace (allocated per call when None)."""
    Bm, H, W = _mask_u8(mask_u8, "mask_bbox")
    lib = libfk.load()
    if out is None:
        out = torch.empty(4, device=mask_u8.device, dtype=torch.int32)
    if ws is None:
        ws = torch.empty(lib.fk_mask_bbox_ws_ints(), device=mask_u8.device, dtype=torch.int32)
    _need_cuda(out, ws)
    if out.dtype != torch.int32 or out.numel() < 4 or not out.is_contiguous() or ws.dtype != torch.int32 or not ws.is_contiguous():
        raise ValueError("out must be int32 [4], ws a contiguous int32 workspace")
    libfk.check(lib.fk_mask_bbox_u8(_ptr(mask_u8), Bm, H, W, int(threshold), _ptr(out), _ptr(ws), ws.numel(), _stream()),
                "fk_mask_bbox_u8")
    return out


def mask_blur(mask_u8, sigma, out=None):
    """The mask feathered with a separable Gaussian of ``sigma`` pixels (taps: ``helpers.gaussian_taps``), uint8 [Bm, H, W]."""
    Bm, H, W = _mask_u8(mask_u8, "mask_blur")
    taps = helpers.gaussian_taps(sigma).to(mask_u8.device)
    plane = torch.empty((Bm, H, W), device=mask_u8.device, dtype=torch.float32)
    if out is None:
        out = torch.empty_like(mask_u8)
    _mask_u8(out, "mask_blur")
    if out.shape != mask_u8.shape:
        raise ValueError("out must have the mask's shape")
    libfk.check(libfk.load().fk_mask_blur_u8(_ptr(mask_u8), _ptr(out), _ptr(plane), _ptr(taps), (taps.numel() - 1) // 2, Bm, H, W,
                                             _stream()), "fk_mask_blur_u8")
    return out


def pixels_box_to_nhwc(u8, box, out_h, out_w, cpad=32, renorm=False, out=None):
    """:func:`pixels_to_nhwc` reading the source box ``(x0, y0, x1, y1)`` with bilinear weights (half-pixel centres)."""
    _need_cuda(u8, out)
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3 or not u8.is_contiguous():
        raise TypeError("pixels_box_to_nhwc takes a contiguous uint8 [B, H, W, 3] tensor")
    B, Hin, Win, _ = u8.shape
    if out is None:
        out = torch.empty((B, out_h, out_w, cpad), device=u8.device, dtype=BF16)
    if out.dtype != BF16 or tuple(out.shape) != (B, out_h, out_w, cpad) or not out.is_contiguous():
        raise ValueError("out must be a contiguous bf16 [B, out_h, out_w, cpad] tensor")
    libfk.check(libfk.load().fk_pixels_u8_box_to_nhwc_bf16(_ptr(u8), _ptr(out), B, Hin, Win, *_box(box), out_h, out_w, cpad,
                                                           int(bool(renorm)), _stream()), "fk_pixels_u8_box_to_nhwc_bf16")
    return out


def image_overlay(img, orig_u8, alpha_u8, box, out=None):
    """Decoder output [B,3,h,w] (bf16/fp32) resampled into ``box`` of the original picture uint8 [1 or B,H,W,3] and blended
    over its bytes with ``alpha_u8`` (uint8 [1 or B,H,W], None = 255 everywhere) -> uint8 [B,H,W,3]."""
    _need_cuda(img, orig_u8, alpha_u8, out)
    if img.dtype not in (BF16, torch.float32) or img.dim() != 4 or img.shape[1] != 3 or not img.is_contiguous():
        raise TypeError("image_overlay takes a contiguous fp32/bf16 [B, 3, h, w] tensor")
    if orig_u8.dtype != torch.uint8 or orig_u8.dim() != 4 or orig_u8.shape[3] != 3 or not orig_u8.is_contiguous():
        raise TypeError("image_overlay takes the original as a contiguous uint8 [1 or B, H, W, 3] tensor")
    B, _, h, w = img.shape
    N, H, W, _ = orig_u8.shape
    Bm = 0
    if alpha_u8 is not None:
        Bm, Ha, Wa = _mask_u8(alpha_u8, "image_overlay")
        if (Ha, Wa) != (H, W):
            raise ValueError(f"alpha is {Ha} x {Wa}, the original {H} x {W}")
    if out is None:
        out = torch.empty((B, H, W, 3), device=img.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 [B, H, W, 3] tensor")
    libfk.check(libfk.load().fk_image_overlay_u8(_ptr(img), int(img.dtype == torch.float32), h, w, _ptr(orig_u8), N,
                                                 _ptr(alpha_u8), Bm, _ptr(out), B, H, W, *_box(box), _stream()),
                "fk_image_overlay_u8")
    return out


# ---- edit-region loss weights (include/fk.h: fk_edit_diff_mask_u8 .. fk_mask_weight_fill_f32; edit_weights.py) -----------------------
def edit_diff_mask(ref_u8, tgt_u8, threshold=18, out=None):
    """255 where Pillow's grey of |ref - tgt| is >= ``threshold``: uint8 NHWC RGB [N, H, W, 3] twice -> uint8 [N, H, W].  The
    reference may be a view whose pictures are contiguous and lie any number of bytes apart (``refs[:, r]`` of [B, R, H, W, 3])."""
    _need_cuda(ref_u8, tgt_u8, out)
    for t in (ref_u8, tgt_u8):
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or not (t.is_contiguous() or (t is ref_u8 and t[0].is_contiguous())):
            raise TypeError("edit_diff_mask takes contiguous uint8 [N, H, W, 3] tensors (the reference: contiguous pictures)")
    if ref_u8.shape != tgt_u8.shape:
        raise ValueError(f"edit_diff_mask: the reference is {tuple(ref_u8.shape)}, the target {tuple(tgt_u8.shape)}")
    N, H, W, _ = ref_u8.shape
    if out is None:
        out = torch.empty((N, H, W), device=ref_u8.device, dtype=torch.uint8)
    _mask_u8(out, "edit_diff_mask")
    if tuple(out.shape) != (N, H, W):
        raise ValueError("out must have the pictures' [N, H, W]")
    ref_bs = ref_u8.stride(0) if N > 1 else H * W * 3
    libfk.check(libfk.load().fk_edit_diff_mask_u8(_ptr(ref_u8), ref_bs, _ptr(tgt_u8), _ptr(out), N, H, W, int(threshold), _stream()),
                "fk_edit_diff_mask_u8")
    return out


def mask_close5(mask, out=None):
    """Closing (dilation, then erosion) with the 5 x 5 ellipse; the outside of the plane is never counted."""
    N, H, W = _mask_u8(mask, "mask_close5")
    if out is None:
        out = torch.empty_like(mask)
    _mask_u8(out, "mask_close5")
    if out.shape != mask.shape:
        raise ValueError("out must have the mask's shape")
    libfk.check(libfk.load().fk_mask_close5_u8(_ptr(mask), _ptr(out), N, H, W, _stream()), "fk_mask_close5_u8")
    return out


def mask_components_ws(N, H, W, device):
    """The labelling workspace of :func:`mask_filter_components` (int32; word 0 is its status)."""
    nbytes = libfk.load().fk_mask_components_ws_bytes(N, H, W)
    return torch.empty(max(nbytes, 4) // 4, device=device, dtype=torch.int32)


def mask_filter_components(mask, keep_num=3, keep_den=10, out=None, ws=None, check=True):
    """Keeps the 8-connected components with ``keep_den * area >= keep_num * white pixels of the plane``.  ``check``: wait for the
    stream and raise when a labelling loop reached its bound (FK_EBOUND); without it the caller hands ``ws`` to
    :func:`mask_and_pool8`, whose counts carry the status."""
    N, H, W = _mask_u8(mask, "mask_filter_components")
    lib = libfk.load()
    if out is None:
        out = torch.empty_like(mask)
    _mask_u8(out, "mask_filter_components")
    if out.shape != mask.shape:
        raise ValueError("out must have the mask's shape")
    if ws is None:
        ws = mask_components_ws(N, H, W, mask.device)
    _need_cuda(ws)
    if ws.dtype != torch.int32 or not ws.is_contiguous():
        raise ValueError("ws must be a contiguous int32 workspace")
    libfk.check(lib.fk_mask_filter_components_u8(_ptr(mask), _ptr(out), N, H, W, int(keep_num), int(keep_den), _ptr(ws),
                                                 ws.numel() * 4, _stream()), "fk_mask_filter_components_u8")
    if check:
        libfk.check(lib.fk_mask_components_status(_ptr(ws), _stream()), "fk_mask_components_status")
    return out


def mask_and_pool8(masks, status=None, out=None):
    """uint8 [B, R, H, W] -> (mask_ds uint8 [B, H // 8, W // 8], counts int32 [B, 2]): AND over R, counts[:, 0] its white pixels,
    the all-white plane where that is 0, 8 x 8 max pool, :func:`mask_close5`, counts[:, 1] the white pixels of mask_ds.
    ``status``: the workspace of :func:`mask_filter_components`; a labelling that reached a bound turns every count into -1.
    ``out``: (pooled, mask_ds, counts), the three buffers the stage writes (allocated per call when None)."""
    _need_cuda(masks, status)
    if masks.dtype != torch.uint8 or masks.dim() != 4 or not masks.is_contiguous():
        raise TypeError("mask_and_pool8 takes a contiguous uint8 [B, R, H, W] tensor")
    B, R, H, W = masks.shape
    if out is None:
        out = (torch.empty((B, H // 8, W // 8), device=masks.device, dtype=torch.uint8),
               torch.empty((B, H // 8, W // 8), device=masks.device, dtype=torch.uint8),
               torch.empty((B, 2), device=masks.device, dtype=torch.int32))
    pooled, mask_ds, counts = out
    _need_cuda(pooled, mask_ds, counts)
    for t, shape, dtype in ((pooled, (B, H // 8, W // 8), torch.uint8), (mask_ds, (B, H // 8, W // 8), torch.uint8),
                            (counts, (B, 2), torch.int32)):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"out must be (pooled, mask_ds, counts): contiguous uint8 {(B, H // 8, W // 8)} twice and int32 {(B, 2)}")
    libfk.check(libfk.load().fk_mask_and_pool8_u8(_ptr(masks), B, R, H, W, _ptr(pooled), _ptr(mask_ds), _ptr(counts), _ptr(status),
                                                  _stream()), "fk_mask_and_pool8_u8")
    return mask_ds, counts


def mask_weight_fill(mask_ds, w, out=None):
    """fp32 [B, 1, h, w]: ``w[b]`` where ``mask_ds`` [B, h, w] is white, 1.0 elsewhere."""
    B, h, wd = _mask_u8(mask_ds, "mask_weight_fill")
    _need_cuda(w, out)
    if w.dtype != torch.float32 or tuple(w.shape) != (B,) or not w.is_contiguous():
        raise TypeError("mask_weight_fill takes the weights as a contiguous fp32 [B] tensor")
    if out is None:
        out = torch.empty((B, 1, h, wd), device=mask_ds.device, dtype=torch.float32)
    if out.dtype != torch.float32 or tuple(out.shape) != (B, 1, h, wd) or not out.is_contiguous():
        raise ValueError("out must be a contiguous fp32 [B, 1, h, w] tensor")
    libfk.check(libfk.load().fk_mask_weight_fill_f32(_ptr(mask_ds), _ptr(w), _ptr(out), B, h, wd, _stream()),
                "fk_mask_weight_fill_f32")
    return out


# ---- antialiased byte resize and byte paste-back (include/fk.h: fk_resample_pass_u8, fk_bytes_overlay_u8) ---------------------------
_resample_tables = {}       # (n_in, n_out, filter, device, axis) -> (bounds, kk) on the device, kk tap-major for axis 1


def _resample_device_tables(n_in, n_out, filter, device, axis):
    key = (n_in, n_out, filter, str(device), axis)
    if key not in _resample_tables:
        bounds, kk, ksize = helpers.resample_coeffs(n_in, n_out, filter)
        kk = kk.t().contiguous() if axis == 1 else kk
        _resample_tables[key] = (bounds.to(device), kk.to(device), ksize)
    return _resample_tables[key]


def resample_pass_u8(src_view, axis, n_out, filter, out=None):
    """One pass of :func:`resample_u8` along ``axis`` (1: horizontal, 0: vertical) of a uint8 view [B, H, W, C]."""
    _need_cuda(src_view, out)
    if (src_view.dtype != torch.uint8 or src_view.dim() != 4 or src_view.shape[3] not in (1, 3) or src_view.stride(3) != 1
            or src_view.stride(2) != src_view.shape[3]):
        raise TypeError("resample_u8 takes a uint8 [B, H, W, C] view, C 1 or 3, whose pixels are contiguous within a row")
    if axis not in (0, 1):
        raise ValueError(f"axis is 0 (vertical) or 1 (horizontal), not {axis!r}")
    B, H, W, C = src_view.shape
    shape = (B, H, n_out, C) if axis == 1 else (B, n_out, W, C)
    if out is None:
        out = torch.empty(shape, device=src_view.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 {shape} tensor")
    bounds, kk, ksize = _resample_device_tables(W if axis == 1 else H, n_out, filter, src_view.device, axis)
    libfk.check(libfk.load().fk_resample_pass_u8(_ptr(src_view), src_view.stride(0), src_view.stride(1), _ptr(out), B, H, W, C, axis,
                                                 n_out, _ptr(bounds), _ptr(kk), ksize, _stream()), "fk_resample_pass_u8")
    return out


def resample_u8(src_view, out_h, out_w, filter, out=None):
    """Pillow's 8-bit antialiased resize (``filter``: "bilinear" | "bicubic" | "lanczos"), byte for byte: uint8 view [B, H, W, C]
    (C 1 or 3; any row and batch stride, so a crop is the slice ``pic[:, y0:y1, x0:x1]``) -> contiguous uint8 [B, out_h, out_w, C].
    Horizontal pass into a uint8 intermediate, then the vertical pass; a pass whose axis keeps its size is skipped.  With both
    skipped and a contiguous source the source itself is returned (copied into ``out`` when one is given) and nothing is launched."""
    if filter not in helpers.RESAMPLE_FILTERS:
        raise ValueError(f"`filter` is one of {sorted(helpers.RESAMPLE_FILTERS)}, not {filter!r}")
    _need_cuda(src_view, out)
    if src_view.dtype != torch.uint8 or src_view.dim() != 4:
        raise TypeError("resample_u8 takes a uint8 [B, H, W, C] view, C 1 or 3, whose pixels are contiguous within a row")
    B, H, W, C = src_view.shape
    out_h, out_w = int(out_h), int(out_w)
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (B, out_h, out_w, C) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 {(B, out_h, out_w, C)} tensor")
    if (out_h, out_w) == (H, W):
        if out is not None:
            return out.copy_(src_view)
        return src_view if src_view.is_contiguous() else src_view.contiguous()
    x = src_view
    if out_w != W:
        x = resample_pass_u8(x, 1, out_w, filter, out=out if out_h == H else None)
    if out_h != H:
        x = resample_pass_u8(x, 0, out_h, filter, out=out)
    return x


def bytes_overlay(res, orig_u8, alpha_u8, box, out=None):
    """:func:`image_overlay` on bytes: ``res`` uint8 [B, y1-y0, x1-x0, 3] (the result already at the box's size) blended over the
    original picture uint8 [1 or B, H, W, 3] with ``alpha_u8`` (uint8 [1 or B, H, W], None = 255 everywhere) -> uint8 [B, H, W, 3]."""
    _need_cuda(res, orig_u8, alpha_u8, out)
    x0, y0, x1, y1 = _box(box)
    if res.dtype != torch.uint8 or res.dim() != 4 or res.shape[3] != 3 or not res.is_contiguous():
        raise TypeError("bytes_overlay takes the result as a contiguous uint8 [B, h, w, 3] tensor")
    if orig_u8.dtype != torch.uint8 or orig_u8.dim() != 4 or orig_u8.shape[3] != 3 or not orig_u8.is_contiguous():
        raise TypeError("bytes_overlay takes the original as a contiguous uint8 [1 or B, H, W, 3] tensor")
    B = res.shape[0]
    N, H, W, _ = orig_u8.shape
    if tuple(res.shape[1:3]) != (y1 - y0, x1 - x0):
        raise ValueError(f"the result is {res.shape[1]} x {res.shape[2]}, the box {y1 - y0} x {x1 - x0}")
    Bm = 0
    if alpha_u8 is not None:
        Bm, Ha, Wa = _mask_u8(alpha_u8, "bytes_overlay")
        if (Ha, Wa) != (H, W):
            raise ValueError(f"alpha is {Ha} x {Wa}, the original {H} x {W}")
    if out is None:
        out = torch.empty((B, H, W, 3), device=res.device, dtype=torch.uint8)
    if out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 [B, H, W, 3] tensor")
    libfk.check(libfk.load().fk_bytes_overlay_u8(_ptr(res), _ptr(orig_u8), N, _ptr(alpha_u8), Bm, _ptr(out), B, H, W, x0, y0, x1, y1,
                                                 _stream()), "fk_bytes_overlay_u8")
    return out


# ---- optimisation step of the denoiser (include/fk.h; reference train_denoiser.py:935-1181) ------------------------
def _reduce_ws(device):
    return torch.empty(libfk.load().fk_reduce_ws_doubles(), dtype=torch.float64, device=device)


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError(f"{what} must be a contiguous fp32 tensor")


def flow_noisy_tokens(x, noise, sigma, out=None):
    """Packed bf16 tokens of (1 - sigma_b) * x + sigma_b * noise; x, noise fp32 [B,C,h,w], sigma fp32 [B].

    ``out``: a [B, (h/2)(w/2), 4C] bf16 view with contiguous samples (e.g. the target half of the token buffer)."""
    _need_cuda(x, noise, sigma, out)
    _f32c(x, "x"); _f32c(noise, "noise"); _f32c(sigma, "sigma")
    B, C, h, w = x.shape
    if out is None:
        out = torch.empty(B, (h // 2) * (w // 2), 4 * C, device=x.device, dtype=BF16)
    if out.shape != (B, (h // 2) * (w // 2), 4 * C) or out.dtype != BF16 or out.stride(2) != 1 or out.stride(1) != 4 * C:
        raise ValueError("out must be a [B, S, 4C] bf16 view with contiguous samples")
    libfk.check(libfk.load().fk_flow_noisy_tokens_bf16(_ptr(x), _ptr(noise), _ptr(sigma), _ptr(out), out.stride(0), B, C,
                                                       h, w, _stream()), "fk_flow_noisy_tokens_bf16")
    return out


def flow_loss(pred, x, noise, weight=None, want_grad=True, area_mask_weights=None, weight_mask=None):
    """(loss fp64 [1], grad bf16 like pred or None) of the reference's flow-matching loss (train_denoiser.py:1106-1166);
    pred: packed bf16 [B, S, 4C] view with contiguous samples.  weighting = weight[b] * area_mask_weights[b, 0, y, x] *
    weight_mask[b, 0, y, x] (fp32 [B] / [B, 1, h, w], each optional); the sum of weighting * (unpack(pred) - (noise - x))^2 is
    divided by weight_mask.sum() * C when weight_mask is given (:1163-1165), by the element count otherwise (loss.mean())."""
    _need_cuda(pred, x, noise, weight, area_mask_weights, weight_mask)
    _f32c(x, "x"); _f32c(noise, "noise")
    B, C, h, w = x.shape
    if pred.shape != (B, (h // 2) * (w // 2), 4 * C) or pred.dtype != BF16 or pred.stride(2) != 1 or pred.stride(1) != 4 * C:
        raise ValueError("pred must be a [B, S, 4C] bf16 view with contiguous samples")
    if weight is not None:
        _f32c(weight, "weight")
        if weight.numel() != B:
            raise ValueError("weight: one fp32 value per sample")
    for name, m in (("area_mask_weights", area_mask_weights), ("weight_mask", weight_mask)):
        if m is not None:
            _f32c(m, name)
            if tuple(m.shape) != (B, 1, h, w):
                raise ValueError(f"{name} must be [B, 1, h, w] at the latent size (nearest-resize it as train_denoiser.py:1131-1148 does)")
    mask_sum = weight_mask.sum().reshape(1) if weight_mask is not None else None     # device scalar: no host round trip
    grad = torch.empty(pred.shape, device=pred.device, dtype=BF16) if want_grad else None
    loss = torch.empty(1, dtype=torch.float64, device=pred.device)
    libfk.check(libfk.load().fk_flow_loss_weighted_bf16(
        _ptr(pred), pred.stride(0), _ptr(x), _ptr(noise), _ptr(weight), _ptr(area_mask_weights), _ptr(weight_mask), _ptr(mask_sum),
        _ptr(grad), grad.stride(0) if want_grad else 0, _ptr(loss), _ptr(_reduce_ws(pred.device)), B, C, h, w, _stream()),
        "fk_flow_loss_weighted_bf16")
    return loss, grad


def sumsq(tensors, out=None):
    """fp64 [1]: sum of squares over a list of contiguous fp32 / bf16 tensors (the squared global gradient norm)."""
    tensors = [tensors] if isinstance(tensors, torch.Tensor) else list(tensors)
    _need_cuda(*tensors)
    dev = tensors[0].device
    if out is None:
        out = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = _reduce_ws(dev)
    lib = libfk.load()
    for i, t in enumerate(tensors):
        if t.dtype not in (torch.float32, BF16) or not t.is_contiguous():
            raise TypeError("sumsq takes contiguous fp32 / bf16 tensors")
        libfk.check(lib.fk_sumsq(_ptr(t), int(t.dtype == BF16), t.numel(), int(i > 0), _ptr(out), _ptr(ws), _stream()),
                    "fk_sumsq")
    return out


def adamw_step(master, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
               grad_sumsq=None, max_grad_norm=1.0, param_bf16=None, grad_scale=1.0):
    """In-place AdamW update of the fp32 ``master`` (and the bf16 copy); ``grad_sumsq`` (fp64 [1]) enables clipping.
    ``grad_scale``: ``grad`` holds sums that still have to be multiplied by it (1 / world after a reduce-scatter)."""
    _need_cuda(master, grad, exp_avg, exp_avg_sq, grad_sumsq, param_bf16)
    for t, what in ((master, "master"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _f32c(t, what)
    if grad.dtype not in (torch.float32, BF16) or not grad.is_contiguous() or grad.numel() != master.numel():
        raise TypeError("grad must be a contiguous fp32 / bf16 tensor of the parameter's size")
    libfk.check(libfk.load().fk_adamw_step_scaled(_ptr(master), _ptr(param_bf16), _ptr(grad), int(grad.dtype == BF16),
                                                  _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(grad_sumsq), float(max_grad_norm),
                                                  float(grad_scale), float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                  float(weight_decay), int(step), master.numel(), _stream()), "fk_adamw_step")
    if param_bf16 is not None:
        param_tree.note_raw_write()      # a parameter changed behind torch's version counters
    return master


# ---- Prodigy (include/fk.h "Prodigy"; csrc/prodigy.hip): begin, moments per tensor, update_d, apply per tensor ----------
def _as_f32(x):
    return ctypes.c_float(float(x)).value


def prodigy_beta3(betas, beta3=None):
    """beta3 (None: sqrt(beta2)) as the kernels see it.  Betas cross the ABI as fp32 in the streaming kernels, so the scalar kernel is
    given the same fp32 values: the whole step runs with ONE set of numbers."""
    import math
    return _as_f32(math.sqrt(float(betas[1])) if beta3 is None else beta3)


def prodigy_init_state(d0=1e-6, device="cuda"):
    """The fp64 scalar buffer of a fresh optimiser: d = d_max = d0, everything else 0 (slots: ``libfk.FK_PRODIGY_SLOTS``)."""
    if not d0 > 0:
        raise ValueError("prodigy: d0 must be positive")
    buf = torch.zeros(len(libfk.FK_PRODIGY_SLOTS), dtype=torch.float64)
    buf[0] = buf[1] = float(d0)
    return buf.to(device)


def prodigy_ws(device):
    """The fp64 workspace of ``prodigy_moments`` (per-block partials); calls that share one must be ordered on one stream."""
    return torch.empty(libfk.load().fk_prodigy_ws_doubles(), dtype=torch.float64, device=device)


def _prodigy_buf(state):
    if state.dtype != torch.float64 or not state.is_contiguous() or state.numel() < len(libfk.FK_PRODIGY_SLOTS):
        raise TypeError(f"the Prodigy state buffer is a contiguous fp64 tensor of >= {len(libfk.FK_PRODIGY_SLOTS)} elements")


def prodigy_begin(state, lr=1.0, betas=(0.9, 0.99), beta3=None, use_bias_correction=True):
    """Step 1: dlr = d * lr * bias correction (from the device-side step count), numerator decay, running sums zeroed."""
    _need_cuda(state)
    _prodigy_buf(state)
    libfk.check(libfk.load().fk_prodigy_begin(_ptr(state), float(lr), _as_f32(betas[0]), _as_f32(betas[1]), prodigy_beta3(betas, beta3),
                                              int(bool(use_bias_correction)), _stream()), "fk_prodigy_begin")
    return state


def prodigy_moments(master, p0, grad, m, v, s, state, betas=(0.9, 0.99), beta3=None, weight_decay=0.0, d0=1e-6, decouple=True,
                    safeguard_warmup=True, grad_sumsq=None, max_grad_norm=1.0, grad_scale=1.0, ws=None):
    """Step 2 for one tensor / chunk: ``m``, ``v``, ``s`` in place, this tensor's ``sum g (p0 - p)`` and ``sum |s|`` added to the
    running sums of ``state`` (fixed order, no atomics).  ``grad_sumsq`` / ``max_grad_norm`` / ``grad_scale`` as ``adamw_step``."""
    _need_cuda(master, p0, grad, m, v, s, state, grad_sumsq, ws)
    _prodigy_buf(state)
    for t, what in ((master, "master"), (p0, "p0"), (m, "m"), (v, "v"), (s, "s")):
        _f32c(t, what)
        if t.numel() != master.numel():
            raise ValueError(f"{what}: {t.numel()} elements, the parameter has {master.numel()}")
    if grad.dtype not in (torch.float32, BF16) or not grad.is_contiguous() or grad.numel() != master.numel():
        raise TypeError("grad must be a contiguous fp32 / bf16 tensor of the parameter's size")
    lib = libfk.load()
    if ws is None:
        ws = torch.empty(lib.fk_prodigy_ws_doubles(), dtype=torch.float64, device=master.device)
    elif ws.dtype != torch.float64 or ws.numel() < lib.fk_prodigy_ws_doubles():
        raise ValueError("ws: fk_prodigy_ws_doubles() fp64 elements")
    libfk.check(lib.fk_prodigy_moments(_ptr(master), _ptr(p0), _ptr(grad), int(grad.dtype == BF16), _ptr(m), _ptr(v), _ptr(s),
                                       _ptr(state), _ptr(grad_sumsq), float(max_grad_norm), float(grad_scale), float(betas[0]),
                                       float(betas[1]), prodigy_beta3(betas, beta3), float(weight_decay), float(d0),
                                       int(bool(decouple)), int(bool(safeguard_warmup)), master.numel(), _ptr(ws), _stream()),
                "fk_prodigy_moments")
    return state


def prodigy_update_d(state, d0=1e-6, d_coef=1.0, growth_rate=float("inf")):
    """Steps 3 and 4 on the running sums (after an all-reduce: the global ones); sets the skipped flag on a zero denominator."""
    _need_cuda(state)
    _prodigy_buf(state)
    libfk.check(libfk.load().fk_prodigy_update_d(_ptr(state), float(d0), float(d_coef), float(growth_rate), _stream()),
                "fk_prodigy_update_d")
    return state


def prodigy_apply(master, m, v, state, eps=1e-8, weight_decay=0.0, decouple=True, param_bf16=None):
    """Step 5 for one tensor / chunk: the fp32 ``master`` and its bf16 copy together; a no-op when the step was skipped."""
    _need_cuda(master, m, v, state, param_bf16)
    _prodigy_buf(state)
    for t, what in ((master, "master"), (m, "m"), (v, "v")):
        _f32c(t, what)
        if t.numel() != master.numel():
            raise ValueError(f"{what}: {t.numel()} elements, the parameter has {master.numel()}")
    if param_bf16 is not None and (param_bf16.dtype != BF16 or not param_bf16.is_contiguous() or param_bf16.numel() != master.numel()):
        raise TypeError("param_bf16 must be a contiguous bf16 tensor of the parameter's size")
    libfk.check(libfk.load().fk_prodigy_apply(_ptr(master), _ptr(param_bf16), _ptr(m), _ptr(v), _ptr(state), float(eps),
                                              float(weight_decay), int(bool(decouple)), master.numel(), _stream()), "fk_prodigy_apply")
    if param_bf16 is not None:
        param_tree.note_raw_write()      # a parameter changed behind torch's version counters
    return master


def prodigy_state(buf):
    """The scalars of a Prodigy state buffer as a dict of python floats (``d``, ``d_max``, ``d_numerator``, ``d_denom``, ``d_hat``,
    ``dlr``, ``k``, ``skipped``, ``sum_dot``, ``sum_abs``) -- the ONE call of the family that synchronises, for logging ``d * lr``
    as the reference does (train_denoiser.py:1364-1373)."""
    vals = buf.detach().cpu().tolist()
    out = dict(zip(libfk.FK_PRODIGY_SLOTS, vals))
    out["k"], out["skipped"] = int(out["k"]), bool(out["skipped"])
    return out
