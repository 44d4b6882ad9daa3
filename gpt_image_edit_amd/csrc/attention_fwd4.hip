// Attention forward, 4 waves x 64 query rows (one wave per SIMD): its own translation unit so that it can be built with
// -fno-slp-vectorize (v_pk_* forms beside MFMAs cost more than the scalar pairs they replace: +10 % on this kernel) without
// touching the code hipcc generates for the 8-wave kernel of attention_fwd.hip.
#include "attention_common.h"

namespace {

// Build-time switches of the experiments behind DESIGN.md section 4.0's attention table (defaults = what measured best):
#ifndef FK_A4_DMA
#define FK_A4_DMA 2      // a tile's 8 LDS-DMA requests: 0 in front of the first K-fragment reads, 1 behind them (under their
#endif                   // latency), 2 one per MFMA slot of the tile's first group, 3 four in each block's third group, 4 two in the first and third group of each block
#ifndef FK_A4_EARLY
#define FK_A4_EARLY 1    // 1: V^T fragments read one group earlier (behind the MFMA that frees the register), K likewise
#endif
#ifndef FK_A4_EWAIT
#define FK_A4_EWAIT 2    // idle states in front of a block's first softmax step (s_nop operand; the hazard needs 12 states in all)
#endif
#define FK_STR2(x) #x
#define FK_STR(x) FK_STR2(x)
constexpr int A4_STAGES = 3, A4_DMA = FK_A4_DMA;
constexpr bool A4_EARLY = FK_A4_EARLY != 0;

#include "mxfp8_quant.h"

// finalize of the MXFP8 form: one query row's 128 columns of head h leave as 128 e4m3 bytes + 4 E8M0 bytes.  o[df] is the lane's
// share of block df = columns [32 df, 32 df + 32) of the head: 16 values, four runs of 4 at columns 8 g + 4 hh (lane ^ 32 holds
// the other 16).  They are rounded to bf16 exactly as the bf16 form stores them and quantized from those bit patterns, the block's
// amax joined across the two halves: the bytes fk_quantize_mxfp8 gives for the stored bf16 row.  Two half swaps then leave each
// lane with 16 consecutive bytes of the block (hh = 0: bytes 0..15, hh = 1: 16..31); the head's four scale bytes leave as one word.
FK_DEV void store_row_mxfp8(const f32x16_t (&o)[4], float inv, const AttnMxOut& mx, int S, int b, int h, int q_row, int hh) {
#if defined(__HIP_DEVICE_COMPILE__)
  const bool in_a = q_row < mx.split;
  const int64_t row = in_a ? (int64_t)b * mx.split + q_row : (int64_t)b * (S - mx.split) + (q_row - mx.split);
  uint8_t* const qrow = (in_a ? mx.qa : mx.qb) + row * mx.ldq + h * HD + 16 * hh;
  uint8_t* const srow = (in_a ? mx.sa : mx.sb) + row * mx.lds + 4 * h;
  uint32_t scales = 0;
#pragma unroll
  for (int df = 0; df < 4; ++df) {
    uint32_t w[8], amax = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      w[i] = pack_bf2(o[df][2 * i] * inv, o[df][2 * i + 1] * inv);
      amax = max(amax, mx_amax_pair(w[i]));
    }
    const auto am = __builtin_amdgcn_permlane32_swap(amax, amax, false, false);
    const uint32_t sbyte = mx_scale_byte(max(am[0], am[1]));
    uint32_t qw[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) qw[g] = mx_quant4(w[2 * g], w[2 * g + 1], sbyte);
    const auto r0 = __builtin_amdgcn_permlane32_swap(qw[0], qw[2], false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(qw[1], qw[3], false, false);
    const u32x4_t bytes = {r0[0], r0[1], r1[0], r1[1]};
    if (q_row < S) *(u32x4_t*)(qrow + 32 * df) = bytes;
    scales |= sbyte << (8 * df);
  }
  if (hh == 0 && q_row < S) *(uint32_t*)srow = scales;      // rows >= S (the ragged last block) store nothing
#endif
}

#define FK_A4_KERNEL attention_fwd4_kernel
#define FK_A4_PARAMS const AttnParams p
#define FK_A4_MX 0
#include "attention_fwd4_kernel.inc"
#undef FK_A4_KERNEL
#undef FK_A4_PARAMS
#undef FK_A4_MX
// the MXFP8-output form (fk_attention_fwd_ws_mxfp8): kernels of its own, the bf16 ones keep their code and their symbols
#define FK_A4_KERNEL attention_fwd4_mx_kernel
#define FK_A4_PARAMS const AttnParams p, const AttnMxOut mx
#define FK_A4_MX 1
#include "attention_fwd4_kernel.inc"
#undef FK_A4_KERNEL
#undef FK_A4_PARAMS
#undef FK_A4_MX

template <bool STREAMK>
int launch4(const AttnParams& p, int grid, hipStream_t stream) {
  constexpr int SMEM = A4_STAGES * STAGE_BYTES + 16;
  auto kern = attention_fwd4_kernel<STREAMK>;
  FK_ENSURE_MAX_LDS(kern, SMEM, "fk_attention_fwd_bf16 (4 waves x 64 rows)");
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), SMEM, stream, p);
  FK_CHECK_LAUNCH("fk_attention_fwd_bf16 (4 waves x 64 rows)");
  return FK_OK;
}
template <bool STREAMK>
int launch4_mx(const AttnParams& p, const AttnMxOut& mx, int grid, hipStream_t stream) {
  constexpr int SMEM = A4_STAGES * STAGE_BYTES + 16;
  auto kern = attention_fwd4_mx_kernel<STREAMK>;
  FK_ENSURE_MAX_LDS(kern, SMEM, "fk_attention_fwd_ws_mxfp8");
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), SMEM, stream, p, mx);
  FK_CHECK_LAUNCH("fk_attention_fwd_ws_mxfp8");
  return FK_OK;
}
}  // namespace

int fk_attention_fwd4_launch(const AttnParams& p, int grid, bool streamk, hipStream_t stream) {
  return streamk ? launch4<true>(p, grid, stream) : launch4<false>(p, grid, stream);
}
int fk_attention_fwd4_mx_launch(const AttnParams& p, const AttnMxOut& mx, int grid, bool streamk, hipStream_t stream) {
  return streamk ? launch4_mx<true>(p, mx, grid, stream) : launch4_mx<false>(p, mx, grid, stream);
}
