// What the denoise-loop step kernels (solver_step.hip: Euler, inpaint, scale_noise, AB2, the float32 state) are made of, each
// piece written once: the 8-element vector forms, the rounded multiply-add, the keep-region value and the two blends -- and the
// elementwise grid, which elementwise.hip shares.  __fmul_rn / __fadd_rn stay a product and a sum only in a file built with
// -ffp-contract=off (Makefile: solver_step.o); the helpers that use them are for that file.
#pragma once
#include "fk_common.h"

inline int ew_grid(int64_t nvec) {
  int64_t g = (nvec + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// float -> bf16 -> float on the host (round-to-nearest-even): a 0-dim fp32 tensor multiplied into a bf16 tensor is cast first
inline float host_round_bf(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// One 16-byte vector of 8 bf16 <-> 8 floats; pack8 is the one rounding to bf16 of a step's result.
FK_DEV void widen8(float* s, u32x4_t w) {
#pragma unroll
  for (int e = 0; e < 4; ++e) s[2 * e] = bf_lo(w[e]), s[2 * e + 1] = bf_hi(w[e]);
}

FK_DEV u32x4_t pack8(const float* s) {
  u32x4_t w;
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = pack_bf2(s[2 * e], s[2 * e + 1]);
  return w;
}

// s += c * w in fp32, the product and the sum rounded once each (no fma: torch restates it op by op)
FK_DEV void axpy8_rn(float* s, float c, u32x4_t w) {
  float t[8];
  widen8(t, w);
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = __fadd_rn(s[j], __fmul_rn(c, t[j]));
}

// keep-region value of a masked edit (FlowMatchEulerDiscreteScheduler.scale_noise on bf16 tensors): the preserved picture
// re-noised to the level the repainted region has after the step.  sb = bf16(sigma), omsb = bf16(1 - sb); shared by the
// inpaint steps and fk_scale_noise_bf16, so the start tokens and the per-step keep values cannot drift apart.
FK_DEV float keep_f(float sb, float omsb, float noise, float x0) {
  return round_bf(round_bf(sb * noise) + round_bf(omsb * x0));
}

// The keep-region operands of a masked step, one kernel argument: x0 / noise rows [B, S_tgt, C] and the compact mask
// [1 or B, S_tgt, 4] at their batch strides (m_bs == 0: one mask for the batch).
struct keep_args {
  const bf16_t* x0;
  int64_t x0_bs;
  const bf16_t* noise;
  int64_t n_bs;
  const bf16_t* mask;
  int64_t m_bs;
};

// Vector i of batch b of the keep-region operands.  One 8-vector spans two channels of one token (C % 8 == 0, cvec = C / 8), and
// element j of a token is sub-pixel j % 4, so the vector's mask pattern is the token's four values twice: one 8-byte load per
// vector, and word e of the vector (elements 2e, 2e + 1) reads mask word e & 1.
FK_DEV void load_keep8(const keep_args& k, int b, int64_t i, int64_t cvec, u32x4_t& zw, u32x4_t& nw, u32x2_t& mw) {
  zw = *(const u32x4_t*)(k.x0 + (int64_t)b * k.x0_bs + i * 8);
  nw = *(const u32x4_t*)(k.noise + (int64_t)b * k.n_bs + i * 8);
  mw = *(const u32x2_t*)(k.mask + (int64_t)b * k.m_bs + (i / cvec) * 4);
}

// The bf16 blend of a masked step (include/fk.h: fk_euler_inpaint_step_bf16), every bf16 tensor op rounded once:
// bf16(bf16(bf16(1 - m) * keep) + bf16(m * bf16(s))), s the step's unrounded fp32 value.  Word by word, as pack_bf2 takes its
// pairs: written element by element over widened operands, ab2_kernel<true, true> needs two more VGPRs.
FK_DEV u32x4_t blend8_bf16(const float* s, const keep_args& k, int b, int64_t i, int64_t cvec, float sb, float omsb) {
  u32x4_t zw, nw, ow;
  u32x2_t mw;
  load_keep8(k, b, i, cvec, zw, nw, mw);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float m0 = bf_lo(mw[e & 1]), m1 = bf_hi(mw[e & 1]);
    const float p0 = round_bf(s[2 * e]), p1 = round_bf(s[2 * e + 1]);
    const float k0 = keep_f(sb, omsb, bf_lo(nw[e]), bf_lo(zw[e]));
    const float k1 = keep_f(sb, omsb, bf_hi(nw[e]), bf_hi(zw[e]));
    ow[e] = pack_bf2(round_bf(round_bf(1.0f - m0) * k0) + round_bf(m0 * p0),
                     round_bf(round_bf(1.0f - m1) * k1) + round_bf(m1 * p1));
  }
  return ow;
}

// The same blend in float32, in place on s (fk_solver_step_f32): the keep value sn * noise + om * x0 and the blend op by op
// in fp32 -- nothing is rounded to bf16 here, so this is not keep_f.
FK_DEV void blend8_f32(float* s, const keep_args& k, int b, int64_t i, int64_t cvec, float sn, float om) {
  u32x4_t zw, nw;
  u32x2_t mw;
  load_keep8(k, b, i, cvec, zw, nw, mw);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float m0 = bf_lo(mw[e & 1]), m1 = bf_hi(mw[e & 1]);
    const float k0 = __fadd_rn(__fmul_rn(sn, bf_lo(nw[e])), __fmul_rn(om, bf_lo(zw[e])));
    const float k1 = __fadd_rn(__fmul_rn(sn, bf_hi(nw[e])), __fmul_rn(om, bf_hi(zw[e])));
    s[2 * e] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, m0), k0), __fmul_rn(m0, s[2 * e]));
    s[2 * e + 1] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, m1), k1), __fmul_rn(m1, s[2 * e + 1]));
  }
}
