// What the denoise-loop step kernels share (elementwise.hip: Euler, inpaint, scale_noise; solver_step.hip: AB2): the keep-region
// value, the host's bf16 rounding of a scalar and the elementwise grid.  One definition each, so the kernels cannot drift apart.
#pragma once
#include "fk_common.h"

// keep-region value of a masked edit (FlowMatchEulerDiscreteScheduler.scale_noise on bf16 tensors): the preserved picture
// re-noised to the level the repainted region has after the step.  sb = bf16(sigma), omsb = bf16(1 - sb); shared by the
// inpaint steps and fk_scale_noise_bf16, so the start tokens and the per-step keep values cannot drift apart.
FK_DEV float keep_f(float sb, float omsb, float noise, float x0) {
  return round_bf(round_bf(sb * noise) + round_bf(omsb * x0));
}

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
