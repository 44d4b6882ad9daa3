// The two per-pixel values at the pipeline's uint8 boundary, each written once: vae_kernels.hip (whole pictures, nearest resize)
// and mask_ops.hip (a source box, bilinear weights) share them, so a box that is the whole picture at equal size gives the
// whole-picture kernels' bits.  Each operation is rounded once with and without -ffp-contract: 2v is exact, so the one product
// that feeds a sum cannot change under contraction.
#pragma once
#include "fk_common.h"

// byte value u (fp32, 0..255) -> [-1, 1]: ((u / 255) - 0.5) / 0.5 (reference cli.py:106-109), optionally 2v - 1 once more
// (VaeImageProcessor.preprocess normalises whenever the tensor has no negative value)
FK_DEV float pixel_norm(float u, int renorm) {
  float v = __fdiv_rn(__fsub_rn(__fdiv_rn(u, 255.0f), 0.5f), 0.5f);
  if (renorm) v = __fsub_rn(__fmul_rn(2.0f, v), 1.0f);
  return v;
}

// decoder output x (bf16 / fp32, in [-1, 1]) -> t = clamp(x / 2 + 0.5, 0, 1) in the tensor's dtype (VaeImageProcessor.postprocess)
template <typename T>
FK_DEV float image_unit(T x) {
  float t;
  if constexpr (sizeof(T) == 4) t = __fadd_rn(__fdiv_rn(x, 2.0f), 0.5f);
  else t = round_bf(round_bf(bf2f(x) * 0.5f) + 0.5f);
  return fminf(fmaxf(t, 0.f), 1.f);
}
