// OCP MXFP8 quantizer arithmetic (e4m3fn elements, one E8M0 scale per 32 consecutive elements), shared by the standalone
// quantizer (gemm_mxfp8.hip: quantize_mxfp8_kernel) and by the producers that emit quantized activations directly (the
// LN + modulate kernels of norm_kernels.hip, the quantized-output epilogue of gemm_epilogue.h).  Every caller starts from
// bf16 bit patterns, so the three give the same bytes for the same bf16 values.  Included INSIDE the anonymous namespace of
// each kernel file, like gemm_epilogue.h.
#pragma once

// |v| < 512 (v = x / 2^e with e >= floor(log2 amax) - 8) -> e4m3fn magnitude code, round-to-nearest-even, saturated to 448
FK_DEV uint32_t e4m3_mag(float a) {
  a = fminf(a, 448.0f);
  if (a < 0.015625f) return (uint32_t)__builtin_rintf(a * 512.0f);   // subnormal: k * 2^-9, k = 0..8 (8 = the smallest normal)
  uint32_t u = __float_as_uint(a);
  u += 0x7ffffu + ((u >> 20) & 1u);      // round the fp32 mantissa to 3 bits (a carry moves into the exponent)
  return (u >> 20) - (120u << 3);        // (biased exp - 127 + 7) << 3 | mantissa
}

// larger magnitude of a word's two bf16 halves, as bf16 magnitude bits: they order like the values, Inf = 0x7f80, NaN above
FK_DEV uint32_t mx_amax_pair(uint32_t w) { return max(w & 0x7fffu, (w >> 16) & 0x7fffu); }

// E8M0 byte of a block from its amax bits: e = max(floor(log2 amax) - 8, -127), byte = e + 127 (bf16 exponent field E:
// floor(log2) = E - 127; subnormal: clamped); an all-zero block 127; a block holding Inf / NaN 0xff
FK_DEV uint32_t mx_scale_byte(uint32_t amax) {
  if (amax >= 0x7f80u) return 0xffu;
  const int E = (int)(amax >> 7);
  return amax == 0 ? 127u : (uint32_t)max(E - 8, 0);
}

// two words of bf16 pairs (elements 0-3 of a block in memory order) -> their four e4m3 bytes; a NaN block (sbyte 0xff): NaN
FK_DEV uint32_t mx_quant4(uint32_t w0, uint32_t w1, uint32_t sbyte) {
  if (sbyte == 0xffu) return 0x7f7f7f7fu;
  const float inv = __uint_as_float((254u - sbyte) << 23);   // 2^-e, exact (254 - byte in [8, 254] for finite blocks)
  uint32_t o = 0;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const uint32_t w = (h >> 1) ? w1 : w0;
    const uint32_t b = (h & 1) ? (w >> 16) : (w & 0xffffu);
    const float v = __uint_as_float((b & 0x7fffu) << 16) * inv;
    o |= (e4m3_mag(v) | ((b >> 8) & 0x80u)) << (8 * h);
  }
  return o;
}

// a whole block held by one thread: 16 words of bf16 pairs -> 8 words of e4m3 bytes; returns the scale byte
FK_DEV uint32_t mx_quant_block(const uint32_t (&w)[16], uint32_t (&out)[8]) {
  uint32_t amax = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) amax = max(amax, mx_amax_pair(w[i]));
  const uint32_t sbyte = mx_scale_byte(amax);
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = mx_quant4(w[2 * i], w[2 * i + 1], sbyte);
  return sbyte;
}
