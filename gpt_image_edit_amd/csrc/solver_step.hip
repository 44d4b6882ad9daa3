// Second-order multistep (Adams-Bashforth 2) update of the denoise loop on a non-uniform sigma grid (scheduler.py:
// FlowMatchMultistepScheduler), one HBM-bound pass over the target rows of the token buffer:
//   s = x + c_v * v  [+ c_h * h]      fp32, each product and each sum rounded once (no fma: torch restates it op by op)
//   p = bf16(s)                        the one rounding of the update
//   hist <- v                          the same pass: the next step's history
// and, with a mask, the keep-region blend of euler_inpaint_kernel with this p in the place of the Euler value.
// The coefficients stay fp32: rounded to bf16 (2^-8 relative) the rule would no longer be second order.
#include "fk_common.h"
#include "step_common.h"

namespace {

// One 8-vector spans two channels of one token (C % 8 == 0), and element j of a token is sub-pixel j % 4, so the vector's
// mask pattern is the token's four values twice: one 8-byte load per vector (as in euler_inpaint_kernel).
template <bool HIST, bool MASK>
__global__ __launch_bounds__(256) void ab2_kernel(bf16_t* x, int64_t x_bs, const bf16_t* v, int64_t v_bs, bf16_t* hist,
                                                  int64_t h_bs, const bf16_t* x0, int64_t x0_bs, const bf16_t* noise,
                                                  int64_t n_bs, const bf16_t* mask, int64_t m_bs, int S_tgt, int C, float c_v,
                                                  float c_h, float sb, float omsb) {
  const int b = blockIdx.y;
  const int64_t cvec = C / 8, nvec = (int64_t)S_tgt * cvec;
  bf16_t* xb = x + (int64_t)b * x_bs;
  const bf16_t* vb = v + (int64_t)b * v_bs;
  bf16_t* hb = hist + (int64_t)b * h_bs;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const u32x4_t xw = *(const u32x4_t*)(xb + i * 8), vw = *(const u32x4_t*)(vb + i * 8);
    float s[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[2 * e] = __fadd_rn(bf_lo(xw[e]), __fmul_rn(c_v, bf_lo(vw[e])));
      s[2 * e + 1] = __fadd_rn(bf_hi(xw[e]), __fmul_rn(c_v, bf_hi(vw[e])));
    }
    if (HIST) {   // this thread's h is read here, before the store below replaces it
      const u32x4_t hw = *(const u32x4_t*)(hb + i * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[2 * e] = __fadd_rn(s[2 * e], __fmul_rn(c_h, bf_lo(hw[e])));
        s[2 * e + 1] = __fadd_rn(s[2 * e + 1], __fmul_rn(c_h, bf_hi(hw[e])));
      }
    }
    *(u32x4_t*)(hb + i * 8) = vw;
    u32x4_t ow;
    if (MASK) {
      const u32x4_t zw = *(const u32x4_t*)(x0 + (int64_t)b * x0_bs + i * 8);
      const u32x4_t nw = *(const u32x4_t*)(noise + (int64_t)b * n_bs + i * 8);
      const u32x2_t mw = *(const u32x2_t*)(mask + (int64_t)b * m_bs + (i / cvec) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m0 = bf_lo(mw[e & 1]), m1 = bf_hi(mw[e & 1]);
        const float p0 = round_bf(s[2 * e]), p1 = round_bf(s[2 * e + 1]);
        const float k0 = keep_f(sb, omsb, bf_lo(nw[e]), bf_lo(zw[e]));
        const float k1 = keep_f(sb, omsb, bf_hi(nw[e]), bf_hi(zw[e]));
        ow[e] = pack_bf2(round_bf(round_bf(1.0f - m0) * k0) + round_bf(m0 * p0),
                         round_bf(round_bf(1.0f - m1) * k1) + round_bf(m1 * p1));
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) ow[e] = pack_bf2(s[2 * e], s[2 * e + 1]);
    }
    *(u32x4_t*)(xb + i * 8) = ow;
  }
}

// The same rule on a float32 state (fk_solver_step_f32): the sum is kept unrounded in `state` from step to step and the token
// rows receive its one rounding to bf16, the model's next input.  The keep-region value and the blend are float32 too -- no
// keep_f here: that is the bf16 formula of the bf16 kernels.  The vector layout is ab2_kernel's; the state is two 16-byte
// accesses per vector.  load_state == 0 (the first executed step) widens the bf16 token rows instead and never reads `state`;
// hist == nullptr (Euler) stores no history.
template <bool HIST, bool MASK>
__global__ __launch_bounds__(256) void state_kernel(float* state, int64_t s_bs, bf16_t* x, int64_t x_bs, const bf16_t* v,
                                                    int64_t v_bs, bf16_t* hist, int64_t h_bs, const bf16_t* x0, int64_t x0_bs,
                                                    const bf16_t* noise, int64_t n_bs, const bf16_t* mask, int64_t m_bs,
                                                    int S_tgt, int C, float c_v, float c_h, int load_state, float sn, float om) {
  const int b = blockIdx.y;
  const int64_t cvec = C / 8, nvec = (int64_t)S_tgt * cvec;
  float* sb = state + (int64_t)b * s_bs;
  bf16_t* xb = x + (int64_t)b * x_bs;
  const bf16_t* vb = v + (int64_t)b * v_bs;
  bf16_t* hb = hist ? hist + (int64_t)b * h_bs : nullptr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    const u32x4_t vw = *(const u32x4_t*)(vb + i * 8);
    float s[8];
    if (load_state) {
      const f32x4_t lo = *(const f32x4_t*)(sb + i * 8), hi = *(const f32x4_t*)(sb + i * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[e] = lo[e], s[4 + e] = hi[e];
    } else {
      const u32x4_t xw = *(const u32x4_t*)(xb + i * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[2 * e] = bf_lo(xw[e]), s[2 * e + 1] = bf_hi(xw[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[2 * e] = __fadd_rn(s[2 * e], __fmul_rn(c_v, bf_lo(vw[e])));
      s[2 * e + 1] = __fadd_rn(s[2 * e + 1], __fmul_rn(c_v, bf_hi(vw[e])));
    }
    if (HIST) {   // this thread's h is read here, before the store below replaces it
      const u32x4_t hw = *(const u32x4_t*)(hb + i * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[2 * e] = __fadd_rn(s[2 * e], __fmul_rn(c_h, bf_lo(hw[e])));
        s[2 * e + 1] = __fadd_rn(s[2 * e + 1], __fmul_rn(c_h, bf_hi(hw[e])));
      }
    }
    if (hb) *(u32x4_t*)(hb + i * 8) = vw;
    if (MASK) {
      const u32x4_t zw = *(const u32x4_t*)(x0 + (int64_t)b * x0_bs + i * 8);
      const u32x4_t nw = *(const u32x4_t*)(noise + (int64_t)b * n_bs + i * 8);
      const u32x2_t mw = *(const u32x2_t*)(mask + (int64_t)b * m_bs + (i / cvec) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m0 = bf_lo(mw[e & 1]), m1 = bf_hi(mw[e & 1]);
        const float k0 = __fadd_rn(__fmul_rn(sn, bf_lo(nw[e])), __fmul_rn(om, bf_lo(zw[e])));
        const float k1 = __fadd_rn(__fmul_rn(sn, bf_hi(nw[e])), __fmul_rn(om, bf_hi(zw[e])));
        s[2 * e] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, m0), k0), __fmul_rn(m0, s[2 * e]));
        s[2 * e + 1] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, m1), k1), __fmul_rn(m1, s[2 * e + 1]));
      }
    }
    *(f32x4_t*)(sb + i * 8) = f32x4_t{s[0], s[1], s[2], s[3]};
    *(f32x4_t*)(sb + i * 8 + 4) = f32x4_t{s[4], s[5], s[6], s[7]};
    u32x4_t ow;
#pragma unroll
    for (int e = 0; e < 4; ++e) ow[e] = pack_bf2(s[2 * e], s[2 * e + 1]);
    *(u32x4_t*)(xb + i * 8) = ow;
  }
}

}  // namespace

extern "C" int fk_solver_step_f32(float* state, int64_t state_batch_stride, void* x, int64_t x_batch_stride, const void* v,
                                  int64_t v_batch_stride, void* hist, int64_t hist_batch_stride, const void* x0,
                                  int64_t x0_batch_stride, const void* noise, int64_t noise_batch_stride, const void* mask,
                                  int64_t mask_batch_stride, int32_t B, int32_t S_tgt, int32_t C, float c_v, float c_h,
                                  int32_t use_hist, int32_t load_state, float sigma_next, fk_stream_t stream) {
  FK_CHECK_ARG(state && x && v && B > 0 && S_tgt > 0 && C > 0 && C % 8 == 0, "fk_solver_step_f32: bad sizes");
  FK_CHECK_ARG(use_hist == 0 || use_hist == 1, "fk_solver_step_f32: use_hist=%d is neither 0 nor 1", (int)use_hist);
  FK_CHECK_ARG(load_state == 0 || load_state == 1, "fk_solver_step_f32: load_state=%d is neither 0 nor 1", (int)load_state);
  FK_CHECK_ARG(hist || !use_hist, "fk_solver_step_f32: use_hist=1 needs a history buffer");
  FK_CHECK_ARG(!hist || (hist != v && hist != x && hist != (void*)state),
               "fk_solver_step_f32: hist must be a buffer of its own (it is written while v, x and state are read)");
  FK_CHECK_ARG((void*)state != x, "fk_solver_step_f32: state must be a buffer of its own (x receives its bf16 rounding)");
  FK_CHECK_ARG(x_batch_stride % 8 == 0 && v_batch_stride % 8 == 0 && (!hist || hist_batch_stride % 8 == 0) &&
                   ((uintptr_t)x % 16 == 0) && ((uintptr_t)v % 16 == 0) && ((uintptr_t)hist % 16 == 0),
               "fk_solver_step_f32: alignment");
  FK_CHECK_ARG(state_batch_stride % 4 == 0 && ((uintptr_t)state % 16 == 0), "fk_solver_step_f32: alignment of the state");
  float om = 0.0f;
  if (mask) {
    FK_CHECK_ARG(x0 && noise, "fk_solver_step_f32: a mask needs x0 and noise");
    FK_CHECK_ARG(x0_batch_stride % 8 == 0 && noise_batch_stride % 8 == 0 && ((uintptr_t)x0 % 16 == 0) &&
                     ((uintptr_t)noise % 16 == 0), "fk_solver_step_f32: alignment of x0 / noise");
    FK_CHECK_ARG(mask_batch_stride % 4 == 0 && ((uintptr_t)mask % 8 == 0), "fk_solver_step_f32: alignment of the mask");
    om = 1.0f - sigma_next;   // float32(1 - sigma_next), formed once: sigma_next itself is not rounded to bf16 here
  }
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  const dim3 grid(ew_grid(nvec), B), block(256);
  hipStream_t s = (hipStream_t)stream;
#define FK_STATE_LAUNCH(HIST, MASK)                                                                                      \
  hipLaunchKernelGGL((state_kernel<HIST, MASK>), grid, block, 0, s, state, state_batch_stride, (bf16_t*)x, x_batch_stride, \
                     (const bf16_t*)v, v_batch_stride, (bf16_t*)hist, hist_batch_stride, (const bf16_t*)x0, x0_batch_stride, \
                     (const bf16_t*)noise, noise_batch_stride, (const bf16_t*)mask, mask_batch_stride, S_tgt, C, c_v, c_h,  \
                     (int)load_state, sigma_next, om)
  if (use_hist && mask) FK_STATE_LAUNCH(true, true);
  else if (use_hist) FK_STATE_LAUNCH(true, false);
  else if (mask) FK_STATE_LAUNCH(false, true);
  else FK_STATE_LAUNCH(false, false);
#undef FK_STATE_LAUNCH
  FK_CHECK_LAUNCH("fk_solver_step_f32");
  return FK_OK;
}

extern "C" int fk_ab2_step_bf16(void* x, int64_t x_batch_stride, const void* v, int64_t v_batch_stride, void* hist,
                                int64_t hist_batch_stride, const void* x0, int64_t x0_batch_stride, const void* noise,
                                int64_t noise_batch_stride, const void* mask, int64_t mask_batch_stride, int32_t B,
                                int32_t S_tgt, int32_t C, float c_v, float c_h, int32_t use_hist, float sigma_next,
                                fk_stream_t stream) {
  FK_CHECK_ARG(x && v && hist && B > 0 && S_tgt > 0 && C > 0 && C % 8 == 0, "fk_ab2_step_bf16: bad sizes");
  FK_CHECK_ARG(hist != v && hist != x, "fk_ab2_step_bf16: hist must be a buffer of its own (it is written while v and x are read)");
  FK_CHECK_ARG(use_hist == 0 || use_hist == 1, "fk_ab2_step_bf16: use_hist=%d is neither 0 nor 1", (int)use_hist);
  FK_CHECK_ARG(x_batch_stride % 8 == 0 && v_batch_stride % 8 == 0 && hist_batch_stride % 8 == 0 &&
                   ((uintptr_t)x % 16 == 0) && ((uintptr_t)v % 16 == 0) && ((uintptr_t)hist % 16 == 0),
               "fk_ab2_step_bf16: alignment");
  float sb = 0.0f, omsb = 0.0f;
  if (mask) {
    FK_CHECK_ARG(x0 && noise, "fk_ab2_step_bf16: a mask needs x0 and noise");
    FK_CHECK_ARG(x0_batch_stride % 8 == 0 && noise_batch_stride % 8 == 0 && ((uintptr_t)x0 % 16 == 0) &&
                     ((uintptr_t)noise % 16 == 0), "fk_ab2_step_bf16: alignment of x0 / noise");
    FK_CHECK_ARG(mask_batch_stride % 4 == 0 && ((uintptr_t)mask % 8 == 0), "fk_ab2_step_bf16: alignment of the mask");
    sb = host_round_bf(sigma_next);
    omsb = host_round_bf(1.0f - sb);
  }
  const int64_t nvec = (int64_t)S_tgt * C / 8;
  const dim3 grid(ew_grid(nvec), B), block(256);
  hipStream_t s = (hipStream_t)stream;
#define FK_AB2_LAUNCH(HIST, MASK)                                                                                        \
  hipLaunchKernelGGL((ab2_kernel<HIST, MASK>), grid, block, 0, s, (bf16_t*)x, x_batch_stride, (const bf16_t*)v,           \
                     v_batch_stride, (bf16_t*)hist, hist_batch_stride, (const bf16_t*)x0, x0_batch_stride,                \
                     (const bf16_t*)noise, noise_batch_stride, (const bf16_t*)mask, mask_batch_stride, S_tgt, C, c_v, c_h, \
                     sb, omsb)
  if (use_hist && mask) FK_AB2_LAUNCH(true, true);
  else if (use_hist) FK_AB2_LAUNCH(true, false);
  else if (mask) FK_AB2_LAUNCH(false, true);
  else FK_AB2_LAUNCH(false, false);
#undef FK_AB2_LAUNCH
  FK_CHECK_LAUNCH("fk_ab2_step_bf16");
  return FK_OK;
}
